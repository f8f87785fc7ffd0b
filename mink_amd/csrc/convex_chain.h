// The kinematic chains of a checker's general convex pairs and the walk down one of them — shared by convex_contacts_kernel
// (convex_pre.hip: rows of q in memory) and convex_sweep_kernel (convex_sweep.hip: rows of q blended between the two ends of an
// edge, joint by joint, as the walk asks for them).  CvPre, the lists themselves, is defined here once: the handle keeps one
// (host_internal.h) and the three pre-pass launchers take it (launch_convex_pre below; launch_convex_sweep and
// launch_convex_check in outer_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include "mkh_types.h"
#include "lie_dev.h"
#include "wide_types.h"

namespace mkh {

struct CvPre {
  int32_t n_cv;
  const int32_t* pair;       // [n_cv] index into WideProblem::pairs
  const int32_t* chain_adr;  // [2·n_cv + 1]: bodies root → body1 of convex pair k at [chain_adr[2k], chain_adr[2k+1]), → body2 behind
  const int32_t* chain;      // body ids
};

// convex_pre.hip: (dist, from, to) of every (row, general convex pair) of B rows of q, (B, n_cv, 7) into `out`
hipError_t launch_convex_pre(hipStream_t stream, const WideProblem* P, const CvPre& C, int B, const double* q, double* out);

// A row of q in memory, as the walk reads it: a scalar joint's coordinate, a free joint's position, a quaternion.
struct CvRowMem {
  const double* q;
  __device__ __forceinline__ double scalar(int qa) const { return q[qa]; }
  __device__ __forceinline__ V3 pos(int qa) const { return V3{q[qa], q[qa + 1], q[qa + 2]}; }
  __device__ __forceinline__ Q4 quat(int qa) const { return Q4{q[qa], q[qa + 1], q[qa + 2], q[qa + 3]}; }
};

// pose of the last body of a chain (root first) at the row `qrow`: mj_kinematics along one branch (the arithmetic of
// wide_kernel.h's FK)
template <class Row>
__device__ __forceinline__ void cv_chain_pose(const WideProblem& P, const Row& qrow, const int32_t* ch, int len, V3& xp, Q4& xq) {
  xp = V3{0, 0, 0};
  xq = Q4{1, 0, 0, 0};
  for (int c = 0; c < len; ++c) {
    const int b = ch[c];
    xp = xp + qrot(xq, V3{P.body_pos[3 * b], P.body_pos[3 * b + 1], P.body_pos[3 * b + 2]});
    xq = qmul(xq, Q4{P.body_quat[4 * b], P.body_quat[4 * b + 1], P.body_quat[4 * b + 2], P.body_quat[4 * b + 3]});
    const int jadr = P.body_jntadr[b], jnum = P.body_jntnum[b];
    for (int jn = 0; jn < jnum; ++jn) {
      const int j = jadr + jn, jt = P.jnt_type[j], qa = P.jnt_qadr[j];
      const V3 axl{P.jnt_axis[3 * j], P.jnt_axis[3 * j + 1], P.jnt_axis[3 * j + 2]};
      const V3 jp{P.jnt_pos[3 * j], P.jnt_pos[3 * j + 1], P.jnt_pos[3 * j + 2]};
      if (jt == JNT_FREE) {
        xp = qrow.pos(qa);
        xq = qnormalize(qrow.quat(qa + 3));
      }
      const V3 ax = qrot(xq, axl), an = xp + qrot(xq, jp);
      if (jt == JNT_SLIDE) {
        xp = xp + (qrow.scalar(qa) - P.jnt_qpos0[j]) * ax;
      } else if (jt == JNT_HINGE || jt == JNT_BALL) {
        const Q4 qloc = (jt == JNT_HINGE) ? axis_angle(axl, qrow.scalar(qa) - P.jnt_qpos0[j]) : qnormalize(qrow.quat(qa));
        xq = qmul(xq, qloc);
        xp = an - qrot(xq, jp);
      }
    }
    xq = qnormalize(xq);
  }
}

}  // namespace mkh
