// The two halves of a swept sample (include/minkhip.h "THE RULE OF THE SWEEP"): b ⊖ a of an edge, formed once, and q(u) = a ⊕ u·(b ⊖ a),
// built in LDS for every sample — shared by sweep_kernel (sweep.hip) and lr_check_kernel (ladder_refine_free.hip), so that a
// sample of either is the same row of q, bit for bit.  The arithmetic of ONE joint sits in the swp_scalar_* / swp_quat_*
// functions below: the row forms call them joint by joint on the group's lanes, and convex_sweep_kernel (convex_sweep.hip) calls
// them per lane for the joints of a kinematic chain, so that the general convex pairs and the analytic pairs of a sample see one
// row of q.
#pragma once
#include <hip/hip_runtime.h>

#include "lie_dev.h"
#include "mkh_types.h"
#include "wide_types.h"

namespace mkh {

// ---- one joint
__device__ __forceinline__ double swp_scalar_difference(double a, double c) {
#pragma clang fp contract(off)      // b − a: one rounded difference, as the numpy restatement forms it
  return c - a;
}

__device__ __forceinline__ double swp_scalar_blend(double a, double d, double u) {
#pragma clang fp contract(off)      // a + u·d: a product and a sum
  return a + u * d;
}

// qn = normalize(q_a), ax | nrm = the axis and the angle of mju_subQuat(q_b, q_a)
__device__ __forceinline__ void swp_quat_difference(Q4 q, Q4 c, Q4& qn, V3& ax, double& nrm) {
#pragma clang fp contract(off)
  const V3 w = quat2vel(qmul(qconj(q), c));
  nrm = sqrt(w.x * w.x + w.y * w.y + w.z * w.z);
  ax = V3{1.0, 0.0, 0.0};
  if (nrm >= 1e-15) ax = V3{w.x / nrm, w.y / nrm, w.z / nrm};
  qn = qnormalize(q);
}

// mju_quatIntegrate on the shortest arc
__device__ __forceinline__ Q4 swp_quat_blend(Q4 qn, V3 ax, double nrm, double u) {
#pragma clang fp contract(off)
  return qnormalize(qmul(qn, axis_angle(ax, u * nrm)));
}

// ---- one row
// a and b ⊖ a of one edge into sA / sD, joint by joint on the group's lanes.  A quaternion: sA = normalize(q_a), sD = axis (3) |
// angle of mju_subQuat(q_b, q_a).
template <int LPR>
__device__ __forceinline__ void swp_difference(const WideProblem& P, const double* __restrict__ a, const double* __restrict__ c,
                                               double* const sA, double* const sD, int sub) {
  for (int j = sub; j < P.njnt; j += LPR) {
    const int jt = P.jnt_type[j];
    int qa = P.jnt_qadr[j];
    if (jt == JNT_SLIDE || jt == JNT_HINGE) {
      sA[qa] = a[qa];
      sD[qa] = swp_scalar_difference(a[qa], c[qa]);
      continue;
    }
    if (jt == JNT_FREE) {
      for (int n = 0; n < 3; ++n) {
        sA[qa + n] = a[qa + n];
        sD[qa + n] = swp_scalar_difference(a[qa + n], c[qa + n]);
      }
      qa += 3;
    }
    Q4 qn; V3 ax; double nrm;
    swp_quat_difference(Q4{a[qa], a[qa + 1], a[qa + 2], a[qa + 3]}, Q4{c[qa], c[qa + 1], c[qa + 2], c[qa + 3]}, qn, ax, nrm);
    sA[qa] = qn.w; sA[qa + 1] = qn.x; sA[qa + 2] = qn.y; sA[qa + 3] = qn.z;
    sD[qa] = ax.x; sD[qa + 1] = ax.y; sD[qa + 2] = ax.z; sD[qa + 3] = nrm;
  }
}

// q(u) = a ⊕ u·(b ⊖ a) into sQ: scalars a + u·(b − a); quaternions mju_quatIntegrate on the shortest arc.
template <int LPR>
__device__ __forceinline__ void swp_blend(const WideProblem& P, const double* const sA, const double* const sD, double u,
                                          double* const sQ, int sub) {
  for (int j = sub; j < P.njnt; j += LPR) {
    const int jt = P.jnt_type[j];
    int qa = P.jnt_qadr[j];
    if (jt == JNT_SLIDE || jt == JNT_HINGE) {
      sQ[qa] = swp_scalar_blend(sA[qa], sD[qa], u);
      continue;
    }
    if (jt == JNT_FREE) {
      for (int n = 0; n < 3; ++n) sQ[qa + n] = swp_scalar_blend(sA[qa + n], sD[qa + n], u);
      qa += 3;
    }
    const Q4 q = swp_quat_blend(Q4{sA[qa], sA[qa + 1], sA[qa + 2], sA[qa + 3]}, V3{sD[qa], sD[qa + 1], sD[qa + 2]}, sD[qa + 3], u);
    sQ[qa] = q.w; sQ[qa + 1] = q.x; sQ[qa + 2] = q.y; sQ[qa + 3] = q.z;
  }
}

}  // namespace mkh
