// The two halves of a swept sample (include/minkhip.h "THE RULE OF THE SWEEP"): b ⊖ a of an edge, formed once, and q(u) = a ⊕ u·(b ⊖ a),
// built in LDS for every sample — shared by sweep_kernel (sweep.hip) and lr_check_kernel (ladder_refine_free.hip), so that a
// sample of either is the same row of q, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "lie_dev.h"
#include "mkh_types.h"
#include "wide_types.h"

namespace mkh {

// a and b ⊖ a of one edge into sA / sD, joint by joint on the group's lanes.  A quaternion: sA = normalize(q_a), sD = axis (3) |
// angle of mju_subQuat(q_b, q_a).
template <int LPR>
__device__ __forceinline__ void swp_difference(const WideProblem& P, const double* __restrict__ a, const double* __restrict__ c,
                                               double* const sA, double* const sD, int sub) {
#pragma clang fp contract(off)      // b − a: one rounded difference, as the numpy restatement forms it
  for (int j = sub; j < P.njnt; j += LPR) {
    const int jt = P.jnt_type[j];
    int qa = P.jnt_qadr[j];
    if (jt == JNT_SLIDE || jt == JNT_HINGE) {
      sA[qa] = a[qa];
      sD[qa] = c[qa] - a[qa];
      continue;
    }
    if (jt == JNT_FREE) {
      for (int n = 0; n < 3; ++n) {
        sA[qa + n] = a[qa + n];
        sD[qa + n] = c[qa + n] - a[qa + n];
      }
      qa += 3;
    }
    const Q4 q{a[qa], a[qa + 1], a[qa + 2], a[qa + 3]};
    const V3 w = quat2vel(qmul(qconj(q), Q4{c[qa], c[qa + 1], c[qa + 2], c[qa + 3]}));
    const double nrm = sqrt(w.x * w.x + w.y * w.y + w.z * w.z);
    V3 ax{1.0, 0.0, 0.0};
    if (nrm >= 1e-15) ax = V3{w.x / nrm, w.y / nrm, w.z / nrm};
    const Q4 qn = qnormalize(q);
    sA[qa] = qn.w; sA[qa + 1] = qn.x; sA[qa + 2] = qn.y; sA[qa + 3] = qn.z;
    sD[qa] = ax.x; sD[qa + 1] = ax.y; sD[qa + 2] = ax.z; sD[qa + 3] = nrm;
  }
}

// q(u) = a ⊕ u·(b ⊖ a) into sQ: scalars a + u·(b − a); quaternions mju_quatIntegrate on the shortest arc.
template <int LPR>
__device__ __forceinline__ void swp_blend(const WideProblem& P, const double* const sA, const double* const sD, double u,
                                          double* const sQ, int sub) {
#pragma clang fp contract(off)      // a + u·d: a product and a sum
  for (int j = sub; j < P.njnt; j += LPR) {
    const int jt = P.jnt_type[j];
    int qa = P.jnt_qadr[j];
    if (jt == JNT_SLIDE || jt == JNT_HINGE) {
      sQ[qa] = sA[qa] + u * sD[qa];
      continue;
    }
    if (jt == JNT_FREE) {
      for (int n = 0; n < 3; ++n) sQ[qa + n] = sA[qa + n] + u * sD[qa + n];
      qa += 3;
    }
    const Q4 q = qnormalize(qmul(Q4{sA[qa], sA[qa + 1], sA[qa + 2], sA[qa + 3]},
                                 axis_angle(V3{sD[qa], sD[qa + 1], sD[qa + 2]}, u * sD[qa + 3])));
    sQ[qa] = q.w; sQ[qa + 1] = q.x; sQ[qa + 2] = q.y; sQ[qa + 3] = q.z;
  }
}

}  // namespace mkh
