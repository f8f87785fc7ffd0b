// The tangent-space distance of multi-start's selection rules (include/minkhip.h): shared by multistart.hip, which ranks the
// final configurations of a target's seeds with it, and trajectory_multistart.hip, which sums it along a candidate path.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"

namespace mkh {

enum : int32_t { MS_JNT_FREE = 0, MS_JNT_BALL = 1 };       // mjtJoint (2 / 3: slide / hinge)

// d = Σ_k w_k·(q ⊖ r)_k², ⊖ = mj_differentiatePos at dt = 1
__device__ __forceinline__ double ms_distance(const int32_t* __restrict__ jnt, int njnt, const double* __restrict__ q,
                                              const double* __restrict__ r, const double* __restrict__ w) {
  double d = 0.0;
  for (int j = 0; j < njnt; ++j) {
    const int jt = jnt[3 * j];
    int qa = jnt[3 * j + 1], va = jnt[3 * j + 2];
    if (jt != MS_JNT_FREE && jt != MS_JNT_BALL) {
      const double dv = q[qa] - r[qa];
      d += (w ? w[va] : 1.0) * dv * dv;
      continue;
    }
    if (jt == MS_JNT_FREE) {
      for (int k = 0; k < 3; ++k) {
        const double dv = q[qa + k] - r[qa + k];
        d += (w ? w[va + k] : 1.0) * dv * dv;
      }
      qa += 3; va += 3;
    }
    // mju_subQuat: rotation vector of conj(r)·q
    const V3 dw = quat2vel(qmul(qconj(Q4{r[qa], r[qa + 1], r[qa + 2], r[qa + 3]}), Q4{q[qa], q[qa + 1], q[qa + 2], q[qa + 3]}));
    d += (w ? w[va] : 1.0) * dw.x * dw.x + (w ? w[va + 1] : 1.0) * dw.y * dw.y + (w ? w[va + 2] : 1.0) * dw.z * dw.z;
  }
  return d;
}

}  // namespace mkh
