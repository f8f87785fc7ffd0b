// The tangent-space distance of multi-start's selection rules (include/minkhip.h): shared by multistart.hip, which ranks the
// final configurations of a target's seeds with it, trajectory_multistart.hip, which sums it along a candidate path, and
// ladder.hip, whose edges it prices.
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

// The same distance from ONE configuration q to N others at once, each read through a stride (element a of q at q[a·qs], of the
// k-th other at r[k + a·rs]): the ladder search (ladder.hip) keeps its rungs component-major in LDS, and N independent sums in
// flight hide the latency of the joint table and LDS reads that one sum waits for in turn.  Term for term, and in the same order
// per sum, the arithmetic above.  Only the first n <= N others exist: the rest re-read the last one (their d is not used).
template <int N>
__device__ __forceinline__ void ms_distance_strided(const int32_t* jnt, int njnt, const double* q, int qs, const double* r, int rs,
                                                    int n, const double* w, double (&d)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) d[k] = 0.0;
  const int last = n - 1;
  for (int j = 0; j < njnt; ++j) {
    const int jt = jnt[3 * j];
    int qa = jnt[3 * j + 1], va = jnt[3 * j + 2];
    if (jt != MS_JNT_FREE && jt != MS_JNT_BALL) {
      const double qv = q[qa * qs], wv = w ? w[va] : 1.0;
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const double dv = qv - r[(k < last ? k : last) + qa * rs];
        d[k] += wv * dv * dv;
      }
      continue;
    }
    if (jt == MS_JNT_FREE) {
      for (int c = 0; c < 3; ++c) {
        const double qv = q[(qa + c) * qs], wv = w ? w[va + c] : 1.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double dv = qv - r[(k < last ? k : last) + (qa + c) * rs];
          d[k] += wv * dv * dv;
        }
      }
      qa += 3; va += 3;
    }
    const Q4 qq{q[qa * qs], q[(qa + 1) * qs], q[(qa + 2) * qs], q[(qa + 3) * qs]};
    const double w0 = w ? w[va] : 1.0, w1 = w ? w[va + 1] : 1.0, w2 = w ? w[va + 2] : 1.0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const double* const rk = r + (k < last ? k : last);
      const V3 dw = quat2vel(qmul(qconj(Q4{rk[qa * rs], rk[(qa + 1) * rs], rk[(qa + 2) * rs], rk[(qa + 3) * rs]}), qq));
      d[k] += w0 * dw.x * dw.x + w1 * dw.y * dw.y + w2 * dw.z * dw.z;
    }
  }
}

}  // namespace mkh
