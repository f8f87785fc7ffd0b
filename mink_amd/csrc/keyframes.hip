// Keyframed trajectory IK (mkh_solve_keyframes, include/minkhip.h "The rule"): the kernels that blend waypoint t's targets from
// keyframes k and k + 1, launched on the caller's stream directly in front of waypoint t's fused loop — and their launchers
// (declared in outer_launch.h).  Segment k and parameter u are chosen on the host and are scalars of
// the launch.  The keyframe arrays are read in place through (instance, keyframe) strides in elements, so batch-major
// (B, K, ·) and time-major (K, B, ·) cost no transpose; the result goes to the (rows, ·) slab the loop reads and, when the
// caller asked for the interpolated targets, to waypoint t of that array as well.  Bandwidth kernels: one thread per pose /
// joint / element, consecutive threads store consecutive addresses, no LDS.  Nothing here touches a solve kernel.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"
#include "outer_launch.h"

namespace mkh {

enum : int32_t { KF_JNT_FREE = 0, KF_JNT_BALL = 1 };       // mjtJoint (2 / 3: slide / hinge)

// Frame targets (wxyz_xyz), one thread per (row, frame task): rotation normalize(q_a ⊗ exp(u·log(q_a⁻¹ ⊗ q_b))), translation
// p_a + u·(p_b − p_a).  u == 0: keyframe k, bit for bit (keyframe k + 1 is not read: k may be the last one).
__global__ __launch_bounds__(256) void keyframe_frames_kernel(const double* __restrict__ keys, long long s_b, long long s_k, int k,
                                                              double u, int rows, int n_frame, double* __restrict__ slab,
                                                              double* __restrict__ out, long long o_sb) {
#pragma clang fp contract(off)      // p_a + u·(p_b − p_a) rounds like the numpy restatement: a difference, a product, a sum
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)rows * n_frame) return;
  const int f = (int)(e % n_frame);
  const long long b = e / n_frame;
  const double* const a = keys + b * s_b + (long long)k * s_k + 7 * f;
  double r[7];
  if (u == 0.0) {
#pragma unroll
    for (int i = 0; i < 7; ++i) r[i] = a[i];
  } else {
    const double* const c = a + s_k;
    const Q4 qa{a[0], a[1], a[2], a[3]}, qb{c[0], c[1], c[2], c[3]};
    const V3 w = so3_log(qmul(qconj(qa), qb));
    const Q4 q = qnormalize(qmul(qa, so3_exp(u * w)));
    r[0] = q.w; r[1] = q.x; r[2] = q.y; r[3] = q.z;
#pragma unroll
    for (int i = 4; i < 7; ++i) r[i] = a[i] + u * (c[i] - a[i]);
  }
  double* const d = slab + e * 7;
#pragma unroll
  for (int i = 0; i < 7; ++i) d[i] = r[i];
  if (out) {
    double* const o = out + b * o_sb + 7 * f;
#pragma unroll
    for (int i = 0; i < 7; ++i) o[i] = r[i];
  }
}

// Posture targets, one thread per (row, posture task, joint), joints fastest: q_a ⊕ u·(q_b ⊖ q_a) with ⊖ = mj_differentiatePos
// at dt = 1 and ⊕ = mj_integratePos.  jnt[3·j + {0,1,2}] = joint type, qpos address, dof address (ms_build_tables).
__global__ __launch_bounds__(256) void keyframe_posture_kernel(const int32_t* __restrict__ jnt, int njnt,
                                                               const double* __restrict__ keys, long long s_b, long long s_k,
                                                               int k, double u, int rows, int n_posture, int nq,
                                                               double* __restrict__ slab, double* __restrict__ out,
                                                               long long o_sb) {
#pragma clang fp contract(off)      // a + u·(b − a): a difference, a product, a sum
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)rows * n_posture * njnt) return;
  const int j = (int)(e % njnt);
  const long long i = e / njnt;
  const int pt = (int)(i % n_posture);
  const long long b = i / n_posture;
  const double* const a = keys + b * s_b + (long long)k * s_k + (long long)pt * nq;
  const double* const c = a + s_k;                         // (read only when u != 0)
  double* const d = slab + i * nq;
  double* const o = out ? out + b * o_sb + (long long)pt * nq : nullptr;
  const int jt = jnt[3 * j];
  int qa = jnt[3 * j + 1];
  if (jt != KF_JNT_FREE && jt != KF_JNT_BALL) {
    const double r = u == 0.0 ? a[qa] : a[qa] + u * (c[qa] - a[qa]);
    d[qa] = r;
    if (o) o[qa] = r;
    return;
  }
  if (jt == KF_JNT_FREE) {
    for (int n = 0; n < 3; ++n) {
      const double r = u == 0.0 ? a[qa + n] : a[qa + n] + u * (c[qa + n] - a[qa + n]);
      d[qa + n] = r;
      if (o) o[qa + n] = r;
    }
    qa += 3;
  }
  Q4 q{a[qa], a[qa + 1], a[qa + 2], a[qa + 3]};
  if (u != 0.0) {
    // mju_quatIntegrate(q_a, mju_subQuat(q_b, q_a), u): the rotation vector of conj(q_a)·q_b (angle in (−π, π]: the shortest
    // arc whatever the sign of either quaternion), its axis turned by u times its angle, applied on the right of q_a
    const V3 w = quat2vel(qmul(qconj(q), Q4{c[qa], c[qa + 1], c[qa + 2], c[qa + 3]}));
    const double nrm = sqrt(w.x * w.x + w.y * w.y + w.z * w.z);
    V3 ax{1.0, 0.0, 0.0};
    if (nrm >= 1e-15) ax = V3{w.x / nrm, w.y / nrm, w.z / nrm};
    q = qnormalize(qmul(qnormalize(q), axis_angle(ax, u * nrm)));
  }
  d[qa] = q.w; d[qa + 1] = q.x; d[qa + 2] = q.y; d[qa + 3] = q.z;
  if (o) { o[qa] = q.w; o[qa + 1] = q.x; o[qa + 2] = q.y; o[qa + 3] = q.z; }
}

// CoM targets, one thread per element of the (rows, width) slab: a + u·(b − a).
__global__ __launch_bounds__(256) void keyframe_com_kernel(const double* __restrict__ keys, long long s_b, long long s_k, int k,
                                                           double u, int rows, int width, double* __restrict__ slab,
                                                           double* __restrict__ out, long long o_sb) {
#pragma clang fp contract(off)      // a + u·(b − a): a difference, a product, a sum
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)rows * width) return;
  const int n = (int)(e % width);
  const long long b = e / width;
  const double* const a = keys + b * s_b + (long long)k * s_k + n;
  const double r = u == 0.0 ? a[0] : a[0] + u * (a[s_k] - a[0]);
  slab[e] = r;
  if (out) out[b * o_sb + n] = r;
}

hipError_t launch_kf_frames(hipStream_t stream, const double* keys, long long s_b, long long s_k, int k, double u, int rows,
                            int n_frame, double* slab, double* out, long long o_sb) {
  const long long total = (long long)rows * n_frame;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(keyframe_frames_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, keys, s_b, s_k, k, u, rows, n_frame, slab, out, o_sb);
  return hipGetLastError();
}

hipError_t launch_kf_posture(hipStream_t stream, const int32_t* jnt, int njnt, const double* keys, long long s_b, long long s_k,
                             int k, double u, int rows, int n_posture, int nq, double* slab, double* out, long long o_sb) {
  const long long total = (long long)rows * n_posture * njnt;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(keyframe_posture_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, jnt, njnt, keys, s_b, s_k, k, u, rows, n_posture,
                     nq, slab, out, o_sb);
  return hipGetLastError();
}

hipError_t launch_kf_com(hipStream_t stream, const double* keys, long long s_b, long long s_k, int k, double u, int rows,
                         int width, double* slab, double* out, long long o_sb) {
  const long long total = (long long)rows * width;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(keyframe_com_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, keys, s_b, s_k, k, u, rows, width, slab, out, o_sb);
  return hipGetLastError();
}

}  // namespace mkh
