// Trajectory IK (mkh_solve_trajectory, include/minkhip.h): the small kernels around the T fused-loop launches — the
// batch-major → time-major transpose of the targets, the transpose of the results back, the finite-difference joint
// velocity between waypoints — and their launchers (declared in outer_launch.h).  The loops
// between them are mkh_solve_until's / mkh_solve_steps' own launches: nothing here touches a solve kernel or its argument
// structs.  All of them are bandwidth kernels: one thread per output element, consecutive threads store consecutive addresses.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"
#include "outer_launch.h"

namespace mkh {

enum : int32_t { TJ_JNT_FREE = 0, TJ_JNT_BALL = 1 };       // mjtJoint (2 / 3: slide / hinge)

// dst (T, B, W) ← src (B, T, W).  Thread e writes dst[e]; its W-runs of src are contiguous.
__global__ __launch_bounds__(256) void trajectory_gather_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                                long long total, int B, int T, int W) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int k = (int)(e % W);
  const long long i = e / W;                               // t·B + b
  const int b = (int)(i % B);
  const long long t = i / B;
  dst[e] = src[((long long)b * T + t) * W + k];
}

// dst (B, T, W) ← src (T, B, W): the results of the loops back into the caller's batch-major arrays.
__global__ __launch_bounds__(256) void trajectory_scatter_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                                 long long total, int B, int T, int W) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int k = (int)(e % W);
  const long long i = e / W;                               // b·T + t
  const int t = (int)(i % T);
  const long long b = i / T;
  dst[e] = src[((long long)t * B + b) * W + k];
}

// The same for the (T, B) int32 results: status, iteration counts, converged flags.
__global__ __launch_bounds__(256) void trajectory_scatter_i32_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                                     long long total, int B, int T) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int t = (int)(e % T);
  const long long b = e / T;
  dst[e] = src[(long long)t * B + b];
}

// qvel[b, t] = mj_differentiatePos(q_{t-1}[b], q_t[b]) at waypoint_dt, q_{-1} = q0[b].  One thread per (instance, waypoint,
// joint), joints fastest.  q_traj and qvel are addressed through (instance, waypoint) strides in elements, so that either
// layout is read and written in place.  jnt[3·j + {0,1,2}] = joint type, qpos address, dof address (ms_build_tables).
__global__ __launch_bounds__(256) void trajectory_qvel_kernel(const int32_t* __restrict__ jnt, int njnt, int B, int T, int nq,
                                                              const double* __restrict__ q0, const double* __restrict__ q_traj,
                                                              long long q_sb, long long q_st, double dt,
                                                              double* __restrict__ qvel, long long v_sb, long long v_st,
                                                              int time_major) {
#pragma clang fp contract(off)      // (q_t − q_{t−1}) / dt rounds like the numpy restatement: a difference, then a quotient
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)B * T * njnt;
  if (e >= total) return;
  const int j = (int)(e % njnt);
  const long long i = e / njnt;
  const int b = (int)(time_major ? i % B : i / T);
  const int t = (int)(time_major ? i / B : i % T);
  const double* const cur = q_traj + b * q_sb + t * q_st;
  const double* const prev = t > 0 ? cur - q_st : q0 + (long long)b * nq;
  double* const out = qvel + b * v_sb + t * v_st;
  const int jt = jnt[3 * j];
  int qa = jnt[3 * j + 1], va = jnt[3 * j + 2];
  if (jt != TJ_JNT_FREE && jt != TJ_JNT_BALL) {
    out[va] = (cur[qa] - prev[qa]) / dt;
    return;
  }
  if (jt == TJ_JNT_FREE) {
    for (int k = 0; k < 3; ++k) out[va + k] = (cur[qa + k] - prev[qa + k]) / dt;
    qa += 3; va += 3;
  }
  // mju_subQuat: rotation vector of conj(q_{t-1})·q_t, over dt
  const V3 dw = quat2vel(qmul(qconj(Q4{prev[qa], prev[qa + 1], prev[qa + 2], prev[qa + 3]}),
                              Q4{cur[qa], cur[qa + 1], cur[qa + 2], cur[qa + 3]}));
  out[va] = dw.x / dt; out[va + 1] = dw.y / dt; out[va + 2] = dw.z / dt;
}

hipError_t launch_tj_gather(hipStream_t stream, const double* src, double* dst, int B, int T, int W) {
  const long long total = (long long)B * T * W;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(trajectory_gather_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, src, dst, total, B, T, W);
  return hipGetLastError();
}

hipError_t launch_tj_scatter(hipStream_t stream, const double* src, double* dst, int B, int T, int W) {
  const long long total = (long long)B * T * W;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(trajectory_scatter_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, src, dst, total, B, T, W);
  return hipGetLastError();
}

hipError_t launch_tj_scatter_i32(hipStream_t stream, const int32_t* src, int32_t* dst, int B, int T) {
  const long long total = (long long)B * T;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(trajectory_scatter_i32_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, src, dst, total, B, T);
  return hipGetLastError();
}

hipError_t launch_tj_qvel(hipStream_t stream, const int32_t* jnt, int njnt, int B, int T, int nq, const double* q0,
                          const double* q_traj, long long q_sb, long long q_st, double dt, double* qvel, long long v_sb,
                          long long v_st, int time_major) {
  const long long total = (long long)B * T * njnt;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(trajectory_qvel_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, jnt, njnt, B, T, nq, q0, q_traj, q_sb, q_st, dt,
                     qvel, v_sb, v_st, time_major);
  return hipGetLastError();
}

}  // namespace mkh
