// Multi-start trajectory IK (mkh_solve_trajectory_multistart, include/minkhip.h "THE RULE"): the two kernels behind the T loop
// launches of the B·S candidate trajectories — scoring every candidate over its whole path and choosing one per instance, then
// gathering the chosen candidate's rows into the caller's arrays — and their launchers (declared in outer_launch.h).  In front
// of the loops sit multistart.hip's seeding and fan-out kernels, behind the gather trajectory.hip's waypoint velocity.  The candidates' results are time-major: row t·(B·S) + b·S + s.  Nothing here touches a solve kernel.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"
#include "ms_distance.h"
#include "outer_launch.h"
#include "wave_ops.h"

namespace mkh {

// One wavefront per instance: lane l walks the paths of candidates l, l + 64, ...; the wave agrees on the candidate with the
// most tracked waypoints, then the shortest path, then the lowest index.
__global__ __launch_bounds__(64) void tms_score_select_kernel(
    int B, int S, int T, int nq, int njnt, const int32_t* __restrict__ jnt, const double* __restrict__ q0,
    const double* __restrict__ q_all, const int32_t* __restrict__ status_all, const int32_t* __restrict__ converged_all,
    const double* __restrict__ weights, const double* __restrict__ edge_margin_all, int32_t* __restrict__ seed_index,
    int32_t* __restrict__ n_tracked, int32_t* __restrict__ n_complete, double* __restrict__ path_length) {
#pragma clang fp contract(off)      // length: a rounded sum of the waypoints' distances, in ascending t
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  const size_t R = (size_t)B * S;
  const double* const start = q0 + (size_t)b * nq;
  constexpr unsigned kNone = 0xffffffffu;
  constexpr double kLast = 1.7976931348623157e308;
  unsigned best_s = kNone, best_n = 0, complete = 0;
  double best_key = __builtin_huge_val(), best_len = 0.0, first_len = 0.0;
  for (int s = lane; s < S; s += 64) {
    const size_t i = (size_t)b * S + s;
    unsigned n = 0;
    double len = 0.0;
    const double* prev = start;                              // (q_{-1}: the caller's q[b], not the seed)
    for (int t = 0; t < T; ++t) {
      const size_t row = (size_t)t * R + i;
      // (~1: MKH_ST_OUTSIDE_LIMITS is no failure.  The flags are optional for mkh_select_trajectory_candidates: absent, every
      // row passes.  edge_margin_all — "THE RULE, with a checker" —: a waypoint entered by a motion that collides, or was not
      // swept (NaN), does not count; waypoint 0's start edge is never asked)
      if ((!converged_all || converged_all[row] != 0) && (!status_all || (status_all[row] & ~1) == 0) &&
          (!edge_margin_all || t == 0 || edge_margin_all[row] >= 0.0))
        ++n;
      const double* const cur = q_all + row * nq;
      len += ms_distance(jnt, njnt, cur, prev, weights);
      prev = cur;
    }
    if (n == (unsigned)T) ++complete;
    double key = len;
    if (!(key >= 0.0) || key > kLast) key = kLast;           // (NaN / inf: last among its count; weights are >= 0, so nothing finite is < 0)
    if (s == lane) first_len = len;
    if (best_s == kNone || n > best_n || (n == best_n && key < best_key)) {  // (ascending s: ties keep the lower index)
      best_s = (unsigned)s; best_n = n; best_key = key; best_len = len;
    }
  }
  const bool has = best_s != kNone;
  const unsigned nmax = wave_max_u32(has ? best_n : 0u);
  const bool in = has && best_n == nmax;
  const unsigned long long cand = __ballot(in);
  const double dmin = wave_min_nonneg(in ? best_key : __builtin_huge_val(), cand);
  const unsigned smin = wave_min_u32((in && best_key == dmin) ? best_s : kNone);
  const int n_comp = (int)wave_sum((double)complete);
  // nobody tracked a waypoint: candidate 0, the caller's own start (smin < S always: the gather indexes with it)
  const int pick = (nmax && smin < (unsigned)S) ? (int)smin : 0;
  const double len_pick = nmax ? readlane_f64(best_len, pick & 63) : readlane_f64(first_len, 0);
  if (lane == 0) {
    seed_index[b] = pick;
    n_tracked[b] = (int)nmax;
    n_complete[b] = n_comp;
    path_length[b] = len_pick;
  }
}

// out[b, t, k] = all[t, b·S + seed_index[b], k] through the (instance, waypoint) strides of `out` in elements: either caller
// layout is written in place.  One thread per output element, k fastest.
template <class V>
__device__ __forceinline__ void tms_gather(const V* __restrict__ all, V* __restrict__ out, const int32_t* __restrict__ seed_index,
                                           long long total, int B, int S, int W, long long o_sb, long long o_st) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int k = (int)(e % W);
  const long long i = e / W;                                 // t·B + b
  const int b = (int)(i % B);
  const long long t = i / B;
  out[b * o_sb + t * o_st + k] = all[((t * B + b) * S + seed_index[b]) * W + k];
}

__global__ __launch_bounds__(256) void tms_gather_kernel(const double* __restrict__ all, double* __restrict__ out,
                                                         const int32_t* __restrict__ seed_index, long long total, int B, int S,
                                                         int W, long long o_sb, long long o_st) {
  tms_gather(all, out, seed_index, total, B, S, W, o_sb, o_st);
}

// The same for the (T, B·S) int32 results: status, iteration counts, converged flags.
__global__ __launch_bounds__(256) void tms_gather_i32_kernel(const int32_t* __restrict__ all, int32_t* __restrict__ out,
                                                             const int32_t* __restrict__ seed_index, long long total, int B,
                                                             int S, long long o_sb, long long o_st) {
  tms_gather(all, out, seed_index, total, B, S, 1, o_sb, o_st);
}

hipError_t launch_tms_score(hipStream_t stream, int B, int S, int T, int nq, int njnt, const int32_t* jnt, const double* q0,
                            const double* q_all, const int32_t* status_all, const int32_t* converged_all, const double* weights,
                            const double* edge_margin_all, int32_t* seed_index, int32_t* n_tracked, int32_t* n_complete,
                            double* path_length) {
  hipLaunchKernelGGL(tms_score_select_kernel, dim3((unsigned)B), dim3(64), 0, stream, B, S, T, nq, njnt, jnt, q0, q_all, status_all,
                     converged_all, weights, edge_margin_all, seed_index, n_tracked, n_complete, path_length);
  return hipGetLastError();
}

hipError_t launch_tms_gather(hipStream_t stream, const double* all, double* out, const int32_t* seed_index, int B, int S, int T,
                             int W, long long o_sb, long long o_st) {
  const long long total = (long long)B * T * W;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tms_gather_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, all, out, seed_index, total, B, S, W, o_sb, o_st);
  return hipGetLastError();
}

hipError_t launch_tms_gather_i32(hipStream_t stream, const int32_t* all, int32_t* out, const int32_t* seed_index, int B, int S,
                                 int T, long long o_sb, long long o_st) {
  const long long total = (long long)B * T;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tms_gather_i32_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, all, out, seed_index, total, B, S, o_sb, o_st);
  return hipGetLastError();
}

}  // namespace mkh
