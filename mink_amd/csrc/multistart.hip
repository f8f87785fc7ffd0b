// Multi-start IK (mkh_solve_multistart, include/minkhip.h): the three small kernels around the fused loop — seeding,
// target fan-out, selection — and their launchers (declared in outer_launch.h).  The loop
// between them is mkh_solve_until's own launch: nothing here touches a solve kernel or its argument structs.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"
#include "ms_distance.h"
#include "outer_launch.h"
#include "wave_ops.h"

namespace mkh {

// per-qpos-address seeding table: seed_i[3·a + {0,1,2}] = kind, quaternion component, draw index; seed_f[2·a + {0,1}] =
// lower bound, width (ball: θmax in the width slot)
enum : int32_t {
  MS_KEEP = 0,     // the caller's value: free joints, unlimited slides
  MS_RANGE = 1,    // lo + width·u(draw): limited hinge / slide
  MS_AROUND = 2,   // (q[b] − π) + 2π·u(draw): unlimited hinge
  MS_BALL = 3,     // one component of the quaternion of a random rotation vector; draws draw, draw + 1, draw + 2
};

// The generator of include/minkhip.h "Random numbers": stateless, a function of (rng_seed, target, seed, draw) alone.
__device__ __forceinline__ unsigned long long ms_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double ms_uniform(unsigned long long rng_seed, unsigned long long target, unsigned s, unsigned draw) {
  constexpr unsigned long long G = 0x9E3779B97F4A7C15ull;
  unsigned long long h = ms_mix(rng_seed + G);
  h = ms_mix((h ^ target) + G);
  h = ms_mix((h ^ (((unsigned long long)s << 32) | draw)) + G);
  return (double)(h >> 11) * 0x1.0p-53;                    // 53 bits: [0, 1), exact
}

// One thread per element of q_seeds (B·S, nq): consecutive threads write consecutive addresses.
__global__ __launch_bounds__(256) void multistart_seed_kernel(const int32_t* __restrict__ seed_i, const double* __restrict__ seed_f,
                                                              int B, int S, int nq, const double* __restrict__ q,
                                                              const double* __restrict__ user_seeds, unsigned long long rng_seed,
                                                              long long target_index0, double* __restrict__ q_seeds) {
#pragma clang fp contract(off)      // lo + width·u and its kin round like the numpy restatement: a product, then a sum
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)B * S * nq;
  if (e >= total) return;
  const int a = (int)(e % nq);
  const long long i = e / nq;
  const int s = (int)(i % S);
  const int b = (int)(i / S);
  const double own = q[(size_t)b * nq + a];
  double val = own;
  if (s > 0 && user_seeds) {
    val = user_seeds[e];
  } else if (s > 0) {
    const int kind = seed_i[3 * a], comp = seed_i[3 * a + 1];
    const unsigned draw = (unsigned)seed_i[3 * a + 2];
    const unsigned long long t = (unsigned long long)(target_index0 + b);
    const double lo = seed_f[2 * a], width = seed_f[2 * a + 1];
    if (kind == MS_RANGE) {
      val = lo + width * ms_uniform(rng_seed, t, (unsigned)s, draw);
    } else if (kind == MS_AROUND) {
      val = (own - M_PI) + (2.0 * M_PI) * ms_uniform(rng_seed, t, (unsigned)s, draw);
    } else if (kind == MS_BALL) {
      const double u1 = ms_uniform(rng_seed, t, (unsigned)s, draw), u2 = ms_uniform(rng_seed, t, (unsigned)s, draw + 1),
                   u3 = ms_uniform(rng_seed, t, (unsigned)s, draw + 2);
      const double z = 2.0 * u1 - 1.0;
      const double r = sqrt(1.0 - z * z);
      const double phi = (2.0 * M_PI) * u2, half = 0.5 * (width * u3);
      double sp, cp, sh, ch;
      sincos_cw(phi, &sp, &cp);
      sincos_cw(half, &sh, &ch);
      val = comp == 0 ? ch : (comp == 1 ? (r * cp) * sh : (comp == 2 ? (r * sp) * sh : z * sh));
    }
  }
  q_seeds[e] = val;
}

// dst (B·S, width): row i is row i / S of src (B, width).  One thread per output element.
__global__ __launch_bounds__(256) void multistart_fanout_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                                long long total, int S, int width) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long long i = e / width;
  const int k = (int)(e % width);
  dst[e] = src[(size_t)(i / S) * width + k];
}

// One wavefront per target: lane l looks at seeds l, l + 64, ...; the wave agrees on the closest converged one.
__global__ __launch_bounds__(64) void multistart_select_kernel(
    int B, int S, int nq, int nv, int njnt, const int32_t* __restrict__ jnt, const double* __restrict__ q_all,
    const double* __restrict__ v_all, const int32_t* __restrict__ status_all, const int32_t* __restrict__ iters_all,
    const int32_t* __restrict__ converged_all, const double* __restrict__ q_ref, const double* __restrict__ weights,
    double* __restrict__ q_best, double* __restrict__ v_best, int32_t* __restrict__ iters, int32_t* __restrict__ status,
    int32_t* __restrict__ converged, int32_t* __restrict__ seed_index, int32_t* __restrict__ n_converged) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  const double* const ref = q_ref + (size_t)b * nq;
  constexpr unsigned kNone = 0xffffffffu;
  double best_d = __builtin_huge_val();
  unsigned best_s = kNone, count = 0;
  for (int s = lane; s < S; s += 64) {
    const size_t i = (size_t)b * S + s;
    if (converged_all[i] == 0 || (status_all[i] & ~1) != 0) continue;       // (~1: MKH_ST_OUTSIDE_LIMITS is no failure)
    ++count;
    double d = ms_distance(jnt, njnt, q_all + i * nq, ref, weights);
    if (!(d >= 0.0) || d > 1.7976931348623157e308) d = 1.7976931348623157e308;   // (NaN / inf: last among the converged)
    if (best_s == kNone || d < best_d) { best_d = d; best_s = (unsigned)s; }     // (ascending s: ties keep the lower index)
  }
  const unsigned long long cand = __ballot(best_s != kNone);
  const double dmin = wave_min_nonneg(best_d, cand);
  const unsigned smin = wave_min_u32((best_s != kNone && best_d == dmin) ? best_s : kNone);
  const int n_conv = (int)wave_sum((double)count);
  const int pick = cand ? (int)smin : 0;                   // nothing converged: seed 0, the caller's own start
  const size_t ip = (size_t)b * S + pick;
  for (int k = lane; k < nq; k += 64) q_best[(size_t)b * nq + k] = q_all[ip * nq + k];
  for (int k = lane; k < nv; k += 64) v_best[(size_t)b * nv + k] = v_all[ip * nv + k];
  if (lane == 0) {
    iters[b] = iters_all[ip];
    status[b] = status_all[ip];
    converged[b] = cand ? 1 : 0;
    seed_index[b] = pick;
    n_converged[b] = n_conv;
  }
}

hipError_t launch_ms_seed(hipStream_t stream, const int32_t* seed_i, const double* seed_f, int B, int S, int nq, const double* q,
                          const double* user_seeds, unsigned long long rng_seed, long long target_index0, double* q_seeds) {
  unsigned grid;
  if (!grid_1d((long long)B * S * nq, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(multistart_seed_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, seed_i, seed_f, B, S, nq, q, user_seeds,
                     rng_seed, target_index0, q_seeds);
  return hipGetLastError();
}

hipError_t launch_ms_fanout(hipStream_t stream, const double* src, double* dst, int B, int S, int width) {
  const long long total = (long long)B * S * width;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(multistart_fanout_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, src, dst, total, S, width);
  return hipGetLastError();
}

hipError_t launch_ms_select(hipStream_t stream, int B, int S, int nq, int nv, int njnt, const int32_t* jnt, const double* q_all,
                            const double* v_all, const int32_t* status_all, const int32_t* iters_all, const int32_t* converged_all,
                            const double* q_ref, const double* weights, double* q_best, double* v_best, int32_t* iters,
                            int32_t* status, int32_t* converged, int32_t* seed_index, int32_t* n_converged) {
  hipLaunchKernelGGL(multistart_select_kernel, dim3((unsigned)B), dim3(64), 0, stream, B, S, nq, nv, njnt, jnt, q_all, v_all,
                     status_all, iters_all, converged_all, q_ref, weights, q_best, v_best, iters, status, converged, seed_index,
                     n_converged);
  return hipGetLastError();
}

}  // namespace mkh
