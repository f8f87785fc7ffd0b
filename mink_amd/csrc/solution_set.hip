// Distinct solution sets (mkh_solve_multistart_set, mkh_select_distinct; include/minkhip.h "THE RULE OF THE SET"): the selection
// behind multi-start's loops that keeps up to K candidates no two of which lie within min_distance of each other, instead of
// one.  One small kernel and its launcher (declared in outer_launch.h); the loops in front of it are mkh_solve_until's own
// launch: nothing here touches a solve kernel or its argument structs.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"
#include "ms_distance.h"
#include "outer_launch.h"
#include "wave_ops.h"

namespace mkh {

// One wavefront per target.  Lane l owns candidates l, l + 64, ...: their d_ref and their state (SS_INELIGIBLE, SS_UNCOVERED or
// the slot that covers them) sit in LDS — S doubles, then S int32 — and are read and written by the owning lane ONLY, so no
// fence stands between the rounds.  Round j: the wave's argmin of d_ref over the uncovered candidates (multi-start's two
// reductions: the minimum, then the lowest index that attains it) is slot j's representative; every lane prices its uncovered
// candidates against it, and what lies within r² is covered and counted.  K·ceil(S / 64) distances per lane at the most.
// The candidates' rows are read from global memory where the loops left them (B·S·nq doubles once for d_ref, the uncovered
// ones once more per round: they stay in L2) — not staged in LDS.
// The optional arrays: without converged_all every candidate is eligible (status_all is then not read); v_all / iters_all /
// status_all and their outputs are absent for a selection over a caller's own candidates; n_converged likewise.
enum : int32_t { SS_INELIGIBLE = -2, SS_UNCOVERED = -1 };

__global__ __launch_bounds__(64) void solution_set_select_kernel(
    int B, int S, int K, int nq, int nv, int njnt, const int32_t* __restrict__ jnt, const double* __restrict__ q_all,
    const double* __restrict__ v_all, const int32_t* __restrict__ status_all, const int32_t* __restrict__ iters_all,
    const int32_t* __restrict__ converged_all, const double* __restrict__ q_ref, const double* __restrict__ weights, double r2,
    double* __restrict__ q_set, double* __restrict__ v_set, int32_t* __restrict__ iters, int32_t* __restrict__ status,
    int32_t* __restrict__ seed_index, int32_t* __restrict__ multiplicity, double* __restrict__ distance,
    int32_t* __restrict__ n_distinct, int32_t* __restrict__ n_converged, int32_t* __restrict__ n_uncovered) {
  extern __shared__ double ss_lds[];
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  double* const d_ref = ss_lds;                            // [S]
  int32_t* const state = (int32_t*)(ss_lds + S);           // [S]
  const double* const ref = q_ref + (size_t)b * nq;
  const size_t row0 = (size_t)b * S;
  constexpr unsigned kNone = 0xffffffffu;

  unsigned count = 0;
  for (int s = lane; s < S; s += 64) {
    const size_t i = row0 + s;
    const bool ok = !converged_all || (converged_all[i] != 0 && (!status_all || (status_all[i] & ~1) == 0));   // (~1: MKH_ST_OUTSIDE_LIMITS is no failure)
    double d = __builtin_huge_val();
    if (ok) {
      ++count;
      d = ms_distance(jnt, njnt, q_all + i * nq, ref, weights);
      if (!(d >= 0.0) || d > 1.7976931348623157e308) d = 1.7976931348623157e308;   // (NaN / inf: last among the eligible)
    }
    d_ref[s] = d;
    state[s] = ok ? SS_UNCOVERED : SS_INELIGIBLE;
  }
  const int n_elig = (int)wave_sum((double)count);
  int left = n_elig, j = 0;                                // (wave-uniform: both come out of reductions)
  for (; j < K && left > 0; ++j) {
    double best_d = __builtin_huge_val();
    unsigned best_s = kNone;
    for (int s = lane; s < S; s += 64) {
      if (state[s] != SS_UNCOVERED) continue;
      const double d = d_ref[s];
      if (best_s == kNone || d < best_d) { best_d = d; best_s = (unsigned)s; }     // (ascending s: ties keep the lower index)
    }
    const unsigned long long cand = __ballot(best_s != kNone);
    const double dmin = wave_min_nonneg(best_d, cand);
    const int rep = (int)wave_min_u32((best_s != kNone && best_d == dmin) ? best_s : kNone);
    const size_t ip = row0 + rep;
    const double* const q_rep = q_all + ip * nq;
    unsigned covered = 0;
    for (int s = lane; s < S; s += 64) {
      if (state[s] != SS_UNCOVERED) continue;
      const double* const q_s = q_all + (row0 + s) * nq;
      bool in = s == rep;                                  // (the representative itself, whatever its own distance says)
      if (!in) in = ms_distance(jnt, njnt, q_s, q_rep, weights) <= r2;      // (NaN: false — stays uncovered)
      if (!in) {                                           // a bitwise copy of the representative's row: covered like the row itself
        int k = 0;                                         // (conj(q)·q of a quaternion joint need not round to the identity)
        while (k < nq && __double_as_longlong(q_s[k]) == __double_as_longlong(q_rep[k])) ++k;
        in = k == nq;
      }
      if (in) { state[s] = j; ++covered; }
    }
    const int mult = (int)wave_sum((double)covered);
    left -= mult;
    const size_t o = (size_t)b * K + j;
    for (int k = lane; k < nq; k += 64) q_set[o * nq + k] = q_rep[k];
    if (v_set) for (int k = lane; k < nv; k += 64) v_set[o * nv + k] = v_all[ip * nv + k];
    if (lane == 0) {
      if (iters) iters[o] = iters_all[ip];
      if (status) status[o] = status_all[ip];
      seed_index[o] = rep;
      multiplicity[o] = mult;
      distance[o] = dmin;
    }
  }
  const int filled = j;
  for (; j < K; ++j) {                                     // empty slots: candidate 0's row, flagged
    const size_t o = (size_t)b * K + j;
    for (int k = lane; k < nq; k += 64) q_set[o * nq + k] = q_all[row0 * nq + k];
    if (v_set) for (int k = lane; k < nv; k += 64) v_set[o * nv + k] = v_all[row0 * nv + k];
    if (lane == 0) {
      if (iters) iters[o] = iters_all[row0];
      if (status) status[o] = status_all[row0];
      seed_index[o] = -1;
      multiplicity[o] = 0;
      distance[o] = __builtin_huge_val();
    }
  }
  if (lane == 0) {
    n_distinct[b] = filled;
    if (n_converged) n_converged[b] = n_elig;
    n_uncovered[b] = left;
  }
}

hipError_t launch_ss_select(hipStream_t stream, int B, int S, int K, int nq, int nv, int njnt, const int32_t* jnt,
                            const double* q_all, const double* v_all, const int32_t* status_all, const int32_t* iters_all,
                            const int32_t* converged_all, const double* q_ref, const double* weights, double r2, const SsOut& o) {
  if (S < 1 || S > kSsMaxCandidates || K < 1) return hipErrorInvalidValue;
  const size_t lds = (size_t)S * (sizeof(double) + sizeof(int32_t));     // (at most 48 KB)
  hipLaunchKernelGGL(solution_set_select_kernel, dim3((unsigned)B), dim3(64), lds, stream, B, S, K, nq, nv, njnt, jnt, q_all, v_all,
                     status_all, iters_all, converged_all, q_ref, weights, r2, o.q_set, o.v_set, o.iters, o.status, o.seed_index,
                     o.multiplicity, o.distance, o.n_distinct, o.n_converged, o.n_uncovered);
  return hipGetLastError();
}

}  // namespace mkh
