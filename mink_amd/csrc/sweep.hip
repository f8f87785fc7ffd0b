// sweep_kernel — the swept clearance of joint-space edges (include/minkhip.h "THE RULE OF THE SWEEP"): mkh_swept_clearance, and
// the stage of the checked ladder calls that marks the edges of the graph whose motion passes through collision.
//
// One edge per wavefront, or — a small arm — per 16-lane DPP row of it, four to a wavefront (launch_clearance's criterion).  The
// group loads the two ends of its edge, forms b ⊖ a ONCE into its slice of LDS (scalars: the difference; quaternions: the axis
// and the angle of the shortest arc, keyframes.hip's arithmetic) and walks the M interior samples: q(u) = a ⊕ u·(b ⊖ a) is built
// in LDS, never in memory, and clr_row (clearance_row.h: the body of clearance_kernel) gives the sample's margin and pair; the
// running minimum over the samples is kept on the same exact integer keys, a strictly smaller key replacing it — the lowest
// sample of a tie, the first NaN.  No atomics, no scratch.
//
// dynamic LDS, per group: poses (7, nbody) | q(u) (nq) | a (nq) | b ⊖ a (nq) doubles
#include <hip/hip_runtime.h>

#include "clearance_row.h"
#include "lie_dev.h"
#include "outer_launch.h"
#include "sweep_blend.h"

namespace mkh {

// What the kernel reads of a SweepArgs, one slot per role whatever the mode (kernel arguments live in scalar registers across the
// whole sample loop): p0 = from | nodes, p1 = to, i0 = sample out | tracked, i1 = pair out | node_index.
struct SweepKernelArgs {
  int32_t mode, M, T, W;
  long long N;
  const double *p0, *p1;
  int32_t *i0, *i1;
  double* margin;
  uint8_t* blocked;
};

template <int LPR>
__global__ __launch_bounds__(64) void sweep_kernel(const WideProblem* __restrict__ Pg, const SweepKernelArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int RPW = kWave / LPR;                             // edges per wavefront
  const WideProblem& P = *Pg;
  const int lane = lane_id(), sub = lane & (LPR - 1), grp = lane / LPR;
  const int nbody = P.nbody, nq = P.nq;
  const long long e_raw = (long long)blockIdx.x * RPW + grp;
  const bool live = e_raw < a.N;                               // (an edge past the end repeats the last one and writes nothing)
  const long long e = live ? e_raw : a.N - 1;
  long long eo = e;                                            // where the edge's outputs go
  // ---- the two ends, and whether the edge is swept at all
  const double *pa, *pb;
  bool swept = true;
  double idle = __builtin_nan("");                             // the margin of an edge that is not swept
  if (a.mode == kSweepPairs) {
    pa = a.p0 + (size_t)e * nq;
    pb = a.p1 + (size_t)e * nq;
  } else {
    const long long W = a.W;
    long long row, src, dst;                                   // waypoint row b·T + t, source node of rung t − 1, destination of t
    if (a.mode == kSweepLadder) {                              // (rungs t >= 1 only: e counts the (T − 1)·W·W edges of an instance)
      const long long per = (long long)(a.T - 1) * W * W, r = e % per;
      row = (e / per) * a.T + 1 + r / (W * W);
      src = r % W;
      dst = (r / W) % W;
      eo = (row * W + dst) * W + src;
    } else {
      row = e;
      dst = a.i1[row];
      src = row % a.T ? a.i1[row - 1] : 0;
    }
    const bool first = row % a.T == 0;
    if (first && a.mode == kSweepPath) idle = __builtin_huge_val();
    swept = !first && a.i0[row * W + dst] != 0;
    pb = a.p0 + (size_t)(row * W + dst) * nq;
    pa = swept ? a.p0 + (size_t)((row - 1) * W + src) * nq : pb;     // (an idle group walks its own node: every address is valid)
  }
  // ---- where this group writes, per lane and in VECTOR registers from here on (null: nothing to write).  With one edge per
  // wavefront everything above is wave-uniform, and the output pointers, the edge index and the mode would sit in scalar registers
  // across the whole sample loop, beside the checker's two dozen table pointers: they were what spilled.
  const bool writer = live && sub == 0;
  double* om = (writer && a.margin) ? a.margin + eo : nullptr;
  int32_t* o0 = (writer && a.mode == kSweepPairs) ? a.i0 + e : nullptr;
  int32_t* o1 = (writer && a.mode == kSweepPairs) ? a.i1 + e : nullptr;
  uint8_t* ob = (writer && a.mode != kSweepPairs && a.blocked) ? a.blocked + eo : nullptr;
  asm volatile("" : "+v"(om), "+v"(o0), "+v"(o1), "+v"(ob));
  ClrRow best{idle, 0, 0};                                     // (n_violated: the sample index here)
  if (__ballot(swept && live) != 0ull) {                       // (wave-uniform: a wavefront with nothing to sweep leaves here)
    double* const sX = smem + (size_t)grp * (7 * nbody + 3 * nq);
    double *const sQ = sX + 7 * nbody, *const sA = sQ + nq, *const sD = sA + nq;
    // ---- an end with a NaN or an infinite entry: every sample is NaN
    bool bad = false;
    for (int i = sub; i < nq; i += LPR) bad = bad || !(pa[i] - pa[i] == 0.0) || !(pb[i] - pb[i] == 0.0);
    {
      const unsigned long long bb = __ballot(bad);
      bad = (LPR == 64 ? bb : (bb >> (grp * LPR)) & ((1ull << (LPR & 63)) - 1ull)) != 0ull;
    }
    swp_difference<LPR>(P, pa, pb, sA, sD, sub);
    wave_sync();
    unsigned long long best_key = ~0ull;                       // (above every key: sample 0 always enters)
    const double steps = (double)(a.M + 1);
    for (int i = 1; i <= a.M; ++i) {
      swp_blend<LPR>(P, sA, sD, (double)i / steps, sQ, sub);
      wave_sync();
      const ClrRow r = clr_row<LPR>(P, sX, sQ, bad, sub, grp, 0, nullptr, 0, nullptr);
      const unsigned long long key = clr_key(r.margin);
      if (swept && key < best_key) { best_key = key; best = ClrRow{r.margin, r.pair, i - 1}; }
      wave_sync();                                             // (the next sample's q(u) and poses overwrite what the pairs read)
    }
  }
  if (om) *om = best.margin;
  if (o0) *o0 = best.n_violated;
  if (o1) *o1 = best.pair;
  if (ob) *ob = (swept && !(best.margin >= 0.0)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void ladder_free_tracked_kernel(const int32_t* __restrict__ tracked, const double* __restrict__ node_margin,
                                                                  long long total, int32_t* __restrict__ tracked_out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  tracked_out[e] = (tracked[e] != 0 && node_margin[e] >= 0.0) ? 1 : 0;
}

// The launch's LDS bytes (beyond 64 KB the launch is refused): four slices where a quarter of a wavefront holds an edge.
size_t sweep_lds_bytes(int nbody, int nq, int n_pairs) {
  const bool quarter = nbody <= 32 && n_pairs <= 32;
  return (size_t)(quarter ? 4 : 1) * (7 * (size_t)nbody + 3 * (size_t)nq) * sizeof(double);
}

hipError_t launch_sweep(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, const SweepArgs& a) {
  const bool quarter = nbody <= 32 && n_pairs <= 32;
  const size_t lds = sweep_lds_bytes(nbody, nq, n_pairs);
  const long long blocks = quarter ? (a.N + 3) / 4 : a.N;
  if (a.N < 1 || a.M < 1 || n_pairs < 1 || lds > 64 * 1024 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (a.mode != kSweepPairs && (a.W < 1 || a.T < 1)) return hipErrorInvalidValue;
  if (a.mode == kSweepLadder && (a.T < 2 || a.N % ((long long)(a.T - 1) * a.W * a.W) != 0)) return hipErrorInvalidValue;
  const WideProblem* const P = (const WideProblem*)wide_problem;
  const bool pairs = a.mode == kSweepPairs;
  if (pairs && (!a.sample || !a.pair)) return hipErrorInvalidValue;          // (the pairs launch writes all three outputs)
  const SweepKernelArgs k{a.mode, a.M, a.T, a.W, a.N, pairs ? a.from : a.nodes, pairs ? a.to : nullptr,
                          pairs ? a.sample : const_cast<int32_t*>(a.tracked), pairs ? a.pair : const_cast<int32_t*>(a.node_index),
                          a.margin, pairs ? nullptr : a.blocked};
  if (quarter)
    hipLaunchKernelGGL(sweep_kernel<16>, dim3((unsigned)blocks), dim3(kWave), lds, stream, P, k);
  else
    hipLaunchKernelGGL(sweep_kernel<64>, dim3((unsigned)blocks), dim3(kWave), lds, stream, P, k);
  return hipGetLastError();
}

hipError_t launch_ladder_free_tracked(hipStream_t stream, const int32_t* tracked, const double* node_margin, long long total,
                                      int32_t* tracked_out) {
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_free_tracked_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, tracked, node_margin, total, tracked_out);
  return hipGetLastError();
}

}  // namespace mkh
