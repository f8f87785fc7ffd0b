// sweep_kernel — the swept clearance of joint-space edges (include/minkhip.h "THE RULE OF THE SWEEP"): mkh_swept_clearance, and
// the stage of the checked ladder calls that marks the edges of the graph whose motion passes through collision.
//
// One edge per wavefront, or — a small arm — per 16-lane DPP row of it, four to a wavefront (launch_clearance's criterion).  The
// group loads the two ends of its edge, forms b ⊖ a ONCE into its slice of LDS (scalars: the difference; quaternions: the axis
// and the angle of the shortest arc, keyframes.hip's arithmetic) and walks the M interior samples: q(u) = a ⊕ u·(b ⊖ a) is built
// in LDS, never in memory, and clr_row (clearance_row.h: the body of clearance_kernel) gives the sample's margin and pair; the
// running minimum over the samples is kept on the same exact integer keys, a strictly smaller key replacing it — the lowest
// sample of a tie, the first NaN.  No atomics, no scratch.  A checker's general convex pairs: convex_sweep_kernel (convex_sweep.hip)
// runs in front on a chunk of edges and leaves their distances per sample row; this kernel then takes the chunk (a first-edge
// offset into the call's edges) and clr_row reads them.
//
// dynamic LDS, per group: poses (7, nbody) | q(u) (nq) | a (nq) | b ⊖ a (nq) doubles
#include <hip/hip_runtime.h>

#include "checker_plan.h"
#include "clearance_row.h"
#include "lie_dev.h"
#include "outer_launch.h"
#include "sweep_blend.h"
#include "sweep_edge.h"

namespace mkh {

// CV: the build for a checker WITH general convex pairs (sweep_cv_kernel below) — a chunk of the call's edges and the distances
// convex_sweep_kernel left for its samples.  Without: sweep_kernel, which reads neither and is the kernel it was.
template <int LPR, bool CV>
__device__ __forceinline__ void sweep_body(const WideProblem* __restrict__ Pg, const SweepKernelArgs& a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int RPW = kWave / LPR;                             // edges per wavefront
  const WideProblem& P = *Pg;
  const int lane = lane_id(), sub = lane & (LPR - 1), grp = lane / LPR;
  const int nbody = P.nbody, nq = P.nq;
  const long long e_raw = (long long)blockIdx.x * RPW + grp;
  const bool live = e_raw < a.N;                               // (an edge past the end repeats the last one and writes nothing)
  const long long e_in = live ? e_raw : a.N - 1, e = CV ? a.e0 + e_in : e_in;        // its place in this launch, and in the call
  // ---- the two ends, and whether the edge is swept at all (sweep_edge.h)
  const SweepEdge g = swp_edge(a, e, nq);
  const double *const pa = g.pa, *const pb = g.pb;
  const bool swept = g.swept;
  const long long eo = g.eo;
  // ---- where this group writes, per lane and in VECTOR registers from here on (null: nothing to write).  With one edge per
  // wavefront everything above is wave-uniform, and the output pointers, the edge index and the mode would sit in scalar registers
  // across the whole sample loop, beside the checker's two dozen table pointers: they were what spilled.
  const bool writer = live && sub == 0;
  double* om = (writer && a.margin) ? a.margin + eo : nullptr;
  int32_t* o0 = (writer && a.mode == kSweepPairs) ? a.i0 + e : nullptr;
  int32_t* o1 = (writer && a.mode == kSweepPairs) ? a.i1 + e : nullptr;
  uint8_t* ob = (writer && a.mode != kSweepPairs && a.blocked) ? a.blocked + eo : nullptr;
  // (general convex pairs: the distances convex_sweep_kernel left for this edge's samples, row i − 1 of them sample i's — the
  //  same treatment: the buffer, its width and the edge's place in the launch stay out of the loop's scalar registers)
  const double* cve = nullptr;
  int n_cv = 0;
  asm volatile("" : "+v"(om), "+v"(o0), "+v"(o1), "+v"(ob));
  if constexpr (CV) {
    cve = a.cv + (size_t)e_in * a.M * a.n_cv;
    n_cv = a.n_cv;
    asm volatile("" : "+v"(cve), "+v"(n_cv));
  }
  ClrRow best{g.idle, 0, 0};                                   // (n_violated: the sample index here)
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
      const ClrRow r = clr_row<LPR, CV ? 1 : 7>(P, sX, sQ, bad, sub, grp, n_cv, cve, CV ? (size_t)(i - 1) : 0, nullptr);
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

template <int LPR>
__global__ __launch_bounds__(64) void sweep_kernel(const WideProblem* __restrict__ Pg, const SweepKernelArgs a) {
  sweep_body<LPR, false>(Pg, a);
}

template <int LPR>
__global__ __launch_bounds__(64) void sweep_cv_kernel(const WideProblem* __restrict__ Pg, const SweepKernelArgs a) {
  sweep_body<LPR, true>(Pg, a);
}

__global__ __launch_bounds__(256) void ladder_free_tracked_kernel(const int32_t* __restrict__ tracked, const double* __restrict__ node_margin,
                                                                  long long total, int32_t* __restrict__ tracked_out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  tracked_out[e] = (tracked[e] != 0 && node_margin[e] >= 0.0) ? 1 : 0;
}

// (the launch's LDS bytes — beyond 64 KB it is refused — and one or four edges per wavefront: checker_plan.h)
hipError_t launch_sweep(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, const SweepArgs& a) {
  const bool quarter = checker_quarter(nbody, n_pairs);
  const size_t lds = sweep_lds_bytes(nbody, nq, n_pairs);
  const long long n = a.count > 0 ? a.count : a.N, blocks = quarter ? (n + 3) / 4 : n;
  if (a.N < 1 || a.M < 1 || n_pairs < 1 || lds > 64 * 1024 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (a.mode != kSweepPairs && (a.W < 1 || a.T < 1)) return hipErrorInvalidValue;
  if (a.mode == kSweepLadder && (a.T < 2 || a.N % ((long long)(a.T - 1) * a.W * a.W) != 0)) return hipErrorInvalidValue;
  const WideProblem* const P = (const WideProblem*)wide_problem;
  if (a.mode == kSweepPairs && (!a.sample || !a.pair)) return hipErrorInvalidValue;          // (the pairs launch writes all three outputs)
  // (a chunk and the general convex pairs' distances come together or not at all)
  if (a.count < 0 || a.first < 0 || (a.count > 0 && a.first + a.count > a.N) || (a.n_cv > 0) != (a.cv != nullptr) || (a.n_cv > 0) != (a.count > 0))
    return hipErrorInvalidValue;
  const SweepKernelArgs k = sweep_kernel_args(a);
  if (a.n_cv > 0) {
    if (quarter)
      hipLaunchKernelGGL(sweep_cv_kernel<16>, dim3((unsigned)blocks), dim3(kWave), lds, stream, P, k);
    else
      hipLaunchKernelGGL(sweep_cv_kernel<64>, dim3((unsigned)blocks), dim3(kWave), lds, stream, P, k);
  } else if (quarter)
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
