// lr_check_kernel — the collision check of one step of the refinement pass "with a checker" (include/minkhip.h "THE RULE OF THE
// REFINEMENT, with a checker"): launched between every loop launch of the pass and the step kernel that commits its result.
//
// One instance per wavefront, or — a small arm — per 16-lane DPP row of it, four to a wavefront (launch_clearance's criterion,
// sweep_kernel's LDS slice).  For an instance that was BAD at waypoint t and whose loop result x tracks, the group evaluates up to
// 2M + 1 rows of q: the clearance of x itself, and — only when x is free — the M interior samples of the NEAR edge (the one the
// acceptance test judges: forward r_{t-1} → x, backward x → r_{t+1}) and of the FAR edge the commit would create (forward
// x → r_{t+1}, backward r_{t-1} → x), each swept only when its destination is effectively tracked.  The rows are built in LDS with
// the sweep's difference and blend (sweep_blend.h) and judged by clr_row (clearance_row.h); nothing is written to memory but three
// doubles per instance and SLOT — margin(x) | near | far, NaN: not evaluated or not swept.  No atomics, no scratch.
//
// The rows of one instance are a serial chain on its group, and a step of the pass waits for the longest chain: the M samples of
// an edge are therefore dealt to NW = gridDim.y slots, block (·, s) taking samples s + 1, s + 1 + NW, …; every slot evaluates
// margin(x) itself (it decides whether the edges are swept at all) and writes the minimum over ITS samples — the step kernel
// takes the minimum over the slots, a NaN deciding (lr_trip in ladder_refine.hip).  The chain is 1 + 2·ceil(M / NW) rows.
//
// A checker's general convex pairs: convex_check_kernel (convex_check.hip) runs in front on a chunk of instances, once for all
// slots, and leaves their distances on x and on every sample of the two edges this kernel could read; lr_check_cv_kernel then
// takes the chunk (a first-instance offset) and clr_row reads them.
//
// dynamic LDS, per group: poses (7, nbody) | q(u) (nq) | a (nq) | b ⊖ a (nq) doubles
#include <hip/hip_runtime.h>

#include "checker_plan.h"
#include "clearance_row.h"
#include "lie_dev.h"
#include "outer_launch.h"
#include "sweep_blend.h"

namespace mkh {

// Whether any lane of this lane's group holds `x`.
template <int LPR>
__device__ __forceinline__ bool lrc_group_any(bool x, int grp) {
  const unsigned long long bb = __ballot(x);
  return (LPR == 64 ? bb : (bb >> (grp * LPR)) & ((1ull << (LPR & 63)) - 1ull)) != 0ull;
}

// CV: the build for a checker WITH general convex pairs (lr_check_cv_kernel below) — a chunk of the call's instances (B of them
// from instance c.first) and the distances convex_check_kernel left for the chunk: row 0 of an instance x's, rows 1 … M the near
// edge's samples, rows M + 1 … 2M the far edge's; every slot reads the same rows.  Without: lr_check_kernel, which reads neither
// and is the kernel it was.  (No __restrict__ on the body's pointers: the kernels' parameters carry it; repeated on the inlined
// body it changes what the compiler may reorder, and lr_check_kernel<16> spilled 9 SGPRs for 6.)
template <int LPR, bool CV>
__device__ __forceinline__ void lr_check_body(const WideProblem* Pg, int B, int T, int M, int ct, int cdir,
                                              const double* r, const int32_t* r_trk,
                                              const double* x, const int32_t* xst,
                                              const int32_t* xcv, const int32_t* bad,
                                              double* trip, const CvChunk& c) {
  const int NW = (int)gridDim.y, slot = (int)blockIdx.y;       // (launch_lr_check: 1 <= NW <= M, so every slot holds a sample)
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int RPW = kWave / LPR;                             // instances per wavefront
  const WideProblem& P = *Pg;
  const int lane = lane_id(), sub = lane & (LPR - 1), grp = lane / LPR;
  const int nbody = P.nbody, nq = P.nq;
  const int b_raw = blockIdx.x * RPW + grp;
  const bool live = b_raw < B;                                 // (an instance past the end repeats the last one and writes nothing)
  const int b_in = live ? b_raw : B - 1, b = CV ? (int)c.first + b_in : b_in;          // its place in this launch, and in the call
  const size_t row = (size_t)b * T + ct;
  // ---- what this instance needs: a bad waypoint whose loop result tracks (the ladder's definition: ladder_refine.hip lr_tracks)
  const bool work = live && bad[b] != 0 && xcv[b] != 0 && (xst[b] & ~1) == 0;
  // ---- where this group writes, per lane and in VECTOR registers from here on (sweep_kernel's idiom: with one instance per
  // wavefront the address would sit in scalar registers across both sample loops, beside the checker's table pointers)
  double* out = (live && sub == 0) ? trip + (size_t)b * 3 * NW + slot : nullptr;
  asm volatile("" : "+v"(out));
  // (general convex pairs: the same treatment — the buffer and its width stay out of the loops' scalar registers)
  const double* cve = nullptr;
  int n_cv = 0;
  if constexpr (CV) {
    cve = c.cv + (size_t)b_in * (2 * M + 1) * c.n_cv;
    n_cv = c.n_cv;
    asm volatile("" : "+v"(cve), "+v"(n_cv));
  }
  const double nan = __builtin_nan("");
  double m_node = nan, m_near = nan, m_far = nan;
  if (__ballot(work) != 0ull) {                                // (wave-uniform: a wavefront in which no group has work leaves here)
    double* const sX = smem + (size_t)grp * (7 * nbody + 3 * nq);
    double *const sQ = sX + 7 * nbody, *const sA = sQ + nq, *const sD = sA + nq;
    const double* const px = x + (size_t)b * nq;
    const double* const node = r + row * nq;                   // (an instance that needs nothing walks its own node: every address is valid)
    // ---- 1. margin(x)
    const double* const pn = work ? px : node;
    bool bad_x = false;
    for (int i = sub; i < nq; i += LPR) bad_x = bad_x || !(pn[i] - pn[i] == 0.0);
    bad_x = lrc_group_any<LPR>(bad_x, grp);
    {
      const ClrRow cr = clr_row<LPR, CV ? 1 : 7>(P, sX, pn, bad_x, sub, grp, n_cv, cve, 0, nullptr);
      if (work) m_node = cr.margin;
      wave_sync();                                             // (the first sample's poses overwrite what the pairs read)
    }
    const bool free_x = work && m_node >= 0.0;                 // (a colliding node skips its two edges)
    // ---- 2. the near edge, 3. the far edge: forward (r_{t-1} → x), (x → r_{t+1}); backward (x → r_{t+1}), (r_{t-1} → x)
    const bool has_prev = ct >= 1, has_next = ct + 1 < T;
    const bool next_trk = has_next && r_trk[has_next ? row + 1 : row] != 0;
    const double steps = (double)(M + 1);
#pragma unroll 1
    for (int e = 0; e < 2; ++e) {
      const bool into_x = (cdir > 0) == (e == 0);              // the edge r_{t-1} → x; else x → r_{t+1}
      // (swept iff its destination is effectively tracked: x is, once free; r_{t+1} by its flag)
      const bool swept = free_x && (into_x ? has_prev : next_trk);
      if (__ballot(swept) == 0ull) continue;                   // (wave-uniform)
      const double* const pa = swept ? (into_x ? node - nq : px) : node;
      const double* const pb = swept ? (into_x ? px : node + nq) : node;
      bool bad_e = false;
      for (int i = sub; i < nq; i += LPR) bad_e = bad_e || !(pa[i] - pa[i] == 0.0) || !(pb[i] - pb[i] == 0.0);
      bad_e = lrc_group_any<LPR>(bad_e, grp);
      swp_difference<LPR>(P, pa, pb, sA, sD, sub);
      wave_sync();
      unsigned long long best_key = ~0ull;                     // (above every key: sample 0 always enters)
      double best = nan;
      for (int i = 1 + slot; i <= M; i += NW) {
        swp_blend<LPR>(P, sA, sD, (double)i / steps, sQ, sub);
        wave_sync();
        const ClrRow cr = clr_row<LPR, CV ? 1 : 7>(P, sX, sQ, bad_e, sub, grp, n_cv, cve, CV ? (size_t)(e * M + i) : 0, nullptr);
        const unsigned long long key = clr_key(cr.margin);
        if (key < best_key) { best_key = key; best = cr.margin; }
        wave_sync();                                           // (the next sample's q(u) and poses overwrite what the pairs read)
      }
      if (swept && e == 0) m_near = best;
      if (swept && e != 0) m_far = best;
    }
  }
  if (out) { out[0] = m_node; out[NW] = m_near; out[2 * NW] = m_far; }
}

template <int LPR>
__global__ __launch_bounds__(64) void lr_check_kernel(const WideProblem* __restrict__ Pg, int B, int T, int M, int ct, int cdir,
                                                      const double* __restrict__ r, const int32_t* __restrict__ r_trk,
                                                      const double* __restrict__ x, const int32_t* __restrict__ xst,
                                                      const int32_t* __restrict__ xcv, const int32_t* __restrict__ bad,
                                                      double* __restrict__ trip) {
  lr_check_body<LPR, false>(Pg, B, T, M, ct, cdir, r, r_trk, x, xst, xcv, bad, trip, CvChunk{});
}

template <int LPR>
__global__ __launch_bounds__(64) void lr_check_cv_kernel(const WideProblem* __restrict__ Pg, int B, int T, int M, int ct, int cdir,
                                                         const double* __restrict__ r, const int32_t* __restrict__ r_trk,
                                                         const double* __restrict__ x, const int32_t* __restrict__ xst,
                                                         const int32_t* __restrict__ xcv, const int32_t* __restrict__ bad,
                                                         double* __restrict__ trip, const CvChunk c) {
  lr_check_body<LPR, true>(Pg, B, T, M, ct, cdir, r, r_trk, x, xst, xcv, bad, trip, c);
}

int lr_check_slots(int M) { return M < kLrMaxSlots ? (M < 1 ? 1 : M) : kLrMaxSlots; }

hipError_t launch_lr_check(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, int B, int T, int M,
                           int commit_t, int commit_dir, const LrWork& w, double* trip, const CvChunk& chunk) {
  const bool quarter = checker_quarter(nbody, n_pairs);
  const size_t lds = sweep_lds_bytes(nbody, nq, n_pairs);
  if (B < 1 || T < 1 || M < 1 || n_pairs < 1 || lds > 64 * 1024 || commit_t < 0 || commit_t >= T) return hipErrorInvalidValue;
  if (commit_dir < 0 && commit_t > T - 2) return hipErrorInvalidValue;       // (a backward step reads t + 1)
  const WideProblem* const P = (const WideProblem*)wide_problem;
  const unsigned nw = (unsigned)lr_check_slots(M);
  // (a chunk and the general convex pairs' distances come together or not at all)
  if ((chunk.cv != nullptr) != (chunk.n_cv > 0) || (chunk.cv != nullptr) != (chunk.count > 0) || chunk.first < 0 || chunk.count < 0 ||
      chunk.first + chunk.count > B)
    return hipErrorInvalidValue;
  if (chunk.cv) {
    const int n = (int)chunk.count;                            // the kernel's B: the instances of this launch
    if (quarter)
      hipLaunchKernelGGL(lr_check_cv_kernel<16>, dim3((unsigned)((n + 3) / 4), nw), dim3(kWave), lds, stream, P, n, T, M, commit_t, commit_dir,
                         w.r, w.r_trk, w.x, w.xst, w.xcv, w.bad, trip, chunk);
    else
      hipLaunchKernelGGL(lr_check_cv_kernel<64>, dim3((unsigned)n, nw), dim3(kWave), lds, stream, P, n, T, M, commit_t, commit_dir, w.r, w.r_trk,
                         w.x, w.xst, w.xcv, w.bad, trip, chunk);
  } else if (quarter)
    hipLaunchKernelGGL(lr_check_kernel<16>, dim3((unsigned)((B + 3) / 4), nw), dim3(kWave), lds, stream, P, B, T, M, commit_t, commit_dir, w.r,
                       w.r_trk, w.x, w.xst, w.xcv, w.bad, trip);
  else
    hipLaunchKernelGGL(lr_check_kernel<64>, dim3((unsigned)B, nw), dim3(kWave), lds, stream, P, B, T, M, commit_t, commit_dir, w.r, w.r_trk,
                       w.x, w.xst, w.xcv, w.bad, trip);
  return hipGetLastError();
}

}  // namespace mkh
