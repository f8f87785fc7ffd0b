// convex_sweep_kernel — the general convex distance routine on the interior samples of swept edges, in front of sweep_kernel.
//
// A checker's pairs without an analytic routine (cylinder–box, cylinder–cylinder, ellipsoid–*, mesh hulls) are pre-evaluated for
// clr_row (clearance_row.h) by a kernel of their own (convex_pre.hip, and why).  That kernel reads rows of q from memory; the
// samples of a sweep exist only in sweep_kernel's LDS.  Here one LANE takes one (edge, sample, general convex pair) of a chunk of
// edges: it decodes its edge as sweep_kernel does (sweep_edge.h), walks the two kinematic chains of its pair with the joints'
// coordinates blended on the fly — q(u) = a ⊕ u·(b ⊖ a) by the per-joint functions of sweep_blend.h, the same doubles
// sweep_kernel puts into LDS for the analytic pairs of that sample —, runs GJK and, for overlapping shapes, the expanding
// polytope (convex_dev.h), and writes the DISTANCE alone, 8 bytes, to row (edge of the chunk · M + sample) of the checker's
// buffer (mkh_problem_set_sweep_rows), which sweep_kernel reads through clr_row<LPR, 1>.
//
// A lane does nothing for an edge that is not swept (an untracked destination, a first waypoint: on a sparse checked ladder
// that is most edges, and a wavefront of them leaves at once) nor for an edge with a NaN or an infinite end (clr_row makes every
// distance of such a sample NaN before it looks at the record; the routine never runs on non-finite poses).  The bounding-sphere
// cull of clr_row is NOT applied here: its test reads body poses out of sweep_kernel's level-by-level FK, the poses here come from
// a walk down one chain, and a value the sweep reads must never be one this kernel skipped.
#include <hip/hip_runtime.h>

#define MKH_POLISH_BY_VALUE 1      // (convex_dev.h cvx_polish: this kernel carries the routine without scratch)
#include "checker_plan.h"
#include "convex_lane.h"
#include "problem_plan.h"
#include "sweep_edge.h"

namespace mkh {

// `ipw` items per wavefront (lanes [0, ipw) work), as in convex_contacts_kernel: one long dependent chain per lane, spread thin.
// The lane body — poses, GJK, the cooperative polytope, the polish — is convex_lane.h's, shared with convex_check_kernel.
__global__ __launch_bounds__(64) void convex_sweep_kernel(const WideProblem* __restrict__ Pg, CvPre C, const SweepKernelArgs a, int ipw,
                                                          double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double ws[kCvLaneWsDoubles];
  const WideProblem& P = *Pg;
  const int lane = lane_id(), nq = P.nq;
  const long long base = (long long)blockIdx.x * ipw, total = a.N * a.M * C.n_cv;
  // item = (edge of the chunk · M + sample) · n_cv + slot: its index in `out`
  auto edge_of = [&](long long item) { return swp_edge(a, a.e0 + item / ((long long)a.M * C.n_cv), nq); };
  auto row_of = [&](int l, int& k) {
    const long long item = base + l, row = item / C.n_cv;
    const SweepEdge g = edge_of(item);
    k = (int)(item - row * C.n_cv);
    return CvRowBlend{g.pa, g.pb, (double)((int)(row % a.M) + 1) / (double)(a.M + 1)};       // (sweep_kernel's u of sample i − 1)
  };
  const long long item = base + lane;
  bool want = lane < ipw && item < total;
  if (want) {                                                  // ---- is the edge swept, and are its ends finite
    const SweepEdge g = edge_of(item);
    want = g.swept;
    if (want)
      for (int i = 0; i < nq; ++i) want = want && (g.pa[i] - g.pa[i] == 0.0) && (g.pb[i] - g.pb[i] == 0.0);
  }
  if (__ballot(want) == 0ull) return;                          // (wave-uniform)
  const double dist = cvx_lane_distance(P, C, want, lane, ws, row_of);
  if (want) out[item] = dist;
}

hipError_t launch_convex_sweep(hipStream_t stream, const void* wide_problem, const CvPre& C, const SweepArgs& a, int ipw) {
  if (a.count < 1 || a.first < 0 || a.first + a.count > a.N || a.M < 1 || a.n_cv < 1 || C.n_cv != a.n_cv || !a.cv) return hipErrorInvalidValue;
  const SweepKernelArgs k = sweep_kernel_args(a);
  const long long total = a.count * a.M * a.n_cv;
  // (launch_convex_pre's choice, measured again here: docs/HISTORY.md)
  if (ipw < 1) ipw = cv_items_per_wave(total);
  if (ipw > 64) ipw = 64;
  const long long blocks = (total + ipw - 1) / ipw;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(convex_sweep_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, (const WideProblem*)wide_problem, C, k, ipw, a.cv);
  return hipGetLastError();
}

}  // namespace mkh
