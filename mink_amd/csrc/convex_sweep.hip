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
#include "mkh_types.h"
#include "wave_ops.h"
#include "collide_dev.h"
#include "clearance_row.h"
#include "convex_chain.h"
#include "problem_plan.h"
#include "sweep_blend.h"
#include "sweep_edge.h"
#include "wide_types.h"

namespace mkh {

// The row q(u) between the rows a and b, formed joint by joint as the chain walk asks: what swp_difference / swp_blend leave
// in LDS, without the row existing anywhere.
struct CvRowBlend {
  const double *a, *b;
  double u;
  __device__ __forceinline__ double scalar(int qa) const { return swp_scalar_blend(a[qa], swp_scalar_difference(a[qa], b[qa]), u); }
  __device__ __forceinline__ V3 pos(int qa) const { return V3{scalar(qa), scalar(qa + 1), scalar(qa + 2)}; }
  __device__ __forceinline__ Q4 quat(int qa) const {
    Q4 qn; V3 ax; double nrm;
    swp_quat_difference(Q4{a[qa], a[qa + 1], a[qa + 2], a[qa + 3]}, Q4{b[qa], b[qa + 1], b[qa + 2], b[qa + 3]}, qn, ax, nrm);
    return swp_quat_blend(qn, ax, nrm, u);
  }
};

// `ipw` items per wavefront (lanes [0, ipw) work), as in convex_contacts_kernel: one long dependent chain per lane, spread thin.
__global__ __launch_bounds__(64) void convex_sweep_kernel(const WideProblem* __restrict__ Pg, CvPre C, const SweepKernelArgs a, int ipw,
                                                          double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double ws[kEpaWsDoubles > 2 * kGjkWsDoubles ? kEpaWsDoubles : 2 * kGjkWsDoubles];
  const WideProblem& P = *Pg;
  const int lane = lane_id(), nq = P.nq;
  const long long base = (long long)blockIdx.x * ipw, total = a.N * a.M * C.n_cv;
  // item = (edge of the chunk · M + sample) · n_cv + slot: its index in `out`
  auto edge_of = [&](long long item) { return swp_edge(a, a.e0 + item / ((long long)a.M * C.n_cv), nq); };
  auto poses = [&](long long item, const SweepEdge& g, const CollisionPairDev*& cpp, V3& gp1, Q4& gq1, V3& gp2, Q4& gq2) {
    const long long row = item / C.n_cv;
    const int k = (int)(item - row * C.n_cv), i = (int)(row % a.M) + 1;
    const CollisionPairDev& cp = P.pairs[C.pair[k]];
    cpp = &cp;
    const CvRowBlend qrow{g.pa, g.pb, (double)i / (double)(a.M + 1)};        // (sweep_kernel's u of sample i − 1)
    V3 xp1, xp2; Q4 xq1, xq2;
    cv_chain_pose(P, qrow, C.chain + C.chain_adr[2 * k], C.chain_adr[2 * k + 1] - C.chain_adr[2 * k], xp1, xq1);
    cv_chain_pose(P, qrow, C.chain + C.chain_adr[2 * k + 1], C.chain_adr[2 * k + 2] - C.chain_adr[2 * k + 1], xp2, xq2);
    gp1 = xp1 + qrot(xq1, V3{cp.lpos1[0], cp.lpos1[1], cp.lpos1[2]});
    gp2 = xp2 + qrot(xq2, V3{cp.lpos2[0], cp.lpos2[1], cp.lpos2[2]});
    gq1 = qmul(xq1, Q4{cp.lquat1[0], cp.lquat1[1], cp.lquat1[2], cp.lquat1[3]});
    gq2 = qmul(xq2, Q4{cp.lquat2[0], cp.lquat2[1], cp.lquat2[2], cp.lquat2[3]});
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
  double dist = 0.0;
  bool need_epa = false;
  if (want) {
    const CollisionPairDev* cp; V3 gp1, gp2, from, to; Q4 gq1, gq2;
    poses(item, edge_of(item), cp, gp1, gq1, gp2, gq2);
    dist = cp->ddetect;
    // geom_distance sorts a pair by type code; sorted here (the distance does not depend on the order, and the witness points
    // are not kept), it has nothing to swap, and behind the test for two boxes — an analytic pair, never in this kernel's list —
    // its box–box routine is dead code, and the scratch of that routine's indexed matrix with it (clr_row's idiom)
    const bool flip = cp->type1 > cp->type2;
    const int ta = flip ? cp->type2 : cp->type1, tb = flip ? cp->type1 : cp->type2;
    const V3 sz1{cp->size1[0], cp->size1[1], cp->size1[2]}, sz2{cp->size2[0], cp->size2[1], cp->size2[2]};
    __builtin_assume(ta <= tb);
    if (!(ta == GEOM_BOX && tb == GEOM_BOX))
      // (two GJK banks: every lane of this kernel holds a convex pair)
      geom_distance<false, true>(ta, clr_sel(flip, sz2, sz1), clr_sel(flip, gp2, gp1), clr_sel(flip, gq2, gq1), tb, clr_sel(flip, sz1, sz2),
                                 clr_sel(flip, gp1, gp2), clr_sel(flip, gq1, gq2), cp->ddetect, dist, from, to, flip ? cp->vert2 : cp->vert1,
                                 flip ? cp->nvert2 : cp->nvert1, flip ? cp->vert1 : cp->vert2, flip ? cp->nvert1 : cp->nvert2, &need_epa,
                                 ws + (lane >> 5) * kGjkWsDoubles + (lane & 31));
  }
  // pairs whose cores overlap: one at a time, the wavefront cooperating on the expanding polytope
  for (unsigned long long em = __ballot(want && need_epa); em; em &= em - 1) {
    const int l = (int)__builtin_ctzll(em);
    const CollisionPairDev* cp; V3 gp1, gp2; Q4 gq1, gq2;
    poses(base + l, edge_of(base + l), cp, gp1, gq1, gp2, gq2);
    // (loose polytope + polish on the pair's lane; without a certificate the tight polytope — collide_dev.h geom_overlap_polish)
    const V3 sz1{cp->size1[0], cp->size1[1], cp->size1[2]}, sz2{cp->size2[0], cp->size2[1], cp->size2[2]};
    bool certified = false;
#pragma nounroll
    for (int pass = geom_overlap_loose(cp->type1, cp->type2) ? 0 : 1; pass < 2 && !certified; ++pass) {
      double d_e; V3 f_e, t_e;
      geom_overlap_distance(cp->type1, sz1, gp1, gq1, cp->type2, sz2, gp2, gq2, d_e, f_e, t_e, cp->vert1, cp->nvert1, cp->vert2, cp->nvert2, ws,
                            pass ? kEpaTol : kLooseEpa);
      bool ok = false;
      if (lane == l) {
        dist = d_e;
        ok = geom_overlap_polish(cp->type1, sz1, gp1, gq1, cp->type2, sz2, gp2, gq2, dist, f_e, t_e, pass != 0);
      }
      certified = __ballot(ok) != 0;
    }
  }
  if (want) out[item] = dist;
}

hipError_t launch_convex_sweep(hipStream_t stream, const void* wide_problem, const int32_t* pair, const int32_t* chain_adr,
                               const int32_t* chain, const SweepArgs& a, int ipw) {
  if (a.count < 1 || a.first < 0 || a.first + a.count > a.N || a.M < 1 || a.n_cv < 1 || !a.cv) return hipErrorInvalidValue;
  const SweepKernelArgs k = sweep_kernel_args(a);
  const CvPre C{a.n_cv, pair, chain_adr, chain};
  const long long total = a.count * a.M * a.n_cv;
  // ≈ 4 096 wavefronts when the chunk allows, at most 64 items each (launch_convex_pre's choice, measured again here:
  // docs/HISTORY.md)
  if (ipw < 1) {
    const long long w = (total + 4095) / 4096;
    ipw = (int)(w < 1 ? 1 : (w > 64 ? 64 : w));
  }
  if (ipw > 64) ipw = 64;
  const long long blocks = (total + ipw - 1) / ipw;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(convex_sweep_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, (const WideProblem*)wide_problem, C, k, ipw, a.cv);
  return hipGetLastError();
}

}  // namespace mkh
