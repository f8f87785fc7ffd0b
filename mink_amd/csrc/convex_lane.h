// The lane body of the kernels that run the general convex distance routine on rows of q that exist nowhere in memory:
// convex_sweep_kernel (convex_sweep.hip: the interior samples of swept edges) and convex_check_kernel (convex_check.hip: the nodes
// and samples a check judges inside its launch).  One LANE holds one (row, general convex pair): the poses of the pair's two
// geoms by a walk down their kinematic chains with the row's coordinates taken through an accessor (convex_chain.h), GJK on the
// sorted pair, the expanding polytope for overlapping cores — the wavefront cooperating on one such lane at a time — and the
// polish on the pair's lane.  The DISTANCE alone comes back.  The kernels differ in how a lane's item decodes into a row and a
// pair: `row_of(l, k)` gives the accessor of the item of lane l of this wavefront and sets k, its slot in the checker's list.
//
// Include behind `#define MKH_POLISH_BY_VALUE 1` (convex_dev.h cvx_polish: these kernels carry the routine without scratch).
#pragma once
#include <hip/hip_runtime.h>

#include "mkh_types.h"
#include "wave_ops.h"
#include "collide_dev.h"
#include "clearance_row.h"
#include "convex_chain.h"
#include "sweep_blend.h"
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

// LDS doubles of a wavefront of these kernels: two GJK banks, or the polytope
constexpr int kCvLaneWsDoubles = kEpaWsDoubles > 2 * kGjkWsDoubles ? kEpaWsDoubles : 2 * kGjkWsDoubles;

// The geoms of pair slot k at the row `qrow`.
template <class Row>
__device__ __forceinline__ void cvx_lane_poses(const WideProblem& P, const CvPre& C, int k, const Row& qrow, const CollisionPairDev*& cpp,
                                               V3& gp1, Q4& gq1, V3& gp2, Q4& gq2) {
  const CollisionPairDev& cp = P.pairs[C.pair[k]];
  cpp = &cp;
  V3 xp1, xp2; Q4 xq1, xq2;
  cv_chain_pose(P, qrow, C.chain + C.chain_adr[2 * k], C.chain_adr[2 * k + 1] - C.chain_adr[2 * k], xp1, xq1);
  cv_chain_pose(P, qrow, C.chain + C.chain_adr[2 * k + 1], C.chain_adr[2 * k + 2] - C.chain_adr[2 * k + 1], xp2, xq2);
  gp1 = xp1 + qrot(xq1, V3{cp.lpos1[0], cp.lpos1[1], cp.lpos1[2]});
  gp2 = xp2 + qrot(xq2, V3{cp.lpos2[0], cp.lpos2[1], cp.lpos2[2]});
  gq1 = qmul(xq1, Q4{cp.lquat1[0], cp.lquat1[1], cp.lquat1[2], cp.lquat1[3]});
  gq2 = qmul(xq2, Q4{cp.lquat2[0], cp.lquat2[1], cp.lquat2[2], cp.lquat2[3]});
}

// The distance of this lane's item (want: the lane holds one that is evaluated; every lane of the wavefront calls).
template <class RowOf>
__device__ __forceinline__ double cvx_lane_distance(const WideProblem& P, const CvPre& C, bool want, int lane, double* ws, const RowOf& row_of) {
  double dist = 0.0;
  bool need_epa = false;
  if (want) {
    const CollisionPairDev* cp; V3 gp1, gp2, from, to; Q4 gq1, gq2;
    int k;
    const auto qrow = row_of(lane, k);
    cvx_lane_poses(P, C, k, qrow, cp, gp1, gq1, gp2, gq2);
    dist = cp->ddetect;
    // geom_distance sorts a pair by type code; sorted here (the distance does not depend on the order, and the witness points
    // are not kept), it has nothing to swap, and behind the test for two boxes — an analytic pair, never in these kernels' list —
    // its box–box routine is dead code, and the scratch of that routine's indexed matrix with it (clr_row's idiom)
    const bool flip = cp->type1 > cp->type2;
    const int ta = flip ? cp->type2 : cp->type1, tb = flip ? cp->type1 : cp->type2;
    const V3 sz1{cp->size1[0], cp->size1[1], cp->size1[2]}, sz2{cp->size2[0], cp->size2[1], cp->size2[2]};
    __builtin_assume(ta <= tb);
    if (!(ta == GEOM_BOX && tb == GEOM_BOX))
      // (two GJK banks: every lane of these kernels holds a convex pair)
      geom_distance<false, true>(ta, clr_sel(flip, sz2, sz1), clr_sel(flip, gp2, gp1), clr_sel(flip, gq2, gq1), tb, clr_sel(flip, sz1, sz2),
                                 clr_sel(flip, gp1, gp2), clr_sel(flip, gq1, gq2), cp->ddetect, dist, from, to, flip ? cp->vert2 : cp->vert1,
                                 flip ? cp->nvert2 : cp->nvert1, flip ? cp->vert1 : cp->vert2, flip ? cp->nvert1 : cp->nvert2, &need_epa,
                                 ws + (lane >> 5) * kGjkWsDoubles + (lane & 31));
  }
  // pairs whose cores overlap: one at a time, the wavefront cooperating on the expanding polytope
  for (unsigned long long em = __ballot(want && need_epa); em; em &= em - 1) {
    const int l = (int)__builtin_ctzll(em);
    const CollisionPairDev* cp; V3 gp1, gp2; Q4 gq1, gq2;
    int k;
    const auto qrow = row_of(l, k);
    cvx_lane_poses(P, C, k, qrow, cp, gp1, gq1, gp2, gq2);
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
  return dist;
}

}  // namespace mkh
