// Descriptors of the lane- and row-per-problem kernels (lane_kernel.h, quad_kernel.h), shared with the host side that fills them
// (problem_plan.hip build_lane_problem).
#pragma once
#include <stdint.h>

#include "mkh_types.h"

namespace mkh {

constexpr int kLaneMaxLinks = 16;       // descriptor of the lane kernel and of the row kernel's one-row builds
constexpr int kLaneMaxDofs = 8;         // the lane kernel's own limit (its register arrays)
constexpr int kLaneDescDofs = 16;       // (the row kernel takes up to 16 dofs on one DPP row)
constexpr int kLaneMaxLinks2 = 32, kLaneDescDofs2 = 32;   // descriptor of the row kernel's two-row build (17 … 32 dofs or links)
constexpr int kLaneMaxFrames = 8;       // frame tasks of a problem (round 3: 4 → 8, a hand's fingertips + its palm)

struct LaneLink {
  int32_t parent;        // link index of the parent body, −1 = world
  int32_t jtype;         // −1 none, JNT_SLIDE, JNT_HINGE; JNT_BALL: the rotation of a free joint (two-row build of the row kernel only —
                         // a free joint is three slide links along the world axes with `pos` = 0 and this link on top of them)
  int32_t dof;           // dof / register index of the joint coordinate
  int32_t qadr;          // JNT_BALL: address of the quaternion in q
  double pos[3], quat[4];
  double axis[3], jpos[3], qpos0;
};

struct LaneFrame {
  int32_t link;          // link the frame is attached to (−1: the world body)
  uint32_t chain;        // dofs on the chain world → frame
  int32_t rowmask, pad;
  double lpos[3], lquat[4], cost[6], gain, lm_damping;
};

// ML links, MD dofs of capacity: two instantiations, so that the two-row build's larger tables leave the layout (and with it
// the register allocation) of the lane kernel and of the one-row builds exactly as it was
template <int ML, int MD>
struct LaneProblemT {
  int32_t nq, nv, nlink, n_frame, n_posture, n_cfg, n_vel, pad;
  LaneLink link[ML];
  int32_t dof_link[MD];   // link whose joint moves dof d (−1: not on any task chain)
  int32_t dof_qadr[MD];
  double range_lo[MD], range_hi[MD];    // joint range for check_limits (±inf)
  LaneFrame frame[kLaneMaxFrames];
  double posture_cost[kMaxPostureTasks][MD], posture_gain[kMaxPostureTasks], posture_lm[kMaxPostureTasks];
  double cfg_gain[kMaxBoxTerms], cfg_lower[kMaxBoxTerms][MD], cfg_upper[kMaxBoxTerms][MD];
  double vel_limit[kMaxBoxTerms][MD];
  // per dof, for the row kernel (quad_kernel.h: one load level less than dof_link → link): the joint's axis and anchor in its
  // body frame, and whether it is a slide joint
  double dof_axis[MD][3], dof_jpos[MD][3];
  int32_t dof_slide[MD];
  // ComTask (two-row build of the row kernel only; appended so that the offsets above stay what they were): every body of the robot
  // is a link then; a link carries its own mass (jointless children folded in) at link_ipos, its subtree is the contiguous range
  // [link, link_last] (links are in body order), link_stmass that range's mass; bodies fixed to the world enter as a constant
  int32_t n_com, com_rowmask;
  double com_cost[3], com_gain, com_lm, com_minv;       // com_minv = 1 / mass of the subtree of body 1
  double com_static[3];                                  // Σ m·p over the bodies of that subtree that are fixed to the world
  double link_mass[ML], link_ipos[ML][3], link_stmass[ML];
  int32_t link_last[ML];
  // RelativeFrameTask (two-row build only; appended for the same reason): frame task t measures its frame in the frame `root`
  struct Rel { int32_t relative, root_link; uint32_t rchain; int32_t pad; double rlpos[3], rlquat[4]; } rel[kLaneMaxFrames];
};
using LaneProblem = LaneProblemT<kLaneMaxLinks, kLaneDescDofs>;
using LaneProblem2 = LaneProblemT<kLaneMaxLinks2, kLaneDescDofs2>;

// the same problem in the smaller descriptor (host side; the builder fills the large one)
template <int ML, int MD, int ML2, int MD2>
inline void lane_problem_narrow(const LaneProblemT<ML2, MD2>& b, LaneProblemT<ML, MD>& a) {
  a.nq = b.nq; a.nv = b.nv; a.nlink = b.nlink; a.n_frame = b.n_frame; a.n_posture = b.n_posture; a.n_cfg = b.n_cfg; a.n_vel = b.n_vel; a.pad = 0;
  for (int i = 0; i < ML; ++i) a.link[i] = b.link[i];
  for (int i = 0; i < kLaneMaxFrames; ++i) a.frame[i] = b.frame[i];
  for (int d = 0; d < MD; ++d) {
    a.dof_link[d] = b.dof_link[d]; a.dof_qadr[d] = b.dof_qadr[d]; a.range_lo[d] = b.range_lo[d]; a.range_hi[d] = b.range_hi[d];
    a.dof_slide[d] = b.dof_slide[d];
    for (int c = 0; c < 3; ++c) { a.dof_axis[d][c] = b.dof_axis[d][c]; a.dof_jpos[d][c] = b.dof_jpos[d][c]; }
    for (int t = 0; t < kMaxPostureTasks; ++t) a.posture_cost[t][d] = b.posture_cost[t][d];
    for (int t = 0; t < kMaxBoxTerms; ++t) { a.cfg_lower[t][d] = b.cfg_lower[t][d]; a.cfg_upper[t][d] = b.cfg_upper[t][d]; a.vel_limit[t][d] = b.vel_limit[t][d]; }
  }
  for (int t = 0; t < kMaxPostureTasks; ++t) { a.posture_gain[t] = b.posture_gain[t]; a.posture_lm[t] = b.posture_lm[t]; }
  for (int t = 0; t < kMaxBoxTerms; ++t) a.cfg_gain[t] = b.cfg_gain[t];
  a.n_com = 0; a.com_rowmask = 0;                        // (no ComTask, no RelativeFrameTask on the small descriptor)
  for (int t = 0; t < kLaneMaxFrames; ++t) a.rel[t].relative = 0;
}

// The sizes of a LaneProblem, by value in the row kernel's arguments (SGPRs at wave start instead of a dependent load).
// `qadr_identity`: dof d reads q[d] (always the case for nq = nv with hinge / slide joints only; checked on the host).
struct LaneDims { int32_t nq, nv, nlink, n_frame, n_posture, n_cfg, n_vel, qadr_identity; };

// bytes of LDS per wavefront: link poses [nlink][7][64] (joint axes and anchors are recomputed from the pose where a
// Jacobian column needs them: ~40 flops instead of 6 more doubles of LDS per link and lane, i.e. residency)
__host__ __device__ inline int lane_lds_bytes(int nlink) { return nlink * 7 * kWave * (int)sizeof(double); }

}  // namespace mkh
