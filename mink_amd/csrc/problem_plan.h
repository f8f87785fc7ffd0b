// Planning of a model and of a problem on the host alone: everything mkh_model_create / mkh_problem_create decide — kernel
// family and tableau size, LDS layouts, the lane tables of the low-rank start, the lane / row and the workgroup-per-problem
// descriptors — as plain data with every device pointer null.  minkhip.hip uploads a plan and patches the pointers
// (upload_problem); nothing here needs a device, so tests/host/plan_cases.cpp runs it under the host sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/minkhip.h"
#include "lane_types.h"
#include "lds_layout.h"
#include "mkh_types.h"
#include "variants.h"
#include "wide_types.h"

namespace mkh {

// MuJoCo's mjtGeom codes and the LDS doubles of the general convex routine's workspace, max(kEpaWsDoubles, kGjkWsDoubles): the
// device side states them in collide_dev.h / convex_dev.h, which need a kernel's headers; convex_pre.hip sees both and asserts
// that they agree.
enum { PLAN_GEOM_PLANE = 0, PLAN_GEOM_SPHERE = 2, PLAN_GEOM_CAPSULE = 3, PLAN_GEOM_ELLIPSOID = 4, PLAN_GEOM_CYLINDER = 5, PLAN_GEOM_BOX = 6,
       PLAN_GEOM_MESH = 7 };
constexpr int kConvexWsDoubles = 768;

// The host's copy of a model: the flat arrays problems are planned from, what follows from them once per model, and the six
// lane tables of the wavefront kernels (left at their defaults when `big`).
struct HostModel {
  int nq = 0, nv = 0, nbody = 0, njnt = 0, ngeom = 0, nsite = 0, nrounds = 0;
  std::vector<int32_t> body_parentid, body_rootid, body_jntnum, body_jntadr, body_dofnum, body_dofadr;
  std::vector<int32_t> jnt_type, jnt_qposadr, jnt_dofadr, jnt_bodyid, jnt_limited;
  std::vector<int32_t> dof_bodyid, dof_jntid, dof_parentid, site_bodyid, geom_bodyid, geom_type;
  std::vector<double> body_pos, body_quat, site_pos, site_quat, geom_size, geom_pos, geom_quat, jnt_range;
  std::vector<double> jnt_pos, jnt_axis, jnt_qpos0;   // (per joint; qpos0 at the joint's first qpos address)
  std::vector<double> body_ipos, body_mass, body_subtreemass;
  bool big = false;                // more than 64 bodies or dofs: no lane tables — every problem runs on the workgroup-per-problem kernel
  std::vector<int32_t> geom_dataid, mesh_vertadr, mesh_vertnum;   // mesh geoms: hull vertices (geom frame) in h_mesh_vert
  std::vector<double> h_mesh_vert;   // (bounding radii of mesh geoms; the upload's source)
  // worked out once: the tree by levels, subtree ranges, the subtree of body 1, joint addresses clamped at 0, per dof its
  // kind / index in the joint / qpos address (−1: free joint) / range seen by check_limits (±inf), and per body the dofs
  // on its chain as chain_words 64-bit words
  std::vector<int32_t> level_start, level_body, subtree_last, in_robot, jntadr0;
  std::vector<int32_t> dof_kind, dof_k, dof_qadr;
  std::vector<double> dof_lo, dof_hi;
  int nlevels = 0, chain_words = 1;
  std::vector<uint64_t> chain;     // [nbody][chain_words]
  uint64_t chain_mask(int body) const { return chain[(size_t)body * chain_words]; }   // (models of one wavefront: the one word)
  // lane tables (mkh_types.h BF_* … DF_*)
  std::vector<double> body_f, jnt_f, dof_f;
  std::vector<int32_t> body_i, jnt_i, dof_i;
};

// Experiment switches of problem creation (tools/README.md MKH_DEBUG_*): all zero in the product library, which never reads the
// environment; an experiment build fills them once per create (minkhip.hip plan_switches).
struct PlanSwitches {
  int max_rows = 0;                // MKH_DEBUG_MAX_ROWS: > 0 caps the half-space rows of the wavefront kernels
  bool wood_always = false, no_com_w3 = false, no_tight_rows = false, no_tight_generic = false, no_pair_rows = false,
       no_convex_split = false;
};

// What creation decides and plan_launch reads (MkhProblem derives from it).
struct ProblemSelect {
  int nt = 8;  // tableau rows per lane (compiled variants: multiples of 8)
  int lds_bytes = 0;
  int blocks_per_cu = 1;
  // feature-rich variants (taps / ComTask / collisions / RelativeFrameTask) need the compiler's full VGPR
  // budget: they never use the high-occupancy register maps of NT ≤ 24 (ik_kernel.h MKH_WAVES)
  int nt_full = 8, lds_bytes_full = 0;
  // the workgroup-per-problem kernel (wide_kernel.h): every call of a model beyond one wavefront (wide_only), or the redo
  // launch of the instances a wavefront kernel flagged MKH_ST_ROW_OVERFLOW
  bool wide_only = false;
  int wide_grid = 0, wide_lds = 0;
  // tight rows (capsule-only collision sets on a small tableau): the same problem with fewer half-space rows than pairs — the
  // tightest contacts get them, dropped ones are checked at the solution — launched first; the full-row variant then re-solves
  // what it flagged (SolveArgs::redo_mask)
  int nt_tight = 0, lds_tight = 0;
  // 3-waves-per-SIMD register map + compact LDS layout (ik_kernel.h MKH_W3; variants without collision rows):
  // LDS bytes per wavefront, 0 when no such variant is compiled for this tableau size or it would not reach 12 waves per CU
  int lds_bytes_w3 = 0;
  bool has_relative = false;
  bool simple_pairs = false;       // every collision pair is plane / sphere / capsule (F_SIMPLE_COLL variants)
  bool convex_pairs = false;       // some pair has no analytic routine: general convex distance (F_CONVEX_COLL variants)
  // low-rank ("Woodbury") start of the QP (ik_kernel.h F_WOOD): compiled (NT, NR) pair or 0 when the
  // problem does not qualify; lower bound of the diagonal part of H without the damping argument, and
  // the largest squared task cost (conditioning gate, evaluated per call because damping is a call argument)
  int wood_nt = 0, wood_nr = 0, wood_lds_bytes = 0, wood_lds_bytes_w3 = 0;
  int wood_lds_bytes_w4 = 0;         // LDS bytes of the four-waves product-form build (`44_32_r44_w4o`) when 16 wavefronts per CU fit, else 0
  // low-rank start WITH half-space rows (round 6; `48_40_r48`): the lane tables are in the descriptor(s), LDS bytes of that layout
  // for the tight-rows descriptor and for the main one (0: not available there)
  bool woodr_tables = false;
  int woodr_lds_tight = 0, woodr_lds = 0;
  bool wood_big = false;           // more than kMu task rows, or S columns in a second register set: the F_COM builds carry those
  double wood_min_diag = 0.0, wood_max_cost2 = 0.0;
  // lane-per-problem kernel for small arms (lane_kernel.h): template size (0 = the problem does not qualify)
  int lane_nv = 0, lane_lds = 0;   // lane kernel's template size (0: not eligible)
  int quad_nt = 0;                 // row kernel's column registers, 8 or 16 (0: not eligible)
  bool quad_loop_ok = true;        // two-row build: its fused loop can integrate every coordinate (a free joint is a link)
  LaneDims lane_dims{};
  bool use_cull = false;
  // seed tables: the default weights of a table made from this problem — [f]: 1 when plain FrameTask f has a position cost > 0,
  // [n_frame + f]: an orientation cost > 0; a RelativeFrameTask: 0 / 0
  std::vector<double> frame_w;
};

// The workgroup-per-problem kernel's descriptor and what it points to, apart from the model's own arrays (HostModel).
struct WidePlan {
  bool built = false;
  WideProblem W{};                 // every pointer null
  std::vector<double> pcost, clo, chi, vlim;     // [n][nv]
  bool use_cull = false;
  long long ws_doubles = 0;        // the workgroups' slices of device memory
  uint32_t redo_cap = 0;           // entries of the redo queue
};

// Everything an upload needs.
struct ProblemPlan {
  ProblemSelect sel;
  DeviceProblem dev{};             // every pointer null
  bool tight = false;
  DeviceProblem dev_tight{};       // the tight-rows twin (sel.nt_tight)
  std::vector<FrameTaskDev> ft;
  std::vector<double> pcost, clo, chi, vlim;     // [n][64]
  std::vector<CollisionPairDev> pairs;           // vert1 / vert2 null: pair_vert
  std::vector<long long> pair_vert;              // [pair][2]: offset of a mesh geom's first vertex in the model's mesh array, in doubles; −1: a primitive
  std::vector<PairCull> culls;
  std::vector<int32_t> pair_geom;                // [pair][2]: the geom ids of the pair list (motion_bound.h reads the model through them)
  std::vector<double> dcost, dwgain;
  int lane_class = 0;              // build_lane_problem's size class (0: none, 32: the large descriptor, else the small one)
  LaneProblem2 lane;
  WidePlan wide;
  int n_cv = 0;                    // general convex pairs evaluated in front of the solve (0: no split)
  std::vector<int32_t> cv_pair, cv_adr, cv_chain;
};

int32_t plan_model(const MkhFlatModel* h, HostModel& m, std::string& err);
int32_t plan_problem(const HostModel& m, const MkhProblemDesc& d, int diag, int max_batch, int num_cus, const PlanSwitches& sw,
                     ProblemPlan& plan, std::string& err);

// Resident wavefronts per CU of a kernel variant: bounded by LDS (160 KiB/CU) and by the register map the
// variant was built for (4 waves/SIMD for NT ≤ 8, 3 for NT ≤ 24, else 2 — ik_kernel.h MKH_WAVES).
inline int waves_per_cu(int nt, int lds_bytes, bool w3 = false) {
  int by_lds = (160 * 1024) / (lds_bytes > 0 ? lds_bytes : 1);
  // gfx950 hands LDS out in granules of 320 dwords: 128 of them per CU.  A persistent kernel must not be launched with more
  // workgroups than are resident at once — the ones that wait for a slot start when the first ones EXIT, i.e. after the whole
  // batch, and then walk their static share alone (round 5: `44_36_r44_w3` asked for 16 064 B, 10 per CU by division, 9 by
  // granules: 2.12 ms instead of 1.44 with a third of the CUs idle; SQ_WAVE_CYCLES / SQ_BUSY_CYCLES gave it away).  Applied
  // where a layout lands between the two figures: the F_COM builds on the one-more-wave map.
  if (w3 && nt == 44 && lds_bytes > (160 * 1024) / 12) by_lds = 128 / ((lds_bytes + 1279) / 1280);
  // (w3: the high-occupancy build of the variant — one more resident wave per SIMD than its plain register map)
  const int by_regs = 4 * (nt <= 8 ? 4 : (nt <= 24 ? (w3 ? 4 : 3) : (w3 ? 3 : 2)));
  const int w = by_lds < by_regs ? by_lds : by_regs;
  return w < 1 ? 1 : w;
}

// LDS bytes per wavefront of one build (nt, nr, feat, one-more-wave map) on descriptor D: the `total` of the layout that build's
// kernel indexes (lds_layout.h build_lds_layout — kernel_lds_layout calls the same function with its compile-time constants).
// (prefetch, compact: 0 / 1 while plan_problem tries them; kFromDescriptor once they are fixed in D)
inline int lds_bytes_of(const DeviceProblem& D, int nt, int nr, int feat, bool w3, int prefetch = kFromDescriptor, int compact = kFromDescriptor) {
  return build_lds_layout(D, nt, nr, feat, w3, prefetch, compact).total * (int)sizeof(double);
}
// The two-waves direct-start builds share one reservation per tableau size, whatever their features: the one with collision
// rows, whose layout ends with the pair-selection block (DeviceProblem::n_hsel — 0 in a problem without pairs).
constexpr int kDirectFeat = F_COLL;

}  // namespace mkh
