// The plain solve's host side: mkh_eval, mkh_solve, mkh_solve_dense, mkh_solve_steps, mkh_solve_until and solve(), the one function
// behind them and behind the loop launches of the outer-loop calls (minkhip.hip).  Three parts: launch planning (plan_launch: what a
// call runs, decided apart from running it) and launching; the call's arrays on their way to the kernel and back, by the table and
// the route of solve_plan.h; the entry points.  Host code only.
#include "solve_host.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "outer_launch.h"

// The wavefront kernel's variants live in their own translation units (mink_amd/csrc/build.py generates one variant_<name>.hip
// per compiled combination so that they build in parallel) and are reached through the generated table of variants.h; these are
// the launchers of the other kernels (those of the outer-loop entry points' small kernels: outer_launch.h).
namespace mkh {
int launch_lane(int nv_max, bool loop, int grid, int lds_bytes, hipStream_t stream, const LaneProblem* P, const SolveArgs& a);
int launch_quad(int nt, bool loop, int grid, hipStream_t stream, const void* P, const LaneDims& dims, const SolveArgs& a);   // returns its LDS bytes per wavefront
int launch_wide(int grid, int lds_bytes, hipStream_t stream, const WideProblem* P, const SolveArgs& a, const TapArgs* taps, bool convex);
constexpr int kLaneMinBatchLoop = 28672;  // fused loops of a small arm: row kernel below, lane kernel from here (M targets/s at 16 384: 39.7 vs 24.1, at 32 768: 42.4 vs 48.2)
constexpr int kLaneMinBatch = 73728;  // plain solves of a small arm: row kernel below, lane kernel from here (plan_launch())
}
using namespace mkh;

// one launch of the workgroup-per-problem kernel: every instance (redo_mask = 0) or the ones a wavefront kernel flagged
static int32_t launch_wide_kernel(MkhProblem* p, const SolveArgs& a, hipStream_t stream, int32_t redo_mask, const TapArgs* dtaps = nullptr) {
  SolveArgs aw = a;
  aw.redo_mask = redo_mask;
  aw.work_counter = p->d_work;        // (redo_mask = 0: the kernel as THE path of a model draws its problems from it)
  int grid = p->wide_grid < a.B ? p->wide_grid : a.B;
  if (grid < 1) grid = 1;
  const int rc = mkh::launch_wide(grid, p->wide_lds, stream, p->d_wide, aw, dtaps, p->convex_pairs);
  if (rc != 0) return fail(MKH_E_HIP, "wide kernel: %s", hipGetErrorString((hipError_t)rc));
  HIP_OK(hipGetLastError());
  return MKH_OK;
}

static int grid_for(const MkhProblem* p, int B) {
  int g = p->model->num_cus * p->blocks_per_cu;
  return B < g ? B : g;
}

// Static rounds of a wavefront kernel's problem distribution (ik_kernel.h): each wavefront first walks `static` problems of its
// XCD's contiguous row range, the rest of the batch goes through the ticket counter.  Static rows share cache lines inside one
// L2 and cost no atomic; the ticket tail evens out what the static part left uneven — QP work varies by ±9 % per problem,
// CUs differ by a few per cent — and that grows with the number of rounds.  Round 1 measured the 1.18-ms kernel of its day
// flat between 4/16 and 14/16 static and took 7/8; on today's kernels (round 5, sweep by sixteenths at 65 536 / 32 768 / 16 384
// G1 instances, the plugin workload and the G1 full example): 21 rounds per wavefront want 6 of them dynamic (0.779 -> 0.752 ms
// on the headline), 10 want 2, 5 want 1, 32 of the two-waves plugin build 6 or more (1.681 -> 1.632 ms).
// `uneven`: resident wavefronts per CU that do not divide by its four SIMDs (ten: 3 + 3 + 2 + 2) — a wavefront that shares its
// SIMD with two others is slower than one that shares it with one, so nearly half of the batch goes through the counter there
// (G1 full example 1.37 -> 1.24 ms).  MKH_DEBUG_STATIC_78=1: the old 7/8 rule; MKH_DEBUG_STATIC_16THS=n: n sixteenths (sweeps).
// Below this many rounds per wavefront the batch is dealt statically as a whole (round 5, kernel ms on G1 config 3, ticket tail /
// one strided share per wavefront: 12 288 instances = 4 rounds 0.186 / 0.177, 16 384 = 5.3 rounds 0.243 / 0.224, 20 480 = 6.7 rounds
// 0.282 / 0.270, 24 576 = 8 rounds 0.321 / 0.335, 32 768 0.409 / 0.422, 65 536 0.754 / 0.827): over a few rounds the work of
// the wavefronts has not drifted apart yet, and a ticket tail only adds its own ragged last round.  Round 1's threshold was 4.
constexpr int kMinRoundsForTickets = 8;
// Smallest batch that takes the four-waves product-form build of the humanoid-size low-rank start where its layout fits (plan_launch).
// Kernel ms on G1 config 3, three-waves twin / four-waves build (docs/HISTORY.md, profiles/r17_batch_ab.txt; medians of three alternating
// rounds): 14 336 instances 0.1566 / 0.1577 (a tie), 16 384 0.1656 / 0.1643 (−0.8 %: inside the parent's own spread), 32 768 0.3057 / 0.2739
// (−10 %), 65 536 0.5707 / 0.5080 (−11 %), 131 072 1.1277 / 0.9882 (−12 %): the switch is where the gain is clear of run-to-run noise.
constexpr long long kW4MinBatch = 32768;
static int static_rounds_for(int per_wave, bool uneven, bool loops = false) {
  static const bool static78 = dbg_env("MKH_DEBUG_STATIC_78") != nullptr;
  static const int dbg_16ths = dbg_env("MKH_DEBUG_STATIC_16THS") ? atoi(dbg_env("MKH_DEBUG_STATIC_16THS")) : -1;
  if (dbg_16ths >= 0 && dbg_16ths <= 16) return (per_wave * dbg_16ths) / 16;
  if (dbg_16ths == 99) return INT32_MAX;                     // (no ticket counter at all: one strided share per wavefront)
  if (static78) return (per_wave * 7) / 8;
  if (uneven) return (per_wave * 9) / 16;
  // (fused loops: a problem is 3 … 40 solves long and the threshold-terminated ones differ by that much — half of the batch
  //  dynamic: converged targets of the headline's loop leg 5.45 -> 5.65 M/s; the fixed-count loops do not care)
  if (loops) return per_wave / 2;
  const int dyn = (3 * per_wave - 2) / 10;
  return per_wave - (dyn < 1 ? 1 : dyn);
}

static int grid_for_variant(const MkhProblem* p, int B, int nt, int lds, bool w3 = false) {
  int wpc = waves_per_cu(nt, lds, w3);
  // diagnostic: cap the resident waves per CU (occupancy experiments, docs/HISTORY.md §7b); never raises it
  static const int dbg = dbg_env("MKH_DEBUG_WAVES_PER_CU") ? atoi(dbg_env("MKH_DEBUG_WAVES_PER_CU")) : 0;
  if (dbg > 0 && dbg < wpc) wpc = dbg;
  int g = p->model->num_cus * wpc;
  return B < g ? B : g;
}

// Experiment builds with -DMKH_CLOCKS (tools/phase_clocks.py): MKH_DEBUG_CLOCKS=<file> makes every launch of this process
// synchronous and writes its (B, 24) cycle stamps to <file> — phase profile of kernels that cannot be tapped
static const char* clk_path() { static const char* const s = dbg_env("MKH_DEBUG_CLOCKS"); return s; }
static hipError_t clk_begin(MkhProblem* p, SolveArgs& a, hipStream_t stream) {
  if (!clk_path()) return hipSuccess;
  if (!p->d_clk)
    if (hipError_t e = hipMalloc((void**)&p->d_clk, (size_t)p->max_batch * 24 * sizeof(long long))) return e;
  a.clk = p->d_clk;
  if (hipError_t e = hipMemsetAsync(p->d_clk, 0, (size_t)a.B * 24 * sizeof(long long), stream)) return e;
  // MKH_DEBUG_PHASE_STOP=k (tools/phase_census.sh): slot 15 of every row = the phase boundary after which the kernel abandons the solve
  static const int stop = dbg_env("MKH_DEBUG_PHASE_STOP") ? atoi(dbg_env("MKH_DEBUG_PHASE_STOP")) : 0;
  if (stop) {
    std::vector<long long> h((size_t)a.B, (long long)stop);
    if (hipError_t e = hipMemcpy2DAsync(p->d_clk + 15, 24 * sizeof(long long), h.data(), sizeof(long long), sizeof(long long), (size_t)a.B,
                                        hipMemcpyHostToDevice, stream)) return e;
    return hipStreamSynchronize(stream);
  }
  return hipSuccess;
}
static hipError_t clk_end(MkhProblem* p, int B, hipStream_t stream) {
  if (!clk_path()) return hipSuccess;
  std::vector<long long> h((size_t)B * 24);
  if (hipError_t e = hipMemcpyAsync(h.data(), p->d_clk, h.size() * sizeof(long long), hipMemcpyDeviceToHost, stream)) return e;
  if (hipError_t e = hipStreamSynchronize(stream)) return e;
  if (FILE* f = fopen(clk_path(), "wb")) { fwrite(h.data(), sizeof(long long), h.size(), f); fclose(f); }
  return hipSuccess;
}

// ---- launch planning: what a call runs (kernel family, build, grid, LDS bytes, ticket share), decided apart from running it
enum class Family { WideOnly, Row, Lane, Wave };
struct WaveLaunch {                // one launch of an ik_solve_kernel build
  int nt = 0, nr = 0, feat = 0;
  bool w3 = false, one_shot = false, w4 = false;
  int grid = 0, lds = 0, static_rounds = INT32_MAX;
  const VariantRow* v = nullptr;   // its row of the table (variants.h); null: not compiled — launch() reports it
};
struct LaunchPlan {
  Family family = Family::Wave;
  bool loop = false;               // row / lane kernels: the fused caller loop (steps / until) build
  WaveLaunch main;                 // wavefront family: the launch on the handle's descriptor ...
  WaveLaunch tight;                // ... and, when has_tight, the tight-rows launch in front of it (p->d_dev_tight)
  bool has_tight = false, tight_redo = false;   // tight_redo: `main` follows as the redo launch of what `tight` flagged
  bool cv_split = false;           // convex_contacts_kernel in front of the analytic collision build
  bool wide_redo = false;          // the workgroup-per-problem kernel behind, on the flagged instances
  bool keep_q = false;             // ... which then needs the call's q as it came (q_out aliases it)
  char last_kernel[64] = "";       // what mkh_problem_last_kernel / mkh_problem_launch_info report after the call
  int last_grid = 0, last_lds = 0, last_nt = 0, last_block = kWave;
};

static void plan_name(LaunchPlan& L, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(L.last_kernel, sizeof L.last_kernel, fmt, ap);
  va_end(ap);
}
static const char* wave_name(const WaveLaunch& w) { return w.v ? w.v->kernel : "(not compiled)"; }

// Fills the plan of one call.  Calls nothing of HIP and writes nothing to the handle: launch() below executes it.
// (`taps`: the host copy of the call's tap pointers, or null)
static int32_t plan_launch(const MkhProblem& P_, const SolveArgs& a, const TapArgs* taps, int32_t flags, LaunchPlan& L) {
  const MkhProblem* p = &P_;
  if (p->wide_only) {
    if (taps && taps->t_cycles)
      return fail(MKH_E_INVALID, "models beyond one wavefront (more than 64 bodies or dofs) run on the workgroup-per-problem kernel, "
                                 "which has no cycle-counter tap");
    L.family = Family::WideOnly;
    plan_name(L, "ik_wide_kernel");
    L.last_grid = p->wide_grid < a.B ? p->wide_grid : a.B; L.last_lds = p->wide_lds; L.last_nt = p->wide.nv + p->wide.max_rows;
    L.last_block = kWideThreads;
    return MKH_OK;
  }
  // Small arms (nv ≤ 8, hinge / slide joints, box limits) have two kernels of their own (plain solves without taps):
  //   * a 16-lane ROW per problem (quad_kernel.h): four problems per wavefront, so 4 096 problems put one wavefront on
  //     every SIMD and each problem still spreads its phases over its lanes.  Its fused loop below
  //     kLaneMinBatchLoop instances (threshold-terminated UR5e loop at 4 096: 22.4 M targets/s against 8.4 on the
  //     wavefront kernel and 6.0 on the lane kernel);
  //   * one LANE per problem (lane_kernel.h): 64 problems per wavefront with every lane busy, one ≈48 µs dependent
  //     instruction stream per problem whatever the batch — the best use of the machine once every SIMD has several
  //     wavefronts to interleave.  Also the fused caller loop (steps / until) from kLaneMinBatchLoop instances.
  // Measured on MI355X, UR5e config 2, M solves/s (tools/bench_small_arm.py; wavefront / row / lane kernel):
  //   B = 256: 12 / 25 / 7.6    4 096: 119 / 219 / 90    8 192: 130 / 449 / 152    32 768: 150 / 839 / 528
  //   65 536: 155 / 900 / 855    131 072: 158 / 1 169 / 1 609    1 048 576: 160 / 1 331 / 3 510
  // — the row kernel up to kLaneMinBatch, the lane kernel beyond.
  // MKH_FLAG_WAVE_KERNEL / _QUAD_KERNEL / _LANE_KERNEL force one of the three (parity switches).
  const bool small_ok = !taps && a.do_qp && !(flags & MKH_FLAG_WAVE_KERNEL);
  const bool small_arm = p->lane_nv && small_ok;                               // (nv ≤ 8: both kernels)
  const bool loop = a.n_steps > 1 || a.q_out || a.pos_threshold >= 0.0;       // fused caller loop (steps / until)
  L.loop = loop;
  // (9 … 16 dofs — hands, mobile arms: the row kernel with sixteen column registers, whatever the batch; there is no lane
  //  kernel of that size to hand over to)
  // (MKH_FLAG_WARM_START: the row kernel keeps its partition in the handle's warm-start buffer like the wavefront kernels)
  // (17 … 32 dofs or links, floating bases — H1, Go1, Spot, Allegro: the row kernel on TWO DPP rows per problem, two problems per
  //  wavefront; its fused loop carries the floating base's quaternion from step to step.  Fused loops, kernel ms two-row against
  //  wavefront kernel, 10 fixed steps / threshold loop, 4 096 … 65 536 instances (tools/bench_two_row_loop.py,
  //  profiles/r07_two_row_loop.txt): H1 with its ComTask 3.2 … 3.7x faster, H1 with RelativeFrameTasks 2.4 … 3.0x (the
  //  wavefront kernel needs its all-feature build for both), the Shadow hand without contacts 1.10 … 1.21x; a floating base under frame / posture tasks alone runs the
  //  wavefront kernel's low-rank loop build faster — H1 0.87 … 0.95x, Go1 0.82 … 1.06x — and stays there.
  //  MKH_FLAG_QUAD_KERNEL forces the two-row loop where it can run: not for a free joint that is no link, see quad_loop_ok.)
  const bool two_row_loop_slower = p->quad_nt == 32 && loop && p->dev.nq != p->dev.nv && !p->has_relative && p->dev.n_com == 0 &&
                                   !(flags & MKH_FLAG_QUAD_KERNEL);
  const bool two_row_loop_bad = p->quad_nt == 32 && loop && !p->quad_loop_ok;
  if (p->quad_nt && small_ok && !two_row_loop_slower && !two_row_loop_bad && !((flags & MKH_FLAG_LANE_KERNEL) && p->lane_nv) &&
      (!p->lane_nv || a.B < (loop ? mkh::kLaneMinBatchLoop : mkh::kLaneMinBatch) || (flags & MKH_FLAG_QUAD_KERNEL))) {
    L.family = Family::Row;
    const int per_wave = p->quad_nt == 32 ? 2 : 4;
    L.last_grid = (a.B + per_wave - 1) / per_wave; L.last_nt = p->quad_nt;   // (last_lds: what launch_quad returns)
    plan_name(L, p->quad_nt == 8 ? (loop ? "ik_quad_kernel_loop" : "ik_quad_kernel")
                                 : (p->quad_nt == 32 ? (loop ? "ik_quad_kernel_32_loop" : "ik_quad_kernel_32")
                                                     : (loop ? "ik_quad_kernel_16_loop" : "ik_quad_kernel_16")));
    return MKH_OK;
  }
  if (small_arm && (a.B >= (loop ? mkh::kLaneMinBatchLoop : mkh::kLaneMinBatch) || (flags & MKH_FLAG_LANE_KERNEL))) {
    L.family = Family::Lane;
    L.last_grid = (a.B + kWave - 1) / kWave; L.last_lds = p->lane_lds; L.last_nt = p->lane_nv;
    plan_name(L, loop ? "ik_lane_kernel_%d_loop" : "ik_lane_kernel_%d", p->lane_nv);
    return MKH_OK;
  }
  // A problem whose rows can outnumber the tableau's: the flagged instances once more, with every row — plain solves, calls
  // with taps (the workgroup-per-problem kernel writes every tap but the cycle counters) and, round 5, the fused loops: an
  // instance that overflows at some step runs its whole loop again from its ORIGINAL q, of which the handle keeps a copy for
  // the duration of the call (q_out may alias q) — a device-to-device copy of B·nq doubles in front of the launch
  L.wide_redo = p->d_wide && a.do_qp && a.status_out && !(taps && taps->t_cycles);
  // (only when q_out really aliases q: otherwise the redo reads the caller's q, which the first launch did not touch — the copy
  //  was a latency cost of every small-batch control loop with collision limits, round-5 advisor finding)
  L.keep_q = L.wide_redo && a.q_out && a.q_out == a.q;
  // lean production variant unless the call needs a feature it leaves out
  int need = 0;
  if (taps) need |= F_TAPS;
  if (p->has_relative) need |= F_REL;
  if (p->dev.n_com > 0) need |= F_COM;
  if (p->dev.n_pairs > 0) need |= F_COLL;
  if (loop) need |= F_STEPS;
  const bool dense = p->dev.n_dense_rows > 0 || p->dev.n_dense_limit_rows > 0 || p->dev.dense_box;
  if (dense) need |= 64;                                              // plugin rows: only the all-feature variants have them
  // (general convex pairs of a plain solve: their contacts come from convex_contacts_kernel, launched in front of the
  //  ANALYTIC build — round 5; without the pre-pass buffers, the build with the routine inside)
  // Measured (ur5e_convex, one cylinder–box pair; in-kernel routine / split): 4 096 instances 0.165 / 0.207 ms, 16 384 0.463 / 0.505,
  // 65 536 1.270 / 0.970: GJK is one long dependent chain per lane — in front of a small batch its latency adds to the solve's, on
  // a large one 64 busy lanes per wavefront beat one busy lane per problem.  The split from 32 768 (instance, pair) items on.
  const bool cv_split = need == F_COLL && p->convex_pairs && p->d_cv != nullptr && (long long)a.B * p->cv.n_cv >= 32768;
  L.cv_split = cv_split;
  int feat;
  if (need == 0) feat = 0;
  else if (need == 64) feat = F_DENSE;                                // plugin rows next to frame / posture tasks and box limits: lean build
  else if (need == F_STEPS) feat = F_STEPS;
  else if (need == F_COLL) feat = p->simple_pairs ? (F_COLL | F_SIMPLE_COLL) : ((p->convex_pairs && !cv_split) ? (F_COLL | F_CONVEX_COLL) : F_COLL);
  // (fused loops over capsule-only collision sets — the Shadow hand's closed loop — have a build of their own: the
  //  all-feature one spills 534 VGPRs at this tableau size)
  else if (need == (F_COLL | F_STEPS) && p->simple_pairs) feat = F_COLL | F_SIMPLE_COLL | F_STEPS;
  else if ((need & ~(F_REL | F_COM)) == 0) feat = F_REL | F_COM;      // box limits only: keeps the block-pivoting active set
  else feat = (need & F_TAPS) ? F_ALL : (F_ALL & ~F_TAPS);
  const bool rich = (feat & (F_ALL & ~F_STEPS)) != 0;
  int nt = rich ? p->nt_full : p->nt, nr = 0, lds = rich ? p->lds_bytes_full : p->lds_bytes;
  // Builds whose register-hungry phases are real calls (ik_kernel.h MKH_CALLS: FEAT 8 / 136 / 30) do not need the 256-register
  // map of a 32-row tableau for the compiler's sake: a small arm keeps a small tableau (UR5e + 2 collision rows: phase 0 on
  // 32 rows was a third of the solve) — at least `calls_nt_min` rows, so that the callees still find a usable register file
  // Measured (UR5e + 2 collision rows, 4 096 instances): analytic pairs 0.060 ms on 32 rows, 0.049 on 16 and on 8; with a
  // cylinder–box pair on the general convex routine (round 4: simplex in LDS, 143 VGPRs) 0.186 ms on 32 rows, 0.156 on 16
  // and on 24 — round 3's register-resident GJK (196 VGPRs) wanted the 2-waves file and kept 32 rows.
  static const int dbg_min = dbg_env("MKH_DEBUG_CALLS_NT") ? atoi(dbg_env("MKH_DEBUG_CALLS_NT")) : 0;
  const int calls_nt_min = dbg_min ? dbg_min : 16;
  const bool calls = feat == F_COLL || feat == (F_ALL & ~F_TAPS) || feat == (F_COLL | F_CONVEX_COLL);
  if (calls && p->nt < 32) {
    // (the smallest compiled size that holds the problem and the minimum, up to the 32 rows of nt_full)
    const int v = size_class(p->nt > calls_nt_min ? p->nt : calls_nt_min, feat);
    if (v && v <= nt) nt = v;
    lds = nt == p->nt ? p->lds_bytes : lds_bytes_of(p->dev, nt, 0, kDirectFeat, false);
  }
  // Low-rank start when the problem qualifies and the diagonal part of H is not tiny against JwᵀJw
  // (error amplification of the quasi-definite elimination ≈ eps·max cost²/min Dg ≤ 1e-9).
  const double dg_min = a.damping + p->wood_min_diag;
  // (taps: only the cycle counters / pivot counts exist in the low-rank variant — profiling)
  const bool prof_only = taps && !taps->t_xpos && !taps->t_xquat && !taps->t_frame_pose && !taps->t_subtree_com &&
                         !taps->t_task_e && !taps->t_task_J && !taps->t_H && !taps->t_c && !taps->t_box_lo &&
                         !taps->t_box_hi && !taps->t_coll_G && !taps->t_coll_h;
  if (p->wood_nt && ((need & ~(F_STEPS | F_COM)) == 0 || (need == F_TAPS && prof_only)) && a.do_qp &&
      !(flags & MKH_FLAG_DIRECT_QP) && dg_min > 0.0 && dg_min >= 1e-7 * p->wood_max_cost2 &&
      !((need & F_TAPS) && ((need & F_COM) || p->wood_big))) {   // (no profiling build of the F_COM low-rank start: direct variant)
    nt = p->wood_nt; nr = p->wood_nr; lds = p->wood_lds_bytes;
    feat = F_WOOD | (need & (F_STEPS | F_TAPS | F_COM)) | (p->wood_big ? F_COM : 0);
  }
  // ... and, round 6, with half-space rows (`48_40_r48`: analytic collision pairs; mkh_problem_create "low-rank start WITH half-space
  // rows"): the launch that does the work of a plain collision solve — the tight-rows one where it exists, else the main one
  const bool woodr_ok = a.do_qp && !taps && feat == F_COLL && !(flags & MKH_FLAG_DIRECT_QP) && dg_min > 0.0 && dg_min >= 1e-7 * p->wood_max_cost2;
  if (woodr_ok && p->woodr_lds && !p->d_dev_tight && nt == 48) { nr = 48; lds = p->woodr_lds; feat = F_WOOD | F_COLL; }
  // three resident waves per SIMD where a variant exists (FrameTask / PostureTask / RelativeFrameTask / ComTask, box limits) and
  // the handle found its LDS layout worth it (mkh_problem_create: lds_bytes_w3 / wood_lds_bytes_w3)
  const int w3_lds = nr ? p->wood_lds_bytes_w3 : p->lds_bytes_w3;
  const bool w3 = w3_lds && !(flags & MKH_FLAG_TWO_WAVES) && find_variant(nt, nr, feat, true);
  if (w3) lds = w3_lds;
  // tight rows first (see mkh_problem_create): plain solves on the capsule-only collision build whose caller takes the status
  const bool tight = p->d_dev_tight && (feat == (F_COLL | F_SIMPLE_COLL) || feat == F_COLL) && !nr && !w3 && a.do_qp && a.status_out && !taps &&
                     !(flags & MKH_FLAG_FULL_ROWS);
  const int num_cus = p->model->num_cus;
  if (tight) {
    // (the tight launch itself on the low-rank start: same descriptor, its own LDS layout)
    const bool tight_wood = woodr_ok && p->woodr_lds_tight != 0;
    WaveLaunch& t = L.tight;
    L.has_tight = true;
    L.tight_redo = !(p->diag & MKH_DIAG_NO_TIGHT_REDO);            // (tests: what the tight launch alone leaves flagged)
    t.nt = p->nt_tight; t.nr = tight_wood ? 48 : 0; t.feat = tight_wood ? (feat | F_WOOD) : feat;
    t.lds = tight_wood ? p->woodr_lds_tight : p->lds_tight;
    t.grid = grid_for_variant(p, a.B, t.nt, t.lds, false);
    const int pw = a.B / t.grid;
    if (L.tight_redo && pw >= kMinRoundsForTickets)
      t.static_rounds = static_rounds_for(pw, t.grid % num_cus == 0 && ((t.grid / num_cus) & 3) != 0);
    t.v = find_variant(t.nt, t.nr, t.feat);
  }
  int grid = grid_for_variant(p, a.B, nt, lds, w3);
  // One problem per workgroup instead of persistent wavefronts, for the humanoid-size builds of the one-more-wave map between
  // 3.5 and 22 rounds (round 5): the hardware's workgroup dispatcher is a ticket counter that costs nothing, and a workgroup of
  // these builds starts cheaply (the phases that need registers are callees).  Kernel ms on G1 config 3, persistent /
  // one per workgroup: 12 288 instances 0.176 / 0.163, 16 384 0.224 / 0.209, 24 576 0.323 / 0.301, 32 768 0.411 / 0.390,
  // 49 152 0.588 / 0.572, 65 536 0.751 / 0.743; outside the range it loses (8 192: 0.111 / 0.117, 131 072: 1.414 / 1.424), and so
  // it does on every two-waves build (plugin workload 1.627 / 1.689, Shadow at 65 536 instances 1.186 / 1.226) and on the G1 full
  // example's 25.6 rounds (1.244 / 1.265; at 16 384 instances 0.392 / 0.349).  Two, three, four problems per workgroup lie
  // between the two shapes (65 536: 0.739 / 0.772 / 0.766).  The XCD still owns one contiguous row range
  // (workgroup g: XCD g % 8, row g / 8 of its range).  MKH_DEBUG_PERSISTENT=1: persistent wavefronts everywhere (A/B).
  static const bool persistent_only = dbg_env("MKH_DEBUG_PERSISTENT") != nullptr;
  // (fused loops, measured: no difference — 13.55 / 13.58 ms for the headline's 20-step loop, converged targets 5.64 / 5.58 M/s — they stay persistent)
  // Round 6: where the build has a twin compiled for this shape (`44_32_r44_w3o`, below) there is no upper end — kernel ms, persistent /
  // one per workgroup on the twin: 12 288 instances 0.166 / 0.151, 65 536 0.737 / 0.701, 73 728 0.817 / 0.786, 131 072 1.400 / 1.379,
  // 262 144 2.750 / 2.728 (below 3.5 rounds the persistent shape stays: 10 240 instances 0.145 on both).
  static const int os_max = dbg_env("MKH_DEBUG_ONE_SHOT_MAX") ? atoi(dbg_env("MKH_DEBUG_ONE_SHOT_MAX")) : 22;    // (A/B switch: upper end of the range, in rounds)
  const bool has_twin = w3 && !taps && find_variant(nt, nr, feat, true, true);
  if (!persistent_only && !tight && w3 && nt == 44 && a.n_steps <= 1 && a.B > grid && 2 * (long long)a.B >= 7LL * grid &&
      (has_twin || a.B <= (long long)os_max * grid))
    grid = a.B;
  // ... and, round 6, on a build WITHOUT the persistent loop's machinery where one exists (`44_32_r44_w3o`: build.py W3_WOOD_ONE_SHOT,
  // ik_kernel.h MKH_ONE_SHOT — 78 → 32 spilled SGPRs in the kernel body, headline 0.713 → 0.703 ms; the F_COM twin measured no gain)
  const bool one_shot = grid == a.B && has_twin;
  // ... and, round 17, on FOUR waves per SIMD where the handle's layout fits (`44_32_r44_w4o`, mkh_problem_create: wood_lds_bytes_w4):
  // from 3.5 rounds of ITS resident wavefronts (16 per CU: 4 096 on 256 CUs, so 14 336 instances) and from the batch size at which
  // it measured clearly faster (kW4MinBatch; MKH_DEBUG_W4_MIN_BATCH=n moves the switch for A/B sweeps, a huge n turns the build off).
  static const long long w4_min = dbg_env("MKH_DEBUG_W4_MIN_BATCH") ? atoll(dbg_env("MKH_DEBUG_W4_MIN_BATCH")) : kW4MinBatch;
  const bool w4 = one_shot && nt == 44 && nr == 44 && feat == F_WOOD && p->wood_lds_bytes_w4 != 0 && a.B >= w4_min &&
                  2 * (long long)a.B >= 7LL * 16 * num_cus && find_variant(nt, nr, feat, true, true, true);
  if (w4) lds = p->wood_lds_bytes_w4;
  // Distribution (ik_kernel.h): most of each wave's share is static — one contiguous row range per XCD — and the tail
  // of the batch goes through the ticket counter (how much: static_rounds_for above).  Round 1, on G1 (kernel ms by static
  // sixteenths): 16 → 1.283, 15 → 1.233, 14 → 1.183, 12 → 1.185, 8 → 1.193, 4 → 1.195, 0 → 1.264: every wave opening with an
  // atomic costs more than the balance returns.  Short problems (the 8-row variants) and thin batches stay static.
  const int per_wave = a.B / grid;
  // (fused loops: problems of very different length — the ticket tail from four rounds on, as before)
  const bool dynamic = nt > 8 && per_wave >= (a.n_steps > 1 ? 4 : kMinRoundsForTickets) && !tight;   // (a redo launch walks its static share, ik_kernel.h)
  WaveLaunch& w = L.main;
  w.nt = nt; w.nr = nr; w.feat = feat; w.w3 = w3; w.one_shot = one_shot; w.w4 = w4; w.grid = grid; w.lds = lds;
  if (dynamic) w.static_rounds = static_rounds_for(per_wave, grid % num_cus == 0 && ((grid / num_cus) & 3) != 0, a.n_steps > 1);
  w.v = find_variant(nt, nr, feat, w3, one_shot, w4);
  // what the call reports: the launch that does the work — the tight one where there is one; "convex_pre+": the pre-pass launch
  // in front, "+redo_<rows>" / "+wide": the launches behind
  const WaveLaunch& rep = tight ? L.tight : L.main;
  L.last_grid = rep.grid; L.last_lds = rep.lds; L.last_nt = rep.nt;
  char redo[16] = "";
  if (tight && L.tight_redo) snprintf(redo, sizeof redo, "+redo_%d", nt);
  if (tight && !L.tight_redo) L.wide_redo = L.keep_q = false;      // (the tight launch alone: nothing behind it)
  plan_name(L, "%s%s%s%s", L.cv_split ? "convex_pre+" : "", wave_name(rep), redo, L.wide_redo ? "+wide" : "");
  return MKH_OK;
}

static int32_t launch_wave(MkhProblem* p, const WaveLaunch& w, const DeviceProblem* d_dev, SolveArgs a, hipStream_t stream, const TapArgs* dtaps) {
  if (!w.v)
    return fail(MKH_E_INVALID, "no kernel variant for %d tableau rows, %d dof rows, features %d%s%s", w.nt, w.nr, w.feat, w.w3 ? ", one more wave" : "",
                w.one_shot ? ", one problem per workgroup" : "");
  a.work_counter = p->d_work;
  a.static_rounds = w.static_rounds;
  w.v->launch(w.grid, w.lds, stream, d_dev, a, dtaps);
  HIP_OK(hipGetLastError());
  return MKH_OK;
}

static int32_t launch(MkhProblem* p, const SolveArgs& a_in, const TapArgs* taps, hipStream_t stream, int32_t flags) {
  // (the kernel choice must not depend on whether the caller wants the status: a call without status_out on a handle with a
  //  tight-rows build keeps it in a buffer of the handle — round-3 advisor finding)
  SolveArgs a = a_in;
  if (!a.status_out && p->d_status_tight && a.do_qp) a.status_out = p->d_status_tight;
  LaunchPlan L;
  if (const int32_t rc = plan_launch(*p, a, taps, flags, L)) return rc;
  memcpy(p->last_kernel, L.last_kernel, sizeof p->last_kernel);
  p->last_grid = L.last_grid; p->last_lds = L.last_lds; p->last_nt = L.last_nt; p->last_block = L.last_block;
  (void)hipGetLastError();          // a stale error of an unrelated earlier runtime call must not be blamed on this launch
  const TapArgs* dtaps = nullptr;
  if (taps) {
    HIP_OK(hipMemcpyAsync(p->d_taps, taps, sizeof(TapArgs), hipMemcpyHostToDevice, stream));
    HIP_OK(hipStreamSynchronize(stream));   // taps are a debug path: keep the host struct's lifetime simple
    dtaps = p->d_taps;
  }
  if (L.family == Family::WideOnly) {
    HIP_OK(clk_begin(p, a, stream));                         // (MKH_DEBUG_CLOCKS=<file>: phase stamps of every problem, tools/wide_phase_clocks.py)
    const int32_t rcw = launch_wide_kernel(p, a, stream, 0, dtaps);
    if (rcw == MKH_OK) HIP_OK(clk_end(p, a.B, stream));
    return rcw;
  }
  if (L.family == Family::Row) {
    HIP_OK(clk_begin(p, a, stream));
    p->last_lds = mkh::launch_quad(p->quad_nt, L.loop, L.last_grid, stream, p->d_lane, p->lane_dims, a);
    HIP_OK(hipGetLastError());
    HIP_OK(clk_end(p, a.B, stream));
    return MKH_OK;
  }
  if (L.family == Family::Lane) {
    if (mkh::launch_lane(p->lane_nv, L.loop, L.last_grid, p->lane_lds, stream, p->d_lane, a) != 0)
      return fail(MKH_E_INVALID, "no kernel variant %s", p->last_kernel);
    HIP_OK(hipGetLastError());
    return MKH_OK;
  }
  const double* q_redo = a.q;
  if (L.keep_q) {
    HIP_OK(p->stage[SS_QKEEP].need((size_t)p->max_batch * p->dev.nq * sizeof(double)));
    HIP_OK(hipMemcpyAsync(p->stage[SS_QKEEP].p, a.q, (size_t)a.B * p->dev.nq * sizeof(double), hipMemcpyDefault, stream));
    q_redo = p->stage[SS_QKEEP].f64();
  }
  SolveArgs al = a;
  HIP_OK(clk_begin(p, al, stream));                          // (clock builds: the stamps of the launch that does the work)
  if (L.has_tight) {
    if (const int32_t rc = launch_wave(p, L.tight, p->d_dev_tight, al, stream, nullptr)) return rc;
    if (!L.tight_redo) return MKH_OK;
    al = a;
    al.redo_mask = MKH_ST_ROW_OVERFLOW;              // the full-row build: only what the tight launch flagged
  }
  if (L.cv_split) {
    const hipError_t rc = mkh::launch_convex_pre(stream, p->d_wide, p->cv, a.B, a.q, p->d_cv);
    if (rc != hipSuccess) return fail(MKH_E_HIP, "convex pre-pass: %s", hipGetErrorString(rc));
  }
  if (const int32_t rc = launch_wave(p, L.main, p->d_dev, al, stream, dtaps)) return rc;
  HIP_OK(clk_end(p, a.B, stream));
  if (L.wide_redo) {
    SolveArgs ar = a;
    ar.q = q_redo;
    HIP_OK(clk_begin(p, ar, stream));                      // (MKH_DEBUG_CLOCKS: the stamps of the redo launch overwrite the main kernel's)
    // (… and the instances whose active rows the sweep tableau found almost dependent, or on which it failed: MKH_ST_DEGENERATE is
    //  internal — the dense Goldfarb–Idnani iteration of the workgroup-per-problem kernel answers for them)
    const int32_t rcr = launch_wide_kernel(p, ar, stream, MKH_ST_ROW_OVERFLOW | MKH_ST_INFEASIBLE | MKH_ST_ITER_LIMIT | 32, dtaps);
    if (rcr == MKH_OK) HIP_OK(clk_end(p, a.B, stream));
    return rcr;
  }
  return MKH_OK;
}

// ---- the call's arrays on their way to the kernel and back (solve_plan.h: the table, the route, the pinned layout)
static SolveShape shape_of(const MkhProblem* p) {
  const DeviceProblem& P = p->dev;
  return {P.nq, P.nv, P.nbody, P.n_frame, P.n_posture, P.n_com, P.n_rows_tap, P.n_pairs,
          P.n_dense_rows, P.n_dense_limit_rows, P.dense_box != 0, p->max_batch};
}

// A served call on its way: the caller's pointers by table row, and the kernel's arguments but for its arrays.
struct SolveRun {
  const SolveCall& c;
  SolveShape s;
  SolveWants w;
  hipStream_t stream;
  SolveArgs a;
  void* user[A_COUNT];
  SolveArrayRow row(int i) const { return solve_array(s, w, i); }
  // where row i goes back to in a host caller's memory (NULL: nowhere)
  void* back(int i) const { return row(i).back ? (i == A_Q ? (void*)c.q_out : user[i]) : nullptr; }
};
static_assert(sizeof(TapArgs) == kNumTaps * sizeof(void*), "one table row per pointer of TapArgs, in MkhTaps' order");

static void user_arrays(const SolveCall& c, void* u[A_COUNT]) {
  memset(u, 0, A_COUNT * sizeof(void*));
  u[A_Q] = (void*)c.q; u[A_FT] = (void*)c.frame_targets; u[A_PT] = (void*)c.posture_target; u[A_CT] = (void*)c.com_target;
  u[A_V] = c.v_out; u[A_STATUS] = c.status_out; u[A_ITERS] = c.iters_out; u[A_CONV] = c.converged_out;
  if (c.dense) memcpy(u + A_DE, c.dense, sizeof *c.dense);
  if (c.taps) memcpy(u + A_TAP0, c.taps, sizeof *c.taps);
}
static SolveWants wants_of(const SolveCall& c, void* const u[A_COUNT]) {
  SolveWants w{c.B, c.n_steps, (c.flags & MKH_FLAG_POSTURE_BATCHED) != 0, (c.flags & MKH_FLAG_COM_BATCHED) != 0,
               (c.flags & MKH_FLAG_DEVICE_PTRS) != 0, (c.flags & MKH_FLAG_UNWIND_TURNS) != 0, c.pos_threshold >= 0.0,
               c.q_out != nullptr, c.taps != nullptr, c.dense != nullptr, 0};
  for (int i = 0; i < A_COUNT; ++i)
    if (u[i]) w.given |= 1u << i;
  return w;
}

// The kernel's arrays: row i of the table at dev[i]; q_out is the caller's own array or q's, in place.  Returns the host copy of
// the call's taps, or null.
static const TapArgs* bind(const SolveRun& r, void* const dev[A_COUNT], void* q_out, SolveArgs& a, TapArgs& t) {
  a.q = (const double*)dev[A_Q]; a.frame_targets = (const double*)dev[A_FT];
  a.posture_target = (const double*)dev[A_PT]; a.com_target = (const double*)dev[A_CT];
  a.v_out = (double*)dev[A_V]; a.status_out = (int32_t*)dev[A_STATUS]; a.q_out = (double*)q_out;
  a.iters_out = (int32_t*)dev[A_ITERS]; a.converged_out = (int32_t*)dev[A_CONV];
  a.dense_e = (const double*)dev[A_DE]; a.dense_J = (const double*)dev[A_DJ]; a.dense_G = (const double*)dev[A_DG];
  a.dense_h = (const double*)dev[A_DH]; a.dense_lo = (const double*)dev[A_DLO]; a.dense_hi = (const double*)dev[A_DHI];
  memcpy(&t, dev + A_TAP0, sizeof t);
  return r.c.taps ? &t : nullptr;
}

// Device pointers: straight in, asynchronous on the caller's stream.
static int32_t via_device(SolveRun& r) {
  TapArgs t;
  const TapArgs* const taps = bind(r, r.user, r.c.q_out, r.a, t);
  // (of the table's zero-first taps this route has always cleared coll_G alone — the host routes clear all six; a device caller's
  //  other taps are written as they come)
  if (t.t_coll_G) HIP_OK(hipMemsetAsync(t.t_coll_G, 0, r.row(A_TAP_COLL_G).bytes((size_t)r.c.B), r.stream));
  return launch(r.c.p, r.a, taps, r.stream, r.c.flags);
}

// Host pointers, small call: everything through the pinned scratch (see PinnedScratch) — inputs, outputs and taps.
static int32_t via_pinned(SolveRun& r) {
  MkhProblem* const p = r.c.p;
  HIP_OK(p->small.ensure());
  char* const h = p->small.host;
  char* const d = p->small.dev;
  const size_t B = (size_t)r.c.B;
  const PinnedLayout L = pinned_layout(r.s, r.w);
  void* dev[A_COUNT] = {};
  for (int i = 0; i < A_COUNT; ++i) {
    const SolveArrayRow row = r.row(i);
    if (!row.live) continue;
    if (row.dir != SD_OUT) memcpy(h + L.off[i], r.user[i], row.bytes(B));
    else if (row.zero) memset(h + L.off[i], 0, row.bytes(B));
    dev[i] = d + L.off[i];
  }
  TapArgs t;
  const TapArgs* const taps = bind(r, dev, r.c.q_out ? dev[A_Q] : nullptr, r.a, t);
  const int32_t rc = launch(p, r.a, taps, r.stream, r.c.flags);
  if (rc != MKH_OK) return rc;
  HIP_OK(hipStreamSynchronize(r.stream));
  for (int k = 0; k < A_COUNT; ++k) {
    const int i = solve_back_order(k);
    if (void* const dst = r.back(i)) memcpy(dst, h + L.off[i], r.row(i).bytes(B));
  }
  return MKH_OK;
}

// Host pointers: staged through the handle's device buffers, in n_chunks chunks of `chunk` instances (the last takes the rest).
// One chunk is the plain case: copies in, launch, copies out, all on the caller's stream.  More (solve_plan.h solve_route): the
// copies in run on a stream of their own and the copies out on another, beside the kernels of their neighbours.
static int32_t via_staged(SolveRun& r, int n_chunks, size_t chunk) {
  MkhProblem* const p = r.c.p;
  const size_t B = (size_t)r.c.B, mb = (size_t)p->max_batch;
  hipStream_t stream = r.stream;
  const bool chunked = n_chunks > 1;
  void* dev[A_COUNT] = {};
  for (int i = 0; i < A_TAP0; ++i) {
    const SolveArrayRow row = r.row(i);
    // (q, frame targets, v and status are sized for max_batch at the first staged call whatever that call has, as they always
    //  were — every other per-instance slot when a call first has its row; a target slot grows to what a call brings)
    const bool always = i == A_Q || i == A_FT || i == A_V || i == A_STATUS;
    if (!always && !row.live) continue;
    const bool halves = row.slot == SS_ITERS || row.slot == SS_DBOX;
    GrowBuf& g = p->stage[row.slot];
    HIP_OK(g.need((i == A_PT || i == A_CT) ? row.bytes(B) : mb * row.width * (halves ? 2 : 1)));
    dev[i] = (char*)g.p + row.half * mb * row.width;
  }
  if (!r.w.has(A_V)) dev[A_V] = nullptr;
  if (chunked && !p->st_in) {
    HIP_OK(hipStreamCreateWithFlags(&p->st_in, hipStreamNonBlocking));
    HIP_OK(hipStreamCreateWithFlags(&p->st_out, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&p->ev_start, hipEventDisableTiming));
    for (int i = 0; i < 4; ++i) {
      HIP_OK(hipEventCreateWithFlags(&p->ev_in[i], hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&p->ev_k[i], hipEventDisableTiming));
    }
  }
  hipStream_t in = chunked ? p->st_in : stream, out = chunked ? p->st_out : stream;
  int32_t rc = MKH_OK;
  hipError_t e = hipSuccess;
  // (an error below must not return: copies that read or write the caller's arrays may be in flight — the first one is latched,
  //  nothing more is enqueued, and the call drains what it started)
  auto ok = [&](hipError_t x) { if (e == hipSuccess) e = x; return e == hipSuccess; };
  if (chunked) {
    // (shared targets on the caller's stream, ahead of the first kernel; the side streams start behind the caller's work)
    for (int i = A_PT; i <= A_CT; ++i)
      if (r.row(i).live && r.row(i).shared) ok(hipMemcpyAsync(dev[i], r.user[i], r.row(i).width, hipMemcpyHostToDevice, stream));
    ok(hipEventRecord(p->ev_start, stream));
    ok(hipStreamWaitEvent(in, p->ev_start, 0));
  }
  TapArgs t;
  for (int c = 0; c < n_chunks && rc == MKH_OK && e == hipSuccess; ++c) {
    const size_t off = c * chunk, Bc = c + 1 < n_chunks ? chunk : B - off;
    void* cd[A_COUNT] = {};
    for (int i = 0; i < A_TAP0 && e == hipSuccess; ++i) {
      const SolveArrayRow row = r.row(i);
      cd[i] = (dev[i] && !row.shared) ? (char*)dev[i] + off * row.width : dev[i];
      if (row.dir == SD_OUT || !row.live) continue;
      if (!row.shared) ok(hipMemcpyAsync(cd[i], (const char*)r.user[i] + off * row.width, Bc * row.width, hipMemcpyHostToDevice, in));
      else if (!chunked) ok(hipMemcpyAsync(cd[i], r.user[i], row.width, hipMemcpyHostToDevice, stream));
    }
    if (chunked && ok(hipEventRecord(p->ev_in[c], in))) ok(hipStreamWaitEvent(stream, p->ev_in[c], 0));
    // (the taps are a debug path: device buffers of their own for the call, freed below whatever happens next; never in chunks)
    for (int i = A_TAP0; i < A_COUNT && rc == MKH_OK && e == hipSuccess; ++i) {
      const SolveArrayRow row = r.row(i);
      if (!row.live) continue;
      if (hipMalloc(&dev[i], row.bytes(B) ? row.bytes(B) : 1) != hipSuccess) { dev[i] = nullptr; rc = fail(MKH_E_HIP, "tap buffer allocation failed"); }
      else if (row.zero && hipMemsetAsync(dev[i], 0, row.bytes(B), stream) != hipSuccess) rc = fail(MKH_E_HIP, "tap buffer clear failed");
      cd[i] = dev[i];
    }
    if (rc != MKH_OK || e != hipSuccess) break;
    SolveArgs ac = r.a;
    ac.B = (int32_t)Bc;
    const TapArgs* const taps = bind(r, cd, r.c.q_out ? cd[A_Q] : nullptr, ac, t);
    if (r.a.warm) ac.warm = r.a.warm + off * (size_t)r.s.nv;
    rc = launch(p, ac, taps, stream, r.c.flags);
    if (rc == MKH_OK && chunked) ok(hipEventRecord(p->ev_k[c], stream));
  }
  for (int c = 0; c < n_chunks && rc == MKH_OK && e == hipSuccess; ++c) {
    const size_t off = c * chunk, Bc = c + 1 < n_chunks ? chunk : B - off;
    if (chunked) ok(hipStreamWaitEvent(out, p->ev_k[c], 0));
    for (int k = 0; k < A_COUNT && e == hipSuccess; ++k) {
      const int i = solve_back_order(k);
      const size_t w = r.row(i).width;
      if (void* const dst = r.back(i)) ok(hipMemcpyAsync((char*)dst + off * w, (const char*)dev[i] + off * w, Bc * w, hipMemcpyDeviceToHost, out));
    }
  }
  // (a failed call still drains what it started: the staging buffers belong to the handle)
  const hipError_t e1 = chunked ? hipStreamSynchronize(in) : hipSuccess, e2 = hipStreamSynchronize(stream),
                   e3 = chunked ? hipStreamSynchronize(out) : hipSuccess;
  if (e == hipSuccess) e = e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3);
  if (rc == MKH_OK && e != hipSuccess) rc = fail(MKH_E_HIP, "solve: %s", hipGetErrorString(e));
  for (int i = A_TAP0; i < A_COUNT; ++i) (void)hipFree(dev[i]);
  return rc;
}

namespace mkh {
int32_t solve(const SolveCall& c) {
  MkhProblem* const p = c.p;
  if (!p) return fail(MKH_E_INVALID, "null problem");
  SolveRun r{c, shape_of(p), {}, (hipStream_t)c.hip_stream, {}, {}};
  user_arrays(c, r.user);
  r.w = wants_of(c, r.user);
  if (const int32_t rc = solve_refuse(r.s, r.w, c.dt > 0.0, g_err)) return rc;      // (the outer-loop callers clear the unwind bit in front of their loops)
  for (int i = A_DE; i <= A_DHI; ++i)
    if (!r.row(i).live) r.user[i] = nullptr;              // (a dense array of rows the problem does not have: ignored)
  HIP_OK(hipSetDevice(p->model->device));
  SolveArgs& a = r.a;
  memset(&a, 0, sizeof a);
  a.B = c.B; a.posture_batched = r.w.posture_batched; a.com_batched = r.w.com_batched; a.do_qp = (c.v_out != nullptr);
  a.dt = c.dt; a.damping = c.damping; a.n_steps = c.n_steps;
  a.pos_threshold = c.pos_threshold; a.ori_threshold = c.ori_threshold;
  if (c.flags & MKH_FLAG_WARM_START) {
    // closed-loop callers solve the same instances again and again: keep each instance's active set on the device
    const size_t nv = (size_t)p->dev.nv;
    if (!p->d_warm) HIP_OK(hipMalloc((void**)&p->d_warm, (size_t)p->max_batch * nv));
    if (p->warm_B != c.B) { HIP_OK(hipMemsetAsync(p->d_warm, 0, (size_t)p->max_batch * nv, r.stream)); p->warm_B = c.B; p->warm_age = 0; }
    a.warm = p->d_warm; a.warm_age = p->warm_age;
    if (c.v_out) ++p->warm_age;
  }
  static const bool no_chunks = dbg_env("MKH_DEBUG_NO_CHUNKS") != nullptr;      // (A/B of the chunked route)
  const SolveRoutePlan route = solve_route(r.s, r.w, no_chunks);
  switch (route.route) {
    case SolveRoute::Device: return via_device(r);
    case SolveRoute::Pinned: return via_pinned(r);
    default: return via_staged(r, route.n_chunks, route.chunk);
  }
}
}  // namespace mkh

extern "C" {

int32_t mkh_problem_launch_info(const MkhProblem* p, int32_t B, int32_t* grid, int32_t* block, int32_t* lds_bytes,
                                int32_t* tableau_rows) {
  if (!p) return fail(MKH_E_INVALID, "null problem");
  // what the most recent launch of this problem used (the variant depends on the call: taps, fused steps, the
  // low-rank QP start); before any launch, the lean direct variant
  if (grid) *grid = p->wide_only ? (p->wide_grid < B ? p->wide_grid : B) : (p->last_nt ? p->last_grid : grid_for(p, B));
  if (block) *block = p->last_block;        // (64: one wavefront per workgroup; 256 on the workgroup-per-problem kernel)
  if (lds_bytes) *lds_bytes = p->last_nt ? p->last_lds : p->lds_bytes;
  if (tableau_rows) *tableau_rows = p->last_nt ? p->last_nt : p->nt;
  return MKH_OK;
}

int32_t mkh_eval(MkhProblem* p, int32_t B, const double* q, const double* frame_targets, const double* posture_target,
                 const double* com_target, double dt, double damping, double* v_out, int32_t* status_out,
                 const MkhTaps* taps, int32_t flags, void* hip_stream) {
  SolveCall c;
  c.p = p; c.B = B; c.q = q; c.frame_targets = frame_targets; c.posture_target = posture_target; c.com_target = com_target;
  c.dt = dt; c.damping = damping; c.v_out = v_out; c.status_out = status_out; c.flags = flags; c.hip_stream = hip_stream;
  c.taps = taps;
  return solve(c);
}

int32_t mkh_solve(MkhProblem* p, int32_t B, const double* q, const double* frame_targets, const double* posture_target,
                  const double* com_target, double dt, double damping, double* v_out, int32_t* status_out,
                  int32_t flags, void* hip_stream) {
  if (!v_out) return fail(MKH_E_INVALID, "v_out is null");
  SolveCall c;
  c.p = p; c.B = B; c.q = q; c.frame_targets = frame_targets; c.posture_target = posture_target; c.com_target = com_target;
  c.dt = dt; c.damping = damping; c.v_out = v_out; c.status_out = status_out; c.flags = flags; c.hip_stream = hip_stream;
  return solve(c);
}

int32_t mkh_solve_dense(MkhProblem* p, int32_t B, const double* q, const double* frame_targets,
                        const double* posture_target, const double* com_target, const MkhDenseRows* dense, double dt,
                        double damping, double* v_out, int32_t* status_out, const MkhTaps* taps, int32_t flags,
                        void* hip_stream) {
  SolveCall c;
  c.p = p; c.B = B; c.q = q; c.frame_targets = frame_targets; c.posture_target = posture_target; c.com_target = com_target;
  c.dt = dt; c.damping = damping; c.v_out = v_out; c.status_out = status_out; c.flags = flags; c.hip_stream = hip_stream;
  c.taps = taps; c.dense = dense;
  return solve(c);
}

int32_t mkh_solve_steps(MkhProblem* p, int32_t B, const double* q, const double* frame_targets,
                        const double* posture_target, const double* com_target, double dt, double damping,
                        int32_t n_steps, double* q_out, double* v_out, int32_t* status_out, int32_t flags,
                        void* hip_stream) {
  if (!v_out || !q_out) return fail(MKH_E_INVALID, "v_out / q_out is null");
  SolveCall c;
  c.p = p; c.B = B; c.q = q; c.frame_targets = frame_targets; c.posture_target = posture_target; c.com_target = com_target;
  c.dt = dt; c.damping = damping; c.v_out = v_out; c.status_out = status_out; c.flags = flags; c.hip_stream = hip_stream;
  c.n_steps = n_steps; c.q_out = q_out;
  return solve(c);
}

int32_t mkh_solve_until(MkhProblem* p, int32_t B, const double* q, const double* frame_targets,
                        const double* posture_target, const double* com_target, double dt, double damping,
                        int32_t max_iters, double pos_threshold, double ori_threshold, double* q_out, double* v_out,
                        int32_t* status_out, int32_t* iters_out, int32_t* converged_out, int32_t flags, void* hip_stream) {
  if (!v_out || !q_out) return fail(MKH_E_INVALID, "v_out / q_out is null");
  if (!(pos_threshold >= 0.0) || !(ori_threshold >= 0.0)) return fail(MKH_E_INVALID, "thresholds must be >= 0");
  SolveCall c;
  c.p = p; c.B = B; c.q = q; c.frame_targets = frame_targets; c.posture_target = posture_target; c.com_target = com_target;
  c.dt = dt; c.damping = damping; c.v_out = v_out; c.status_out = status_out; c.flags = flags; c.hip_stream = hip_stream;
  c.n_steps = max_iters; c.q_out = q_out; c.pos_threshold = pos_threshold; c.ori_threshold = ori_threshold;
  c.iters_out = iters_out; c.converged_out = converged_out;
  return solve(c);
}

}  // extern "C"
