// What the host translation units of the C ABI share: minkhip.hip (the handles, the outer-loop entry points), solve_host.hip (the
// plain solve: launch planning, launching and the four ways a call's arrays travel) and checker_host.hip (the collision checker's
// calls and stages).  The error string and its one writer, the handles, the workspace and the Stager every outer-loop call stages
// through — and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/minkhip.h"
#include "convex_chain.h"
#include "problem_plan.h"
#include "solve_plan.h"

// Experiment switches (A/B runs, sweeps, phase censuses): environment variables MKH_DEBUG_* that change kernel selection, launch
// shapes or caps.  They exist only in builds made with -DMKH_DEBUG_SWITCHES (MKH_EXTRA_FLAGS=-DMKH_DEBUG_SWITCHES python -m
// mink_amd.csrc.build, normally under an MKH_BUILD_TAG): the product library never reads the environment, so a stray variable
// cannot change a production handle's results or speed (round-5 review).  The four switches the parity tests and bench.py need
// are per-handle diagnostic options of the ABI instead: mkh_problem_create_diag, MKH_DIAG_*.
#if defined(MKH_CLOCKS) && !defined(MKH_DEBUG_SWITCHES)
#define MKH_DEBUG_SWITCHES 1     // (a clock build is an experiment build: MKH_DEBUG_CLOCKS / MKH_DEBUG_PHASE_STOP drive its stamps)
#endif
#ifdef MKH_DEBUG_SWITCHES
static inline const char* dbg_env(const char* name) { return getenv(name); }
#else
static inline const char* dbg_env(const char*) { return nullptr; }
#endif

namespace mkh {
// mkh_last_error's text, per thread, and the one function that formats into it (both defined in minkhip.hip; plan_model,
// plan_problem and checker_refuse write into g_err by reference).  Hidden: the library's own, never another module's `fail`.
__attribute__((visibility("hidden"))) extern thread_local std::string g_err;
__attribute__((visibility("hidden"))) int32_t fail(int32_t code, const char* fmt, ...);
}  // namespace mkh
#define HIP_OK(expr)                                                                                  \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess) return mkh::fail(MKH_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                           __FILE__, __LINE__);                                       \
  } while (0)

// Small host-pointer calls (a control loop's single configuration: the reference's everyday use) go through ONE pinned,
// device-visible host buffer: the kernel reads its inputs and writes its outputs across the bus itself — a launch and a
// synchronize instead of five staged copies of ≈8 µs host time each, whatever their size (mkh::kSmallCallBytes: solve_plan.h).
struct PinnedScratch {
  char* host = nullptr;
  char* dev = nullptr;
  hipError_t ensure() {
    if (host) return hipSuccess;
    if (hipError_t e = hipHostMalloc((void**)&host, mkh::kSmallCallBytes, hipHostMallocDefault)) { host = nullptr; return e; }
    if (hipError_t e = hipHostGetDevicePointer((void**)&dev, host, 0)) { (void)hipHostFree(host); host = nullptr; return e; }
    return hipSuccess;
  }
  void release() { if (host) (void)hipHostFree(host); host = dev = nullptr; }
};

// A device buffer of the outer-loop entry points' workspace (MkhProblem::ws) or of the plain solve's staging (MkhProblem::stage): grown to what a call needs (never beyond what
// max_batch allows), kept for the next call, never shrunk.
struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t need(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    (void)hipFree(p); p = nullptr; cap = 0;
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
    if (e == hipSuccess) cap = bytes; else p = nullptr;
    return e;
  }
  void release() { (void)hipFree(p); p = nullptr; cap = 0; }
  double* f64() const { return (double*)p; }
  int32_t* i32() const { return (int32_t*)p; }
};

// The slots of that workspace, named by what a buffer HOLDS, not by the entry point that asked for it: one call is in flight
// per handle (include/minkhip.h), so mkh_solve_multistart, mkh_solve_trajectory, mkh_solve_keyframes and
// mkh_solve_trajectory_multistart share them.  Two roles that one call needs at the same time are two slots.
enum WsRole {
  // the per-qpos-address seeding table and the joint list (ms_build_tables, at the first call that needs them)
  WS_SEED_I, WS_SEED_F, WS_JNT,
  // inputs of a host-pointer call, staged as they came
  WS_IN_Q, WS_IN_FT, WS_IN_PT, WS_IN_CT, WS_IN_SEEDS, WS_IN_REF, WS_IN_W,
  // the B·S candidate rows: what the loops read and write (time-major (T, B·S, .) for a trajectory; one buffer per array, so
  // that a caller's *_all array replaces its own), the starts, and ONE fanned-out (B·S, .) slab per target group.  Who asks:
  // the entry point asks for the rows it hands to ms_loops (the multi-start calls all of C_Q … C_STARTS; a ladder or a goal set
  // C_Q alone, for one chunk's starts, when the caller wants no seeds_out; the ladder on nodes C_Q … C_CV for one chunk);
  // ms_loops itself asks for C_FT / C_PT / C_CT and, with a seed table, for the IN_SEEDS slab — per chunk, the largest first
  WS_C_Q, WS_C_V, WS_C_ST, WS_C_IT, WS_C_CV, WS_C_STARTS, WS_C_FT, WS_C_PT, WS_C_CT,
  // a batch-major trajectory call: time-major copies of its targets, the loops' time-major results (TM_I32: status | iters |
  // converged)
  WS_TM_FT, WS_TM_PT, WS_TM_CT, WS_TM_Q, WS_TM_V, WS_TM_I32,
  // keyframes: ONE (B, .) slab per target group, rewritten in front of every waypoint's loop
  WS_KF_FT, WS_KF_PT, WS_KF_CT,
  // outputs of a host-pointer call in the caller's layout, until they are copied back (OUT_I32: status | iters | converged
  // per row; OUT_PICK: the per-instance integers of a selection; OUT_LEN: path lengths; OUT_FT / PT / CT: the interpolated
  // targets a keyframed call was asked for — the only buffers of a call's targets that grow with T)
  WS_OUT_Q, WS_OUT_V, WS_OUT_I32, WS_OUT_QVEL, WS_OUT_PICK, WS_OUT_LEN, WS_OUT_FT, WS_OUT_PT, WS_OUT_CT,
  // a ladder: the (B, T, S, .) node rows (one buffer per array, so that a caller's *_all array replaces its own), the tracked
  // flags, the starts a host caller asked for, q fanned out to the (B·T) targets of the multi-start launch, and the search's
  // break masks | back-pointers
  WS_L_Q, WS_L_V, WS_L_ST, WS_L_IT, WS_L_CV, WS_L_TRK, WS_L_STARTS, WS_L_Q0, WS_L_PRED,
  // a ladder refinement: the working path r and the loops' velocities of its repaired nodes, (B, T, .); R_I32: tracked |
  // repaired | status | iters | converged | break bits of r, (B, T) each; what one loop launch reads and writes — R_X: start | x
  // | v, R_XI: status | iters | converged | bad flags, (B, .) each; a host caller's path and flags as they came (IN_PATH,
  // IN_TRK); OUT_REF: tracked_out | repaired (B, T) | refined (B,) of a host-pointer call
  WS_R_Q, WS_R_V, WS_R_I32, WS_R_X, WS_R_XI, WS_IN_PATH, WS_IN_TRK, WS_OUT_REF,
  // a goal set: a host caller's goal_cost and goal_valid, (B, G) each, as they came.  Its (B, G, S, .) candidate rows, its
  // starts and q fanned out to the (B·G) pairs are a ladder's node rows with G for T and live in WS_L_Q … WS_L_Q0; its outputs
  // go through WS_OUT_Q / V (q_best | q_goal), OUT_I32 (iters | status, per target then per goal), OUT_PICK (converged |
  // goal_index | seed_index | n_reached (B,), then seed_index_goal | reached | n_converged_goal (B, G)) and OUT_LEN (score |
  // distance_goal)
  WS_IN_GCOST, WS_IN_GVALID,
  // turn unwinding: the per-qpos-address table (mode, range_lo, range_hi), built with the seeding table
  WS_UNW,
  // a ladder on deduplicated nodes: its (B, T, K, .) node rows live in a plain ladder's WS_L_Q … WS_L_TRK with K for S, the
  // candidates of ONE chunk of rungs in multi-start's WS_C_Q … WS_C_CV, asked for by the call itself.  A host caller's set outputs — N_I32: node_seed_index |
  // node_multiplicity (B, T, K), then n_distinct | n_converged | n_uncovered | seed_index (B, T); N_DIST: node_distance (B, T, K)
  WS_N_I32, WS_N_DIST,
  // swept clearance and the checked ladder calls: a host caller's q_to as it came (q_from goes through WS_C_Q); the nodes'
  // clearance margins (B, T, S) and effective tracked flags; the blocked flag of every edge, (B, T, S, S) bytes; every edge's swept
  // margin when the caller asked for it; a host caller's outputs — F_OUT_I: edge_collision (B, T) | n_edge_collisions (B,), F_OUT_F:
  // edge_margin (B, T).  The certifying ladder calls: F_OUT_I holds edge_verdict | edge_n_samples (B, T) | n_certified (B,) behind
  // those, F_OUT_F edge_lower_bound (B, T) behind edge_margin; F_EVERDICT: every edge's verdict, (B, T, S, S) bytes, when a host
  // caller asked for it
  WS_SW_TO, WS_F_NMARGIN, WS_F_TRK, WS_F_BLOCK, WS_F_EMARGIN, WS_F_OUT_I, WS_F_OUT_F, WS_F_EVERDICT,
  // a ladder refinement with a checker: RF_MARGIN: the node margins and the edge margins of the input path, then of the working
  // path, (B, T) each; RF_TRIP: what lr_check_kernel leaves per step, (B, 3, slots); RF_IDX: the index array of the input path seen as a
  // ladder of width 1 (zeros) | its effective flags, (B, T) each.  A host caller's outputs go through F_OUT_I, F_OUT_F and
  // F_NMARGIN, as a checked ladder's do.  Checked candidate tracking (trajectory_free.hip) has no slot of its own: every row's
  // node and edge margins, (T, B·S) each, live in F_NMARGIN and F_EMARGIN; a host caller's outputs in F_OUT_F (node_margin |
  // edge_margin, (B, T) each) and F_OUT_I (edge_collision (B, T) | n_edge_collisions (B,)); the selection alone keeps the
  // caller's candidates and flags in C_Q and C_CV and its status of zeros in C_ST
  WS_RF_MARGIN, WS_RF_TRIP, WS_RF_IDX,
  WS_COUNT
};

struct MkhModel : mkh::HostModel {     // (the host arrays problems are planned from: problem_plan.h)
  int device = 0;
  PinnedScratch small;             // mkh_integrate, host pointers
  std::mutex small_mutex;          // one model serves many callers (every Configuration of a FlatModel shares it): the small
                                   // host-pointer path of mkh_integrate is serialised, so the entry point stays re-entrant
  double* d_mesh_vert = nullptr;   // hull vertices of the mesh geoms (HostModel::h_mesh_vert)
  // device tables
  double* d_body_f = nullptr;
  int32_t* d_body_i = nullptr;
  double* d_jnt_f = nullptr;
  int32_t* d_jnt_i = nullptr;
  int32_t* d_dof_i = nullptr;
  double* d_dof_f = nullptr;
  int num_cus = 0;
};

// The distances of a checker's general convex pairs on the rows of one chunk of a launch, [rows][n_cv] (checker_host.hip
// cv_rows_resize: the one routine that sizes it).
struct CvRows {
  double* d = nullptr;
  int64_t rows = 0;
};

struct MkhProblem : mkh::ProblemSelect {     // (what creation decided and plan_launch reads: problem_plan.h)
  PinnedScratch small;             // solve(), small host-pointer calls
  MkhModel* model = nullptr;
  int device = 0;                  // (copied: the destructor must not depend on the model still being alive)
  mkh::DeviceProblem dev{};
  int max_batch = 0;
  mkh::DeviceProblem* d_dev_tight = nullptr;   // the tight-rows twin of `dev` (ProblemSelect::nt_tight)
  int32_t* d_status_tight = nullptr;   // status of a call with a redo launch whose caller passed no status_out (the redo launch reads it)
  mkh::WideProblem wide{};
  mkh::WideProblem* d_wide = nullptr;
  // device memory the handle keeps only to free it: what the descriptors point to (frame tasks, cost and limit tables, pairs,
  // the wide kernel's arrays, workspace and redo queue, the convex split's lists)
  std::vector<void*> owned;
  mkh::LaneProblem* d_lane = nullptr;
  char last_kernel[64] = "";
  int32_t diag = 0;                // MKH_DIAG_* of mkh_problem_create_diag (parity / measurement switches of this handle)
  mkh::DeviceProblem* d_dev = nullptr;   // device copy of `dev` (the kernel reads the descriptor from memory)
  mkh::TapArgs* d_taps = nullptr;
  int last_grid = 0, last_lds = 0, last_nt = 0, last_block = mkh::kWave;   // geometry of the most recent launch (mkh_problem_launch_info)
  long long* d_clk = nullptr;      // MKH_DEBUG_CLOCKS (experiment builds): cycle stamps of the last launch
  // general convex pairs of plain solves: evaluated by convex_contacts_kernel in front of the analytic collision build
  mkh::CvPre cv{};
  double* d_cv = nullptr;          // [max_batch][n_cv][7]
  CvRows cv_sweep;                 // a chunk of swept samples (mkh_problem_set_sweep_rows)
  CvRows cv_check;                 // the rows a check judges inside its launch (mkh_problem_set_check_rows)
  // the certified sweep's reach table (motion_bound.h), [n_pairs][njnt][2]: filled from pair_geom and uploaded at the first call
  // that needs it (checker_host.hip ensure_reach), then a constant of the handle
  std::vector<int32_t> pair_geom;  // [n_pairs][2]: the geom ids of the pair list
  std::vector<double> h_reach;
  double* d_reach = nullptr;
  int8_t* d_warm = nullptr;        // MKH_FLAG_WARM_START: active set of every instance after the previous solve (max_batch × nv)
  int warm_age = 0, warm_B = 0;    // solves since the state was reset / the batch size it belongs to
  uint32_t* d_work = nullptr;      // ticket counter of the dynamic problem distribution (zeroed by the kernel's last draw)
  // staging buffers of the plain solve's host-pointer calls, by table row (solve_plan.h SolveSlot; the per-instance ones sized
  // for max_batch at their first use) — apart from ws[]: the outer-loop calls hold WS_IN_* while they run plain solves.  SS_QKEEP:
  // fused loops with a redo launch behind them keep the call's q as it came (q_out may alias it)
  GrowBuf stage[mkh::SS_COUNT];
  // host-pointer calls on large batches: copies of chunk c + 1 / c − 1 run beside the kernel of chunk c
  hipStream_t st_in = nullptr, st_out = nullptr;
  hipEvent_t ev_start = nullptr, ev_in[4] = {nullptr, nullptr, nullptr, nullptr}, ev_k[4] = {nullptr, nullptr, nullptr, nullptr};
  // the outer-loop entry points' workspace, by role (WsRole)
  bool ws_tables = false;
  GrowBuf ws[WS_COUNT];
  const MkhSeedTable* seed_table = nullptr;    // attached by mkh_problem_set_seed_table
  MkhProblem* checker = nullptr;               // attached by mkh_problem_set_collision_check
};

// One outer-loop call's traffic with the workspace and with the caller's arrays.  The first HIP error is latched and everything
// after it is skipped; finish() is the only way out once something is enqueued: a host-pointer call may have copies from or to
// the caller's arrays in flight, so it drains the stream before it returns, whatever happened.
struct Stager {
  MkhProblem* p;
  hipStream_t stream;
  bool devp;                         // MKH_FLAG_DEVICE_PTRS: the caller's arrays are used in place, nothing is staged
  const char* who;                   // the entry point, in messages
  hipError_t err = hipSuccess;
  size_t oom_bytes = 0;              // the size of the allocation that failed, if one did
  size_t cand_bytes = 0;             // a call with candidates: what their results take (the out-of-memory message states it)

  bool ok() const { return err == hipSuccess; }
  void latch(hipError_t e) { if (err == hipSuccess) err = e; }
  // slot `role` grown to `bytes`; NULL when that failed (or an error is latched already)
  void* need(WsRole role, size_t bytes) {
    if (!ok()) return nullptr;
    GrowBuf& g = p->ws[role];
    if ((err = g.need(bytes)) != hipSuccess) { oom_bytes = bytes; return nullptr; }
    return g.p;
  }
  double* f64(WsRole role, size_t n) { return (double*)need(role, n * sizeof(double)); }
  int32_t* i32(WsRole role, size_t n) { return (int32_t*)need(role, n * sizeof(int32_t)); }
  // `n` doubles of a caller's input on the device: `src` itself, or its staged copy in slot `role`
  const double* up(WsRole role, const double* src, size_t n) {
    if (devp || !src) return src;
    double* const d = f64(role, n);
    if (d) latch(hipMemcpyAsync(d, src, n * sizeof(double), hipMemcpyHostToDevice, stream));
    return d;
  }
  const int32_t* up_i32(WsRole role, const int32_t* src, size_t n) {       // (the same for `n` int32)
    if (devp || !src) return src;
    int32_t* const d = i32(role, n);
    if (d) latch(hipMemcpyAsync(d, src, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    return d;
  }
  // rows the loops write: the caller's own array where it is a device buffer, else slot `role`
  void* given_or(WsRole role, void* given, size_t bytes) { return (devp && given) ? given : need(role, bytes); }
  // a result back into a host caller's array (an output the caller did not ask for: dst == NULL)
  void down(void* dst, const void* src, size_t bytes) {
    if (dst && ok()) latch(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
  }
  // the way out: `rc` != MKH_OK is a refusal or failure of a loop launch, whose message stands
  int32_t finish(int32_t rc = MKH_OK) {
    if (devp && ok() && rc == MKH_OK) return MKH_OK;         // (asynchronous on the caller's stream)
    latch(hipStreamSynchronize(stream));                     // (a failed call still drains what it started)
    if (rc != MKH_OK || ok()) return rc;
    if (oom_bytes && cand_bytes)
      return mkh::fail(MKH_E_HIP, "%s: no device memory for a buffer of %zu bytes (the candidates' results take T*B*S*((nq+nv)*8+12) = %zu bytes)",
                       who, oom_bytes, cand_bytes);
    return mkh::fail(MKH_E_HIP, "%s: %s", who, hipGetErrorString(err));
  }
};
// a launcher's hipError_t into the latch; not launched at all behind an earlier error
#define ST_LAUNCH(st, call) do { if ((st).ok()) (st).latch(call); } while (0)
