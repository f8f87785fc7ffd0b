// Launchers of the small kernels around the loop launches of the outer-loop entry points (mkh_solve_multistart,
// mkh_solve_multistart_set, mkh_solve_goalset, mkh_solve_trajectory, mkh_solve_keyframes, mkh_solve_trajectory_multistart, the ladder calls) and of
// the seed tables in front of them: declared once, for the thirteen files that define them and for the two host files that call them
// (minkhip.hip; checker_host.hip: the clearance, sweep and check launchers and their pre-passes) — a signature that
// drifts fails to compile in the file that drifted.  In minkhip.hip the multi-start calls, the ladder calls and the goal set
// launch the seeding, the seed-table query and the target fan-out from one place, the loop stage ms_loops(), which also asks for
// their workspace slots (WS_C_FT / PT / CT, the WS_IN_SEEDS slab); mkh_solve_trajectory_multistart has its own (time-major) ones.
// Every other launcher below is called by the entry point that asked for the slots it reads and writes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace mkh {

struct CvPre;                      // a checker's lists of general convex pairs (convex_chain.h)

// What launch_tmf_check / launch_lr_check read of a chunk of their items on a checker WITH general convex pairs: its first item,
// their count, and the distances launch_convex_check (below) left for the chunk.  cv null: all items in one launch — a checker
// without such pairs, the kernels they always were.
struct CvChunk {
  long long first = 0, count = 0;
  const double* cv = nullptr;
  int32_t n_cv = 0;
};

constexpr int kOuterBlock = 256;        // threads per block of every one-thread-per-element kernel of these files

// Blocks of kOuterBlock threads that cover `total` elements; false when the grid would not fit (the launcher then reports
// hipErrorInvalidValue).
static inline bool grid_1d(long long total, unsigned* grid) {
  const long long g = (total + kOuterBlock - 1) / kOuterBlock;
  if (g > 0x7fffffffLL) return false;
  *grid = (unsigned)g;
  return true;
}

// multi-start IK (multistart.hip): seeding, target fan-out, selection — the kernels around the loop of mkh_solve_multistart
hipError_t launch_ms_seed(hipStream_t stream, const int32_t* seed_i, const double* seed_f, int B, int S, int nq, const double* q,
                          const double* user_seeds, unsigned long long rng_seed, long long target_index0, double* q_seeds);
hipError_t launch_ms_fanout(hipStream_t stream, const double* src, double* dst, int B, int S, int width);
hipError_t launch_ms_select(hipStream_t stream, int B, int S, int nq, int nv, int njnt, const int32_t* jnt, const double* q_all,
                            const double* v_all, const int32_t* status_all, const int32_t* iters_all, const int32_t* converged_all,
                            const double* q_ref, const double* weights, double* q_best, double* v_best, int32_t* iters,
                            int32_t* status, int32_t* converged, int32_t* seed_index, int32_t* n_converged);
// distinct solution sets (solution_set.hip): up to K representatives per target among its S candidates, no two within r2 (a
// squared distance) of each other — (B, K, .) outputs.  v_all / iters_all / status_all with their outputs, converged_all
// (absent: every candidate is eligible) and n_converged are optional.  S beyond kSsMaxCandidates: hipErrorInvalidValue (the
// per-candidate state of one target, 12 bytes each, lives in LDS).
constexpr int kSsMaxCandidates = 4096;
constexpr int kSsMaxSolutions = 64;
struct SsOut {
  double *q_set, *v_set;
  int32_t *iters, *status, *seed_index, *multiplicity;
  double* distance;
  int32_t *n_distinct, *n_converged, *n_uncovered;
};
hipError_t launch_ss_select(hipStream_t stream, int B, int S, int K, int nq, int nv, int njnt, const int32_t* jnt,
                            const double* q_all, const double* v_all, const int32_t* status_all, const int32_t* iters_all,
                            const int32_t* converged_all, const double* q_ref, const double* weights, double r2, const SsOut& o);
// turn unwinding (unwind.hip): n_rows rows of nq entries moved to the full turn nearest q_ref[row / rows_per_ref] at every
// address whose table entry says so — table (nq, 3): mode, range_lo, range_hi.  q_out may be q_rows.
constexpr double kUnwCopy = 0.0, kUnwFree = 1.0, kUnwRange = 2.0;
hipError_t launch_unwind_turns(hipStream_t stream, const double* table, long long n_rows, long long rows_per_ref, int nq,
                               const double* q_rows, const double* q_ref, double* q_out);
// the ladder on deduplicated nodes (ladder_nodes.hip): tracked and converged of the (rungs, K) slots a selection filled, from the
// slots' seed_index (>= 0: filled) and the (rungs, S) converged flags of the candidates
hipError_t launch_ladder_nodes_flags(hipStream_t stream, long long rungs, int S, int K, const int32_t* converged_all,
                                     const int32_t* seed_index, int32_t* tracked, int32_t* converged);
// goal sets (goalset.hip): per goal the closest eligible of its S candidates, per target the reached goal with the smallest
// goal_cost + distance, over (B, G, S, .) rows — (B, G, .) and (B, .) outputs.  converged_all (absent: every candidate is
// eligible), status_all / iters_all / v_all with their outputs, goal_cost (zeros) and goal_valid (every goal) are optional.
// B·G·S beyond int32: hipErrorInvalidValue.
struct GsIn {
  const double* __restrict__ q_all;
  const double* __restrict__ v_all;
  const int32_t* __restrict__ status_all;
  const int32_t* __restrict__ iters_all;
  const int32_t* __restrict__ converged_all;
  const double* __restrict__ q_ref;
  const double* __restrict__ weights;
  const double* __restrict__ goal_cost;
  const int32_t* __restrict__ goal_valid;
};
struct GsOut {
  double* __restrict__ q_best;
  double* __restrict__ v_best;
  int32_t *iters, *status, *converged, *goal_index, *seed_index, *n_reached;
  double* score;
  double* __restrict__ q_goal;
  double* __restrict__ v_goal;
  int32_t *iters_goal, *status_goal, *seed_index_goal, *reached, *n_converged_goal;
  double* distance_goal;
};
hipError_t launch_gs_select(hipStream_t stream, int B, int G, int S, int nq, int nv, int njnt, const int32_t* jnt, const GsIn& in,
                            const GsOut& o);
// trajectory IK (trajectory.hip): (B, T, W) ↔ (T, B, W) transposes and the joint velocity between waypoints — the kernels
// around the T loop launches of mkh_solve_trajectory
hipError_t launch_tj_gather(hipStream_t stream, const double* src, double* dst, int B, int T, int W);
hipError_t launch_tj_scatter(hipStream_t stream, const double* src, double* dst, int B, int T, int W);
hipError_t launch_tj_scatter_i32(hipStream_t stream, const int32_t* src, int32_t* dst, int B, int T);
hipError_t launch_tj_qvel(hipStream_t stream, const int32_t* jnt, int njnt, int B, int T, int nq, const double* q0,
                          const double* q_traj, long long q_sb, long long q_st, double dt, double* qvel, long long v_sb,
                          long long v_st, int time_major);
// keyframed trajectory IK (keyframes.hip): waypoint t's targets blended from keyframes k and k + 1 at parameter u, read in place
// through (instance, keyframe) strides, written to the loop's slab and (optionally) to waypoint t of the caller's *_targets_out
hipError_t launch_kf_frames(hipStream_t stream, const double* keys, long long s_b, long long s_k, int k, double u, int rows,
                            int n_frame, double* slab, double* out, long long o_sb);
hipError_t launch_kf_posture(hipStream_t stream, const int32_t* jnt, int njnt, const double* keys, long long s_b, long long s_k,
                             int k, double u, int rows, int n_posture, int nq, double* slab, double* out, long long o_sb);
hipError_t launch_kf_com(hipStream_t stream, const double* keys, long long s_b, long long s_k, int k, double u, int rows,
                         int width, double* slab, double* out, long long o_sb);
// multi-start trajectory IK (trajectory_multistart.hip): every candidate scored over its path and one chosen per instance, the
// chosen candidate's rows of the time-major (T, B·S, .) results gathered through the (instance, waypoint) strides of `out`.
// status_all / converged_all absent: every row passes that test; edge_margin_all (T, B·S) given: the score of "THE RULE, with a
// checker" — a waypoint t >= 1 counts only when edge_margin_all >= 0 (absent: the plain rule, bitwise)
hipError_t launch_tms_score(hipStream_t stream, int B, int S, int T, int nq, int njnt, const int32_t* jnt, const double* q0,
                            const double* q_all, const int32_t* status_all, const int32_t* converged_all, const double* weights,
                            const double* edge_margin_all, int32_t* seed_index, int32_t* n_tracked, int32_t* n_complete,
                            double* path_length);
hipError_t launch_tms_gather(hipStream_t stream, const double* all, double* out, const int32_t* seed_index, int B, int S, int T,
                             int W, long long o_sb, long long o_st);
hipError_t launch_tms_gather_i32(hipStream_t stream, const int32_t* all, int32_t* out, const int32_t* seed_index, int B, int S,
                                 int T, long long o_sb, long long o_st);
// checked candidate tracking (trajectory_free.hip; include/minkhip.h "THE RULE, with a checker" of mkh_solve_trajectory_multistart):
// launch_tmf_check judges the T·B·S rows of the time-major candidates q_all in one launch — node_margin_all, MKH_ST_IN_COLLISION
// OR-ed into status_all, and edge_margin_all: +inf at waypoint 0, the swept margin of the M >= 1 interior samples of the edge from
// the same candidate's row t − 1 where the row is eligible, NaN elsewhere — on the CHECKER's per-body descriptor (a device
// WideProblem; with general convex pairs the rows go in chunks — `chunk`, above — behind launch_convex_check, without a chunk
// it has none; nbody and n_pairs choose the build as in launch_clearance, the LDS is
// checker_plan.h's sweep_lds_bytes).  converged_all absent: every row counts as converged.  launch_tmf_edge_flags: the chosen candidate's
// edge_collision through the (instance, waypoint) strides of the caller's layout, and n_edge_collisions (B,).
hipError_t launch_tmf_check(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, int B, int S, int T, int M,
                            const double* q_all, const int32_t* converged_all, int32_t* status_all, double* node_margin_all,
                            double* edge_margin_all, const CvChunk& chunk = CvChunk{});
hipError_t launch_tmf_edge_flags(hipStream_t stream, int B, int S, int T, const int32_t* seed_index, const int32_t* converged_all,
                                 const int32_t* status_all, const double* edge_margin_all, int32_t* edge_collision, long long o_sb,
                                 long long o_st, int32_t* n_edge_collisions);
// seed tables (seed_table.hip): a chunk's (n, n_frame, 7) poses into the table's (n_frame·7, N) keys at entries j0 …, and the
// K entries nearest to each of B targets — indices (B, K), distances (B, K), the entries' q into rows 1 … K of a
// (B, K + 1, nq) slab; each output optional
hipError_t launch_st_keys(hipStream_t stream, const double* poses, int n, int n_frame, long long N, long long j0, double* keys);
hipError_t launch_st_query(hipStream_t stream, const double* keys, const double* q_tab, const double* weights, int N, int n_frame,
                           int nq, int B, const double* targets, int K, int32_t* index_out, double* dist_out, double* seeds_out);
// ladder-graph trajectory IK (ladder.hip): nodes tracked or not from the loops' flags, the dynamic program over the (B, T, S, nq)
// nodes with its back-trace (pred: B·T·S bytes; brk: B·T·ceil(S / 64) break masks), and the chosen nodes' rows of a (rows, S, W)
// array gathered through node_index (rows = B·T).  ladder_source_tile: the source nodes per LDS tile of a search launch (0: the
// model does not fit) and the launch's LDS bytes.
int ladder_source_tile(int S, int nq, int nv, int njnt, size_t* lds_bytes, bool mask = false);   // (mask: 64 flag bytes per source node more)
hipError_t launch_ladder_tracked(hipStream_t stream, const int32_t* converged, const int32_t* status, long long total,
                                 int32_t* tracked);
hipError_t launch_ladder_search(hipStream_t stream, int B, int T, int S, int nq, int nv, int njnt, const int32_t* jnt,
                                const double* q0, const double* q_nodes, const int32_t* tracked, const double* weights, double max_step_sq,
                                uint8_t* pred, unsigned long long* brk, int32_t* node_index, int32_t* n_tracked, int32_t* n_breaks,
                                double* path_length, int32_t* edge_break);
hipError_t launch_ladder_gather(hipStream_t stream, const double* all, double* out, const int32_t* node_index, long long rows, int S,
                                int W);
hipError_t launch_ladder_gather_i32(hipStream_t stream, const int32_t* all, int32_t* out, const int32_t* node_index, long long rows,
                                    int S);
// ladder refinement (ladder_refine.hip): the pass's private arrays — the working path r (B, T, nq) with its flags, the loops'
// rows of the repaired nodes, the break bits of r, and what one loop launch reads (start) and writes (x …) with the bad flags
// beside it, (B, .) each — and the device outputs of the guard (v … converged: optional).  launch_lr_step commits waypoint
// commit_t of the sweep in direction commit_dir (+1 / −1; commit_t < 0: nothing) and decides waypoint next_t of the sweep in
// direction next_dir (next_t < 0: nothing); launch_lr_guard prices r and the input path p, and returns the better one.
struct LrWork {
  double *r, *r_v;
  int32_t *r_trk, *r_rep, *r_st, *r_it, *r_cv, *r_eb;
  double *start, *x, *xv;
  int32_t *xst, *xit, *xcv, *bad;
};
struct LrOut {
  double *q, *v, *path_length;
  int32_t *tracked, *repaired, *refined, *edge_break, *n_tracked, *n_breaks, *status, *iters, *converged;
};
hipError_t launch_lr_step(hipStream_t stream, int B, int T, int nq, int nv, int njnt, const int32_t* jnt, const double* q0,
                          const double* weights, double max_step_sq, int commit_t, int commit_dir, int next_t, int next_dir,
                          const LrWork& w);
hipError_t launch_lr_guard(hipStream_t stream, int B, int T, int nq, int nv, int njnt, const int32_t* jnt, const double* q0,
                           const double* weights, double max_step_sq, const double* p, const int32_t* p_trk, const LrWork& w,
                           const LrOut& o);
// ladder refinement "with a checker" (ladder_refine.hip, ladder_refine_free.hip; include/minkhip.h "THE RULE OF THE REFINEMENT, with
// a checker"): r_trk and the guard's p_trk are then EFFECTIVE flags.  LrFreeWork: the node and edge margins of the working path,
// (B, T) each, and the three margins lr_check_kernel leaves per instance, step and SLOT, (B, 3, slots) — margin(x) | near edge |
// far edge, NaN: not evaluated or not swept; the samples of an edge are dealt to slots = lr_check_slots(M) blocks, each writes
// the minimum over its own, the step kernel the minimum over the slots.  LrFreeGuard: both paths' margins, and the returned path's (node_margin: optional).  launch_lr_check
// runs between the loop launch of waypoint commit_t and the launch_lr_step_free that commits it, on the CHECKER's per-body
// descriptor (a device WideProblem; with general convex pairs the instances go in chunks — `chunk`, above — behind
// launch_convex_check, without a chunk it has none; nbody and n_pairs choose the build as in launch_clearance, the
// LDS is checker_plan.h's sweep_lds_bytes); M >= 1 interior samples per edge.
constexpr int kLrMaxSlots = 8;
int lr_check_slots(int M);
struct LrFreeWork {
  double *r_nm, *r_em, *trip;
  int slots;
};
struct LrFreeGuard {
  const double *p_nm, *p_em, *r_nm, *r_em;
  double *node_margin, *edge_margin;
  int32_t *edge_collision, *n_edge_collisions;
};
hipError_t launch_lr_check(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, int B, int T, int M,
                           int commit_t, int commit_dir, const LrWork& w, double* trip, const CvChunk& chunk = CvChunk{});
hipError_t launch_lr_step_free(hipStream_t stream, int B, int T, int nq, int nv, int njnt, const int32_t* jnt, const double* q0,
                               const double* weights, double max_step_sq, int commit_t, int commit_dir, int next_t, int next_dir,
                               const LrWork& w, const LrFreeWork& f);
hipError_t launch_lr_guard_free(hipStream_t stream, int B, int T, int nq, int nv, int njnt, const int32_t* jnt, const double* q0,
                                const double* weights, double max_step_sq, const double* p, const int32_t* p_trk, const LrWork& w,
                                const LrOut& o, const LrFreeGuard& f);
// clearance (clearance.hip; include/minkhip.h "THE RULE OF CLEARANCE"): margin / pair / n_violated (N,) and distance (N, n_pairs) of
// N rows of q against the n_pairs >= 1 pairs of a checker's per-body descriptor (a device WideProblem), each output optional.
// nbody and n_pairs choose between one and four rows per wavefront and size the launch's LDS: beyond 64 KB of poses
// hipErrorInvalidValue.  cv: the (N, n_cv, 7) records launch_convex_pre left for the same rows, read for the pairs without an
// analytic routine.  status given: kStInCollision is OR-ed into the rows that are in collision.
constexpr int32_t kStInCollision = 64;   // MKH_ST_IN_COLLISION
hipError_t launch_clearance(hipStream_t stream, const void* wide_problem, int nbody, int n_pairs, int n_cv, const double* cv, int N,
                            const double* q, double* margin, int32_t* pair, int32_t* n_violated, double* distance, int32_t* status);
// swept clearance (sweep.hip; include/minkhip.h "THE RULE OF THE SWEEP"): the M interior samples of N edges against the pairs of a
// checker, one edge per wavefront or per DPP row by launch_clearance's criterion (general convex pairs: in chunks behind
// launch_convex_sweep, below).  Which edges:
//   kSweepPairs  edge e runs from row e of `from` to row e of `to`, (N, nq) each.
//   kSweepLadder N = B·(T − 1)·W·W, T >= 2: the edges (b, t >= 1, s', s) from node (t − 1, s) to node (t, s') of `nodes`
//                (B, T, W, nq), their outputs at ((b·T + t)·W + s')·W + s of (B, T, W, W) arrays whose t = 0 entries the launch
//                leaves alone; a destination with tracked == 0: not swept — margin NaN, blocked 0.
//   kSweepPath   N = B·T: the edge into waypoint t of the path `node_index` (B, T) through the same nodes; t = 0: margin +inf;
//                a destination with tracked == 0: as above.
// margin is optional; sample and pair (N,) are kSweepPairs' and required there; blocked, bytes, 1 where the edge collides, is the
// ladder modes' and optional.
// A checker WITH general convex pairs: the call's edges go in chunks — count > 0: this launch takes the edges [first, first + count)
// of the N, every index and output address still the whole call's — and cv (count·M, n_cv) holds the distances
// launch_convex_sweep left for the chunk's samples, sample i of the chunk's edge c in row c·M + i.  count = 0: all N edges, no cv.
enum : int32_t { kSweepPairs = 0, kSweepLadder = 1, kSweepPath = 2 };
struct SweepArgs {
  int32_t mode, M, T, W;
  long long N;
  const double *from, *to, *nodes;
  const int32_t *tracked, *node_index;
  double* margin;
  int32_t *sample, *pair;
  uint8_t* blocked;
  long long first, count;
  double* cv;
  int32_t n_cv;
};
hipError_t launch_sweep(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, const SweepArgs& a);
// certified sweep (certified_sweep.hip; include/minkhip.h "THE RULE OF THE CERTIFIED SWEEP"): N edges from row e of `from` to row e
// of `to`, each at the sample count its own motion bound asks for, on launch_sweep's geometry.  reach: the checker's
// (n_pairs, njnt, 2) table on the device (motion_bound.h).  Every output (N,) and required.  A checker of analytic pairs only.
// The modes of a ladder (include/minkhip.h THE RULE, "with a certifying checker"), edges and output places as launch_sweep has them:
//   kSweepLadder N = B·(T − 1)·W·W: per edge `blocked` under `policy` (MKH_EDGE_*; required), optionally the margin (double) and
//                the verdict (verdict_all, int8) — an edge that is not swept: 0, NaN, −1.
//   kSweepPath   N = B·T: margin, lower_bound, n_samples and verdict per (b, t), all required — t = 0: +inf, +inf, 0, −1; an
//                edge that is not swept: NaN, NaN, 0, −1.
// The other outputs are kSweepPairs' and are not read in these modes.
struct CertifiedArgs {
  long long N;
  const double *from, *to, *reach;
  double resolution;
  int32_t max_samples;
  double *margin, *lower_bound, *motion;
  int32_t *sample, *pair, *segment, *bound_pair, *n_samples, *capped, *verdict;
  // (behind the outputs of kSweepPairs, whose offsets in the kernel-argument segment stand)
  int32_t mode, T, W, policy;
  const double* nodes;
  const int32_t *tracked, *node_index;
  uint8_t* blocked;
  int8_t* verdict_all;
};
hipError_t launch_certified_sweep(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, const CertifiedArgs& a);
// n_certified[b] = the waypoints t >= 1 of instance b whose entry of verdict (B, T) is 1
hipError_t launch_certified_count(hipStream_t stream, int B, int T, const int32_t* verdict, int32_t* n_certified);
// The pre-pass of a chunk (convex_sweep.hip): the general convex distance routine on every interior sample of the chunk's swept
// edges with finite ends, one lane per (edge, sample, general convex pair), into a.cv — which the caller passes on to launch_sweep
// with the same SweepArgs.  C: the checker's lists of those pairs, C.n_cv = a.n_cv.
// ipw: items per wavefront, 0 = chosen from the size of the chunk (checker_plan.h cv_items_per_wave).
hipError_t launch_convex_sweep(hipStream_t stream, const void* wide_problem, const CvPre& C, const SweepArgs& a, int ipw);
// The pre-pass of the checks that judge rows INSIDE their launch (convex_check.hip), for a checker WITH general convex pairs: the
// distances of those pairs on every row the check of the items [first, first + count) could read — its conditions without the
// node's verdict —, one lane per (item, row, pair), into row (item − first)·rows_per_item + j of `out` (mkh_problem_set_check_rows).
//   kCvCheckTrack   launch_tmf_check's rows: item g of the (T, R, nq) candidates, rows_per_item = 1 + M (the node, the M samples
//                   of the edge from row g − R); status is read as it stands in front of the check.
//   kCvCheckRefine  launch_lr_check's instances at waypoint ct of a sweep in direction cdir: rows_per_item = 1 + 2M (x, the near
//                   edge, the far edge).
// The check of the same chunk then runs with the same first / count and `out` for its cv.
enum : int32_t { kCvCheckTrack = 0, kCvCheckRefine = 1 };
struct CvCheckArgs {
  int32_t mode, M;
  long long first, count;
  // kCvCheckTrack
  long long R;
  const double* q_all;
  const int32_t *converged, *status;
  // kCvCheckRefine
  int32_t T, ct, cdir;
  const double *r, *x;
  const int32_t *r_trk, *xst, *xcv, *bad;
};
hipError_t launch_convex_check(hipStream_t stream, const void* wide_problem, const CvPre& C, const CvCheckArgs& a, double* out);
// the nodes of a checked ladder: tracked_out[i] = tracked[i] != 0 && node_margin[i] >= 0
hipError_t launch_ladder_free_tracked(hipStream_t stream, const int32_t* tracked, const double* node_margin, long long total,
                                      int32_t* tracked_out);
// launch_ladder_search with the mask of blocked edges (B, T, S, S) bytes of a kSweepLadder launch (include/minkhip.h THE RULE,
// "with a checker"), and the back-trace's edge_collision (B, T) and n_edge_collisions (B,)
hipError_t launch_ladder_search_free(hipStream_t stream, int B, int T, int S, int nq, int nv, int njnt, const int32_t* jnt,
                                     const double* q0, const double* q_nodes, const int32_t* tracked, const uint8_t* blocked,
                                     const double* weights, double max_step_sq, uint8_t* pred, unsigned long long* brk,
                                     int32_t* node_index, int32_t* n_tracked, int32_t* n_breaks, double* path_length,
                                     int32_t* edge_break, int32_t* edge_collision, int32_t* n_edge_collisions);

}  // namespace mkh
