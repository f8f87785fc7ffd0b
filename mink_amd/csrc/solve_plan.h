// Everything about a plain solve (mkh_eval, mkh_solve, mkh_solve_dense, mkh_solve_steps, mkh_solve_until and the loop launches of
// the outer-loop calls) that can be decided from integers, on the host alone: whether the call is served (code and message of the
// refusal), the table of its arrays, the way they travel (device pointers, the pinned scratch, staged copies, staged copies in
// overlapped chunks) and where each lies in the pinned scratch.  solve_host.hip asks on behalf of a handle and executes; nothing
// here needs a device, so tests/host/solve_plan_cases.cpp walks it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/minkhip.h"

namespace mkh {

// Small host-pointer calls (a control loop's single configuration: the reference's everyday use) go through ONE pinned,
// device-visible host buffer (host_internal.h PinnedScratch) of this size.
constexpr size_t kSmallCallBytes = 64 << 10;

// ---- what the decisions read of a handle
struct SolveShape {
  int nq, nv, nbody, n_frame, n_posture, n_com, n_rows_tap, n_pairs;
  int n_dense_rows, n_dense_limit_rows, dense_box;
  int max_batch;
};

// ---- the call's arrays, in the order the pinned scratch holds them
enum SolveArray {
  A_Q, A_FT, A_PT, A_CT,                                   // inputs (q_out comes back in place of q)
  A_V, A_STATUS, A_ITERS, A_CONV,                          // outputs; the three int32 arrays are one block of the scratch
  A_DE, A_DJ, A_DG, A_DH, A_DLO, A_DHI,                    // dense (plugin) rows: MkhDenseRows, in its order
  A_TAP0,                                                  // the taps: MkhTaps / TapArgs, in their order
  A_TAP_SUBTREE_COM = A_TAP0 + 3, A_TAP_COLL_G = A_TAP0 + 10, A_TAP_QP_ITERS = A_TAP0 + 12,
  A_COUNT = A_TAP0 + 14
};
constexpr int kNumTaps = A_COUNT - A_TAP0;
static_assert(sizeof(MkhTaps) == kNumTaps * sizeof(void*) && sizeof(MkhDenseRows) == (A_TAP0 - A_DE) * sizeof(void*),
              "one table row per pointer of MkhTaps and of MkhDenseRows");

// ---- what they read of a call: bit i of `given` = the caller's pointer of row i is not NULL (a tap: asked for)
struct SolveWants {
  int32_t B, n_steps;
  bool posture_batched, com_batched, device_ptrs, unwind;  // MKH_FLAG_*
  bool until;                                              // thresholds given: the threshold-terminated loop
  bool q_out;
  bool taps, dense;                                        // the MkhTaps / MkhDenseRows pointer itself
  uint32_t given;
  constexpr bool has(int i) const { return (given >> i & 1u) != 0; }
  constexpr bool any_dense_box() const { return has(A_DLO) || has(A_DHI); }
};

// ---- the refusal: which test fails first, in the order the messages have always had
enum SolveRefusal {
  SR_OK, SR_BATCH, SR_UNWIND, SR_Q_NULL, SR_FT_NULL, SR_PT_NULL, SR_CT_NULL, SR_DT, SR_N_STEPS, SR_LIMIT_BOX, SR_DENSE_MISSING,
  SR_DENSE_TASK_NULL, SR_DENSE_LIMIT_NULL, SR_DENSE_STEPS, SR_MAX_BATCH, SR_UNTIL_NO_FRAME, SR_COUNT
};
constexpr SolveRefusal solve_refusal(const SolveShape& s, const SolveWants& w, bool dt_ok) {
  if (w.B < 1) return SR_BATCH;
  if (w.unwind) return SR_UNWIND;
  if (!w.has(A_Q)) return SR_Q_NULL;
  if (s.n_frame > 0 && !w.has(A_FT)) return SR_FT_NULL;
  if (s.n_posture > 0 && !w.has(A_PT)) return SR_PT_NULL;
  if (s.n_com > 0 && !w.has(A_CT)) return SR_CT_NULL;
  if (!dt_ok) return SR_DT;
  if (w.n_steps < 1) return SR_N_STEPS;
  if (!s.dense_box && w.dense && w.any_dense_box()) return SR_LIMIT_BOX;
  if (s.n_dense_rows || s.n_dense_limit_rows || s.dense_box) {
    if (!w.dense) return SR_DENSE_MISSING;
    if (s.n_dense_rows && (!w.has(A_DE) || !w.has(A_DJ))) return SR_DENSE_TASK_NULL;
    if (s.n_dense_limit_rows && (!w.has(A_DG) || !w.has(A_DH))) return SR_DENSE_LIMIT_NULL;
    if (w.n_steps > 1 || w.q_out) return SR_DENSE_STEPS;
  }
  // max_batch bounds everything the handle owns per instance — staging buffers, the warm-start active sets — whichever
  // kind of pointer the caller passes (a device-pointer warm start used to write past d_warm here)
  if (w.B > s.max_batch) return SR_MAX_BATCH;
  if (w.until && s.n_frame < 1) return SR_UNTIL_NO_FRAME;
  return SR_OK;
}

// The texts the other entry points' refusals share with a plain solve's (minkhip.hip refuse_unwind, refuse_inputs): %s = who asks.
constexpr const char* kUnwindRefusalFmt = "%s: MKH_FLAG_UNWIND_TURNS is honoured by mkh_solve_multistart_set and "
                                          "mkh_solve_trajectory_ladder_nodes only";
constexpr const char* kUntilNoFrameFmt = "%s needs at least one frame task to test the thresholds on";
constexpr const char* kNullInputText[4] = {"q is null", "frame_targets is null (TargetNotSet)", "posture_target is null (TargetNotSet)",
                                           "com_target is null (TargetNotSet)"};

// Code and message (into `err`, as checker_refuse does) of the refusal; MKH_OK: served.
inline int32_t solve_refuse(const SolveShape& s, const SolveWants& w, bool dt_ok, std::string& err) {
  char buf[512];
  buf[0] = 0;
  switch (solve_refusal(s, w, dt_ok)) {
    case SR_OK: case SR_COUNT: return MKH_OK;
    case SR_BATCH: snprintf(buf, sizeof buf, "B must be >= 1"); break;
    case SR_UNWIND: snprintf(buf, sizeof buf, kUnwindRefusalFmt, "a solve"); break;
    case SR_Q_NULL: snprintf(buf, sizeof buf, "%s", kNullInputText[A_Q]); break;
    case SR_FT_NULL: snprintf(buf, sizeof buf, "%s", kNullInputText[A_FT]); break;
    case SR_PT_NULL: snprintf(buf, sizeof buf, "%s", kNullInputText[A_PT]); break;
    case SR_CT_NULL: snprintf(buf, sizeof buf, "%s", kNullInputText[A_CT]); break;
    case SR_DT: snprintf(buf, sizeof buf, "dt must be > 0"); break;
    case SR_N_STEPS: snprintf(buf, sizeof buf, "n_steps must be >= 1"); break;
    case SR_LIMIT_BOX: snprintf(buf, sizeof buf, "limit_lo / limit_hi need a problem created with dense_limit_box = 1"); break;
    case SR_DENSE_MISSING: snprintf(buf, sizeof buf, "this problem has dense (plugin) rows: call mkh_solve_dense"); break;
    case SR_DENSE_TASK_NULL: snprintf(buf, sizeof buf, "dense task_e / task_J is null"); break;
    case SR_DENSE_LIMIT_NULL: snprintf(buf, sizeof buf, "dense limit_G / limit_h is null"); break;
    case SR_DENSE_STEPS: snprintf(buf, sizeof buf, "dense (plugin) rows are evaluated by the caller at q: no fused steps"); break;
    case SR_MAX_BATCH: snprintf(buf, sizeof buf, "B=%d exceeds max_batch=%d of this problem", w.B, s.max_batch); break;
    case SR_UNTIL_NO_FRAME: snprintf(buf, sizeof buf, kUntilNoFrameFmt, "mkh_solve_until"); break;
  }
  err = buf;
  return MKH_E_INVALID;
}

// ---- one row of the table
enum SolveDir { SD_IN, SD_OUT, SD_IN_OUT };        // SD_IN_OUT: q of a fused loop — q_out is written in place of it
// The staging buffer of a row on the handle (MkhProblem::stage): iterations | converged and limit_lo | limit_hi are halves of one.
enum SolveSlot { SS_Q, SS_FT, SS_PT, SS_CT, SS_V, SS_STATUS, SS_ITERS, SS_DE, SS_DJ, SS_DG, SS_DH, SS_DBOX, SS_QKEEP, SS_COUNT };
struct SolveArrayRow {
  size_t width;        // bytes per instance; of the whole array when `shared`
  bool shared;         // one for the call (a target that is not batched)
  SolveDir dir;
  bool zero;           // cleared in front of the launch (the kernel writes only part of it)
  bool live;           // the call has it
  bool back;           // copied back to a host caller: v, q_out in place of q, status only with v_out, iters / converged only under
                       // thresholds, every tap asked for
  int slot, half;      // its staging buffer: SolveSlot, 0 / 1 for the first / second max_batch-sized half; -1: none (a tap)
  constexpr size_t bytes(size_t B) const { return shared ? width : B * width; }
};
constexpr SolveArrayRow solve_array(const SolveShape& s, const SolveWants& w, int i) {
  const size_t nq = (size_t)s.nq, nv = (size_t)s.nv, d = sizeof(double), i4 = sizeof(int32_t);
  const bool v = w.has(A_V);
  switch (i) {
    case A_Q: return {nq * d, false, w.q_out ? SD_IN_OUT : SD_IN, false, true, w.q_out, SS_Q, 0};
    case A_FT: return {(size_t)s.n_frame * 7 * d, false, SD_IN, false, s.n_frame > 0, false, SS_FT, 0};
    case A_PT: return {(size_t)s.n_posture * nq * d, !w.posture_batched, SD_IN, false, s.n_posture > 0, false, SS_PT, 0};
    case A_CT: return {(size_t)s.n_com * 3 * d, !w.com_batched, SD_IN, false, s.n_com > 0, false, SS_CT, 0};
    case A_V: return {nv * d, false, SD_OUT, false, v, v, SS_V, 0};
    case A_STATUS: return {i4, false, SD_OUT, false, true, w.has(A_STATUS) && v, SS_STATUS, 0};
    case A_ITERS: return {i4, false, SD_OUT, false, w.until, w.until && w.has(A_ITERS), SS_ITERS, 0};
    case A_CONV: return {i4, false, SD_OUT, false, w.until, w.until && w.has(A_CONV), SS_ITERS, 1};
    case A_DE: return {(size_t)s.n_dense_rows * d, false, SD_IN, false, s.n_dense_rows > 0, false, SS_DE, 0};
    case A_DJ: return {(size_t)s.n_dense_rows * nv * d, false, SD_IN, false, s.n_dense_rows > 0, false, SS_DJ, 0};
    case A_DG: return {(size_t)s.n_dense_limit_rows * nv * d, false, SD_IN, false, s.n_dense_limit_rows > 0, false, SS_DG, 0};
    case A_DH: return {(size_t)s.n_dense_limit_rows * d, false, SD_IN, false, s.n_dense_limit_rows > 0, false, SS_DH, 0};
    case A_DLO: return {nv * d, false, SD_IN, false, s.dense_box != 0 && w.has(A_DLO), false, SS_DBOX, 0};
    case A_DHI: return {nv * d, false, SD_IN, false, s.dense_box != 0 && w.has(A_DHI), false, SS_DBOX, 1};
    default: break;
  }
  // the taps: (width, zero first)
  const size_t rows = (size_t)s.n_rows_tap, pairs = (size_t)s.n_pairs;
  const size_t tap_w[kNumTaps] = {(size_t)s.nbody * 3 * 8, (size_t)s.nbody * 4 * 8, (size_t)s.n_frame * 7 * 8, 3 * 8, rows * 8, rows * nv * 8, nv * nv * 8,
                                  nv * 8, nv * 8, nv * 8, pairs * nv * 8, pairs * 8, 4, 16 * 8};
  const bool tap_zero[kNumTaps] = {false, false, false, true, true, true, false, false, false, false, true, false, true, true};
  const bool on = w.taps && w.has(i);
  return {tap_w[i - A_TAP0], false, SD_OUT, tap_zero[i - A_TAP0], on, on, -1, 0};
}
// Outputs come back in the order they always have: v, q_out, then the rest as the table has them.
constexpr int solve_back_order(int k) { return k == 0 ? A_V : (k <= A_V ? k - 1 : k); }

// ---- the pinned scratch: where every row of a small host-pointer call lies.  Every block is rounded up to 8 bytes; status |
// iterations | converged are ONE block of int32 (the offsets of the latter two are B and 2·B int32 into it).
constexpr size_t round8(size_t n) { return (n + 7) & ~(size_t)7; }
struct PinnedLayout {
  size_t off[A_COUNT];
  size_t total;
};
constexpr PinnedLayout pinned_layout(const SolveShape& s, const SolveWants& w) {
  PinnedLayout L{};
  const size_t B = (size_t)w.B;
  size_t o = 0;
  for (int i = A_Q; i <= A_V; ++i) {
    L.off[i] = o;
    const SolveArrayRow r = solve_array(s, w, i);
    if (r.live) o += round8(r.bytes(B));
  }
  L.off[A_STATUS] = o; L.off[A_ITERS] = o + B * sizeof(int32_t); L.off[A_CONV] = o + 2 * B * sizeof(int32_t);
  o += round8(B * (w.until ? 3 : 1) * sizeof(int32_t));
  for (int i = A_TAP0; i < A_COUNT; ++i) {
    L.off[i] = o;
    const SolveArrayRow r = solve_array(s, w, i);
    if (r.live) o += round8(r.bytes(B));
  }
  L.total = o;
  return L;
}

// ---- the way the arrays travel
enum class SolveRoute { Device, Pinned, Staged, Chunked };
struct SolveRoutePlan {
  SolveRoute route;
  int n_chunks;        // Chunked: 2 … 4; else 1
  size_t chunk;        // instances of every chunk but the last, which takes the remainder; B when there is one chunk
};
// Large plain solves in chunks: the host → device copy of chunk c + 1 and the device → host copy of chunk c − 1 run on
// streams of their own beside the kernel of chunk c (the single-shot sequence copy in, solve, copy out left the GPU idle
// for more than half of a 65 536-instance G1 call).  Chunks of at least 8 192 instances; each is dispatched by its own
// size (a small arm's chunk may run the row kernel where the whole batch would have taken the lane kernel: same optimum).
// Only where the copies are worth overlapping (≥ 32 MB staged: tools/bench_host_path.py — G1 at 65 536 instances
// 2.02 → 1.72 ms per call, the G1 full example 2.79 → 2.19 ms; a 65 536-instance UR5e call moves 10 MB around a 0.08 ms
// kernel and LOSES 0.15 ms to the events and the three extra launches).
constexpr int kMinChunk = 8192, kMaxChunks = 4;
constexpr size_t kMinChunkedBytes = (size_t)32 << 20;
// (`no_chunks`: MKH_DEBUG_NO_CHUNKS of an experiment build, read by the caller — the A/B of the chunked route)
constexpr SolveRoutePlan solve_route(const SolveShape& s, const SolveWants& w, bool no_chunks) {
  const size_t B = (size_t)w.B;
  if (w.device_ptrs) return {SolveRoute::Device, 1, B};
  const bool dense = s.n_dense_rows || s.n_dense_limit_rows || s.dense_box;
  if (!dense && pinned_layout(s, w).total <= kSmallCallBytes) return {SolveRoute::Pinned, 1, B};
  size_t staged = 0;                                       // per instance: q, frame targets, batched targets, v — and q_out
  for (int i = A_Q; i <= A_V; ++i) {
    const SolveArrayRow r = solve_array(s, w, i);
    if (!r.shared) staged += r.width;
  }
  if (w.q_out) staged += (size_t)s.nq * sizeof(double);
  staged *= B;
  if (no_chunks || w.taps || dense || !w.has(A_V) || w.B < 2 * kMinChunk || staged < kMinChunkedBytes) return {SolveRoute::Staged, 1, B};
  const int n = w.B / kMinChunk < kMaxChunks ? w.B / kMinChunk : kMaxChunks;
  return {SolveRoute::Chunked, n, (B / n) / 64 * 64};
}

namespace solve_plan_test {
// the byte count of a small call as the solve path summed it before there was a layout
constexpr size_t pinned_sum(const SolveShape& s, const SolveWants& w) {
  const size_t B = (size_t)w.B;
  size_t n = (B * s.nq + B * s.n_frame * 7 + (size_t)s.n_posture * s.nq * (w.posture_batched ? B : 1) +
              (size_t)s.n_com * 3 * (w.com_batched ? B : 1) + (w.has(A_V) ? B * s.nv : 0)) * sizeof(double) +
             round8(B * (w.until ? 3 : 1) * sizeof(int32_t));
  for (int i = A_TAP0; i < A_COUNT; ++i)
    if (w.taps && w.has(i)) n += round8(B * solve_array(s, w, i).width);
  return n;
}
constexpr bool cell_holds(const SolveShape& s, const SolveWants& w) {
  const PinnedLayout L = pinned_layout(s, w);
  if (L.total != pinned_sum(s, w)) return false;
  for (int i = 0; i < A_COUNT; ++i)
    if (i != A_ITERS && i != A_CONV && L.off[i] % 8 != 0) return false;          // (every block; the two are inside the int32 block)
  const SolveRoutePlan r = solve_route(s, w, false);
  if (r.route != SolveRoute::Chunked) return r.n_chunks == 1 && solve_route(s, w, true).route == r.route;
  return solve_route(s, w, true).route == SolveRoute::Staged && r.n_chunks >= 2 && r.n_chunks <= kMaxChunks && r.chunk >= (size_t)kMinChunk &&
         r.chunk % 64 == 0 && (size_t)(r.n_chunks - 1) * r.chunk < (size_t)w.B;
}
// two humanoids (nq 44 and 36, the second with a COM task and collision pairs) and a small arm; B around one instance, the 64 KB boundary and the chunk rule;
// eval, solve, steps, until; targets batched or not; no tap, the pivot counts alone, all of them
constexpr bool shape_holds(const SolveShape& s) {
  const int Bs[] = {1, 7, 48, 96, 16383, 16384, 36316, 40001, 65536};
  const uint32_t in = 1u << A_Q | 1u << A_FT | 1u << A_PT | 1u << A_CT, all_taps = ((1u << kNumTaps) - 1) << A_TAP0;
  for (int B : Bs)
    for (int kind = 0; kind < 4; ++kind)
      for (int bat = 0; bat < 2; ++bat)
        for (int tp = 0; tp < 3; ++tp) {
          SolveWants w{B, kind >= 2 ? 3 : 1, bat != 0, bat != 0, false, false, kind == 3, kind >= 2, tp != 0, false, in};
          if (kind >= 1) w.given |= 1u << A_V | 1u << A_STATUS;
          if (kind == 3) w.given |= 1u << A_ITERS | 1u << A_CONV;
          if (tp) w.given |= tp == 1 ? 1u << A_TAP_QP_ITERS : all_taps;
          if (!cell_holds(s, w)) return false;
        }
  return true;
}
static_assert(shape_holds(SolveShape{44, 43, 45, 4, 1, 0, 67, 0, 0, 0, 0, 65536}), "layout = sum, blocks on 8 bytes, chunks inside B: humanoid");
static_assert(shape_holds(SolveShape{36, 35, 31, 3, 1, 1, 56, 4, 0, 0, 0, 65536}), "... with a COM task and collision pairs");
static_assert(shape_holds(SolveShape{6, 6, 8, 1, 1, 0, 12, 0, 0, 0, 0, 65536}), "... small arm");
static_assert(solve_route(SolveShape{44, 43, 45, 4, 1, 0, 67, 0, 0, 0, 0, 65536},
                          SolveWants{40001, 1, false, false, false, false, false, false, false, false, 1u << A_Q | 1u << A_FT | 1u << A_PT | 1u << A_V}, false)
                  .route == SolveRoute::Chunked, "40 001 humanoid instances stage 32 MB: chunks");
}  // namespace solve_plan_test

}  // namespace mkh
