// Everything about a collision checker that can be decided from integers, on the host alone: whether a handle can serve a call
// (code and message of the refusal), how many items of a chunked launch its buffers hold, and the launch geometry the host and the
// kernel files' launchers share.  checker_host.hip asks on behalf of a handle; nothing here needs a device, so
// tests/host/checker_cases.cpp walks it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/minkhip.h"

namespace mkh {

// ---- launch geometry
// Four rows (edges, items) per wavefront, each on a 16-lane DPP row with its own slice of LDS, where a quarter of a wavefront
// holds a row's bodies and pairs in a trip or two; else one per wavefront.
constexpr bool checker_quarter(int nbody, int n_pairs) { return nbody <= 32 && n_pairs <= 32; }
// LDS bytes of a clearance launch: the body poses of its rows.
constexpr size_t clearance_lds_bytes(int nbody, int n_pairs) {
  return (size_t)(checker_quarter(nbody, n_pairs) ? 4 : 1) * 7 * (size_t)nbody * sizeof(double);
}
// ... and of a launch that walks the samples of edges (sweep.hip, trajectory_free.hip, ladder_refine_free.hip): per slice the poses
// and three rows of q.
constexpr size_t sweep_lds_bytes(int nbody, int nq, int n_pairs) {
  return (size_t)(checker_quarter(nbody, n_pairs) ? 4 : 1) * (7 * (size_t)nbody + 3 * (size_t)nq) * sizeof(double);
}
// ... and of a certified sweep (certified_sweep.hip): the sweep's slice and three rows of n_pairs per group — the motion bounds
// L_k of the edge, the previous point's margins, the current point's distances.
constexpr size_t certified_lds_bytes(int nbody, int nq, int n_pairs) {
  return (size_t)(checker_quarter(nbody, n_pairs) ? 4 : 1) * (7 * (size_t)nbody + 3 * (size_t)nq + 3 * (size_t)n_pairs) * sizeof(double);
}
constexpr size_t kCheckerLdsMax = 64 * 1024;
// Items per wavefront of the general convex pre-passes (convex_pre.hip, and why): ≈ 4 096 wavefronts when the launch allows
// (2 resident per SIMD x 1 024 SIMDs, twice over), at most 64 items each.
constexpr int cv_items_per_wave(long long total) {
  const long long w = (total + 4095) / 4096;
  return (int)(w < 1 ? 1 : (w > 64 ? 64 : w));
}

// ---- what the decisions read of a handle
struct CheckerShape {
  int n_pairs, n_cv;               // collision pairs; those of them pre-evaluated as general convex pairs
  bool convex_pairs, has_wide;     // some pair has no analytic routine; the per-body arrays exist
  int nbody, nq, max_batch;        // (max_batch >= 1: problem creation refuses anything else)
  int64_t sweep_rows, check_rows;  // mkh_problem_set_sweep_rows / mkh_problem_set_check_rows
};

// ---- what a call does with the checker
struct CheckerUse {
  int32_t sweeps_edges;            // M >= 1: it sweeps edges known in front of a launch, M samples each, general convex pairs
                                   // through sweep_rows; 0: it sweeps none
  int32_t item_rows;               // > 0: it judges rows INSIDE a launch, so many per item, general convex pairs through
                                   // check_rows; 0: it judges none
  int32_t certifies = 0;           // 1: a certified sweep — per-edge sample counts, which the sweep_rows chunking does not hold
  // (a sample count may reach these before the entry point has judged it: below 1 it counts as 1)
  static constexpr int32_t samples(int32_t M) { return M < 1 ? 1 : M; }
  static constexpr int32_t tracking_item(int32_t M) { return 1 + samples(M); }          // the node, the edge into it
  static constexpr int32_t refinement_item(int32_t M) { return 1 + 2 * samples(M); }    // x, the near edge, the far edge
  static constexpr CheckerUse clearance_only() { return {0, 0}; }                       // rows of q in memory, nothing else
  static constexpr CheckerUse sweep(int32_t M) { return {samples(M), 0}; }
  static constexpr CheckerUse tracking(int32_t M) { return {0, tracking_item(M)}; }
  static constexpr CheckerUse refinement(int32_t M) { return {samples(M), refinement_item(M)}; }
  static constexpr CheckerUse ladder(int32_t M, bool refined) { return refined ? refinement(M) : sweep(M); }
  static constexpr CheckerUse certified() { return {0, 0, 1}; }
};

// ---- the refusal: which test fails first, in the order the messages have always had
enum CheckerRefusal {
  CK_OK, CK_NO_PAIRS, CK_NO_WIDE, CK_CONVEX_NOT_PRE, CK_POSES_LDS,       // what a clearance refuses
  CK_NO_CHECK_ROWS, CK_NO_SWEEP_ROWS, CK_CHECK_ROWS_SHORT, CK_SWEEP_ROWS_SHORT, CK_SWEEP_LDS,
  CK_CERT_CONVEX, CK_CERT_LDS                                            // what a certified sweep refuses beyond a clearance
};
constexpr CheckerRefusal checker_refusal(const CheckerShape& s, const CheckerUse& u) {
  if (s.n_pairs < 1) return CK_NO_PAIRS;
  if (!s.has_wide) return CK_NO_WIDE;
  if (s.convex_pairs && s.n_cv == 0) return CK_CONVEX_NOT_PRE;
  if ((size_t)s.nbody * 7 * sizeof(double) > kCheckerLdsMax) return CK_POSES_LDS;
  if (u.certifies) {
    if (s.convex_pairs) return CK_CERT_CONVEX;
    return certified_lds_bytes(s.nbody, s.nq, s.n_pairs) > kCheckerLdsMax ? CK_CERT_LDS : CK_OK;
  }
  if (u.sweeps_edges < 1 && u.item_rows < 1) return CK_OK;
  if (s.n_cv > 0) {                                            // room for the distances of the general convex pairs
    if (u.item_rows > 0 && s.check_rows == 0) return CK_NO_CHECK_ROWS;
    if (u.sweeps_edges > 0 && s.sweep_rows == 0) return CK_NO_SWEEP_ROWS;
    if (u.item_rows > 0 && s.check_rows < u.item_rows) return CK_CHECK_ROWS_SHORT;
    if (u.sweeps_edges > 0 && s.sweep_rows < u.sweeps_edges) return CK_SWEEP_ROWS_SHORT;
  }
  if (sweep_lds_bytes(s.nbody, s.nq, s.n_pairs) > kCheckerLdsMax) return CK_SWEEP_LDS;
  return CK_OK;
}

// Code and message (into `err`, as plan_problem does) of the refusal of shape `s` for use `u` by entry point `who`; MKH_OK: served.
inline int32_t checker_refuse(const CheckerShape& s, const CheckerUse& u, const char* who, std::string& err) {
  char buf[512];
  int32_t code = MKH_E_INVALID;
  buf[0] = 0;
  switch (checker_refusal(s, u)) {
    case CK_OK:
      return MKH_OK;
    case CK_NO_PAIRS:
      snprintf(buf, sizeof buf, "%s: the checker has no collision pairs (a problem with CollisionAvoidanceLimits is one)", who);
      break;
    case CK_NO_WIDE:
      snprintf(buf, sizeof buf, "%s: the checker was created with MKH_DIAG_NO_WIDE_REDO: it has no per-body arrays to compute poses from", who);
      break;
    case CK_CONVEX_NOT_PRE:
      snprintf(buf, sizeof buf, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls) that are not pre-evaluated "
                                "on this handle (a model beyond 64 bodies or dofs): no clearance", who);
      break;
    case CK_POSES_LDS:
      code = MKH_E_LIMIT;
      snprintf(buf, sizeof buf, "%s: %d bodies: the poses of one row do not fit 64 KB of LDS (at most 1170 bodies)", who, s.nbody);
      break;
    case CK_NO_CHECK_ROWS:
      snprintf(buf, sizeof buf, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls): they are pre-evaluated on "
                                "rows in memory, and this call judges rows it produces inside a launch (mkh_problem_set_check_rows / "
                                "CollisionChecker(check_rows=) reserves room for their distances)", who);
      break;
    case CK_NO_SWEEP_ROWS:
      if (u.item_rows > 0)
        snprintf(buf, sizeof buf, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls) and check_rows, but this "
                                  "call also sweeps edges of paths (mkh_problem_set_sweep_rows / CollisionChecker(sweep_rows=) reserves "
                                  "room for their distances)", who);
      else
        snprintf(buf, sizeof buf, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls): they are pre-evaluated on "
                                  "rows in memory, and the samples of a sweep are never written there (mkh_problem_set_sweep_rows / "
                                  "CollisionChecker(sweep_rows=) reserves room for their distances)", who);
      break;
    case CK_CHECK_ROWS_SHORT:
      code = MKH_E_LIMIT;
      snprintf(buf, sizeof buf, "%s: check_rows = %lld holds less than one item of %d rows", who, (long long)s.check_rows, u.item_rows);
      break;
    case CK_SWEEP_ROWS_SHORT:
      code = MKH_E_LIMIT;
      snprintf(buf, sizeof buf, "%s: sweep_rows = %lld holds less than one edge of n_samples = %d samples", who, (long long)s.sweep_rows,
               u.sweeps_edges);
      break;
    case CK_SWEEP_LDS:
      code = MKH_E_LIMIT;
      snprintf(buf, sizeof buf, "%s: %d bodies, nq = %d: the poses of a sample and the three rows of q beside them do not fit 64 KB of LDS "
                                "(7 nbody + 3 nq <= 8192)", who, s.nbody, s.nq);
      break;
    case CK_CERT_CONVEX:
      snprintf(buf, sizeof buf, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls): they are not certified "
                                "yet — the per-edge sample counts of a certified sweep do not fit the chunks of sweep_rows", who);
      break;
    case CK_CERT_LDS:
      code = MKH_E_LIMIT;
      snprintf(buf, sizeof buf, "%s: %d bodies, nq = %d, %d pairs: the sweep's slice and the three rows of pairs beside it do not fit "
                                "64 KB of LDS (%s(7 nbody + 3 nq + 3 n_pairs) <= 8192)", who, s.nbody, s.nq, s.n_pairs,
               checker_quarter(s.nbody, s.n_pairs) ? "4 " : "");
      break;
  }
  err = buf;
  return code;
}

// ---- the chunks of the launches that go through a buffer of bounded rows.  Each is >= 1 for every use checker_refusal serves
// and 0 for a use that does not go through that buffer (the static test below; tests/host/checker_cases.cpp over the matrix) —
// the chunk runner of checker_host.hip takes its `per` from here and nowhere else.
// Rows of a clearance launch: the buffer of pre-evaluated convex pairs holds max_batch of them.
constexpr long long clearance_chunk(const CheckerShape& s) { return s.max_batch; }
// Edges of a sweep launch on a checker with general convex pairs: M rows of sweep_rows each.
constexpr long long sweep_chunk(const CheckerShape& s, const CheckerUse& u) { return u.sweeps_edges > 0 ? s.sweep_rows / u.sweeps_edges : 0; }
// Items of a check that judges rows inside its launch, on such a checker: item_rows rows of check_rows each.
constexpr long long check_chunk(const CheckerShape& s, const CheckerUse& u) { return u.item_rows > 0 ? s.check_rows / u.item_rows : 0; }

namespace checker_plan_test {
// every (sweep_rows, check_rows) up to 8 against every use at M = 1 … 3: a served use has room for one item in each buffer it
// goes through, and never more items than rows
constexpr bool chunks_hold(const CheckerShape& s, const CheckerUse& u) {
  if (checker_refusal(s, u) != CK_OK) return true;
  if (clearance_chunk(s) < 1) return false;
  if (s.n_cv == 0) return true;                                // (one launch: no chunks)
  if (u.sweeps_edges > 0 && (sweep_chunk(s, u) < 1 || sweep_chunk(s, u) * u.sweeps_edges > s.sweep_rows)) return false;
  if (u.item_rows > 0 && (check_chunk(s, u) < 1 || check_chunk(s, u) * u.item_rows > s.check_rows)) return false;
  return true;
}
constexpr bool all_chunks_hold() {
  for (int n_cv = 0; n_cv <= 2; n_cv += 2)
    for (int sr = 0; sr <= 8; ++sr)
      for (int cr = 0; cr <= 8; ++cr)
        for (int M = 1; M <= 3; ++M) {
          const CheckerShape s{3, n_cv, n_cv > 0, true, 7, 6, 1, sr, cr};
          const CheckerUse uses[] = {CheckerUse::clearance_only(), CheckerUse::sweep(M), CheckerUse::tracking(M), CheckerUse::refinement(M),
                                     CheckerUse::ladder(M, false), CheckerUse::ladder(M, true)};
          for (const CheckerUse& u : uses)
            if (!chunks_hold(s, u)) return false;
        }
  return true;
}
static_assert(all_chunks_hold(), "a use the refusal serves has a chunk of at least one item");
static_assert(checker_refusal(CheckerShape{3, 2, true, true, 7, 6, 1, 64, 64}, CheckerUse::certified()) == CK_CERT_CONVEX &&
              checker_refusal(CheckerShape{3, 0, false, true, 7, 6, 1, 0, 0}, CheckerUse::certified()) == CK_OK &&
              checker_refusal(CheckerShape{2720, 0, false, true, 7, 6, 1, 0, 0}, CheckerUse::certified()) == CK_CERT_LDS,
              "a certified sweep: no general convex pairs whatever the buffers hold, and its own LDS slice");
static_assert(checker_refusal(CheckerShape{3, 2, true, true, 7, 6, 1, 1, 4}, CheckerUse::refinement(2)) == CK_CHECK_ROWS_SHORT &&
              checker_refusal(CheckerShape{3, 2, true, true, 7, 6, 1, 1, 5}, CheckerUse::refinement(2)) == CK_SWEEP_ROWS_SHORT,
              "check_rows is judged before sweep_rows");
}  // namespace checker_plan_test

}  // namespace mkh
