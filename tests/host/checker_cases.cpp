// Host-only driver of mink_amd/csrc/checker_plan.h for tests/test_checker_plan_cpu.py: the refusal of a checker handle for a use,
// and the chunk sizes of the uses it serves, over a matrix of shapes — one JSON object per line.  Beside each cell the answer of the
// REFERENCE: clearance_refuse / sweep_refuse as minkhip.hip had them before the checker's planning was split out (the functions
// below, copied verbatim with `fail` writing into a string of this program), called as the entry points called them.  Built with
// the host sanitizers by the test and run as a child process.
#include <cstdarg>
#include <cstdio>
#include <set>
#include <string>

#include "../../mink_amd/csrc/checker_plan.h"

namespace ref {

std::string g_err;
int32_t fail(int32_t code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// what the copied functions read of a handle
struct Model { int nbody, nq; };
struct Problem {
  struct { int n_pairs; } dev;
  const void* d_wide;
  bool convex_pairs;
  struct { int n_cv; } cv;
  const Model* model;
  int64_t sweep_rows, check_rows;
};
typedef Problem MkhProblem;
namespace mkh {
size_t sweep_lds_bytes(int nbody, int nq, int n_pairs) {
  const bool quarter = nbody <= 32 && n_pairs <= 32;
  return (size_t)(quarter ? 4 : 1) * (7 * (size_t)nbody + 3 * (size_t)nq) * sizeof(double);
}
}  // namespace mkh

// ---- verbatim from here
static int32_t clearance_refuse(const MkhProblem* ck, const char* who) {
  if (ck->dev.n_pairs < 1) return fail(MKH_E_INVALID, "%s: the checker has no collision pairs (a problem with CollisionAvoidanceLimits is one)", who);
  if (!ck->d_wide)
    return fail(MKH_E_INVALID, "%s: the checker was created with MKH_DIAG_NO_WIDE_REDO: it has no per-body arrays to compute poses from", who);
  if (ck->convex_pairs && ck->cv.n_cv == 0)
    return fail(MKH_E_INVALID, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls) that are not pre-evaluated "
                               "on this handle (a model beyond 64 bodies or dofs): no clearance", who);
  if ((size_t)ck->model->nbody * 7 * sizeof(double) > 64 * 1024)
    return fail(MKH_E_LIMIT, "%s: %d bodies: the poses of one row do not fit 64 KB of LDS (at most 1170 bodies)", who, ck->model->nbody);
  return MKH_OK;
}

static int32_t sweep_refuse(const MkhProblem* ck, const char* who, int32_t n_samples = 0, int32_t check_item = 0) {
  if (const int32_t rc = clearance_refuse(ck, who)) return rc;
  if (ck->cv.n_cv > 0 && check_item > 0) {
    if (ck->check_rows == 0)
      return fail(MKH_E_INVALID, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls): they are pre-evaluated on "
                                 "rows in memory, and this call judges rows it produces inside a launch (mkh_problem_set_check_rows / "
                                 "CollisionChecker(check_rows=) reserves room for their distances)", who);
    if (n_samples >= 1 && ck->sweep_rows == 0)
      return fail(MKH_E_INVALID, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls) and check_rows, but this "
                                 "call also sweeps edges of paths (mkh_problem_set_sweep_rows / CollisionChecker(sweep_rows=) reserves "
                                 "room for their distances)", who);
    if (ck->check_rows < check_item)
      return fail(MKH_E_LIMIT, "%s: check_rows = %lld holds less than one item of %d rows", who, (long long)ck->check_rows, check_item);
    if (n_samples >= 1 && ck->sweep_rows < n_samples)
      return fail(MKH_E_LIMIT, "%s: sweep_rows = %lld holds less than one edge of n_samples = %d samples", who, (long long)ck->sweep_rows,
                  n_samples);
  } else if (ck->cv.n_cv > 0 && (n_samples < 1 || ck->sweep_rows == 0))
    return fail(MKH_E_INVALID, "%s: the checker has general convex pairs (cylinder-box, ellipsoid-*, mesh hulls): they are pre-evaluated on "
                               "rows in memory, and the samples of a sweep are never written there%s", who,
                n_samples < 1 ? " (this call does not take them through sweep_rows either)"
                              : " (mkh_problem_set_sweep_rows / CollisionChecker(sweep_rows=) reserves room for their distances)");
  if (ck->cv.n_cv > 0 && ck->sweep_rows < n_samples)
    return fail(MKH_E_LIMIT, "%s: sweep_rows = %lld holds less than one edge of n_samples = %d samples", who, (long long)ck->sweep_rows,
                n_samples);
  if (mkh::sweep_lds_bytes(ck->model->nbody, ck->model->nq, ck->dev.n_pairs) > 64 * 1024)
    return fail(MKH_E_LIMIT, "%s: %d bodies, nq = %d: the poses of a sample and the three rows of q beside them do not fit 64 KB of LDS "
                             "(7 nbody + 3 nq <= 8192)", who, ck->model->nbody, ck->model->nq);
  return MKH_OK;
}

static int32_t tracking_item(int32_t n_samples) { return 1 + (n_samples < 1 ? 1 : n_samples); }
static int32_t refinement_item(int32_t n_samples) { return 1 + 2 * (n_samples < 1 ? 1 : n_samples); }
// ---- verbatim to here

}  // namespace ref

using mkh::CheckerShape;
using mkh::CheckerUse;

namespace {

enum Use { CLEARANCE, SWEEP, TRACKING, REFINEMENT, LADDER, LADDER_REFINED, N_USES };
const char* const kUseName[N_USES] = {"clearance", "sweep", "tracking", "refinement", "ladder", "ladder_refined"};

// the use as the new code names it, and the reference as the entry points of the parent called it (n: the call's n_samples)
CheckerUse use_of(Use u, int n) {
  switch (u) {
    case CLEARANCE: return CheckerUse::clearance_only();
    case SWEEP: return CheckerUse::sweep(n);
    case TRACKING: return CheckerUse::tracking(n);
    case REFINEMENT: return CheckerUse::refinement(n);
    case LADDER: return CheckerUse::ladder(n, false);
    default: return CheckerUse::ladder(n, true);
  }
}
int32_t ref_of(Use u, int n, const ref::Problem* ck, const char* who) {
  switch (u) {
    case CLEARANCE: return ref::clearance_refuse(ck, who);                                        // mkh_clearance, the setters
    case SWEEP: return ref::sweep_refuse(ck, who, n);                                             // mkh_swept_clearance (n >= 1 judged first)
    case TRACKING: return ref::sweep_refuse(ck, who, 0, ref::tracking_item(n));                   // trajectory_core, mkh_select_trajectory_candidates
    case REFINEMENT: return ref::sweep_refuse(ck, who, n < 1 ? 1 : n, ref::refinement_item(n));   // ladder_refine_call
    case LADDER: return ref::sweep_refuse(ck, who, n < 1 ? 1 : n, 0);                             // ladder_free_refuse, refined = false
    default: return ref::sweep_refuse(ck, who, n < 1 ? 1 : n, ref::refinement_item(n));           // ... refined = true
  }
}

void json_string(const std::string& s) {
  putchar('"');
  for (const char c : s) {
    if (c == '"' || c == '\\') putchar('\\');
    putchar(c);
  }
  putchar('"');
}

void cell(const char* group, const CheckerShape& s, Use u, int n) {
  const char* const who = "mkh_some_call";
  const ref::Model rm{s.nbody, s.nq};
  const ref::Problem rp{{s.n_pairs}, s.has_wide ? &rm : nullptr, s.convex_pairs, {s.n_cv}, &rm, s.sweep_rows, s.check_rows};
  ref::g_err.clear();
  const int32_t ref_rc = ref_of(u, n, &rp, who);
  const CheckerUse use = use_of(u, n);
  std::string err;
  const int32_t rc = mkh::checker_refuse(s, use, who, err);
  printf("{\"group\": \"%s\", \"use\": \"%s\", \"n_samples\": %d, \"n_pairs\": %d, \"n_cv\": %d, \"convex_pairs\": %d, \"has_wide\": %d, "
         "\"nbody\": %d, \"nq\": %d, \"max_batch\": %d, \"sweep_rows\": %lld, \"check_rows\": %lld, \"sweeps_edges\": %d, \"item_rows\": %d, "
         "\"rc\": %d, \"ref_rc\": %d, \"clearance_chunk\": %lld, \"sweep_chunk\": %lld, \"check_chunk\": %lld, \"err\": ",
         group, kUseName[u], n, s.n_pairs, s.n_cv, (int)s.convex_pairs, (int)s.has_wide, s.nbody, s.nq, s.max_batch, (long long)s.sweep_rows,
         (long long)s.check_rows, use.sweeps_edges, use.item_rows, rc, ref_rc, mkh::clearance_chunk(s), mkh::sweep_chunk(s, use),
         mkh::check_chunk(s, use));
  json_string(err);
  printf(", \"ref_err\": ");
  json_string(ref_rc ? ref::g_err : std::string());
  printf("}\n");
}

// every use at every sample count an entry point can pass on (below 1: the checker is judged first, with the count clamped),
// over the rows of both buffers around one item of that use
void matrix(const char* group, const CheckerShape& base) {
  for (int u = 0; u < N_USES; ++u)
    for (int n = -1; n <= 2; ++n) {
      if (u == CLEARANCE && n != 1) continue;                  // (no sample count)
      if (u == SWEEP && n < 1) continue;                       // (mkh_swept_clearance judges its count first)
      const int M = n < 1 ? 1 : n;
      const int items[2] = {1 + M, 1 + 2 * M};
      std::set<long long> sweep_rows = {0, M - 1, M, 10 * M + 1}, check_rows = {0};
      for (const int item : items)
        for (const long long r : {(long long)item - 1, (long long)item, 3LL * item + 1}) check_rows.insert(r);
      for (const long long sr : sweep_rows)
        for (const long long cr : check_rows) {
          CheckerShape s = base;
          s.sweep_rows = sr; s.check_rows = cr;
          cell(group, s, (Use)u, n);
        }
    }
}

}  // namespace

int main() {
  // n_pairs, n_cv, convex_pairs, has_wide, nbody, nq, max_batch, sweep_rows, check_rows
  matrix("analytic", CheckerShape{5, 0, false, true, 8, 6, 4, 0, 0});
  matrix("convex", CheckerShape{5, 3, true, true, 8, 6, 4, 0, 0});
  // the structural refusals, each under every use and every state of the buffers
  matrix("no_pairs", CheckerShape{0, 0, false, true, 8, 6, 4, 0, 0});
  matrix("no_wide", CheckerShape{5, 3, true, false, 8, 6, 4, 0, 0});
  matrix("convex_not_pre", CheckerShape{5, 0, true, true, 70, 69, 4, 0, 0});
  matrix("bodies_1170", CheckerShape{40, 3, true, true, 1170, 0, 4, 0, 0});        // 7 x 1170 = 8190 doubles: the last that fit
  matrix("bodies_1171", CheckerShape{40, 3, true, true, 1171, 0, 4, 0, 0});
  matrix("sweep_lds_fits", CheckerShape{40, 3, true, true, 1000, 397, 4, 0, 0});   // 7000 + 3 x 397 = 8191
  matrix("sweep_lds_over", CheckerShape{40, 3, true, true, 1000, 398, 4, 0, 0});   // 8194
  matrix("quarter_lds", CheckerShape{32, 3, true, true, 32, 700, 4, 0, 0});        // four slices of 224 + 2100: over; one would fit
  matrix("whole_lds", CheckerShape{33, 3, true, true, 32, 700, 4, 0, 0});
  return 0;
}
