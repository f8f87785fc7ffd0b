// The collision checker's host side: the entry points that run a checker handle on its own (mkh_clearance, mkh_swept_clearance),
// the ones that attach one or size its buffers, and the five stages the checked calls of minkhip.hip run on their Stager
// (checker_host.h).  Every decision that needs only integers — refusals, chunk sizes, launch geometry — is checker_plan.h's; here
// a handle is read into a CheckerShape, and launches are enqueued.
//
// A checker WITH general convex pairs (cylinder-box, ellipsoid-*, mesh hulls) has them evaluated by a pre-pass in front of the
// kernel that judges the rows, through a buffer of bounded rows: a stage then goes in chunks, pre-pass then consumer on each, the
// stream ordering the reuse of the buffer (run_chunks).  Without such pairs every stage but the clearance is the one launch it
// always was.
#include "checker_host.h"

#include <algorithm>
#include <cmath>

#include "motion_bound.h"

using namespace mkh;

static_assert(kStInCollision == MKH_ST_IN_COLLISION, "outer_launch.h: the bit clearance.hip sets");

static CheckerShape shape_of(const MkhProblem* ck) {
  return CheckerShape{ck->dev.n_pairs, ck->cv.n_cv, ck->convex_pairs, ck->d_wide != nullptr, ck->model->nbody, ck->model->nq,
                      ck->max_batch, ck->cv_sweep.rows, ck->cv_check.rows};
}
static int32_t refuse(const MkhProblem* ck, const char* who, const CheckerUse& u) { return checker_refuse(shape_of(ck), u, who, g_err); }

// total items in chunks of `per` (checker_plan.h's *_chunk of a use the refusal served: >= 1; anything else is an error here, never
// a loop that does not advance): enqueue(first, count) per chunk, until one fails.
template <class F>
static void run_chunks(Stager& st, long long total, long long per, F&& enqueue) {
  if (per < 1) { st.latch(hipErrorInvalidValue); return; }
  for (long long first = 0; first < total && st.ok(); first += per) enqueue(first, total - first < per ? total - first : per);
}

// The reach table of the checker's pair list on the host (motion_bound.h), filled once.
static const std::vector<double>& reach_of(MkhProblem* ck) {
  if (ck->h_reach.empty()) {
    const HostModel& m = *ck->model;
    auto ptr = [](const auto& v) { return v.empty() ? nullptr : v.data(); };
    const MotionModel mm{m.nbody, m.njnt, ptr(m.body_parentid), ptr(m.body_jntnum), ptr(m.body_jntadr), ptr(m.body_pos), ptr(m.jnt_type),
                         ptr(m.jnt_limited), ptr(m.jnt_pos), ptr(m.jnt_range), ptr(m.jnt_qpos0), ptr(m.geom_bodyid), ptr(m.geom_type),
                         ptr(m.geom_size), ptr(m.geom_pos), ptr(m.geom_dataid), ptr(m.mesh_vertadr), ptr(m.mesh_vertnum),
                         ptr(m.h_mesh_vert)};
    const int np = ck->dev.n_pairs;
    ck->h_reach.assign((size_t)np * m.njnt * 2 + 1, 0.0);      // (+ 1: a model without joints still has a table that is "filled")
    motion_reach(mm, np, ck->pair_geom.data(), ck->h_reach.data());
  }
  return ck->h_reach;
}

// ... and on the device, uploaded once (synchronous: a constant of the handle from here on).
static hipError_t upload_reach(MkhProblem* ck) {
  if (ck->d_reach) return hipSuccess;
  const std::vector<double>& h = reach_of(ck);
  hipError_t e = hipMalloc((void**)&ck->d_reach, h.size() * sizeof(double));
  if (e != hipSuccess) { ck->d_reach = nullptr; return e; }
  e = hipMemcpy(ck->d_reach, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(ck->d_reach); ck->d_reach = nullptr; }
  return e;
}
static int32_t ensure_reach(MkhProblem* ck) {
  HIP_OK(upload_reach(ck));
  return MKH_OK;
}

namespace mkh {

int32_t refuse_checker(const MkhProblem* p, const char* who) {
  if (p->checker)
    return fail(MKH_E_INVALID, "%s: a collision checker is attached to this problem (mkh_problem_set_collision_check) and this call would "
                               "not run it: mkh_solve_multistart, mkh_solve_multistart_set and mkh_solve_goalset are the calls that "
                               "do — detach it first", who);
  return MKH_OK;
}

int32_t sweep_refuse_for(const MkhProblem* p, const MkhProblem* ck, const char* who, const CheckerUse& u) {
  if (!ck) return fail(MKH_E_INVALID, "%s: null checker", who);
  if (ck->device != p->device)
    return fail(MKH_E_INVALID, "%s: the checker lives on device %d, the problem on device %d", who, ck->device, p->device);
  if (ck->model != p->model) return fail(MKH_E_INVALID, "%s: the checker belongs to another MkhModel than the problem", who);
  return refuse(ck, who, u);
}

// ---- clearance (include/minkhip.h "THE RULE OF CLEARANCE"; kernel: clearance.hip, in front of it convex_pre.hip's for the pairs
// without an analytic routine): in chunks of the checker's max_batch — its buffer of pre-evaluated convex pairs holds that many rows
void clearance_rows(Stager& st, MkhProblem* ck, size_t N, const double* d_q, double* margin, int32_t* pair, int32_t* n_violated,
                    double* distance, int32_t* status) {
  const size_t nq = ck->model->nq, np = ck->dev.n_pairs;
  run_chunks(st, (long long)N, clearance_chunk(shape_of(ck)), [&](long long first, long long count) {
    const size_t r0 = (size_t)first;
    const int n = (int)count;
    const double* const q = d_q + r0 * nq;
    if (ck->cv.n_cv > 0) st.latch(launch_convex_pre(st.stream, ck->d_wide, ck->cv, n, q, ck->d_cv));
    ST_LAUNCH(st, launch_clearance(st.stream, ck->d_wide, ck->model->nbody, (int)np, ck->cv.n_cv, ck->d_cv, n, q, margin ? margin + r0 : nullptr,
                                   pair ? pair + r0 : nullptr, n_violated ? n_violated + r0 : nullptr,
                                   distance ? distance + r0 * np : nullptr, status ? status + r0 : nullptr));
  });
}

// ---- swept clearance (include/minkhip.h "THE RULE OF THE SWEEP"; kernel: sweep.hip): general convex pairs in chunks of
// floor(sweep_rows / M) edges, convex_sweep_kernel then sweep_kernel on each
void sweep_edges(Stager& st, const MkhProblem* ck, SweepArgs a) {
  const int nbody = ck->model->nbody, nq = ck->model->nq, np = ck->dev.n_pairs;
  if (ck->cv.n_cv == 0) {
    ST_LAUNCH(st, launch_sweep(st.stream, ck->d_wide, nbody, nq, np, a));
    return;
  }
  a.cv = ck->cv_sweep.d; a.n_cv = ck->cv.n_cv;
  const char* const ipw_env = dbg_env("MKH_DEBUG_CONVEX_SWEEP_IPW");       // (experiment builds: items per wavefront of the pre-pass)
  const int ipw = ipw_env ? atoi(ipw_env) : 0;
  run_chunks(st, a.N, sweep_chunk(shape_of(ck), CheckerUse::sweep(a.M)), [&](long long first, long long count) {
    a.first = first; a.count = count;
    ST_LAUNCH(st, launch_convex_sweep(st.stream, ck->d_wide, ck->cv, a, ipw));
    ST_LAUNCH(st, launch_sweep(st.stream, ck->d_wide, nbody, nq, np, a));
  });
}

// ---- certified sweep (include/minkhip.h "THE RULE OF THE CERTIFIED SWEEP"; kernel: certified_sweep.hip): one launch in every mode —
// a checker with general convex pairs never gets here (CheckerUse::certified)
void certify_edges(Stager& st, MkhProblem* ck, CertifiedArgs a) {
  if (!st.ok()) return;
  st.latch(upload_reach(ck));
  a.reach = ck->d_reach;
  ST_LAUNCH(st, launch_certified_sweep(st.stream, ck->d_wide, ck->model->nbody, ck->model->nq, ck->dev.n_pairs, a));
}

// ---- checked candidate tracking (kernels: trajectory_free.hip): general convex pairs in chunks of floor(check_rows / (1 + M))
// rows, convex_check_kernel then the check on each — the pre-pass reads a chunk's status in front of the check that ORs into it
void tmf_check(Stager& st, const MkhProblem* ck, int B, int S, int T, int M, const double* q_all, const int32_t* cv_all, int32_t* st_all,
               double* nm_all, double* em_all) {
  const int nbody = ck->model->nbody, nq = ck->model->nq, np = ck->dev.n_pairs;
  if (ck->cv.n_cv == 0) {
    ST_LAUNCH(st, launch_tmf_check(st.stream, ck->d_wide, nbody, nq, np, B, S, T, M, q_all, cv_all, st_all, nm_all, em_all));
    return;
  }
  CvCheckArgs a{};
  a.mode = kCvCheckTrack; a.M = M; a.R = (long long)B * S; a.q_all = q_all; a.converged = cv_all; a.status = st_all;
  run_chunks(st, (long long)B * S * T, check_chunk(shape_of(ck), CheckerUse::tracking(M)), [&](long long first, long long count) {
    a.first = first; a.count = count;
    const CvChunk c{first, count, ck->cv_check.d, ck->cv.n_cv};
    ST_LAUNCH(st, launch_convex_check(st.stream, ck->d_wide, ck->cv, a, ck->cv_check.d));
    ST_LAUNCH(st, launch_tmf_check(st.stream, ck->d_wide, nbody, nq, np, B, S, T, M, q_all, cv_all, st_all, nm_all, em_all, c));
  });
}

// ---- the refinement pass "with a checker" (kernels: ladder_refine_free.hip): general convex pairs in chunks of
// floor(check_rows / (1 + 2M)) instances, convex_check_kernel — once for all the slots of the check — then the check on each
void lr_check_step(Stager& st, const MkhProblem* ck, int B, int T, int M, int ct, int cdir, const LrWork& w, double* trip) {
  const int nbody = ck->model->nbody, nq = ck->model->nq, np = ck->dev.n_pairs;
  if (ck->cv.n_cv == 0) {
    ST_LAUNCH(st, launch_lr_check(st.stream, ck->d_wide, nbody, nq, np, B, T, M, ct, cdir, w, trip));
    return;
  }
  CvCheckArgs a{};
  a.mode = kCvCheckRefine; a.M = M; a.T = T; a.ct = ct; a.cdir = cdir;
  a.r = w.r; a.x = w.x; a.r_trk = w.r_trk; a.xst = w.xst; a.xcv = w.xcv; a.bad = w.bad;
  run_chunks(st, B, check_chunk(shape_of(ck), CheckerUse::refinement(M)), [&](long long first, long long count) {
    a.first = first; a.count = count;
    const CvChunk c{first, count, ck->cv_check.d, ck->cv.n_cv};
    ST_LAUNCH(st, launch_convex_check(st.stream, ck->d_wide, ck->cv, a, ck->cv_check.d));
    ST_LAUNCH(st, launch_lr_check(st.stream, ck->d_wide, nbody, nq, np, B, T, M, ct, cdir, w, trip, c));
  });
}

}  // namespace mkh

// `buf` resized to `rows` rows of the checker's general convex pairs (0, or a checker without such pairs: no memory), on behalf
// of the setter `who`.
static int32_t cv_rows_resize(MkhProblem* ck, CvRows& buf, int64_t rows, const char* who) {
  if (const int32_t rc = refuse(ck, who, CheckerUse::clearance_only())) return rc;
  const uint64_t width = (uint64_t)ck->cv.n_cv * sizeof(double);
  if (width > 0 && (uint64_t)rows > (uint64_t)0x7fffffffffffLL / width)
    return fail(MKH_E_LIMIT, "%s: rows = %lld x %d general convex pairs x 8 bytes overflows", who, (long long)rows, ck->cv.n_cv);
  HIP_OK(hipSetDevice(ck->model->device));
  HIP_OK(hipDeviceSynchronize());                              // (a launch in flight may still read the old buffer)
  (void)hipFree(buf.d);
  buf = CvRows{};
  if (rows > 0 && width > 0) {
    // (zeroed: a row the pre-pass skips is never judged by what stands here, and what is read of it is at least a number)
    HIP_OK(hipMalloc((void**)&buf.d, (size_t)rows * width));
    HIP_OK(hipMemset(buf.d, 0, (size_t)rows * width));
    HIP_OK(hipDeviceSynchronize());
  }
  buf.rows = rows;
  return MKH_OK;
}

extern "C" {

int32_t mkh_clearance(MkhProblem* ck, int32_t N, const double* q_rows, const MkhClearanceIO* io, int32_t flags, void* hip_stream) {
  const char* const who = "mkh_clearance";
  if (!ck) return fail(MKH_E_INVALID, "null problem");
  if (N < 1) return fail(MKH_E_INVALID, "%s: N = %d must be >= 1", who, N);
  if (flags & ~MKH_FLAG_DEVICE_PTRS) return fail(MKH_E_INVALID, "%s: flags = %d: only MKH_FLAG_DEVICE_PTRS is accepted", who, flags);
  if (!q_rows || !io || !io->margin || !io->pair || !io->n_violated)
    return fail(MKH_E_INVALID, "%s: q_rows, io and its outputs margin, pair, n_violated are required", who);
  if (const int32_t rc = refuse(ck, who, CheckerUse::clearance_only())) return rc;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  HIP_OK(hipSetDevice(ck->model->device));
  Stager st{ck, (hipStream_t)hip_stream, devp, "clearance"};
  const size_t Nz = N, nq = ck->model->nq, np = ck->dev.n_pairs, f8 = sizeof(double), i4 = sizeof(int32_t);
  const double* const d_q = st.up(WS_C_Q, q_rows, Nz * nq);
  double *o_m = io->margin, *o_d = io->distance;
  int32_t *o_p = io->pair, *o_n = io->n_violated;
  if (!devp) {
    o_m = st.f64(WS_OUT_LEN, Nz);
    o_p = st.i32(WS_OUT_PICK, 2 * Nz); o_n = o_p ? o_p + Nz : nullptr;
    if (o_d) o_d = st.f64(WS_OUT_Q, Nz * np);
  }
  if (!st.ok()) return st.finish();
  clearance_rows(st, ck, Nz, d_q, o_m, o_p, o_n, o_d, nullptr);
  if (devp) return st.finish();
  st.down(io->margin, o_m, Nz * f8);
  st.down(io->pair, o_p, Nz * i4);
  st.down(io->n_violated, o_n, Nz * i4);
  st.down(io->distance, o_d, Nz * np * f8);
  return st.finish();
}

int32_t mkh_problem_set_collision_check(MkhProblem* p, MkhProblem* checker) {
  const char* const who = "mkh_problem_set_collision_check";
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (checker) {
    if (checker->device != p->device)
      return fail(MKH_E_INVALID, "%s: the checker lives on device %d, the problem on device %d", who, checker->device, p->device);
    if (checker->model != p->model) return fail(MKH_E_INVALID, "%s: the checker belongs to another MkhModel than the problem", who);
    if (const int32_t rc = refuse(checker, who, CheckerUse::clearance_only())) return rc;
  }
  p->checker = checker;
  return MKH_OK;
}

int32_t mkh_problem_set_sweep_rows(MkhProblem* ck, int64_t rows) {
  const char* const who = "mkh_problem_set_sweep_rows";
  if (!ck) return fail(MKH_E_INVALID, "null problem");
  if (rows < 0) return fail(MKH_E_INVALID, "%s: rows = %lld must be >= 0", who, (long long)rows);
  return cv_rows_resize(ck, ck->cv_sweep, rows, who);
}

int32_t mkh_problem_set_check_rows(MkhProblem* ck, int64_t rows) {
  const char* const who = "mkh_problem_set_check_rows";
  if (!ck) return fail(MKH_E_INVALID, "null problem");
  if (rows < 0) return fail(MKH_E_INVALID, "%s: rows = %lld must be >= 0", who, (long long)rows);
  return cv_rows_resize(ck, ck->cv_check, rows, who);
}

int32_t mkh_swept_clearance(MkhProblem* ck, int32_t N, const double* q_from, const double* q_to, int32_t n_samples,
                            const MkhSweptClearanceIO* io, int32_t flags, void* hip_stream) {
  const char* const who = "mkh_swept_clearance";
  if (!ck) return fail(MKH_E_INVALID, "null problem");
  if (N < 1) return fail(MKH_E_INVALID, "%s: N = %d must be >= 1", who, N);
  if (n_samples < 1) return fail(MKH_E_INVALID, "%s: n_samples = %d must be >= 1", who, n_samples);
  if (flags & ~MKH_FLAG_DEVICE_PTRS) return fail(MKH_E_INVALID, "%s: flags = %d: only MKH_FLAG_DEVICE_PTRS is accepted", who, flags);
  if (!q_from || !q_to || !io || !io->margin || !io->sample || !io->pair)
    return fail(MKH_E_INVALID, "%s: q_from, q_to, io and its outputs margin, sample, pair are required", who);
  if (const int32_t rc = refuse(ck, who, CheckerUse::sweep(n_samples))) return rc;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  HIP_OK(hipSetDevice(ck->model->device));
  Stager st{ck, (hipStream_t)hip_stream, devp, "swept_clearance"};
  const size_t Nz = N, nq = ck->model->nq;
  SweepArgs a{};
  a.mode = kSweepPairs; a.M = n_samples; a.N = N;
  a.from = st.up(WS_C_Q, q_from, Nz * nq);
  a.to = st.up(WS_SW_TO, q_to, Nz * nq);
  a.margin = io->margin; a.sample = io->sample; a.pair = io->pair;
  if (!devp) {
    a.margin = st.f64(WS_OUT_LEN, Nz);
    a.sample = st.i32(WS_OUT_PICK, 2 * Nz); a.pair = a.sample ? a.sample + Nz : nullptr;
  }
  if (!st.ok()) return st.finish();
  sweep_edges(st, ck, a);
  if (devp) return st.finish();
  st.down(io->margin, a.margin, Nz * sizeof(double));
  st.down(io->sample, a.sample, Nz * sizeof(int32_t));
  st.down(io->pair, a.pair, Nz * sizeof(int32_t));
  return st.finish();
}

int32_t mkh_checker_motion_reach(MkhProblem* ck, double* out) {
  const char* const who = "mkh_checker_motion_reach";
  if (!ck) return fail(MKH_E_INVALID, "null problem");
  if (!out) return fail(MKH_E_INVALID, "%s: out is required", who);
  if (ck->dev.n_pairs < 1) return fail(MKH_E_INVALID, "%s: the checker has no collision pairs (a problem with CollisionAvoidanceLimits is one)", who);
  const std::vector<double>& h = reach_of(ck);
  std::copy(h.begin(), h.begin() + (size_t)ck->dev.n_pairs * ck->model->njnt * 2, out);
  return MKH_OK;
}

// (include/minkhip.h "THE RULE OF THE CERTIFIED SWEEP"; kernel: certified_sweep.hip): one launch
int32_t mkh_certified_sweep(MkhProblem* ck, int32_t N, const double* q_from, const double* q_to, double resolution, int32_t max_samples,
                            const MkhCertifiedSweepIO* io, int32_t flags, void* hip_stream) {
  const char* const who = "mkh_certified_sweep";
  if (!ck) return fail(MKH_E_INVALID, "null problem");
  if (N < 1) return fail(MKH_E_INVALID, "%s: N = %d must be >= 1", who, N);
  if (!std::isfinite(resolution) || !(resolution > 0.0))
    return fail(MKH_E_INVALID, "%s: resolution = %g must be finite and > 0", who, resolution);
  if (max_samples < 1 || max_samples > 4096) return fail(MKH_E_INVALID, "%s: max_samples = %d must be in [1, 4096]", who, max_samples);
  if (flags & ~MKH_FLAG_DEVICE_PTRS) return fail(MKH_E_INVALID, "%s: flags = %d: only MKH_FLAG_DEVICE_PTRS is accepted", who, flags);
  if (!q_from || !q_to || !io || !io->margin || !io->sample || !io->pair || !io->lower_bound || !io->segment || !io->bound_pair ||
      !io->n_samples || !io->motion || !io->capped || !io->verdict)
    return fail(MKH_E_INVALID, "%s: q_from, q_to, io and its ten outputs are required", who);
  if (const int32_t rc = refuse(ck, who, CheckerUse::certified())) return rc;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  HIP_OK(hipSetDevice(ck->model->device));
  if (const int32_t rc = ensure_reach(ck)) return rc;
  Stager st{ck, (hipStream_t)hip_stream, devp, "certified_sweep"};
  const size_t Nz = N, nq = ck->model->nq, f8 = sizeof(double), i4 = sizeof(int32_t);
  CertifiedArgs a{};
  a.mode = kSweepPairs; a.N = N; a.resolution = resolution; a.max_samples = max_samples;
  a.from = st.up(WS_C_Q, q_from, Nz * nq);
  a.to = st.up(WS_SW_TO, q_to, Nz * nq);
  a.margin = io->margin; a.lower_bound = io->lower_bound; a.motion = io->motion;
  a.sample = io->sample; a.pair = io->pair; a.segment = io->segment; a.bound_pair = io->bound_pair;
  a.n_samples = io->n_samples; a.capped = io->capped; a.verdict = io->verdict;
  if (!devp) {                                                 // (OUT_LEN: margin | lower_bound | motion; OUT_PICK: the seven integers)
    double* const f = st.f64(WS_OUT_LEN, 3 * Nz);
    int32_t* const i = st.i32(WS_OUT_PICK, 7 * Nz);
    if (f && i) {
      a.margin = f; a.lower_bound = f + Nz; a.motion = f + 2 * Nz;
      a.sample = i; a.pair = i + Nz; a.segment = i + 2 * Nz; a.bound_pair = i + 3 * Nz;
      a.n_samples = i + 4 * Nz; a.capped = i + 5 * Nz; a.verdict = i + 6 * Nz;
    }
  }
  if (!st.ok()) return st.finish();
  certify_edges(st, ck, a);
  if (devp) return st.finish();
  st.down(io->margin, a.margin, Nz * f8); st.down(io->lower_bound, a.lower_bound, Nz * f8); st.down(io->motion, a.motion, Nz * f8);
  st.down(io->sample, a.sample, Nz * i4); st.down(io->pair, a.pair, Nz * i4); st.down(io->segment, a.segment, Nz * i4);
  st.down(io->bound_pair, a.bound_pair, Nz * i4); st.down(io->n_samples, a.n_samples, Nz * i4); st.down(io->capped, a.capped, Nz * i4);
  st.down(io->verdict, a.verdict, Nz * i4);
  return st.finish();
}

}  // extern "C"
