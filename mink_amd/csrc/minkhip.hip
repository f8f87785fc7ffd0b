// libminkhip.so — host side of the C ABI declared in include/minkhip.h.
//
// mkh_model_create / mkh_problem_create upload what problem_plan.hip plans on the host — the mjModel
// fields and the Task/Limit plugin objects of one mink.solve_ik call site, flattened into lane tables
// (mkh_types.h); the outer-loop entry points run their loops through the plain solve of solve_host.hip.
#include "../../include/minkhip.h"

#include <hip/hip_runtime.h>
#include <cstdlib>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "checker_host.h"
#include "collide_dev.h"
#include "host_internal.h"
#include "lie_dev.h"
#include "outer_launch.h"
#include "problem_plan.h"
#include "solve_host.h"

namespace mkh {
// q_out = q ⊕ v·dt (mj_integratePos; Configuration.integrate, mink/configuration.py:214-226).
// One thread per (problem, joint).
__global__ __launch_bounds__(256) void integrate_kernel(const DeviceProblem P, int B, const double* __restrict__ q,
                                                        const double* __restrict__ v, double dt,
                                                        double* __restrict__ q_out) {
  const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)B * P.njnt;
  if (tid >= total) return;
  const int b = (int)(tid / P.njnt), j = (int)(tid % P.njnt);
  const int jt = P.jnt_i[j * JI_COUNT + JI_TYPE];
  int qa = P.jnt_i[j * JI_COUNT + JI_QADR];
  int va = P.jnt_i[j * JI_COUNT + JI_DADR];
  const double* qi = q + (size_t)b * P.nq;
  const double* vi = v + (size_t)b * P.nv;
  double* qo = q_out + (size_t)b * P.nq;
  if (jt == JNT_HINGE || jt == JNT_SLIDE) { qo[qa] = qi[qa] + dt * vi[va]; return; }
  if (jt == JNT_FREE) {
    for (int i = 0; i < 3; ++i) qo[qa + i] = qi[qa + i] + dt * vi[va + i];
    qa += 3; va += 3;
  }
  // mju_quatIntegrate: q ← normalize(q) ⊗ axisangle(v̂, dt·|v|)
  V3 w{vi[va], vi[va + 1], vi[va + 2]};
  const double n = sqrt(dot(w, w));
  V3 ax = (n < 1e-15) ? V3{1.0, 0.0, 0.0} : (1.0 / n) * w;
  const double ang = dt * n;
  Q4 qr = (ang == 0.0) ? Q4{1, 0, 0, 0} : axis_angle(ax, ang);
  Q4 q0 = qnormalize(Q4{qi[qa], qi[qa + 1], qi[qa + 2], qi[qa + 3]});
  Q4 r = qmul(q0, qr);
  qo[qa] = r.w; qo[qa + 1] = r.x; qo[qa + 2] = r.y; qo[qa + 3] = r.z;
}

// mkh_last_error's text and its writer (host_internal.h)
thread_local std::string g_err;
int32_t fail(int32_t code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
}
using namespace mkh;

// MKH_FLAG_UNWIND_TURNS in front of an entry point that has no distinct-set selection to unwind for (include/minkhip.h).
static int32_t refuse_unwind(int32_t flags, const char* who) {
  if (flags & MKH_FLAG_UNWIND_TURNS)
    return fail(MKH_E_INVALID, kUnwindRefusalFmt, who);
  return MKH_OK;
}

template <class T>
static hipError_t upload(const std::vector<T>& h, T** d) {
  *d = nullptr;
  const size_t n = h.empty() ? 1 : h.size();
  hipError_t e = hipMalloc((void**)d, n * sizeof(T));
  if (e != hipSuccess) return e;
  if (!h.empty()) e = hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  return e;
}

// A seed table (include/minkhip.h "Seed tables"): device memory of its own — nothing of the problem that made it is kept.
struct MkhSeedTable {
  int device = 0;
  int N = 0, nq = 0, njnt = 0, n_frame = 0;
  double* d_q = nullptr;             // (N, nq)
  double* d_keys = nullptr;          // (n_frame·7, N): seed_table.hip
  double* d_w = nullptr;             // (2·n_frame): position weights, orientation weights
};




extern "C" {

int32_t mkh_version(void) { return MKH_VERSION; }
const char* mkh_last_error(void) { return g_err.c_str(); }

int32_t mkh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t mkh_model_create(const MkhFlatModel* h, int32_t device, MkhModel** out) {
  if (!h || !out) return fail(MKH_E_INVALID, "null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MKH_E_NOGPU, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(MKH_E_INVALID, "device %d out of range (%d visible)", device, ndev);
  HIP_OK(hipSetDevice(device));
  MkhModel* m = new MkhModel();
  m->device = device;
  if (const int32_t rc = plan_model(h, *m, g_err)) { delete m; return rc; }
  hipError_t e = upload(m->body_f, &m->d_body_f);
  if (e == hipSuccess) e = upload(m->body_i, &m->d_body_i);
  if (e == hipSuccess) e = upload(m->jnt_f, &m->d_jnt_f);
  if (e == hipSuccess) e = upload(m->jnt_i, &m->d_jnt_i);
  if (e == hipSuccess) e = upload(m->dof_i, &m->d_dof_i);
  if (e == hipSuccess) e = upload(m->dof_f, &m->d_dof_f);
  hipDeviceProp_t prop;
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
  if (e == hipSuccess && !m->h_mesh_vert.empty()) e = upload(m->h_mesh_vert, &m->d_mesh_vert);
  if (e != hipSuccess) { mkh_model_destroy(m); return fail(MKH_E_HIP, "model upload: %s", hipGetErrorString(e)); }
  m->num_cus = prop.multiProcessorCount;
  *out = m;
  return MKH_OK;
}

void mkh_model_destroy(MkhModel* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipFree(m->d_body_f); (void)hipFree(m->d_body_i); (void)hipFree(m->d_jnt_f); (void)hipFree(m->d_jnt_i);
  (void)hipFree(m->d_dof_i); (void)hipFree(m->d_dof_f); (void)hipFree(m->d_mesh_vert);
  m->small.release();
  delete m;
}

int32_t mkh_problem_create(MkhModel* m, const MkhProblemDesc* d, int32_t max_batch, MkhProblem** out) {
  return mkh_problem_create_diag(m, d, max_batch, 0, out);
}

// The experiment switches of problem creation (problem_plan.h PlanSwitches; tools/README.md): read at every create, in experiment
// builds only — dbg_env is a constant nullptr in the product library.
static PlanSwitches plan_switches() {
  PlanSwitches s;
  if (const char* cap = dbg_env("MKH_DEBUG_MAX_ROWS")) s.max_rows = atoi(cap);
  s.wood_always = dbg_env("MKH_DEBUG_WOOD_ALWAYS") != nullptr;
  s.no_com_w3 = dbg_env("MKH_DEBUG_NO_COM_W3") != nullptr;
  s.no_tight_rows = dbg_env("MKH_DEBUG_NO_TIGHT_ROWS") != nullptr;
  s.no_tight_generic = dbg_env("MKH_DEBUG_NO_TIGHT_GENERIC") != nullptr;
  s.no_pair_rows = dbg_env("MKH_DEBUG_NO_PAIR_ROWS") != nullptr;
  s.no_convex_split = dbg_env("MKH_DEBUG_NO_CONVEX_SPLIT") != nullptr;
  return s;
}

// A planned problem on the device: the only place that allocates and fills descriptor memory.  Every array a descriptor points to
// goes into p->owned; the descriptors are copied once, after their pointer fields are patched.  One error path: the caller
// destroys the handle, which frees whatever was allocated.
static int32_t upload_problem(MkhProblem* p, const ProblemPlan& plan) {
  const MkhModel* m = p->model;
  hipError_t e = hipSuccess;
  auto up = [&](const auto& v) {                       // a host vector, owned by the handle
    typename std::decay_t<decltype(v)>::value_type* dp = nullptr;
    if (e == hipSuccess) e = upload(v, &dp);
    if (dp) p->owned.push_back(dp);
    return dp;
  };
  auto alloc = [&](auto** out, size_t bytes) { if (e == hipSuccess) e = hipMalloc((void**)out, bytes); };
  auto put = [&](auto** out, const void* src, size_t bytes) {
    alloc(out, bytes);
    if (e == hipSuccess) e = hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice);
  };
  // mesh geoms: the hull's vertices in the model's device array
  std::vector<CollisionPairDev> pairs = plan.pairs;
  for (size_t k = 0; k < pairs.size(); ++k) {
    if (plan.pair_vert[2 * k] >= 0) pairs[k].vert1 = m->d_mesh_vert + plan.pair_vert[2 * k];
    if (plan.pair_vert[2 * k + 1] >= 0) pairs[k].vert2 = m->d_mesh_vert + plan.pair_vert[2 * k + 1];
  }
  DeviceProblem& P = p->dev;
  P = plan.dev;
  if (!plan.sel.wide_only) {
    P.body_f = m->d_body_f; P.body_i = m->d_body_i; P.jnt_f = m->d_jnt_f; P.jnt_i = m->d_jnt_i;
    P.dof_i = m->d_dof_i; P.dof_f = m->d_dof_f;
    P.frame = up(plan.ft); P.posture_cost = up(plan.pcost); P.cfg_lower = up(plan.clo); P.cfg_upper = up(plan.chi);
    P.vel_limit = up(plan.vlim); P.pairs = up(pairs); P.cull = plan.sel.use_cull ? up(plan.culls) : nullptr;
    P.dense_cost = up(plan.dcost); P.dense_wgain = up(plan.dwgain);
    if (plan.lane_class) {
      // (the lane kernel and the one-row builds of the row kernel read the small descriptor, the two-row build the large one)
      LaneProblem lp1;
      if (plan.lane_class != 32) lane_problem_narrow(plan.lane, lp1);
      if (plan.lane_class == 32) put(&p->d_lane, &plan.lane, sizeof(LaneProblem2));
      else put(&p->d_lane, &lp1, sizeof(LaneProblem));
    }
    if (plan.tight) {
      DeviceProblem T = plan.dev_tight;                // (planned before the convex split: no pre-evaluated contacts)
      T.body_f = P.body_f; T.body_i = P.body_i; T.jnt_f = P.jnt_f; T.jnt_i = P.jnt_i; T.dof_i = P.dof_i; T.dof_f = P.dof_f;
      T.frame = P.frame; T.posture_cost = P.posture_cost; T.cfg_lower = P.cfg_lower; T.cfg_upper = P.cfg_upper;
      T.vel_limit = P.vel_limit; T.pairs = P.pairs; T.cull = P.cull; T.dense_cost = P.dense_cost; T.dense_wgain = P.dense_wgain;
      put(&p->d_dev_tight, &T, sizeof(DeviceProblem));
      alloc(&p->d_status_tight, (size_t)p->max_batch * sizeof(int32_t));
    }
  }
  if (plan.wide.built) {
    const WidePlan& wp = plan.wide;
    WideProblem& W = p->wide;
    W = wp.W;
    W.level_start = up(m->level_start); W.level_body = up(m->level_body); W.body_parent = up(m->body_parentid);
    W.body_jntadr = up(m->jntadr0); W.body_jntnum = up(m->body_jntnum); W.body_last = up(m->subtree_last);
    W.body_inrobot = up(m->in_robot); W.body_pos = up(m->body_pos); W.body_quat = up(m->body_quat); W.body_ipos = up(m->body_ipos);
    W.body_mass = up(m->body_mass); W.body_stmass = up(m->body_subtreemass); W.jnt_type = up(m->jnt_type);
    W.jnt_qadr = up(m->jnt_qposadr); W.jnt_dadr = up(m->jnt_dofadr); W.jnt_axis = up(m->jnt_axis); W.jnt_pos = up(m->jnt_pos);
    W.jnt_qpos0 = up(m->jnt_qpos0); W.dof_jnt = up(m->dof_jntid); W.dof_kind = up(m->dof_kind); W.dof_k = up(m->dof_k);
    W.dof_body = up(m->dof_bodyid); W.dof_qadr = up(m->dof_qadr); W.dof_lo = up(m->dof_lo); W.dof_hi = up(m->dof_hi);
    W.chain = up(m->chain);
    W.frame = up(plan.ft); W.posture_cost = up(wp.pcost); W.dense_cost = up(plan.dcost); W.dense_wgain = up(plan.dwgain);
    W.cfg_lower = up(wp.clo); W.cfg_upper = up(wp.chi); W.vel_limit = up(wp.vlim); W.pairs = up(pairs);
    W.cull = wp.use_cull ? up(plan.culls) : nullptr;
    alloc(&W.ws, (size_t)wp.ws_doubles * 8);
    if (W.ws) p->owned.push_back(W.ws);
    // the redo queue: every entry empty (−1), head and tail behind it
    alloc(&W.redo_queue, ((size_t)wp.redo_cap + 4) * sizeof(int32_t));
    if (W.redo_queue) p->owned.push_back(W.redo_queue);
    if (e == hipSuccess) e = hipMemset(W.redo_queue, 0xff, (size_t)wp.redo_cap * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(W.redo_queue + wp.redo_cap, 0, 4 * sizeof(int32_t));
    W.redo_ctr = reinterpret_cast<uint32_t*>(W.redo_queue + wp.redo_cap);
    put(&p->d_wide, &W, sizeof(WideProblem));
    if (!p->d_status_tight) alloc(&p->d_status_tight, (size_t)p->max_batch * sizeof(int32_t));
  }
  if (plan.n_cv > 0) {
    // general convex pairs of plain solves: the chains convex_contacts_kernel walks and the contacts it leaves for the solve
    p->cv = mkh::CvPre{plan.n_cv, up(plan.cv_pair), up(plan.cv_adr), up(plan.cv_chain)};
    alloc(&p->d_cv, (size_t)p->max_batch * plan.n_cv * 7 * sizeof(double));
    P.cv_contacts = p->d_cv;
  }
  if (!plan.sel.wide_only) put(&p->d_dev, &P, sizeof(DeviceProblem));
  alloc(&p->d_taps, sizeof(TapArgs));
  alloc(&p->d_work, 128);
  if (e == hipSuccess) e = hipMemset(p->d_work, 0, 128);
  if (e == hipSuccess) e = hipDeviceSynchronize();   // (hipMemset may return before the fill has run; launches may come on any stream)
  if (e != hipSuccess) return fail(MKH_E_HIP, "problem upload: %s", hipGetErrorString(e));
  return MKH_OK;
}

int32_t mkh_problem_create_diag(MkhModel* m, const MkhProblemDesc* d, int32_t max_batch, int32_t diag, MkhProblem** out) {
  if (!m || !d || !out) return fail(MKH_E_INVALID, "null argument");
  *out = nullptr;
  ProblemPlan plan;
  if (const int32_t rc = plan_problem(*m, *d, diag, max_batch, m->num_cus, plan_switches(), plan, g_err)) return rc;
  HIP_OK(hipSetDevice(m->device));
  MkhProblem* p = new MkhProblem();
  static_cast<ProblemSelect&>(*p) = plan.sel;
  p->model = m;
  p->device = m->device;
  p->max_batch = max_batch;
  p->diag = diag;
  p->pair_geom = plan.pair_geom;
  if (const int32_t rc = upload_problem(p, plan)) { mkh_problem_destroy(p); return rc; }
  if (p->wide_only) {
    snprintf(p->last_kernel, sizeof(p->last_kernel), "ik_wide_kernel");
    p->last_grid = p->wide_grid; p->last_lds = p->wide_lds; p->last_nt = p->wide.nv + p->wide.max_rows; p->last_block = kWideThreads;
  }
  *out = p;
  return MKH_OK;
}

void mkh_problem_destroy(MkhProblem* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  for (void* w : p->owned) (void)hipFree(w);
  (void)hipFree(p->d_dev); (void)hipFree(p->d_taps); (void)hipFree(p->d_work);
  (void)hipFree(p->d_lane); (void)hipFree(p->d_warm);
  (void)hipFree(p->d_cv); (void)hipFree(p->cv_sweep.d); (void)hipFree(p->cv_check.d); (void)hipFree(p->d_reach); (void)hipFree(p->d_dev_tight); (void)hipFree(p->d_status_tight);
  (void)hipFree(p->d_clk);
  (void)hipFree(p->d_wide);
  for (GrowBuf& g : p->stage) g.release();
  for (GrowBuf& g : p->ws) g.release();
  p->small.release();
  if (p->st_in) (void)hipStreamDestroy(p->st_in);
  if (p->st_out) (void)hipStreamDestroy(p->st_out);
  if (p->ev_start) (void)hipEventDestroy(p->ev_start);
  for (int i = 0; i < 4; ++i) { if (p->ev_in[i]) (void)hipEventDestroy(p->ev_in[i]); if (p->ev_k[i]) (void)hipEventDestroy(p->ev_k[i]); }
  delete p;
}

const char* mkh_problem_last_kernel(const MkhProblem* p) { return p ? p->last_kernel : ""; }
int32_t mkh_problem_num_task_rows(const MkhProblem* p) { return p ? p->dev.n_rows_tap : 0; }
int32_t mkh_problem_num_collision_pairs(const MkhProblem* p) { return p ? p->dev.n_pairs : 0; }

// What every outer-loop call refuses about its inputs (a plain solve: solve_plan.h solve_refusal), in this order: a NULL q, a threshold loop without a frame task to test (`until_who`
// names the entry point; NULL: no thresholds), a NULL target of a task group the problem has, and — for the entry points that
// cannot serve plugin rows at all — those (`no_plugin` ends the message: what besides the fused loop they rule out; NULL: the
// caller has its own rules for them).
static int32_t refuse_inputs(const DeviceProblem& P, const double* q, const double* frame_targets, const double* posture_target,
                             const double* com_target, const char* until_who, const char* no_plugin) {
  if (!q) return fail(MKH_E_INVALID, "%s", kNullInputText[A_Q]);
  if (until_who && P.n_frame < 1) return fail(MKH_E_INVALID, kUntilNoFrameFmt, until_who);
  if (P.n_frame > 0 && !frame_targets) return fail(MKH_E_INVALID, "%s", kNullInputText[A_FT]);
  if (P.n_posture > 0 && !posture_target) return fail(MKH_E_INVALID, "%s", kNullInputText[A_PT]);
  if (P.n_com > 0 && !com_target) return fail(MKH_E_INVALID, "%s", kNullInputText[A_CT]);
  if (no_plugin && (P.n_dense_rows || P.n_dense_limit_rows || P.dense_box))
    return fail(MKH_E_INVALID, "dense (plugin) rows are evaluated by the caller at q: no fused loop, no %s", no_plugin);
  return MKH_OK;
}


}  // extern "C"

// The per-qpos-address seeding table and the joint list of the selection's tangent-space difference (multistart.hip).
static int32_t ms_build_tables(MkhProblem* p) {
  if (p->ws_tables) return MKH_OK;
  const MkhModel* m = p->model;
  const int nq = m->nq, njnt = m->njnt;
  std::vector<int32_t> si(3 * (size_t)nq, 0), jn(3 * (size_t)njnt, 0);
  std::vector<double> sf(2 * (size_t)nq, 0.0), uw(3 * (size_t)nq, 0.0);     // (uw: kUnwCopy everywhere but at eligible hinges)
  for (int j = 0; j < njnt; ++j) {
    const int jt = m->jnt_type[j], qa = m->jnt_qposadr[j];
    jn[3 * j] = jt; jn[3 * j + 1] = qa; jn[3 * j + 2] = m->jnt_dofadr[j];
    const bool limited = m->jnt_limited[j] != 0;
    const double lo = m->jnt_range[2 * j], hi = m->jnt_range[2 * j + 1];
    if (jt == 3) {                                     // the unwinding's eligibility: "THE RULE OF THE UNWINDING"
      if (!limited) uw[3 * qa] = mkh::kUnwFree;
      else if (hi - lo >= 6.283185307179586) { uw[3 * qa] = mkh::kUnwRange; uw[3 * qa + 1] = lo; uw[3 * qa + 2] = hi; }
    }
    if (jt == 2 || jt == 3) {                          // slide / hinge
      si[3 * qa + 2] = qa;
      if (limited) { si[3 * qa] = 1; sf[2 * qa] = lo; sf[2 * qa + 1] = hi - lo; }
      else if (jt == 3) si[3 * qa] = 2;                // unlimited hinge: around the caller's value (unlimited slide: kept)
    } else if (jt == 1) {                              // ball: four addresses, one draw triple
      for (int c = 0; c < 4; ++c) {
        si[3 * (qa + c)] = 3; si[3 * (qa + c) + 1] = c; si[3 * (qa + c) + 2] = qa;
        sf[2 * (qa + c) + 1] = limited ? hi : M_PI;
      }
    }                                                  // free joint: the caller's value (zeros)
  }
  HIP_OK(p->ws[WS_SEED_I].need(si.size() * sizeof(int32_t)));
  HIP_OK(p->ws[WS_SEED_F].need(sf.size() * sizeof(double)));
  HIP_OK(p->ws[WS_JNT].need(jn.size() * sizeof(int32_t)));
  HIP_OK(hipMemcpy(p->ws[WS_SEED_I].p, si.data(), si.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(p->ws[WS_SEED_F].p, sf.data(), sf.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(p->ws[WS_JNT].p, jn.data(), jn.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_OK(p->ws[WS_UNW].need(uw.size() * sizeof(double)));
  HIP_OK(hipMemcpy(p->ws[WS_UNW].p, uw.data(), uw.size() * sizeof(double), hipMemcpyHostToDevice));
  p->ws_tables = true;
  return MKH_OK;
}

// ---- seed tables
// device buffers of one call, freed on every way out
struct DevTmp {
  std::vector<void*> all;
  ~DevTmp() { for (void* x : all) (void)hipFree(x); }
  hipError_t get(void** out, size_t bytes) {
    *out = nullptr;
    const hipError_t e = hipMalloc(out, bytes ? bytes : 8);
    if (e == hipSuccess) all.push_back(*out);
    return e;
  }
};

// Whether `tab` can seed a call on `p` that wants `k` rows per instance (k < 0: attaching — the row count is the call's).
static int32_t st_refuse(const MkhProblem* p, const MkhSeedTable* tab, int k, const char* who) {
  const MkhModel* m = p->model;
  if (tab->device != m->device)
    return fail(MKH_E_INVALID, "%s: the seed table lives on device %d, the problem on device %d", who, tab->device, m->device);
  if (tab->nq != m->nq || tab->njnt != m->njnt)
    return fail(MKH_E_INVALID, "%s: the seed table belongs to another model (nq = %d, njnt = %d; this problem: nq = %d, njnt = %d)",
                who, tab->nq, tab->njnt, m->nq, m->njnt);
  if (tab->n_frame != p->dev.n_frame)
    return fail(MKH_E_INVALID, "%s: the seed table is keyed on %d frame-task frames, this problem has %d", who, tab->n_frame,
                p->dev.n_frame);
  bool any = false;
  for (double w : p->frame_w) any = any || w > 0.0;
  if (!any)
    return fail(MKH_E_INVALID, "%s: the problem has no plain FrameTask with a non-zero cost (%d frame tasks): nothing to look a "
                               "world pose up by", who, p->dev.n_frame);
  if (k > tab->N)
    return fail(MKH_E_INVALID, "%s: n_seeds - 1 = %d exceeds the seed table's %d entries", who, k, tab->N);
  if (k > 255) return fail(MKH_E_LIMIT, "%s: n_seeds - 1 = %d rows from a seed table, at most 255", who, k);
  return MKH_OK;
}

extern "C" {

void mkh_seed_table_destroy(MkhSeedTable* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  (void)hipFree(t->d_q); (void)hipFree(t->d_keys); (void)hipFree(t->d_w);
  delete t;
}

int32_t mkh_seed_table_create(MkhProblem* p, int32_t n_entries, const double* q0, const double* entries, uint64_t rng_seed,
                              const double* pos_weight, const double* ori_weight, MkhSeedTable** out) {
  if (!p || !out) return fail(MKH_E_INVALID, "null argument");
  *out = nullptr;
  if (n_entries < 1) return fail(MKH_E_INVALID, "n_entries = %d must be >= 1", n_entries);
  if (!q0 && !entries) return fail(MKH_E_INVALID, "q0 is null (the configuration the entries are drawn around) and so is entries");
  const DeviceProblem& P = p->dev;
  const MkhModel* m = p->model;
  const int nf = P.n_frame, nq = P.nq;
  if (P.n_dense_rows || P.n_dense_limit_rows || P.dense_box)
    return fail(MKH_E_INVALID, "dense (plugin) rows are evaluated by the caller at q: no seed table");
  std::vector<double> w(p->frame_w);
  bool any_default = false;
  for (double x : w) any_default = any_default || x > 0.0;
  if (!any_default)
    return fail(MKH_E_INVALID, "mkh_seed_table_create: the problem has no plain FrameTask with a non-zero cost (%d frame tasks): "
                               "nothing to key the entries on", nf);
  for (int f = 0; f < nf; ++f) {
    if (pos_weight) w[f] = pos_weight[f];
    if (ori_weight) w[nf + f] = ori_weight[f];
  }
  bool any = false;
  for (int f = 0; f < 2 * nf; ++f) {
    if (!(w[f] >= 0.0) || !std::isfinite(w[f]))
      return fail(MKH_E_INVALID, "%s weight of frame %d is %g: weights must be finite and >= 0", f < nf ? "position" : "orientation",
                  f % nf, w[f]);
    any = any || w[f] > 0.0;
  }
  if (!any) return fail(MKH_E_INVALID, "all %d position and orientation weights are 0: every entry would be at distance 0", 2 * nf);
  HIP_OK(hipSetDevice(m->device));
  if (!entries)
    if (const int32_t rc = ms_build_tables(p)) return rc;
  const size_t Nz = (size_t)n_entries, f8 = sizeof(double);
  MkhSeedTable* t = new MkhSeedTable();
  t->device = m->device; t->N = n_entries; t->nq = nq; t->njnt = m->njnt; t->n_frame = nf;
  auto bail = [&](int32_t code) { mkh_seed_table_destroy(t); return code; };
  auto hip_bail = [&](hipError_t e, const char* what) {
    (void)hipDeviceSynchronize();
    return bail(fail(MKH_E_HIP, "mkh_seed_table_create: %s: %s", what, hipGetErrorString(e)));
  };
  hipError_t e;
  if ((e = hipMalloc((void**)&t->d_q, Nz * nq * f8)) || (e = hipMalloc((void**)&t->d_keys, Nz * nf * 7 * f8)) ||
      (e = hipMalloc((void**)&t->d_w, 2 * (size_t)nf * f8)))
    return hip_bail(e, "no device memory for the table");
  if ((e = hipMemcpy(t->d_w, w.data(), 2 * (size_t)nf * f8, hipMemcpyHostToDevice))) return hip_bail(e, "weights");
  DevTmp tmp;
  hipStream_t stream = nullptr;
  // ---- the entries
  if (entries) {
    if ((e = hipMemcpy(t->d_q, entries, Nz * nq * f8, hipMemcpyHostToDevice))) return hip_bail(e, "entries");
  } else {
    // entry j = row s = 1 of "target" j of multi-start's seed kernel around q0: (N, 2, nq) starts from N copies of q0
    std::vector<double> tiled(Nz * nq);
    for (size_t j = 0; j < Nz; ++j) memcpy(&tiled[j * nq], q0, (size_t)nq * f8);
    double *d_q0 = nullptr, *d_draw = nullptr;
    if ((e = tmp.get((void**)&d_q0, Nz * nq * f8)) || (e = tmp.get((void**)&d_draw, 2 * Nz * nq * f8)))
      return hip_bail(e, "no device memory to draw the entries in");
    if ((e = hipMemcpy(d_q0, tiled.data(), Nz * nq * f8, hipMemcpyHostToDevice))) return hip_bail(e, "q0");
    if ((e = launch_ms_seed(stream, p->ws[WS_SEED_I].i32(), p->ws[WS_SEED_F].f64(), n_entries, 2, nq, d_q0, nullptr,
                            (unsigned long long)rng_seed, 0, d_draw)))
      return hip_bail(e, "seed kernel");
    if ((e = hipMemcpy2DAsync(t->d_q, (size_t)nq * f8, d_draw + nq, 2 * (size_t)nq * f8, (size_t)nq * f8, Nz, hipMemcpyDeviceToDevice,
                              stream)))
      return hip_bail(e, "entries");
  }
  // ---- the keys: the frame_pose tap of mkh_eval on the entries, in chunks of max_batch.  The evaluation's targets do not
  //      enter a frame's pose: identity poses, the first entry as every posture target, a zero CoM target.
  const size_t chunk = (size_t)p->max_batch < Nz ? (size_t)p->max_batch : Nz;
  double *d_pose = nullptr, *d_ft = nullptr, *d_pt = nullptr, *d_ct = nullptr;
  std::vector<double> ident(chunk * nf * 7, 0.0);
  for (size_t i = 0; i < chunk * nf; ++i) ident[7 * i] = 1.0;
  if ((e = tmp.get((void**)&d_pose, chunk * nf * 7 * f8)) || (e = tmp.get((void**)&d_ft, chunk * nf * 7 * f8)) ||
      (e = tmp.get((void**)&d_pt, (size_t)P.n_posture * nq * f8)) || (e = tmp.get((void**)&d_ct, (size_t)P.n_com * 3 * f8)))
    return hip_bail(e, "no device memory to evaluate the keys in");
  if ((e = hipMemcpy(d_ft, ident.data(), ident.size() * f8, hipMemcpyHostToDevice))) return hip_bail(e, "targets");
  for (int k = 0; k < P.n_posture; ++k)
    if ((e = hipMemcpyAsync(d_pt + (size_t)k * nq, t->d_q, (size_t)nq * f8, hipMemcpyDeviceToDevice, stream))) return hip_bail(e, "targets");
  if (P.n_com && (e = hipMemsetAsync(d_ct, 0, (size_t)P.n_com * 3 * f8, stream))) return hip_bail(e, "targets");
  MkhTaps taps;
  memset(&taps, 0, sizeof taps);
  taps.frame_pose = d_pose;
  for (size_t j0 = 0; j0 < Nz; j0 += chunk) {
    const size_t n = Nz - j0 < chunk ? Nz - j0 : chunk;
    if (const int32_t rc = mkh_eval(p, (int32_t)n, t->d_q + j0 * nq, d_ft, P.n_posture ? d_pt : nullptr, P.n_com ? d_ct : nullptr, 1.0,
                                    1e-12, nullptr, nullptr, &taps, MKH_FLAG_DEVICE_PTRS, stream)) {
      (void)hipDeviceSynchronize();
      return bail(rc);
    }
    if ((e = launch_st_keys(stream, d_pose, (int)n, nf, (long long)Nz, (long long)j0, t->d_keys))) return hip_bail(e, "key kernel");
  }
  if ((e = hipStreamSynchronize(stream))) return hip_bail(e, "evaluating the keys");
  *out = t;
  return MKH_OK;
}

int32_t mkh_seed_table_read(const MkhSeedTable* t, double* q_out, double* keys_out) {
  if (!t) return fail(MKH_E_INVALID, "null seed table");
  HIP_OK(hipSetDevice(t->device));
  const size_t Nz = (size_t)t->N, f8 = sizeof(double);
  if (q_out) HIP_OK(hipMemcpy(q_out, t->d_q, Nz * t->nq * f8, hipMemcpyDeviceToHost));
  if (keys_out) {
    // (N, n_frame, 7) for the caller from the table's (n_frame·7, N)
    const size_t rows = (size_t)t->n_frame * 7;
    std::vector<double> k(rows * Nz);
    HIP_OK(hipMemcpy(k.data(), t->d_keys, rows * Nz * f8, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < Nz; ++j)
      for (size_t r = 0; r < rows; ++r) keys_out[j * rows + r] = k[r * Nz + j];
  }
  return MKH_OK;
}

int32_t mkh_seed_table_query(const MkhSeedTable* t, int32_t B, const double* frame_targets, int32_t K, int32_t* index_out,
                             double* dist_out, double* seeds_out, int32_t flags, void* hip_stream) {
  if (!t) return fail(MKH_E_INVALID, "null seed table");
  if (B < 1) return fail(MKH_E_INVALID, "B = %d must be >= 1", B);
  if (K < 1) return fail(MKH_E_INVALID, "K = %d must be >= 1", K);
  if (K > 255) return fail(MKH_E_LIMIT, "K = %d: a query returns at most 255 entries per target", K);
  if (K > t->N) return fail(MKH_E_INVALID, "K = %d exceeds the seed table's %d entries", K, t->N);
  if (const int32_t rc = refuse_unwind(flags, "mkh_seed_table_query")) return rc;
  if (!frame_targets) return fail(MKH_E_INVALID, "frame_targets is null");
  if (!index_out && !dist_out && !seeds_out) return fail(MKH_E_INVALID, "index_out, dist_out and seeds_out are all null");
  HIP_OK(hipSetDevice(t->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  const int nf = t->n_frame, nq = t->nq;
  if (flags & MKH_FLAG_DEVICE_PTRS) {
    HIP_OK(launch_st_query(stream, t->d_keys, t->d_q, t->d_w, t->N, nf, nq, B, frame_targets, K, index_out, dist_out, seeds_out));
    return MKH_OK;
  }
  // host pointers: staged through buffers of this call (a table is shared by handles and threads: it owns no workspace)
  DevTmp tmp;
  const size_t Bz = B, Kz = K, f8 = sizeof(double);
  double *d_ft = nullptr, *d_dist = nullptr, *d_seeds = nullptr;
  int32_t* d_idx = nullptr;
  HIP_OK(tmp.get((void**)&d_ft, Bz * nf * 7 * f8));
  if (index_out) HIP_OK(tmp.get((void**)&d_idx, Bz * Kz * sizeof(int32_t)));
  if (dist_out) HIP_OK(tmp.get((void**)&d_dist, Bz * Kz * f8));
  if (seeds_out) HIP_OK(tmp.get((void**)&d_seeds, Bz * (Kz + 1) * nq * f8));
  hipError_t e = hipMemcpyAsync(d_ft, frame_targets, Bz * nf * 7 * f8, hipMemcpyHostToDevice, stream);
  // (row 0 of the caller's slab is left alone: it goes down and comes back as it was)
  if (e == hipSuccess && seeds_out) e = hipMemcpyAsync(d_seeds, seeds_out, Bz * (Kz + 1) * nq * f8, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = launch_st_query(stream, t->d_keys, t->d_q, t->d_w, t->N, nf, nq, B, d_ft, K, d_idx, d_dist, d_seeds);
  if (e == hipSuccess && index_out) e = hipMemcpyAsync(index_out, d_idx, Bz * Kz * sizeof(int32_t), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && dist_out) e = hipMemcpyAsync(dist_out, d_dist, Bz * Kz * f8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && seeds_out) e = hipMemcpyAsync(seeds_out, d_seeds, Bz * (Kz + 1) * nq * f8, hipMemcpyDeviceToHost, stream);
  const hipError_t es = hipStreamSynchronize(stream);      // (whatever happened: copies from or to the caller's arrays may be in flight)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(MKH_E_HIP, "mkh_seed_table_query: %s", hipGetErrorString(e));
  return MKH_OK;
}

int32_t mkh_problem_set_seed_table(MkhProblem* p, const MkhSeedTable* table) {
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (table)
    if (const int32_t rc = st_refuse(p, table, -1, "mkh_problem_set_seed_table")) return rc;
  p->seed_table = table;
  return MKH_OK;
}

// ---- the loop stage of every call that fans a target out to S starts (kernels: multistart.hip, seed_table.hip): the two
// multi-start calls below, the rungs of the ladder calls and the goals of mkh_solve_goalset.  It works on device arrays and on
// the caller's Stager; which arrays, the caller says.
struct LoopSpec {                  // what a threshold loop is run with
  double dt, damping;
  int32_t max_iters;
  double pos_threshold, ori_threshold;
};

// What these calls refuse about the loop's scalars, in this order (`why`: the entry point's own words on the thresholds).
static int32_t loops_refuse(const LoopSpec& ls, int64_t target_index0, bool with_dt, const char* who = nullptr,
                            const char* why = nullptr) {
  if (ls.max_iters < 1) return fail(MKH_E_INVALID, "max_iters must be >= 1");
  if (target_index0 < 0) return fail(MKH_E_INVALID, "target_index0 must be >= 0");
  if (with_dt && !(ls.dt > 0.0)) return fail(MKH_E_INVALID, "dt must be > 0");
  if (!(ls.pos_threshold >= 0.0) || !(ls.ori_threshold >= 0.0))
    return why ? fail(MKH_E_INVALID, "%s: thresholds must be >= 0 (%s)", who, why) : fail(MKH_E_INVALID, "thresholds must be >= 0");
  return MKH_OK;
}

// An attached seed table gives rows s >= 1 unless the caller brought seeds of their own: the table of this call, or none.
static int32_t seed_table_for(const MkhProblem* p, const double* seeds, int S, const char* who, const MkhSeedTable** tab) {
  *tab = (!seeds && S > 1) ? p->seed_table : nullptr;
  return *tab ? st_refuse(p, *tab, S - 1, who) : MKH_OK;
}

struct MsIn {                      // what the stage reads, one row per target (pt / ct: one row in all where not batched)
  const double *q, *ft, *pt, *ct;
  const double* user;              // the caller's (B, S, nq) seeds, or NULL
  const MkhSeedTable* tab;         // seed_table_for()
};
struct MsRows {                    // the (B·S, .) candidate rows it writes
  double* starts;                  // the seed kernel writes them, the loop reads them; q_all itself: the loop runs in place
  double *q_all, *v_all;
  int32_t *status, *iters, *converged;
  double* kept;                    // a copy of the starts set aside in front of an in-place loop, or NULL
};

// Seeds (rows s >= 1 from the seed table's nearest entries, the caller's seeds, or drawn), the three target groups fanned out,
// and the loops: mkh_solve_until's own path and dispatch on the B·S instances.  Candidate 0 of a target is its row of in.q.
// Returns the refusal of the loop launch; HIP errors are latched in `st`, and nothing is launched behind one.
static int32_t ms_loops(Stager& st, int B, int S, const MsIn& in, const LoopSpec& ls, uint64_t rng_seed, int64_t target_index0,
                        const MsRows& c, int32_t flags) {
  MkhProblem* const p = st.p;
  const DeviceProblem& P = p->dev;
  hipStream_t stream = st.stream;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  const size_t Nz = (size_t)B * S, nq = P.nq;
  const size_t ft_w = (size_t)P.n_frame * 7, pt_w = (size_t)P.n_posture * nq, ct_w = (size_t)P.n_com * 3;
  const double* d_user = in.user;
  if (in.tab) {                       // the S − 1 entries nearest to each target, into the slab a caller's seeds would be in
    double* const slab = st.f64(WS_IN_SEEDS, Nz * nq);
    ST_LAUNCH(st, launch_st_query(stream, in.tab->d_keys, in.tab->d_q, in.tab->d_w, in.tab->N, P.n_frame, (int)nq, B, in.ft, S - 1,
                                  nullptr, nullptr, slab));
    d_user = slab;
  }
  ST_LAUNCH(st, launch_ms_seed(stream, p->ws[WS_SEED_I].i32(), p->ws[WS_SEED_F].f64(), B, S, (int)nq, in.q, d_user,
                               (unsigned long long)rng_seed, (long long)target_index0, c.starts));
  if (c.kept) st.latch(hipMemcpyAsync(c.kept, c.starts, Nz * nq * sizeof(double), hipMemcpyDeviceToDevice, stream));
  // target fan-out: every per-instance target S times (the solve kernels index targets by instance)
  auto fanout = [&](WsRole role, const double* src, size_t w) -> const double* {
    double* const dst = st.f64(role, Nz * w);
    ST_LAUNCH(st, launch_ms_fanout(stream, src, dst, B, S, (int)w));
    return dst;
  };
  const double* const c_ft = fanout(WS_C_FT, in.ft, ft_w);
  const double* const c_pt = (pt_w && pbat) ? fanout(WS_C_PT, in.pt, pt_w) : in.pt;
  const double* const c_ct = (ct_w && cbat) ? fanout(WS_C_CT, in.ct, ct_w) : in.ct;
  if (!st.ok()) return MKH_OK;
  const int32_t loop_flags = (flags & ~(MKH_FLAG_WARM_START | MKH_FLAG_UNWIND_TURNS)) | MKH_FLAG_DEVICE_PTRS;
  SolveCall sc;
  sc.p = p; sc.B = (int32_t)Nz; sc.q = c.starts; sc.frame_targets = c_ft; sc.posture_target = c_pt; sc.com_target = c_ct;
  sc.dt = ls.dt; sc.damping = ls.damping; sc.v_out = c.v_all; sc.status_out = c.status; sc.flags = loop_flags; sc.hip_stream = (void*)stream;
  sc.n_steps = ls.max_iters; sc.q_out = c.q_all; sc.pos_threshold = ls.pos_threshold; sc.ori_threshold = ls.ori_threshold;
  sc.iters_out = c.iters; sc.converged_out = c.converged;
  return solve(sc);
}

// R flattened rows of targets (a ladder's rungs, a goal set's goals) through ms_loops, whole rows per chunk of at most
// max_batch / S of them: chunk r0 … reads rows r0 … of `in` and draws with target index index0 + r0; rows_at(r0) names the
// candidate rows it writes, then(r0, n) is what the caller enqueues behind its n rows' loops.  The first chunk is the largest:
// a slot sized for it is not grown while an earlier chunk's work is queued.  Returns as ms_loops does.
static int32_t ms_rungs(Stager& st, size_t R, int S, const MsIn& in, const LoopSpec& ls, uint64_t rng_seed, int64_t index0,
                        int32_t flags, const std::function<MsRows(size_t)>& rows_at,
                        const std::function<void(size_t, size_t)>& then = nullptr) {
  const DeviceProblem& P = st.p->dev;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  const size_t nq = P.nq, ft_w = (size_t)P.n_frame * 7, pt_w = (size_t)P.n_posture * nq, ct_w = (size_t)P.n_com * 3;
  const size_t per = (size_t)st.p->max_batch / S;
  for (size_t r0 = 0; r0 < R; r0 += per) {
    const size_t n = R - r0 < per ? R - r0 : per;
    const MsIn chunk{in.q + r0 * nq, in.ft + r0 * ft_w, (pt_w && pbat) ? in.pt + r0 * pt_w : in.pt,
                     (ct_w && cbat) ? in.ct + r0 * ct_w : in.ct, in.user ? in.user + r0 * S * nq : nullptr, in.tab};
    const int32_t rc = ms_loops(st, (int)n, S, chunk, ls, rng_seed, index0 + (int64_t)r0, rows_at(r0), flags);
    if (rc || !st.ok()) return rc;
    if (then) then(r0, n);
  }
  return MKH_OK;
}

// ---- mkh_solve_multistart and mkh_solve_multistart_set: everything in front of their selections
static int32_t ms_refuse(const MkhProblem* p, int32_t B, int32_t n_seeds, const double* q, const double* frame_targets,
                         const double* posture_target, const double* com_target, const double* seeds, const char* who,
                         const MkhSeedTable** tab) {
  if (const int32_t rc = refuse_inputs(p->dev, q, frame_targets, posture_target, com_target, who, "multi-start")) return rc;
  const long long N = (long long)B * n_seeds;
  if (N > p->max_batch)
    return fail(MKH_E_INVALID, "B * n_seeds = %lld exceeds max_batch=%d of this problem", N, p->max_batch);
  return seed_table_for(p, seeds, n_seeds, who, tab);
}

struct MsCall {                    // what the two calls stage: the loops' inputs and rows, and the selections' reference and weights
  MsIn in;
  MsRows c;
  const double *ref, *w;
};
// The inputs on the device, and the B·S candidate rows: the caller's *_all arrays where they are device buffers.  Seeds go into
// the caller's seeds_out when it is a device buffer (the loop then reads them there), else into the workspace, where the loop
// runs in place (a host caller's seeds_out: set aside before the loop overwrites them).
static MsCall ms_stage(Stager& st, int B, int S, const double* q, const double* frame_targets, const double* posture_target,
                       const double* com_target, const MkhSeedTable* tab, const MkhMultistartIO& io, int32_t flags) {
  const DeviceProblem& P = st.p->dev;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  const size_t Bz = B, Nz = Bz * S, nq = P.nq, nv = P.nv, i4 = sizeof(int32_t);
  const size_t ft_w = (size_t)P.n_frame * 7, pt_w = (size_t)P.n_posture * nq, ct_w = (size_t)P.n_com * 3;
  MsCall m;
  m.in.q = st.up(WS_IN_Q, q, Bz * nq);
  m.in.ft = st.up(WS_IN_FT, frame_targets, Bz * ft_w);
  m.in.pt = pt_w ? st.up(WS_IN_PT, posture_target, pt_w * (pbat ? Bz : 1)) : posture_target;
  m.in.ct = ct_w ? st.up(WS_IN_CT, com_target, ct_w * (cbat ? Bz : 1)) : com_target;
  const double* const d_ref = st.up(WS_IN_REF, io.q_ref, Bz * nq);
  m.ref = d_ref ? d_ref : m.in.q;
  m.w = st.up(WS_IN_W, io.weights, nv);
  m.in.user = st.up(WS_IN_SEEDS, io.seeds, Nz * nq);             // (the seed kernel reads them once)
  m.in.tab = tab;
  double* const c_q = st.f64(WS_C_Q, Nz * nq);
  m.c.starts = (st.devp && io.seeds_out) ? io.seeds_out : c_q;
  m.c.q_all = (st.devp && io.q_all) ? io.q_all : c_q;
  m.c.v_all = st.f64(WS_C_V, Nz * nv);
  m.c.status = (int32_t*)st.given_or(WS_C_ST, io.status_all, Nz * i4);
  m.c.iters = (int32_t*)st.given_or(WS_C_IT, io.iters_all, Nz * i4);
  m.c.converged = (int32_t*)st.given_or(WS_C_CV, io.converged_all, Nz * i4);
  m.c.kept = (!st.devp && io.seeds_out) ? st.f64(WS_C_STARTS, Nz * nq) : nullptr;
  return m;
}
// a host caller's optional per-instance arrays
static void ms_down(Stager& st, size_t Nz, const MkhMultistartIO& io, const MsRows& c) {
  const size_t nq = st.p->dev.nq, f8 = sizeof(double), i4 = sizeof(int32_t);
  st.down(io.q_all, c.q_all, Nz * nq * f8);
  st.down(io.status_all, c.status, Nz * i4);
  st.down(io.iters_all, c.iters, Nz * i4);
  st.down(io.converged_all, c.converged, Nz * i4);
  st.down(io.seeds_out, c.kept, Nz * nq * f8);
}

int32_t mkh_solve_multistart(MkhProblem* p, int32_t B, const double* q, const double* frame_targets,
                             const double* posture_target, const double* com_target, double dt, double damping,
                             int32_t max_iters, double pos_threshold, double ori_threshold, int32_t n_seeds,
                             uint64_t rng_seed, int64_t target_index0, const MkhMultistartIO* io, int32_t flags,
                             void* hip_stream) {
  const char* const who = "mkh_solve_multistart";
  const LoopSpec ls{dt, damping, max_iters, pos_threshold, ori_threshold};
  const int S = n_seeds;
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (B < 1) return fail(MKH_E_INVALID, "B must be >= 1");
  if (S < 1) return fail(MKH_E_INVALID, "n_seeds must be >= 1");
  if (const int32_t rc = loops_refuse(ls, target_index0, false)) return rc;
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;
  if (!io || !io->q_best || !io->v_best || !io->iters || !io->status || !io->converged || !io->seed_index || !io->n_converged)
    return fail(MKH_E_INVALID, "io and its per-target outputs (q_best, v_best, iters, status, converged, seed_index, n_converged) are required");
  const MkhSeedTable* tab;
  if (const int32_t rc = ms_refuse(p, B, S, q, frame_targets, posture_target, com_target, io->seeds, who, &tab)) return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  Stager st{p, (hipStream_t)hip_stream, devp, "multistart"};
  const size_t Bz = B, nq = p->dev.nq, nv = p->dev.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  const MsCall m = ms_stage(st, B, S, q, frame_targets, posture_target, com_target, tab, *io, flags);
  if (const int32_t rc = ms_loops(st, B, S, m.in, ls, rng_seed, target_index0, m.c, flags); rc || !st.ok()) return st.finish(rc);
  if (p->checker) clearance_rows(st, p->checker, Bz * S, m.c.q_all, nullptr, nullptr, nullptr, nullptr, m.c.status);
  // ---- selection
  double *o_q = io->q_best, *o_v = io->v_best;
  int32_t *o_it = io->iters, *o_st = io->status, *o_cv = io->converged, *o_si = io->seed_index, *o_nc = io->n_converged;
  if (!devp) {
    o_q = st.f64(WS_OUT_Q, Bz * nq); o_v = st.f64(WS_OUT_V, Bz * nv);
    o_it = st.i32(WS_OUT_I32, 3 * Bz); o_st = o_it + Bz; o_cv = o_it + 2 * Bz;
    o_si = st.i32(WS_OUT_PICK, 2 * Bz); o_nc = o_si + Bz;
  }
  ST_LAUNCH(st, launch_ms_select(st.stream, B, S, (int)nq, (int)nv, p->model->njnt, p->ws[WS_JNT].i32(), m.c.q_all, m.c.v_all,
                                 m.c.status, m.c.iters, m.c.converged, m.ref, m.w, o_q, o_v, o_it, o_st, o_cv, o_si, o_nc));
  if (devp) return st.finish();
  st.down(io->q_best, o_q, Bz * nq * f8);
  st.down(io->v_best, o_v, Bz * nv * f8);
  st.down(io->iters, o_it, Bz * i4);
  st.down(io->status, o_st, Bz * i4);
  st.down(io->converged, o_cv, Bz * i4);
  st.down(io->seed_index, o_si, Bz * i4);
  st.down(io->n_converged, o_nc, Bz * i4);
  ms_down(st, Bz * S, *io, m.c);
  return st.finish();
}

// ---- distinct solution sets (include/minkhip.h "THE RULE OF THE SET"; kernel: solution_set.hip)
struct SetSpec {
  int32_t K;                       // n_solutions
  double r2;                       // min_distance²
  const MkhSolutionSetIO* io;      // the outputs (checked by the entry point)
};
// The selection on device arrays into set.io's outputs: in place for a device-pointer call, else through the workspace and
// down.  v / status / iters / conv may be absent (a selection over a caller's own candidates: conv is then its `valid`).
static void set_select(Stager& st, int B, int S, const SetSpec& set, const double* d_q_all, const double* d_v_all,
                       const int32_t* d_status, const int32_t* d_iters, const int32_t* d_conv, const double* d_ref, const double* d_w) {
  const MkhProblem* const p = st.p;
  const MkhSolutionSetIO& io = *set.io;
  const size_t R = (size_t)B * set.K, Bz = B, nq = p->dev.nq, nv = p->dev.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  mkh::SsOut o{io.q_set, d_v_all ? io.v_set : nullptr, d_iters ? io.iters : nullptr, d_status ? io.status : nullptr, io.seed_index,
               io.multiplicity, io.distance, io.n_distinct, io.n_converged, io.n_uncovered};
  if (!st.devp) {
    o.q_set = st.f64(WS_OUT_Q, R * nq);
    if (o.v_set) o.v_set = st.f64(WS_OUT_V, R * nv);
    int32_t* const rows = st.i32(WS_OUT_I32, 2 * R);
    if (o.iters) o.iters = rows;
    if (o.status) o.status = rows ? rows + R : nullptr;
    int32_t* const pick = st.i32(WS_OUT_PICK, 2 * R + 3 * Bz);
    o.seed_index = pick; o.multiplicity = pick ? pick + R : nullptr;
    o.n_distinct = pick ? pick + 2 * R : nullptr;
    if (o.n_converged) o.n_converged = pick ? pick + 2 * R + Bz : nullptr;
    o.n_uncovered = pick ? pick + 2 * R + 2 * Bz : nullptr;
    o.distance = st.f64(WS_OUT_LEN, R);
  }
  ST_LAUNCH(st, launch_ss_select(st.stream, B, S, set.K, (int)nq, (int)nv, p->model->njnt, p->ws[WS_JNT].i32(), d_q_all, d_v_all,
                                 d_status, d_iters, d_conv, d_ref, d_w, set.r2, o));
  if (st.devp) return;
  st.down(io.q_set, o.q_set, R * nq * f8);
  if (o.v_set) st.down(io.v_set, o.v_set, R * nv * f8);
  if (o.iters) st.down(io.iters, o.iters, R * i4);
  if (o.status) st.down(io.status, o.status, R * i4);
  st.down(io.seed_index, o.seed_index, R * i4);
  st.down(io.multiplicity, o.multiplicity, R * i4);
  st.down(io.distance, o.distance, R * f8);
  st.down(io.n_distinct, o.n_distinct, Bz * i4);
  if (o.n_converged) st.down(io.n_converged, o.n_converged, Bz * i4);
  st.down(io.n_uncovered, o.n_uncovered, Bz * i4);
}

// What both entry points refuse about K and r.
static int32_t set_refuse(int32_t n_solutions, double min_distance, const char* who) {
  if (n_solutions < 1 || n_solutions > mkh::kSsMaxSolutions)
    return fail(MKH_E_INVALID, "%s: n_solutions = %d must be in 1 ... %d", who, n_solutions, mkh::kSsMaxSolutions);
  if (!(min_distance >= 0.0) || min_distance > 1.7976931348623157e308)
    return fail(MKH_E_INVALID, "%s: min_distance = %g must be >= 0 and finite (0: exact duplicates only)", who, min_distance);
  return MKH_OK;
}

// mkh_solve_multistart with the distinct set's selection behind the loops, the results unwound in front of it when asked.
int32_t mkh_solve_multistart_set(MkhProblem* p, int32_t B, const double* q, const double* frame_targets,
                                 const double* posture_target, const double* com_target, double dt, double damping,
                                 int32_t max_iters, double pos_threshold, double ori_threshold, int32_t n_seeds,
                                 int32_t n_solutions, double min_distance, uint64_t rng_seed, int64_t target_index0,
                                 const MkhSolutionSetIO* io, int32_t flags, void* hip_stream) {
  const char* const who = "mkh_solve_multistart_set";
  const LoopSpec ls{dt, damping, max_iters, pos_threshold, ori_threshold};
  const int S = n_seeds;
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (const int32_t rc = set_refuse(n_solutions, min_distance, who)) return rc;
  if (!io || !io->q_set || !io->v_set || !io->iters || !io->status || !io->seed_index || !io->multiplicity || !io->distance ||
      !io->n_distinct || !io->n_converged || !io->n_uncovered)
    return fail(MKH_E_INVALID, "%s: io and its outputs q_set, v_set, iters, status, seed_index, multiplicity, distance, n_distinct, "
                               "n_converged, n_uncovered are required", who);
  if (B < 1) return fail(MKH_E_INVALID, "B must be >= 1");
  if (S < 1) return fail(MKH_E_INVALID, "n_seeds must be >= 1");
  if (const int32_t rc = loops_refuse(ls, target_index0, false)) return rc;
  if (S > mkh::kSsMaxCandidates)
    return fail(MKH_E_LIMIT, "%s: n_seeds = %d candidates per target, at most %d (their selection state lives in LDS)", who, S,
                mkh::kSsMaxCandidates);
  const MkhSeedTable* tab;
  if (const int32_t rc = ms_refuse(p, B, S, q, frame_targets, posture_target, com_target, io->seeds, who, &tab)) return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  Stager st{p, (hipStream_t)hip_stream, (flags & MKH_FLAG_DEVICE_PTRS) != 0, "multistart_set"};
  MkhMultistartIO mio{};           // what the staging reads: the inputs and the optional per-instance arrays
  mio.seeds = io->seeds; mio.q_ref = io->q_ref; mio.weights = io->weights;
  mio.q_all = io->q_all; mio.converged_all = io->converged_all; mio.iters_all = io->iters_all; mio.status_all = io->status_all;
  mio.seeds_out = io->seeds_out;
  const MsCall m = ms_stage(st, B, S, q, frame_targets, posture_target, com_target, tab, mio, flags);
  if (const int32_t rc = ms_loops(st, B, S, m.in, ls, rng_seed, target_index0, m.c, flags); rc || !st.ok()) return st.finish(rc);
  // (the checker in front of the unwinding: it judges the loops' own results, and whole turns move no body)
  if (p->checker) clearance_rows(st, p->checker, (size_t)B * S, m.c.q_all, nullptr, nullptr, nullptr, nullptr, m.c.status);
  if (flags & MKH_FLAG_UNWIND_TURNS)     // in place, where q_all is read from: the loops' flags are carried over
    ST_LAUNCH(st, launch_unwind_turns(st.stream, p->ws[WS_UNW].f64(), (long long)B * S, S, (int)p->dev.nq, m.c.q_all, m.ref, m.c.q_all));
  const SetSpec set{n_solutions, min_distance * min_distance, io};
  set_select(st, B, S, set, m.c.q_all, m.c.v_all, m.c.status, m.c.iters, m.c.converged, m.ref, m.w);
  if (!st.devp) ms_down(st, (size_t)B * S, mio, m.c);
  return st.finish();
}

int32_t mkh_select_distinct(MkhProblem* p, int32_t B, int32_t S, const double* q_candidates, const int32_t* valid,
                            const double* q_ref, const double* weights, int32_t n_solutions, double min_distance,
                            const MkhSolutionSetIO* io, int32_t flags, void* hip_stream) {
  const char* const who = "mkh_select_distinct";
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (B < 1) return fail(MKH_E_INVALID, "%s: B = %d must be >= 1", who, B);
  if (S < 1) return fail(MKH_E_INVALID, "%s: S = %d must be >= 1", who, S);
  if (S > mkh::kSsMaxCandidates)
    return fail(MKH_E_LIMIT, "%s: S = %d candidates per target, at most %d (their selection state lives in LDS)", who, S,
                mkh::kSsMaxCandidates);
  if ((long long)B * S > 0x7fffffffLL) return fail(MKH_E_LIMIT, "%s: B * S = %lld rows", who, (long long)B * S);
  if (const int32_t rc = set_refuse(n_solutions, min_distance, who)) return rc;
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;       // (the caller's own candidates: mkh_unwind_turns in front)
  if (!q_candidates || !q_ref) return fail(MKH_E_INVALID, "%s: q_candidates and q_ref are required", who);
  if (!io || !io->q_set || !io->seed_index || !io->multiplicity || !io->distance || !io->n_distinct || !io->n_uncovered)
    return fail(MKH_E_INVALID, "%s: io and its outputs q_set, seed_index, multiplicity, distance, n_distinct, n_uncovered are required", who);
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  Stager st{p, (hipStream_t)hip_stream, devp, "select_distinct"};
  const size_t Bz = B, N = Bz * S, nq = p->dev.nq;
  const double* const d_cand = st.up(WS_C_Q, q_candidates, N * nq);
  const double* const d_ref = st.up(WS_IN_REF, q_ref, Bz * nq);
  const double* const d_w = st.up(WS_IN_W, weights, p->dev.nv);
  const int32_t* const d_valid = st.up_i32(WS_C_CV, valid, N);
  if (!st.ok()) return st.finish();
  MkhSolutionSetIO sio = *io;      // (the selection alone has no loop rows: n_converged is the count of `valid`, when asked for)
  const SetSpec set{n_solutions, min_distance * min_distance, &sio};
  set_select(st, B, S, set, d_cand, nullptr, nullptr, nullptr, d_valid, d_ref, d_w);
  return st.finish();
}

// ---- turn unwinding (include/minkhip.h "THE RULE OF THE UNWINDING"; kernel: unwind.hip)
int32_t mkh_unwind_turns(MkhProblem* p, int32_t n_rows, int32_t rows_per_ref, const double* q_rows, const double* q_ref,
                         double* q_out, int32_t flags, void* hip_stream) {
  const char* const who = "mkh_unwind_turns";
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (n_rows < 1) return fail(MKH_E_INVALID, "%s: n_rows = %d must be >= 1", who, n_rows);
  if (rows_per_ref < 1) return fail(MKH_E_INVALID, "%s: rows_per_ref = %d must be >= 1", who, rows_per_ref);
  if (flags & ~MKH_FLAG_DEVICE_PTRS) return fail(MKH_E_INVALID, "%s: flags = %d: only MKH_FLAG_DEVICE_PTRS is accepted", who, flags);
  if (!q_rows || !q_ref || !q_out) return fail(MKH_E_INVALID, "%s: q_rows, q_ref and q_out are required", who);
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  Stager st{p, (hipStream_t)hip_stream, devp, "unwind_turns"};
  const size_t Nz = n_rows, nq = p->dev.nq, n_ref = (Nz + rows_per_ref - 1) / (size_t)rows_per_ref;
  const double* const d_rows = st.up(WS_C_Q, q_rows, Nz * nq);
  const double* const d_ref = st.up(WS_IN_REF, q_ref, n_ref * nq);
  double* const d_out = devp ? q_out : (double*)d_rows;      // (a host caller's rows are unwound in place in their staged copy)
  if (!st.ok()) return st.finish();
  ST_LAUNCH(st, launch_unwind_turns(st.stream, p->ws[WS_UNW].f64(), n_rows, rows_per_ref, (int)nq, d_rows, d_ref, d_out));
  if (!devp) st.down(q_out, d_out, Nz * nq * sizeof(double));
  return st.finish();
}

}  // extern "C"

// What mkh_solve_keyframes adds to a trajectory call: the targets have a K axis where the trajectory call has its T axis, and
// waypoint t's targets are blended from keyframes seg_k[t], seg_k[t] + 1 at seg_u[t] in front of its loop (keyframes.hip).
struct KeyframeSpec {
  int32_t K;
  const double *key_times, *waypoint_times;                // host
  double *ft_out, *pt_out, *ct_out;                        // the caller's optional *_targets_out
  std::vector<int32_t> seg_k;
  std::vector<double> seg_u;
};

// The segment of every waypoint (include/minkhip.h "THE RULE"), or the first thing wrong with the two time arrays.
static int32_t kf_segments(KeyframeSpec* kf, int32_t T) {
  const int32_t K = kf->K;
  const double *kt = kf->key_times, *wt = kf->waypoint_times;
  if (K < 1) return fail(MKH_E_INVALID, "K must be >= 1");
  if (!kt || !wt) return fail(MKH_E_INVALID, "key_times and waypoint_times are required (host arrays)");
  for (int32_t k = 0; k < K; ++k) {
    if (kt[k] != kt[k]) return fail(MKH_E_INVALID, "key_times[%d] is NaN", k);
    if (k && !(kt[k - 1] < kt[k])) return fail(MKH_E_INVALID, "key_times must be strictly increasing (at index %d)", k);
  }
  kf->seg_k.resize(T);
  kf->seg_u.resize(T);
  int32_t k = 0;
  for (int32_t t = 0; t < T; ++t) {
    const double tau = wt[t];
    if (tau != tau) return fail(MKH_E_INVALID, "waypoint_times[%d] is NaN", t);
    if (t && tau < wt[t - 1]) return fail(MKH_E_INVALID, "waypoint_times must be non-decreasing (at index %d)", t);
    if (tau < kt[0] || tau > kt[K - 1])
      return fail(MKH_E_INVALID, "waypoint_times[%d] = %g lies outside the keyframes' range [%g, %g]: no extrapolation", t, tau,
                  kt[0], kt[K - 1]);
    while (k + 1 < K && kt[k + 1] <= tau) ++k;             // (waypoint times do not decrease: k never goes back)
    double u = 0.0;
    if (k < K - 1)
      u = (tau - kt[k]) / (kt[k + 1] - kt[k]);
    kf->seg_k[t] = k;
    kf->seg_u[t] = u;
  }
  return MKH_OK;
}

// What mkh_solve_trajectory_multistart adds to a trajectory call: the loops run on B·S candidate rows — instance b's targets
// fanned out S times in front of every waypoint's loop, the starts drawn by multi-start's seed kernel — into time-major
// (T, B·S, .) results of their own, and the call's (B, T, .) outputs are the rows of one candidate per instance, chosen by the
// score over the whole path (trajectory_multistart.hip).
struct CandidateSpec {
  int32_t S;
  uint64_t rng_seed;
  int64_t target_index0;
  const double *seeds, *weights;                           // optional inputs: (B, S, nq) starts, (nv,) weights of the length
  int32_t *seed_index, *n_tracked, *n_complete;            // (B,) required
  double* path_length;                                     // (B,) required
  double *seeds_out, *q_all, *v_all;                       // optional: (B·S, nq), (T, B·S, nq), (T, B·S, nv)
  int32_t *status_all, *iters_all, *converged_all;         // optional: (T, B·S)
  // mkh_solve_trajectory_multistart_free ("THE RULE, with a checker"): the checker, the samples per edge and the free outputs
  bool checked;
  MkhProblem* ck;
  int32_t M;
  const MkhTrajectoryFreeIO* fio;
};

// ---- checked candidate tracking (include/minkhip.h "THE RULE, with a checker" of mkh_solve_trajectory_multistart; kernels:
// trajectory_free.hip): what mkh_solve_trajectory_multistart_free and mkh_select_trajectory_candidates share
struct TmfDev {                    // device arrays: every row's margins, (T, B·S), and the chosen candidate's outputs in the caller's layout
  double *nm_all, *em_all;
  double *node_margin, *edge_margin;
  int32_t *edge_collision, *n_edge_collisions;
};

// What both calls refuse about the sample count and the free outputs: from the arguments alone.
static int32_t tmf_refuse_args(int32_t n_samples, const MkhTrajectoryFreeIO* f, const char* who) {
  if (n_samples < 1) return fail(MKH_E_INVALID, "%s: n_samples = %d must be >= 1", who, n_samples);
  if (!f || !f->node_margin || !f->edge_margin || !f->edge_collision || !f->n_edge_collisions)
    return fail(MKH_E_INVALID, "%s: free_io and its outputs node_margin, edge_margin, edge_collision, n_edge_collisions are required", who);
  return MKH_OK;
}

// N = B·T rows of the chosen candidate, NR = T·B·S rows in all.  The *_all margins always exist on the device: the score reads
// the edges', the gathers both.
static TmfDev tmf_stage(Stager& st, const MkhTrajectoryFreeIO& f, size_t N, size_t Bz, size_t NR) {
  TmfDev d{};
  d.nm_all = (double*)st.given_or(WS_F_NMARGIN, f.node_margin_all, NR * sizeof(double));
  d.em_all = (double*)st.given_or(WS_F_EMARGIN, f.edge_margin_all, NR * sizeof(double));
  d.node_margin = f.node_margin; d.edge_margin = f.edge_margin;
  d.edge_collision = f.edge_collision; d.n_edge_collisions = f.n_edge_collisions;
  if (!st.devp) {
    d.node_margin = st.f64(WS_F_OUT_F, 2 * N); d.edge_margin = d.node_margin ? d.node_margin + N : nullptr;
    d.edge_collision = st.i32(WS_F_OUT_I, N + Bz); d.n_edge_collisions = d.edge_collision ? d.edge_collision + N : nullptr;
  }
  return d;
}

// The chosen candidate's margins (plain gathers: edge_margin_all carries +inf at waypoint 0) and its edge flags, through the
// (instance, waypoint) strides sb / sw of a (B, T) array in the caller's layout.
static void tmf_chosen(Stager& st, int B, int S, int T, const int32_t* o_si, const int32_t* cv_all, const int32_t* st_all, const TmfDev& d,
                       long long sb, long long sw) {
  ST_LAUNCH(st, launch_tms_gather(st.stream, d.nm_all, d.node_margin, o_si, B, S, T, 1, sb, sw));
  ST_LAUNCH(st, launch_tms_gather(st.stream, d.em_all, d.edge_margin, o_si, B, S, T, 1, sb, sw));
  ST_LAUNCH(st, launch_tmf_edge_flags(st.stream, B, S, T, o_si, cv_all, st_all, d.em_all, d.edge_collision, sb, sw, d.n_edge_collisions));
}

static void tmf_down(Stager& st, const MkhTrajectoryFreeIO& f, const TmfDev& d, size_t N, size_t Bz, size_t NR) {
  st.down(f.node_margin, d.node_margin, N * sizeof(double));
  st.down(f.edge_margin, d.edge_margin, N * sizeof(double));
  st.down(f.edge_collision, d.edge_collision, N * sizeof(int32_t));
  st.down(f.n_edge_collisions, d.n_edge_collisions, Bz * sizeof(int32_t));
  st.down(f.node_margin_all, d.nm_all, NR * sizeof(double));
  st.down(f.edge_margin_all, d.em_all, NR * sizeof(double));
}

// mkh_solve_trajectory and, with `kf`, mkh_solve_keyframes, or, with `cs`, mkh_solve_trajectory_multistart: the T
// stream-ordered loop launches between slabs of time-major buffers and everything around them.  `who` names the entry point
// in messages.
static int32_t trajectory_core(MkhProblem* p, int32_t B, int32_t T, const double* q, const double* frame_targets,
                               const double* posture_target, const double* com_target, double dt, double damping,
                               int32_t n_steps, double pos_threshold, double ori_threshold, const MkhTrajectoryIO* io,
                               int32_t flags, void* hip_stream, KeyframeSpec* kf, const CandidateSpec* cs, const char* who) {
  // (what can be judged from the arguments alone comes first: it needs neither a handle nor a device)
  if (B < 1) return fail(MKH_E_INVALID, "B must be >= 1");
  if (T < 1) return fail(MKH_E_INVALID, "T must be >= 1");
  if (n_steps < 1) return fail(MKH_E_INVALID, "n_steps must be >= 1");
  if (cs && cs->S < 1) return fail(MKH_E_INVALID, "n_seeds must be >= 1");
  if (cs && cs->target_index0 < 0) return fail(MKH_E_INVALID, "target_index0 must be >= 0");
  if (!(dt > 0.0)) return fail(MKH_E_INVALID, "dt must be > 0");
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;
  const bool until = pos_threshold >= 0.0 && ori_threshold >= 0.0;
  if (!until && !(pos_threshold < 0.0 && ori_threshold < 0.0))
    return fail(MKH_E_INVALID, "thresholds must both be >= 0 (threshold mode) or both be < 0 (fixed count)");
  if (cs && !until)
    return fail(MKH_E_INVALID, "%s runs in threshold mode only: a fixed count leaves nothing to score (both thresholds must be >= 0)", who);
  if (!io || !io->q_traj || !io->v_traj || !io->status)
    return fail(MKH_E_INVALID, "io and its outputs q_traj, v_traj, status are required");
  if (cs && (!io->iters || !io->converged || !cs->seed_index || !cs->n_tracked || !cs->n_complete || !cs->path_length))
    return fail(MKH_E_INVALID, "io's outputs iters, converged, seed_index, n_tracked, n_complete, path_length are required");
  if (cs && cs->checked) {
    if (const int32_t rc = tmf_refuse_args(cs->M, cs->fio, who)) return rc;
    if (!cs->ck) return fail(MKH_E_INVALID, "%s: null checker", who);
  }
  if (!until && (io->iters || io->converged))
    return fail(MKH_E_INVALID, "iters / converged are outputs of threshold mode: they must be NULL with a fixed count");
  if (io->qvel && !(io->waypoint_dt > 0.0)) return fail(MKH_E_INVALID, "qvel needs waypoint_dt > 0");
  if (kf) {
    if (const int32_t rc = kf_segments(kf, T)) return rc;
    if ((kf->pt_out && !io->posture_per_waypoint) || (kf->ct_out && !io->com_per_waypoint))
      return fail(MKH_E_INVALID, "posture_targets_out / com_targets_out must be NULL for a target that is held");
  }
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (const int32_t rc = refuse_checker(p, who)) return rc;
  const bool checked = cs && cs->checked;
  if (checked)
    if (const int32_t rc = sweep_refuse_for(p, cs->ck, who, CheckerUse::tracking(cs->M))) return rc;
  const DeviceProblem& P = p->dev;
  if (const int32_t rc = refuse_inputs(P, q, frame_targets, posture_target, com_target, until ? who : nullptr, "trajectory"))
    return rc;
  if (B > p->max_batch) return fail(MKH_E_INVALID, "B=%d exceeds max_batch=%d of this problem", B, p->max_batch);
  if (cs && (long long)B * cs->S > p->max_batch)
    return fail(MKH_E_INVALID, "B * n_seeds = %lld exceeds max_batch=%d of this problem", (long long)B * cs->S, p->max_batch);
  // an attached seed table gives the candidates' starts unless the caller brought seeds of their own
  const MkhSeedTable* const tab = (cs && !cs->seeds && cs->S > 1) ? p->seed_table : nullptr;
  if (tab)
    if (const int32_t rc = st_refuse(p, tab, cs->S - 1, who)) return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (cs || io->qvel || (kf && io->posture_per_waypoint && P.n_posture > 0))
    if (const int32_t rc = ms_build_tables(p)) return rc;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0, tm = io->time_major != 0;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  const bool ptime = io->posture_per_waypoint != 0 && P.n_posture > 0, ctime = io->com_per_waypoint != 0 && P.n_com > 0;
  const size_t Bz = B, Tz = T, N = Bz * Tz, nq = P.nq, nv = P.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  const size_t ft_w = (size_t)P.n_frame * 7, pt_w = (size_t)P.n_posture * nq, ct_w = (size_t)P.n_com * 3;
  const size_t Kz = kf ? (size_t)kf->K : Tz;                 // the length of the targets' time axis
  const int S = cs ? cs->S : 1;
  const size_t Rz = Bz * (size_t)S, NR = Tz * Rz;            // rows of a loop launch (the candidates, or the instances), of all T
  const size_t pt_n = pt_w * (pbat ? Bz : 1) * (ptime ? Kz : 1), ct_n = ct_w * (cbat ? Bz : 1) * (ctime ? Kz : 1);
  Stager st{p, (hipStream_t)hip_stream, devp, who};
  if (cs) st.cand_bytes = NR * ((nq + nv) * f8 + 3 * i4);
  hipStream_t stream = st.stream;
  GrowBuf* const ws = p->ws;

  // ---- inputs and the caller-layout outputs on the device
  const double* const d_q = st.up(WS_IN_Q, q, Bz * nq);
  const double* d_ft = ft_w ? st.up(WS_IN_FT, frame_targets, Bz * Kz * ft_w) : frame_targets;
  const double* d_pt = pt_w ? st.up(WS_IN_PT, posture_target, pt_n) : posture_target;
  const double* d_ct = ct_w ? st.up(WS_IN_CT, com_target, ct_n) : com_target;
  double *o_q = io->q_traj, *o_v = io->v_traj, *o_qvel = io->qvel;
  int32_t *o_st = io->status, *o_it = io->iters, *o_cv = io->converged;
  if (!devp) {
    o_q = st.f64(WS_OUT_Q, N * nq); o_v = st.f64(WS_OUT_V, N * nv);
    o_qvel = io->qvel ? st.f64(WS_OUT_QVEL, N * nv) : nullptr;
    o_st = st.i32(WS_OUT_I32, 3 * N);
    o_it = io->iters ? o_st + N : nullptr;
    o_cv = io->converged ? o_st + 2 * N : nullptr;
  }
  // ---- candidates: optional inputs and the per-instance outputs on the device
  const double *d_user = nullptr, *d_w = nullptr;
  int32_t *o_si = nullptr, *o_nt = nullptr, *o_nc = nullptr;
  double* o_len = nullptr;
  if (cs) {
    d_user = st.up(WS_IN_SEEDS, cs->seeds, Rz * nq); d_w = st.up(WS_IN_W, cs->weights, nv);
    o_si = cs->seed_index; o_nt = cs->n_tracked; o_nc = cs->n_complete; o_len = cs->path_length;
    if (!devp) {
      o_si = st.i32(WS_OUT_PICK, 3 * Bz); o_nt = o_si + Bz; o_nc = o_si + 2 * Bz;
      o_len = st.f64(WS_OUT_LEN, Bz);
    }
  }
  TmfDev tf{};
  if (checked) tf = tmf_stage(st, *cs->fio, N, Bz, NR);
  // ---- keyframes: one slab per target group for all waypoints; the interpolated targets, where asked for, in the caller's layout
  double *k_ft = nullptr, *k_pt = nullptr, *k_ct = nullptr, *k_ft_out = nullptr, *k_pt_out = nullptr, *k_ct_out = nullptr;
  const size_t pt_rows = pbat ? Bz : 1, ct_rows = cbat ? Bz : 1;
  if (kf) {
    k_ft_out = ft_w ? kf->ft_out : nullptr; k_pt_out = ptime ? kf->pt_out : nullptr; k_ct_out = ctime ? kf->ct_out : nullptr;
    if (ft_w) k_ft = st.f64(WS_KF_FT, Bz * ft_w);
    if (ptime) k_pt = st.f64(WS_KF_PT, pt_rows * pt_w);
    if (ctime) k_ct = st.f64(WS_KF_CT, ct_rows * ct_w);
    if (!devp) {
      if (k_ft_out) k_ft_out = st.f64(WS_OUT_FT, N * ft_w);
      if (k_pt_out) k_pt_out = st.f64(WS_OUT_PT, Tz * pt_rows * pt_w);
      if (k_ct_out) k_ct_out = st.f64(WS_OUT_CT, Tz * ct_rows * ct_w);
    }
  }
  // ---- what the loops read and write: time-major slabs.  A time-major call: the caller's own arrays; a batch-major call:
  //      transposed copies of the targets and a workspace for the results
  //      Candidates: the loops' results are (T, B·S, .) arrays of their own — the caller's *_all where they are device
  //      buffers, else the handle's workspace —, the starts sit beside them
  double *l_q = o_q, *l_v = o_v;
  int32_t *l_st = o_st, *l_it = o_it, *l_cv = o_cv;
  double *d_seeds = nullptr, *c_ft = nullptr, *c_pt = nullptr, *c_ct = nullptr;
  if (cs) {
    l_q = (double*)st.given_or(WS_C_Q, cs->q_all, NR * nq * f8);
    l_v = (double*)st.given_or(WS_C_V, cs->v_all, NR * nv * f8);
    l_st = (int32_t*)st.given_or(WS_C_ST, cs->status_all, NR * i4);
    l_it = (int32_t*)st.given_or(WS_C_IT, cs->iters_all, NR * i4);
    l_cv = (int32_t*)st.given_or(WS_C_CV, cs->converged_all, NR * i4);
    d_seeds = (double*)st.given_or(WS_C_STARTS, cs->seeds_out, Rz * nq * f8);
    if (S > 1) {
      if (ft_w) c_ft = st.f64(WS_C_FT, Rz * ft_w);
      if (pt_w && pbat) c_pt = st.f64(WS_C_PT, Rz * pt_w);
      if (ct_w && cbat) c_ct = st.f64(WS_C_CT, Rz * ct_w);
    }
  } else if (!tm) {
    l_q = st.f64(WS_TM_Q, N * nq); l_v = st.f64(WS_TM_V, N * nv);
    l_st = st.i32(WS_TM_I32, 3 * N);
    l_it = o_it ? l_st + N : nullptr;
    l_cv = o_cv ? l_st + 2 * N : nullptr;
  }
  if (!tm && !kf) {                  // (keyframes are read in place through strides: no transposed copy)
    auto time_major = [&](WsRole role, const double* src, size_t w) -> const double* {
      double* const dst = st.f64(role, N * w);
      ST_LAUNCH(st, launch_tj_gather(stream, src, dst, B, T, (int)w));
      return dst;
    };
    if (ft_w) d_ft = time_major(WS_TM_FT, d_ft, ft_w);
    if (ptime && pbat) d_pt = time_major(WS_TM_PT, d_pt, pt_w);      // (a target without a B axis has its T axis in front already)
    if (ctime && cbat) d_ct = time_major(WS_TM_CT, d_ct, ct_w);
  }
  // ---- the waypoints: one loop launch each on the caller's stream, slab t - 1 → slab t, nothing in between
  const int32_t loop_flags = flags | MKH_FLAG_DEVICE_PTRS;
  const size_t pt_step = ptime ? pt_w * (pbat ? Bz : 1) : 0, ct_step = ctime ? ct_w * (cbat ? Bz : 1) : 0;
  int32_t rc = MKH_OK;
  // (instance, keyframe) strides of a keyframe array and the (instance stride, waypoint stride) of a *_targets_out, in
  // elements, for a group of `rows` rows of width w
  auto key_sb = [&](size_t rows, size_t w) { return (long long)(rows == 1 ? 0 : (tm ? w : Kz * w)); };
  auto key_sk = [&](size_t rows, size_t w) { return (long long)(tm ? rows * w : w); };
  auto out_sb = [&](size_t rows, size_t w) { return (long long)(rows == 1 ? 0 : (tm ? w : Tz * w)); };
  auto out_st = [&](size_t rows, size_t w) { return tm ? rows * w : w; };
  if (cs) {
    // the starts (candidate 0: q[b] itself), and a batched target that is held: fanned out once, in front of waypoint 0
    if (tab) {                        // the S − 1 entries nearest to waypoint 0's targets (d_ft is time-major here: its first slab)
      double* const slab = st.f64(WS_IN_SEEDS, Rz * nq);
      ST_LAUNCH(st, launch_st_query(stream, tab->d_keys, tab->d_q, tab->d_w, tab->N, P.n_frame, (int)nq, B, d_ft, S - 1, nullptr,
                                    nullptr, slab));
      d_user = slab;
    }
    ST_LAUNCH(st, launch_ms_seed(stream, ws[WS_SEED_I].i32(), ws[WS_SEED_F].f64(), B, S, (int)nq, d_q, d_user,
                                 (unsigned long long)cs->rng_seed, (long long)cs->target_index0, d_seeds));
    if (S > 1 && pt_w && pbat && !ptime) { ST_LAUNCH(st, launch_ms_fanout(stream, d_pt, c_pt, B, S, (int)pt_w)); d_pt = c_pt; }
    if (S > 1 && ct_w && cbat && !ctime) { ST_LAUNCH(st, launch_ms_fanout(stream, d_ct, c_ct, B, S, (int)ct_w)); d_ct = c_ct; }
  }
  for (size_t t = 0; t < Tz && rc == MKH_OK && st.ok(); ++t) {
    const double* const q_in = t ? l_q + (t - 1) * Rz * nq : (cs ? d_seeds : d_q);
    const double *t_ft = nullptr, *t_pt = d_pt, *t_ct = d_ct;       // (held targets: the same array for every waypoint)
    if (!kf) {
      t_ft = d_ft ? d_ft + t * Bz * ft_w : nullptr;
      t_pt = d_pt ? d_pt + t * pt_step : nullptr;
      t_ct = d_ct ? d_ct + t * ct_step : nullptr;
    } else {
      const int k = kf->seg_k[t];
      const double u = kf->seg_u[t];
      if (ft_w) {
        ST_LAUNCH(st, launch_kf_frames(stream, d_ft, key_sb(Bz, ft_w), key_sk(Bz, ft_w), k, u, B, P.n_frame, k_ft,
                                       k_ft_out ? k_ft_out + t * out_st(Bz, ft_w) : nullptr, out_sb(Bz, ft_w)));
        t_ft = k_ft;
      }
      if (ptime) {
        ST_LAUNCH(st, launch_kf_posture(stream, ws[WS_JNT].i32(), p->model->njnt, d_pt, key_sb(pt_rows, pt_w), key_sk(pt_rows, pt_w),
                                        k, u, (int)pt_rows, P.n_posture, (int)nq, k_pt,
                                        k_pt_out ? k_pt_out + t * out_st(pt_rows, pt_w) : nullptr, out_sb(pt_rows, pt_w)));
        t_pt = k_pt;
      }
      if (ctime) {
        ST_LAUNCH(st, launch_kf_com(stream, d_ct, key_sb(ct_rows, ct_w), key_sk(ct_rows, ct_w), k, u, (int)ct_rows, (int)ct_w, k_ct,
                                    k_ct_out ? k_ct_out + t * out_st(ct_rows, ct_w) : nullptr, out_sb(ct_rows, ct_w)));
        t_ct = k_ct;
      }
    }
    if (cs && S > 1) {
      // waypoint t's (B, .) slabs repeated for the S candidates of every instance, into the ONE (B·S, .) slab of each group
      if (ft_w) { ST_LAUNCH(st, launch_ms_fanout(stream, t_ft, c_ft, B, S, (int)ft_w)); t_ft = c_ft; }
      if (ptime && pbat) { ST_LAUNCH(st, launch_ms_fanout(stream, t_pt, c_pt, B, S, (int)pt_w)); t_pt = c_pt; }
      if (ctime && cbat) { ST_LAUNCH(st, launch_ms_fanout(stream, t_ct, c_ct, B, S, (int)ct_w)); t_ct = c_ct; }
    }
    if (!st.ok()) break;
    SolveCall sc;
    sc.p = p; sc.B = (int32_t)Rz; sc.q = q_in; sc.frame_targets = t_ft; sc.posture_target = t_pt; sc.com_target = t_ct;
    sc.dt = dt; sc.damping = damping; sc.v_out = l_v + t * Rz * nv; sc.status_out = l_st + t * Rz; sc.flags = loop_flags; sc.hip_stream = hip_stream;
    sc.n_steps = n_steps; sc.q_out = l_q + t * Rz * nq;
    if (until) { sc.pos_threshold = pos_threshold; sc.ori_threshold = ori_threshold; }
    sc.iters_out = l_it ? l_it + t * Rz : nullptr; sc.converged_out = l_cv ? l_cv + t * Rz : nullptr;
    rc = solve(sc);
  }
  if (rc != MKH_OK || !st.ok()) return st.finish(rc);
  // (instance, waypoint) strides in elements of an array of width w in the caller's layout
  auto sb = [&](size_t w) { return (long long)(tm ? w : Tz * w); };
  auto sw = [&](size_t w) { return (long long)(tm ? Bz * w : w); };
  if (cs) {
    // the score over every candidate's path and the choice, then the chosen rows into the caller's layout
    // (with a checker: one launch over all T·B·S rows behind the last loop — nodes, the status bit, edges — and the score on them)
    if (checked) tmf_check(st, cs->ck, B, S, T, cs->M, l_q, l_cv, l_st, tf.nm_all, tf.em_all);
    ST_LAUNCH(st, launch_tms_score(stream, B, S, T, (int)nq, p->model->njnt, ws[WS_JNT].i32(), d_q, l_q, l_st, l_cv, d_w,
                                   checked ? tf.em_all : nullptr, o_si, o_nt, o_nc, o_len));
    ST_LAUNCH(st, launch_tms_gather(stream, l_q, o_q, o_si, B, S, T, (int)nq, sb(nq), sw(nq)));
    ST_LAUNCH(st, launch_tms_gather(stream, l_v, o_v, o_si, B, S, T, (int)nv, sb(nv), sw(nv)));
    ST_LAUNCH(st, launch_tms_gather_i32(stream, l_st, o_st, o_si, B, S, T, sb(1), sw(1)));
    ST_LAUNCH(st, launch_tms_gather_i32(stream, l_it, o_it, o_si, B, S, T, sb(1), sw(1)));
    ST_LAUNCH(st, launch_tms_gather_i32(stream, l_cv, o_cv, o_si, B, S, T, sb(1), sw(1)));
    if (checked) tmf_chosen(st, B, S, T, o_si, l_cv, l_st, tf, sb(1), sw(1));
    if (o_qvel)
      ST_LAUNCH(st, launch_tj_qvel(stream, ws[WS_JNT].i32(), p->model->njnt, B, T, (int)nq, d_q, o_q, sb(nq), sw(nq), io->waypoint_dt,
                                   o_qvel, sb(nv), sw(nv), tm ? 1 : 0));
  } else {
    if (!tm) {
      ST_LAUNCH(st, launch_tj_scatter(stream, l_q, o_q, B, T, (int)nq));
      ST_LAUNCH(st, launch_tj_scatter(stream, l_v, o_v, B, T, (int)nv));
      ST_LAUNCH(st, launch_tj_scatter_i32(stream, l_st, o_st, B, T));
      if (o_it) ST_LAUNCH(st, launch_tj_scatter_i32(stream, l_it, o_it, B, T));
      if (o_cv) ST_LAUNCH(st, launch_tj_scatter_i32(stream, l_cv, o_cv, B, T));
    }
    if (o_qvel)                      // (from the loops' time-major q, into the caller's layout)
      ST_LAUNCH(st, launch_tj_qvel(stream, ws[WS_JNT].i32(), p->model->njnt, B, T, (int)nq, d_q, l_q, (long long)nq,
                                   (long long)(Bz * nq), io->waypoint_dt, o_qvel, sb(nv), sw(nv), tm ? 1 : 0));
  }
  if (devp) return st.finish();
  st.down(io->q_traj, o_q, N * nq * f8);
  st.down(io->v_traj, o_v, N * nv * f8);
  st.down(io->status, o_st, N * i4);
  st.down(io->iters, o_it, N * i4);
  st.down(io->converged, o_cv, N * i4);
  st.down(io->qvel, o_qvel, N * nv * f8);
  if (kf) {
    st.down(kf->ft_out, k_ft_out, N * ft_w * f8);
    st.down(kf->pt_out, k_pt_out, Tz * pt_rows * pt_w * f8);
    st.down(kf->ct_out, k_ct_out, Tz * ct_rows * ct_w * f8);
  }
  if (cs) {
    st.down(cs->seed_index, o_si, Bz * i4);
    st.down(cs->n_tracked, o_nt, Bz * i4);
    st.down(cs->n_complete, o_nc, Bz * i4);
    st.down(cs->path_length, o_len, Bz * f8);
    st.down(cs->seeds_out, d_seeds, Rz * nq * f8);
    st.down(cs->q_all, l_q, NR * nq * f8);
    st.down(cs->v_all, l_v, NR * nv * f8);
    st.down(cs->status_all, l_st, NR * i4);
    st.down(cs->iters_all, l_it, NR * i4);
    st.down(cs->converged_all, l_cv, NR * i4);
    if (checked) tmf_down(st, *cs->fio, tf, N, Bz, NR);
  }
  return st.finish();
}

extern "C" {

int32_t mkh_solve_trajectory(MkhProblem* p, int32_t B, int32_t T, const double* q, const double* frame_targets,
                             const double* posture_target, const double* com_target, double dt, double damping,
                             int32_t n_steps, double pos_threshold, double ori_threshold, const MkhTrajectoryIO* io,
                             int32_t flags, void* hip_stream) {
  return trajectory_core(p, B, T, q, frame_targets, posture_target, com_target, dt, damping, n_steps, pos_threshold,
                         ori_threshold, io, flags, hip_stream, nullptr, nullptr, "mkh_solve_trajectory");
}

int32_t mkh_solve_keyframes(MkhProblem* p, int32_t B, int32_t K, int32_t T, const double* q, const double* frame_keys,
                            const double* posture_keys, const double* com_keys, const double* key_times,
                            const double* waypoint_times, double dt, double damping, int32_t n_steps, double pos_threshold,
                            double ori_threshold, const MkhKeyframeIO* io, int32_t flags, void* hip_stream) {
  // the trajectory call's view of the struct: same outputs, a K axis where *_per_waypoint puts the T axis
  MkhTrajectoryIO tio;
  KeyframeSpec kf;
  kf.K = K; kf.key_times = key_times; kf.waypoint_times = waypoint_times;
  kf.ft_out = kf.pt_out = kf.ct_out = nullptr;
  if (io) {
    tio.q_traj = io->q_traj; tio.v_traj = io->v_traj; tio.status = io->status; tio.iters = io->iters;
    tio.converged = io->converged; tio.qvel = io->qvel; tio.waypoint_dt = io->waypoint_dt;
    tio.posture_per_waypoint = io->posture_keyframed; tio.com_per_waypoint = io->com_keyframed; tio.time_major = io->time_major;
    kf.ft_out = io->frame_targets_out; kf.pt_out = io->posture_targets_out; kf.ct_out = io->com_targets_out;
  }
  return trajectory_core(p, B, T, q, frame_keys, posture_keys, com_keys, dt, damping, n_steps, pos_threshold, ori_threshold,
                         io ? &tio : nullptr, flags, hip_stream, &kf, nullptr, "mkh_solve_keyframes");
}

int32_t mkh_solve_trajectory_multistart(MkhProblem* p, int32_t B, int32_t T, int32_t n_seeds, const double* q,
                                        const double* frame_targets, const double* posture_target, const double* com_target,
                                        double dt, double damping, int32_t n_steps, double pos_threshold, double ori_threshold,
                                        uint64_t rng_seed, int64_t target_index0, const MkhTrajectoryMultistartIO* io,
                                        int32_t flags, void* hip_stream) {
  // the trajectory call's view of the struct: the chosen candidate's outputs; everything about the candidates beside it
  MkhTrajectoryIO tio;
  CandidateSpec cs{};
  cs.S = n_seeds; cs.rng_seed = rng_seed; cs.target_index0 = target_index0;
  if (io) {
    tio.q_traj = io->q_traj; tio.v_traj = io->v_traj; tio.status = io->status; tio.iters = io->iters;
    tio.converged = io->converged; tio.qvel = io->qvel; tio.waypoint_dt = io->waypoint_dt;
    tio.posture_per_waypoint = io->posture_per_waypoint; tio.com_per_waypoint = io->com_per_waypoint; tio.time_major = io->time_major;
    cs.seeds = io->seeds; cs.weights = io->weights;
    cs.seed_index = io->seed_index; cs.n_tracked = io->n_tracked; cs.n_complete = io->n_complete; cs.path_length = io->path_length;
    cs.seeds_out = io->seeds_out; cs.q_all = io->q_all; cs.v_all = io->v_all;
    cs.status_all = io->status_all; cs.iters_all = io->iters_all; cs.converged_all = io->converged_all;
  }
  return trajectory_core(p, B, T, q, frame_targets, posture_target, com_target, dt, damping, n_steps, pos_threshold, ori_threshold,
                         io ? &tio : nullptr, flags, hip_stream, nullptr, &cs, "mkh_solve_trajectory_multistart");
}

int32_t mkh_solve_trajectory_multistart_free(MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, int32_t n_seeds, const double* q,
                                             const double* frame_targets, const double* posture_target, const double* com_target,
                                             double dt, double damping, int32_t n_steps, double pos_threshold, double ori_threshold,
                                             uint64_t rng_seed, int64_t target_index0, int32_t n_samples,
                                             const MkhTrajectoryMultistartIO* io, const MkhTrajectoryFreeIO* fio, int32_t flags,
                                             void* hip_stream) {
  // mkh_solve_trajectory_multistart's view of the call, with the checker beside it
  MkhTrajectoryIO tio;
  CandidateSpec cs{};
  cs.S = n_seeds; cs.rng_seed = rng_seed; cs.target_index0 = target_index0;
  cs.checked = true; cs.ck = ck; cs.M = n_samples; cs.fio = fio;
  if (io) {
    tio.q_traj = io->q_traj; tio.v_traj = io->v_traj; tio.status = io->status; tio.iters = io->iters;
    tio.converged = io->converged; tio.qvel = io->qvel; tio.waypoint_dt = io->waypoint_dt;
    tio.posture_per_waypoint = io->posture_per_waypoint; tio.com_per_waypoint = io->com_per_waypoint; tio.time_major = io->time_major;
    cs.seeds = io->seeds; cs.weights = io->weights;
    cs.seed_index = io->seed_index; cs.n_tracked = io->n_tracked; cs.n_complete = io->n_complete; cs.path_length = io->path_length;
    cs.seeds_out = io->seeds_out; cs.q_all = io->q_all; cs.v_all = io->v_all;
    cs.status_all = io->status_all; cs.iters_all = io->iters_all; cs.converged_all = io->converged_all;
  }
  return trajectory_core(p, B, T, q, frame_targets, posture_target, com_target, dt, damping, n_steps, pos_threshold, ori_threshold,
                         io ? &tio : nullptr, flags, hip_stream, nullptr, &cs, "mkh_solve_trajectory_multistart_free");
}

// The selection alone, over the caller's own candidates: the score and the choice of "THE RULE" on the caller's flags, or — with
// a checker — of "THE RULE, with a checker" with `tracked` for converged_all and a status of zeros.
int32_t mkh_select_trajectory_candidates(MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, int32_t S, const double* q,
                                         const double* q_paths, const int32_t* tracked, const double* weights, int32_t n_samples,
                                         const MkhTrajectoryCandidatesIO* io, const MkhTrajectoryFreeIO* fio, int32_t flags,
                                         void* hip_stream) {
  const char* const who = "mkh_select_trajectory_candidates";
  if (B < 1) return fail(MKH_E_INVALID, "%s: B = %d must be >= 1", who, B);
  if (T < 1) return fail(MKH_E_INVALID, "%s: T = %d must be >= 1", who, T);
  if (S < 1) return fail(MKH_E_INVALID, "%s: S = %d must be >= 1", who, S);
  if (flags & ~MKH_FLAG_DEVICE_PTRS) return fail(MKH_E_INVALID, "%s: flags = %d: only MKH_FLAG_DEVICE_PTRS is accepted", who, flags);
  if (!q || !q_paths) return fail(MKH_E_INVALID, "%s: q and q_paths are required", who);
  if (!io || !io->seed_index || !io->n_tracked || !io->n_complete || !io->path_length)
    return fail(MKH_E_INVALID, "%s: io and its outputs seed_index, n_tracked, n_complete, path_length are required", who);
  if (!ck && fio) return fail(MKH_E_INVALID, "%s: free_io is given without a checker: free_io is NULL iff checker is NULL", who);
  if (ck)
    if (const int32_t rc = tmf_refuse_args(n_samples, fio, who)) return rc;
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (ck)
    if (const int32_t rc = sweep_refuse_for(p, ck, who, CheckerUse::tracking(n_samples))) return rc;
  if ((long long)B * S * T > 0x7fffffffLL)
    return fail(MKH_E_LIMIT, "%s: B * S * T = %lld rows, at most 2^31 - 1", who, (long long)B * S * T);
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  const size_t Bz = B, N = Bz * T, Rz = Bz * S, NR = Rz * T, nq = p->dev.nq, nv = p->dev.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  for (size_t k = 0; !devp && weights && k < nv; ++k)
    if (!(weights[k] >= 0.0)) return fail(MKH_E_INVALID, "%s: weights[%zu] = %g: the weights of the length must be >= 0", who, k, weights[k]);
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  Stager st{p, (hipStream_t)hip_stream, devp, "select_trajectory_candidates"};
  const double* const d_q = st.up(WS_IN_Q, q, Bz * nq);
  const double* const d_paths = st.up(WS_C_Q, q_paths, NR * nq);
  const double* const d_w = st.up(WS_IN_W, weights, nv);
  const int32_t* const d_trk = st.up_i32(WS_C_CV, tracked, NR);
  int32_t *o_si = io->seed_index, *o_nt = io->n_tracked, *o_nc = io->n_complete;
  double *o_len = io->path_length, *o_q = io->q_path;
  if (!devp) {
    o_si = st.i32(WS_OUT_PICK, 3 * Bz); o_nt = o_si ? o_si + Bz : nullptr; o_nc = o_si ? o_si + 2 * Bz : nullptr;
    o_len = st.f64(WS_OUT_LEN, Bz);
    o_q = io->q_path ? st.f64(WS_OUT_Q, N * nq) : nullptr;
  }
  TmfDev tf{};
  int32_t* d_st = nullptr;           // with a checker: the status the rule takes as 0, and the kernel ORs its bit into
  if (ck) {
    tf = tmf_stage(st, *fio, N, Bz, NR);
    d_st = st.i32(WS_C_ST, NR);
  }
  if (!st.ok()) return st.finish();
  if (ck) {
    st.latch(hipMemsetAsync(d_st, 0, NR * i4, st.stream));
    tmf_check(st, ck, B, S, T, n_samples, d_paths, d_trk, d_st, tf.nm_all, tf.em_all);
  }
  ST_LAUNCH(st, launch_tms_score(st.stream, B, S, T, (int)nq, p->model->njnt, p->ws[WS_JNT].i32(), d_q, d_paths, d_st, d_trk, d_w,
                                 ck ? tf.em_all : nullptr, o_si, o_nt, o_nc, o_len));
  if (o_q) ST_LAUNCH(st, launch_tms_gather(st.stream, d_paths, o_q, o_si, B, S, T, (int)nq, (long long)(T * nq), (long long)nq));
  if (ck) tmf_chosen(st, B, S, T, o_si, d_trk, d_st, tf, (long long)T, 1);
  if (devp) return st.finish();
  st.down(io->seed_index, o_si, Bz * i4);
  st.down(io->n_tracked, o_nt, Bz * i4);
  st.down(io->n_complete, o_nc, Bz * i4);
  st.down(io->path_length, o_len, Bz * f8);
  st.down(io->q_path, o_q, N * nq * f8);
  if (ck) tmf_down(st, *fio, tf, N, Bz, NR);
  return st.finish();
}

// ---- ladder-graph trajectory IK (include/minkhip.h "THE RULE"; kernels: ladder.hip)
// What both ladder entry points refuse about the graph's shape and gate.
static int32_t ladder_refuse(const MkhProblem* p, int32_t B, int32_t T, int32_t S, double max_step_sq, const char* who) {
  if (B < 1) return fail(MKH_E_INVALID, "%s: B = %d must be >= 1", who, B);
  if (T < 1) return fail(MKH_E_INVALID, "%s: T = %d must be >= 1", who, T);
  if (S < 1) return fail(MKH_E_INVALID, "%s: S = %d must be >= 1", who, S);
  if (S > 256) return fail(MKH_E_LIMIT, "%s: S = %d nodes per rung, at most 256 (back-pointers are bytes)", who, S);
  if (T > 65535) return fail(MKH_E_LIMIT, "%s: T = %d waypoints, at most 65535", who, T);
  if (!(max_step_sq >= 0.0)) return fail(MKH_E_INVALID, "%s: max_step_sq = %g must be >= 0 (+inf: no gate)", who, max_step_sq);
  if (ladder_source_tile(S, p->dev.nq, p->dev.nv, p->model->njnt, nullptr) < 1)
    return fail(MKH_E_LIMIT, "%s: nq = %d: one destination tile and one source node do not fit 64 KB of LDS", who, p->dev.nq);
  if ((long long)B * T > 0x7fffffffLL) return fail(MKH_E_LIMIT, "%s: B * T = %lld rows", who, (long long)B * T);
  return MKH_OK;
}

// The search on device arrays, into device outputs, on the call's stream.
static void ladder_search(Stager& st, int B, int T, int S, const double* d_q, const double* d_nodes, const int32_t* d_tracked,
                          const double* d_w, double max_step_sq, int32_t* o_node, int32_t* o_nt, int32_t* o_nb, double* o_len,
                          int32_t* o_eb) {
  const MkhProblem* const p = st.p;
  const size_t R = (size_t)B * T, nch = ((size_t)S + 63) / 64;
  unsigned long long* const brk = (unsigned long long*)st.need(WS_L_PRED, R * nch * 8 + R * S);
  uint8_t* const pred = (uint8_t*)(brk + R * nch);
  ST_LAUNCH(st, launch_ladder_search(st.stream, B, T, S, p->dev.nq, p->dev.nv, p->model->njnt, p->ws[WS_JNT].i32(), d_q, d_nodes, d_tracked, d_w,
                                     max_step_sq, pred, brk, o_node, o_nt, o_nb, o_len, o_eb));
}

static int32_t ladder_weights_refuse(const double* w, int nv, const char* who) {
  for (int k = 0; w && k < nv; ++k)
    if (!(w[k] >= 0.0)) return fail(MKH_E_INVALID, "%s: weights[%d] = %g: the weights of the edge cost must be >= 0", who, k, w[k]);
  return MKH_OK;
}

int32_t mkh_ladder_select(MkhProblem* p, int32_t B, int32_t T, int32_t S, const double* q, const double* q_nodes,
                          const int32_t* tracked, const double* weights, double max_step_sq, const MkhLadderIO* io, int32_t flags,
                          void* hip_stream) {
  const char* const who = "mkh_ladder_select";
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (const int32_t rc = ladder_refuse(p, B, T, S, max_step_sq, who)) return rc;
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;
  if (!q || !q_nodes || !tracked) return fail(MKH_E_INVALID, "%s: q, q_nodes and tracked are required", who);
  if (!io || !io->node_index || !io->n_tracked || !io->n_breaks || !io->path_length || !io->edge_break)
    return fail(MKH_E_INVALID, "%s: io and its outputs node_index, n_tracked, n_breaks, path_length, edge_break are required", who);
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  if (!devp)
    if (const int32_t rc = ladder_weights_refuse(weights, p->dev.nv, who)) return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  Stager st{p, (hipStream_t)hip_stream, devp, "ladder_select"};
  const size_t Bz = B, R = Bz * T, N = R * S, nq = p->dev.nq, f8 = sizeof(double), i4 = sizeof(int32_t);
  const double* const d_q = st.up(WS_IN_Q, q, Bz * nq);
  const double* const d_nodes = st.up(WS_L_Q, q_nodes, N * nq);
  const double* const d_w = st.up(WS_IN_W, weights, p->dev.nv);
  const int32_t* const d_trk = st.up_i32(WS_L_TRK, tracked, N);
  int32_t *o_node = io->node_index, *o_eb = io->edge_break, *o_nt = io->n_tracked, *o_nb = io->n_breaks;
  double *o_len = io->path_length, *o_q = io->q_path;
  if (!devp) {
    o_node = st.i32(WS_OUT_PICK, 2 * R + 2 * Bz); o_eb = o_node + R; o_nt = o_node + 2 * R; o_nb = o_nt + Bz;
    o_len = st.f64(WS_OUT_LEN, Bz);
    o_q = io->q_path ? st.f64(WS_OUT_Q, R * nq) : nullptr;
  }
  if (!st.ok()) return st.finish();
  ladder_search(st, B, T, S, d_q, d_nodes, d_trk, d_w, max_step_sq, o_node, o_nt, o_nb, o_len, o_eb);
  if (o_q) ST_LAUNCH(st, launch_ladder_gather(st.stream, d_nodes, o_q, o_node, (long long)R, S, (int)nq));
  if (devp) return st.finish();
  st.down(io->node_index, o_node, R * i4);
  st.down(io->edge_break, o_eb, R * i4);
  st.down(io->n_tracked, o_nt, Bz * i4);
  st.down(io->n_breaks, o_nb, Bz * i4);
  st.down(io->path_length, o_len, Bz * f8);
  st.down(io->q_path, o_q, R * nq * f8);
  return st.finish();
}

// ---- the checked ladder (include/minkhip.h THE RULE "with a checker"; kernels: sweep.hip, ladder.hip)
// How a checked ladder call judges an edge: M interior samples (THE RULE "with a checker"), or — certified — THE RULE OF THE
// CERTIFIED SWEEP at a resolution, a cap and a policy (THE RULE "with a certifying checker").
struct EdgeRule {
  int M = 0;
  bool certified = false;
  double resolution = 0.0;
  int32_t max_samples = 0, policy = 0;
  CheckerUse use(bool refined) const { return certified ? CheckerUse::certified() : CheckerUse::ladder(M, refined); }
};

// device arrays: the back-trace's (B, T) / (B,) outputs and every edge's margin or NULL; behind them the certified rule's — the
// chosen edges' verdict, lower bound and count, n_certified, every edge's verdict or NULL (all NULL under the sampled rule)
struct LadderFreeOut {
  int32_t *edge_collision, *n_edge_collisions;
  double *edge_margin, *edge_margin_all;
  int32_t* edge_verdict = nullptr;
  double* edge_lower_bound = nullptr;
  int32_t *edge_n_samples = nullptr, *n_certified = nullptr;
  int8_t* edge_verdict_all = nullptr;
};

// The device side of a checked call's edge outputs: the caller's arrays for a device-pointer call, else workspace (F_OUT_I:
// edge_collision | n_edge_collisions | edge_verdict | edge_n_samples | n_certified; F_OUT_F: edge_margin | edge_lower_bound).
static LadderFreeOut ladder_free_out(Stager& st, int B, int T, int W, const EdgeRule& rule, const MkhLadderFreeIO* fio,
                                     const MkhLadderCertifiedIO* cio) {
  const size_t Bz = B, R = Bz * T;
  const bool cert = rule.certified;
  LadderFreeOut o{fio->edge_collision, fio->n_edge_collisions, fio->edge_margin, fio->edge_margin_all};
  if (cert) {
    o.edge_verdict = cio->edge_verdict; o.edge_lower_bound = cio->edge_lower_bound; o.edge_n_samples = cio->edge_n_samples;
    o.n_certified = cio->n_certified; o.edge_verdict_all = cio->edge_verdict_all;
  }
  if (st.devp) return o;
  o.edge_collision = st.i32(WS_F_OUT_I, cert ? 3 * R + 2 * Bz : R + Bz);
  o.n_edge_collisions = o.edge_collision ? o.edge_collision + R : nullptr;
  o.edge_margin = st.f64(WS_F_OUT_F, cert ? 2 * R : R);
  if (o.edge_margin_all) o.edge_margin_all = st.f64(WS_F_EMARGIN, R * W * W);
  if (cert && st.ok()) {
    o.edge_verdict = o.n_edge_collisions + Bz; o.edge_n_samples = o.edge_verdict + R; o.n_certified = o.edge_n_samples + R;
    o.edge_lower_bound = o.edge_margin + R;
    if (o.edge_verdict_all) o.edge_verdict_all = (int8_t*)st.need(WS_F_EVERDICT, R * W * W);
  }
  return o;
}

static void ladder_free_out_down(Stager& st, int B, int T, int W, const LadderFreeOut& o, const MkhLadderFreeIO* fio,
                                 const MkhLadderCertifiedIO* cio) {
  const size_t Bz = B, R = Bz * T, f8 = sizeof(double), i4 = sizeof(int32_t);
  st.down(fio->edge_collision, o.edge_collision, R * i4);
  st.down(fio->n_edge_collisions, o.n_edge_collisions, Bz * i4);
  st.down(fio->edge_margin, o.edge_margin, R * f8);
  st.down(fio->edge_margin_all, o.edge_margin_all, R * W * W * f8);
  if (!cio) return;
  st.down(cio->edge_verdict, o.edge_verdict, R * i4);
  st.down(cio->edge_lower_bound, o.edge_lower_bound, R * f8);
  st.down(cio->edge_n_samples, o.edge_n_samples, R * i4);
  st.down(cio->n_certified, o.n_certified, Bz * i4);
  st.down(cio->edge_verdict_all, o.edge_verdict_all, R * W * W);
}

// The sweep of every edge into a tracked node, the masked search, and the chosen edges' margins — on device arrays, on the call's
// stream.  d_tracked: the EFFECTIVE flags.  The sampled rule: two launches of sweep_kernel around the search; the certified
// rule: two of certified_sweep_kernel in their place, and the count of the chosen edges that are proven free.
static void ladder_search_free(Stager& st, MkhProblem* ck, int B, int T, int S, const EdgeRule& rule, const double* d_q,
                               const double* d_nodes, const int32_t* d_tracked, const double* d_w, double max_step_sq, int32_t* o_node,
                               int32_t* o_nt, int32_t* o_nb, double* o_len, int32_t* o_eb, const LadderFreeOut& f) {
  const MkhProblem* const p = st.p;
  const size_t R = (size_t)B * T, nch = ((size_t)S + 63) / 64, E = R * S * S;
  uint8_t* const blocked = (uint8_t*)st.need(WS_F_BLOCK, E);
  unsigned long long* const brk = (unsigned long long*)st.need(WS_L_PRED, R * nch * 8 + R * S);
  uint8_t* const pred = (uint8_t*)(brk + R * nch);
  if (!st.ok()) return;
  // (rung 0 has no edges: its flags are never read, and its margins are NaN — every byte 0xff is one —, its verdicts −1 — too)
  if (f.edge_margin_all)
    ST_LAUNCH(st, hipMemset2DAsync(f.edge_margin_all, (size_t)T * S * S * sizeof(double), 0xff, (size_t)S * S * sizeof(double), B, st.stream));
  if (f.edge_verdict_all)
    ST_LAUNCH(st, hipMemset2DAsync(f.edge_verdict_all, (size_t)T * S * S, 0xff, (size_t)S * S, B, st.stream));
  mkh::CertifiedArgs ca{};
  ca.resolution = rule.resolution; ca.max_samples = rule.max_samples; ca.policy = rule.policy;
  ca.T = T; ca.W = S; ca.nodes = d_nodes; ca.tracked = d_tracked;
  if (T > 1) {
    if (rule.certified) {
      mkh::CertifiedArgs a = ca;
      a.mode = mkh::kSweepLadder; a.N = (long long)(E - (size_t)B * S * S);
      a.margin = f.edge_margin_all; a.blocked = blocked; a.verdict_all = f.edge_verdict_all;
      certify_edges(st, ck, a);
    } else {
      mkh::SweepArgs a{};
      a.mode = mkh::kSweepLadder; a.M = rule.M; a.T = T; a.W = S; a.N = (long long)(E - (size_t)B * S * S);
      a.nodes = d_nodes; a.tracked = d_tracked; a.margin = f.edge_margin_all; a.blocked = blocked;
      sweep_edges(st, ck, a);
    }
  }
  ST_LAUNCH(st, launch_ladder_search_free(st.stream, B, T, S, p->dev.nq, p->dev.nv, p->model->njnt, p->ws[WS_JNT].i32(), d_q, d_nodes,
                                          d_tracked, blocked, d_w, max_step_sq, pred, brk, o_node, o_nt, o_nb, o_len, o_eb,
                                          f.edge_collision, f.n_edge_collisions));
  if (rule.certified) {
    mkh::CertifiedArgs c = ca;
    c.mode = mkh::kSweepPath; c.N = (long long)R; c.node_index = o_node;
    c.margin = f.edge_margin; c.lower_bound = f.edge_lower_bound; c.n_samples = f.edge_n_samples; c.verdict = f.edge_verdict;
    certify_edges(st, ck, c);
    ST_LAUNCH(st, mkh::launch_certified_count(st.stream, B, T, f.edge_verdict, f.n_certified));
    return;
  }
  mkh::SweepArgs c{};
  c.mode = mkh::kSweepPath; c.M = rule.M; c.T = T; c.W = S; c.N = (long long)R;
  c.nodes = d_nodes; c.tracked = d_tracked; c.node_index = o_node; c.margin = f.edge_margin;
  sweep_edges(st, ck, c);
}

// What the checked calls refuse about the checker, the edge rule and the graph's size (cio: the certified rule's outputs).
static int32_t ladder_free_refuse(const MkhProblem* p, const MkhProblem* ck, int32_t B, int32_t T, int32_t S, const EdgeRule& rule,
                                  const MkhLadderFreeIO* f, const MkhLadderCertifiedIO* cio, const char* who, bool refined) {
  if (rule.certified) {                                        // (mkh_certified_sweep's argument checks, and the policy)
    if (!std::isfinite(rule.resolution) || !(rule.resolution > 0.0))
      return fail(MKH_E_INVALID, "%s: resolution = %g must be finite and > 0", who, rule.resolution);
    if (rule.max_samples < 1 || rule.max_samples > 4096)
      return fail(MKH_E_INVALID, "%s: max_samples = %d must be in [1, 4096]", who, rule.max_samples);
    if (rule.policy != MKH_EDGE_REJECT_COLLIDING && rule.policy != MKH_EDGE_REQUIRE_CERTIFIED)
      return fail(MKH_E_INVALID, "%s: edge_policy = %d: MKH_EDGE_REJECT_COLLIDING (0) or MKH_EDGE_REQUIRE_CERTIFIED (1)", who, rule.policy);
  }
  // (general convex pairs: through the checker's sweep_rows where the call sweeps and nothing else; with refinement through its
  //  check_rows as well; the certified rule refuses them whatever the buffers hold)
  if (const int32_t rc = sweep_refuse_for(p, ck, who, rule.use(refined))) return rc;
  if (!rule.certified && rule.M < 1) return fail(MKH_E_INVALID, "%s: n_samples = %d must be >= 1", who, rule.M);
  if (!f || !f->edge_collision || !f->n_edge_collisions || !f->edge_margin)
    return fail(MKH_E_INVALID, "%s: free_io and its outputs edge_collision, n_edge_collisions, edge_margin are required", who);
  if (rule.certified && (!cio || !cio->edge_verdict || !cio->edge_lower_bound || !cio->edge_n_samples || !cio->n_certified))
    return fail(MKH_E_INVALID, "%s: certified_io and its outputs edge_verdict, edge_lower_bound, edge_n_samples, n_certified are required", who);
  if ((long long)B * T * S * S > 0x7fffffffLL)
    return fail(MKH_E_LIMIT, "%s: B * T * S^2 = %lld edges, at most 2^31 - 1", who, (long long)B * T * S * S);
  return MKH_OK;
}

// mkh_ladder_select_free (cio == NULL) and mkh_ladder_select_certified.
static int32_t ladder_select_checked(const char* who, const char* tag, const EdgeRule& rule, MkhProblem* p, MkhProblem* ck, int32_t B,
                                     int32_t T, int32_t S, const double* q, const double* q_nodes, const int32_t* tracked,
                                     const double* weights, double max_step_sq, const MkhLadderIO* io, const MkhLadderFreeIO* fio,
                                     const MkhLadderCertifiedIO* cio, int32_t flags, void* hip_stream) {
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (const int32_t rc = ladder_refuse(p, B, T, S, max_step_sq, who)) return rc;
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;
  if (!q || !q_nodes || !tracked) return fail(MKH_E_INVALID, "%s: q, q_nodes and tracked are required", who);
  if (!io || !io->node_index || !io->n_tracked || !io->n_breaks || !io->path_length || !io->edge_break)
    return fail(MKH_E_INVALID, "%s: io and its outputs node_index, n_tracked, n_breaks, path_length, edge_break are required", who);
  if (const int32_t rc = ladder_free_refuse(p, ck, B, T, S, rule, fio, cio, who, false)) return rc;
  if (mkh::ladder_source_tile(S, p->dev.nq, p->dev.nv, p->model->njnt, nullptr, true) < 1)
    return fail(MKH_E_LIMIT, "%s: nq = %d: one destination tile and one source node with its flags do not fit 64 KB of LDS", who, p->dev.nq);
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  if (!devp)
    if (const int32_t rc = ladder_weights_refuse(weights, p->dev.nv, who)) return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  Stager st{p, (hipStream_t)hip_stream, devp, tag};
  const size_t Bz = B, R = Bz * T, N = R * S, nq = p->dev.nq, f8 = sizeof(double), i4 = sizeof(int32_t);
  const double* const d_q = st.up(WS_IN_Q, q, Bz * nq);
  const double* const d_nodes = st.up(WS_L_Q, q_nodes, N * nq);
  const double* const d_w = st.up(WS_IN_W, weights, p->dev.nv);
  const int32_t* const d_trk = st.up_i32(WS_L_TRK, tracked, N);
  int32_t *o_node = io->node_index, *o_eb = io->edge_break, *o_nt = io->n_tracked, *o_nb = io->n_breaks;
  double *o_len = io->path_length, *o_q = io->q_path;
  if (!devp) {
    o_node = st.i32(WS_OUT_PICK, 2 * R + 2 * Bz); o_eb = o_node + R; o_nt = o_node + 2 * R; o_nb = o_nt + Bz;
    o_len = st.f64(WS_OUT_LEN, Bz);
    o_q = io->q_path ? st.f64(WS_OUT_Q, R * nq) : nullptr;
  }
  const LadderFreeOut f = ladder_free_out(st, B, T, S, rule, fio, cio);
  double* const d_nm = (double*)st.given_or(WS_F_NMARGIN, fio->node_margin, N * f8);
  int32_t* const d_eff = st.i32(WS_F_TRK, N);
  if (!st.ok()) return st.finish();
  // ---- the nodes' clearance, their effective flags, the edges, the search
  clearance_rows(st, ck, N, d_nodes, d_nm, nullptr, nullptr, nullptr, nullptr);
  ST_LAUNCH(st, launch_ladder_free_tracked(st.stream, d_trk, d_nm, (long long)N, d_eff));
  ladder_search_free(st, ck, B, T, S, rule, d_q, d_nodes, d_eff, d_w, max_step_sq, o_node, o_nt, o_nb, o_len, o_eb, f);
  if (o_q) ST_LAUNCH(st, launch_ladder_gather(st.stream, d_nodes, o_q, o_node, (long long)R, S, (int)nq));
  if (devp) return st.finish();
  st.down(io->node_index, o_node, R * i4);
  st.down(io->edge_break, o_eb, R * i4);
  st.down(io->n_tracked, o_nt, Bz * i4);
  st.down(io->n_breaks, o_nb, Bz * i4);
  st.down(io->path_length, o_len, Bz * f8);
  st.down(io->q_path, o_q, R * nq * f8);
  st.down(fio->node_margin, d_nm, N * f8);
  ladder_free_out_down(st, B, T, S, f, fio, cio);
  return st.finish();
}

int32_t mkh_ladder_select_free(MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, int32_t S, const double* q, const double* q_nodes,
                               const int32_t* tracked, const double* weights, double max_step_sq, int32_t n_samples,
                               const MkhLadderIO* io, const MkhLadderFreeIO* fio, int32_t flags, void* hip_stream) {
  EdgeRule rule;
  rule.M = n_samples;
  return ladder_select_checked("mkh_ladder_select_free", "ladder_select_free", rule, p, ck, B, T, S, q, q_nodes, tracked, weights,
                               max_step_sq, io, fio, nullptr, flags, hip_stream);
}

int32_t mkh_ladder_select_certified(MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, int32_t S, const double* q,
                                    const double* q_nodes, const int32_t* tracked, const double* weights, double max_step_sq,
                                    double resolution, int32_t max_samples, int32_t edge_policy, const MkhLadderIO* io,
                                    const MkhLadderFreeIO* fio, const MkhLadderCertifiedIO* cio, int32_t flags, void* hip_stream) {
  EdgeRule rule;
  rule.certified = true; rule.resolution = resolution; rule.max_samples = max_samples; rule.policy = edge_policy;
  return ladder_select_checked("mkh_ladder_select_certified", "ladder_select_certified", rule, p, ck, B, T, S, q, q_nodes, tracked,
                               weights, max_step_sq, io, fio, cio, flags, hip_stream);
}

// The refinement pass (include/minkhip.h "THE RULE OF THE REFINEMENT") on device arrays, into device outputs, on the call's stream:
// the targets' time-major slabs as mkh_solve_trajectory builds them, the working path, then per waypoint of the two sweeps one
// step kernel and one loop launch through solve(), and the guard.  Returns the first refusal of a loop launch; HIP errors are
// latched in `st`.
// With a checker (rf != NULL: "THE RULE OF THE REFINEMENT, with a checker"; kernels: ladder_refine_free.hip and the _free builds of
// ladder_refine.hip) the state of the input path comes first — one clearance of its rows on the checker handle, one kSweepPath
// launch over it as a ladder of width 1 —, lr_check_kernel runs between every loop launch and its step kernel, and the guard
// compares on the amended key.  Nothing of it touches the plain pass.
struct RefineFree {
  MkhProblem* ck;
  int M;                           // samples per edge
  double *node_margin, *edge_margin;             // device outputs of the returned path, (B, T); node_margin: optional
  int32_t *edge_collision, *n_edge_collisions;   // (B, T), (B,)
};
static int32_t refine_pass(Stager& st, int B, int T, const double* d_q, const double* d_path, const int32_t* d_trk, const double* d_ft,
                           const double* d_pt, const double* d_ct, const LoopSpec& ls, const double* d_w, double max_step_sq,
                           const mkh::LrOut& out, int32_t flags, const RefineFree* rf = nullptr) {
  MkhProblem* const p = st.p;
  const DeviceProblem& P = p->dev;
  hipStream_t stream = st.stream;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  const size_t Bz = B, Tz = T, R = Bz * Tz, nq = P.nq, nv = P.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  const size_t ft_w = (size_t)P.n_frame * 7, pt_w = (size_t)P.n_posture * nq, ct_w = (size_t)P.n_com * 3;
  auto time_major = [&](WsRole role, const double* src, size_t w) -> const double* {
    double* const dst = st.f64(role, R * w);
    ST_LAUNCH(st, launch_tj_gather(stream, src, dst, B, T, (int)w));
    return dst;
  };
  if (ft_w) d_ft = time_major(WS_TM_FT, d_ft, ft_w);
  if (pt_w && pbat) d_pt = time_major(WS_TM_PT, d_pt, pt_w);
  if (ct_w && cbat) d_ct = time_major(WS_TM_CT, d_ct, ct_w);
  const size_t pt_step = (pt_w && pbat) ? Bz * pt_w : 0, ct_step = (ct_w && cbat) ? Bz * ct_w : 0;
  mkh::LrWork w;
  w.r = st.f64(WS_R_Q, R * nq); w.r_v = st.f64(WS_R_V, R * nv);
  w.r_trk = st.i32(WS_R_I32, 6 * R);
  w.r_rep = w.r_trk + R; w.r_st = w.r_trk + 2 * R; w.r_it = w.r_trk + 3 * R; w.r_cv = w.r_trk + 4 * R; w.r_eb = w.r_trk + 5 * R;
  w.start = st.f64(WS_R_X, Bz * (2 * nq + nv)); w.x = w.start + Bz * nq; w.xv = w.x + Bz * nq;
  w.xst = st.i32(WS_R_XI, 4 * Bz); w.xit = w.xst + Bz; w.xcv = w.xst + 2 * Bz; w.bad = w.xst + 3 * Bz;
  mkh::LrFreeWork fw{};
  double *p_nm = nullptr, *p_em = nullptr;
  int32_t *p_idx = nullptr, *p_eff = nullptr;
  if (rf) {
    p_nm = st.f64(WS_RF_MARGIN, 4 * R); p_em = p_nm + R; fw.r_nm = p_nm + 2 * R; fw.r_em = p_nm + 3 * R;
    fw.slots = mkh::lr_check_slots(rf->M);
    fw.trip = st.f64(WS_RF_TRIP, 3 * Bz * fw.slots);
    p_idx = st.i32(WS_RF_IDX, 2 * R); p_eff = p_idx + R;
  }
  if (!st.ok()) return MKH_OK;
  if (rf) {                                                  // the state of p: its nodes' margins, effective flags, edges' margins
    clearance_rows(st, rf->ck, R, d_path, p_nm, nullptr, nullptr, nullptr, nullptr);
    ST_LAUNCH(st, launch_ladder_free_tracked(stream, d_trk, p_nm, (long long)R, p_eff));
    st.latch(hipMemsetAsync(p_idx, 0, R * i4, stream));
    mkh::SweepArgs a{};
    a.mode = mkh::kSweepPath; a.M = rf->M; a.T = T; a.W = 1; a.N = (long long)R;
    a.nodes = d_path; a.tracked = p_eff; a.node_index = p_idx; a.margin = p_em;
    sweep_edges(st, rf->ck, a);
    st.latch(hipMemcpyAsync(fw.r_nm, p_nm, 2 * R * f8, hipMemcpyDeviceToDevice, stream));     // (r's state = p's)
  }
  st.latch(hipMemcpyAsync(w.r, d_path, R * nq * f8, hipMemcpyDeviceToDevice, stream));
  st.latch(hipMemcpyAsync(w.r_trk, rf ? p_eff : d_trk, R * i4, hipMemcpyDeviceToDevice, stream));
  st.latch(hipMemsetAsync(w.r_rep, 0, R * i4, stream));
  const int32_t loop_flags = (flags & ~MKH_FLAG_WARM_START) | MKH_FLAG_DEVICE_PTRS;
  const int njnt = p->model->njnt;
  const int32_t* const jnt = p->ws[WS_JNT].i32();
  auto step = [&](int ct, int cdir, int nt, int ndir) {
    if (!rf) {
      ST_LAUNCH(st, launch_lr_step(stream, B, T, (int)nq, (int)nv, njnt, jnt, d_q, d_w, max_step_sq, ct, cdir, nt, ndir, w));
      return;
    }
    if (ct >= 0) lr_check_step(st, rf->ck, B, T, rf->M, ct, cdir, w, fw.trip);
    ST_LAUNCH(st, launch_lr_step_free(stream, B, T, (int)nq, (int)nv, njnt, jnt, d_q, d_w, max_step_sq, ct, cdir, nt, ndir, w, fw));
  };
  auto loop = [&](size_t t) -> int32_t {
    if (!st.ok()) return MKH_OK;
    SolveCall sc;
    sc.p = p; sc.B = B; sc.q = w.start; sc.frame_targets = d_ft ? d_ft + t * Bz * ft_w : nullptr;
    sc.posture_target = d_pt ? d_pt + t * pt_step : nullptr; sc.com_target = d_ct ? d_ct + t * ct_step : nullptr;
    sc.dt = ls.dt; sc.damping = ls.damping; sc.v_out = w.xv; sc.status_out = w.xst; sc.flags = loop_flags; sc.hip_stream = (void*)stream;
    sc.n_steps = ls.max_iters; sc.q_out = w.x; sc.pos_threshold = ls.pos_threshold; sc.ori_threshold = ls.ori_threshold;
    sc.iters_out = w.xit; sc.converged_out = w.xcv;
    return solve(sc);
  };
  step(-1, 1, 0, 1);
  for (int t = 0; t < T; ++t) {                              // forward; its last commit decides the first backward waypoint
    if (const int32_t rc = loop(t)) return rc;
    if (t + 1 < T) step(t, 1, t + 1, 1); else step(t, 1, T - 2, -1);       // (T = 1: T - 2 < 0, nothing follows)
  }
  for (int t = T - 2; t >= 0; --t) {                         // backward
    if (const int32_t rc = loop(t)) return rc;
    step(t, -1, t - 1, -1);
  }
  if (rf) {
    const mkh::LrFreeGuard g{p_nm, p_em, fw.r_nm, fw.r_em, rf->node_margin, rf->edge_margin, rf->edge_collision, rf->n_edge_collisions};
    ST_LAUNCH(st, launch_lr_guard_free(stream, B, T, (int)nq, (int)nv, njnt, jnt, d_q, d_w, max_step_sq, d_path, p_eff, w, out, g));
    return MKH_OK;
  }
  ST_LAUNCH(st, launch_lr_guard(stream, B, T, (int)nq, (int)nv, njnt, jnt, d_q, d_w, max_step_sq, d_path, d_trk, w, out));
  return MKH_OK;
}

// What both refining entry points refuse about the loops of the pass.
static int32_t refine_refuse(const MkhProblem* p, int32_t B, int32_t T, double max_step_sq, const LoopSpec& ls, const char* who) {
  if (B < 1) return fail(MKH_E_INVALID, "%s: B = %d must be >= 1", who, B);
  if (T < 1) return fail(MKH_E_INVALID, "%s: T = %d must be >= 1", who, T);
  if (T > 65535) return fail(MKH_E_LIMIT, "%s: T = %d waypoints, at most 65535", who, T);
  if (!(max_step_sq >= 0.0)) return fail(MKH_E_INVALID, "%s: max_step_sq = %g must be >= 0 (+inf: no gate)", who, max_step_sq);
  if ((long long)B * T > 0x7fffffffLL) return fail(MKH_E_LIMIT, "%s: B * T = %lld rows", who, (long long)B * T);
  if (const int32_t rc = loops_refuse(ls, 0, true, who, "a fixed count leaves no tracked flag to judge a repair by")) return rc;
  if (B > p->max_batch) return fail(MKH_E_INVALID, "%s: B=%d exceeds max_batch=%d of this problem (a sweep's loop launch is one chunk)", who, B, p->max_batch);
  return MKH_OK;
}

// mkh_ladder_refine (fio == NULL) and mkh_ladder_refine_free (the checker ck, n_samples and fio: the pass "with a checker").
static int32_t ladder_refine_call(MkhProblem* p, MkhProblem* ck, int32_t n_samples, const MkhLadderRefineFreeIO* fio, const char* who,
                                  int32_t B, int32_t T, const double* q, const double* q_path, const int32_t* tracked_path,
                                  const double* frame_targets, const double* posture_target, const double* com_target, double dt,
                                  double damping, int32_t max_iters, double pos_threshold, double ori_threshold,
                                  const MkhLadderRefineIO* io, int32_t flags, void* hip_stream, bool free_call) {
  const LoopSpec ls{dt, damping, max_iters, pos_threshold, ori_threshold};
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (!io) return fail(MKH_E_INVALID, "%s: io is required", who);
  if (const int32_t rc = refine_refuse(p, B, T, io->max_step_sq, ls, who)) return rc;
  if (const int32_t rc = refuse_checker(p, who)) return rc;
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;
  if (free_call) {
    if (const int32_t rc = sweep_refuse_for(p, ck, who, CheckerUse::refinement(n_samples))) return rc;
    if (n_samples < 1) return fail(MKH_E_INVALID, "%s: n_samples = %d must be >= 1", who, n_samples);
    if (!fio || !fio->edge_collision || !fio->n_edge_collisions || !fio->edge_margin)
      return fail(MKH_E_INVALID, "%s: free_io and its outputs edge_collision, n_edge_collisions, edge_margin are required", who);
  }
  if (!q_path || !tracked_path) return fail(MKH_E_INVALID, "%s: q_path and tracked_path are required", who);
  if (!io->q_path_out || !io->tracked_out || !io->repaired || !io->refined || !io->edge_break || !io->n_tracked || !io->n_breaks ||
      !io->path_length)
    return fail(MKH_E_INVALID, "%s: io's outputs q_path_out, tracked_out, repaired, refined, edge_break, n_tracked, n_breaks, "
                               "path_length are required", who);
  const DeviceProblem& P = p->dev;
  if (const int32_t rc = refuse_inputs(P, q, frame_targets, posture_target, com_target, who, "ladder refinement")) return rc;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  if (!devp)
    if (const int32_t rc = ladder_weights_refuse(io->weights, P.nv, who)) return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  Stager st{p, (hipStream_t)hip_stream, devp, free_call ? "ladder_refine_free" : "ladder_refine"};
  const size_t Bz = B, R = Bz * T, nq = P.nq, nv = P.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  const size_t ft_w = (size_t)P.n_frame * 7, pt_w = (size_t)P.n_posture * nq, ct_w = (size_t)P.n_com * 3;
  const double* const d_q = st.up(WS_IN_Q, q, Bz * nq);
  const double* const d_path = st.up(WS_IN_PATH, q_path, R * nq);
  const double* const d_ft = st.up(WS_IN_FT, frame_targets, R * ft_w);
  const double* const d_pt = pt_w ? st.up(WS_IN_PT, posture_target, pt_w * (pbat ? R : 1)) : posture_target;
  const double* const d_ct = ct_w ? st.up(WS_IN_CT, com_target, ct_w * (cbat ? R : 1)) : com_target;
  const double* const d_w = st.up(WS_IN_W, io->weights, nv);
  const int32_t* const d_trk = st.up_i32(WS_IN_TRK, tracked_path, R);
  mkh::LrOut o{io->q_path_out, io->v, io->path_length, io->tracked_out, io->repaired, io->refined, io->edge_break, io->n_tracked,
               io->n_breaks, io->status, io->iters, io->converged};
  RefineFree rf{};
  if (free_call) rf = RefineFree{ck, n_samples, fio->node_margin, fio->edge_margin, fio->edge_collision, fio->n_edge_collisions};
  if (free_call && !devp) {
    rf.edge_collision = st.i32(WS_F_OUT_I, R + Bz); rf.n_edge_collisions = rf.edge_collision ? rf.edge_collision + R : nullptr;
    rf.edge_margin = st.f64(WS_F_OUT_F, R);
    if (rf.node_margin) rf.node_margin = st.f64(WS_F_NMARGIN, R);
  }
  if (!devp) {
    o.q = st.f64(WS_OUT_Q, R * nq);
    o.path_length = st.f64(WS_OUT_LEN, Bz);
    o.tracked = st.i32(WS_OUT_REF, 2 * R + Bz); o.repaired = o.tracked + R; o.refined = o.tracked + 2 * R;
    o.edge_break = st.i32(WS_OUT_PICK, R + 2 * Bz); o.n_tracked = o.edge_break + R; o.n_breaks = o.n_tracked + Bz;
    // the optional rows: the caller's values go in, the repaired rows are replaced, everything comes back
    o.v = io->v ? st.f64(WS_OUT_V, R * nv) : nullptr;
    int32_t* const oi = st.i32(WS_OUT_I32, 3 * R);
    o.status = io->status ? oi : nullptr; o.iters = io->iters ? oi + R : nullptr; o.converged = io->converged ? oi + 2 * R : nullptr;
    if (st.ok()) {
      if (o.v) st.latch(hipMemcpyAsync(o.v, io->v, R * nv * f8, hipMemcpyHostToDevice, st.stream));
      if (o.status) st.latch(hipMemcpyAsync(o.status, io->status, R * i4, hipMemcpyHostToDevice, st.stream));
      if (o.iters) st.latch(hipMemcpyAsync(o.iters, io->iters, R * i4, hipMemcpyHostToDevice, st.stream));
      if (o.converged) st.latch(hipMemcpyAsync(o.converged, io->converged, R * i4, hipMemcpyHostToDevice, st.stream));
    }
  }
  if (!st.ok()) return st.finish();
  if (const int32_t rc = refine_pass(st, B, T, d_q, d_path, d_trk, d_ft, d_pt, d_ct, ls, d_w, io->max_step_sq, o, flags,
                                     free_call ? &rf : nullptr))
    return st.finish(rc);
  if (devp) return st.finish();
  if (free_call) {
    st.down(fio->edge_collision, rf.edge_collision, R * i4);
    st.down(fio->n_edge_collisions, rf.n_edge_collisions, Bz * i4);
    st.down(fio->edge_margin, rf.edge_margin, R * f8);
    st.down(fio->node_margin, rf.node_margin, R * f8);
  }
  st.down(io->q_path_out, o.q, R * nq * f8);
  st.down(io->tracked_out, o.tracked, R * i4);
  st.down(io->repaired, o.repaired, R * i4);
  st.down(io->refined, o.refined, Bz * i4);
  st.down(io->edge_break, o.edge_break, R * i4);
  st.down(io->n_tracked, o.n_tracked, Bz * i4);
  st.down(io->n_breaks, o.n_breaks, Bz * i4);
  st.down(io->path_length, o.path_length, Bz * f8);
  st.down(io->v, o.v, R * nv * f8);
  st.down(io->status, o.status, R * i4);
  st.down(io->iters, o.iters, R * i4);
  st.down(io->converged, o.converged, R * i4);
  return st.finish();
}

int32_t mkh_ladder_refine(MkhProblem* p, int32_t B, int32_t T, const double* q, const double* q_path, const int32_t* tracked_path,
                          const double* frame_targets, const double* posture_target, const double* com_target, double dt,
                          double damping, int32_t max_iters, double pos_threshold, double ori_threshold, const MkhLadderRefineIO* io,
                          int32_t flags, void* hip_stream) {
  return ladder_refine_call(p, nullptr, 0, nullptr, "mkh_ladder_refine", B, T, q, q_path, tracked_path, frame_targets, posture_target,
                            com_target, dt, damping, max_iters, pos_threshold, ori_threshold, io, flags, hip_stream, false);
}

int32_t mkh_ladder_refine_free(MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, const double* q, const double* q_path,
                               const int32_t* tracked_path, const double* frame_targets, const double* posture_target,
                               const double* com_target, double dt, double damping, int32_t max_iters, double pos_threshold,
                               double ori_threshold, int32_t n_samples, const MkhLadderRefineIO* io,
                               const MkhLadderRefineFreeIO* fio, int32_t flags, void* hip_stream) {
  return ladder_refine_call(p, ck, n_samples, fio, "mkh_ladder_refine_free", B, T, q, q_path, tracked_path, frame_targets,
                            posture_target, com_target, dt, damping, max_iters, pos_threshold, ori_threshold, io, flags, hip_stream,
                            true);
}

// ---- the fused ladder calls: mkh_solve_trajectory_ladder(_refined) on the loops' S nodes per rung, and
// mkh_solve_trajectory_ladder_nodes on K deduplicated ones.  They share everything but the width W of the (B·T, W, .) node
// arrays and what fills them: refuse → stage → rungs → pick → refine, qvel → copy back.
struct LadderCall {
  MsIn in;                         // the (B·T) flattened targets; in.q: q once per (instance, waypoint), their "current posture"
  const double *q, *w;             // q (B, nq); the edge cost's weights
  // the nodes, (B·T, W, .): the caller's *_all arrays where they are device buffers; the starts, (B·T, S, nq), when asked for
  double *l_q, *l_v;
  int32_t *l_st, *l_it, *l_cv, *l_trk;
  double* l_starts;
  // the device-side outputs, (B, T, .) and (B,): the caller's arrays for a device-pointer call, else carved from WS_OUT_*.  The
  // path's rows, the search's integers, and the refinement's three arrays (NULL without a pass)
  double *o_q, *o_v, *o_qvel, *o_len;
  int32_t *o_st, *o_it, *o_cv, *o_node, *o_eb, *o_nt, *o_nb, *o_trk, *o_rep, *o_ref;
};

// What both calls refuse behind their own checks of the graph's shape, in this order (`nodes`: the call on distinct nodes).
static int32_t ladder_call_refuse(const MkhProblem* p, int32_t B, int32_t T, int S, const LoopSpec& ls, int64_t target_index0,
                                  const double* q, const double* frame_targets, const double* posture_target,
                                  const double* com_target, const MkhTrajectoryLadderIO* io, const MkhLadderNodesIO* nodes,
                                  const MkhLadderRefineIO* refine, bool devp, const char* who, const MkhSeedTable** tab) {
  if (const int32_t rc = loops_refuse(ls, target_index0, true, who, "a fixed count leaves no tracked flag to search on")) return rc;
  if (const int32_t rc = refuse_checker(p, who)) return rc;
  if (!io->q_traj || !io->v_traj || !io->status || !io->iters || !io->converged || !io->node_index || !io->n_tracked ||
      !io->n_breaks || !io->path_length || !io->edge_break)
    return fail(MKH_E_INVALID, "%s: io's outputs q_traj, v_traj, status, iters, converged, node_index, n_tracked, n_breaks, path_length, "
                               "edge_break are required", who);
  if (nodes && (!nodes->node_seed_index || !nodes->node_multiplicity || !nodes->node_distance || !nodes->n_distinct ||
                !nodes->n_converged || !nodes->n_uncovered || !nodes->seed_index))
    return fail(MKH_E_INVALID, "%s: nodes' outputs node_seed_index, node_multiplicity, node_distance, n_distinct, n_converged, "
                               "n_uncovered, seed_index are required", who);
  if (io->qvel && !(io->waypoint_dt > 0.0)) return fail(MKH_E_INVALID, "qvel needs waypoint_dt > 0");
  if (refine) {
    if (const int32_t rc = refine_refuse(p, B, T, io->max_step_sq, ls, who)) return rc;
    if (!refine->tracked_out || !refine->repaired || !refine->refined)
      return fail(MKH_E_INVALID, "%s: refine's outputs tracked_out, repaired, refined are required", who);
  }
  if (const int32_t rc = refuse_inputs(p->dev, q, frame_targets, posture_target, com_target, who, "ladder")) return rc;
  if (S > p->max_batch) return fail(MKH_E_INVALID, "%s: n_seeds = %d exceeds max_batch=%d of this problem (a rung is one chunk)", who, S, p->max_batch);
  if (!devp)
    if (const int32_t rc = ladder_weights_refuse(io->weights, p->dev.nv, who)) return rc;
  return seed_table_for(p, io->seeds, S, who, tab);
}

// The inputs on the device with q fanned out to the rungs, the node arrays, and the outputs.
static LadderCall ladder_stage(Stager& st, int B, int T, int S, int W, const double* q, const double* frame_targets,
                               const double* posture_target, const double* com_target, const MkhSeedTable* tab,
                               const MkhTrajectoryLadderIO* io, const MkhLadderRefineIO* refine, int32_t flags) {
  const DeviceProblem& P = st.p->dev;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  const size_t Bz = B, R = Bz * T, N = R * S, M = R * W, nq = P.nq, nv = P.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  const size_t ft_w = (size_t)P.n_frame * 7, pt_w = (size_t)P.n_posture * nq, ct_w = (size_t)P.n_com * 3;
  LadderCall c;
  c.q = st.up(WS_IN_Q, q, Bz * nq);
  c.in.ft = st.up(WS_IN_FT, frame_targets, R * ft_w);
  c.in.pt = pt_w ? st.up(WS_IN_PT, posture_target, pt_w * (pbat ? R : 1)) : posture_target;
  c.in.ct = ct_w ? st.up(WS_IN_CT, com_target, ct_w * (cbat ? R : 1)) : com_target;
  c.w = st.up(WS_IN_W, io->weights, nv);
  c.in.user = st.up(WS_IN_SEEDS, io->seeds, N * nq);
  c.in.tab = tab;
  double* const d_q0 = st.f64(WS_L_Q0, R * nq);
  ST_LAUNCH(st, launch_ms_fanout(st.stream, c.q, d_q0, B, T, (int)nq));
  c.in.q = d_q0;
  c.l_q = (double*)st.given_or(WS_L_Q, io->q_all, M * nq * f8);
  c.l_v = (double*)st.given_or(WS_L_V, io->v_all, M * nv * f8);
  c.l_st = (int32_t*)st.given_or(WS_L_ST, io->status_all, M * i4);
  c.l_it = (int32_t*)st.given_or(WS_L_IT, io->iters_all, M * i4);
  c.l_cv = (int32_t*)st.given_or(WS_L_CV, io->converged_all, M * i4);
  c.l_trk = st.i32(WS_L_TRK, M);
  c.l_starts = io->seeds_out ? (double*)st.given_or(WS_L_STARTS, io->seeds_out, N * nq * f8) : nullptr;
  c.o_q = io->q_traj; c.o_v = io->v_traj; c.o_qvel = io->qvel; c.o_len = io->path_length;
  c.o_st = io->status; c.o_it = io->iters; c.o_cv = io->converged;
  c.o_node = io->node_index; c.o_eb = io->edge_break; c.o_nt = io->n_tracked; c.o_nb = io->n_breaks;
  c.o_trk = refine ? refine->tracked_out : nullptr; c.o_rep = refine ? refine->repaired : nullptr; c.o_ref = refine ? refine->refined : nullptr;
  if (!st.devp) {
    c.o_q = st.f64(WS_OUT_Q, R * nq); c.o_v = st.f64(WS_OUT_V, R * nv);
    c.o_qvel = io->qvel ? st.f64(WS_OUT_QVEL, R * nv) : nullptr;
    c.o_st = st.i32(WS_OUT_I32, 3 * R); c.o_it = c.o_st + R; c.o_cv = c.o_st + 2 * R;
    c.o_node = st.i32(WS_OUT_PICK, 2 * R + 2 * Bz); c.o_eb = c.o_node + R; c.o_nt = c.o_node + 2 * R; c.o_nb = c.o_nt + Bz;
    c.o_len = st.f64(WS_OUT_LEN, Bz);
    if (refine) { c.o_trk = st.i32(WS_OUT_REF, 2 * R + Bz); c.o_rep = c.o_trk + R; c.o_ref = c.o_trk + 2 * R; }
  }
  return c;
}

// A checked call's part of a ladder call (ck == NULL: a plain one): the checker, how it judges an edge, and the outputs.
struct LadderFree {
  MkhProblem* ck = nullptr;
  EdgeRule rule{};
  const MkhLadderFreeIO* io = nullptr;
  const MkhLadderCertifiedIO* cio = nullptr;       // the certified rule's outputs, else NULL
  LadderFreeOut o{};               // device arrays (ladder_free_stage)
};

// The device side of a checked call's outputs: the caller's arrays for a device-pointer call, else workspace.
static void ladder_free_stage(Stager& st, int B, int T, int W, LadderFree& lf) {
  if (lf.ck) lf.o = ladder_free_out(st, B, T, W, lf.rule, lf.io, lf.cio);
}

static void ladder_free_down(Stager& st, int B, int T, int W, const LadderFree& lf) {
  if (lf.ck) ladder_free_out_down(st, B, T, W, lf.o, lf.io, lf.cio);
}

// The search on the (B, T, W) nodes — behind the sweep of their edges in a checked call —, and the chosen nodes' rows.
static void ladder_pick(Stager& st, int B, int T, int W, const LadderCall& c, double max_step_sq, const LadderFree& lf) {
  const long long R = (long long)B * T;
  const int nq = st.p->dev.nq, nv = st.p->dev.nv;
  if (lf.ck)
    ladder_search_free(st, lf.ck, B, T, W, lf.rule, c.q, c.l_q, c.l_trk, c.w, max_step_sq, c.o_node, c.o_nt, c.o_nb, c.o_len, c.o_eb, lf.o);
  else
    ladder_search(st, B, T, W, c.q, c.l_q, c.l_trk, c.w, max_step_sq, c.o_node, c.o_nt, c.o_nb, c.o_len, c.o_eb);
  ST_LAUNCH(st, launch_ladder_gather(st.stream, c.l_q, c.o_q, c.o_node, R, W, nq));
  ST_LAUNCH(st, launch_ladder_gather(st.stream, c.l_v, c.o_v, c.o_node, R, W, nv));
  ST_LAUNCH(st, launch_ladder_gather_i32(st.stream, c.l_st, c.o_st, c.o_node, R, W));
  ST_LAUNCH(st, launch_ladder_gather_i32(st.stream, c.l_it, c.o_it, c.o_node, R, W));
  ST_LAUNCH(st, launch_ladder_gather_i32(st.stream, c.l_cv, c.o_cv, c.o_node, R, W));
}

// The optional pass over the chosen path, and the waypoint velocities.  The chosen nodes' flags are the path's; the pass reads
// path and flags in place and writes the returned ones over them.  Returns as refine_pass does.
static int32_t ladder_refine_qvel(Stager& st, int B, int T, int W, const LadderCall& c, const LoopSpec& ls,
                                  const MkhTrajectoryLadderIO* io, bool refine, int32_t flags, const LadderFree& lf) {
  const MkhProblem* const p = st.p;
  const int nq = p->dev.nq, nv = p->dev.nv;
  if (refine) {
    ST_LAUNCH(st, launch_ladder_gather_i32(st.stream, c.l_trk, c.o_trk, c.o_node, (long long)B * T, W));
    const mkh::LrOut o{c.o_q, c.o_v, c.o_len, c.o_trk, c.o_rep, c.o_ref, c.o_eb, c.o_nt, c.o_nb, c.o_st, c.o_it, c.o_cv};
    // (a checked call: the pass "with a checker"; the returned path's edge outputs replace the search's)
    const RefineFree rf{lf.ck, lf.rule.M, nullptr, lf.o.edge_margin, lf.o.edge_collision, lf.o.n_edge_collisions};
    if (const int32_t rc = refine_pass(st, B, T, c.q, c.o_q, c.o_trk, c.in.ft, c.in.pt, c.in.ct, ls, c.w, io->max_step_sq, o, flags,
                                       lf.ck ? &rf : nullptr))
      return rc;
  }
  if (c.o_qvel)
    ST_LAUNCH(st, launch_tj_qvel(st.stream, p->ws[WS_JNT].i32(), p->model->njnt, B, T, nq, c.q, c.o_q, (long long)T * nq, (long long)nq,
                                 io->waypoint_dt, c.o_qvel, (long long)T * nv, (long long)nv, 0));
  return MKH_OK;
}

// A host caller's results: io's, then (through `between`) what the entry point adds, then the pass's.
static void ladder_down(Stager& st, int B, int T, int S, int W, const LadderCall& c, const MkhTrajectoryLadderIO* io,
                        const MkhLadderRefineIO* refine, const std::function<void()>& between = nullptr) {
  const size_t Bz = B, R = Bz * T, N = R * S, M = R * W, nq = st.p->dev.nq, nv = st.p->dev.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  st.down(io->q_traj, c.o_q, R * nq * f8);
  st.down(io->v_traj, c.o_v, R * nv * f8);
  st.down(io->status, c.o_st, R * i4);
  st.down(io->iters, c.o_it, R * i4);
  st.down(io->converged, c.o_cv, R * i4);
  st.down(io->node_index, c.o_node, R * i4);
  st.down(io->edge_break, c.o_eb, R * i4);
  st.down(io->n_tracked, c.o_nt, Bz * i4);
  st.down(io->n_breaks, c.o_nb, Bz * i4);
  st.down(io->path_length, c.o_len, Bz * f8);
  st.down(io->qvel, c.o_qvel, R * nv * f8);
  st.down(io->q_all, c.l_q, M * nq * f8);
  st.down(io->v_all, c.l_v, M * nv * f8);
  st.down(io->status_all, c.l_st, M * i4);
  st.down(io->iters_all, c.l_it, M * i4);
  st.down(io->converged_all, c.l_cv, M * i4);
  st.down(io->seeds_out, c.l_starts, N * nq * f8);
  if (between) between();
  if (refine) {
    st.down(refine->tracked_out, c.o_trk, R * i4);
    st.down(refine->repaired, c.o_rep, R * i4);
    st.down(refine->refined, c.o_ref, Bz * i4);
  }
}

int32_t mkh_solve_trajectory_ladder(MkhProblem* p, int32_t B, int32_t T, int32_t n_seeds, const double* q,
                                    const double* frame_targets, const double* posture_target, const double* com_target, double dt,
                                    double damping, int32_t max_iters, double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                    int64_t target_index0, const MkhTrajectoryLadderIO* io, int32_t flags, void* hip_stream) {
  return mkh_solve_trajectory_ladder_refined(p, B, T, n_seeds, q, frame_targets, posture_target, com_target, dt, damping, max_iters,
                                             pos_threshold, ori_threshold, rng_seed, target_index0, io, nullptr, flags, hip_stream);
}

// The plain ladder call and its checked twin (lf.ck given: mkh_solve_trajectory_ladder_free without n_nodes, which has refused
// the checker and a refinement already).
static int32_t ladder_plain_call(MkhProblem* p, LadderFree lf, const char* who, int32_t B, int32_t T, int32_t n_seeds, const double* q,
                                 const double* frame_targets, const double* posture_target, const double* com_target, double dt,
                                 double damping, int32_t max_iters, double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                 int64_t target_index0, const MkhTrajectoryLadderIO* io, const MkhLadderRefineIO* refine, int32_t flags,
                                 void* hip_stream);

int32_t mkh_solve_trajectory_ladder_refined(MkhProblem* p, int32_t B, int32_t T, int32_t n_seeds, const double* q,
                                            const double* frame_targets, const double* posture_target, const double* com_target,
                                            double dt, double damping, int32_t max_iters, double pos_threshold, double ori_threshold,
                                            uint64_t rng_seed, int64_t target_index0, const MkhTrajectoryLadderIO* io,
                                            const MkhLadderRefineIO* refine, int32_t flags, void* hip_stream) {
  return ladder_plain_call(p, LadderFree{}, refine ? "mkh_solve_trajectory_ladder_refined" : "mkh_solve_trajectory_ladder", B, T, n_seeds,
                           q, frame_targets, posture_target, com_target, dt, damping, max_iters, pos_threshold, ori_threshold, rng_seed,
                           target_index0, io, refine, flags, hip_stream);
}

static int32_t ladder_plain_call(MkhProblem* p, LadderFree lf, const char* who, int32_t B, int32_t T, int32_t n_seeds, const double* q,
                                 const double* frame_targets, const double* posture_target, const double* com_target, double dt,
                                 double damping, int32_t max_iters, double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                 int64_t target_index0, const MkhTrajectoryLadderIO* io, const MkhLadderRefineIO* refine, int32_t flags,
                                 void* hip_stream) {
  const LoopSpec ls{dt, damping, max_iters, pos_threshold, ori_threshold};
  const int S = n_seeds;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (!io) return fail(MKH_E_INVALID, "%s: io is required", who);
  if (const int32_t rc = ladder_refuse(p, B, T, S, io->max_step_sq, who)) return rc;
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;
  const MkhSeedTable* tab;
  if (const int32_t rc = ladder_call_refuse(p, B, T, S, ls, target_index0, q, frame_targets, posture_target, com_target, io, nullptr,
                                            refine, devp, who, &tab))
    return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  Stager st{p, (hipStream_t)hip_stream, devp, "trajectory_ladder"};
  const size_t R = (size_t)B * T, per = (size_t)p->max_batch / S, nq = p->dev.nq, nv = p->dev.nv;
  const LadderCall c = ladder_stage(st, B, T, S, S, q, frame_targets, posture_target, com_target, tab, io, refine, flags);
  ladder_free_stage(st, B, T, S, lf);
  // (without the caller's seeds_out the starts of one chunk go through multi-start's candidate slot; the loops write the nodes)
  double* const c_q = c.l_starts ? nullptr : st.f64(WS_C_Q, (per < R ? per : R) * S * nq);
  if (!st.ok()) return st.finish();
  // ---- the rungs: multi-start on the (B·T) flattened targets, straight into the node arrays
  auto rows_at = [&](size_t r0) {
    const size_t i0 = r0 * S;
    return MsRows{c.l_starts ? c.l_starts + i0 * nq : c_q, c.l_q + i0 * nq, c.l_v + i0 * nv, c.l_st + i0, c.l_it + i0, c.l_cv + i0,
                  nullptr};
  };
  if (const int32_t rc = ms_rungs(st, R, S, c.in, ls, rng_seed, target_index0 * T, flags, rows_at)) return st.finish(rc);
  // (a checked call: MKH_ST_IN_COLLISION into the nodes' status rows, so that a colliding node is not tracked)
  if (lf.ck) clearance_rows(st, lf.ck, R * S, c.l_q, nullptr, nullptr, nullptr, nullptr, c.l_st);
  ST_LAUNCH(st, launch_ladder_tracked(st.stream, c.l_cv, c.l_st, (long long)(R * S), c.l_trk));
  ladder_pick(st, B, T, S, c, io->max_step_sq, lf);
  if (const int32_t rc = ladder_refine_qvel(st, B, T, S, c, ls, io, refine != nullptr, flags, lf)) return st.finish(rc);
  if (!devp) ladder_down(st, B, T, S, S, c, io, refine, [&] { ladder_free_down(st, B, T, S, lf); });
  return st.finish();
}

// The ladder on deduplicated nodes (include/minkhip.h mkh_solve_trajectory_ladder_nodes; kernels: unwind.hip, solution_set.hip,
// ladder_nodes.hip, ladder.hip): the loops write the candidate buffers of ONE chunk of rungs, which this call requests itself;
// behind every chunk's loops its unwinding, the distinct-set selection into the chunk's K slots per rung of the node arrays, and
// the slots' flags.  Everything behind the rungs is the plain ladder's with K for S.
static int32_t ladder_nodes_call(MkhProblem* p, LadderFree lf, const char* who, int32_t B, int32_t T, int32_t n_seeds, int32_t n_nodes,
                                 double min_distance, const double* q, const double* frame_targets, const double* posture_target,
                                 const double* com_target, double dt, double damping, int32_t max_iters, double pos_threshold,
                                 double ori_threshold, uint64_t rng_seed, int64_t target_index0, const MkhTrajectoryLadderIO* io,
                                 const MkhLadderNodesIO* nodes, const MkhLadderRefineIO* refine, int32_t flags, void* hip_stream);

int32_t mkh_solve_trajectory_ladder_nodes(MkhProblem* p, int32_t B, int32_t T, int32_t n_seeds, int32_t n_nodes, double min_distance,
                                          const double* q, const double* frame_targets, const double* posture_target,
                                          const double* com_target, double dt, double damping, int32_t max_iters, double pos_threshold,
                                          double ori_threshold, uint64_t rng_seed, int64_t target_index0,
                                          const MkhTrajectoryLadderIO* io, const MkhLadderNodesIO* nodes, const MkhLadderRefineIO* refine,
                                          int32_t flags, void* hip_stream) {
  return ladder_nodes_call(p, LadderFree{}, "mkh_solve_trajectory_ladder_nodes", B, T, n_seeds, n_nodes, min_distance, q, frame_targets,
                           posture_target, com_target, dt, damping, max_iters, pos_threshold, ori_threshold, rng_seed, target_index0, io,
                           nodes, refine, flags, hip_stream);
}

// ... and its checked twin (lf.ck given: mkh_solve_trajectory_ladder_free with n_nodes).
static int32_t ladder_nodes_call(MkhProblem* p, LadderFree lf, const char* who, int32_t B, int32_t T, int32_t n_seeds, int32_t n_nodes,
                                 double min_distance, const double* q, const double* frame_targets, const double* posture_target,
                                 const double* com_target, double dt, double damping, int32_t max_iters, double pos_threshold,
                                 double ori_threshold, uint64_t rng_seed, int64_t target_index0, const MkhTrajectoryLadderIO* io,
                                 const MkhLadderNodesIO* nodes, const MkhLadderRefineIO* refine, int32_t flags, void* hip_stream) {
  const LoopSpec ls{dt, damping, max_iters, pos_threshold, ori_threshold};
  const int S = n_seeds, K = n_nodes;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (!io || !nodes) return fail(MKH_E_INVALID, "%s: io and nodes are required", who);
  if (S < 1) return fail(MKH_E_INVALID, "%s: n_seeds = %d must be >= 1", who, S);
  if (S > mkh::kSsMaxCandidates)
    return fail(MKH_E_LIMIT, "%s: n_seeds = %d candidates per rung, at most %d (their selection state lives in LDS)", who, S,
                mkh::kSsMaxCandidates);
  if (const int32_t rc = set_refuse(K, min_distance, who)) return rc;
  if (const int32_t rc = ladder_refuse(p, B, T, K, io->max_step_sq, who)) return rc;       // (the search runs on K nodes per rung)
  if ((long long)B * T * K > 0x7fffffffLL) return fail(MKH_E_LIMIT, "%s: B * T * n_nodes = %lld nodes", who, (long long)B * T * K);
  const MkhSeedTable* tab;
  if (const int32_t rc = ladder_call_refuse(p, B, T, S, ls, target_index0, q, frame_targets, posture_target, com_target, io, nodes,
                                            refine, devp, who, &tab))
    return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  const bool unwind = (flags & MKH_FLAG_UNWIND_TURNS) != 0;
  flags &= ~MKH_FLAG_UNWIND_TURNS;                           // (the loops and the pass below know nothing of it)
  Stager st{p, (hipStream_t)hip_stream, devp, "trajectory_ladder_nodes"};
  const size_t R = (size_t)B * T, M = R * K, nq = p->dev.nq, nv = p->dev.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  const size_t per = (size_t)p->max_batch / S, chunk = (per < R ? per : R) * S;      // rungs, and loops, of one chunk
  const LadderCall c = ladder_stage(st, B, T, S, K, q, frame_targets, posture_target, com_target, tab, io, refine, flags);
  ladder_free_stage(st, B, T, K, lf);
  // ---- the candidates of one chunk, in multi-start's slots: the loops run in place in c_q
  double *const c_q = st.f64(WS_C_Q, chunk * nq), *const c_v = st.f64(WS_C_V, chunk * nv);
  int32_t *const c_st = st.i32(WS_C_ST, chunk), *const c_it = st.i32(WS_C_IT, chunk), *const c_cv = st.i32(WS_C_CV, chunk);
  // ---- the set's outputs per slot and per rung
  int32_t *n_si = nodes->node_seed_index, *n_mu = nodes->node_multiplicity, *n_nd = nodes->n_distinct, *n_nc = nodes->n_converged,
          *n_nu = nodes->n_uncovered, *n_pick = nodes->seed_index;
  double* n_dist = nodes->node_distance;
  if (!devp) {
    n_si = st.i32(WS_N_I32, 2 * M + 4 * R); n_mu = n_si + M; n_nd = n_si + 2 * M; n_nc = n_nd + R; n_nu = n_nd + 2 * R; n_pick = n_nd + 3 * R;
    n_dist = st.f64(WS_N_DIST, M);
  }
  if (!st.ok()) return st.finish();
  // ---- the rungs: multi-start on the (B·T) flattened targets, then the chunk's nodes
  auto rows_at = [&](size_t r0) {
    return MsRows{c.l_starts ? c.l_starts + r0 * S * nq : c_q, c_q, c_v, c_st, c_it, c_cv, nullptr};
  };
  auto select = [&](size_t r0, size_t n) {
    const size_t m0 = r0 * K;
    const double* const ref = c.in.q + r0 * nq;
    if (unwind)
      ST_LAUNCH(st, launch_unwind_turns(st.stream, p->ws[WS_UNW].f64(), (long long)(n * S), S, (int)nq, c_q, ref, c_q));
    // (a checked call: MKH_ST_IN_COLLISION into the chunk's candidate rows, so that a colliding candidate takes no slot)
    if (lf.ck) clearance_rows(st, lf.ck, n * S, c_q, nullptr, nullptr, nullptr, nullptr, c_st);
    const mkh::SsOut so{c.l_q + m0 * nq, c.l_v + m0 * nv, c.l_it + m0, c.l_st + m0, n_si + m0, n_mu + m0, n_dist + m0,
                        n_nd + r0, n_nc + r0, n_nu + r0};
    ST_LAUNCH(st, launch_ss_select(st.stream, (int)n, S, K, (int)nq, (int)nv, p->model->njnt, p->ws[WS_JNT].i32(), c_q, c_v, c_st, c_it,
                                   c_cv, ref, c.w, min_distance * min_distance, so));
    ST_LAUNCH(st, launch_ladder_nodes_flags(st.stream, (long long)n, S, K, c_cv, n_si + m0, c.l_trk + m0, c.l_cv + m0));
  };
  if (const int32_t rc = ms_rungs(st, R, S, c.in, ls, rng_seed, target_index0 * T, flags, rows_at, select)) return st.finish(rc);
  ladder_pick(st, B, T, K, c, io->max_step_sq, lf);
  ST_LAUNCH(st, launch_ladder_gather_i32(st.stream, n_si, n_pick, c.o_node, (long long)R, K));
  if (const int32_t rc = ladder_refine_qvel(st, B, T, K, c, ls, io, refine != nullptr, flags, lf)) return st.finish(rc);
  if (!devp)
    ladder_down(st, B, T, S, K, c, io, refine, [&] {
      st.down(nodes->node_seed_index, n_si, M * i4);
      st.down(nodes->node_multiplicity, n_mu, M * i4);
      st.down(nodes->node_distance, n_dist, M * f8);
      st.down(nodes->n_distinct, n_nd, R * i4);
      st.down(nodes->n_converged, n_nc, R * i4);
      st.down(nodes->n_uncovered, n_nu, R * i4);
      st.down(nodes->seed_index, n_pick, R * i4);
      ladder_free_down(st, B, T, K, lf);
    });
  return st.finish();
}

// mkh_solve_trajectory_ladder_free (refine refused), mkh_solve_trajectory_ladder_free_refined (refine required) and
// mkh_solve_trajectory_ladder_certified (rule.certified with cio; refine refused).
static int32_t ladder_free_call(const char* who, bool refined, MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, int32_t n_seeds,
                                int32_t n_nodes, double min_distance, const double* q, const double* frame_targets,
                                const double* posture_target, const double* com_target, double dt, double damping, int32_t max_iters,
                                double pos_threshold, double ori_threshold, uint64_t rng_seed, int64_t target_index0, const EdgeRule& rule,
                                const MkhTrajectoryLadderIO* io, const MkhLadderNodesIO* nodes, const MkhLadderRefineIO* refine,
                                const MkhLadderFreeIO* fio, const MkhLadderCertifiedIO* cio, int32_t flags, void* hip_stream) {
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (rule.certified && refine)
    return fail(MKH_E_INVALID, "%s: the refinement pass still samples its edges (certifying it is the follow-up): refine must be NULL", who);
  if (!refined && refine)
    return fail(MKH_E_INVALID, "%s: the refinement pass knows nothing of collisions: refine must be NULL", who);
  if (refined && !refine)
    return fail(MKH_E_INVALID, "%s: refine is required (without it the call is mkh_solve_trajectory_ladder_free)", who);
  if (n_nodes < 0 || (n_nodes == 0) != (nodes == nullptr))
    return fail(MKH_E_INVALID, "%s: n_nodes = %d with nodes %s: n_nodes = 0 and nodes = NULL is the plain ladder, n_nodes >= 1 with nodes "
                               "the ladder on distinct nodes", who, n_nodes, nodes ? "given" : "NULL");
  const int W = n_nodes ? n_nodes : n_seeds;
  if (B < 1 || T < 1 || W < 1 || W > 256) return fail(MKH_E_INVALID, "%s: B = %d, T = %d and %d nodes per rung: B, T >= 1, 1 <= nodes <= 256", who, B, T, W);
  if (const int32_t rc = ladder_free_refuse(p, ck, B, T, W, rule, fio, cio, who, refined)) return rc;
  if (fio->node_margin)
    return fail(MKH_E_INVALID, "%s: node_margin is mkh_ladder_select_free's output: here the nodes' verdict is MKH_ST_IN_COLLISION in status_all", who);
  if (mkh::ladder_source_tile(W, p->dev.nq, p->dev.nv, p->model->njnt, nullptr, true) < 1)
    return fail(MKH_E_LIMIT, "%s: nq = %d: one destination tile and one source node with its flags do not fit 64 KB of LDS", who, p->dev.nq);
  LadderFree lf;
  lf.ck = ck; lf.rule = rule; lf.io = fio; lf.cio = cio;
  if (!n_nodes)
    return ladder_plain_call(p, lf, who, B, T, n_seeds, q, frame_targets, posture_target, com_target, dt, damping, max_iters, pos_threshold,
                             ori_threshold, rng_seed, target_index0, io, refine, flags, hip_stream);
  return ladder_nodes_call(p, lf, who, B, T, n_seeds, n_nodes, min_distance, q, frame_targets, posture_target, com_target, dt, damping,
                           max_iters, pos_threshold, ori_threshold, rng_seed, target_index0, io, nodes, refine, flags, hip_stream);
}

int32_t mkh_solve_trajectory_ladder_free(MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, int32_t n_seeds, int32_t n_nodes,
                                         double min_distance, const double* q, const double* frame_targets, const double* posture_target,
                                         const double* com_target, double dt, double damping, int32_t max_iters, double pos_threshold,
                                         double ori_threshold, uint64_t rng_seed, int64_t target_index0, int32_t n_samples,
                                         const MkhTrajectoryLadderIO* io, const MkhLadderNodesIO* nodes, const MkhLadderRefineIO* refine,
                                         const MkhLadderFreeIO* fio, int32_t flags, void* hip_stream) {
  EdgeRule rule;
  rule.M = n_samples;
  return ladder_free_call("mkh_solve_trajectory_ladder_free", false, p, ck, B, T, n_seeds, n_nodes, min_distance, q, frame_targets,
                          posture_target, com_target, dt, damping, max_iters, pos_threshold, ori_threshold, rng_seed, target_index0,
                          rule, io, nodes, refine, fio, nullptr, flags, hip_stream);
}

int32_t mkh_solve_trajectory_ladder_certified(MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, int32_t n_seeds, int32_t n_nodes,
                                              double min_distance, const double* q, const double* frame_targets,
                                              const double* posture_target, const double* com_target, double dt, double damping,
                                              int32_t max_iters, double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                              int64_t target_index0, double resolution, int32_t max_samples, int32_t edge_policy,
                                              const MkhTrajectoryLadderIO* io, const MkhLadderNodesIO* nodes,
                                              const MkhLadderRefineIO* refine, const MkhLadderFreeIO* fio,
                                              const MkhLadderCertifiedIO* cio, int32_t flags, void* hip_stream) {
  EdgeRule rule;
  rule.certified = true; rule.resolution = resolution; rule.max_samples = max_samples; rule.policy = edge_policy;
  return ladder_free_call("mkh_solve_trajectory_ladder_certified", false, p, ck, B, T, n_seeds, n_nodes, min_distance, q, frame_targets,
                          posture_target, com_target, dt, damping, max_iters, pos_threshold, ori_threshold, rng_seed, target_index0,
                          rule, io, nodes, refine, fio, cio, flags, hip_stream);
}

int32_t mkh_solve_trajectory_ladder_free_refined(MkhProblem* p, MkhProblem* ck, int32_t B, int32_t T, int32_t n_seeds, int32_t n_nodes,
                                                 double min_distance, const double* q, const double* frame_targets,
                                                 const double* posture_target, const double* com_target, double dt, double damping,
                                                 int32_t max_iters, double pos_threshold, double ori_threshold, uint64_t rng_seed,
                                                 int64_t target_index0, int32_t n_samples, const MkhTrajectoryLadderIO* io,
                                                 const MkhLadderNodesIO* nodes, const MkhLadderRefineIO* refine,
                                                 const MkhLadderFreeIO* fio, int32_t flags, void* hip_stream) {
  EdgeRule rule;
  rule.M = n_samples;
  return ladder_free_call("mkh_solve_trajectory_ladder_free_refined", true, p, ck, B, T, n_seeds, n_nodes, min_distance, q,
                          frame_targets, posture_target, com_target, dt, damping, max_iters, pos_threshold, ori_threshold, rng_seed,
                          target_index0, rule, io, nodes, refine, fio, nullptr, flags, hip_stream);
}

// ---- goal sets (include/minkhip.h "THE RULE OF THE GOAL SET"; kernel: goalset.hip)
// What both entry points refuse about the shape, the outputs and a host caller's costs.
static int32_t goalset_refuse(int32_t B, int32_t G, int32_t S, const MkhGoalSetIO* io, bool loops, bool devp, const char* who) {
  if (B < 1) return fail(MKH_E_INVALID, "%s: B = %d must be >= 1", who, B);
  if (G < 1) return fail(MKH_E_INVALID, "%s: n_goals = %d must be >= 1", who, G);
  if (S < 1) return fail(MKH_E_INVALID, "%s: n_seeds = %d must be >= 1", who, S);
  if (!io || !io->q_best || !io->converged || !io->goal_index || !io->seed_index || !io->n_reached || !io->score || !io->q_goal ||
      !io->seed_index_goal || !io->reached || !io->n_converged_goal || !io->distance_goal)
    return fail(MKH_E_INVALID, "%s: io and its outputs q_best, converged, goal_index, seed_index, n_reached, score, q_goal, "
                               "seed_index_goal, reached, n_converged_goal, distance_goal are required", who);
  if (loops && (!io->v_best || !io->iters || !io->status || !io->v_goal || !io->iters_goal || !io->status_goal))
    return fail(MKH_E_INVALID, "%s: io's outputs v_best, iters, status, v_goal, iters_goal, status_goal are required", who);
  if ((long long)B * G * S > 0x7fffffffLL) return fail(MKH_E_LIMIT, "%s: B * n_goals * n_seeds = %lld rows", who, (long long)B * G * S);
  if (!devp && io->goal_cost)
    for (size_t r = 0, R = (size_t)B * G; r < R; ++r)
      if (!(io->goal_cost[r] >= 0.0) || io->goal_cost[r] > 1.7976931348623157e308)
        return fail(MKH_E_INVALID, "%s: goal_cost[%zu] = %g must be finite and >= 0", who, r, io->goal_cost[r]);
  return MKH_OK;
}

// The two levels on device arrays into io's outputs: in place for a device-pointer call, else through the workspace and down.
// v / status / iters may be absent (a selection over a caller's own candidates: conv is then its `valid`, or absent too).
static void goalset_select(Stager& st, int B, int G, int S, const MkhGoalSetIO& io, const double* d_q_all, const double* d_v_all,
                           const int32_t* d_status, const int32_t* d_iters, const int32_t* d_conv, const double* d_ref,
                           const double* d_w) {
  const MkhProblem* const p = st.p;
  const size_t Bz = B, R = Bz * G, nq = p->dev.nq, nv = p->dev.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  const bool loops = d_v_all != nullptr;
  const double* const d_cost = st.up(WS_IN_GCOST, io.goal_cost, R);
  const int32_t* const d_gvalid = st.up_i32(WS_IN_GVALID, io.goal_valid, R);
  mkh::GsOut o{io.q_best, loops ? io.v_best : nullptr, loops ? io.iters : nullptr, loops ? io.status : nullptr, io.converged,
               io.goal_index, io.seed_index, io.n_reached, io.score, io.q_goal, loops ? io.v_goal : nullptr,
               loops ? io.iters_goal : nullptr, loops ? io.status_goal : nullptr, io.seed_index_goal, io.reached,
               io.n_converged_goal, io.distance_goal};
  if (!st.devp) {
    double* const oq = st.f64(WS_OUT_Q, (Bz + R) * nq);
    double* const ov = loops ? st.f64(WS_OUT_V, (Bz + R) * nv) : nullptr;
    int32_t* const rows = loops ? st.i32(WS_OUT_I32, 2 * (Bz + R)) : nullptr;
    int32_t* const pick = st.i32(WS_OUT_PICK, 4 * Bz + 3 * R);
    double* const len = st.f64(WS_OUT_LEN, Bz + R);
    if (!st.ok()) return;
    o.q_best = oq; o.q_goal = oq + Bz * nq;
    if (loops) {
      o.v_best = ov; o.v_goal = ov + Bz * nv;
      o.iters = rows; o.status = rows + Bz; o.iters_goal = rows + 2 * Bz; o.status_goal = rows + 2 * Bz + R;
    }
    o.converged = pick; o.goal_index = pick + Bz; o.seed_index = pick + 2 * Bz; o.n_reached = pick + 3 * Bz;
    o.seed_index_goal = pick + 4 * Bz; o.reached = pick + 4 * Bz + R; o.n_converged_goal = pick + 4 * Bz + 2 * R;
    o.score = len; o.distance_goal = len + Bz;
  }
  const mkh::GsIn in{d_q_all, d_v_all, d_status, d_iters, d_conv, d_ref, d_w, d_cost, d_gvalid};
  ST_LAUNCH(st, launch_gs_select(st.stream, B, G, S, (int)nq, (int)nv, p->model->njnt, p->ws[WS_JNT].i32(), in, o));
  if (st.devp) return;
  st.down(io.q_best, o.q_best, Bz * nq * f8);
  st.down(io.q_goal, o.q_goal, R * nq * f8);
  if (loops) {
    st.down(io.v_best, o.v_best, Bz * nv * f8);
    st.down(io.v_goal, o.v_goal, R * nv * f8);
    st.down(io.iters, o.iters, Bz * i4);
    st.down(io.status, o.status, Bz * i4);
    st.down(io.iters_goal, o.iters_goal, R * i4);
    st.down(io.status_goal, o.status_goal, R * i4);
  }
  st.down(io.converged, o.converged, Bz * i4);
  st.down(io.goal_index, o.goal_index, Bz * i4);
  st.down(io.seed_index, o.seed_index, Bz * i4);
  st.down(io.n_reached, o.n_reached, Bz * i4);
  st.down(io.seed_index_goal, o.seed_index_goal, R * i4);
  st.down(io.reached, o.reached, R * i4);
  st.down(io.n_converged_goal, o.n_converged_goal, R * i4);
  st.down(io.score, o.score, Bz * f8);
  st.down(io.distance_goal, o.distance_goal, R * f8);
}

int32_t mkh_solve_goalset(MkhProblem* p, int32_t B, int32_t n_goals, const double* q, const double* frame_targets,
                          const double* posture_target, const double* com_target, double dt, double damping, int32_t max_iters,
                          double pos_threshold, double ori_threshold, int32_t n_seeds, uint64_t rng_seed, int64_t target_index0,
                          const MkhGoalSetIO* io, int32_t flags, void* hip_stream) {
  const char* const who = "mkh_solve_goalset";
  const LoopSpec ls{dt, damping, max_iters, pos_threshold, ori_threshold};
  if (!p) return fail(MKH_E_INVALID, "null problem");
  const int G = n_goals, S = n_seeds;
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  if (const int32_t rc = goalset_refuse(B, G, S, io, true, devp, who)) return rc;
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;
  if (const int32_t rc = loops_refuse(ls, target_index0, false)) return rc;
  const DeviceProblem& P = p->dev;
  if (const int32_t rc = refuse_inputs(P, q, frame_targets, posture_target, com_target, who, "goal set")) return rc;
  if (S > p->max_batch)
    return fail(MKH_E_INVALID, "%s: n_seeds = %d exceeds max_batch=%d of this problem (a goal is one chunk)", who, S, p->max_batch);
  const MkhSeedTable* tab;
  if (const int32_t rc = seed_table_for(p, io->seeds, S, who, &tab)) return rc;
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  Stager st{p, (hipStream_t)hip_stream, devp, "goalset"};
  const size_t Bz = B, R = Bz * G, N = R * S, nq = P.nq, nv = P.nv, f8 = sizeof(double), i4 = sizeof(int32_t);
  const size_t ft_w = (size_t)P.n_frame * 7, pt_w = (size_t)P.n_posture * nq, ct_w = (size_t)P.n_com * 3;
  const size_t per = (size_t)p->max_batch / S;
  // ---- inputs on the device; q once per (target, goal): the flattened pairs' "current posture"
  MsIn in;
  const double* const d_q = st.up(WS_IN_Q, q, Bz * nq);
  in.ft = st.up(WS_IN_FT, frame_targets, R * ft_w);
  in.pt = pt_w ? st.up(WS_IN_PT, posture_target, pt_w * (pbat ? R : 1)) : posture_target;
  in.ct = ct_w ? st.up(WS_IN_CT, com_target, ct_w * (cbat ? R : 1)) : com_target;
  const double* const d_ref = st.up(WS_IN_REF, io->q_ref, Bz * nq);
  const double* const d_w = st.up(WS_IN_W, io->weights, nv);
  in.user = st.up(WS_IN_SEEDS, io->seeds, N * nq);
  in.tab = tab;
  double* const d_q0 = st.f64(WS_L_Q0, R * nq);
  ST_LAUNCH(st, launch_ms_fanout(st.stream, d_q, d_q0, B, G, (int)nq));
  in.q = d_q0;
  // ---- the candidates' rows, in the ladder's node slots: the caller's *_all arrays where they are device buffers (without the
  // caller's seeds_out the starts of one chunk go through multi-start's candidate slot)
  double* const l_q = (double*)st.given_or(WS_L_Q, io->q_all, N * nq * f8);
  double* const l_v = st.f64(WS_L_V, N * nv);
  int32_t* const l_st = (int32_t*)st.given_or(WS_L_ST, io->status_all, N * i4);
  int32_t* const l_it = (int32_t*)st.given_or(WS_L_IT, io->iters_all, N * i4);
  int32_t* const l_cv = (int32_t*)st.given_or(WS_L_CV, io->converged_all, N * i4);
  double* const l_starts = io->seeds_out ? (double*)st.given_or(WS_L_STARTS, io->seeds_out, N * nq * f8) : nullptr;
  double* const c_q = l_starts ? nullptr : st.f64(WS_C_Q, (per < R ? per : R) * S * nq);
  if (!st.ok()) return st.finish();
  // ---- the loops: multi-start on the (B·G) flattened pairs
  auto rows_at = [&](size_t r0) {
    const size_t i0 = r0 * S;
    return MsRows{l_starts ? l_starts + i0 * nq : c_q, l_q + i0 * nq, l_v + i0 * nv, l_st + i0, l_it + i0, l_cv + i0, nullptr};
  };
  if (const int32_t rc = ms_rungs(st, R, S, in, ls, rng_seed, target_index0 * G, flags, rows_at)) return st.finish(rc);
  if (p->checker) clearance_rows(st, p->checker, N, l_q, nullptr, nullptr, nullptr, nullptr, l_st);
  // ---- the two levels
  goalset_select(st, B, G, S, *io, l_q, l_v, l_st, l_it, l_cv, d_ref ? d_ref : d_q, d_w);
  if (devp) return st.finish();
  st.down(io->q_all, l_q, N * nq * f8);
  st.down(io->status_all, l_st, N * i4);
  st.down(io->iters_all, l_it, N * i4);
  st.down(io->converged_all, l_cv, N * i4);
  st.down(io->seeds_out, l_starts, N * nq * f8);
  return st.finish();
}

int32_t mkh_select_goalset(MkhProblem* p, int32_t B, int32_t G, int32_t S, const double* q_candidates, const int32_t* valid,
                           const double* q_ref, const double* weights, const MkhGoalSetIO* io, int32_t flags, void* hip_stream) {
  const char* const who = "mkh_select_goalset";
  if (!p) return fail(MKH_E_INVALID, "null problem");
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  if (const int32_t rc = goalset_refuse(B, G, S, io, false, devp, who)) return rc;
  if (const int32_t rc = refuse_unwind(flags, who)) return rc;
  if (!q_candidates || !q_ref) return fail(MKH_E_INVALID, "%s: q_candidates and q_ref are required", who);
  HIP_OK(hipSetDevice(p->model->device));
  if (const int32_t rc = ms_build_tables(p)) return rc;
  Stager st{p, (hipStream_t)hip_stream, devp, "select_goalset"};
  const size_t Bz = B, N = Bz * G * S, nq = p->dev.nq;
  const double* const d_cand = st.up(WS_L_Q, q_candidates, N * nq);
  const double* const d_ref = st.up(WS_IN_REF, q_ref, Bz * nq);
  const double* const d_w = st.up(WS_IN_W, weights, p->dev.nv);
  const int32_t* const d_valid = st.up_i32(WS_L_CV, valid, N);
  if (!st.ok()) return st.finish();
  goalset_select(st, B, G, S, *io, d_cand, nullptr, nullptr, nullptr, d_valid, d_ref, d_w);
  return st.finish();
}

int32_t mkh_integrate(MkhModel* m, int32_t B, const double* q, const double* v, double dt, double* q_out,
                      int32_t flags, void* hip_stream) {
  if (!m || !q || !v || !q_out) return fail(MKH_E_INVALID, "null argument");
  if (B < 1) return fail(MKH_E_INVALID, "B must be >= 1");
  if (const int32_t rc = refuse_unwind(flags, "mkh_integrate")) return rc;
  HIP_OK(hipSetDevice(m->device));
  hipStream_t stream = (hipStream_t)hip_stream;
  DeviceProblem P;
  memset(&P, 0, sizeof P);
  P.nq = m->nq; P.nv = m->nv; P.njnt = m->njnt; P.jnt_i = m->d_jnt_i;       // (all the kernel reads)
  const long long total = (long long)B * m->njnt;
  const int block = 256;
  const int grid = (int)((total + block - 1) / block);
  if (flags & MKH_FLAG_DEVICE_PTRS) {
    hipLaunchKernelGGL(integrate_kernel, dim3(grid), dim3(block), 0, stream, P, B, q, v, dt, q_out);
    HIP_OK(hipGetLastError());
    return MKH_OK;
  }
  const size_t bq = (size_t)B * m->nq * 8, bv = (size_t)B * m->nv * 8;
  if (2 * bq + bv <= kSmallCallBytes) {               // small call: through the pinned scratch (see PinnedScratch)
    std::lock_guard<std::mutex> lock(m->small_mutex);   // (threads of one process share the model: round-3 advisor finding)
    HIP_OK(m->small.ensure());
    char* const h = m->small.host;
    char* const d = m->small.dev;
    memcpy(h, q, bq);
    memcpy(h + bq, v, bv);
    hipLaunchKernelGGL(integrate_kernel, dim3(grid), dim3(block), 0, stream, P, B, (const double*)d, (const double*)(d + bq), dt,
                       (double*)(d + bq + bv));
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(stream));
    memcpy(q_out, h + bq + bv, bq);
    return MKH_OK;
  }
  double *dq = nullptr, *dv = nullptr, *dout = nullptr;
  HIP_OK(hipMalloc((void**)&dq, bq));
  hipError_t e = hipMalloc((void**)&dv, bv);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, bq);
  if (e == hipSuccess) e = hipMemcpyAsync(dq, q, bq, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dv, v, bv, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(integrate_kernel, dim3(grid), dim3(block), 0, stream, P, B, dq, dv, dt, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(q_out, dout, bq, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(dq); (void)hipFree(dv); (void)hipFree(dout);
  if (e != hipSuccess) return fail(MKH_E_HIP, "integrate: %s", hipGetErrorString(e));
  return MKH_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ mkh_lie_eval
namespace {
__device__ void assemble_ljacinv(V3 v, V3 w, double* o) {
  double J[9], Q[9];
  bool ident;
  se3_ljacinv(v, w, J, Q, ident);
  // [[J, −J·Q·J],[0, J]]  (se3.py:217-218; identity when θ² < 1e-10)
  double JQ[9], B[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) JQ[3 * i + j] = J[3 * i] * Q[j] + J[3 * i + 1] * Q[3 + j] + J[3 * i + 2] * Q[6 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) B[3 * i + j] = -(JQ[3 * i] * J[j] + JQ[3 * i + 1] * J[3 + j] + JQ[3 * i + 2] * J[6 + j]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      o[6 * i + j] = J[3 * i + j];
      o[6 * i + 3 + j] = ident ? 0.0 : B[3 * i + j];
      o[6 * (i + 3) + j] = 0.0;
      o[6 * (i + 3) + 3 + j] = J[3 * i + j];
    }
}
__device__ SE3 load_se3(const double* p) { return SE3{Q4{p[0], p[1], p[2], p[3]}, V3{p[4], p[5], p[6]}}; }
__device__ void store_se3(double* o, SE3 T) {
  o[0] = T.q.w; o[1] = T.q.x; o[2] = T.q.y; o[3] = T.q.z; o[4] = T.p.x; o[5] = T.p.y; o[6] = T.p.z;
}
__global__ __launch_bounds__(64) void lie_eval_kernel(int op, int n, const double* __restrict__ a,
                                                      const double* __restrict__ b, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  V3 v, w;
  switch (op) {
    case MKH_LIE_SE3_LOG: {
      se3_log(load_se3(a + 7 * i), v, w);
      double* o = out + 6 * i;
      o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = w.x; o[4] = w.y; o[5] = w.z;
    } break;
    case MKH_LIE_SE3_JLOG: {
      se3_log(load_se3(a + 7 * i), v, w);
      assemble_ljacinv(-1.0 * v, -1.0 * w, out + 36 * i);      // jlog(T) = ljacinv(−log T)
    } break;
    case MKH_LIE_SE3_LJACINV: {
      const double* t = a + 6 * i;
      assemble_ljacinv(V3{t[0], t[1], t[2]}, V3{t[3], t[4], t[5]}, out + 36 * i);
    } break;
    case MKH_LIE_SE3_MULTIPLY: store_se3(out + 7 * i, se3_mul(load_se3(a + 7 * i), load_se3(b + 7 * i))); break;
    case MKH_LIE_SE3_INVERSE: store_se3(out + 7 * i, se3_inv(load_se3(a + 7 * i))); break;
    case MKH_LIE_SE3_RMINUS: {
      se3_log(se3_mul(se3_inv(load_se3(b + 7 * i)), load_se3(a + 7 * i)), v, w);
      double* o = out + 6 * i;
      o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = w.x; o[4] = w.y; o[5] = w.z;
    } break;
    case MKH_LIE_SO3_LOG: {
      const double* q = a + 4 * i;
      w = so3_log(Q4{q[0], q[1], q[2], q[3]});
      out[3 * i] = w.x; out[3 * i + 1] = w.y; out[3 * i + 2] = w.z;
    } break;
    case MKH_LIE_SO3_MATRIX: {
      const double* q = a + 4 * i;
      const M3 R = qmat(Q4{q[0], q[1], q[2], q[3]});
      for (int k = 0; k < 9; ++k) out[9 * i + k] = R.m[k];
    } break;
    case MKH_LIE_SE3_APPLY: {
      const SE3 T = load_se3(a + 7 * i);
      const V3 r = qrot(T.q, V3{b[3 * i], b[3 * i + 1], b[3 * i + 2]}) + T.p;
      out[3 * i] = r.x; out[3 * i + 1] = r.y; out[3 * i + 2] = r.z;
    } break;
  }
}
}  // namespace

extern "C" int32_t mkh_lie_eval(int32_t device, int32_t op, int32_t n, const double* a, const double* b, double* out,
                                int32_t flags, void* hip_stream) {
  static const int in_a[] = {7, 7, 6, 7, 7, 7, 4, 4, 7}, in_b[] = {0, 0, 0, 7, 0, 7, 0, 0, 3},
                   n_out[] = {6, 36, 36, 7, 7, 6, 3, 9, 3};
  if (op < 0 || op > MKH_LIE_SE3_APPLY) return fail(MKH_E_INVALID, "mkh_lie_eval: unknown op %d", op);
  if (n < 1 || !a || !out || (in_b[op] && !b)) return fail(MKH_E_INVALID, "mkh_lie_eval: null argument or n < 1");
  if (const int32_t rc = refuse_unwind(flags, "mkh_lie_eval")) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MKH_E_NOGPU, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(MKH_E_INVALID, "device %d out of range (%d visible)", device, ndev);
  HIP_OK(hipSetDevice(device));
  hipStream_t stream = (hipStream_t)hip_stream;
  const int grid = (n + 63) / 64;
  if (flags & MKH_FLAG_DEVICE_PTRS) {
    hipLaunchKernelGGL(lie_eval_kernel, dim3(grid), dim3(64), 0, stream, op, n, a, b, out);
    HIP_OK(hipGetLastError());
    return MKH_OK;
  }
  double *da = nullptr, *db = nullptr, *dout = nullptr;
  const size_t ba = (size_t)n * in_a[op] * 8, bb = (size_t)n * in_b[op] * 8, bo = (size_t)n * n_out[op] * 8;
  hipError_t e = hipMalloc((void**)&da, ba);
  if (e == hipSuccess) e = hipMalloc((void**)&db, bb ? bb : 8);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, bo);
  if (e == hipSuccess) e = hipMemcpyAsync(da, a, ba, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess && bb) e = hipMemcpyAsync(db, b, bb, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(lie_eval_kernel, dim3(grid), dim3(64), 0, stream, op, n, da, db, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, bo, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
  if (e != hipSuccess) return fail(MKH_E_HIP, "lie_eval: %s", hipGetErrorString(e));
  return MKH_OK;
}

// ------------------------------------------------------------------ mkh_geom_distance_eval
namespace {
// One geom pair per lane through the device's geom_distance (collide_dev.h / convex_dev.h) — the routine behind the
// collision rows — with the wave-level second half for general convex pairs whose cores overlap.  A pair is 22 doubles: two
// records of (type, size[3], pos[3], quat[4] wxyz).
__global__ __launch_bounds__(64) void geom_distance_eval_kernel(int n, const double* __restrict__ g, double distmax,
                                                                double* __restrict__ dist_out, double* __restrict__ fromto_out) {
  __shared__ __attribute__((aligned(16))) double ws[kEpaWsDoubles > 2 * kGjkWsDoubles ? kEpaWsDoubles : 2 * kGjkWsDoubles];
  const int lane = lane_id();
  const int base = blockIdx.x * 64;
  auto load = [&](int i, int& t1, V3& s1, V3& p1, Q4& q1, int& t2, V3& s2, V3& p2, Q4& q2) {
    const double* r = g + 22 * (size_t)i;
    t1 = (int)r[0]; s1 = {r[1], r[2], r[3]}; p1 = {r[4], r[5], r[6]}; q1 = {r[7], r[8], r[9], r[10]};
    t2 = (int)r[11]; s2 = {r[12], r[13], r[14]}; p2 = {r[15], r[16], r[17]}; q2 = {r[18], r[19], r[20], r[21]};
  };
  const int i = base + lane;
  const bool want = i < n;
  double dist = distmax;
  V3 from{0, 0, 0}, to{0, 0, 0};
  bool need_epa = false, known = true;
  if (want) {
    int t1, t2; V3 s1, p1, s2, p2; Q4 q1, q2;
    load(i, t1, s1, p1, q1, t2, s2, p2, q2);
    // (two GJK banks: every lane of this kernel may hold a convex pair)
    known = geom_distance<false, true>(t1, s1, p1, q1, t2, s2, p2, q2, distmax, dist, from, to, nullptr, 0, nullptr, 0, &need_epa,
                                       ws + (lane >> 5) * kGjkWsDoubles + (lane & 31));
  }
  for (unsigned long long em = __ballot(want && need_epa); em; em &= em - 1) {
    const int l = (int)__builtin_ctzll(em);
    int t1, t2; V3 s1, p1, s2, p2; Q4 q1, q2;
    load(base + l, t1, s1, p1, q1, t2, s2, p2, q2);
    // (loose polytope + polish on the pair's lane; without a certificate the tight polytope — collide_dev.h geom_overlap_polish)
    bool certified = false;
#pragma nounroll
    for (int pass = geom_overlap_loose(t1, t2) ? 0 : 1; pass < 2 && !certified; ++pass) {
      double d_e; V3 f_e, t_e;
      geom_overlap_distance(t1, s1, p1, q1, t2, s2, p2, q2, d_e, f_e, t_e, nullptr, 0, nullptr, 0, ws, pass ? mkh::kEpaTol : mkh::kLooseEpa);
      bool ok = false;
      if (lane == l) { dist = d_e; from = f_e; to = t_e; ok = geom_overlap_polish(t1, s1, p1, q1, t2, s2, p2, q2, dist, from, to, pass != 0); }
      certified = __ballot(ok) != 0;
    }
  }
  if (want) {
    dist_out[i] = known ? dist : __builtin_nan("");
    double* o = fromto_out + 6 * (size_t)i;
    o[0] = from.x; o[1] = from.y; o[2] = from.z; o[3] = to.x; o[4] = to.y; o[5] = to.z;
  }
}
}  // namespace

extern "C" int32_t mkh_geom_distance_eval(int32_t device, int32_t n, const double* pairs, double distmax, double* dist_out,
                                          double* fromto_out, void* hip_stream) {
  if (n < 1 || !pairs || !dist_out || !fromto_out) return fail(MKH_E_INVALID, "mkh_geom_distance_eval: null argument or n < 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MKH_E_NOGPU, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(MKH_E_INVALID, "device %d out of range (%d visible)", device, ndev);
  HIP_OK(hipSetDevice(device));
  hipStream_t stream = (hipStream_t)hip_stream;
  double *dg = nullptr, *dd = nullptr, *df = nullptr;
  hipError_t e = hipMalloc((void**)&dg, (size_t)n * 22 * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&dd, (size_t)n * 8);
  if (e == hipSuccess) e = hipMalloc((void**)&df, (size_t)n * 48);
  if (e == hipSuccess) e = hipMemcpyAsync(dg, pairs, (size_t)n * 22 * 8, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(geom_distance_eval_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, n, dg, distmax, dd, df);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(dist_out, dd, (size_t)n * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(fromto_out, df, (size_t)n * 48, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  (void)hipFree(dg); (void)hipFree(dd); (void)hipFree(df);
  if (e != hipSuccess) return fail(MKH_E_HIP, "geom_distance_eval: %s", hipGetErrorString(e));
  return MKH_OK;
}
