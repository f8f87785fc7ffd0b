// Host-only driver of mink_amd/csrc/solve_plan.h for tests/test_solve_plan_cpu.py: the refusal of a plain solve, the route of its
// arrays, the chunks and the pinned layout over a matrix of shapes and calls — one JSON object per line.  Beside each cell the
// answer of the REFERENCE: run() as minkhip.hip had it before the plain solve's planning was split out — its refusal sequence, its
// byte sum and cursor over the pinned scratch and its chunk rule, copied verbatim into ref::run below (`fail` writes into a string
// of this program; where run() went on to launch, the copy records what it had decided and returns).  Built with the host
// sanitizers by the test and run as a child process.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../mink_amd/csrc/solve_plan.h"

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

// what the copied code reads of a handle and writes for the kernel
struct DeviceProblem { int nq, nv, nbody, n_frame, n_posture, n_com, n_rows_tap, n_pairs, n_dense_rows, n_dense_limit_rows, dense_box; };
struct MkhProblem { DeviceProblem dev; int max_batch; };
struct SolveArgs {
  const double *q, *frame_targets, *posture_target, *com_target;
  double* v_out; int32_t* status_out; double* q_out; int32_t *iters_out, *converged_out;
};
struct TapArgs {
  double *t_xpos, *t_xquat, *t_frame_pose, *t_subtree_com, *t_task_e, *t_task_J, *t_H, *t_c, *t_box_lo,
      *t_box_hi, *t_coll_G, *t_coll_h;
  int32_t* t_qp_iters;
  long long* t_cycles;
};
constexpr size_t kSmallCallBytes = 64 << 10;
static bool g_no_chunks = false;                    // MKH_DEBUG_NO_CHUNKS of the experiment builds
static const char* dbg_env(const char*) { return g_no_chunks ? "1" : nullptr; }

// what run() had decided when it reached a transport
enum Route { DEVICE, PINNED, STAGED, CHUNKED };
struct Decision {
  Route route; int n_chunks; size_t chunk, bytes;
  SolveArgs a; TapArgs t;                           // PINNED: the kernel's pointers into the device view of the scratch
};
static char g_host[kSmallCallBytes], g_dev[kSmallCallBytes];      // the scratch and its device view
static const double g_src[kSmallCallBytes / 8] = {};              // what a caller's input of a small call points to

// ---- verbatim from here (refuse_unwind, refuse_inputs, assign_taps, run; a `decided` where run() went on to launch)
static int32_t refuse_unwind(int32_t flags, const char* who) {
  if (flags & MKH_FLAG_UNWIND_TURNS)
    return fail(MKH_E_INVALID, "%s: MKH_FLAG_UNWIND_TURNS is honoured by mkh_solve_multistart_set and "
                               "mkh_solve_trajectory_ladder_nodes only", who);
  return MKH_OK;
}

template <typename Alloc>
static void assign_taps(const MkhTaps* taps, const DeviceProblem& P, size_t Bz, TapArgs& t, Alloc&& alloc) {
  const size_t nv = P.nv;
  t.t_xpos = (double*)alloc(taps->xpos, Bz * P.nbody * 3 * 8, false);
  t.t_xquat = (double*)alloc(taps->xquat, Bz * P.nbody * 4 * 8, false);
  t.t_frame_pose = (double*)alloc(taps->frame_pose, Bz * P.n_frame * 7 * 8, false);
  t.t_subtree_com = (double*)alloc(taps->subtree_com, Bz * 3 * 8, true);
  t.t_task_e = (double*)alloc(taps->task_e, Bz * P.n_rows_tap * 8, true);
  t.t_task_J = (double*)alloc(taps->task_J, Bz * P.n_rows_tap * nv * 8, true);
  t.t_H = (double*)alloc(taps->H, Bz * nv * nv * 8, false);
  t.t_c = (double*)alloc(taps->c, Bz * nv * 8, false);
  t.t_box_lo = (double*)alloc(taps->box_lo, Bz * nv * 8, false);
  t.t_box_hi = (double*)alloc(taps->box_hi, Bz * nv * 8, false);
  t.t_coll_G = (double*)alloc(taps->coll_G, Bz * P.n_pairs * nv * 8, true);
  t.t_coll_h = (double*)alloc(taps->coll_h, Bz * P.n_pairs * 8, false);
  t.t_qp_iters = (int32_t*)alloc(taps->qp_iters, Bz * 4, true);
  t.t_cycles = (long long*)alloc(taps->cycles, Bz * 16 * 8, true);
}

static int32_t refuse_inputs(const DeviceProblem& P, const double* q, const double* frame_targets, const double* posture_target,
                             const double* com_target, const char* until_who, const char* no_plugin) {
  if (!q) return fail(MKH_E_INVALID, "q is null");
  if (until_who && P.n_frame < 1)
    return fail(MKH_E_INVALID, "%s needs at least one frame task to test the thresholds on", until_who);
  if (P.n_frame > 0 && !frame_targets) return fail(MKH_E_INVALID, "frame_targets is null (TargetNotSet)");
  if (P.n_posture > 0 && !posture_target) return fail(MKH_E_INVALID, "posture_target is null (TargetNotSet)");
  if (P.n_com > 0 && !com_target) return fail(MKH_E_INVALID, "com_target is null (TargetNotSet)");
  if (no_plugin && (P.n_dense_rows || P.n_dense_limit_rows || P.dense_box))
    return fail(MKH_E_INVALID, "dense (plugin) rows are evaluated by the caller at q: no fused loop, no %s", no_plugin);
  return MKH_OK;
}

static int32_t run(MkhProblem* p, int32_t B, const double* q, const double* frame_targets, const double* posture_target,
                   const double* com_target, double dt, double damping, double* v_out, int32_t* status_out,
                   const MkhTaps* taps, int32_t flags, void* hip_stream, int32_t n_steps, double* q_out,
                   const MkhDenseRows* dense, double pos_threshold, double ori_threshold,
                   int32_t* iters_out, int32_t* converged_out, Decision& decided) {
  if (!p) return fail(MKH_E_INVALID, "null problem");
  if (B < 1) return fail(MKH_E_INVALID, "B must be >= 1");
  if (const int32_t rc = refuse_unwind(flags, "a solve")) return rc;       // (the outer-loop callers clear the bit in front of their loops)
  const DeviceProblem& P = p->dev;
  if (const int32_t rc = refuse_inputs(P, q, frame_targets, posture_target, com_target, nullptr, nullptr)) return rc;
  if (!(dt > 0.0)) return fail(MKH_E_INVALID, "dt must be > 0");
  if (n_steps < 1) return fail(MKH_E_INVALID, "n_steps must be >= 1");
  const size_t Kd = P.n_dense_rows, Md = P.n_dense_limit_rows;
  const bool Bd = P.dense_box != 0;
  if (!Bd && dense && (dense->limit_lo || dense->limit_hi))
    return fail(MKH_E_INVALID, "limit_lo / limit_hi need a problem created with dense_limit_box = 1");
  if (Kd || Md || Bd) {
    if (!dense) return fail(MKH_E_INVALID, "this problem has dense (plugin) rows: call mkh_solve_dense");
    if (Kd && (!dense->task_e || !dense->task_J)) return fail(MKH_E_INVALID, "dense task_e / task_J is null");
    if (Md && (!dense->limit_G || !dense->limit_h)) return fail(MKH_E_INVALID, "dense limit_G / limit_h is null");
    if (n_steps > 1 || q_out) return fail(MKH_E_INVALID, "dense (plugin) rows are evaluated by the caller at q: no fused steps");
  }
  // max_batch bounds everything the handle owns per instance — staging buffers, the warm-start active sets — whichever
  // kind of pointer the caller passes (a device-pointer warm start used to write past d_warm here)
  if (B > p->max_batch) return fail(MKH_E_INVALID, "B=%d exceeds max_batch=%d of this problem", B, p->max_batch);
  const bool devp = (flags & MKH_FLAG_DEVICE_PTRS) != 0;
  const bool pbat = (flags & MKH_FLAG_POSTURE_BATCHED) != 0, cbat = (flags & MKH_FLAG_COM_BATCHED) != 0;
  SolveArgs a;
  memset(&a, 0, sizeof a);
  TapArgs t;
  memset(&t, 0, sizeof t);
  const bool until = pos_threshold >= 0.0;
  if (until && P.n_frame < 1) return fail(MKH_E_INVALID, "mkh_solve_until needs at least one frame task to test the thresholds on");
  const size_t nq = P.nq, nv = P.nv;
  const size_t n_pt = (size_t)P.n_posture * nq * (pbat ? B : 1), n_ct = (size_t)P.n_com * 3 * (cbat ? B : 1);
  if (devp) {
    decided = {DEVICE, 1, (size_t)B, 0, a, t};
    return MKH_OK;
  }
  // ---- host pointers, small call: everything through the pinned scratch (see PinnedScratch) — inputs, outputs and taps
  {
    const size_t Bz = B;
    const size_t d_q = Bz * nq, d_ft = Bz * P.n_frame * 7, d_v = v_out ? Bz * nv : 0;
    size_t bytes = (d_q + d_ft + n_pt + n_ct + d_v) * sizeof(double) + ((Bz * (until ? 3 : 1) * sizeof(int32_t) + 7) & ~(size_t)7);
    if (taps) {
      TapArgs sizes;
      assign_taps(taps, P, Bz, sizes, [&](void* host, size_t n, bool) -> void* { if (host) bytes += (n + 7) & ~(size_t)7; return nullptr; });
    }
    decided.bytes = bytes;
    if (!Kd && !Md && !Bd && bytes <= kSmallCallBytes) {
      char* const h = g_host;
      char* const d = g_dev;
      size_t o = 0;                                    // (bytes; every block a multiple of 8)
      auto put = [&](const double* src, size_t n) -> const double* {
        if (!n) return nullptr;
        memcpy(h + o, src, n * sizeof(double));
        const double* r = (const double*)(d + o);
        o += n * sizeof(double);
        return r;
      };
      a.q = put(q, d_q);
      a.frame_targets = put(frame_targets, d_ft);
      a.posture_target = put(posture_target, n_pt);
      a.com_target = put(com_target, n_ct);
      const size_t o_v = o;
      a.v_out = v_out ? (double*)(d + o_v) : nullptr;
      o += d_v * sizeof(double);
      const size_t o_i = o;
      int32_t* const di32 = (int32_t*)(d + o_i);
      a.status_out = di32;
      a.q_out = q_out ? (double*)a.q : nullptr;        // in place, as in the staged path
      if (until) { a.iters_out = di32 + Bz; a.converged_out = di32 + 2 * Bz; }
      o += (Bz * (until ? 3 : 1) * sizeof(int32_t) + 7) & ~(size_t)7;
      struct Back { void* host; size_t off, n; };
      std::vector<Back> back;
      if (taps)
        assign_taps(taps, P, Bz, t, [&](void* host, size_t n, bool zero) -> void* {
          if (!host) return nullptr;
          if (zero) memset(h + o, 0, n);
          back.push_back({host, o, n});
          void* r = d + o;
          o += (n + 7) & ~(size_t)7;
          return r;
        });
      decided = {PINNED, 1, (size_t)B, o, a, t};
      return MKH_OK;
    }
  }
  const bool no_chunks = dbg_env("MKH_DEBUG_NO_CHUNKS") != nullptr;      // (A/B of this path; `static` in run(): read once per process)
  const size_t staged_bytes = (size_t)B * sizeof(double) *
      (nq + (size_t)P.n_frame * 7 + nv + (pbat ? (size_t)P.n_posture * nq : 0) + (cbat ? (size_t)P.n_com * 3 : 0) + (q_out ? nq : 0));
  const int n_chunks = (!no_chunks && !taps && !Kd && !Md && !Bd && v_out && B >= 2 * 8192 && staged_bytes >= ((size_t)32 << 20))
                           ? (B / 8192 < 4 ? B / 8192 : 4) : 1;
  if (n_chunks > 1) {
    const size_t chunk = ((size_t)B / n_chunks) / 64 * 64;          // ≥ 8 192; the last chunk takes the remainder
    decided = {CHUNKED, n_chunks, chunk, decided.bytes, a, t};
    return MKH_OK;
  }
  decided = {STAGED, 1, (size_t)B, decided.bytes, a, t};
  (void)damping; (void)hip_stream; (void)ori_threshold; (void)status_out; (void)iters_out; (void)converged_out;
  return MKH_OK;
}
// ---- verbatim up to here

}  // namespace ref

using namespace mkh;

struct Shape { const char* name; SolveShape s; };
static const Shape kShapes[] = {
    //                 nq  nv nbody fr po co rows pairs Kd Md box  max_batch
    {"g1_like",       {36, 35, 31, 4, 1, 0, 59, 0, 0, 0, 0, 131072}},
    {"g1",            {44, 43, 45, 4, 1, 0, 67, 0, 0, 0, 0, 131072}},
    {"ur5e_like",     {6, 6, 8, 1, 1, 0, 12, 2, 0, 0, 0, 262144}},
    {"no_frame",      {6, 6, 8, 0, 1, 0, 6, 0, 0, 0, 0, 65536}},
    {"com",           {36, 35, 31, 4, 1, 1, 62, 3, 0, 0, 0, 65536}},
    {"big_tree",      {120, 120, 121, 4, 1, 0, 144, 0, 0, 0, 0, 65536}},     // (the workgroup-per-problem kernel's: two chunks at 16 384)
    {"dense_rows",    {6, 6, 8, 1, 1, 0, 12, 0, 3, 0, 0, 65536}},
    {"dense_limits",  {6, 6, 8, 1, 1, 0, 12, 0, 0, 2, 0, 65536}},
    {"dense_box",     {6, 6, 8, 1, 1, 0, 12, 0, 0, 0, 1, 65536}},
};
static const char* const kKinds[] = {"eval", "solve", "steps", "until", "until_no_counts"};
static const char* const kRoutes[] = {"device", "pinned", "staged", "chunked"};

// a call of the matrix
struct Cell {
  int B, kind, batched, taps, devp, null_input, dt_ok, n_steps, dense, no_chunks, unwind;
};

static double g_out[1];              // what a caller's output points to (never written: nothing is launched)
static int32_t g_iout[1];

static void emit(const Shape& sh, const Cell& c) {
  const SolveShape& s = sh.s;
  // the caller's arguments
  const double* in[4] = {ref::g_src, ref::g_src, ref::g_src, ref::g_src};
  if (c.null_input >= 0) in[c.null_input] = nullptr;
  double* const v_out = c.kind >= 1 ? g_out : nullptr;
  int32_t* const status_out = c.kind >= 1 ? g_iout : nullptr;
  double* const q_out = c.kind >= 2 ? g_out : nullptr;
  const bool until = c.kind >= 3;
  int32_t* const iters = c.kind == 3 ? g_iout : nullptr;
  const int n_steps = c.kind >= 2 ? c.n_steps : (c.n_steps < 1 ? c.n_steps : 1);
  MkhTaps taps;
  memset(&taps, 0, sizeof taps);
  if (c.taps == 1) taps.qp_iters = g_iout;
  if (c.taps == 2) {
    taps.xpos = taps.xquat = taps.frame_pose = taps.subtree_com = taps.task_e = taps.task_J = taps.H = taps.c = taps.box_lo = taps.box_hi =
        taps.coll_G = taps.coll_h = g_out;
    taps.qp_iters = g_iout;
    taps.cycles = (int64_t*)g_out;
  }
  // dense: 0 none, 1 all six arrays, 2 no box arrays, 3 task_J missing, 4 limit_h missing
  MkhDenseRows dense{ref::g_src, ref::g_src, ref::g_src, ref::g_src, ref::g_src, ref::g_src};
  if (c.dense >= 2) dense.limit_lo = dense.limit_hi = nullptr;
  if (c.dense == 3) dense.task_J = nullptr;
  if (c.dense == 4) dense.limit_h = nullptr;
  const int32_t flags = (c.batched ? MKH_FLAG_POSTURE_BATCHED | MKH_FLAG_COM_BATCHED : 0) | (c.devp ? MKH_FLAG_DEVICE_PTRS : 0) |
                        (c.unwind ? MKH_FLAG_UNWIND_TURNS : 0);
  const double dt = c.dt_ok ? 5e-3 : 0.0;

  // the reference
  ref::MkhProblem rp{{s.nq, s.nv, s.nbody, s.n_frame, s.n_posture, s.n_com, s.n_rows_tap, s.n_pairs, s.n_dense_rows, s.n_dense_limit_rows, s.dense_box},
                     s.max_batch};
  ref::Decision rd{};
  ref::g_err.clear();
  ref::g_no_chunks = c.no_chunks != 0;
  const int32_t ref_rc = ref::run(&rp, c.B, in[0], in[1], in[2], in[3], dt, 0.1, v_out, status_out, c.taps ? &taps : nullptr, flags, nullptr,
                                  n_steps, q_out, c.dense ? &dense : nullptr, until ? 1e-3 : -1.0, until ? 1e-2 : -1.0, iters, iters, rd);

  // the plan
  SolveWants w{c.B, n_steps, c.batched != 0, c.batched != 0, c.devp != 0, c.unwind != 0, until, q_out != nullptr, c.taps != 0, c.dense != 0, 0};
  const void* user[A_COUNT] = {};
  user[A_Q] = in[0]; user[A_FT] = in[1]; user[A_PT] = in[2]; user[A_CT] = in[3];
  user[A_V] = v_out; user[A_STATUS] = status_out; user[A_ITERS] = iters; user[A_CONV] = iters;
  if (c.dense) memcpy(user + A_DE, &dense, sizeof dense);
  if (c.taps) memcpy(user + A_TAP0, &taps, sizeof taps);
  for (int i = 0; i < A_COUNT; ++i)
    if (user[i]) w.given |= 1u << i;
  std::string err;
  const int32_t rc = solve_refuse(s, w, dt > 0.0, err);

  printf("{\"shape\":\"%s\",\"B\":%d,\"kind\":\"%s\",\"batched\":%d,\"taps\":%d,\"devp\":%d,\"null_input\":%d,\"dt_ok\":%d,\"n_steps\":%d,\"dense\":%d,"
         "\"no_chunks\":%d,\"unwind\":%d,\"refusal\":%d,\"rc\":%d,\"err\":\"%s\",\"ref_rc\":%d,\"ref_err\":\"%s\"",
         sh.name, c.B, kKinds[c.kind], c.batched, c.taps, c.devp, c.null_input, c.dt_ok, c.n_steps, c.dense, c.no_chunks, c.unwind,
         (int)solve_refusal(s, w, dt > 0.0), rc, err.c_str(), ref_rc, ref::g_err.c_str());
  if (rc == MKH_OK && ref_rc == MKH_OK) {
    const SolveRoutePlan r = solve_route(s, w, c.no_chunks != 0);
    const PinnedLayout L = pinned_layout(s, w);
    printf(",\"route\":\"%s\",\"n_chunks\":%d,\"chunk\":%zu,\"ref_route\":\"%s\",\"ref_n_chunks\":%d,\"ref_chunk\":%zu", kRoutes[(int)r.route],
           r.n_chunks, r.chunk, kRoutes[rd.route], rd.n_chunks, rd.chunk);
    if (!c.devp) printf(",\"pinned_total\":%zu,\"ref_pinned_total\":%zu", L.total, rd.bytes);
    if (rd.route == ref::PINNED) {
      // every row's offset: the layout's where the row is live, the reference's from the pointer the kernel would have got (-1: none)
      const void* rptr[A_COUNT] = {};
      rptr[A_Q] = rd.a.q; rptr[A_FT] = rd.a.frame_targets; rptr[A_PT] = rd.a.posture_target; rptr[A_CT] = rd.a.com_target;
      rptr[A_V] = rd.a.v_out; rptr[A_STATUS] = rd.a.status_out; rptr[A_ITERS] = rd.a.iters_out; rptr[A_CONV] = rd.a.converged_out;
      memcpy(rptr + A_TAP0, &rd.t, sizeof rd.t);
      printf(",\"off\":[");
      for (int i = 0; i < A_COUNT; ++i) printf("%s%lld", i ? "," : "", solve_array(s, w, i).live ? (long long)L.off[i] : -1LL);
      printf("],\"ref_off\":[");
      for (int i = 0; i < A_COUNT; ++i) printf("%s%lld", i ? "," : "", rptr[i] ? (long long)((const char*)rptr[i] - ref::g_dev) : -1LL);
      printf("],\"ref_q_out_in_place\":%d", (int)((const void*)rd.a.q_out == (q_out ? (const void*)rd.a.q : nullptr)));
    }
  }
  printf("}\n");
}

// the smallest B at which `pred` of the reference's decision turns true (0: never below `limit`), by bisection on a monotone rule
template <class F>
static int first_B(int limit, F&& pred) {
  if (!pred(limit)) return 0;
  int lo = 0, hi = limit;                   // pred(lo) false, pred(hi) true
  while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; (pred(mid) ? hi : lo) = mid; }
  return hi;
}

int main() {
  for (const Shape& sh : kShapes) {
    const SolveShape& s = sh.s;
    const bool dense_shape = s.n_dense_rows || s.n_dense_limit_rows || s.dense_box;
    std::vector<int> Bs = {0, 1, 7, 48, 96, 16383, 16384, 26000, 36315, 36316, 40001, 65536, s.max_batch, s.max_batch + 1};
    // ... and this shape's own boundaries, from the reference's formulas: the first plain solve past 64 KB and the first at 32 MB staged
    const size_t small = ((size_t)s.nq + (size_t)s.n_frame * 7 + s.nv) * 8 + 4, shared = ((size_t)s.n_posture * s.nq + (size_t)s.n_com * 3) * 8;
    const int b64 = first_B(1 << 20, [&](int B) { return (size_t)B * (small - 4) + shared + (((size_t)B * 4 + 7) & ~(size_t)7) > ref::kSmallCallBytes; });
    const int b32 = first_B(1 << 20, [&](int B) { return (size_t)B * (small - 4) >= ((size_t)32 << 20); });
    for (int b : {b64 - 1, b64, b32 - 1, b32})
      if (b > 0 && b <= s.max_batch) Bs.push_back(b);
    for (int B : Bs)
      for (int kind = 0; kind < 5; ++kind)
        for (int devp = 0; devp < 2; ++devp)
          for (int dense = 0; dense < (dense_shape ? 5 : 2); ++dense) {
            // the axes a refusal does not read, on a call that is otherwise in order ...
            for (int batched = 0; batched < 2; ++batched)
              for (int taps = 0; taps < 3; ++taps)
                for (int no_chunks = 0; no_chunks < ((devp || B < 16384) ? 1 : 2); ++no_chunks)
                  emit(sh, Cell{B, kind, batched, taps, devp, -1, 1, 3, dense, no_chunks, 0});
            // ... and the ones it reads, one at a time and two at a time where the order decides
            for (int null_input = 0; null_input < 4; ++null_input) emit(sh, Cell{B, kind, 0, 0, devp, null_input, 1, 3, dense, 0, 0});
            for (int n_steps : {0, 1}) emit(sh, Cell{B, kind, 0, 0, devp, -1, 1, n_steps, dense, 0, 0});
            emit(sh, Cell{B, kind, 0, 0, devp, -1, 0, 3, dense, 0, 0});
            emit(sh, Cell{B, kind, 0, 0, devp, -1, 0, 0, dense, 0, 0});
            emit(sh, Cell{B, kind, 0, 0, devp, 0, 0, 3, dense, 0, 1});
            emit(sh, Cell{B, kind, 0, 0, devp, -1, 1, 3, dense, 0, 1});
          }
  }
  return 0;
}
