// convex_check_kernel — the general convex distance routine on the rows a check judges INSIDE its launch, in front of
// tmf_check_cv_kernel (trajectory_free.hip: candidate tracking) and lr_check_cv_kernel (ladder_refine_free.hip: the refinement
// pass "with a checker").
//
// Those checks decide inside the kernel which edges they sweep — only behind a free node —, and a pre-pass cannot know that
// verdict.  Everything ELSE their conditions read is in memory before the launch, so this pre-pass is SPECULATIVE: it evaluates
// the general convex pairs of every row the check could read, the check's conditions without the node's verdict, and the check
// reads a subset.  The invariant: every value the check reads was written here, for the same chunk, behind the same conditions.
//
// One LANE takes one (item, row j of the item, general convex pair k) of a chunk of items; the lane body is convex_lane.h's,
// shared with convex_sweep_kernel.  The distance alone goes to row (item − first) · rows_per_item + j of the checker's buffer
// (mkh_problem_set_check_rows), which the checks read through clr_row<LPR, 1>.  Two decodes of an item:
//
//   tracking    the item is row g of the time-major (T, R, nq) candidates, rows j = 0 … M.  j = 0: the node, the row as it stands
//               in memory (the plain accessor, not a blend at u = 1), evaluated iff the row is finite.  j >= 1: sample j of the
//               edge q_all[g − R] → q_all[g], evaluated iff g >= R, the row converged (or `converged` is null), its status AS IT
//               STANDS IN FRONT OF THE CHECK has no failure bit, and both ends are finite.
//   refinement  the item is instance b, rows j = 0 … 2M.  j = 0: x[b]; j = 1 … M: the near edge; j = M + 1 … 2M: the far edge —
//               lr_check_kernel's `work`, `has_prev` and `next_trk` without `free_x`.  Every slot of the check reads the same
//               buffer.
//
// The samples' coordinates are CvRowBlend's (sweep_blend.h's per-joint functions, u = j / (M + 1)): the analytic pairs of a sample,
// which the check builds in LDS, see the same doubles.  No bounding-sphere cull (convex_sweep.hip, and why).  A wavefront with no
// live item leaves at once.
#include <hip/hip_runtime.h>

#define MKH_POLISH_BY_VALUE 1      // (convex_dev.h cvx_polish: this kernel carries the routine without scratch)
#include "checker_plan.h"
#include "convex_lane.h"
#include "outer_launch.h"
#include "problem_plan.h"

namespace mkh {

// A row of an item: the row `b` as it stands (plain), or q(u) between a and b — one accessor, so that the chain walk and the
// routine behind it are in the kernel once.
struct CvRowCheck {
  CvRowBlend e;
  bool plain;
  __device__ __forceinline__ double scalar(int qa) const { return plain ? e.b[qa] : e.scalar(qa); }
  __device__ __forceinline__ V3 pos(int qa) const { return V3{scalar(qa), scalar(qa + 1), scalar(qa + 2)}; }
  __device__ __forceinline__ Q4 quat(int qa) const {
    // (deliberate: a node row forms the blend too and drops it — one row in 1 + M, and a branch here would put the chain walk
    //  behind it in the kernel twice)
    const Q4 s = e.quat(qa);
    return plain ? Q4{e.b[qa], e.b[qa + 1], e.b[qa + 2], e.b[qa + 3]} : s;
  }
};

struct CvCheckRow {                // what row j of an item is
  const double *pa, *pb;           // the ends of its edge (the node: pb, twice)
  bool live;                       // the check's conditions, without the node's verdict and without the finiteness of the ends
  bool node;
  int sample;                      // 1 … M
};

__device__ __forceinline__ CvCheckRow cvc_row(const CvCheckArgs& a, long long c, int j, int nq) {
  CvCheckRow w;
  w.node = j == 0;
  if (a.mode == kCvCheckTrack) {
    const long long g = a.first + c;
    w.pb = a.q_all + (size_t)g * nq;
    const bool first = g < a.R;
    w.pa = (w.node || first) ? w.pb : w.pb - (size_t)a.R * nq;         // (every address is valid)
    w.sample = j;
    w.live = w.node || (!first && (a.converged ? a.converged[g] != 0 : true) && (a.status[g] & ~1) == 0);
  } else {
    const long long b = a.first + c;
    const bool work = a.bad[b] != 0 && a.xcv[b] != 0 && (a.xst[b] & ~1) == 0;
    const size_t row = (size_t)b * a.T + a.ct;
    const double* const px = a.x + (size_t)b * nq;
    const double* const nd = a.r + row * nq;
    const bool has_prev = a.ct >= 1, has_next = a.ct + 1 < a.T;
    const bool next_trk = has_next && a.r_trk[has_next ? row + 1 : row] != 0;
    const int e = j > a.M ? 1 : 0;                                   // 0: the near edge, 1: the far edge
    const bool into_x = (a.cdir > 0) == (e == 0);                    // the edge r_{t-1} → x; else x → r_{t+1}
    const bool swept = w.node || (into_x ? has_prev : next_trk);
    w.sample = e ? j - a.M : j;
    w.live = work && swept;
    w.pa = (w.node || !w.live) ? px : (into_x ? nd - nq : px);
    w.pb = (w.node || !w.live) ? px : (into_x ? px : nd + nq);
  }
  return w;
}

// `ipw` items per wavefront (lanes [0, ipw) work), by launch_convex_pre's rule.
__global__ __launch_bounds__(64) void convex_check_kernel(const WideProblem* __restrict__ Pg, CvPre C, const CvCheckArgs a, int ipw,
                                                          double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double ws[kCvLaneWsDoubles];
  const WideProblem& P = *Pg;
  const int lane = lane_id(), nq = P.nq;
  const int rpi = a.mode == kCvCheckTrack ? 1 + a.M : 1 + 2 * a.M;         // rows per item
  const long long base = (long long)blockIdx.x * ipw, total = a.count * rpi * C.n_cv;
  // lane item = ((item of the chunk · rows per item + j) · n_cv + slot): its index in `out`
  auto decode = [&](long long it, int& k) {
    const long long row = it / C.n_cv;
    k = (int)(it - row * C.n_cv);
    return cvc_row(a, row / rpi, (int)(row % rpi), nq);
  };
  auto row_of = [&](int l, int& k) {
    const CvCheckRow w = decode(base + l, k);
    return CvRowCheck{CvRowBlend{w.pa, w.pb, (double)w.sample / (double)(a.M + 1)}, w.node};
  };
  const long long item = base + lane;
  bool want = lane < ipw && item < total;
  if (want) {
    int k;
    const CvCheckRow w = decode(item, k);
    want = w.live;
    if (want)
      for (int i = 0; i < nq; ++i) want = want && (w.pa[i] - w.pa[i] == 0.0) && (w.pb[i] - w.pb[i] == 0.0);
  }
  if (__ballot(want) == 0ull) return;                          // (wave-uniform)
  const double dist = cvx_lane_distance(P, C, want, lane, ws, row_of);
  if (want) out[item] = dist;
}

hipError_t launch_convex_check(hipStream_t stream, const void* wide_problem, const CvPre& C, const CvCheckArgs& a, double* out) {
  const int n_cv = C.n_cv;
  if (a.count < 1 || a.first < 0 || a.M < 1 || n_cv < 1 || !out) return hipErrorInvalidValue;
  if (a.mode == kCvCheckTrack) {
    if (a.R < 1 || !a.q_all || !a.status) return hipErrorInvalidValue;
  } else if (a.mode == kCvCheckRefine) {
    if (a.T < 1 || a.ct < 0 || a.ct >= a.T || !a.r || !a.r_trk || !a.x || !a.xst || !a.xcv || !a.bad) return hipErrorInvalidValue;
  } else {
    return hipErrorInvalidValue;
  }
  const long long rpi = a.mode == kCvCheckTrack ? 1 + (long long)a.M : 1 + 2 * (long long)a.M;
  const long long total = a.count * rpi * n_cv;
  const int ipw = cv_items_per_wave(total);
  const long long blocks = (total + ipw - 1) / ipw;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(convex_check_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, (const WideProblem*)wide_problem, C, a, ipw, out);
  return hipGetLastError();
}

}  // namespace mkh
