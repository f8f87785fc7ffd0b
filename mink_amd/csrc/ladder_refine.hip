// Ladder refinement (mkh_ladder_refine, mkh_solve_trajectory_ladder_refined; include/minkhip.h "THE RULE OF THE REFINEMENT"):
// the two small kernels around the 2T − 1 loop launches of the pass — the step kernel, which commits one waypoint's loop result
// and decides the next waypoint, and the guard kernel, which prices the working path r and the input path p and returns the
// better one — and their launchers (declared in outer_launch.h).  The loops are the solve kernels' own, launched by minkhip.hip
// the way mkh_solve_trajectory launches a waypoint.  Paths are batch-major: row b·T + t.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"
#include "ms_distance.h"
#include "outer_launch.h"
#include "wave_ops.h"

namespace mkh {

// c(a → b) of THE RULE: multi-start's distance from a to b; a NaN or an overflow prices the edge at +inf.
__device__ __forceinline__ double lr_edge_cost(const int32_t* jnt, int njnt, const double* a, const double* b, const double* w) {
  double d[1];
  ms_distance_strided<1>(jnt, njnt, b, 1, a, 1, 1, w, d);
  return (d[0] >= 0.0 && d[0] <= 1.7976931348623157e308) ? d[0] : __builtin_huge_val();
}

// Whether a loop result tracks: the ladder's definition (ladder.hip, ladder_tracked_kernel).
__device__ __forceinline__ bool lr_tracks(int32_t converged, int32_t status) { return converged != 0 && (status & ~1) == 0; }

// One of the three margins lr_check_kernel left for instance b (k = 0: margin(x), 1: near edge, 2: far edge): the minimum over
// the nw slots its samples were dealt to, a NaN deciding — numpy's min over all samples.
__device__ __forceinline__ double lr_trip(const double* __restrict__ trip, int b, int k, int nw) {
  const double* const s = trip + ((size_t)b * 3 + k) * nw;
  double m = s[0];
  for (int i = 1; i < nw; ++i) {
    const double v = s[i];
    if (v != v || m != m) m = __builtin_nan("");
    else if (v < m) m = v;
  }
  return m;
}

// One thread per instance; called between two loop launches.  (1) COMMIT waypoint ct of the sweep in direction cdir (+1
// forward, −1 backward; ct < 0: nothing to commit): an instance that was bad there takes the loop's result x when it tracks and
// the edge to the neighbour the sweep came from stays within the gate.  (2) DECIDE waypoint nt of the sweep in direction ndir
// (nt < 0: nothing follows): the bad flag, and the start of the next loop — the neighbour the sweep comes from where bad, the
// node itself elsewhere.  r is read after it is written here, by the thread that wrote it: none of its pointers is restrict.
// FREE: THE RULE OF THE REFINEMENT "with a checker" — r_trk holds EFFECTIVE flags; trip (B, 3, nw) is what lr_check_kernel left for
// the committed waypoint: margin(x) | the near edge's swept margin | the far edge's; r_nm / r_em (B, T) are r's node and edge
// margins, maintained here.  An edge collides iff it was swept — its destination is effectively tracked — and !(margin >= 0).
template <bool FREE>
__device__ __forceinline__ void ladder_refine_step_body(
    int B, int T, int nq, int nv, int njnt, const int32_t* __restrict__ jnt, const double* __restrict__ q0,
    const double* __restrict__ weights, double max_step_sq, int ct, int cdir, int nt, int ndir, double* r, int32_t* r_trk,
    int32_t* __restrict__ r_rep, double* __restrict__ r_v, int32_t* __restrict__ r_st, int32_t* __restrict__ r_it,
    int32_t* __restrict__ r_cv, const double* __restrict__ x, const double* __restrict__ xv, const int32_t* __restrict__ xst,
    const int32_t* __restrict__ xit, const int32_t* __restrict__ xcv, int32_t* __restrict__ bad, double* __restrict__ start,
    double* r_nm, double* r_em, const double* __restrict__ trip, int nw) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const size_t row0 = (size_t)b * T;
  if (ct >= 0 && bad[b] != 0) {
    const double* const xb = x + (size_t)b * nq;
    bool ok = lr_tracks(xcv[b], xst[b]);
    double m_node = 0.0, near = 0.0;
    if constexpr (FREE) {
      m_node = lr_trip(trip, b, 0, nw);
      near = lr_trip(trip, b, 1, nw);
      ok = ok && m_node >= 0.0;                                  // (margin(x): a NaN is in collision)
    }
    if (ok && cdir > 0 && ct >= 1) ok = !(lr_edge_cost(jnt, njnt, r + (row0 + ct - 1) * nq, xb, weights) > max_step_sq);
    if (ok && cdir < 0) ok = !(lr_edge_cost(jnt, njnt, xb, r + (row0 + ct + 1) * nq, weights) > max_step_sq);
    if constexpr (FREE) {
      // the near edge: forward r_{t-1} → x, swept always (x is free); backward x → r_{t+1}, swept iff r_{t+1} is tracked
      if (ok && cdir > 0 && ct >= 1) ok = near >= 0.0;
      if (ok && cdir < 0 && r_trk[row0 + ct + 1] != 0) ok = near >= 0.0;
    }
    if (ok) {
      const size_t row = row0 + ct;
      if constexpr (FREE) {
        const double far = lr_trip(trip, b, 2, nw);                // (near, far: NaN where lr_check_kernel did not sweep)
        r_nm[row] = m_node;
        if (cdir > 0) {
          if (ct >= 1) r_em[row] = near;
          if (ct + 1 < T) r_em[row + 1] = far;
        } else {
          r_em[row + 1] = near;
          if (ct >= 1) r_em[row] = far;
        }
      }
      for (int k = 0; k < nq; ++k) r[row * nq + k] = xb[k];
      for (int k = 0; k < nv; ++k) r_v[row * nv + k] = xv[(size_t)b * nv + k];
      r_st[row] = xst[b]; r_it[row] = xit[b]; r_cv[row] = xcv[b];
      r_trk[row] = 1;
      r_rep[row] = cdir > 0 ? 1 : 2;
    }
  }
  if (nt < 0) return;
  const size_t row = row0 + nt;
  const double* const node = r + row * nq;
  const double* from;                                     // the neighbour the sweep comes from
  bool is_bad = r_trk[row] == 0;
  if (ndir > 0) {
    from = nt ? node - nq : q0 + (size_t)b * nq;
    if (!is_bad && nt >= 1) is_bad = lr_edge_cost(jnt, njnt, from, node, weights) > max_step_sq;     // (the start edge is never a break)
    if constexpr (FREE)
      if (!is_bad && nt >= 1) is_bad = !(r_em[row] >= 0.0);      // (the node is tracked: the edge into it was swept)
  } else {
    from = node + nq;
    if (!is_bad) is_bad = lr_edge_cost(jnt, njnt, node, from, weights) > max_step_sq;
    if constexpr (FREE)
      if (!is_bad) is_bad = r_trk[row + 1] != 0 && !(r_em[row + 1] >= 0.0);
  }
  bad[b] = is_bad ? 1 : 0;
  const double* const src = is_bad ? from : node;
  for (int k = 0; k < nq; ++k) start[(size_t)b * nq + k] = src[k];
}

__global__ __launch_bounds__(256) void ladder_refine_step_kernel(
    int B, int T, int nq, int nv, int njnt, const int32_t* __restrict__ jnt, const double* __restrict__ q0,
    const double* __restrict__ weights, double max_step_sq, int ct, int cdir, int nt, int ndir, double* r, int32_t* r_trk,
    int32_t* __restrict__ r_rep, double* __restrict__ r_v, int32_t* __restrict__ r_st, int32_t* __restrict__ r_it,
    int32_t* __restrict__ r_cv, const double* __restrict__ x, const double* __restrict__ xv, const int32_t* __restrict__ xst,
    const int32_t* __restrict__ xit, const int32_t* __restrict__ xcv, int32_t* __restrict__ bad, double* __restrict__ start) {
  ladder_refine_step_body<false>(B, T, nq, nv, njnt, jnt, q0, weights, max_step_sq, ct, cdir, nt, ndir, r, r_trk, r_rep, r_v, r_st, r_it,
                                 r_cv, x, xv, xst, xit, xcv, bad, start, nullptr, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(256) void ladder_refine_step_free_kernel(
    int B, int T, int nq, int nv, int njnt, const int32_t* __restrict__ jnt, const double* __restrict__ q0,
    const double* __restrict__ weights, double max_step_sq, int ct, int cdir, int nt, int ndir, double* r, int32_t* r_trk,
    int32_t* __restrict__ r_rep, double* __restrict__ r_v, int32_t* __restrict__ r_st, int32_t* __restrict__ r_it,
    int32_t* __restrict__ r_cv, const double* __restrict__ x, const double* __restrict__ xv, const int32_t* __restrict__ xst,
    const int32_t* __restrict__ xit, const int32_t* __restrict__ xcv, int32_t* __restrict__ bad, double* __restrict__ start,
    double* r_nm, double* r_em, const double* __restrict__ trip, int nw) {
  ladder_refine_step_body<true>(B, T, nq, nv, njnt, jnt, q0, weights, max_step_sq, ct, cdir, nt, ndir, r, r_trk, r_rep, r_v, r_st, r_it,
                                r_cv, x, xv, xst, xit, xcv, bad, start, r_nm, r_em, trip, nw);
}

// One wavefront per instance.  The edges of both paths are priced 64 waypoints at a time, lane = waypoint; the counts of a key
// come from ballots, its length from lane 0, which adds the 64 costs in ascending t — one rounded addition each, as the search
// does.  Then the choice — r only on a strictly smaller key — and the copy: every output row of the returned path, the loops'
// rows only where the returned path was repaired.  p and tracked may be the arrays q_out and trk_out themselves: all of p is
// read before the first row is written, and a row is copied by the lanes that wrote it.
// FREE: the amended key of THE RULE OF THE REFINEMENT "with a checker" — p_trk / r_trk hold EFFECTIVE flags, f holds both paths'
// node and edge margins; a waypoint is lost when it is not effectively tracked or — t >= 1 — the edge into it collides (it was
// swept, its destination being tracked, and !(margin >= 0)).  The margins and the collision flags of the returned path go out.
template <bool FREE>
__device__ __forceinline__ void ladder_refine_guard_body(
    int B, int T, int nq, int nv, int njnt, const int32_t* __restrict__ jnt, const double* __restrict__ q0,
    const double* __restrict__ weights, double max_step_sq, const double* p, const int32_t* p_trk, const double* __restrict__ r,
    const int32_t* __restrict__ r_trk, const int32_t* __restrict__ r_rep, const double* __restrict__ r_v,
    const int32_t* __restrict__ r_st, const int32_t* __restrict__ r_it, const int32_t* __restrict__ r_cv, int32_t* r_eb,
    double* q_out, int32_t* trk_out, int32_t* __restrict__ rep_out, int32_t* __restrict__ refined, int32_t* edge_break,
    int32_t* __restrict__ n_tracked, int32_t* __restrict__ n_breaks, double* __restrict__ path_length, double* __restrict__ v_out,
    int32_t* __restrict__ st_out, int32_t* __restrict__ it_out, int32_t* __restrict__ cv_out, const LrFreeGuard& f) {
#pragma clang fp contract(off)      // length: one rounded addition per edge, never fused into the distance
  __shared__ double cost_p[64], cost_r[64];
  __shared__ int take_r;
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  const size_t row0 = (size_t)b * T;
  int lost_p = 0, lost_r = 0, brk_p = 0, brk_r = 0, col_p = 0, col_r = 0;
  double len_p = 0.0, len_r = 0.0;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    bool bp = false, br = false, lp = false, lr = false, cp_ = false, cr_ = false;
    if (t < T) {
      const size_t row = row0 + t;
      const double cp = lr_edge_cost(jnt, njnt, t ? p + (row - 1) * nq : q0 + (size_t)b * nq, p + row * nq, weights);
      const double cr = lr_edge_cost(jnt, njnt, t ? r + (row - 1) * nq : q0 + (size_t)b * nq, r + row * nq, weights);
      cost_p[lane] = cp; cost_r[lane] = cr;
      bp = t != 0 && cp > max_step_sq;                    // (the start edge is never a break)
      br = t != 0 && cr > max_step_sq;
      lp = p_trk[row] == 0; lr = r_trk[row] == 0;
      if constexpr (FREE) {
        cp_ = t != 0 && !lp && !(f.p_em[row] >= 0.0);
        cr_ = t != 0 && !lr && !(f.r_em[row] >= 0.0);
        lp = lp || cp_; lr = lr || cr_;
      }
      edge_break[row] = bp ? 1 : 0;
      r_eb[row] = br ? 1 : 0;
    }
    lost_p += __popcll(__ballot(lp)); lost_r += __popcll(__ballot(lr));
    if constexpr (FREE) { col_p += __popcll(__ballot(cp_)); col_r += __popcll(__ballot(cr_)); }
    brk_p += __popcll(__ballot(bp)); brk_r += __popcll(__ballot(br));
    __syncthreads();
    if (lane == 0) {
      const int n = T - t0 < 64 ? T - t0 : 64;
      for (int k = 0; k < n; ++k) { len_p = len_p + cost_p[k]; len_r = len_r + cost_r[k]; }
    }
    __syncthreads();
  }
  if (lane == 0) {
    const bool better = lost_r < lost_p || (lost_r == lost_p && (brk_r < brk_p || (brk_r == brk_p && len_r < len_p)));
    take_r = better ? 1 : 0;
    refined[b] = better ? 1 : 0;
    n_tracked[b] = T - (better ? lost_r : lost_p);
    n_breaks[b] = better ? brk_r : brk_p;
    path_length[b] = better ? len_r : len_p;
    if constexpr (FREE) f.n_edge_collisions[b] = better ? col_r : col_p;
  }
  __syncthreads();
  const bool take = take_r != 0;
  const double* const src = take ? r : p;
  for (size_t e = lane; e < (size_t)T * nq; e += 64) q_out[row0 * nq + e] = src[row0 * nq + e];
  for (int t = lane; t < T; t += 64) {
    const size_t row = row0 + t;
    const int rep = take ? r_rep[row] : 0;
    trk_out[row] = (take ? r_trk[row] : p_trk[row]) != 0 ? 1 : 0;
    rep_out[row] = rep;
    if (take) edge_break[row] = r_eb[row];
    if constexpr (FREE) {
      const double em = take ? f.r_em[row] : f.p_em[row];
      f.edge_margin[row] = em;
      f.edge_collision[row] = (t != 0 && trk_out[row] != 0 && !(em >= 0.0)) ? 1 : 0;
      if (f.node_margin) f.node_margin[row] = take ? f.r_nm[row] : f.p_nm[row];
    }
    if (rep) {
      if (st_out) st_out[row] = r_st[row];
      if (it_out) it_out[row] = r_it[row];
      if (cv_out) cv_out[row] = r_cv[row];
    }
  }
  if (take && v_out)
    for (size_t e = lane; e < (size_t)T * nv; e += 64)
      if (r_rep[row0 + e / nv]) v_out[row0 * nv + e] = r_v[row0 * nv + e];
}

#define MKH_LR_GUARD_PARAMS                                                                                                          \
    int B, int T, int nq, int nv, int njnt, const int32_t* __restrict__ jnt, const double* __restrict__ q0,                          \
    const double* __restrict__ weights, double max_step_sq, const double* p, const int32_t* p_trk, const double* __restrict__ r,     \
    const int32_t* __restrict__ r_trk, const int32_t* __restrict__ r_rep, const double* __restrict__ r_v,                            \
    const int32_t* __restrict__ r_st, const int32_t* __restrict__ r_it, const int32_t* __restrict__ r_cv, int32_t* r_eb,             \
    double* q_out, int32_t* trk_out, int32_t* __restrict__ rep_out, int32_t* __restrict__ refined, int32_t* edge_break,              \
    int32_t* __restrict__ n_tracked, int32_t* __restrict__ n_breaks, double* __restrict__ path_length, double* __restrict__ v_out,   \
    int32_t* __restrict__ st_out, int32_t* __restrict__ it_out, int32_t* __restrict__ cv_out
#define MKH_LR_GUARD_ARGS                                                                                                            \
    B, T, nq, nv, njnt, jnt, q0, weights, max_step_sq, p, p_trk, r, r_trk, r_rep, r_v, r_st, r_it, r_cv, r_eb, q_out, trk_out, rep_out, \
    refined, edge_break, n_tracked, n_breaks, path_length, v_out, st_out, it_out, cv_out

__global__ __launch_bounds__(64) void ladder_refine_guard_kernel(MKH_LR_GUARD_PARAMS) {
  ladder_refine_guard_body<false>(MKH_LR_GUARD_ARGS, LrFreeGuard{});
}

__global__ __launch_bounds__(64) void ladder_refine_guard_free_kernel(MKH_LR_GUARD_PARAMS, const LrFreeGuard f) {
  ladder_refine_guard_body<true>(MKH_LR_GUARD_ARGS, f);
}

hipError_t launch_lr_step(hipStream_t stream, int B, int T, int nq, int nv, int njnt, const int32_t* jnt, const double* q0,
                          const double* weights, double max_step_sq, int commit_t, int commit_dir, int next_t, int next_dir,
                          const LrWork& w) {
  if (B < 1 || T < 1 || commit_t >= T || next_t >= T) return hipErrorInvalidValue;
  if ((commit_dir < 0 && commit_t > T - 2) || (next_dir < 0 && next_t > T - 2)) return hipErrorInvalidValue;   // (a backward step reads t + 1)
  unsigned grid;
  if (!grid_1d(B, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_refine_step_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, B, T, nq, nv, njnt, jnt, q0, weights,
                     max_step_sq, commit_t, commit_dir, next_t, next_dir, w.r, w.r_trk, w.r_rep, w.r_v, w.r_st, w.r_it, w.r_cv, w.x,
                     w.xv, w.xst, w.xit, w.xcv, w.bad, w.start);
  return hipGetLastError();
}

hipError_t launch_lr_step_free(hipStream_t stream, int B, int T, int nq, int nv, int njnt, const int32_t* jnt, const double* q0,
                               const double* weights, double max_step_sq, int commit_t, int commit_dir, int next_t, int next_dir,
                               const LrWork& w, const LrFreeWork& f) {
  if (B < 1 || T < 1 || commit_t >= T || next_t >= T || f.slots < 1) return hipErrorInvalidValue;
  if ((commit_dir < 0 && commit_t > T - 2) || (next_dir < 0 && next_t > T - 2)) return hipErrorInvalidValue;   // (a backward step reads t + 1)
  unsigned grid;
  if (!grid_1d(B, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_refine_step_free_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, B, T, nq, nv, njnt, jnt, q0, weights,
                     max_step_sq, commit_t, commit_dir, next_t, next_dir, w.r, w.r_trk, w.r_rep, w.r_v, w.r_st, w.r_it, w.r_cv, w.x,
                     w.xv, w.xst, w.xit, w.xcv, w.bad, w.start, f.r_nm, f.r_em, (const double*)f.trip, f.slots);
  return hipGetLastError();
}

hipError_t launch_lr_guard(hipStream_t stream, int B, int T, int nq, int nv, int njnt, const int32_t* jnt, const double* q0,
                           const double* weights, double max_step_sq, const double* p, const int32_t* p_trk, const LrWork& w,
                           const LrOut& o) {
  if (B < 1 || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_refine_guard_kernel, dim3((unsigned)B), dim3(64), 0, stream, B, T, nq, nv, njnt, jnt, q0, weights,
                     max_step_sq, p, p_trk, w.r, w.r_trk, w.r_rep, w.r_v, w.r_st, w.r_it, w.r_cv, w.r_eb, o.q, o.tracked, o.repaired,
                     o.refined, o.edge_break, o.n_tracked, o.n_breaks, o.path_length, o.v, o.status, o.iters, o.converged);
  return hipGetLastError();
}

hipError_t launch_lr_guard_free(hipStream_t stream, int B, int T, int nq, int nv, int njnt, const int32_t* jnt, const double* q0,
                                const double* weights, double max_step_sq, const double* p, const int32_t* p_trk, const LrWork& w,
                                const LrOut& o, const LrFreeGuard& f) {
  if (B < 1 || T < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_refine_guard_free_kernel, dim3((unsigned)B), dim3(64), 0, stream, B, T, nq, nv, njnt, jnt, q0, weights,
                     max_step_sq, p, p_trk, w.r, w.r_trk, w.r_rep, w.r_v, w.r_st, w.r_it, w.r_cv, w.r_eb, o.q, o.tracked, o.repaired,
                     o.refined, o.edge_break, o.n_tracked, o.n_breaks, o.path_length, o.v, o.status, o.iters, o.converged, f);
  return hipGetLastError();
}

}  // namespace mkh
