// The LDS layout of the wavefront-per-problem kernel's builds and the feature bits that select it: what the kernel indexes
// (ik_kernel.h kernel_lds_layout) and what the host reserves when it plans a problem (problem_plan.hip) — one statement, in a
// header that needs no kernel.  Moved verbatim out of ik_kernel.h: nothing here may be wrapped, merged or reordered (the order of
// the scalar loads of build_lds_layout is pinned by the kernels' code hashes).
#pragma once
#include <hip/hip_runtime.h>

#include "mkh_types.h"

namespace mkh {

// ------------------------------------------------------------------ LDS layout
// Row stride of the staged half-space rows A[s][:]: the smallest column-load size ≥ nv (tab_asm.inc load_lo_*),
// not the wave width — 40 rows × 64 doubles were 20 KB of Shadow's 37 KB and cost it a third of its occupancy.
__host__ __device__ inline int a_stride_for(int nv) {
  return nv <= 16 ? 16 : (nv <= 24 ? 24 : (nv <= 32 ? 32 : (nv <= 44 ? 44 : (nv <= 48 ? 48 : 64))));
}

// Row stride of the staged Jacobian rows of the direct start: only the dof rows are read (rank1_leading_rows)
__host__ __device__ inline int j_stride_direct(int nv, int nt) { const int a = a_stride_for(nv); return a < nt ? a : nt; }

constexpr int kPivBuf = kWave + 8;   // doubles per pivot broadcast buffer
constexpr int kMu = 18, kMuBig = 24; // low-rank start: compiled capacities of task-residual rows of one problem (WoodElim in tab_asm.inc)
constexpr int kWoodRow = 64;         // low-rank start: doubles of the published-row buffer — (S[r][c], w_c) pairs — in the pivot buffers, followed by 1/d_r
struct LdsLayout {
  int q, X, jnt, tgt, task, J, dof, com, col, A, piv, S, q2, tgt2, hsel, total;  // offsets in doubles
};
__host__ __device__ inline int lds_even(int x) { return (x + 1) & ~1; }
__host__ __device__ inline LdsLayout lds_layout(int nq, int nv, int nbody, int njnt, int n_frame,
                                                int n_posture, int n_com, int max_rows, int j_rows, int j_stride,
                                                int s_doubles = 0, bool prefetch = false, bool compact = false,
                                                bool wood = false, int n_hsel = 0, bool piv_small = false, bool wood_rows = false) {
  LdsLayout L;
  int o = 0;
  const int x_sz = 7 * lds_even(nbody), jnt_sz = lds_even(njnt * 6);
  const int j_sz = lds_even(j_rows * j_stride);
  L.q = o;    o += lds_even(nq);
  if (wood_rows) {
    // low-rank start WITH half-space rows (round 6; F_WOOD | F_COLL builds): the rows [r][NT] of Jh — the dof part AND, behind it,
    // the half-space rows' columns of the elimination — overwrite the joint axes and the task blocks as in the compact layout (one
    // pass of (task, dof) pair lanes: the host checks n_jpairs <= 64), but the body poses, the dof axes and h of every pair stay:
    // collision_phase reads them again after the QP (dropped contacts at the solution).  One pivot buffer (no look-ahead publishing).
    L.tgt = o;  o += lds_even(n_frame * 7 + n_com * 3);
    L.X = o;    o += x_sz;
    const int u0 = o;
    L.jnt = o;  o += jnt_sz;
    L.task = o; o += n_frame * 64;
    if (o - u0 < j_sz) o = u0 + j_sz;
    L.J = u0;
    L.dof = o;  o += lds_even(nv * 10);
    L.com = o;  o += (n_com > 0 ? nbody * 4 : 0);
    L.col = o;  o += max_rows * 16;
    L.A = o;    o += max_rows * a_stride_for(nv);
    L.piv = o;  o += kWoodRow + 2 * kMuBig;
    L.S = o;    o += lds_even(s_doubles);
    L.q2 = prefetch ? o : L.q;     o += prefetch ? lds_even(nq) : 0;
    L.tgt2 = prefetch ? o : L.tgt; o += prefetch ? lds_even(n_frame * 7 + n_com * 3) : 0;
    L.hsel = o; o += lds_even(n_hsel);
    L.total = o;
    return L;
  }
  // compact (3-waves-per-SIMD variants, no collision rows): ranges that are not alive at the same time share storage.
  //   direct start:   {body poses, joint axes}              | {staged Jacobian rows of one task, pivot buffers}
  //   low-rank start: {body poses, joint axes, task blocks} | {all Jacobian rows} — the pair lanes hold their entries in
  //                   registers until every lane has read its task block (wood_start); the pivot buffers stay apart
  //                   (they carry the published rows and 1/d_r of the elimination)
  const int task_sz = n_frame * 64;
  if (compact && wood) { L.tgt = o; o += lds_even(n_frame * 7 + n_com * 3); }
  const int u0 = o;
  L.X = o;    o += x_sz;                             // body poses, component-major: X[c][body] (c = x y z qw qx qy qz)
  L.jnt = o;  o += jnt_sz;
  if (compact && wood) {
    L.task = o; o += task_sz;
    if (o - u0 < j_sz) o = u0 + j_sz;
  } else {
    if (compact) { const int need = j_sz + 2 * kPivBuf; o = u0 + (x_sz + jnt_sz > need ? x_sz + jnt_sz : need); }
    L.tgt = o;  o += lds_even(n_frame * 7 + n_com * 3);
    L.task = o; o += task_sz;
  }
  // weighted Jacobian rows [r][j_stride]: the 6 rows of ONE task at a time (direct start, stride NT), or
  // every task row + one vector (low-rank start, stride NR)
  L.J = compact ? u0 : o;    o += compact ? 0 : j_sz;
  L.dof = o;  o += lds_even(nv * 10);
  L.com = o;  o += (n_com > 0 ? nbody * 4 : 0);
  L.col = o;  o += max_rows * 16;
  L.A = o;    o += max_rows * a_stride_for(nv);       // half-space rows A[s][0..stride)
  const bool piv_apart = !compact || wood;
  // two pivot column broadcast buffers (64 entries + 8 scalar slots of the pivot lane): look-ahead publishing.  (piv_small, the
  // F_COM builds with one more resident wave: a low-rank start never publishes ahead — one buffer for the QP, and the
  // elimination's published row + 1/d_r + ω_r = kWoodRow + 2·kMuBig doubles: 32 doubles less, the difference between 9 and 10
  // wavefronts per CU for the G1 full example — LDS is handed out in 1 280-byte granules on gfx950)
  L.piv = piv_apart ? o : u0 + j_sz;  o += piv_apart ? (piv_small ? kWoodRow + 2 * kMuBig : 2 * kPivBuf) : 0;
  L.S = o;    o += lds_even(s_doubles);   // low-rank start: columns of −Jh·Jhᵀ + right-hand sides
  // second buffers of the per-problem inputs: the next problem's q / targets are fetched straight into LDS
  // (global_load_lds) while the current problem is being solved
  // (only when the host found that they do not cost a resident wave: DeviceProblem::prefetch)
  L.q2 = prefetch ? o : L.q;     o += prefetch ? lds_even(nq) : 0;
  L.tgt2 = prefetch ? o : L.tgt; o += prefetch ? lds_even(n_frame * 7 + n_com * 3) : 0;
  // more collision pairs than tableau rows: h of EVERY pair, for the selection of the tightest rows and the check of the
  // dropped ones at the solution (collision_phase) — the ALOHA pair set of the reference is 1 104 pairs for 48 rows
  L.hsel = o; o += lds_even(n_hsel);
  L.total = o;
  return L;
}

// The layout of the four-waves product-form build (MKH_W4P: `44_32_r44_w4o`, one problem per workgroup, frame + posture tasks, one
// pass of pair lanes): 16 wavefronts per CU need ≤ 8 LDS granules of 1 280 B each, so EVERYTHING that is dead once the pair lanes
// hold their entries in registers — body poses, task blocks (in the joint axes' range: the dof lanes have read those before the
// task lanes write), dof stash, q and the targets — is one union with what lives after: the rows of Jh and, behind them, S.  (q
// and the targets are fetched again when a solve refactorises.)  One pivot range: the elimination's published row, 1/d_r and ω_r
// sized for kMu rows; the QP's scalar slots (sPiv + kWave) and the history's scalars (sPiv + kPivBuf, 2 per slot) reuse it.
template <class PT>
__host__ __device__ __forceinline__ LdsLayout build_lds_layout_w4p(const PT& P0, int nr) {
  LdsLayout L;
  const int n_mu = P0.n_jrows, sp = lds_even(n_mu);
  const int x_sz = 7 * lds_even(P0.nbody), jnt_sz = lds_even(P0.njnt * 6), task_sz = P0.n_frame * 64;
  int o = 0;
  L.X = o;    o += x_sz;
  L.jnt = o;  L.task = o;  o += jnt_sz > task_sz ? jnt_sz : task_sz;
  L.dof = o;  o += lds_even(P0.nv * 10);
  L.q = o;    o += lds_even(P0.nq);
  L.tgt = o;  o += lds_even(P0.n_frame * 7 + P0.n_com * 3);
  L.J = 0;
  L.S = lds_even((n_mu + 1) * nr);
  const int after = L.S + lds_even(n_mu * (sp + 1));
  if (o < after) o = after;
  L.com = o; L.col = o; L.A = o;
  L.piv = o;  o += kWoodRow + 2 * kMu;
  L.q2 = L.q; L.tgt2 = L.tgt; L.hsel = o;
  L.total = o;
  return L;
}

// Low-rank start: the n_mu × (sp + 1) block of −Jh·Jhᵀ and right-hand sides fits in the dof stash?
// (n_com_bodies: the subtree-CoM array that follows the dof stash — nbody when the problem has ComTasks, else 0)
__host__ __device__ inline bool wood_s_aliases_dof(int nv, int n_mu, int sp, int n_com_bodies = 0) {
  return n_mu * (sp + 1) <= lds_even(nv * 10) + n_com_bodies * 4;
}

// Compile-time feature set of a kernel variant (ik_kernel.h "the kernel" says what each bit builds).
enum : int { F_TAPS = 1, F_REL = 2, F_COM = 4, F_COLL = 8, F_STEPS = 16, F_ALL = 31, F_WOOD = 32, F_SIMPLE_COLL = 64, F_CONVEX_COLL = 128,
              F_DENSE = 256 };   // F_DENSE alone: the lean build of the plugin route (dense task / limit rows next to frame + posture tasks and box limits)

// The LDS layout of ONE BUILD (NT, NR, FEAT, one-more-wave map) for a descriptor P0: the kernel indexes it (kernel_lds_layout,
// with its compile-time constants) and the host reserves its `total` (problem_plan.hip lds_bytes_of) — one statement, so the two
// cannot disagree.  `prefetch` (second input buffers) and `compact` (the compact layout of a two-waves low-rank build) are the
// two choices the host tries both ways, 0 / 1, before it fixes them in the descriptor; kFromDescriptor: as fixed there — which
// of the descriptor's prefetch flags belongs to which layout is part of this statement (layout_prefetch).
// (The descriptor's fields are read in the order of lds_layout's arguments, the two choices included: the order of these scalar
//  loads decides the compiler's schedule of the kernels' prologues, and the device code is pinned by hash.)
constexpr int kFromDescriptor = -1;
template <class PT>
__host__ __device__ __forceinline__ bool layout_prefetch(const PT& P0, int feat, bool w3) {
  const bool wood = (feat & F_WOOD) != 0;
  const bool wood_rows = wood && (feat & (F_COLL | F_DENSE)) != 0;    // low-rank start with half-space rows: its own layout
  if (w3) return (wood ? P0.prefetch_w3w : P0.prefetch_w3) != 0;
  return ((wood_rows || (wood && P0.wood_compact != 0)) ? P0.prefetch_wc : P0.prefetch) != 0;
}
template <class PT>
__host__ __device__ __forceinline__ LdsLayout build_lds_layout(const PT& P0, int nt, int nr, int feat, bool w3, int prefetch = kFromDescriptor,
                                                               int compact = kFromDescriptor) {
  const bool wood = (feat & F_WOOD) != 0;
  const bool wood_rows = wood && (feat & (F_COLL | F_DENSE)) != 0;
  return lds_layout(P0.nq, P0.nv, P0.nbody, P0.njnt, P0.n_frame, P0.n_posture, P0.n_com, P0.max_rows,
                    wood ? P0.n_jrows + 1 : 6, wood ? nr : j_stride_direct(P0.nv, nt),
                    // the S block: in the dof stash where it fits — never with half-space rows (collision_phase reads the axes again after the QP)
                    (wood && (wood_rows || !wood_s_aliases_dof(P0.nv, P0.n_jrows, lds_even(P0.n_jrows), P0.n_com > 0 ? P0.nbody : 0)))
                        ? P0.n_jrows * (lds_even(P0.n_jrows) + 1) : 0,
                    prefetch < 0 ? layout_prefetch(P0, feat, w3) : prefetch != 0,
                    !wood_rows && (w3 || (wood && (compact < 0 ? P0.wood_compact != 0 : compact != 0))), wood,
                    (feat & F_COLL) ? P0.n_hsel : 0,        // (a compile-time 0 without collision rows: one value less to keep)
                    wood_rows || (w3 && wood && (feat & F_COM) != 0),   // (piv_small: ... and the F_COM builds with one more resident wave)
                    wood_rows);
}

}  // namespace mkh
