// tmf_check_kernel — the collision check of candidate tracking (include/minkhip.h "THE RULE, with a checker" of
// mkh_solve_trajectory_multistart): ONE launch behind the last loop of mkh_solve_trajectory_multistart_free, or over the caller's
// candidates in mkh_select_trajectory_candidates, judges every row (t, i) of the time-major (T, B·S, nq) candidates as a node and
// sweeps the motion into it from the same candidate's row (t − 1, i).
//
// One row per wavefront, or — a small arm — per 16-lane DPP row of it, four to a wavefront (launch_clearance's criterion,
// sweep_kernel's LDS slice).  The group walks 1 + M rows of q through ONE clr_row (clearance_row.h): row 0 is the node itself,
// copied into LDS as it stands; behind it the group knows the node's margin, ORs MKH_ST_IN_COLLISION into the status it read and
// evaluates eligible(t, i) from the flags in memory; only an eligible row with t >= 1 then walks the M interior samples of b ⊖ a
// (sweep_blend.h; formed once, in front of the loop), built in LDS and never written to memory, keeping the minimum on clr_key as sweep_kernel does —
// a strictly smaller key replacing it: the lowest sample of a tie, the first NaN.  A wavefront none of whose rows is swept leaves
// behind row 0.  One lane of the group writes the two margins and, for a row in collision, the status word: plain vector
// stores, no atomics, no scratch.
//
// A checker's general convex pairs: convex_check_kernel (convex_check.hip) runs in front on a chunk of rows and leaves their
// distances on the node and on every sample this kernel could read; tmf_check_cv_kernel then takes the chunk (a first-row offset
// into the call's rows) and clr_row reads them.
//
// dynamic LDS, per group: poses (7, nbody) | q(u) (nq) | a (nq) | b ⊖ a (nq) doubles
#include <hip/hip_runtime.h>

#include "checker_plan.h"
#include "clearance_row.h"
#include "lie_dev.h"
#include "outer_launch.h"
#include "sweep_blend.h"

namespace mkh {

// What the kernel reads of a launch (kernel arguments live in scalar registers across the whole sample loop: as few as it takes).
struct TmfKernelArgs {
  long long N, R;                  // rows of this launch (T·B·S, or a chunk of them), rows per waypoint B·S
  int32_t M;
  const double* q_all;             // (T, R, nq)
  const int32_t* converged;        // (T, R), or null: every row counts as converged
  int32_t* status;                 // (T, R): read, and MKH_ST_IN_COLLISION OR-ed into the rows in collision
  double *node_margin, *edge_margin;     // (T, R) each
};

// Whether any lane of this lane's group holds `x`.
template <int LPR>
__device__ __forceinline__ bool tmf_group_any(bool x, int grp) {
  const unsigned long long bb = __ballot(x);
  return (LPR == 64 ? bb : (bb >> (grp * LPR)) & ((1ull << (LPR & 63)) - 1ull)) != 0ull;
}

// CV: the build for a checker WITH general convex pairs (tmf_check_cv_kernel below) — a chunk of the call's rows (a.N of them
// from row c.first) and the distances convex_check_kernel left for the chunk, row j of a chunk's item its walk's row j.  Without:
// tmf_check_kernel, which reads neither and is the kernel it was.  (Pg without __restrict__ here: the kernels' parameter carries
// it, and a second one on the inlined body's changes what the compiler may reorder — tmf_check_kernel<64> then spilled 8 SGPRs.)
template <int LPR, bool CV>
__device__ __forceinline__ void tmf_check_body(const WideProblem* Pg, const TmfKernelArgs& a, const CvChunk& c) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int RPW = kWave / LPR;                             // rows per wavefront
  const WideProblem& P = *Pg;
  const int lane = lane_id(), sub = lane & (LPR - 1), grp = lane / LPR;
  const int nbody = P.nbody, nq = P.nq;
  const long long g_raw = (long long)blockIdx.x * RPW + grp;
  const bool live = g_raw < a.N;                               // (a row past the end repeats the last one and writes nothing)
  const long long g_in = live ? g_raw : a.N - 1, g = CV ? c.first + g_in : g_in;     // its place in this launch, and in the call
  const bool first = g < a.R;                                  // waypoint 0: the start edge is never swept
  const double* const pb = a.q_all + (size_t)g * nq;
  const double* const pa = first ? pb : pb - (size_t)a.R * nq;       // (a row of waypoint 0 walks its own node: every address is valid)
  int32_t st = a.status[g];
  // what is left of eligible(t, i) && t >= 1 once the node's verdict is known
  int32_t may_sweep = (live && !first && (a.converged ? a.converged[g] != 0 : true)) ? 1 : 0;
  // ---- where this group writes, per lane and in VECTOR registers from here on (sweep_kernel's idiom: with one row per wavefront
  // the addresses — and the row's flags — would sit in scalar registers across the sample loop, beside the checker's table
  // pointers)
  const bool writer = live && sub == 0;
  double* on = writer ? a.node_margin + g : nullptr;
  double* oe = writer ? a.edge_margin + g : nullptr;
  int32_t* os = writer ? a.status + g : nullptr;
  asm volatile("" : "+v"(on), "+v"(oe), "+v"(os), "+v"(st), "+v"(may_sweep));
  // (general convex pairs: the same treatment — the buffer and its width stay out of the loop's scalar registers)
  const double* cve = nullptr;
  int n_cv = 0;
  if constexpr (CV) {
    cve = c.cv + (size_t)g_in * (a.M + 1) * c.n_cv;
    n_cv = c.n_cv;
    asm volatile("" : "+v"(cve), "+v"(n_cv));
  }
  double* const sX = smem + (size_t)grp * (7 * nbody + 3 * nq);
  double *const sQ = sX + 7 * nbody, *const sA = sQ + nq, *const sD = sA + nq;
  // ---- a row with a NaN or an infinite entry: its node is NaN, and so is every sample of an edge that touches it
  bool bad_b = false, bad_a = false;
  for (int i = sub; i < nq; i += LPR) {
    bad_b = bad_b || !(pb[i] - pb[i] == 0.0);
    bad_a = bad_a || !(pa[i] - pa[i] == 0.0);
  }
  bad_b = tmf_group_any<LPR>(bad_b, grp);
  int32_t bad = (bad_b ? 1 : 0) | ((bad_b || tmf_group_any<LPR>(bad_a, grp)) ? 2 : 0);      // bit 0: the node, bit 1: the edge
  double node = __builtin_nan("");
  double edge = first ? __builtin_huge_val() : __builtin_nan("");    // (the start edge: +inf; an edge that is not swept: NaN)
  asm volatile("" : "+v"(bad), "+v"(edge));                    // (wave-uniform with one row per wavefront: see above)
  bool swept = false;
  unsigned long long best_key = ~0ull;                         // (above every key: sample 0 always enters)
  const double steps = (double)(a.M + 1);
  // ---- row 0, the node as it stands, and b ⊖ a of the edge into it.  The difference is formed HERE, in front of the loop and
  // for every row, not behind the node's verdict for the eligible ones only: inside the loop its quaternion arithmetic shares
  // the allocation of clr_row and the kernel took 230 / 192 vector registers (two waves per SIMD); in front of it 158 / 146
  // (three, sweep_kernel's).  What it costs a row that is then not swept is a subtraction per joint.
  for (int k = sub; k < nq; k += LPR) sQ[k] = pb[k];
  swp_difference<LPR>(P, pa, pb, sA, sD, sub);
  wave_sync();
  // (row 0 is told apart by a value the compiler cannot see through: a loop whose first trip is known to differ is peeled, and
  // clr_row — most of the kernel's code and registers — would be there twice)
  int row0 = 0;
  asm volatile("" : "+s"(row0));
#pragma unroll 1
  for (int i = 0; i <= a.M; ++i) {
    const ClrRow r = clr_row<LPR, CV ? 1 : 7>(P, sX, sQ, (bad & (i == row0 ? 1 : 2)) != 0, sub, grp, n_cv, cve, CV ? (size_t)i : 0, nullptr);
    wave_sync();                                               // (the next row's q(u) and poses overwrite what the pairs read)
    if (i == row0) {
      node = r.margin;
      const int32_t st1 = (node >= 0.0) ? st : (st | kStInCollision);
      swept = may_sweep != 0 && (st1 & ~1) == 0;               // eligible(t, i), t >= 1 (~1: MKH_ST_OUTSIDE_LIMITS is no failure)
      if (__ballot(swept) == 0ull) break;                      // (wave-uniform: a wavefront with nothing to sweep leaves here)
    } else {
      const unsigned long long key = clr_key(r.margin);
      if (swept && key < best_key) { best_key = key; edge = r.margin; }
    }
    swp_blend<LPR>(P, sA, sD, (double)(i + 1) / steps, sQ, sub);     // (sample i + 1 of M; behind the last one a row nobody reads)
    wave_sync();
  }
  if (on) *on = node;
  if (oe) *oe = edge;
  if (os && !(node >= 0.0)) *os = st | kStInCollision;
}

template <int LPR>
__global__ __launch_bounds__(64) void tmf_check_kernel(const WideProblem* __restrict__ Pg, const TmfKernelArgs a) {
  tmf_check_body<LPR, false>(Pg, a, CvChunk{});
}

template <int LPR>
__global__ __launch_bounds__(64) void tmf_check_cv_kernel(const WideProblem* __restrict__ Pg, const TmfKernelArgs a, const CvChunk c) {
  tmf_check_body<LPR, true>(Pg, a, c);
}

// edge_collision[b, t] = t >= 1 && swept && !(edge_margin >= 0) of the chosen candidate, through the (instance, waypoint) strides
// of the caller's layout, and their count per instance.  One thread per instance.
__global__ __launch_bounds__(256) void tmf_edge_flags_kernel(int B, int S, int T, const int32_t* __restrict__ seed_index,
                                                             const int32_t* __restrict__ converged_all,
                                                             const int32_t* __restrict__ status_all,
                                                             const double* __restrict__ edge_margin_all,
                                                             int32_t* __restrict__ edge_collision, long long o_sb, long long o_st,
                                                             int32_t* __restrict__ n_edge_collisions) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const size_t R = (size_t)B * S, i = (size_t)b * S + seed_index[b];
  int n = 0;
  for (int t = 0; t < T; ++t) {
    const size_t row = (size_t)t * R + i;
    const bool swept = t >= 1 && (!converged_all || converged_all[row] != 0) && (status_all[row] & ~1) == 0;
    const int c = (swept && !(edge_margin_all[row] >= 0.0)) ? 1 : 0;
    edge_collision[b * o_sb + t * o_st] = c;
    n += c;
  }
  n_edge_collisions[b] = n;
}

hipError_t launch_tmf_check(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, int B, int S, int T, int M,
                            const double* q_all, const int32_t* converged_all, int32_t* status_all, double* node_margin_all,
                            double* edge_margin_all, const CvChunk& chunk) {
  const bool quarter = checker_quarter(nbody, n_pairs);
  const size_t lds = sweep_lds_bytes(nbody, nq, n_pairs);
  const long long R = (long long)B * S, N = R * T;
  // (a chunk and the general convex pairs' distances come together or not at all)
  if ((chunk.cv != nullptr) != (chunk.n_cv > 0) || (chunk.cv != nullptr) != (chunk.count > 0) || chunk.first < 0 || chunk.count < 0 ||
      chunk.first + chunk.count > N)
    return hipErrorInvalidValue;
  const long long n = chunk.cv ? chunk.count : N, blocks = quarter ? (n + 3) / 4 : n;
  if (B < 1 || S < 1 || T < 1 || M < 1 || n_pairs < 1 || lds > 64 * 1024 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (!q_all || !status_all || !node_margin_all || !edge_margin_all) return hipErrorInvalidValue;
  const WideProblem* const P = (const WideProblem*)wide_problem;
  const TmfKernelArgs k{n, R, M, q_all, converged_all, status_all, node_margin_all, edge_margin_all};
  if (chunk.cv) {
    if (quarter)
      hipLaunchKernelGGL(tmf_check_cv_kernel<16>, dim3((unsigned)blocks), dim3(kWave), lds, stream, P, k, chunk);
    else
      hipLaunchKernelGGL(tmf_check_cv_kernel<64>, dim3((unsigned)blocks), dim3(kWave), lds, stream, P, k, chunk);
  } else if (quarter)
    hipLaunchKernelGGL(tmf_check_kernel<16>, dim3((unsigned)blocks), dim3(kWave), lds, stream, P, k);
  else
    hipLaunchKernelGGL(tmf_check_kernel<64>, dim3((unsigned)blocks), dim3(kWave), lds, stream, P, k);
  return hipGetLastError();
}

hipError_t launch_tmf_edge_flags(hipStream_t stream, int B, int S, int T, const int32_t* seed_index, const int32_t* converged_all,
                                 const int32_t* status_all, const double* edge_margin_all, int32_t* edge_collision, long long o_sb,
                                 long long o_st, int32_t* n_edge_collisions) {
  unsigned grid;
  if (B < 1 || !grid_1d(B, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tmf_edge_flags_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, B, S, T, seed_index, converged_all, status_all,
                     edge_margin_all, edge_collision, o_sb, o_st, n_edge_collisions);
  return hipGetLastError();
}

}  // namespace mkh
