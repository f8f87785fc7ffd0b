// clearance_kernel — the clearance of a batch of configurations (include/minkhip.h "THE RULE OF CLEARANCE"): mkh_clearance, and the
// stage behind the loops of mkh_solve_multistart / mkh_solve_multistart_set / mkh_solve_goalset that marks the candidates whose
// final q is in collision (MKH_ST_IN_COLLISION).
//
// One row of q per wavefront, or — a small arm — per 16-lane DPP row of it, four to a wavefront.  The body poses of the row go into
// LDS level by level (mj_kinematics: the arithmetic of wide_kernel.h's FK and of convex_pre.hip's cv_chain_pose, so a pre-evaluated
// convex pair belongs to the same poses); the row's lanes then stride over the checker's pairs — bounding spheres first where the
// checker has cull records, the analytic routines of collide_dev.h behind them.  Pairs without an analytic routine are NOT
// evaluated here: convex_contacts_kernel runs in front (launch_convex_pre on the checker's own lists) and this kernel reads its
// (dist, from, to) records through cv_slot, as the analytic collision build of the solve kernel does.  The minimum over the pairs
// is an exact reduction of order-preserving integer keys (no rounding, ties to the lowest pair index); one lane writes the row's
// outputs.  No atomics, no scratch.
// The row body — FK, pair loop, key reduction — is clr_row of clearance_row.h, which sweep.hip runs on the samples of an edge.
#include <hip/hip_runtime.h>

#include "checker_plan.h"
#include "clearance_row.h"
#include "outer_launch.h"

namespace mkh {

// LPR lanes per row of q, 64 / LPR rows per wavefront: a small arm (a dozen bodies, a dozen pairs) fills a quarter of a wavefront,
// so four of its rows share one — each on its own DPP row, with its own slice of LDS.
template <int LPR>
__global__ __launch_bounds__(64) void clearance_kernel(const WideProblem* __restrict__ Pg, int n_cv, const double* __restrict__ cv, int N,
                                                       const double* __restrict__ q, double* __restrict__ margin, int32_t* __restrict__ pair,
                                                       int32_t* __restrict__ n_violated, double* __restrict__ distance,
                                                       int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int RPW = kWave / LPR;                             // rows per wavefront
  const WideProblem& P = *Pg;
  const int lane = lane_id(), sub = lane & (LPR - 1), grp = lane / LPR;
  const int nbody = P.nbody, n_pairs = P.n_pairs;
  const long long row_raw = (long long)blockIdx.x * RPW + grp;
  const bool live = row_raw < N;                               // (a row past the end repeats the last one and writes nothing)
  const int row = live ? (int)row_raw : N - 1;
  double* const sX = smem + (size_t)grp * 7 * nbody;           // this row's body poses, one array per component: x y z | w x y z
  const double* const sq = q + (size_t)row * P.nq;
  // ---- a row with a NaN or an infinite entry: every d_k is NaN
  bool bad_q = false;
  for (int i = sub; i < P.nq; i += LPR) bad_q = bad_q || !(sq[i] - sq[i] == 0.0);
  {
    const unsigned long long bb = __ballot(bad_q);
    bad_q = (LPR == 64 ? bb : (bb >> (grp * LPR)) & ((1ull << (LPR & 63)) - 1ull)) != 0ull;
  }
  const ClrRow r = clr_row<LPR>(P, sX, sq, bad_q, sub, grp, n_cv, cv, (size_t)row,
                                (distance && live) ? distance + (size_t)row * n_pairs : nullptr);
  if (sub == 0 && live) {
    if (margin) margin[row] = r.margin;
    if (pair) pair[row] = r.pair;
    if (n_violated) n_violated[row] = r.n_violated;
    if (status && !(r.margin >= 0.0)) status[row] |= kStInCollision;
  }
}

// `status` given: MKH_ST_IN_COLLISION OR-ed into the rows that are in collision (margin / pair / n_violated / distance may then be
// null).  `cv`: the (N, n_cv, 7) records of convex_contacts_kernel on the same rows.  At least one pair.
hipError_t launch_clearance(hipStream_t stream, const void* wide_problem, int nbody, int n_pairs, int n_cv, const double* cv, int N,
                            const double* q, double* margin, int32_t* pair, int32_t* n_violated, double* distance, int32_t* status) {
  const bool quarter = checker_quarter(nbody, n_pairs);        // (four rows per wavefront or one, and their poses in LDS: checker_plan.h)
  const size_t lds = clearance_lds_bytes(nbody, n_pairs);
  if (N < 1 || n_pairs < 1 || lds > 64 * 1024) return hipErrorInvalidValue;
  const WideProblem* const P = (const WideProblem*)wide_problem;
  if (quarter)
    hipLaunchKernelGGL(clearance_kernel<16>, dim3((unsigned)((N + 3) / 4)), dim3(kWave), lds, stream, P, n_cv, cv, N, q, margin, pair,
                       n_violated, distance, status);
  else
    hipLaunchKernelGGL(clearance_kernel<64>, dim3((unsigned)N), dim3(kWave), lds, stream, P, n_cv, cv, N, q, margin, pair, n_violated,
                       distance, status);
  return hipGetLastError();
}

}  // namespace mkh
