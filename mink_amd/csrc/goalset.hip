// Goal sets (mkh_solve_goalset, mkh_select_goalset; include/minkhip.h "THE RULE OF THE GOAL SET"): the two-level selection
// behind multi-start's loops on the B·G flattened (target, goal) pairs — per goal the closest eligible seed, per target the
// reached goal with the smallest cost + distance.  One small kernel and its launcher (declared in outer_launch.h); the loops
// in front of it are mkh_solve_until's own launch: nothing here touches a solve kernel or its argument structs.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"
#include "ms_distance.h"
#include "outer_launch.h"
#include "wave_ops.h"

namespace mkh {

// One wavefront per target, its goals in turn.  Level 1 is multistart_select_kernel's body on the goal's S rows: lane l looks at
// seeds l, l + 64, ..., the wave agrees on the closest eligible one with the same two reductions, so a goal's row is bitwise
// what that kernel writes for the flattened pair.  Level 2 is a running best in wave-uniform registers.  A goal's row of q / v
// goes out with consecutive lanes on consecutive addresses; its scalars wait in lane g mod 64 and go out 64 goals at a time,
// lane l to goal g0 + l.  The candidates' rows are read from global memory where the loops left them, once.
// The optional arrays: without converged_all every candidate is eligible; status_all / iters_all / v_all and their outputs are
// absent for a selection over a caller's own candidates.
__global__ __launch_bounds__(64) void goalset_select_kernel(int B, int G, int S, int nq, int nv, int njnt,
                                                            const int32_t* __restrict__ jnt, const GsIn in, const GsOut o) {
#pragma clang fp contract(off)      // score = cost + d_ref: one rounded addition
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  const double* const ref = in.q_ref + (size_t)b * nq;
  constexpr unsigned kNone = 0xffffffffu;
  // level 2, wave-uniform
  double best_score = __builtin_huge_val();
  int best_g = -1, best_s = 0, first_valid = -1, n_reached = 0;
  // the scalars of goal g, held by lane g mod 64 until the flush
  double my_d = __builtin_huge_val();
  int my_seed = 0, my_reached = 0, my_nconv = 0, my_it = 0, my_st = 0;
  for (int g = 0; g < G; ++g) {
    const size_t r = (size_t)b * G + g, row0 = r * S;
    double best_d = __builtin_huge_val();
    unsigned best_seed = kNone, count = 0;
    for (int s = lane; s < S; s += 64) {
      const size_t i = row0 + s;
      if (in.converged_all && in.converged_all[i] == 0) continue;
      if (in.status_all && (in.status_all[i] & ~1) != 0) continue;           // (~1: MKH_ST_OUTSIDE_LIMITS is no failure)
      ++count;
      double d = ms_distance(jnt, njnt, in.q_all + i * nq, ref, in.weights);
      if (!(d >= 0.0) || d > 1.7976931348623157e308) d = 1.7976931348623157e308;   // (NaN / inf: last among the eligible)
      if (best_seed == kNone || d < best_d) { best_d = d; best_seed = (unsigned)s; }   // (ascending s: ties keep the lower index)
    }
    const unsigned long long cand = __ballot(best_seed != kNone);
    const double dmin = wave_min_nonneg(best_d, cand);
    const unsigned smin = wave_min_u32((best_seed != kNone && best_d == dmin) ? best_seed : kNone);
    const int n_conv = (int)wave_sum((double)count);
    const bool valid = !in.goal_valid || in.goal_valid[r] != 0;
    const bool reached = valid && cand != 0;
    const int pick = reached ? (int)smin : 0;              // an unreached goal: seed 0, the caller's own start
    const size_t ip = row0 + pick;
    for (int k = lane; k < nq; k += 64) o.q_goal[r * nq + k] = in.q_all[ip * nq + k];
    if (o.v_goal) for (int k = lane; k < nv; k += 64) o.v_goal[r * nv + k] = in.v_all[ip * nv + k];
    if (lane == (g & 63)) {
      my_seed = pick; my_reached = reached ? 1 : 0; my_nconv = n_conv;
      my_d = reached ? dmin : __builtin_huge_val();
      if (o.iters_goal) my_it = in.iters_all[ip];
      if (o.status_goal) my_st = in.status_all[ip];
    }
    if ((g & 63) == 63 || g == G - 1) {
      const int gl = (g & ~63) + lane;
      if (gl <= g) {
        const size_t rl = (size_t)b * G + gl;
        o.seed_index_goal[rl] = my_seed; o.reached[rl] = my_reached; o.n_converged_goal[rl] = my_nconv;
        o.distance_goal[rl] = my_d;
        if (o.iters_goal) o.iters_goal[rl] = my_it;
        if (o.status_goal) o.status_goal[rl] = my_st;
      }
    }
    if (valid && first_valid < 0) first_valid = g;
    if (reached) {
      ++n_reached;
      const double score = (in.goal_cost ? in.goal_cost[r] : 0.0) + dmin;
      if (score == score && (best_g < 0 || score < best_score)) {            // (a NaN score loses; ascending g: ties keep the lower index)
        best_score = score; best_g = g; best_s = pick;
      }
    }
  }
  // nothing chosen: seed 0 of the lowest valid goal, of goal 0 when none is valid
  const int g_row = best_g >= 0 ? best_g : (first_valid >= 0 ? first_valid : 0);
  const size_t ip = ((size_t)b * G + g_row) * S + best_s;
  for (int k = lane; k < nq; k += 64) o.q_best[(size_t)b * nq + k] = in.q_all[ip * nq + k];
  if (o.v_best) for (int k = lane; k < nv; k += 64) o.v_best[(size_t)b * nv + k] = in.v_all[ip * nv + k];
  if (lane == 0) {
    if (o.iters) o.iters[b] = in.iters_all[ip];
    if (o.status) o.status[b] = in.status_all[ip];
    o.converged[b] = best_g >= 0 ? 1 : 0;
    o.goal_index[b] = best_g >= 0 ? best_g : first_valid;
    o.seed_index[b] = best_s;
    o.n_reached[b] = n_reached;
    o.score[b] = best_g >= 0 ? best_score : __builtin_huge_val();
  }
}

hipError_t launch_gs_select(hipStream_t stream, int B, int G, int S, int nq, int nv, int njnt, const int32_t* jnt, const GsIn& in,
                            const GsOut& o) {
  if (B < 1 || G < 1 || S < 1 || (long long)B * G * S > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(goalset_select_kernel, dim3((unsigned)B), dim3(64), 0, stream, B, G, S, nq, nv, njnt, jnt, in, o);
  return hipGetLastError();
}

}  // namespace mkh
