// The ladder on deduplicated nodes (mkh_solve_trajectory_ladder_nodes; include/minkhip.h): the one kernel between the
// distinct-set selection of a chunk of rungs (solution_set.hip) and the search (ladder.hip) — the flags of the (rung, slot)
// nodes.  Its launcher is declared in outer_launch.h; nothing here touches a solve kernel or its argument structs.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "outer_launch.h"

namespace mkh {

// One thread per node (rung r, slot j).  A filled slot (seed_index >= 0) is a tracked node and carries its candidate's
// converged flag; an empty slot is not tracked and carries candidate 0's flag, as it carries candidate 0's row.
__global__ __launch_bounds__(kOuterBlock) void ladder_nodes_flags_kernel(long long rungs, int S, int K,
                                                                          const int32_t* __restrict__ converged_all,
                                                                          const int32_t* __restrict__ seed_index,
                                                                          int32_t* __restrict__ tracked,
                                                                          int32_t* __restrict__ converged) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= rungs * K) return;
  const long long r = e / K;
  const int s = seed_index[e];
  const bool filled = s >= 0 && s < S;
  tracked[e] = filled ? 1 : 0;
  converged[e] = converged_all[r * S + (filled ? s : 0)];
}

hipError_t launch_ladder_nodes_flags(hipStream_t stream, long long rungs, int S, int K, const int32_t* converged_all,
                                     const int32_t* seed_index, int32_t* tracked, int32_t* converged) {
  unsigned grid;
  if (rungs < 1 || S < 1 || K < 1 || !grid_1d(rungs * K, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_nodes_flags_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, rungs, S, K, converged_all, seed_index,
                     tracked, converged);
  return hipGetLastError();
}

}  // namespace mkh
