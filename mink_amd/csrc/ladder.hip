// Ladder-graph trajectory IK (mkh_ladder_select, mkh_solve_trajectory_ladder; include/minkhip.h "THE RULE"): the dynamic program
// over the T rungs of S nodes of every instance, the back-trace, and the gather of the chosen nodes' rows — and their launchers
// (declared in outer_launch.h).  The rungs themselves are multi-start's (multistart.hip and the solve kernels); behind the gather
// sits trajectory.hip's waypoint velocity.  Nodes are batch-major: row (b·T + t)·S + s.  Nothing here touches a solve kernel.
// The checked calls (mkh_ladder_select_free, mkh_solve_trajectory_ladder_free; THE RULE "with a checker") run the same dynamic
// program on the mask of blocked edges that sweep.hip leaves: ladder_search_free_kernel, the MASK build of the one search body.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lie_dev.h"
#include "ms_distance.h"
#include "outer_launch.h"
#include "wave_ops.h"

namespace mkh {

constexpr int kLdDest = 64;             // destination nodes per pass: one per lane
constexpr int kLdIlp = 4;               // source nodes whose edge costs a lane accumulates side by side

// One wavefront per instance.  For every waypoint t the destinations are taken 64 at a time, lane = destination node s'; the
// sources (rung t − 1; for t = 0 the caller's posture alone) pass through LDS in tiles of TS nodes.  Both tiles are
// component-major: component a of the lane's destination at dq[a·64 + lane] — 32 consecutive doubles per half-wave, every bank
// once — and component a of source j at sq[a·TS + j], the same address in every lane: a broadcast.  The running keys of rung
// t − 1 and t sit in LDS too (every lane reads the source's key, a broadcast again): (lost << 16 | breaks) as one uint32 that
// compares like the pair, and the length.  A lane works out the costs of kLdIlp edges side by side (independent sums: the
// latency of one joint's table and LDS reads is paid once for all of them), then takes the sources in ascending s, replacing the
// best on a strictly smaller key, so a tie keeps the lowest s.  Back-pointers go to `pred` as bytes, the break bit of every
// node's best edge to `brk` as one ballot per pass; lane 0 finds the end node and walks back.
//
// dynamic LDS: dq (nq, 64) doubles | sq (nq, TS) doubles | lengths (2, S) doubles | weights (nv) doubles | counts (2, S) uint32 |
// joint table (njnt, 3) int32 | MASK: flags (TS, 64) bytes
//
// MASK (THE RULE "with a checker"): `blocked` (B, T, S, S) bytes, 1 where the edge from node (t − 1, s) to node (t, s') collides
// — byte ((b·T + t)·S + s')·S + s, so a destination's sources are consecutive.  The flags of a (destination pass, source tile)
// are staged in LDS beside the source tile, source-major: the flag of source j at fl[j·64 + lane], consecutive lanes consecutive
// bytes.  The destination's lost bit then depends on the source — lost(t, s') | blocked(t, s', s) — and enters the candidate's
// count inside the loop over the sources; without MASK it is added once behind it, as before.
template <bool MASK>
__device__ __forceinline__ void ladder_search_body(
    int B, int T, int S, int nq, int nv, int njnt, int TS, const int32_t* __restrict__ jnt, const double* __restrict__ q0,
    const double* __restrict__ q_nodes, const int32_t* __restrict__ tracked, const uint8_t* __restrict__ blocked,
    const double* __restrict__ weights, double max_step_sq, uint8_t* __restrict__ pred, unsigned long long* __restrict__ brk,
    int32_t* __restrict__ node_index, int32_t* __restrict__ n_tracked, int32_t* __restrict__ n_breaks, double* __restrict__ path_length,
    int32_t* __restrict__ edge_break, int32_t* __restrict__ edge_collision, int32_t* __restrict__ n_edge_collisions) {
#pragma clang fp contract(off)      // length: one rounded addition per edge, never fused into the distance
  extern __shared__ double ld_lds[];
  const int b = blockIdx.x;
  if (b >= B) return;
  const int lane = lane_id();
  double* const dq = ld_lds;
  double* const sq = dq + (size_t)nq * kLdDest;
  double* const klen = sq + (size_t)nq * TS;
  double* const wl = klen + 2 * (size_t)S;
  uint32_t* const kcnt = (uint32_t*)(wl + nv);
  int32_t* const jl = (int32_t*)(kcnt + 2 * (size_t)S);
  uint8_t* const fl = (uint8_t*)(jl + 3 * (size_t)njnt);                     // (MASK only)
  // the joint table and the weights (ones without) in LDS: every lane reads the same word — a broadcast, and a vector register
  // where a read from memory would hold scalar ones across the whole search
  for (int e = lane; e < 3 * njnt; e += 64) jl[e] = jnt[e];
  for (int e = lane; e < nv; e += 64) wl[e] = weights ? weights[e] : 1.0;
  const int nch = (S + kLdDest - 1) / kLdDest;
  constexpr double kMax = 1.7976931348623157e308;
  const double kInf = __builtin_huge_val();

  for (int t = 0; t < T; ++t) {
    const int cur = t & 1, prv = cur ^ 1;
    const size_t rung = ((size_t)b * T + t) * S;                             // first node row of rung t
    const double* const src_rung = t ? q_nodes + (rung - S) * nq : q0 + (size_t)b * nq;
    const int n_src = t ? S : 1;
    for (int c = 0; c < nch; ++c) {
      const int s1 = c * kLdDest + lane;
      const bool valid = s1 < S;
      const int n_dst = S - c * kLdDest < kLdDest ? S - c * kLdDest : kLdDest;
      __syncthreads();                // the previous pass has read both tiles
      for (int e = lane; e < n_dst * nq; e += 64) {
        const int j = e / nq, a = e - j * nq;
        dq[a * kLdDest + j] = q_nodes[(rung + (size_t)c * kLdDest) * nq + e];
      }
      uint32_t lost_dst = 0u;           // (MASK: the destination's own lost bit, known in front of the sources)
      if constexpr (MASK) lost_dst = (valid && tracked[rung + s1] == 0) ? 1u : 0u;
      uint32_t best_cnt = 0xffffffffu;  // (above every key: the first source always wins)
      double best_len = kInf;
      int best_s = 0;
      bool best_brk = false;
      for (int tile0 = 0; tile0 < n_src; tile0 += TS) {
        const int n_tile = n_src - tile0 < TS ? n_src - tile0 : TS;
        if (tile0) __syncthreads();   // the previous tile is consumed
        for (int e = lane; e < n_tile * nq; e += 64) {
          const int j = e / nq, a = e - j * nq;
          sq[a * TS + j] = src_rung[(size_t)tile0 * nq + e];
        }
        if constexpr (MASK) {
          // (e runs along a destination's sources, so the global reads are contiguous — the whole n_dst x n_tile block when the
          // tile is the rung — and the LDS byte stores of consecutive lanes lie 64 bytes apart: they share four banks.  The other
          // order would store contiguously and read memory at a stride of S bytes.  One byte per edge against the nq-term cost of
          // the same edge behind it: the staging was not measured apart from the call, profiles/r22_swept.txt has the call.)
          if (t)
            for (int e = lane; e < n_dst * n_tile; e += 64) {
              const int d = e / n_tile, j = e - d * n_tile;
              fl[j * kLdDest + d] = blocked[(rung + (size_t)c * kLdDest + d) * S + tile0 + j];
            }
        }
        __syncthreads();
        for (int j0 = 0; valid && j0 < n_tile; j0 += kLdIlp) {
          double d[kLdIlp];
          ms_distance_strided<kLdIlp>(jl, njnt, dq + lane, kLdDest, sq + j0, TS, n_tile - j0, wl, d);
#pragma unroll
          for (int k = 0; k < kLdIlp; ++k) {                                   // (ascending s: a tie keeps the lowest)
            if (j0 + k >= n_tile) break;
            const int s = tile0 + j0 + k;
            const double cost = (d[k] >= 0.0 && d[k] <= kMax) ? d[k] : kInf;
            const bool bk = t != 0 && cost > max_step_sq;                      // (the start edge is never a break)
            uint32_t cnt = (t ? kcnt[prv * S + s] : 0u) + (bk ? 1u : 0u);
            if constexpr (MASK) cnt += (lost_dst | (t ? (uint32_t)fl[(j0 + k) * kLdDest + lane] : 0u)) << 16;
            const double len = (t ? klen[prv * S + s] : 0.0) + cost;
            if (cnt < best_cnt || (cnt == best_cnt && len < best_len)) {
              best_cnt = cnt; best_len = len; best_s = s; best_brk = bk;
            }
          }
        }
      }
      if (valid) {
        uint32_t lost = 0u;
        if constexpr (!MASK) lost = tracked[rung + s1] == 0 ? 1u : 0u;
        kcnt[cur * S + s1] = best_cnt + (lost << 16);
        klen[cur * S + s1] = best_len;
        pred[rung + s1] = (uint8_t)best_s;
      }
      const unsigned long long mask = __ballot(valid && best_brk);
      if (lane == 0) brk[((size_t)b * T + t) * nch + c] = mask;
    }
  }
  __syncthreads();                    // rung T − 1's keys, and every back-pointer and break mask of this instance, are written
  if (lane != 0) return;
  const int last = (T - 1) & 1;
  uint32_t end_cnt = kcnt[last * S];
  double end_len = klen[last * S];
  int node = 0;
  for (int s = 1; s < S; ++s) {
    const uint32_t cnt = kcnt[last * S + s];
    const double len = klen[last * S + s];
    if (cnt < end_cnt || (cnt == end_cnt && len < end_len)) { end_cnt = cnt; end_len = len; node = s; }
  }
  n_tracked[b] = T - (int)(end_cnt >> 16);
  n_breaks[b] = (int)(end_cnt & 0xffffu);
  path_length[b] = end_len;
  int n_col = 0;
  for (int t = T - 1; t >= 0; --t) {
    const size_t row = (size_t)b * T + t;
    node_index[row] = node;
    edge_break[row] = (int32_t)((brk[row * nch + (node >> 6)] >> (node & 63)) & 1ull);
    const int from = pred[row * S + node];
    if constexpr (MASK) {
      const int col = t ? (int)blocked[(row * S + node) * S + from] : 0;
      edge_collision[row] = col;
      n_col += col;
    }
    node = from;
  }
  if constexpr (MASK) n_edge_collisions[b] = n_col;
}

__global__ __launch_bounds__(64) void ladder_search_kernel(
    int B, int T, int S, int nq, int nv, int njnt, int TS, const int32_t* __restrict__ jnt, const double* __restrict__ q0,
    const double* __restrict__ q_nodes, const int32_t* __restrict__ tracked, const double* __restrict__ weights,
    double max_step_sq, uint8_t* __restrict__ pred, unsigned long long* __restrict__ brk, int32_t* __restrict__ node_index,
    int32_t* __restrict__ n_tracked, int32_t* __restrict__ n_breaks, double* __restrict__ path_length,
    int32_t* __restrict__ edge_break) {
  ladder_search_body<false>(B, T, S, nq, nv, njnt, TS, jnt, q0, q_nodes, tracked, nullptr, weights, max_step_sq, pred, brk, node_index,
                            n_tracked, n_breaks, path_length, edge_break, nullptr, nullptr);
}

__global__ __launch_bounds__(64) void ladder_search_free_kernel(
    int B, int T, int S, int nq, int nv, int njnt, int TS, const int32_t* __restrict__ jnt, const double* __restrict__ q0,
    const double* __restrict__ q_nodes, const int32_t* __restrict__ tracked, const uint8_t* __restrict__ blocked,
    const double* __restrict__ weights, double max_step_sq, uint8_t* __restrict__ pred, unsigned long long* __restrict__ brk,
    int32_t* __restrict__ node_index, int32_t* __restrict__ n_tracked, int32_t* __restrict__ n_breaks, double* __restrict__ path_length,
    int32_t* __restrict__ edge_break, int32_t* __restrict__ edge_collision, int32_t* __restrict__ n_edge_collisions) {
  ladder_search_body<true>(B, T, S, nq, nv, njnt, TS, jnt, q0, q_nodes, tracked, blocked, weights, max_step_sq, pred, brk, node_index,
                           n_tracked, n_breaks, path_length, edge_break, edge_collision, n_edge_collisions);
}

// out[b, t, k] = all[b, t, node_index[b, t], k]: one thread per output element, k fastest.
template <class V>
__device__ __forceinline__ void ladder_gather(const V* __restrict__ all, V* __restrict__ out, const int32_t* __restrict__ node_index,
                                              long long total, int S, int W) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int k = (int)(e % W);
  const long long row = e / W;                               // b·T + t
  out[e] = all[(row * S + node_index[row]) * W + k];
}

__global__ __launch_bounds__(256) void ladder_gather_kernel(const double* __restrict__ all, double* __restrict__ out,
                                                            const int32_t* __restrict__ node_index, long long total, int S, int W) {
  ladder_gather(all, out, node_index, total, S, W);
}

__global__ __launch_bounds__(256) void ladder_gather_i32_kernel(const int32_t* __restrict__ all, int32_t* __restrict__ out,
                                                                const int32_t* __restrict__ node_index, long long total, int S) {
  ladder_gather(all, out, node_index, total, S, 1);
}

// tracked[i] = converged[i] != 0 && (status[i] & ~MKH_ST_OUTSIDE_LIMITS) == 0 over the B·T·S nodes.
__global__ __launch_bounds__(256) void ladder_tracked_kernel(const int32_t* __restrict__ converged, const int32_t* __restrict__ status,
                                                             long long total, int32_t* __restrict__ tracked) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  tracked[e] = (converged[e] != 0 && (status[e] & ~1) == 0) ? 1 : 0;
}

// The source tile of a search launch: the whole rung when it fits beside the destination tile and the keys in 64 KB of LDS, else
// the largest tile that does; 0 when not even one source node fits.
int ladder_source_tile(int S, int nq, int nv, int njnt, size_t* lds_bytes, bool mask) {
  const size_t fixed = (size_t)nq * kLdDest * sizeof(double) + 2 * (size_t)S * (sizeof(double) + sizeof(uint32_t)) +
                       (size_t)nv * sizeof(double) + 3 * (size_t)njnt * sizeof(int32_t);
  const size_t cap = 64u << 10, node = (size_t)nq * sizeof(double) + (mask ? kLdDest : 0);
  if (fixed + node > cap) return 0;
  size_t ts = (cap - fixed) / node;
  if (ts > (size_t)S) ts = (size_t)S;
  if (lds_bytes) *lds_bytes = fixed + ts * node;
  return (int)ts;
}

hipError_t launch_ladder_search(hipStream_t stream, int B, int T, int S, int nq, int nv, int njnt, const int32_t* jnt,
                                const double* q0, const double* q_nodes, const int32_t* tracked, const double* weights, double max_step_sq,
                                uint8_t* pred, unsigned long long* brk, int32_t* node_index, int32_t* n_tracked, int32_t* n_breaks,
                                double* path_length, int32_t* edge_break) {
  size_t lds = 0;
  const int TS = ladder_source_tile(S, nq, nv, njnt, &lds);
  if (B < 1 || T < 1 || S < 1 || S > 256 || T > 65535 || TS < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_search_kernel, dim3((unsigned)B), dim3(64), lds, stream, B, T, S, nq, nv, njnt, TS, jnt, q0, q_nodes, tracked,
                     weights, max_step_sq, pred, brk, node_index, n_tracked, n_breaks, path_length, edge_break);
  return hipGetLastError();
}

hipError_t launch_ladder_search_free(hipStream_t stream, int B, int T, int S, int nq, int nv, int njnt, const int32_t* jnt,
                                     const double* q0, const double* q_nodes, const int32_t* tracked, const uint8_t* blocked,
                                     const double* weights, double max_step_sq, uint8_t* pred, unsigned long long* brk,
                                     int32_t* node_index, int32_t* n_tracked, int32_t* n_breaks, double* path_length,
                                     int32_t* edge_break, int32_t* edge_collision, int32_t* n_edge_collisions) {
  size_t lds = 0;
  const int TS = ladder_source_tile(S, nq, nv, njnt, &lds, true);
  if (B < 1 || T < 1 || S < 1 || S > 256 || T > 65535 || TS < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_search_free_kernel, dim3((unsigned)B), dim3(64), lds, stream, B, T, S, nq, nv, njnt, TS, jnt, q0, q_nodes,
                     tracked, blocked, weights, max_step_sq, pred, brk, node_index, n_tracked, n_breaks, path_length, edge_break,
                     edge_collision, n_edge_collisions);
  return hipGetLastError();
}

hipError_t launch_ladder_gather(hipStream_t stream, const double* all, double* out, const int32_t* node_index, long long rows, int S,
                                int W) {
  const long long total = rows * W;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_gather_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, all, out, node_index, total, S, W);
  return hipGetLastError();
}

hipError_t launch_ladder_gather_i32(hipStream_t stream, const int32_t* all, int32_t* out, const int32_t* node_index, long long rows,
                                    int S) {
  if (rows == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(rows, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_gather_i32_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, all, out, node_index, rows, S);
  return hipGetLastError();
}

hipError_t launch_ladder_tracked(hipStream_t stream, const int32_t* converged, const int32_t* status, long long total,
                                 int32_t* tracked) {
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ladder_tracked_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, converged, status, total, tracked);
  return hipGetLastError();
}

}  // namespace mkh
