// Seed tables (mkh_seed_table_*, include/minkhip.h): stored postures keyed on the world poses their frame-task frames reach, and
// the exact K-nearest query that multi-start runs in front of its seed kernel.  The entries are drawn by multi-start's own seed
// kernel and keyed by mkh_eval's frame_pose tap (minkhip.hip drives both); what lives here is the key layout and the scan.
// Nothing here touches a solve kernel or its argument structs.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "outer_launch.h"
#include "wave_ops.h"

namespace mkh {

// keys (n_frame·7, N): component r = 7·f + c of entry j at keys[r·N + j] — lanes that walk consecutive entries read consecutive
// addresses.  One thread per element of the (n, n_frame·7) poses of a chunk that starts at entry j0; consecutive threads write
// consecutive entries.
__global__ __launch_bounds__(256) void seed_table_keys_kernel(const double* __restrict__ poses, long long total, int n, int rows,
                                                              long long N, long long j0, double* __restrict__ keys) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int i = (int)(e % n);
  const int r = (int)(e / n);
  keys[(size_t)r * N + j0 + i] = poses[(size_t)i * rows + r];
}

constexpr int kStTargetRec = 8;         // doubles of a target's record per frame in LDS: x y z, w x y z, squared norm

// One wavefront per target, kStWaves... blockDim.x / 64 targets per workgroup.  The workgroup streams the table through LDS in
// tiles of 2^te_shift entries: a tile is read from memory once and serves every target of the workgroup.  Lane l of a wave
// looks at entry (64·k + l) of the tile; the wave keeps its target's K best (d, j) as a sorted list in LDS, tests the 64
// candidates against the list's last distance with one ballot and inserts only the lanes that pass, in ascending j — entries
// arrive in ascending j, so a tie with a listed distance goes behind it and the rule "smallest (d, j)" needs no index compare.
//
// dynamic LDS: tile (n_frame·7, TE) doubles | targets (waves, n_frame, 8) doubles | list distances (waves, K) doubles | list
// indices (waves, K) int32
__global__ __launch_bounds__(1024) void seed_table_query_kernel(const double* __restrict__ keys, const double* __restrict__ q_tab,
                                                                const double* __restrict__ weights, int N, int n_frame, int nq,
                                                                int B, const double* __restrict__ targets, int K, int te_shift,
                                                                int32_t* __restrict__ index_out, double* __restrict__ dist_out,
                                                                double* __restrict__ seeds_out) {
#pragma clang fp contract(off)      // the metric rounds like its numpy restatement: products, then sums, in the stated order
  extern __shared__ double st_lds[];
  const int waves = (int)(blockDim.x >> 6), wave = (int)(threadIdx.x >> 6), lane = lane_id();
  const int TE = 1 << te_shift, rows = n_frame * 7;
  double* const tile = st_lds;
  double* const tg = tile + (size_t)rows * TE + (size_t)wave * n_frame * kStTargetRec;
  double* const ld = tile + (size_t)rows * TE + (size_t)waves * n_frame * kStTargetRec + (size_t)wave * K;
  int32_t* const li = (int32_t*)(tile + (size_t)rows * TE + (size_t)waves * n_frame * kStTargetRec + (size_t)waves * K) + (size_t)wave * K;
  const int b = (int)blockIdx.x * waves + wave;
  const bool live = b < B;            // (a wave without a target still loads tiles and meets the barriers)
  constexpr double kLast = 1.7976931348623157e308;
  if (live)
    for (int f = lane; f < n_frame; f += 64) {
      const double* const T = targets + ((size_t)b * n_frame + f) * 7;
      const double w = T[0], x = T[1], y = T[2], z = T[3];
      double* const rec = tg + f * kStTargetRec;
      rec[0] = T[4]; rec[1] = T[5]; rec[2] = T[6];
      rec[3] = w; rec[4] = x; rec[5] = y; rec[6] = z;
      rec[7] = ((w * w + x * x) + y * y) + z * z;
    }
  int cnt = 0;
  double thr = __builtin_huge_val();
  for (int tile0 = 0; tile0 < N; tile0 += TE) {
    __syncthreads();                  // the previous tile is consumed (first pass: the targets' records are written)
    for (int idx = (int)threadIdx.x; idx < rows * TE; idx += (int)blockDim.x) {
      const int r = idx >> te_shift, j = tile0 + (idx & (TE - 1));
      tile[idx] = j < N ? keys[(size_t)r * N + j] : 0.0;
    }
    __syncthreads();
    if (!live) continue;
    for (int sub = 0; sub < TE && tile0 + sub < N; sub += 64) {
      const int e = sub + lane, j = tile0 + e;
      const bool valid = e < TE && j < N;
      double d = 0.0;
      if (valid) {
        for (int f = 0; f < n_frame; ++f) {
          const double* const rec = tg + f * kStTargetRec;
          const double* const k = tile + (size_t)(7 * f) * TE + e;
          const double ew = k[0], ex = k[TE], ey = k[2 * TE], ez = k[3 * TE];
          const double dx = k[4 * TE] - rec[0], dy = k[5 * TE] - rec[1], dz = k[6 * TE] - rec[2];
          const double ne = ((ew * ew + ex * ex) + ey * ey) + ez * ez;
          const double c = (((rec[3] * ew + rec[4] * ex) + rec[5] * ey) + rec[6] * ez) / sqrt(rec[7] * ne);
          double o = 4.0 * (1.0 - c * c);
          o = o < 0.0 ? 0.0 : o;      // (a NaN stays a NaN: it is sorted last below)
          d = d + (weights[f] * ((dx * dx + dy * dy) + dz * dz) + weights[n_frame + f] * o);
        }
        if (!(d >= 0.0) || d > kLast) d = kLast;      // (NaN / inf: last, as in multistart_select_kernel)
      }
      unsigned long long mask = __ballot(valid && (cnt < K || d < thr));
      while (mask) {
        const int l = (int)__builtin_ctzll(mask);
        const double dl = readlane_f64(d, l);
        const int jl = tile0 + sub + l;
        // where it goes: behind every listed distance <= dl
        int pos = 0;
        for (int c0 = 0; c0 < cnt; c0 += 64) {
          const int i = c0 + lane;
          pos += (int)__builtin_popcountll(__ballot(i < cnt && ld[i] <= dl));
        }
        // [pos, last) moves up by one (a full list drops its last element): every read, then every write
        const int last = cnt < K ? cnt : K - 1;
        double rd[4];
        int32_t ri[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = c * 64 + lane;
          rd[c] = 0.0; ri[c] = 0;
          if (i >= pos && i < last) { rd[c] = ld[i]; ri[c] = li[i]; }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = c * 64 + lane;
          if (i >= pos && i < last) { ld[i + 1] = rd[c]; li[i + 1] = ri[c]; }
        }
        if (lane == 0) { ld[pos] = dl; li[pos] = jl; }
        __builtin_amdgcn_wave_barrier();
        if (cnt < K) ++cnt;
        mask &= mask - 1;
        if (cnt == K) {
          thr = ld[K - 1];
          mask &= __ballot(d < thr);
        }
      }
    }
  }
  if (!live) return;
  for (int i = lane; i < cnt; i += 64) {
    if (index_out) index_out[(size_t)b * K + i] = li[i];
    if (dist_out) dist_out[(size_t)b * K + i] = ld[i];
  }
  if (seeds_out)
    for (int e = lane; e < cnt * nq; e += 64) {
      const int i = e / nq, a = e - i * nq;
      seeds_out[((size_t)b * (K + 1) + 1 + i) * nq + a] = q_tab[(size_t)li[i] * nq + a];
    }
}

hipError_t launch_st_keys(hipStream_t stream, const double* poses, int n, int n_frame, long long N, long long j0, double* keys) {
  const long long total = (long long)n * n_frame * 7;
  if (total == 0) return hipSuccess;
  unsigned grid;
  if (!grid_1d(total, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seed_table_keys_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, poses, total, n, n_frame * 7, N, j0, keys);
  return hipGetLastError();
}

// The shape of a query launch: the most targets per workgroup (16, 8 or 4 wavefronts) and the largest tile (256 … 32 entries)
// whose LDS stays within 64 KB — a bigger tile means fewer barriers, more targets per workgroup mean fewer passes over the table.
hipError_t launch_st_query(hipStream_t stream, const double* keys, const double* q_tab, const double* weights, int N, int n_frame,
                           int nq, int B, const double* targets, int K, int32_t* index_out, double* dist_out, double* seeds_out) {
  if (B < 1 || N < 1 || n_frame < 1 || K < 1 || K > 255 || K > N) return hipErrorInvalidValue;
  int waves = 16, te_shift = n_frame <= 2 ? 8 : (n_frame <= 4 ? 7 : 6);
  auto lds = [&]() {
    const size_t doubles = (size_t)n_frame * 7 * ((size_t)1 << te_shift) + (size_t)waves * n_frame * kStTargetRec + (size_t)waves * K;
    return doubles * sizeof(double) + (size_t)waves * K * sizeof(int32_t);
  };
  while (lds() > (64u << 10)) {
    if (waves > 4) waves /= 2;
    else if (te_shift > 5) --te_shift;
    else return hipErrorInvalidValue;
  }
  const unsigned grid = (unsigned)((B + waves - 1) / waves);
  hipLaunchKernelGGL(seed_table_query_kernel, dim3(grid), dim3(64 * waves), lds(), stream, keys, q_tab, weights, N, n_frame, nq, B,
                     targets, K, te_shift, index_out, dist_out, seeds_out);
  return hipGetLastError();
}

}  // namespace mkh
