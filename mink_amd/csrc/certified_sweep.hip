// certified_sweep_kernel — joint-space edges swept at a sample count chosen from a bound on their motion, with a proof that the
// space between the samples is free (include/minkhip.h "THE RULE OF THE CERTIFIED SWEEP"): mkh_certified_sweep.
//
// sweep_kernel's geometry (sweep.hip): one edge per wavefront, or — a small arm — per 16-lane DPP row of it, four to a wavefront.
// The group forms b ⊖ a once (swp_difference), reads the edge's joint weights off it and lets its lanes stride the checker's
// pairs for L_k = Σ_j coef·weight (the reach table of motion_bound.h), kept in LDS — divided by M + 1 once the largest L_k has given
// the sample count M: what a pair's cones drop over one segment.  The walk over the M + 2 points u_i = i / (M + 1), both ends included, is the sweep's: q(u) by swp_blend, the point's clearance by
// clr_row, whose distance row is the group's own LDS row — so a sample is the clearance of its row, bit for bit.  Beside the
// running minimum of the margins every lane keeps the lowest crossing point of the two cones of its pairs, ½·((m_i + m_{i+1}) −
// L_k / (M + 1)), from the previous point's margins in a second LDS row; both minima live on exact integer keys, the lanes'
// bounds are reduced once behind the walk.  No atomics, no scratch.  The groups of a wavefront have different M: the wavefront
// walks to the largest (clr_row synchronises the wave), and a group past its own count evaluates its last point again and keeps
// nothing.
//
// dynamic LDS, per group: poses (7, nbody) | q(u) (nq) | a (nq) | b ⊖ a (nq) | L (n_pairs) | margins of the previous point (n_pairs) |
// distances of this point (n_pairs) doubles
#include <hip/hip_runtime.h>

#include "checker_plan.h"
#include "clearance_row.h"
#include "lie_dev.h"
#include "outer_launch.h"
#include "sweep_blend.h"
#include "sweep_edge.h"

namespace mkh {

// What the motion of the edge's joints can add to the distance of pair k: row `c` of the reach table against the weights of b ⊖ a
// in sD.  A weight of 0 contributes 0 whatever its coefficient (an infinite one included).
__device__ __forceinline__ double cert_pair_motion(const WideProblem& P, const double* __restrict__ c, const double* const sD) {
#pragma clang fp contract(off)
  double L = 0.0;
  for (int j = 0; j < P.njnt; ++j) {
    const int jt = P.jnt_type[j], qa = P.jnt_qadr[j];
    double lin = 0.0, rot = 0.0;
    if (jt == JNT_HINGE) rot = fabs(sD[qa]);
    else if (jt == JNT_SLIDE) lin = fabs(sD[qa]);
    else if (jt == JNT_BALL) rot = sD[qa + 3];
    else {
      lin = sqrt(sD[qa] * sD[qa] + sD[qa + 1] * sD[qa + 1] + sD[qa + 2] * sD[qa + 2]);
      rot = sD[qa + 6];
    }
    if (lin > 0.0) L += c[2 * j] * lin;
    if (rot > 0.0) L += c[2 * j + 1] * rot;
  }
  return L;
}

// The crossing point of the two cones over one segment.
__device__ __forceinline__ double cert_cone(double m0, double m1, double drop) {
#pragma clang fp contract(off)
  return 0.5 * ((m0 + m1) - drop);
}

// Maximum of non-negative doubles (+inf allowed) over the lanes of a group, exactly, in every lane of it.
template <int LPR>
__device__ __forceinline__ double cert_max_nonneg(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  const unsigned h = (unsigned)(b >> 32), l = (unsigned)b;
  const unsigned mh = ~clr_min_u32<LPR>(~h);
  const unsigned ml = ~clr_min_u32<LPR>(h == mh ? ~l : 0xffffffffu);
  return __longlong_as_double((long long)(((unsigned long long)mh << 32) | ml));
}

template <int LPR>
__device__ __forceinline__ bool cert_any(bool x, int grp) {
  const unsigned long long bb = __ballot(x);
  return (LPR == 64 ? bb : (bb >> (grp * LPR)) & ((1ull << (LPR & 63)) - 1ull)) != 0ull;
}

// The kernel's second argument as it lies in the kernel-argument segment: behind the descriptor pointer, at its own alignment
// (the code object's metadata states the same offsets: .args of certified_sweep_kernel, offset 0 size 8, offset 8 size 128).
static_assert(alignof(CertifiedArgs) == sizeof(void*) && sizeof(CertifiedArgs) == 184 && offsetof(CertifiedArgs, mode) == 128,
              "cert_args: the second kernel argument at offset 8, the modes' fields behind the ten outputs");
__device__ __forceinline__ const CertifiedArgs& cert_args() {
  return *reinterpret_cast<const CertifiedArgs*>((const char*)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(void*));   // (the cast leaves address space 4)
}

// Where a writing lane of a graph build writes and what it knows of its edge, in ONE 64-bit vector register across the walk: the
// output index (below 2^31: the entry points refuse more edges), kCertSwept where the edge is swept, kCertFirst at waypoint 0 of
// a path; −1: the lane writes nothing.
constexpr long long kCertSwept = 1ll << 40, kCertFirst = 1ll << 41, kCertIndex = kCertSwept - 1;

// MODE: kSweepPairs — mkh_certified_sweep, the kernel it was, which reads none of the modes' fields — or a graph build, whose
// edges and output places are sweep_edge.h's (kSweepLadder: every edge of a ladder; kSweepPath: the edges of a chosen path).
template <int LPR, int MODE>
__global__ __launch_bounds__(64) void certified_sweep_kernel(const WideProblem* __restrict__ Pg, const CertifiedArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int RPW = kWave / LPR;                             // edges per wavefront
  constexpr bool kGraph = MODE != kSweepPairs;
  const WideProblem& P = *Pg;
  const int lane = lane_id(), sub = lane & (LPR - 1), grp = lane / LPR;
  const int nbody = P.nbody, nq = P.nq, n_pairs = P.n_pairs;
  const long long e_raw = (long long)blockIdx.x * RPW + grp;
  const bool live = e_raw < a.N;                               // (an edge past the end repeats the last one and writes nothing)
  const long long e = live ? e_raw : a.N - 1;
  // ---- whether this lane writes, and where: the edge index alone, in a vector register from here on.  The ten output pointers
  // are read from the kernel-argument segment behind the walk (cert_args below): as kernel arguments they would sit in twenty
  // scalar registers across the whole walk beside the checker's two dozen table pointers, parked in vector registers as
  // sweep_body parks its four they cost twenty of those — 188 instead of 168, two waves per SIMD instead of the sweep's three.
  const double *pa, *pb;
  long long eo;
  bool swept = true;
  if constexpr (kGraph) {
    const SweepKernelArgs k{MODE, 0, a.T, a.W, a.N, a.nodes, nullptr, const_cast<int32_t*>(a.tracked), const_cast<int32_t*>(a.node_index),
                            nullptr, nullptr, 0, nullptr, 0};
    const SweepEdge g = swp_edge(k, e, nq);
    pa = g.pa; pb = g.pb;
    swept = g.swept && live;
    eo = (live && sub == 0) ? (g.eo | (g.swept ? kCertSwept : 0) | (g.idle > 0.0 ? kCertFirst : 0)) : -1;       // (idle: NaN, or +inf at waypoint 0)
  } else {
    pa = a.from + (size_t)e * nq; pb = a.to + (size_t)e * nq;
    eo = (live && sub == 0) ? e : -1;
  }
  asm volatile("" : "+v"(eo));
  ClrRow best{0.0, 0, 0};                                      // (n_violated: the sample index here)
  double bound = 0.0, motion = 0.0;
  int bound_seg = 0, bound_k = 0, M = 1, cap = 0;
  // (a graph build: a wavefront none of whose groups sweeps leaves here, for the idle values at the end)
  if (!kGraph || __ballot(swept) != 0ull) {
  double* const sX = smem + (size_t)grp * (7 * nbody + 3 * nq + 3 * n_pairs);
  double *const sQ = sX + 7 * nbody, *const sA = sQ + nq, *const sD = sA + nq;
  double *const sL = sD + nq, *const sP = sL + n_pairs, *const sC = sP + n_pairs;
  // ---- an end with a NaN or an infinite entry; a limited slide joint outside its range at either end (D presumes the range)
  bool bad = false, outside = false;
  for (int i = sub; i < nq; i += LPR) bad = bad || !(pa[i] - pa[i] == 0.0) || !(pb[i] - pb[i] == 0.0);
  for (int j = sub; j < P.njnt; j += LPR)
    if (P.jnt_type[j] == JNT_SLIDE) {
      const int qa = P.jnt_qadr[j], dd = P.jnt_dadr[j];
      const double lo = P.dof_lo[dd], hi = P.dof_hi[dd];
      outside = outside || pa[qa] < lo || pa[qa] > hi || pb[qa] < lo || pb[qa] > hi;
    }
  bad = cert_any<LPR>(bad, grp);
  outside = cert_any<LPR>(outside, grp);
  swp_difference<LPR>(P, pa, pb, sA, sD, sub);
  wave_sync();
  // ---- L_k, the group's lanes striding the pairs; motion = the largest
  for (int k = sub; k < n_pairs; k += LPR) {
    const double L = cert_pair_motion(P, a.reach + (size_t)k * P.njnt * 2, sD);
    sL[k] = L;
    motion = fmax(motion, L);
  }
  motion = cert_max_nonneg<LPR>(motion);
  // ---- the sample count
  const bool unbounded = !(motion < __builtin_huge_val()) || outside;
  const double want = ceil(motion / a.resolution) - 1.0;
  const bool capped = want > (double)a.max_samples;
  M = (unbounded || capped) ? a.max_samples : (want < 1.0 ? 1 : (int)want);
  if (bad) M = 1;
  if (kGraph && !swept) M = 1;                                 // (an idle group walks its own node and does not lengthen the walk)
  int Mmax = M;                                                // (the wavefront walks to its largest count)
  if constexpr (LPR != 64) {
    const int m0 = __builtin_amdgcn_readlane(M, 0), m1 = __builtin_amdgcn_readlane(M, 16);
    const int m2 = __builtin_amdgcn_readlane(M, 32), m3 = __builtin_amdgcn_readlane(M, 48);
    Mmax = max(max(m0, m1), max(m2, m3));
  } else {
    Mmax = __builtin_amdgcn_readfirstlane(M);
  }
  // ---- the M + 2 points
  unsigned long long best_key = ~0ull, bound_key = ~0ull;      // (above every key: point 0 and segment 0 always enter)
  const double steps = (double)(M + 1);
  for (int k = sub; k < n_pairs; k += LPR) sL[k] = sL[k] / steps;          // (L_k / (M + 1): what a pair's cones drop over one segment)
  for (int i = 0; i <= Mmax + 1; ++i) {
    const bool mine = i <= M + 1;
    swp_blend<LPR>(P, sA, sD, (double)(mine ? i : M + 1) / steps, sQ, sub);
    wave_sync();
    const ClrRow r = clr_row<LPR>(P, sX, sQ, bad, sub, grp, 0, nullptr, 0, sC);
    const unsigned long long key = clr_key(r.margin);
    if (mine && key < best_key) { best_key = key; best = ClrRow{r.margin, r.pair, i}; }
    wave_sync();
    // the segment that ends here, on the lanes that evaluated its pairs (ascending segments, ascending pairs: a strict < keeps the
    // lowest segment, then the lowest pair, of a lane's ties)
    for (int k = sub; k < n_pairs; k += LPR) {
      const double m = (sC[k] - P.pairs[k].dmin) + 0.0;
      if (mine && i > 0) {
        const double v = cert_cone(sP[k], m, sL[k]);
        const unsigned long long vk = clr_key(v);
        if (vk < bound_key) { bound_key = vk; bound = v; bound_seg = i - 1; bound_k = k; }
      }
      sP[k] = m;
    }
    wave_sync();                                               // (the next point's q(u) and poses overwrite what the pairs read)
  }
  // ---- the lowest bound over the group's lanes, exactly: high words, low words among their ties, then segment, then pair
  {
    const unsigned kh = (unsigned)(bound_key >> 32), kl = (unsigned)bound_key;
    const unsigned mh = clr_min_u32<LPR>(kh);
    const unsigned ml = clr_min_u32<LPR>(kh == mh ? kl : 0xffffffffu);
    const bool tie = kh == mh && kl == ml;
    const unsigned smin = clr_min_u32<LPR>(tie ? (unsigned)bound_seg : 0xffffffffu);
    const unsigned kmin = clr_min_u32<LPR>((tie && (unsigned)bound_seg == smin) ? (unsigned)bound_k : 0xffffffffu);
    bound = bperm_f64(bound, grp * LPR + (int)(kmin & (LPR - 1)));        // (the lane of the group that holds pair kmin)
    bound_seg = (int)smin;
    bound_k = (int)kmin;
  }
  if (unbounded) { bound = -__builtin_huge_val(); bound_seg = 0; bound_k = 0; }
  cap = capped ? 1 : 0;
  if (bad) {
    best = ClrRow{__builtin_nan(""), 0, 0};
    bound = motion = __builtin_nan("");
    bound_seg = bound_k = cap = 0;
  }
  }
  if (eo >= 0) {                                               // (one lane of a live group)
    const CertifiedArgs& o = cert_args();
    const int verdict = !(best.margin >= 0.0) ? 2 : (bound >= 0.0 ? 1 : 0);
    if constexpr (!kGraph) {
      o.margin[eo] = best.margin; o.lower_bound[eo] = bound; o.motion[eo] = motion;
      o.sample[eo] = best.n_violated; o.pair[eo] = best.pair; o.segment[eo] = bound_seg; o.bound_pair[eo] = bound_k;
      o.n_samples[eo] = M; o.capped[eo] = cap;
      o.verdict[eo] = verdict;
    } else {
      // (an edge that is not swept kept nothing of its walk: the idle values — +inf at waypoint 0 of a path, else NaN)
      const bool did = (eo & kCertSwept) != 0;
      const long long at = eo & kCertIndex;
      const double idle = (eo & kCertFirst) ? __builtin_huge_val() : __builtin_nan("");
      if constexpr (MODE == kSweepLadder) {
        o.blocked[at] = (did && (o.policy == MKH_EDGE_REQUIRE_CERTIFIED ? verdict != MKH_SWEEP_CERTIFIED : verdict == MKH_SWEEP_COLLIDES)) ? 1 : 0;
        if (o.margin) o.margin[at] = did ? best.margin : idle;
        if (o.verdict_all) o.verdict_all[at] = did ? (int8_t)verdict : (int8_t)-1;
      } else {
        o.margin[at] = did ? best.margin : idle; o.lower_bound[at] = did ? bound : idle;
        o.n_samples[at] = did ? M : 0; o.verdict[at] = did ? verdict : -1;
      }
    }
  }
}

// n_certified of a chosen path: one thread per instance over its T verdicts (entry 0 is −1)
__global__ __launch_bounds__(256) void certified_count_kernel(int B, int T, const int32_t* __restrict__ verdict, int32_t* __restrict__ n_certified) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int n = 0;
  for (int t = 1; t < T; ++t) n += verdict[(size_t)b * T + t] == MKH_SWEEP_CERTIFIED ? 1 : 0;
  n_certified[b] = n;
}

// (the launch's LDS bytes — beyond 64 KB it is refused — and one or four edges per wavefront: checker_plan.h)
hipError_t launch_certified_sweep(hipStream_t stream, const void* wide_problem, int nbody, int nq, int n_pairs, const CertifiedArgs& a) {
  const bool quarter = checker_quarter(nbody, n_pairs);
  const size_t lds = certified_lds_bytes(nbody, nq, n_pairs);
  const long long blocks = quarter ? (a.N + 3) / 4 : a.N;
  if (a.N < 1 || n_pairs < 1 || lds > kCheckerLdsMax || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (!(a.resolution > 0.0) || !(a.resolution < __builtin_huge_val()) || a.max_samples < 1) return hipErrorInvalidValue;
  if (!a.reach) return hipErrorInvalidValue;
  const WideProblem* const P = (const WideProblem*)wide_problem;
  if (a.mode == kSweepPairs) {
    if (!a.from || !a.to || !a.margin || !a.lower_bound || !a.motion || !a.sample || !a.pair || !a.segment || !a.bound_pair ||
        !a.n_samples || !a.capped || !a.verdict)
      return hipErrorInvalidValue;
    if (quarter)
      hipLaunchKernelGGL((certified_sweep_kernel<16, kSweepPairs>), dim3((unsigned)blocks), dim3(kWave), lds, stream, P, a);
    else
      hipLaunchKernelGGL((certified_sweep_kernel<64, kSweepPairs>), dim3((unsigned)blocks), dim3(kWave), lds, stream, P, a);
    return hipGetLastError();
  }
  // ---- the graph builds: launch_sweep's conditions on the shape, an output index below 2^31 (kCertIndex holds it), the policy
  if (a.W < 1 || a.T < 1 || !a.nodes || !a.tracked || (long long)a.N * (a.mode == kSweepLadder ? 1 : a.W) > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (a.mode == kSweepLadder) {
    if (a.T < 2 || a.N % ((long long)(a.T - 1) * a.W * a.W) != 0 || (a.N / (a.T - 1)) * a.T > 0x7fffffffLL) return hipErrorInvalidValue;
    if (!a.blocked || (a.policy != MKH_EDGE_REJECT_COLLIDING && a.policy != MKH_EDGE_REQUIRE_CERTIFIED)) return hipErrorInvalidValue;
    if (quarter)
      hipLaunchKernelGGL((certified_sweep_kernel<16, kSweepLadder>), dim3((unsigned)blocks), dim3(kWave), lds, stream, P, a);
    else
      hipLaunchKernelGGL((certified_sweep_kernel<64, kSweepLadder>), dim3((unsigned)blocks), dim3(kWave), lds, stream, P, a);
  } else if (a.mode == kSweepPath) {
    if (!a.node_index || !a.margin || !a.lower_bound || !a.n_samples || !a.verdict) return hipErrorInvalidValue;
    if (quarter)
      hipLaunchKernelGGL((certified_sweep_kernel<16, kSweepPath>), dim3((unsigned)blocks), dim3(kWave), lds, stream, P, a);
    else
      hipLaunchKernelGGL((certified_sweep_kernel<64, kSweepPath>), dim3((unsigned)blocks), dim3(kWave), lds, stream, P, a);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_certified_count(hipStream_t stream, int B, int T, const int32_t* verdict, int32_t* n_certified) {
  unsigned grid;
  if (B < 1 || T < 1 || !verdict || !n_certified || !grid_1d(B, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(certified_count_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, B, T, verdict, n_certified);
  return hipGetLastError();
}

}  // namespace mkh
