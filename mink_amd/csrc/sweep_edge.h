// Which edge a group of sweep_kernel (sweep.hip) or a lane of convex_sweep_kernel (convex_sweep.hip) works on: the kernels'
// arguments and the decode of an edge index in the three modes of outer_launch.h — one place, so that the pre-pass of the general
// convex pairs and the sweep behind it agree on every address and on which edges are swept at all.
#pragma once
#include <hip/hip_runtime.h>

#include "outer_launch.h"

namespace mkh {

// What the kernels read of a SweepArgs, one slot per role whatever the mode (kernel arguments live in scalar registers across the
// whole sample loop): p0 = from | nodes, p1 = to, i0 = sample out | tracked, i1 = pair out | node_index.  N: the edges of THIS
// launch, e0: the index of its first one (a chunk of a call with general convex pairs; otherwise 0).  cv: the (N·M, n_cv)
// distances convex_sweep_kernel left for this launch's samples, or null.
struct SweepKernelArgs {
  int32_t mode, M, T, W;
  long long N;
  const double *p0, *p1;
  int32_t *i0, *i1;
  double* margin;
  uint8_t* blocked;
  long long e0;
  const double* cv;
  int32_t n_cv;
};

inline SweepKernelArgs sweep_kernel_args(const SweepArgs& a) {
  const bool pairs = a.mode == kSweepPairs;
  return SweepKernelArgs{a.mode, a.M, a.T, a.W, a.count > 0 ? a.count : a.N, pairs ? a.from : a.nodes, pairs ? a.to : nullptr,
                         pairs ? a.sample : const_cast<int32_t*>(a.tracked), pairs ? a.pair : const_cast<int32_t*>(a.node_index),
                         a.margin, pairs ? nullptr : a.blocked, a.count > 0 ? a.first : 0, a.cv, a.n_cv};
}

struct SweepEdge {
  const double *pa, *pb;           // the two ends (an edge that is not swept: its own node twice — every address is valid)
  long long eo;                    // where the edge's outputs go
  bool swept;
  double idle;                     // the margin of an edge that is not swept
};

// Edge e (a GLOBAL index: e0 + its place in the launch) of a launch on rows of nq doubles.
__device__ __forceinline__ SweepEdge swp_edge(const SweepKernelArgs& a, long long e, int nq) {
  SweepEdge g;
  g.eo = e;
  g.swept = true;
  g.idle = __builtin_nan("");
  if (a.mode == kSweepPairs) {
    g.pa = a.p0 + (size_t)e * nq;
    g.pb = a.p1 + (size_t)e * nq;
  } else {
    const long long W = a.W;
    long long row, src, dst;                                   // waypoint row b·T + t, source node of rung t − 1, destination of t
    if (a.mode == kSweepLadder) {                              // (rungs t >= 1 only: e counts the (T − 1)·W·W edges of an instance)
      const long long per = (long long)(a.T - 1) * W * W, r = e % per;
      row = (e / per) * a.T + 1 + r / (W * W);
      src = r % W;
      dst = (r / W) % W;
      g.eo = (row * W + dst) * W + src;
    } else {
      row = e;
      dst = a.i1[row];
      src = row % a.T ? a.i1[row - 1] : 0;
    }
    const bool first = row % a.T == 0;
    if (first && a.mode == kSweepPath) g.idle = __builtin_huge_val();
    g.swept = !first && a.i0[row * W + dst] != 0;
    g.pb = a.p0 + (size_t)(row * W + dst) * nq;
    g.pa = g.swept ? a.p0 + (size_t)((row - 1) * W + src) * nq : g.pb;     // (an idle group walks its own node)
  }
  return g;
}

}  // namespace mkh
