// Turn unwinding (mkh_unwind_turns, MKH_FLAG_UNWIND_TURNS; include/minkhip.h "THE RULE OF THE UNWINDING"): the rows of a batch of
// configurations moved to the full turn of every eligible hinge that lies nearest a reference posture, in front of the
// distinct-set selection.  One small kernel and its launcher (declared in outer_launch.h); nothing here touches a solve kernel
// or its argument structs.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "outer_launch.h"

namespace mkh {

// One thread per entry (row i, qpos address k).  `table` holds three doubles per address: the mode (kUnwCopy, kUnwFree: an
// eligible unlimited hinge, kUnwRange: an eligible limited one), range_lo and range_hi — built on the host from the model
// (minkhip.hip ms_build_tables), so the eligibility test range_hi - range_lo >= TWO_PI is made once, in the same arithmetic as
// the numpy restatement.  q_out may be q_rows: every thread reads and writes its own entry only.
//
// What follows from the rule (the header states it in full):
//  - idempotent, bitwise: the quotient of a result lies within 1/2 of 0, a second pass finds k = 0 or a k that the limits cut
//    back to 0, and k == 0 returns x itself — never x + 0·TWO_PI, which would turn -0.0 into +0.0;
//  - a value inside its range stays inside: the two loops stop at the first k whose shifted value is, at k = 0 at the latest;
//  - the pose moves only by the rounding of k·TWO_PI and of the sum;
//  - the loops' converged flags are carried over by the callers, not re-evaluated here: this kernel sees configurations only.
__global__ __launch_bounds__(kOuterBlock) void unwind_turns_kernel(const double* __restrict__ table, long long n_rows,
                                                                    long long rows_per_ref, int nq, const double* q_rows,
                                                                    const double* __restrict__ q_ref, double* q_out) {
#pragma clang fp contract(off)      // x + k·TWO_PI rounds like the numpy restatement: a product, then a sum
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_rows * nq) return;
  const long long i = e / nq;
  const int a = (int)(e - i * nq);
  const double x = q_rows[e];
  const double mode = table[3 * a];
  double out = x;
  if (mode != kUnwCopy) {
    constexpr double kTwoPi = 6.283185307179586;
    const double r = q_ref[(i / rows_per_ref) * nq + a];
    const double quot = (r - x) / kTwoPi;
    double k = __builtin_rint(quot);                         // (round half to even: the default rounding mode)
    // (x or r NaN or infinite makes the quotient NaN or infinite: the one test covers the three)
    if (!(__builtin_fabs(quot) <= 1e6)) k = 0.0;
    if (mode == kUnwRange) {
      const double lo = table[3 * a + 1], hi = table[3 * a + 2];
      while (k > 0.0 && x + k * kTwoPi > hi) k -= 1.0;       // (at most |k| <= 1e6 steps; a value in range needs (hi - lo) / TWO_PI)
      while (k < 0.0 && x + k * kTwoPi < lo) k += 1.0;
    }
    if (k != 0.0) out = x + k * kTwoPi;
  }
  q_out[e] = out;
}

hipError_t launch_unwind_turns(hipStream_t stream, const double* table, long long n_rows, long long rows_per_ref, int nq,
                               const double* q_rows, const double* q_ref, double* q_out) {
  unsigned grid;
  if (n_rows < 1 || rows_per_ref < 1 || nq < 1 || !grid_1d(n_rows * nq, &grid)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(unwind_turns_kernel, dim3(grid), dim3(kOuterBlock), 0, stream, table, n_rows, rows_per_ref, nq, q_rows, q_ref,
                     q_out);
  return hipGetLastError();
}

}  // namespace mkh
