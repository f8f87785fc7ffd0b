// The table of compiled ik_solve_kernel builds.  build.py VARIANTS is the one list; it generates a translation unit per entry
// and, in _build/dispatch.hip, one row per entry here.  Everything the host knows about WHICH builds exist — tableau size
// classes, whether a one-more-wave or one-shot twin is compiled, a kernel's name — is a query of this table (minkhip.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "mkh_types.h"

namespace mkh {

struct VariantRow {
  int nt, nr, feat;          // MKH_NT, MKH_NR (0: direct start), MKH_FEAT
  bool w3, one_shot;         // MKH_W3 (one more resident wave per SIMD), MKH_ONE_SHOT (one problem per workgroup)
  const char* kernel;        // "ik_solve_kernel_<name>"; a name with "_w4" is the twin of the "_w3" build with the same fields on the
                             // four-waves product-form map (MKH_W4P)
  void (*launch)(int grid, int lds_bytes, hipStream_t stream, const DeviceProblem* P, const SolveArgs& a, const TapArgs* taps);
};
const VariantRow* variant_table();   // kNumVariants rows (a function-local table: a namespace-scope constant would be emitted for the device, too)
extern const int kNumVariants;

inline const VariantRow* find_variant(int nt, int nr, int feat, bool w3 = false, bool one_shot = false, bool w4 = false) {
  const VariantRow* const table = variant_table();
  for (int i = 0; i < kNumVariants; ++i) {
    const VariantRow& v = table[i];
    if (v.nt == nt && v.nr == nr && v.feat == feat && v.w3 == w3 && v.one_shot == one_shot && (strstr(v.kernel, "_w4") != nullptr) == w4) return &v;
  }
  return nullptr;
}

// Smallest compiled tableau size ≥ at_least among the two-waves builds of `feat` — direct start, or low-rank start with
// NR = NT (`wood`); 0 when there is none.
inline int size_class(int at_least, int feat, bool wood = false) {
  const VariantRow* const table = variant_table();
  int best = 0;
  for (int i = 0; i < kNumVariants; ++i) {
    const VariantRow& v = table[i];
    if (v.feat == feat && v.nr == (wood ? v.nt : 0) && !v.w3 && !v.one_shot && v.nt >= at_least && (!best || v.nt < best)) best = v.nt;
  }
  return best;
}

}  // namespace mkh
