"""CPU-side check of the fused loop on the row kernel's two-row build (quad_kernel.h, `ik_quad_kernel<32, true, 32>`): it is
compiled into the library, free of VGPR spills, at the occupancy its launch assumes."""

import json


def test_two_row_loop_build_is_compiled_spill_free():
    from mink_amd.csrc import build as hipbuild
    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    table = table.get("kernels", table)
    e = table.get("ik_quad_kernel<32,1,32>")
    assert e is not None, sorted(k for k in table if "quad" in k)
    assert e["vgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0, e
    assert e["occupancy_waves_per_simd"] >= 2, e
    # (the single-solve build beside it keeps its three waves per SIMD)
    assert table["ik_quad_kernel<32,0,32>"]["occupancy_waves_per_simd"] == 3
