"""What checked candidate tracking and checked refinement on checkers with general convex pairs rest on that needs no GPU: the new
entry point in the header, the library and the Python prototypes; the host-side judgement of `check_rows`; the conditions on the
tracking case of tests/convex_check_cases.py that make tests/test_gpu_convex_checks.py a test of the general convex pairs — stated
on the numpy reference alone —; and the resources the compiler reports for the new kernels and for the builds beside them."""

import json
import os
import re

import numpy as np
import pytest

import convex_check_cases as cc
import swept_convex_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_prototyped():
    import ctypes
    from mink_amd import _native as nat
    text = open(os.path.join(REPO, "include", "minkhip.h")).read()
    assert re.search(r"int32_t\s+mkh_problem_set_check_rows\(MkhProblem \*checker, int64_t rows", text)
    rule = text[text.index("THE RULE OF THE SWEEP (mkh_swept_clearance"):text.index("typedef struct MkhSweptClearanceIO")]
    assert "mkh_problem_set_check_rows" in rule and "1 + 2M" in rule and "SPECULATIVE" in rule
    assert "mkh_problem_set_check_rows" in nat.EXPORTED_SYMBOLS
    L = nat.lib()
    assert L.mkh_problem_set_check_rows.argtypes == [ctypes.c_void_p, ctypes.c_int64] and L.mkh_problem_set_check_rows.restype is ctypes.c_int32
    assert L.mkh_problem_set_check_rows(None, 8) == -1 and b"null problem" in L.mkh_last_error()
    assert L.mkh_version() == 108                                # (the change is additive)
    assert callable(nat.NativeProblem.set_check_rows)


def test_check_rows_is_judged_on_the_host():
    import mink_amd
    model, spec, _ = sc.shapes()
    limits = sc.limit_objects(model, spec)
    ck = mink_amd.CollisionChecker(model, limits)
    assert ck.check_rows == 0 and ck.sweep_rows == 0
    ck = mink_amd.CollisionChecker(model, limits, sweep_rows=6, check_rows=np.int64(96))
    assert ck.check_rows == 96 and ck.sweep_rows == 6
    for bad in (-1, 1.5, "8", None, True):
        with pytest.raises(ValueError, match="check_rows must be an int >= 0"):
            mink_amd.CollisionChecker(model, limits, check_rows=bad)


def test_the_tracking_case_exercises_the_general_convex_pairs():
    """On the reference alone (about 2 s): 33 of the 64 nodes collide and a general convex pair attains the margin of 44; 21 edges
    are swept, 6 collide, a general convex pair attains the margin of 13; no judged margin within 1e-6 of zero."""
    assert cc.tracking_counts() == cc.TRACK_COUNTS
    (model, limits, q, q_all), want = cc.tracking()
    assert q_all.shape == (4, 16, model.nq) and want["seed_index"].shape == (2,)
    # what the speculative pre-pass evaluates against what the check reads: every row with a predecessor is converged with status
    # 0 here, so 48 edges are pre-evaluated and the 21 behind a free node are read
    T, R = want["node_margin_all"].shape
    assert R * (T - 1) == 48 and len(want["swept"]) == 21 and all(want["node_margin_all"][t, i] >= 0.0 for t, i in want["swept"])
    # the cases' own split of the pair list is the fixture's: 9 of 15 general convex, 27 of 45 in the wide list
    from clearance_ref import limits_of
    assert cc.convex_mask(model, limits).tolist() == [g for _, _, g in sc.PAIRS]
    assert sum(len(p) for p, _, _ in cc.without_convex(model, limits)) == 6
    wide_model, wide_spec = cc.shapes_spec(wide=True)
    assert int(cc.convex_mask(wide_model, limits_of(sc.limit_objects(wide_model, wide_spec))).sum()) == 27


# registers, spills, scratch and occupancy of the builds this feature re-included or put behind a template parameter, as the
# commit before it compiled them
PARENT = {
    "tmf_check_kernel<16>": dict(vgprs=158, agprs=0, sgprs=97, vgpr_spills=0, sgpr_spills=0, scratch_bytes_per_lane=0, occupancy_waves_per_simd=3),
    "tmf_check_kernel<64>": dict(vgprs=148, agprs=0, sgprs=106, vgpr_spills=0, sgpr_spills=0, scratch_bytes_per_lane=0, occupancy_waves_per_simd=3),
    "lr_check_kernel<16>": dict(vgprs=234, agprs=0, sgprs=106, vgpr_spills=0, sgpr_spills=6, scratch_bytes_per_lane=0, occupancy_waves_per_simd=2),
    "lr_check_kernel<64>": dict(vgprs=193, agprs=0, sgprs=106, vgpr_spills=0, sgpr_spills=25, scratch_bytes_per_lane=0, occupancy_waves_per_simd=2),
    "sweep_kernel<16>": dict(vgprs=160, agprs=0, sgprs=93, vgpr_spills=0, sgpr_spills=0, scratch_bytes_per_lane=0, occupancy_waves_per_simd=3),
    "sweep_kernel<64>": dict(vgprs=150, agprs=0, sgprs=104, vgpr_spills=0, sgpr_spills=0, scratch_bytes_per_lane=0, occupancy_waves_per_simd=3),
    "sweep_cv_kernel<16>": dict(vgprs=166, agprs=0, sgprs=95, vgpr_spills=0, sgpr_spills=0, scratch_bytes_per_lane=0, occupancy_waves_per_simd=3),
    "sweep_cv_kernel<64>": dict(vgprs=154, agprs=0, sgprs=106, vgpr_spills=0, sgpr_spills=0, scratch_bytes_per_lane=0, occupancy_waves_per_simd=3),
    "convex_sweep_kernel": dict(vgprs=256, agprs=92, sgprs=106, vgpr_spills=0, sgpr_spills=146, scratch_bytes_per_lane=0, occupancy_waves_per_simd=1),
}
NEW = ("convex_check_kernel", "tmf_check_cv_kernel<16>", "tmf_check_cv_kernel<64>", "lr_check_cv_kernel<16>", "lr_check_cv_kernel<64>")


def _table():
    return json.load(open(os.path.join(REPO, "mink_amd", "kernel_resources.json")))


def test_new_kernels_are_free_of_spills_scratch_and_callees():
    table = _table()
    for k in NEW:
        e = table[k]
        assert e["vgpr_spills"] == 0 and e["vgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0 and e["callees"] == {}, (k, e)
    # the check builds sit at their twins' occupancy; the pre-pass at convex_sweep_kernel's registers
    assert [table["tmf_check_cv_kernel<%d>" % n]["occupancy_waves_per_simd"] for n in (16, 64)] == [3, 3]
    assert [table["lr_check_cv_kernel<%d>" % n]["occupancy_waves_per_simd"] for n in (16, 64)] == [2, 2]
    assert (table["convex_check_kernel"]["vgprs"], table["convex_check_kernel"]["agprs"]) == (256, 92)


@pytest.mark.parametrize("name", list(PARENT))
def test_builds_beside_them_keep_their_resources(name):
    """Vector registers, accumulation registers, spilled vector registers, scratch, occupancy and callees exactly; scalar registers
    and scalar spills (which go to vector lanes, not to memory) not above what they were."""
    e, was = _table()[name], PARENT[name]
    for k in ("vgprs", "agprs", "vgpr_spills", "scratch_bytes_per_lane", "occupancy_waves_per_simd"):
        assert e[k] == was[k], (name, k, e[k], was[k])
    assert e["callees"] == {} and e["vgpr_spills_with_callees"] == 0
    assert e["sgprs"] <= was["sgprs"] and e["sgpr_spills"] <= was["sgpr_spills"], (name, e["sgprs"], e["sgpr_spills"], was)


def test_static_lds_is_what_the_compiler_reports():
    """Static LDS per block from the compiler's remarks: none in the checks and the sweeps, whose group slices are dynamic
    (sweep_lds_bytes, one launcher for both builds of each); the pre-pass holds convex_sweep_kernel's 12 288 bytes, the lane
    header's workspace, which that kernel had before it was re-included."""
    table = _table()
    for k in list(PARENT) + list(NEW):
        want = 12288 if k in ("convex_sweep_kernel", "convex_check_kernel") else 0
        assert table[k]["lds_bytes_per_block"] == want, (k, table[k]["lds_bytes_per_block"])
