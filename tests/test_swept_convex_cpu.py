"""What the sweeps on checkers with general convex pairs rest on that needs no GPU: the new entry point in the header, the library
and the Python prototypes; the host-side judgement of `sweep_rows`; the conditions on the cases of tests/swept_convex_cases.py that
make tests/test_gpu_swept_convex.py a test of the general convex pairs — stated on the numpy reference alone —; and the resources
the compiler reports for the new kernel."""

import json
import os
import re

import numpy as np
import pytest

import swept_convex_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_prototyped():
    import ctypes
    from mink_amd import _native as nat
    text = open(os.path.join(REPO, "include", "minkhip.h")).read()
    assert re.search(r"int32_t\s+mkh_problem_set_sweep_rows\(MkhProblem \*checker, int64_t rows", text)
    rule = text[text.index("THE RULE OF THE SWEEP (mkh_swept_clearance"):text.index("typedef struct MkhSweptClearanceIO")]
    assert "mkh_problem_set_sweep_rows" in rule and "MKH_E_LIMIT" in rule
    assert "mkh_problem_set_sweep_rows" in nat.EXPORTED_SYMBOLS
    L = nat.lib()
    assert L.mkh_problem_set_sweep_rows.argtypes == [ctypes.c_void_p, ctypes.c_int64] and L.mkh_problem_set_sweep_rows.restype is ctypes.c_int32
    assert L.mkh_problem_set_sweep_rows(None, 8) == -1 and b"null problem" in L.mkh_last_error()


def test_sweep_rows_is_judged_on_the_host():
    import mink_amd
    model, spec, _ = sc.shapes()
    limits = sc.limit_objects(model, spec)
    assert mink_amd.CollisionChecker(model, limits).sweep_rows == 0
    assert mink_amd.CollisionChecker(model, limits, sweep_rows=np.int64(96)).sweep_rows == 96
    for bad in (-1, 1.5, "8", None, True):
        with pytest.raises(ValueError, match="sweep_rows must be an int >= 0"):
            mink_amd.CollisionChecker(model, limits, sweep_rows=bad)


def test_convex_shapes_exercises_the_general_convex_pairs():
    """On the reference alone: (a) at least 8 colliding and 8 free kept edges, (b) general convex pairs of at least two families
    and an analytic pair attain the minimum on kept edges, (c) at least 5 sample evaluations of a general convex pair overlap (the
    expanding polytope), (d) at most a quarter of the candidates dropped — pinned: none."""
    _, _, ref, dist = sc.shapes_sweep()
    keep = sc.keep(ref, 0, 16)
    assert int(ref.in_collision[keep].sum()) >= 8 and int((~ref.in_collision[keep]).sum()) >= 8
    conv = np.array([g for _, _, g in sc.PAIRS])
    deciding = {sc.family(k) for k in ref.pair[keep] if conv[k]}
    print("general convex families deciding:", sorted(deciding), "- analytic:", sorted({sc.family(k) for k in ref.pair[keep] if not conv[k]}))
    assert len(deciding) >= 2 and (~conv[ref.pair[keep]]).any()
    assert int((dist[:, :, conv] < 0.0).sum()) >= 5
    families = {sc.family(k) for k in range(len(sc.PAIRS)) if conv[k]}
    assert families == {"cylinder-box", "cylinder-cylinder", "ellipsoid-box", "ellipsoid-cylinder", "capsule-ellipsoid", "ellipsoid-ellipsoid"}
    assert {sc.family(k) for k in range(len(sc.PAIRS)) if not conv[k]} == {"capsule-box", "box-box", "capsule-capsule", "capsule-cylinder"}


def test_pair_list_splits_as_the_cases_say():
    """The geoms of the model are the types the pair list names, and `general` marks the families without an analytic routine."""
    model, spec, _ = sc.shapes()
    types = np.asarray(model.geom_type)
    names = {2: "sphere", 3: "capsule", 4: "ellipsoid", 5: "cylinder", 6: "box"}
    for (a, b, general), pair in zip(sc.PAIRS, spec[0]["geom_pairs"]):
        got = sorted([names[int(types[pair[0][0]])], names[int(types[pair[1][0]])]])
        assert got == sorted([sc.TYPES[a % 4], sc.TYPES[b % 4]])
        assert general == (("ellipsoid" in got) or got in (["box", "cylinder"], ["cylinder", "cylinder"]))


def test_the_other_cases_keep_what_they_are_for():
    a, b, ref = sc.ur5e_convex_edges()
    keep = sc.keep(ref, 0, 32)
    assert len(a) == 43 and (ref.pair[keep] == sc.UR5E_CONVEX_PAIR).any() and 0 < ref.in_collision[keep].sum() < len(keep)
    _, _, _, _, cref = sc.cans()
    assert len(sc.keep(cref, 0, 4)) == 4 and 0 < cref.in_collision.sum() < 4
    for sparse in (False, True):
        _, _, trk, want = sc.ladder(sparse)
        em = want["edge_margin_all"]
        swept = np.isfinite(em)
        assert np.abs(em[swept]).min() > 1e-6 and np.abs(want["node_margin"]).min() > 1e-6
        assert want["blocked"].any() and (swept & ~want["blocked"]).any()
        unswept = int((~swept[:, 1:]).sum())
        assert unswept > 0                                       # (edges the pre-pass has to skip)
        if sparse:
            assert unswept > sc.ladder(False)[3]["edge_margin_all"][:, 1:].size - int(np.isfinite(sc.ladder(False)[3]["edge_margin_all"]).sum())


def test_new_kernel_is_free_of_spills_scratch_and_callees():
    path = os.path.join(REPO, "mink_amd", "kernel_resources.json")
    table = json.load(open(path))
    e = table["convex_sweep_kernel"]
    assert e["vgpr_spills"] == 0 and e["vgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0 and e["callees"] == {}, e
    # ... and so are the sweep's two builds behind it, and the builds for checkers without such pairs, which stay what they were
    for k in ("sweep_cv_kernel<16>", "sweep_cv_kernel<64>", "sweep_kernel<16>", "sweep_kernel<64>"):
        assert table[k]["vgpr_spills_with_callees"] == 0 and table[k]["sgpr_spills_with_callees"] == 0, (k, table[k])
        assert table[k]["scratch_bytes_per_lane"] == 0 and table[k]["callees"] == {}, (k, table[k])
    assert (table["sweep_kernel<16>"]["vgprs"], table["sweep_kernel<64>"]["vgprs"]) == (160, 150)      # (profiles/r22_swept.txt)
