"""The collision checker's kernels on random trees with ball and stacked joints (tests/tree_cases.py) against the numpy references:
what no other fixture of the family reaches — the ball branch and the anchor arithmetic of clr_row's FK for jnt_pos != 0 below the
first level, swp_difference / swp_blend on a quaternion that is not the free joint's, cert_pair_motion's ball weight, the reach
table's D_after and 2 |jnt_pos| terms, and cv_chain_pose through CvRowMem, CvRowBlend and CvRowCheck on ball joints.

* clearance — every distance, margin, pair and n_violated of the 48 rows of `tree_small`, `tree_wide` and `tree_convex`, and one
  ragged call of 5 rows;
* swept clearance — the 24 edges (rows 0 .. 23 -> 24 .. 47, s = 0.3) at 1 and 8 samples; `tree_convex` with sweep_rows = 16, whose
  8-sample edges are walked in chunks of two;
* certified sweep on `tree_small` and `tree_wide` — tests/test_gpu_certified_sweep.py's own test bodies on the tree cases: every
  output field at resolution 0.05 with max_samples 64 and 4, the reach table, margin = the device's own clearance and sweep, the
  certificate on 257 dense device rows;
* the sign and the scale of quaternion ends on the device;
* ladder_path with a certifying checker on `tree_small` nodes, both policies (tests/test_gpu_ladder_certified.py's body on
  ladder_certified_cases' case "tree");
* candidate_path on `tree_convex` with check_rows = 8 (tests/test_gpu_convex_checks.py's comparison).

Tolerances: doubles to 1e-9 absolute, the reach table to 1e-12 relative, integers exactly on the candidates the references alone
separate by more than 1e-6 (the existing filters, unchanged); the number of candidates dropped is pinned in tests/tree_cases.py —
0 in every case.  Every checker has max_rows = 256."""

import numpy as np
import pytest

import clearance_ref as cr
import ladder_certified_cases as lc
import swept_convex_cases as sc
import test_gpu_certified_sweep as tg
import test_gpu_convex_checks as tcc
import test_gpu_ladder_certified as tlc
import trajectory_multistart_ref as tmref
import tree_cases as tc

pytestmark = pytest.mark.gpu
TOL = 1e-9
ALL = ["tree_small", "tree_wide", "tree_convex"]
TREES = ["tree_small", "tree_wide"]
SWEEP_ROWS = {"tree_small": 0, "tree_wide": 0, "tree_convex": 16}


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _checker(name, **kw):
    import mink_amd
    model, _, _ = cr.fixture(name)
    return mink_amd.CollisionChecker(model, cr.fixture_limits(name), max_rows=256, **kw)


# ------------------------------------------------------------------ clearance
@pytest.mark.parametrize("name", ALL)
def test_clearance_against_the_reference(nat, name):
    _, _, q = cr.fixture(name)
    ref, keep = cr.fixture_ref(name), tc.clearance_keep(name)
    ck = _checker(name)
    out = ck.clearance(q, return_distances=True)
    part = ck.clearance(q[:5], return_distances=True)          # a ragged call: a wavefront and a row of the next, or five wavefronts
    ck.close()
    e_m, e_d = np.abs(out.margin - ref.margin).max(), np.abs(out.distance - ref.distance).max()
    print("%s: %d rows x %d pairs: max |margin - ref| %.2e, max |distance - ref| %.2e, %d in collision, %d rows kept" %
          (name, len(q), ck.n_pairs, e_m, e_d, int(out.in_collision.sum()), len(keep)))
    assert out.margin.shape == (len(q),) and out.distance.shape == (len(q), ck.n_pairs)
    assert out.pair.dtype == np.int32 and out.n_violated.dtype == np.int32 and out.in_collision.dtype == bool
    assert e_m <= TOL and e_d <= TOL
    for f in ("in_collision", "n_violated", "pair"):
        np.testing.assert_array_equal(getattr(out, f)[keep], getattr(ref, f)[keep], err_msg=f)
    assert (out.distance <= ck.detection_distance[None, :]).all()
    rows = np.arange(len(q))
    np.testing.assert_array_equal(out.margin, out.distance[rows, out.pair] - ck.minimum_distance[out.pair])
    for f in out._fields:
        np.testing.assert_array_equal(getattr(part, f), getattr(out, f)[:5], err_msg=f"5 rows: {f}")


# ------------------------------------------------------------------ swept clearance
@pytest.mark.parametrize("M", tc.SWEEP_SAMPLES)
@pytest.mark.parametrize("name", ALL)
def test_swept_clearance_against_the_reference(nat, name, M):
    a, b, ref, keep = tc.sweep_case(name, M)
    ck = _checker(name, sweep_rows=SWEEP_ROWS[name])
    out = ck.swept_clearance(a, b, n_samples=M)
    ck.close()
    assert out.margin.shape == (tc.N_EDGES,) and out.sample.dtype == np.int32 and out.pair.dtype == np.int32
    err = np.abs(out.margin - ref.margin).max()
    print("%s: %d edges x %d samples, %d kept: max |margin - ref| %.2e, %d collide" % (name, len(a), M, len(keep), err, int(ref.in_collision.sum())))
    assert err <= TOL
    for f in ("sample", "pair", "in_collision"):
        np.testing.assert_array_equal(np.asarray(getattr(out, f))[keep], getattr(ref, f)[keep], err_msg=f)


# ------------------------------------------------------------------ certified sweep: tests/test_gpu_certified_sweep.py's bodies
@pytest.mark.parametrize("case", ["tree_small", "tree_small_capped", "tree_wide", "tree_wide_capped"])
def test_certified_sweep_against_the_reference(nat, case):
    out = tg._against_reference(case)
    name = tg.CASES[case][0]
    key = "verdicts_at_4" if case.endswith("_capped") else "verdicts"
    assert tuple(np.bincount(out.verdict, minlength=3)) == tc.PINNED[name][key]
    assert int(out.capped.sum()) == tc.PINNED[name]["capped_at_4" if case.endswith("_capped") else "capped"]


@pytest.mark.parametrize("name", TREES)
def test_reach_table_matches_the_reference(nat, name):
    tg.test_reach_table_matches_the_reference(nat, name)


@pytest.mark.parametrize("name", TREES)
def test_margin_is_the_devices_own_clearance_and_sweep(nat, name):
    tg.margin_is_the_devices_own_clearance_and_sweep(name)


@pytest.mark.parametrize("name", TREES)
def test_certified_edges_hold_on_dense_device_rows(nat, name):
    tg.certified_edges_hold_on_dense_device_rows(name, tc.PINNED[name]["verdicts"][1])


# ------------------------------------------------------------------ quaternion ends
@pytest.mark.parametrize("name", TREES)
def test_sign_and_scale_of_quaternion_ends_on_the_device(nat, name):
    """b with every ball and free quaternion negated, and both ends with every such quaternion scaled by its own factor in
    [0.5, 2], through swept_clearance and certified_sweep: integers equal, doubles within 1e-9 of the plain call."""
    model, _, _ = cr.fixture(name)
    _, a, b, resolution, mx, _, keep = tg.case(name)
    a, b = a[keep], b[keep]
    ck = _checker(name)
    plain_s, plain_c = ck.swept_clearance(a, b, n_samples=8), ck.certified_sweep(a, b, resolution, max_samples=mx)
    for what, (a2, b2) in (("negated", (a, tc.negated(model, b))), ("scaled", (tc.scaled(model, a, 1), tc.scaled(model, b, 2)))):
        assert not np.array_equal(b2, b)
        s, c = ck.swept_clearance(a2, b2, n_samples=8), ck.certified_sweep(a2, b2, resolution, max_samples=mx)
        for f in ("sample", "pair", "in_collision"):
            np.testing.assert_array_equal(getattr(s, f), getattr(plain_s, f), err_msg=f"{what}: swept {f}")
        for f in tg.INTS:
            np.testing.assert_array_equal(getattr(c, f), getattr(plain_c, f), err_msg=f"{what}: certified {f}")
        errs = {"swept margin": np.abs(s.margin - plain_s.margin).max()}
        for f in tg.DOUBLES:
            x, y = getattr(c, f), getattr(plain_c, f)
            np.testing.assert_array_equal(np.isinf(x), np.isinf(y), err_msg=f"{what}: {f}")
            errs[f] = np.abs(x[np.isfinite(y)] - y[np.isfinite(y)]).max()
        print("%s, %s: %s" % (name, what, ", ".join("%s %.2e" % kv for kv in errs.items())))
        assert max(errs.values()) <= TOL, (what, errs)
    ck.close()


# ------------------------------------------------------------------ graph decode
def test_certifying_ladder_on_tree_nodes(nat):
    """ladder_path(collision_check=, edge_resolution=0.05) under both policies on `tree_small` nodes, (B, T, S) = (2, 4, 3)."""
    def conditions(c):
        assert c["fixture"] == "tree_small" and c["q_nodes"].shape[:3] == (2, 4, 3) and c["resolution"] == 0.05
        assert tlc._verdicts(c) == {0, 1, 2} and tlc._differs(c).any()
        assert len(c["keep"]) == 2
    tlc._against_reference("tree", conditions, max_rows=256)


# ------------------------------------------------------------------ the check kernel
def test_candidate_path_on_tree_convex(nat):
    """candidate_path(collision_check=) on `tree_convex`, T, B, S = 3, 2, 4, three samples per edge, check_rows = 8 (two items of
    a node and its three samples per chunk): general convex pairs below ball joints attain the margin of nodes and of samples."""
    import mink_amd as mink
    (model, limits, q, q_all), want, counts = tc.tracking()
    assert counts == tc.TRACK_COUNTS
    T, B, S, M = (tc.TRACK[k] for k in "TBSM")
    ck = _checker("tree_convex", check_rows=8)
    out = mink.candidate_path(mink.Configuration(model, q.copy()), tmref.by_instance(q_all, B, S), collision_check=ck, edge_samples=M)
    ck.close()
    assert isinstance(out, mink.FreeCandidatePath) and out.edge_margin_all.shape == (B, S, T)
    tcc._against_tracking(out, want, B, S, "tree_convex")
    assert int((~(out.node_margin_all >= 0.0)).sum()) == counts["nodes_in_collision"]
