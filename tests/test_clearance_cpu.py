"""Clearance without a GPU: the numpy reference of tests/clearance_ref.py against closed-form numbers, the conditions the GPU
tests' fixtures must meet (checked with the reference alone, so that those tests cannot pass vacuously or sit on a decision
boundary), what the two new entry points refuse without a device, the new kernel's compiled resources, and the Python surface."""

import ctypes
import importlib
import inspect
import json
import os

import numpy as np
import pytest

import clearance_ref as cr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TWO_SPHERES = """<mujoco><worldbody>
  <geom name="fixed" type="sphere" size=".07" pos="0 0 0.5"/>
  <body name="b" pos="0 0 0.5"><joint name="j" type="slide" axis="1 0 0"/>
    <geom name="moving" type="sphere" size=".05"/>
  </body></worldbody></mujoco>"""
R1, R2, DMIN, DDETECT = 0.07, 0.05, 0.03, 0.4


def _two_spheres():
    import mink_amd
    m = mink_amd.loads_mjcf(TWO_SPHERES)
    pair = [(m.name2id("geom", "fixed"), m.name2id("geom", "moving"))]
    return m, [(np.array(pair), DMIN, DDETECT)]


def test_reference_against_closed_form():
    """Two spheres on one slide joint: margin = |x| − r1 − r2 − dmin, the distance capped at ddetect, one pair, and a NaN row in
    collision."""
    m, limits = _two_spheres()
    x = np.array([-0.6, -0.3, -0.14, -0.05, 0.0, 0.1, 0.149, 0.151, 0.3, 0.519, 0.521, 2.0])
    r = cr.clearance(m, limits, x[:, None])
    d = np.minimum(np.abs(x) - R1 - R2, DDETECT)
    np.testing.assert_allclose(r.distance[:, 0], d, rtol=0, atol=1e-15)
    np.testing.assert_allclose(r.margin, d - DMIN, rtol=0, atol=1e-15)
    assert (r.distance[np.abs(x) - R1 - R2 > DDETECT, 0] == DDETECT).all()          # the cap, exactly
    assert (r.pair == 0).all()
    np.testing.assert_array_equal(r.in_collision, np.abs(x) < R1 + R2 + DMIN)
    np.testing.assert_array_equal(r.n_violated, r.in_collision.astype(np.int32))
    assert r.in_collision.any() and not r.in_collision.all()
    nan = cr.clearance(m, limits, np.array([[np.nan]]))
    assert np.isnan(nan.margin[0]) and nan.in_collision[0] and nan.n_violated[0] == 1 and nan.pair[0] == 0


def test_reference_rule_on_hand_made_distances():
    """min / lowest index on ties / violated count / NaN decides, on distances written by hand (two limits of different dmin)."""
    dmin = np.array([0.25, 0.25, 0.5])     # (binary fractions: every difference below is exact)
    dist = np.array([[0.75, 0.75, 1.0],     # every term 0.5: the lowest pair
                     [0.75, 0.375, 0.625],  # terms 0.5, 0.125, 0.125: pair 1, free
                     [0.125, 0.0, 0.25],    # terms −0.125, −0.25, −0.25: all three violated, pair 1
                     [0.75, np.nan, 0.0],   # a NaN term decides, whatever else is there
                     [0.25, 0.25, 0.5]])    # touching dmin exactly: margin 0, free
    r = cr.from_distances(dist, dmin)
    np.testing.assert_array_equal(r.margin[[0, 1, 2, 4]], [0.5, 0.125, -0.25, 0.0])
    np.testing.assert_array_equal(r.pair, [0, 1, 1, 1, 0])
    np.testing.assert_array_equal(r.n_violated, [0, 0, 3, 2, 0])
    np.testing.assert_array_equal(r.in_collision, [False, False, True, True, False])
    assert np.isnan(r.margin[3])


# (fixture, pairs, rows, at least this share of rows in collision AND free) — the G1 fixture has its own bounds below
FIXTURES = [("ur5e_wrist", 2, 256), ("ur5e_convex", 2, 256), ("ur5e_all", 14, 256), ("chain", 92, 16), ("shapes", 30, 64),
            ("shapes_wide", 60, 64)]


@pytest.mark.parametrize("name,n_pairs,n_rows", FIXTURES)
def test_fixture_conditions(name, n_pairs, n_rows):
    """Seen here: ur5e_wrist 114 of 256 rows in collision, min |d − dmin| 5.2e-3; ur5e_convex 113, 5.8e-3, 102 overlapping pair
    evaluations; ur5e_all 144, 3.8e-4; chain 11 of 16, 3.8e-4."""
    model, _, q = cr.fixture(name)
    limits = cr.limits_of(cr.fixture_limits(name))
    pairs, dmin, ddet = cr.pair_list(limits)
    ref = cr.fixture_ref(name)
    assert len(pairs) == n_pairs and q.shape == (n_rows, model.nq)
    n_coll = int(ref.in_collision.sum())
    gap = float(np.abs(ref.distance - dmin[None, :]).min())
    print("%s: %d pairs, %d rows, %d in collision, min |d - dmin| %.2e, %d overlapping evaluations" %
          (name, n_pairs, n_rows, n_coll, gap, int((ref.distance < 0).sum())))
    assert n_coll >= 0.1 * n_rows and n_rows - n_coll >= 0.1 * n_rows
    assert gap > 1e-6
    assert (ref.distance <= ddet[None, :]).all()
    if name == "ur5e_convex":
        assert int(model.geom_type[model.name2id("geom", "wrist_3_link")]) == 5          # a cylinder: the general convex routine
        assert int((ref.distance < 0).sum()) >= 20                                        # the polytope path is exercised
    if name == "chain":
        assert model.nbody == 81 and n_pairs > 64                                         # beyond a wavefront of bodies and of pairs
    if name in ("shapes", "shapes_wide"):
        # seen here (shapes): 50 of 64 rows in collision, min |d − dmin| 7.6e-5; of the 15 box–box pairs' 960 evaluations 624 separated
        # and in range, 56 overlapping; capsule–capsule 133 in range, capsule–cylinder 105, sphere–capsule 30, sphere–sphere 10
        types = np.sort(np.array([(int(model.geom_type[a]), int(model.geom_type[b])) for a, b in pairs]), axis=1)
        in_range = lambda t: ref.distance[:, (types == t).all(axis=1)] < ddet[(types == t).all(axis=1)][None, :]
        bb = ref.distance[:, (types == (6, 6)).all(axis=1)]
        assert (types == (6, 6)).all(axis=1).sum() >= 15
        assert ((bb > 0) & in_range((6, 6))).sum() >= 100 and (bb < 0).sum() >= 30          # box–box: separated and overlapping
        for t in ((3, 3), (2, 3), (3, 5), (2, 2)):                                          # capsule–capsule, sphere–capsule, …
            assert in_range(t).sum() >= 10, t
        # the quarter-wavefront build's second trip: more than 16 bodies on one level, more than 16 pairs
        assert 16 < model.nbody <= 32 and (n_pairs <= 32) == (name == "shapes")


def test_fixture_conditions_g1():
    """Seen here: 6 of 129 rows in collision, 67 with every pair at the cap (the tie rule: pair 0), min |d − dmin| 1.2e-3."""
    model, _, q = cr.fixture("g1")
    pairs, dmin, ddet = cr.pair_list(cr.limits_of(cr.fixture_limits("g1")))
    ref = cr.fixture_ref("g1")
    capped = (ref.distance == ddet[None, :]).all(axis=1)
    gap = float(np.abs(ref.distance - dmin[None, :]).min())
    print("g1: %d pairs, %d rows, %d in collision, %d all capped, min |d - dmin| %.2e" %
          (len(pairs), len(q), int(ref.in_collision.sum()), int(capped.sum()), gap))
    assert len(pairs) == 46 and len(q) == 129
    assert int(ref.in_collision.sum()) >= 3 and int(capped.sum()) >= 50
    assert (ref.pair[capped] == 0).all() and (ref.margin[capped] == ddet[0] - dmin[0]).all()
    assert gap > 1e-6
    types = {tuple(sorted((int(model.geom_type[a]), int(model.geom_type[b])))) for a, b in pairs}
    assert {(0, 2), (2, 2), (0, 5), (0, 6), (2, 5), (2, 6)} <= types                      # every analytic family of the list


def test_entry_points_refuse_null_arguments():
    from mink_amd import _native as nat
    lib = nat.lib()
    io = nat.MkhClearanceIO()
    assert lib.mkh_clearance(None, 1, None, ctypes.byref(io), 0, None) == -1
    assert b"null problem" in lib.mkh_last_error()
    assert lib.mkh_problem_set_collision_check(None, None) == -1
    assert b"null problem" in lib.mkh_last_error()
    assert ctypes.sizeof(nat.MkhClearanceIO) == 4 * ctypes.sizeof(ctypes.c_void_p)
    assert nat.ST_IN_COLLISION == 64


def test_clearance_kernel_resources():
    """The new kernel: no spilled VGPR (callees included), no scratch, no callee, and no entry in the spill budget."""
    from mink_amd import _native as nat
    nat.lib()
    with open(os.path.join(REPO, "mink_amd", "kernel_resources.json")) as fh:
        res = json.load(fh)
    names = sorted(k for k in res if k.startswith("clearance_kernel"))
    assert names == ["clearance_kernel<16>", "clearance_kernel<64>"]          # four rows per wavefront, one row per wavefront
    for name in names:
        e = res[name]
        print(name, {k: e[k] for k in ("vgprs", "sgprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")})
        assert e["vgpr_spills_with_callees"] == 0 and e["vgpr_spills"] == 0 and e["sgpr_spills_with_callees"] == 0
        assert e["scratch_bytes_per_lane"] == 0 and e["callees"] == {}
    with open(os.path.join(REPO, "tests", "golden", "spill_budget.json")) as fh:
        assert "clearance_kernel" not in json.dumps(json.load(fh))


def test_python_surface():
    import mink_amd
    sik = importlib.import_module("mink_amd.solve_ik")         # (the package attribute of that name is the function)
    for name in ("CollisionChecker", "Clearance", "ST_IN_COLLISION"):
        assert name in mink_amd.__all__ and hasattr(mink_amd, name), name
    assert mink_amd.ST_IN_COLLISION == 64
    assert mink_amd.Clearance._fields == ("margin", "pair", "n_violated", "in_collision", "distance")
    for fn in (mink_amd.solve_ik_multistart, mink_amd.solve_ik_solutions, mink_amd.solve_ik_goalset):
        p = inspect.signature(fn).parameters["collision_check"]
        assert p.default is None
        assert "never worse" in fn.__doc__ and "collision_check" in fn.__doc__
    # the bit is a verdict, not a QP failure: no SolverError for it, still one for a real failure beside it
    sik._status_epilogue(np.array([0, 64, 65], dtype=np.int32), "x", "y", "z")
    with pytest.raises(mink_amd.SolverError):
        sik._status_epilogue(np.array([0, 64 | 2], dtype=np.int32), "x", "y", "{n} {of} {first} {status}")


def test_collision_checker_on_the_host():
    import mink_amd
    sik = importlib.import_module("mink_amd.solve_ik")         # (the package attribute of that name is the function)
    model, _, _ = cr.fixture("ur5e_all")
    lims = cr.fixture_limits("ur5e_all") + cr.fixture_limits("ur5e_wrist")
    ck = mink_amd.CollisionChecker(model, lims, max_rows=64)
    assert ck.n_pairs == 16 and ck.geom_id_pairs.shape == (16, 2) and ck.geom_id_pairs.dtype == np.int32
    np.testing.assert_array_equal(ck.geom_id_pairs, np.concatenate([np.asarray(l.geom_id_pairs) for l in lims]))
    np.testing.assert_array_equal(ck.minimum_distance, [0.02] * 14 + [0.05] * 2)
    np.testing.assert_array_equal(ck.detection_distance, [0.2] * 14 + [0.3] * 2)

    class Mine(mink_amd.CollisionAvoidanceLimit):
        def compute_qp_inequalities(self, configuration, dt):
            return super().compute_qp_inequalities(configuration, dt)

    with pytest.raises(mink_amd.LimitDefinitionError, match="compute_qp_inequalities"):
        mink_amd.CollisionChecker(model, [Mine(model, [(["wrist_3_link"], ["floor"])])])
    with pytest.raises(mink_amd.LimitDefinitionError):
        mink_amd.CollisionChecker(model, [mink_amd.ConfigurationLimit(model)])
    with pytest.raises(mink_amd.LimitDefinitionError, match="at least one"):
        mink_amd.CollisionChecker(model, [])
    with pytest.raises(ValueError, match="shape"):
        ck.clearance(np.zeros((3, model.nq + 1)))
    cfg = mink_amd.Configuration(mink_amd.load_robot("g1"))
    with pytest.raises(ValueError, match="another model"):
        sik._check_collision_check(ck, cfg)
    with pytest.raises(ValueError, match="CollisionChecker"):
        sik._check_collision_check(object(), cfg)
    ck.close()
    with pytest.raises(ValueError, match="closed"):
        ck.clearance(np.zeros(model.nq))
