"""mkh_clearance on the device against the numpy reference of tests/clearance_ref.py (include/minkhip.h "THE RULE OF CLEARANCE"):
every fixture of tests/test_clearance_cpu.py — analytic pairs, the general convex routine, a model beyond 64 bodies with more than
a wavefront of pairs —, chunking, host against device pointers, the bounding-sphere cull against none, and a checker without pairs.

Tolerance: margin and distance to 1e-9 absolute — what tests/test_gpu_collision_shapes.py holds h = gain·(d − dmin)/dt to; pair,
n_violated and in_collision exactly (the fixtures keep every d_k more than 1e-6 away from its dmin_k)."""

import numpy as np
import pytest

import clearance_ref as cr

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _checker(name, max_rows):
    import mink_amd
    model, _, _ = cr.fixture(name)
    return mink_amd.CollisionChecker(model, cr.fixture_limits(name), max_rows=max_rows)


# (fixture, max_rows): 64 rows per launch walks the 256 / 129 rows in chunks, the last one ragged for G1
@pytest.mark.parametrize("name,max_rows", [("ur5e_wrist", 256), ("ur5e_convex", 64), ("ur5e_all", 64), ("g1", 64), ("chain", 16),
                                           ("shapes", 64), ("shapes_wide", 30)])
def test_clearance_against_the_reference(nat, name, max_rows):
    _, _, q = cr.fixture(name)
    ref = cr.fixture_ref(name)
    ck = _checker(name, max_rows)
    out = ck.clearance(q, return_distances=True)
    ck.close()
    e_m, e_d = np.abs(out.margin - ref.margin).max(), np.abs(out.distance - ref.distance).max()
    print("%s: %d rows x %d pairs: max |margin - ref| %.2e, max |distance - ref| %.2e, %d in collision" %
          (name, len(q), ck.n_pairs, e_m, e_d, int(out.in_collision.sum())))
    assert out.margin.shape == (len(q),) and out.distance.shape == (len(q), ck.n_pairs)
    assert out.pair.dtype == np.int32 and out.n_violated.dtype == np.int32 and out.in_collision.dtype == bool
    np.testing.assert_array_equal(out.in_collision, ref.in_collision)
    np.testing.assert_array_equal(out.n_violated, ref.n_violated)
    np.testing.assert_array_equal(out.pair, ref.pair)
    assert e_m <= TOL and e_d <= TOL
    assert (out.distance <= ck.detection_distance[None, :]).all()
    # the margin is one of the row's own terms, bit for bit: the minimum is exact
    rows = np.arange(len(q))
    np.testing.assert_array_equal(out.margin, out.distance[rows, out.pair] - ck.minimum_distance[out.pair])


def test_chunking_and_leading_shapes(nat):
    """N = 129 on a checker of 64 rows per launch against one launch; (nq,) and (..., nq) rows; distances only when asked."""
    _, _, q = cr.fixture("g1")
    whole, chunked = _checker("g1", 256), _checker("g1", 64)
    a, b = whole.clearance(q, return_distances=True), chunked.clearance(q, return_distances=True)
    for f in a._fields:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    one = chunked.clearance(q[5])
    assert one.margin.shape == () and one.distance is None and one.margin == a.margin[5] and one.pair == a.pair[5]
    grid = chunked.clearance(q[:128].reshape(4, 32, -1), return_distances=True)
    assert grid.margin.shape == (4, 32) and grid.distance.shape == (4, 32, 46) and grid.in_collision.shape == (4, 32)
    np.testing.assert_array_equal(grid.distance.reshape(128, 46), a.distance[:128])
    whole.close(); chunked.close()
    # four rows share a wavefront on a small arm: a row count that is no multiple of four, one launch and several
    _, _, qa = cr.fixture("ur5e_all")
    ref = cr.fixture_ref("ur5e_all")
    for max_rows in (64, 6):
        ck = _checker("ur5e_all", max_rows)
        part = ck.clearance(qa[:23], return_distances=True)
        ck.close()
        np.testing.assert_array_equal(part.pair, ref.pair[:23])
        np.testing.assert_array_equal(part.in_collision, ref.in_collision[:23])
        assert np.abs(part.distance - ref.distance[:23]).max() <= TOL and np.abs(part.margin - ref.margin[:23]).max() <= TOL


@pytest.mark.parametrize("max_rows", [5, 1])
def test_pre_evaluated_pairs_do_not_depend_on_the_chunking(nat, max_rows):
    """`shapes` (general convex pairs behind their pre-pass, analytic pairs beside them): 7 rows in chunks of 5 + 2 and of one row
    each against one launch, bit for bit — the buffer of pre-evaluated pairs is reused by every chunk."""
    _, _, q = cr.fixture("shapes")
    whole, chunked = _checker("shapes", 256), _checker("shapes", max_rows)
    a, b = whole.clearance(q[:7], return_distances=True), chunked.clearance(q[:7], return_distances=True)
    whole.close(); chunked.close()
    assert a.margin.shape == (7,)
    for f in a._fields:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)


@pytest.mark.parametrize("name", ["shapes", "shapes_wide", "ur5e_convex", "g1"])
def test_rows_with_nan_or_inf_are_in_collision(nat, name):
    """A row of q with a NaN or an infinite entry: every d_k NaN, margin NaN, pair 0, every pair violated, in collision — on
    capsule–capsule pairs (whose routine would answer "out of range" to NaN poses), on pre-evaluated convex pairs, on both builds
    of the kernel; the rows around it are untouched."""
    _, _, q = cr.fixture(name)
    ref = cr.fixture_ref(name)
    rows = q[:11].copy()
    rows[2, 0] = np.nan
    rows[5, -1] = np.inf
    rows[6, :] = np.nan
    rows[9, rows.shape[1] // 2] = -np.inf
    bad = np.array([2, 5, 6, 9])
    good = np.setdiff1d(np.arange(11), bad)
    model, _, _ = cr.fixture(name)
    want = cr.clearance(model, cr.limits_of(cr.fixture_limits(name)), rows)
    assert want.in_collision[bad].all() and np.isnan(want.margin[bad]).all() and (want.pair[bad] == 0).all()
    ck = _checker(name, 8)
    out = ck.clearance(rows, return_distances=True)
    ck.close()
    assert np.isnan(out.margin[bad]).all() and np.isnan(out.distance[bad]).all()
    assert out.in_collision[bad].all() and (out.pair[bad] == 0).all() and (out.n_violated[bad] == ck.n_pairs).all()
    np.testing.assert_array_equal(out.in_collision, want.in_collision)
    np.testing.assert_array_equal(out.pair, want.pair)
    np.testing.assert_array_equal(out.n_violated, want.n_violated)
    np.testing.assert_array_equal(out.pair[good], ref.pair[good])
    assert np.abs(out.distance[good] - ref.distance[good]).max() <= TOL and np.abs(out.margin[good] - ref.margin[good]).max() <= TOL


def test_host_pointers_against_device_pointers(nat):
    import torch
    for name in ("ur5e_convex", "chain"):
        _, _, q = cr.fixture(name)
        ck = _checker(name, 64)
        host = ck.clearance(q, return_distances=True)
        dev = ck.clearance(torch.as_tensor(q, device="cuda"), return_distances=True)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in dev)
        for f in host._fields:
            np.testing.assert_array_equal(getattr(dev, f).cpu().numpy(), getattr(host, f), err_msg=f"{name}: {f}")
        ck.close()


def test_pair_cull_changes_nothing(nat):
    """The 92-pair chain: bounding spheres in front of the distance routines (more than a wavefront of pairs) against none."""
    _, _, q = cr.fixture("chain")
    ck, ck_nocull = _checker("chain", 16), _checker("chain", 16)
    a = ck.clearance(q, return_distances=True)
    with nat.diag_options(nat.DIAG_NO_PAIR_CULL):          # (the handle is created on first use, inside the block)
        b = ck_nocull.clearance(q, return_distances=True)
    assert [p.diag for _, p in ck_nocull._handles.values()] == [nat.DIAG_NO_PAIR_CULL] and [p.diag for _, p in ck._handles.values()] == [0]
    capped = int((a.distance == ck.detection_distance[None, :]).sum())
    print("chain: %d of %d pair evaluations at the cap" % (capped, a.distance.size))
    assert 0 < capped < a.distance.size
    for f in a._fields:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
    ck.close(); ck_nocull.close()


def test_refusals(nat):
    from mink_amd import workloads
    m = workloads.load_robot("ur5e")
    nm = nat.NativeModel(m, 0)
    bare = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "attachment_site"), "cost": [1.0] * 6}],
                             max_batch=4)
    with pytest.raises(nat.MinkHipError, match="no collision pairs"):
        bare.clearance(np.zeros((2, m.nq)))
    assert nat.lib().mkh_problem_set_collision_check(bare.handle, bare.handle) == -1
    assert b"no collision pairs" in nat.lib().mkh_last_error()
    with pytest.raises(ValueError, match="shape"):
        bare.clearance(np.zeros((2, m.nq + 1)))
    bare.close(); nm.close()
    # general convex pairs on a model beyond 64 bodies: not pre-evaluated there, refused (a documented limit)
    import wide_cases as wc
    from mink_amd.mjcf import loads_mjcf
    wide = loads_mjcf(wc.mjcf_text("hinge80")[0])
    assert wide.nbody == 81
    wide.geom_type, wide.geom_size = wide.geom_type.copy(), wide.geom_size.copy()
    wide.geom_type[3], wide.geom_type[40] = 5, 6                        # a cylinder and a box: no analytic routine for the pair
    wide.geom_size[3], wide.geom_size[40] = (0.01, 0.02, 0.0), (0.01, 0.01, 0.01)
    nmw = nat.NativeModel(wide, 0)
    col = {"geom_id_pairs": np.array([[3, 40], [5, 50]]), "gain": 0.85, "minimum_distance_from_collisions": 0.01,
           "collision_detection_distance": 0.1, "bound_relaxation": 0.0}
    prob = nat.NativeProblem(nmw, collision_limits=[col], max_batch=4)
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        prob.clearance(np.zeros((2, wide.nq)))
    prob.close(); nmw.close()
