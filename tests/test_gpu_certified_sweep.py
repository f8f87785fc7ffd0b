"""mkh_certified_sweep on the device against the numpy reference of tests/certified_ref.py (include/minkhip.h "THE RULE OF THE
CERTIFIED SWEEP"): four edges per wavefront whose groups take different sample counts, with a ragged last wavefront; one edge per
wavefront with slide joints, box-box pairs and a negative minimum distance; a free joint on the shortest arc; the reach table; the
device's own clearance and sweep; the certificate on dense device rows; an edge from a row to itself; non-finite ends; an
unlimited slide; max_samples = 1; leading shapes and device tensors; the refusals.

Tolerances: doubles to 1e-9 absolute (the project's tolerance for a margin), the reach table to 1e-12 relative, integers and
verdicts exactly.  The integers are thresholds and argmins of doubles that agree only to 1e-9, so the compared edges of a case are
the FIRST n of its candidates that pass four conditions on the reference alone: |margin| > 1e-6; |lower_bound| > 1e-6; the two
smallest entries of each minimum more than 1e-6 apart or exactly equal — held for EVERY entry within 1e-6 of the smallest, not only
the runner-up (pairs at their detection cap are equal bit for bit: the lowest index wins on both sides) —; motion / resolution more than 1e-6 from an integer.  The number of candidates dropped is pinned per case and is at most
a quarter of them, so the filter cannot silently grow.

Edges: the fixtures' own row pairs, shortened to b = a (+) s (b0 (-) a) — the raw pairs span the whole joint range (motion 11 .. 27 m
on the UR5e, 35 of 40 collide)."""

import ctypes

import numpy as np
import pytest

import certified_ref as cf
import clearance_ref as cr
import keyframe_ref as kf
from tree_cases import CERTIFIED_COMPARED as TREE_N, CERTIFIED_DROPPED as TREE_DROPPED

pytestmark = pytest.mark.gpu
TOL = 1e-9
DOUBLES = ("margin", "lower_bound", "motion")
INTS = ("sample", "pair", "segment", "bound_pair", "n_samples", "capped", "verdict")


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


def _limits(name):
    return cr.limits_of(cr.fixture_limits(name))


def _shortened(model, a, b0, s):
    return np.stack([kf.blend_posture(model, x, y, s) for x, y in zip(a, b0)])


def _minimum_is_separated(x):
    """Every entry is more than 1e-6 above the smallest or exactly equal to it.  (The two smallest alone do not settle an argmin: a
    link whose distance does not depend on the joints that move has one margin at every point but for rounding — two points equal
    bit for bit and a third an ulp beside them, at a lower index.)"""
    v = np.asarray(x).ravel()
    near = v[v - v.min() <= 1e-6]
    return bool((near == v.min()).all())


def comparable(ref, resolution):
    """(N,) bool: the edges of a reference whose integers do not hang on a difference below 1e-6."""
    ok = (np.abs(ref.margin) > 1e-6) & (np.abs(ref.lower_bound) > 1e-6)
    ratio = ref.motion / resolution
    ok &= ~np.isfinite(ratio) | (np.abs(ratio - np.round(ratio)) > 1e-6)
    for e in range(len(ok)):
        ok[e] &= _minimum_is_separated(ref.points[e]) and (ref.cones[e] is None or _minimum_is_separated(ref.cones[e]))
    return ok


def _g1_turned(q, rng):
    out = q.copy()
    for i in range(len(q)):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.5, 2.0)
        r = np.concatenate([[np.cos(0.5 * ang)], np.sin(0.5 * ang) * axis])
        w0, v0 = q[i, 3], q[i, 4:7]
        out[i, 3:7] = np.concatenate([[w0 * r[0] - v0 @ r[1:]], w0 * r[1:] + r[0] * v0 + np.cross(v0, r[1:])])
    return out


# name -> (fixture, rows of a, rows of b0, s, resolution, max_samples, compared, dropped)
CASES = {
    "ur5e_fine": ("ur5e_all", slice(0, 60), slice(100, 160), 0.05, 0.02, 64, 50, 3),
    "ur5e_coarse": ("ur5e_all", slice(0, 60), slice(100, 160), 0.1, 0.05, 64, 50, 2),
    "shapes_wide": ("shapes_wide", slice(0, 20), slice(20, 40), 0.2, 0.02, 64, 16, 0),
    "g1": ("g1", slice(0, 12), slice(12, 24), 0.1, 0.02, 64, 8, 0),
    # the random trees of tests/tree_cases.py (run by tests/test_gpu_tree_checker.py): ball and stacked joints, anchors off the body
    # origins, slides behind rotations; at max_samples = 4 most of the edges are capped
    "tree_small": ("tree_small", slice(0, 24), slice(24, 48), 0.3, 0.05, 64, TREE_N["tree_small"], TREE_DROPPED["tree_small"]),
    "tree_small_capped": ("tree_small", slice(0, 24), slice(24, 48), 0.3, 0.05, 4, TREE_N["tree_small_capped"], TREE_DROPPED["tree_small_capped"]),
    "tree_wide": ("tree_wide", slice(0, 16), slice(24, 40), 0.3, 0.05, 64, TREE_N["tree_wide"], TREE_DROPPED["tree_wide"]),
    "tree_wide_capped": ("tree_wide", slice(0, 16), slice(24, 40), 0.3, 0.05, 4, TREE_N["tree_wide_capped"], TREE_DROPPED["tree_wide_capped"]),
}
_case_cache = {}


def case(name):
    """(fixture, a, b, resolution, max_samples, RefCertified of ALL candidates, indices of the compared ones), computed once."""
    if name not in _case_cache:
        fixture, ia, ib, s, resolution, mx, n, dropped = CASES[name]
        model, _, q = cr.fixture(fixture)
        a, b0 = q[ia].copy(), q[ib].copy()
        if fixture == "g1":
            b0 = _g1_turned(b0, np.random.default_rng(4))
        b = _shortened(model, a, b0, s)
        if fixture == "g1":
            b[1::2, 3:7] *= -1.0                               # either sign of a quaternion is the same rotation
        ref = cf.certified_sweep(model, _limits(fixture), a, b, resolution, mx)
        ok = comparable(ref, resolution)
        assert int((~ok).sum()) == dropped, (name, np.nonzero(~ok)[0], dropped)
        assert 4 * dropped <= len(a) and ok.sum() >= n, (name, ok.sum(), n)
        for x in (a, b):
            x.setflags(write=False)
        _case_cache[name] = (fixture, a, b, resolution, mx, ref, np.nonzero(ok)[0][:n])
    return _case_cache[name]


def _against_reference(name):
    fixture, a, b, resolution, mx, full, keep = case(name)
    ck = _checker(fixture)
    out = ck.certified_sweep(a[keep], b[keep], resolution, max_samples=mx)
    ck.close()
    for f in DOUBLES:
        got, want = getattr(out, f), getattr(full, f)[keep]
        assert got.dtype == np.float64 and got.shape == (len(keep),)
        inf = np.isinf(want)
        np.testing.assert_array_equal(got[inf], want[inf], err_msg=f)
        err = np.abs(got[~inf] - want[~inf]).max()
        print("%s: %d edges: max |%s - ref| %.2e" % (name, len(keep), f, err))
        assert err <= TOL, (f, err)
    for f in INTS:
        assert getattr(out, f).dtype == np.int32
        np.testing.assert_array_equal(getattr(out, f), getattr(full, f)[keep], err_msg=f)
    np.testing.assert_array_equal(out.certified, out.verdict == 1)
    np.testing.assert_array_equal(out.in_collision, out.verdict == 2)
    assert out.certified.dtype == bool and out.in_collision.dtype == bool
    return out


def test_small_arm_four_edges_per_wavefront_with_their_own_counts(nat):
    """`ur5e_all`, 14 pairs on 16-lane rows: 50 edges — twelve full wavefronts and a ragged thirteenth —, the groups of a wavefront at
    different counts; at s = 0.05 / resolution 0.02 and at s = 0.1 / resolution 0.05, which has undecided edges."""
    fine, coarse = _against_reference("ur5e_fine"), _against_reference("ur5e_coarse")
    counts = fine.n_samples[:48].reshape(12, 4)
    assert (counts.max(axis=1) > counts.min(axis=1)).all()     # every full wavefront walks groups of different counts
    assert fine.n_samples.min() < 20 and fine.n_samples.max() == 64
    verdicts = set(fine.verdict.tolist()) | set(coarse.verdict.tolist())
    assert verdicts == {0, 1, 2} and (coarse.verdict == 0).sum() > 0
    assert fine.capped.sum() > 0                               # (the 53rd candidate, the last of the 50 compared)


def test_one_edge_per_wavefront_slides_boxes_negative_dmin(nat):
    """`shapes_wide`: 60 pairs (beyond a quarter wavefront), slide and hinge joints, box-box pairs, the second limit's dmin < 0."""
    _against_reference("shapes_wide")


def test_free_joint_on_the_shortest_arc(nat):
    """`g1`: the base quaternion of q_to turned by up to 2 rad and given as -q on every second row."""
    out = _against_reference("g1")
    fixture, a, b, resolution, mx, full, keep = case("g1")
    ck = _checker(fixture)
    b2 = b[keep].copy()
    b2[:, 3:7] *= -1.0
    again = ck.certified_sweep(a[keep], b2, resolution, max_samples=mx)
    ck.close()
    for f in INTS:
        np.testing.assert_array_equal(getattr(again, f), getattr(out, f), err_msg=f)
    for f in DOUBLES:
        assert np.abs(getattr(again, f) - getattr(out, f)).max() <= TOL


@pytest.mark.parametrize("name", ["ur5e_all", "shapes_wide", "g1"])
def test_reach_table_matches_the_reference(nat, name):
    model, _, _ = cr.fixture(name)
    limits = _limits(name)
    want = cf.reach_table(model, cr.pair_list(limits)[0])
    ck = _checker(name)
    got = ck.motion_reach()
    ck.close()
    assert got.shape == want.shape == (len(cr.pair_list(limits)[0]), model.njnt, 2)
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=0)
    assert (want[fin] > 0).any()


def margin_is_the_devices_own_clearance_and_sweep(name):
    """Every candidate edge of a case: min(clearance(q_from), swept_clearance at the edge's own n_samples, clearance(q_to)) is
    the certified sweep's margin to 1e-9 — the edges grouped by their count."""
    fixture, a, b, resolution, mx, _, _ = case(name)
    ck = _checker(fixture)
    out = ck.certified_sweep(a, b, resolution, max_samples=mx)
    ends = np.minimum(ck.clearance(a).margin, ck.clearance(b).margin)
    inner = np.full(len(a), np.nan)
    for M in np.unique(out.n_samples):
        of = np.nonzero(out.n_samples == M)[0]
        inner[of] = ck.swept_clearance(a[of], b[of], n_samples=int(M)).margin
    ck.close()
    err = np.abs(np.minimum(ends, inner) - out.margin).max()
    print("%s: %d edges, %d distinct counts: max |min(ends, sweep) - margin| %.2e" % (name, len(a), len(np.unique(out.n_samples)), err))
    assert err <= TOL


def test_margin_is_the_devices_own_clearance_and_sweep(nat):
    margin_is_the_devices_own_clearance_and_sweep("ur5e_fine")


def certified_edges_hold_on_dense_device_rows(name, at_least):
    """Device soundness: on the certified edges of a case (`at_least` of them), the device's clearance of 257 numpy-blended rows
    never falls below lower_bound - 1e-9."""
    fixture, a, b, resolution, mx, _, _ = case(name)
    model, _, _ = cr.fixture(fixture)
    ck = _checker(fixture)
    out = ck.certified_sweep(a, b, resolution, max_samples=mx)
    edges = np.nonzero(out.certified)[0]
    assert len(edges) >= at_least and (out.lower_bound[edges] >= 0.0).all()
    rows = np.stack([kf.blend_posture(model, a[e], b[e], float(i) / 256.0) for e in edges for i in range(257)])
    dense = ck.clearance(rows).margin.reshape(len(edges), 257).min(axis=1)
    ck.close()
    slack = (dense - out.lower_bound[edges]).min()
    print("%s: %d certified edges x 257 rows: smallest dense margin - lower_bound = %.3e" % (name, len(edges), slack))
    assert slack >= -TOL


def test_certified_edges_hold_on_dense_device_rows(nat):
    certified_edges_hold_on_dense_device_rows("ur5e_fine", 20)


def test_an_edge_from_a_row_to_itself(nat):
    _, _, q = cr.fixture("ur5e_all")
    ck = _checker("ur5e_all")
    rows = q[:23]
    own = ck.clearance(rows)
    out = ck.certified_sweep(rows, rows, 0.02)
    assert (out.motion == 0.0).all() and (out.n_samples == 1).all() and (out.capped == 0).all()
    np.testing.assert_array_equal(out.lower_bound, out.margin)          # bit for bit: three equal points, 1/2 ((m + m) - 0)
    np.testing.assert_array_equal(out.margin, own.margin)               # ... and a + u (a - a) = a: the row's own clearance
    np.testing.assert_array_equal(out.pair, own.pair)
    np.testing.assert_array_equal(out.verdict, np.where(own.margin >= 0.0, 1, 2))
    assert (out.sample == 0).all() and (out.segment == 0).all()
    assert 0 < out.certified.sum() < len(rows)
    ck.close()


@pytest.mark.parametrize("name", ["ur5e_all", "shapes_wide"])
def test_non_finite_ends(nat, name):
    """A NaN in q_from, an infinity in q_to, a row of -inf: the stated outputs, on both builds; the edges beside them in the same
    wavefront are untouched."""
    fixture, a, b, resolution, mx, full, keep = case({"ur5e_all": "ur5e_fine", "shapes_wide": "shapes_wide"}[name])
    keep = keep[:7]
    a, b = a[keep].copy(), b[keep].copy()
    a[1, 0] = np.nan
    b[4, -1] = np.inf
    a[5, :] = -np.inf
    bad = np.array([1, 4, 5])
    good = np.setdiff1d(np.arange(7), bad)
    ck = _checker(fixture)
    out = ck.certified_sweep(a, b, resolution, max_samples=mx)
    ck.close()
    for f in DOUBLES:
        assert np.isnan(getattr(out, f)[bad]).all(), f
        assert np.abs(getattr(out, f)[good] - getattr(full, f)[keep][good]).max() <= TOL, f
    for f in ("sample", "pair", "segment", "bound_pair", "capped"):
        assert (getattr(out, f)[bad] == 0).all(), f
    assert (out.n_samples[bad] == 1).all() and (out.verdict[bad] == 2).all() and out.in_collision[bad].all() and not out.certified[bad].any()
    for f in INTS:
        np.testing.assert_array_equal(getattr(out, f)[good], getattr(full, f)[keep][good], err_msg=f)


UNLIMITED_SLIDE_MJCF = """<mujoco><compiler angle="radian"/><worldbody>
  <geom name="floor" type="plane" size="1 1 0.1"/>
  <body name="turret" pos="0 0 0.4">
    <joint name="turn" type="hinge" axis="0 1 0" range="-1 1"/>
    <geom name="turret_g" type="sphere" size="0.05" mass="0.1"/>
    <body name="boom" pos="0.1 0 0">
      <joint name="reach" type="slide" axis="1 0 0"/>
      <geom name="boom_g" type="capsule" size="0.03 0.1" pos="0.15 0 0" mass="0.1"/>
    </body>
  </body>
  <body name="post" pos="0.6 0 0.3"><geom name="post_g" type="box" size="0.05 0.05 0.3" mass="1"/></body>
</worldbody></mujoco>"""


def test_unlimited_slide_below_a_hinge_is_unbounded(nat):
    """A hinge that carries a body on an unlimited slide: D of that body is infinite, so the hinge's reach is, and every edge that
    turns the hinge is UNBOUNDED — n_samples = max_samples, capped, lower_bound = -inf, never certified.  An edge that moves the
    slide alone has the slide's travel for its motion, and an edge that moves nothing has none: both are bounded."""
    import mink_amd
    from mink_amd.mjcf import loads_mjcf
    model = loads_mjcf(UNLIMITED_SLIDE_MJCF)
    gid = lambda n: model.name2id("geom", n)
    lim = mink_amd.CollisionAvoidanceLimit(model, geom_pairs=[([gid("boom_g")], [gid("post_g")]), ([gid("boom_g")], [gid("floor")])],
                                           minimum_distance_from_collisions=0.01, collision_detection_distance=0.3)
    ck = mink_amd.CollisionChecker(model, [lim], max_rows=16)
    limits = cr.limits_of([lim])
    table, want = ck.motion_reach(), cf.reach_table(model, cr.pair_list(limits)[0])
    np.testing.assert_array_equal(table, want)                  # (0, inf) for the hinge, (1, 0) for the slide, on both pairs
    assert np.isinf(table[:, 0, 1]).all() and (table[:, 1] == [1.0, 0.0]).all()
    a = np.array([[0.0, 0.1], [0.05, -0.2], [0.0, 0.0], [0.1, 0.0]])
    b = np.array([[0.1, 0.3], [0.0, 0.2], [0.0, 0.0], [0.1, 0.05]])
    out = ck.certified_sweep(a, b, 0.02, max_samples=12)
    ref = cf.certified_sweep(model, limits, a, b, 0.02, 12)
    ck.close()
    for f in ("n_samples", "capped", "verdict"):
        np.testing.assert_array_equal(getattr(out, f), getattr(ref, f), err_msg=f)
    assert np.abs(out.margin - ref.margin).max() <= TOL
    assert (out.n_samples[:2] == 12).all() and (out.capped[:2] == 1).all() and (out.motion[:2] == np.inf).all()
    assert (out.lower_bound[:2] == -np.inf).all() and (out.segment[:2] == 0).all() and (out.bound_pair[:2] == 0).all()
    assert not (out.verdict == 1)[:2].any() and not out.certified[:2].any()
    assert out.motion[2] == 0.0 and out.n_samples[2] == 1 and out.lower_bound[2] == out.margin[2]
    assert abs(out.motion[3] - 0.05) <= TOL and out.n_samples[3] == 2 and out.capped[3] == 0
    assert np.abs(out.lower_bound[2:] - ref.lower_bound[2:]).max() <= TOL


def test_max_samples_one(nat):
    """Every edge at one interior sample: three points, two segments; capped wherever the resolution asked for more."""
    fixture, a, b, resolution, _, _, _ = case("ur5e_fine")
    model, _, _ = cr.fixture(fixture)
    ref = cf.certified_sweep(model, _limits(fixture), a[:12], b[:12], resolution, 1)
    keep = np.nonzero(comparable(ref, resolution))[0]
    assert len(keep) >= 9
    ck = _checker(fixture)
    out = ck.certified_sweep(a[:12][keep], b[:12][keep], resolution, max_samples=1)
    ck.close()
    assert (out.n_samples == 1).all() and (out.capped == 1).all() and (out.sample <= 2).all() and (out.segment <= 1).all()
    for f in INTS:
        np.testing.assert_array_equal(getattr(out, f), getattr(ref, f)[keep], err_msg=f)
    for f in DOUBLES:
        assert np.abs(getattr(out, f) - getattr(ref, f)[keep]).max() <= TOL, f


def test_leading_shapes_single_edge_device_tensors(nat):
    fixture, a, b, resolution, mx, _, _ = case("ur5e_fine")
    ck = _checker(fixture)
    flat = ck.certified_sweep(a[:12], b[:12], resolution, max_samples=mx)
    grid = ck.certified_sweep(a[:12].reshape(3, 4, -1), b[:12].reshape(3, 4, -1), resolution, max_samples=mx)
    for f in flat._fields:
        assert getattr(grid, f).shape == (3, 4), f
        np.testing.assert_array_equal(getattr(grid, f).ravel(), getattr(flat, f), err_msg=f)
    one = ck.certified_sweep(a[5], b[5], resolution, max_samples=mx)
    for f in flat._fields:
        assert getattr(one, f).shape == () and np.array_equal(getattr(one, f), getattr(flat, f)[5], equal_nan=True), f
    import torch
    dev = ck.certified_sweep(torch.as_tensor(a[:12].copy(), device="cuda"), torch.as_tensor(b[:12].copy(), device="cuda"), resolution, max_samples=mx)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in dev)
    assert dev.certified.dtype == torch.bool and dev.verdict.dtype == torch.int32 and dev.margin.dtype == torch.float64
    for f in flat._fields:
        np.testing.assert_array_equal(getattr(dev, f).cpu().numpy(), getattr(flat, f), err_msg=f)
    ck.close()


def test_refusals(nat):
    _, _, q = cr.fixture("ur5e_convex")
    for rows in (0, 64):
        ck = _checker("ur5e_convex", sweep_rows=rows)
        assert ck.clearance(q[:2]).margin.shape == (2,)                # (a checker the clearance accepts)
        with pytest.raises(nat.MinkHipError, match=r"error -1: mkh_certified_sweep: the checker has general convex pairs .* not certified yet"):
            ck.certified_sweep(q[:2], q[2:4], 0.02)
        assert ck.motion_reach().shape == (ck.n_pairs, ck.model.njnt, 2)   # (the table itself serves any pair list)
        ck.close()
    fixture, a, b, _, _, _, _ = case("ur5e_fine")
    ck = _checker(fixture)
    for resolution in (0.0, -0.02, np.nan, np.inf):
        with pytest.raises(nat.MinkHipError, match=r"error -1: mkh_certified_sweep: resolution = .* must be finite and > 0"):
            ck.certified_sweep(a[:2], b[:2], resolution)
    for mx in (0, 4097):
        with pytest.raises(nat.MinkHipError, match=r"error -1: mkh_certified_sweep: max_samples = %d must be in \[1, 4096\]" % mx):
            ck.certified_sweep(a[:2], b[:2], 0.02, max_samples=mx)
    assert ck.certified_sweep(a[:2], b[:2], 0.02, max_samples=4096).margin.shape == (2,)
    # the C entry point itself: N < 1, a flag it does not know, a missing output
    prob = next(iter(ck._handles.values()))[1]
    io = nat.MkhCertifiedSweepIO()
    buf = np.zeros(8)
    for f in nat.CERTIFIED_SWEEP_FIELDS:
        setattr(io, f, buf.ctypes.data)
    rows = np.ascontiguousarray(a[:1])
    call = lambda N, flags: nat.lib().mkh_certified_sweep(prob.handle, N, rows.ctypes.data, rows.ctypes.data, 0.02, 8, ctypes.byref(io), flags, None)
    assert call(0, 0) == -1 and b"N = 0 must be >= 1" in nat.lib().mkh_last_error()
    assert call(1, 4) == -1 and b"only MKH_FLAG_DEVICE_PTRS is accepted" in nat.lib().mkh_last_error()
    io.motion = None
    assert call(1, 0) == -1 and b"ten outputs are required" in nat.lib().mkh_last_error()
    ck.close()
