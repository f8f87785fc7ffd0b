"""mkh_swept_clearance on the device against the numpy reference of tests/swept_ref.py (include/minkhip.h "THE RULE OF THE
SWEEP"): four edges per wavefront with a ragged last one, one edge per wavefront with slide joints and box-box pairs, a free
joint whose quaternion turns by a large angle and comes with either sign, an edge from a row to itself, non-finite ends, and the
refusal of a checker with general convex pairs.

Tolerance: margin to 1e-9 absolute (what tests/test_gpu_clearance.py holds a row's margin to); sample, pair and in_collision
exactly.  `sample` is an argmin over margins that agree to 1e-9, so — like the flags, which are thresholds on margins — it can be
exact only where the reference alone separates the smallest sample from the runner-up: a link whose distance to the floor does
not depend on the joints that move along an edge has the same margin at every sample but for rounding (the UR5e's shoulder
against the floor is one).  The edges are therefore the FIRST n of the fixture's rows, in order, whose reference margins keep the
two smallest samples more than 1e-6 apart and the smallest more than 1e-6 away from zero — a condition on the reference alone,
asserted to leave enough edges, and the number of candidates it drops is pinned per case (8 of 90, 1 of 10 and 3 of 12; none on
`shapes_wide` and with one sample), so the filter cannot silently grow; exact ties (lowest sample wins) are the business of the
row-to-itself test."""

import ctypes

import numpy as np
import pytest

import clearance_ref as cr
import swept_ref as sref

pytestmark = pytest.mark.gpu
TOL = 1e-9


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _checker(name, max_rows=256):
    import mink_amd
    model, _, _ = cr.fixture(name)
    return mink_amd.CollisionChecker(model, cr.fixture_limits(name), max_rows=max_rows)


def _limits(name):
    return cr.limits_of(cr.fixture_limits(name))


def _separated(ref, n, dropped):
    """The first n edges of a reference whose decision is not within 1e-6 of a tie; `dropped`: how many of the candidates are."""
    order = np.sort(ref.samples, axis=1)
    ok = np.abs(ref.margin) > 1e-6
    if ref.samples.shape[1] > 1:
        ok &= order[:, 1] - order[:, 0] > 1e-6
    keep = np.nonzero(ok)[0]
    assert int((~ok).sum()) == dropped, (np.nonzero(~ok)[0], dropped)
    assert len(keep) >= n, (len(keep), n)
    return keep[:n]


def _against_reference(name, a, b, M, n, dropped):
    """The first n separated edges among a -> b, against the reference."""
    model, _, _ = cr.fixture(name)
    full = sref.sweep(model, _limits(name), a, b, M)
    keep = _separated(full, n, dropped)
    a, b = np.ascontiguousarray(a[keep]), np.ascontiguousarray(b[keep])
    ref = sref.RefSweep(*[x[keep] for x in full])
    ck = _checker(name)
    out = ck.swept_clearance(a, b, n_samples=M)
    ck.close()
    err = np.abs(out.margin - ref.margin).max()
    order = np.sort(ref.samples, axis=1)
    gap = (order[:, 1] - order[:, 0]).min() if M > 1 else np.inf
    print("%s: %d edges x %d samples: max |margin - ref| %.2e, %d collide, min |ref margin| %.2e, min gap to the runner-up sample %.2e"
          % (name, len(a), M, err, int(ref.in_collision.sum()), np.abs(ref.margin).min(), gap))
    assert out.margin.shape == (len(a),) and out.sample.dtype == np.int32 and out.pair.dtype == np.int32
    assert out.in_collision.dtype == bool
    np.testing.assert_array_equal(out.sample, ref.sample)
    np.testing.assert_array_equal(out.pair, ref.pair)
    np.testing.assert_array_equal(out.in_collision, ref.in_collision)
    assert err <= TOL
    return ref, out, a, b


@pytest.mark.parametrize("M", [1, 7])
def test_small_arm_four_edges_per_wavefront(nat, M):
    """`ur5e_all`, 14 pairs on 16-lane rows: 50 edges — twelve full wavefronts and a ragged thirteenth."""
    _, _, q = cr.fixture("ur5e_all")
    ref = _against_reference("ur5e_all", q[:90], q[100:190], M, 50, {1: 0, 7: 8}[M])[0]
    assert 0 < ref.in_collision.sum() < 50


def test_one_edge_per_wavefront_slides_hinges_boxes(nat):
    """`shapes_wide`: 60 pairs (beyond a quarter wavefront), slide and hinge joints, every analytic pair family."""
    _, _, q = cr.fixture("shapes_wide")
    _against_reference("shapes_wide", q[:18], q[18:36], 5, 16, 0)


def test_free_joint_on_the_shortest_arc(nat):
    """`g1`: the base quaternion of q_to turned by a random rotation of up to about 2 rad and given as -q on half of the rows."""
    model, _, q = cr.fixture("g1")
    rng = np.random.default_rng(4)
    a, b = q[:12].copy(), q[12:24].copy()
    for i in range(12):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.5, 2.0)
        r = np.concatenate([[np.cos(0.5 * ang)], np.sin(0.5 * ang) * axis])
        w0, v0 = b[i, 3], b[i, 4:7]
        turned = np.concatenate([[w0 * r[0] - v0 @ r[1:]], w0 * r[1:] + r[0] * v0 + np.cross(v0, r[1:])])
        b[i, 3:7] = turned if i % 2 else -turned
    ref, out, a, b = _against_reference("g1", a, b, 3, 8, 3)
    # the sign of either end does not enter: the same edges with every q_to quaternion negated
    ck = _checker("g1")
    b2 = b.copy()
    b2[:, 3:7] *= -1.0
    again = ck.swept_clearance(a, b2, n_samples=3)
    ck.close()
    np.testing.assert_array_equal(again.sample, out.sample)
    np.testing.assert_array_equal(again.pair, out.pair)
    assert np.abs(again.margin - out.margin).max() <= TOL


def test_an_edge_from_a_row_to_itself_is_the_rows_clearance(nat):
    _, _, q = cr.fixture("ur5e_all")
    ck = _checker("ur5e_all")
    rows = q[:23]
    own = ck.clearance(rows)
    for M in (1, 4):
        out = ck.swept_clearance(rows, rows, n_samples=M)
        np.testing.assert_array_equal(out.margin, own.margin)         # bit for bit: a + u (a - a) = a, and the same row body
        np.testing.assert_array_equal(out.pair, own.pair)
        np.testing.assert_array_equal(out.in_collision, own.in_collision)
        assert (out.sample == 0).all()
    # leading shapes, one edge, device pointers
    grid = ck.swept_clearance(q[:12].reshape(3, 4, -1), q[12:24].reshape(3, 4, -1), n_samples=2)
    flat = ck.swept_clearance(q[:12], q[12:24], n_samples=2)
    assert grid.margin.shape == (3, 4) and grid.in_collision.shape == (3, 4)
    np.testing.assert_array_equal(grid.margin.ravel(), flat.margin)
    one = ck.swept_clearance(q[0], q[12], n_samples=2)
    assert one.margin.shape == () and one.margin == flat.margin[0] and one.sample == flat.sample[0]
    import torch
    dev = ck.swept_clearance(torch.as_tensor(q[:12], device="cuda"), torch.as_tensor(q[12:24], device="cuda"), n_samples=2)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in dev)
    for f in flat._fields:
        np.testing.assert_array_equal(getattr(dev, f).cpu().numpy(), getattr(flat, f), err_msg=f)
    ck.close()


@pytest.mark.parametrize("name", ["ur5e_all", "shapes_wide"])
def test_non_finite_ends(nat, name):
    """A NaN in q_from, an infinity in q_to: margin NaN, sample 0, pair 0, in collision — on both builds; the edges beside them
    in the same wavefront are untouched."""
    model, _, q = cr.fixture(name)
    keep = _separated(sref.sweep(model, _limits(name), q[:10], q[10:20], 3), 7, {"ur5e_all": 1, "shapes_wide": 0}[name])
    a, b = q[:10][keep].copy(), q[10:20][keep].copy()
    a[1, 0] = np.nan
    b[4, -1] = np.inf
    a[5, :] = -np.inf
    bad = np.array([1, 4, 5])
    good = np.setdiff1d(np.arange(7), bad)
    ref = sref.sweep(model, _limits(name), a, b, 3)
    assert np.isnan(ref.margin[bad]).all() and (ref.sample[bad] == 0).all() and (ref.pair[bad] == 0).all()
    ck = _checker(name)
    out = ck.swept_clearance(a, b, n_samples=3)
    ck.close()
    assert np.isnan(out.margin[bad]).all() and (out.sample[bad] == 0).all() and (out.pair[bad] == 0).all() and out.in_collision[bad].all()
    np.testing.assert_array_equal(out.sample[good], ref.sample[good])
    np.testing.assert_array_equal(out.pair[good], ref.pair[good])
    assert np.abs(out.margin[good] - ref.margin[good]).max() <= TOL


def test_general_convex_pairs_are_refused(nat):
    _, _, q = cr.fixture("ur5e_convex")
    ck = _checker("ur5e_convex")
    assert ck.clearance(q[:2]).margin.shape == (2,)                    # (a checker the clearance accepts)
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        ck.swept_clearance(q[:2], q[2:4], n_samples=2)
    prob = next(iter(ck._handles.values()))[1]
    io = nat.MkhSweptClearanceIO()
    buf = np.zeros(4)
    io.margin = io.sample = io.pair = buf.ctypes.data
    rows = np.ascontiguousarray(q[:2])
    assert nat.lib().mkh_swept_clearance(prob.handle, 1, rows.ctypes.data, rows.ctypes.data, 2, ctypes.byref(io), 0, None) == -1      # MKH_E_INVALID
    ck.close()
