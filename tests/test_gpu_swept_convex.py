"""Swept clearance and the checked ladder on checkers WITH general convex pairs (cylinder-box, cylinder-cylinder, ellipsoid-*:
`CollisionChecker(sweep_rows=)`, mkh_problem_set_sweep_rows, convex_sweep.hip) against the numpy references of tests/swept_ref.py and
tests/ladder_free_ref.py on the cases of tests/swept_convex_cases.py.

Tolerance: margins to 1e-9 absolute, the bound tests/test_gpu_clearance.py holds `ur5e_convex` rows to.  `sample`, `pair`,
`in_collision` and `edge_collision` exactly, on the edges the reference alone separates (tests/test_gpu_swept.py's rule: the smallest
sample's margin more than 1e-6 from zero and from the runner-up); the number of candidates that rule drops is pinned per case and
at most a quarter (tests/test_swept_convex_cpu.py holds the same counts without a GPU).  Outputs must not depend on `sweep_rows`:
every chunking is compared bit for bit."""

import numpy as np
import pytest

import clearance_ref as cr
import ladder_free_ref as lfref
import swept_convex_cases as sc

pytestmark = pytest.mark.gpu
TOL = 1e-9
SWEPT = ("margin", "sample", "pair", "in_collision")
LADDER_EXACT = ("node_index", "n_tracked", "n_breaks", "edge_break", "edge_collision", "n_edge_collisions")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _shapes_checker(sweep_rows, max_rows=256):
    import mink_amd
    model, spec, _ = sc.shapes()
    return mink_amd.CollisionChecker(model, sc.limit_objects(model, spec), max_rows=max_rows, sweep_rows=sweep_rows)


def _against_sweep(out, ref, keep, what):
    err = np.abs(out.margin[keep] - ref.margin[keep]).max()
    print("%s: %d kept edges of %d, max |margin - ref| %.2e, %d collide" % (what, len(keep), len(ref.margin), err,
                                                                          int(ref.in_collision[keep].sum())))
    for f in ("sample", "pair", "in_collision"):
        np.testing.assert_array_equal(np.asarray(getattr(out, f))[keep], getattr(ref, f)[keep], err_msg=f"{what}: {f}")
    assert err <= TOL, what


def _same(a, b, fields, what):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        x, y = [v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v) for v in (x, y)]
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {f}")


def test_swept_clearance_against_the_reference(nat):
    """`convex_shapes`: 32 edges x 3 samples, 15 pairs on 16-lane rows (four edges per wavefront), general convex and analytic
    pairs interleaved in the pair loop; sweep_rows = 64 holds 21 edges: two chunks."""
    a, b, ref, _ = sc.shapes_sweep()
    keep = sc.keep(ref, 0, 16)
    ck = _shapes_checker(64)
    out = ck.swept_clearance(a, b, n_samples=sc.N_SAMPLES)
    ck.close()
    assert out.margin.shape == (sc.N_EDGES,) and out.sample.dtype == np.int32 and out.pair.dtype == np.int32
    _against_sweep(out, ref, keep, "convex_shapes")
    conv = np.array([g for _, _, g in sc.PAIRS])
    assert conv[out.pair[keep]].any() and not conv[out.pair[keep]].all()


def test_outputs_do_not_depend_on_the_chunking(nat):
    """One chunk (3·32 rows), seven chunks with a ragged last one (3·5), one edge per chunk (3): bit for bit, with host arrays
    and with device tensors."""
    import torch
    a, b, _, _ = sc.shapes_sweep()
    ta, tb = torch.as_tensor(np.array(a), device="cuda"), torch.as_tensor(np.array(b), device="cuda")
    outs = {}
    for rows in (3 * 32, 3 * 5, 3):
        ck = _shapes_checker(rows)
        outs[rows] = ck.swept_clearance(a, b, n_samples=3)
        dev = ck.swept_clearance(ta, tb, n_samples=3)
        torch.cuda.synchronize()
        ck.close()
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in dev)
        _same(dev, outs[rows], SWEPT, "device tensors, sweep_rows = %d" % rows)
    for rows in (3 * 5, 3):
        _same(outs[rows], outs[3 * 32], SWEPT, "sweep_rows = %d" % rows)


def test_ur5e_convex_one_sample_per_edge(nat):
    """The real robot's chain depth: 43 edges between fixture rows near the wall, one sample each; the cylinder-box pair decides
    some of the kept ones."""
    import mink_amd
    model, _, _ = cr.fixture("ur5e_convex")
    a, b, ref = sc.ur5e_convex_edges()
    keep = sc.keep(ref, 0, 32)
    assert (ref.pair[keep] == sc.UR5E_CONVEX_PAIR).any()
    ck = mink_amd.CollisionChecker(model, cr.fixture_limits("ur5e_convex"), sweep_rows=16)
    out = ck.swept_clearance(a, b, n_samples=1)
    ck.close()
    _against_sweep(out, ref, keep, "ur5e_convex")


def test_free_joint_large_turns_and_both_signs(nat):
    """The quaternion branch of the per-lane blend: a floating body with three cylinders against boxes and cylinders, 4 edges x 2
    samples, q_to turned by 1.5 to 2.5 rad and given as -q on the odd edges; negating every q_to changes nothing."""
    import mink_amd
    model, spec, a, b, ref = sc.cans()
    keep = sc.keep(ref, 0, 4)
    ck = mink_amd.CollisionChecker(model, sc.limit_objects(model, spec), sweep_rows=4)
    out = ck.swept_clearance(a, b, n_samples=sc.CANS_SAMPLES)
    _against_sweep(out, ref, keep, "floating cans")
    b2 = b.copy()
    b2[:, 3:7] *= -1.0
    again = ck.swept_clearance(a, b2, n_samples=sc.CANS_SAMPLES)
    ck.close()
    np.testing.assert_array_equal(again.sample, out.sample)
    np.testing.assert_array_equal(again.pair, out.pair)
    assert np.abs(again.margin - out.margin).max() <= TOL


def test_non_finite_ends(nat):
    """A NaN in q_from, an infinity in q_to, a row of -inf: margin NaN, sample 0, pair 0, in collision, the call succeeds — the
    pre-pass skips those edges — and the other edges of the launch are what they are without them."""
    a, b, ref, _ = sc.shapes_sweep()
    a, b = a[:9].copy(), b[:9].copy()
    a[1, 0] = np.nan
    b[4, -1] = np.inf
    a[6, :] = -np.inf
    bad = np.array([1, 4, 6])
    good = np.setdiff1d(np.arange(9), bad)
    ck = _shapes_checker(12)
    out = ck.swept_clearance(a, b, n_samples=3)
    whole = ck.swept_clearance(*sc.shapes_sweep()[:2], n_samples=3)
    ck.close()
    assert np.isnan(out.margin[bad]).all() and (out.sample[bad] == 0).all() and (out.pair[bad] == 0).all() and out.in_collision[bad].all()
    for f in SWEPT:
        np.testing.assert_array_equal(getattr(out, f)[good], getattr(whole, f)[good], err_msg=f)
    keep = good[sc.separated(ref)[good]]
    assert len(keep) == len(good)
    _against_sweep(out, ref, keep, "beside non-finite ends")


def _ladder_against(out, want, what):
    for f in LADDER_EXACT:
        np.testing.assert_array_equal(np.asarray(getattr(out, f)).astype(np.int64), want[f].astype(np.int64), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(out.q, want["q_path"], err_msg=f"{what}: q")
    assert np.abs(out.path_length / want["path_length"] - 1.0).max() <= 1e-12
    for f in ("edge_margin", "node_margin", "edge_margin_all"):
        x, y = np.asarray(getattr(out, f), dtype=np.float64), want[f]
        np.testing.assert_array_equal(np.isnan(x), np.isnan(y), err_msg=f"{what}: {f}: NaN placement")
        np.testing.assert_array_equal(np.isinf(x), np.isinf(y), err_msg=f"{what}: {f}: inf placement")
        ok = np.isfinite(x)
        err = np.abs(x[ok] - y[ok]).max() if ok.any() else 0.0
        print("%s: %s: max |device - ref| %.2e over %d finite entries" % (what, f, err, int(ok.sum())))
        assert err <= TOL, (what, f)


@pytest.mark.parametrize("sparse", [False, True])
def test_ladder_path_against_the_reference(nat, sparse):
    """B, T, S = 2, 3, 3, two samples per edge, every node tracked or about half of them (edges into the others are not swept:
    the pre-pass skips them).  sweep_rows = 8: chunks of four edges, whose boundaries fall inside the 9 edges of one (b, t) —
    the first-edge offset in ladder mode; 72 rows hold every edge at once: bit for bit the same."""
    import mink_amd as mink
    model, _, _ = sc.shapes()
    q, q_nodes, trk, want = sc.ladder(sparse)
    em = want["edge_margin_all"]
    assert np.abs(em[np.isfinite(em)]).min() > 1e-6 and np.abs(want["node_margin"]).min() > 1e-6
    cfg = mink.Configuration(model, q.copy())
    outs = []
    for rows in (8, 72):
        ck = _shapes_checker(rows)
        outs.append(mink.ladder_path(cfg, q_nodes, trk, collision_check=ck, edge_samples=sc.LADDER_M))
        ck.close()
    _ladder_against(outs[0], want, "ladder_path, sparse = %s" % sparse)
    _same(outs[0], outs[1], outs[0]._fields, "sweep_rows 8 against 72")


B, T, S, K, M, ITERS = 2, 3, 4, 2, 2, 20
THR = (1e-4, 1e-4)


@pytest.mark.parametrize("n_nodes", [None, K])
def test_fused_ladder_call_on_ur5e_convex(nat, n_nodes):
    """solve_ik_trajectory_ladder(collision_check=) on `ur5e_convex`: q_all and the loops' outputs are the unchecked call's, bit for
    bit, and the checked fields are ladder_free_ref's on the returned rows."""
    import mink_amd as mink
    model, _, rows = cr.fixture("ur5e_convex")
    limits = cr.limits_of(cr.fixture_limits("ur5e_convex"))
    free_rows = rows[~cr.fixture_ref("ur5e_convex").in_collision][:B * T]
    tg = mink.Configuration(model, free_rows).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz.reshape(B, T, 7)
    home = np.tile(model.key_qpos[model.name2id("key", "home")], (B, 1))
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)

    def call(**kw):
        cfg = mink.Configuration(model, home.copy())
        return mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, S, ITERS, *THR, limits=[mink.ConfigurationLimit(model)],
                                               damping=1e-3, rng_seed=5, update=False, return_all=True, **kw)

    plain = call()
    ck = mink.CollisionChecker(model, cr.fixture_limits("ur5e_convex"), sweep_rows=10)      # (chunks of five edges)
    free = call(collision_check=ck, edge_samples=M, **({} if n_nodes is None else dict(n_nodes=n_nodes)))
    ck.close()
    if n_nodes is None:
        np.testing.assert_array_equal(free.q_all, plain.q_all)
        for f in ("v_all", "iters_all", "converged_all", "seeds"):
            np.testing.assert_array_equal(getattr(free, f), getattr(plain, f), err_msg=f)
        assert ((free.status_all & ~mink.ST_IN_COLLISION) == plain.status_all).all()
        node_trk = plain.converged_all & ((plain.status_all & ~1) == 0)
    else:
        node_trk = free.node_seed_index >= 0
    want = lfref.select(model, limits, home, free.q_all, node_trk, None, np.inf, M)
    em = want["edge_margin_all"]
    assert np.abs(em[np.isfinite(em)]).min() > 1e-6 and np.abs(want["node_margin"]).min() > 1e-6      # (the reference alone separates)
    for f in LADDER_EXACT:
        np.testing.assert_array_equal(np.asarray(getattr(free, f)).astype(np.int64), want[f].astype(np.int64), err_msg=f)
    np.testing.assert_array_equal(free.q, want["q_path"])
    x, y = np.asarray(free.edge_margin), want["edge_margin"]
    np.testing.assert_array_equal(np.isfinite(x), np.isfinite(y))
    assert np.abs(x[np.isfinite(x)] - y[np.isfinite(y)]).max(initial=0.0) <= TOL
    hit = (free.status_all & mink.ST_IN_COLLISION) != 0
    if n_nodes is None:
        np.testing.assert_array_equal(hit, ~(want["node_margin"] >= 0.0))
    print("n_nodes %s: %d swept edges, %d blocked, n_tracked %s, n_edge_collisions %s" %
          (n_nodes, int(np.isfinite(em).sum()), int(want["blocked"].sum()), free.n_tracked.tolist(), free.n_edge_collisions.tolist()))


def test_sweep_rows_changes_nothing_without_general_convex_pairs(nat):
    """`ur5e_all`: 14 capsule pairs, one launch whatever sweep_rows is."""
    import mink_amd
    model, _, q = cr.fixture("ur5e_all")
    outs = []
    for rows in (0, 64):
        ck = mink_amd.CollisionChecker(model, cr.fixture_limits("ur5e_all"), sweep_rows=rows)
        outs.append(ck.swept_clearance(q[:90], q[100:190], n_samples=7))       # (90 x 7 samples: far more than sweep_rows)
        ck.close()
    _same(outs[0], outs[1], SWEPT, "sweep_rows 64 against 0")


def test_less_than_one_edge_of_rows_is_a_limit(nat):
    a, b, _, _ = sc.shapes_sweep()
    ck = _shapes_checker(2)
    with pytest.raises(nat.MinkHipError, match=r"error -4: .*sweep_rows = 2 .*n_samples = 3"):
        ck.swept_clearance(a, b, n_samples=3)
    assert ck.swept_clearance(a, b, n_samples=2).margin.shape == (sc.N_EDGES,)
    # the handle itself: a negative size; 0 restores the refusal, its message naming the way out
    prob = next(iter(ck._handles.values()))[1]
    assert nat.lib().mkh_problem_set_sweep_rows(prob.handle, -1) == -1
    assert nat.lib().mkh_problem_set_sweep_rows(prob.handle, 1 << 62) == -4
    assert ck.swept_clearance(a, b, n_samples=2).margin.shape == (sc.N_EDGES,)       # (a refused size leaves the buffer alone)
    prob.set_sweep_rows(0)
    with pytest.raises(nat.MinkHipError, match="general convex pairs.*sweep_rows"):
        ck.swept_clearance(a, b, n_samples=2)
    assert nat.lib().mkh_problem_set_sweep_rows(None, 4) == -1
    ck.close()


def test_refinement_and_candidate_tracking_still_refuse(nat):
    """What they sweep is produced inside the same call: refused whatever sweep_rows is."""
    import mink_amd as mink
    cmodel, _, crow = cr.fixture("ur5e_convex")
    cck = mink.CollisionChecker(cmodel, cr.fixture_limits("ur5e_convex"), sweep_rows=4096)
    ccfg = mink.Configuration(cmodel, crow[0].copy())
    ctask = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    tg = mink.Configuration(cmodel, crow[:2]).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz.reshape(2, 7)
    assert cck.swept_clearance(crow[:2], crow[2:4], n_samples=2).margin.shape == (2,)        # (the checker sweeps)
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        mink.refine_path(ccfg, [ctask], 1.0, {ctask: tg}, crow[:2], collision_check=cck)
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        mink.solve_ik_trajectory_ladder(ccfg, [ctask], 1.0, {ctask: tg}, 2, 3, *THR, update=False, collision_check=cck, refine="free")
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        mink.solve_ik_trajectory_multistart(ccfg, [ctask], 1.0, {ctask: tg[:1]}, 2, 3, *THR, update=False, collision_check=cck)
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        mink.candidate_path(mink.Configuration(cmodel, crow[:1].copy()), crow[:6].reshape(1, 2, 3, -1), collision_check=cck)
    cck.close()
