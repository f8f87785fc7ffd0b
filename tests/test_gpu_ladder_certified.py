"""The certifying ladder on the device (include/minkhip.h THE RULE "with a certifying checker"): ladder_path(edge_resolution=...)
against the numpy reference of tests/ladder_certified_ref.py on the cases of tests/ladder_certified_cases.py, under both edge
policies; the chosen path's outputs against the arrays of every edge and, bit for bit, against checker.certified_sweep on the same
rows; solve_ik_trajectory_ladder(edge_resolution=...) — plain and on distinct nodes — against the composition of the calls it
fuses; T = 1, a non-finite node, wavefronts with nothing to sweep, device tensors, an unbatched configuration; the refusals.

Doubles to 1e-9 absolute (the project's tolerance for a margin) with the NaN and inf placement exact, path_length to 1e-12 relative
(tests/test_gpu_ladder.py's bound); every integer, byte and the path exactly.  The integers are thresholds of doubles that agree
only to 1e-9, so an instance is compared when the reference alone keeps every such threshold more than 1e-6 away
(ladder_certified_cases.comparable); the number of instances dropped is pinned per case — 0 in all of them.

Cases: A — `ur5e_all`, (B, T, S) = (4, 5, 4), four edges per wavefront at different counts; B — (1, 2, 3), nine edges: a ragged
last wavefront, S no multiple of 4; C — `shapes_wide`, (2, 3, 2), one edge per wavefront, slides and boxes; D — `ur5e_all`,
(3, 3, 2) at a larger spread, where REQUIRE_CERTIFIED loses waypoints that REJECT_COLLIDING keeps."""

import ctypes
import importlib

import numpy as np
import pytest

import clearance_ref as cr
import ladder_certified_cases as lc

pytestmark = pytest.mark.gpu
TOL = 1e-9
EXACT = ("node_index", "n_tracked", "n_breaks", "edge_break", "edge_collision", "n_edge_collisions", "edge_verdict", "edge_n_samples",
         "n_certified", "edge_verdict_all")
CLOSE = ("edge_margin", "edge_lower_bound", "node_margin", "edge_margin_all")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _checker(fixture, max_rows=4096, **kw):
    import mink_amd as mink
    model, _, _ = cr.fixture(fixture)
    return mink.CollisionChecker(model, cr.fixture_limits(fixture), max_rows=max_rows, **kw)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what}: NaN placement")
    np.testing.assert_array_equal(np.isinf(a), np.isinf(b), err_msg=f"{what}: inf placement")
    np.testing.assert_array_equal(a[np.isinf(a)], b[np.isinf(b)], err_msg=f"{what}: the sign of an infinity")
    ok = np.isfinite(a)
    err = np.abs(a[ok] - b[ok]).max() if ok.any() else 0.0
    print("%s: max |device - ref| %.2e over %d finite entries" % (what, err, int(ok.sum())))
    assert err <= TOL, what


def _edge_rows(q_nodes, idx):
    """(q_from, q_to) of the edges idx (n, 4): rows (b, t, s', s)."""
    return (np.stack([q_nodes[b, t - 1, s] for b, t, s1, s in idx]), np.stack([q_nodes[b, t, s1] for b, t, s1, s in idx]))


def _device_invariants(out, ck, q_nodes, resolution, mx, policy, what):
    """What holds of a result whatever the reference says: the chosen path's outputs are the arrays of every edge gathered along
    node_index; every swept edge is, bit for bit, checker.certified_sweep on its pair of rows; edge_collision is the mask's entry."""
    B, T, S = q_nodes.shape[:3]
    path = np.asarray(out.node_index)
    va, ma = np.asarray(out.edge_verdict_all), np.asarray(out.edge_margin_all)
    assert va.dtype == np.int8 and va.shape == (B, T, S, S) and ma.shape == (B, T, S, S)
    assert (va[:, 0] == -1).all() and np.isnan(ma[:, 0]).all()
    np.testing.assert_array_equal(va == -1, np.isnan(ma) & (va != 2), err_msg=f"{what}: unswept edges")
    assert (out.edge_verdict[:, 0] == -1).all() and np.isposinf(out.edge_margin[:, 0]).all() and np.isposinf(out.edge_lower_bound[:, 0]).all()
    assert (out.edge_n_samples[:, 0] == 0).all() and not np.asarray(out.edge_collision)[:, 0].any()
    blocked = (va != 1) & (va != -1) if policy else va == 2
    for b in range(B):
        for t in range(1, T):
            e = (b, t, path[b, t], path[b, t - 1])
            assert out.edge_verdict[b, t] == va[e], (what, e)
            np.testing.assert_array_equal(out.edge_margin[b, t], ma[e], err_msg=f"{what}: edge_margin {e}")
            assert bool(out.edge_collision[b, t]) == bool(blocked[e]), (what, e)
            if va[e] == -1:
                assert np.isnan(out.edge_lower_bound[b, t]) and out.edge_n_samples[b, t] == 0, (what, e)
    np.testing.assert_array_equal(out.n_edge_collisions, np.asarray(out.edge_collision).sum(axis=1), err_msg=what)
    np.testing.assert_array_equal(out.n_certified, (np.asarray(out.edge_verdict)[:, 1:] == 1).sum(axis=1), err_msg=what)
    # ---- every swept edge, and the chosen ones with their bounds and counts, against the stand-alone call
    idx = np.argwhere(va != -1)
    if len(idx):
        cs = ck.certified_sweep(*_edge_rows(q_nodes, idx), resolution, max_samples=mx)
        np.testing.assert_array_equal(ma[tuple(idx.T)], cs.margin, err_msg=f"{what}: edge_margin_all is certified_sweep's margin")
        np.testing.assert_array_equal(va[tuple(idx.T)], cs.verdict.astype(np.int8), err_msg=f"{what}: edge_verdict_all")
    chosen = np.array([(b, t, path[b, t], path[b, t - 1]) for b in range(B) for t in range(1, T) if out.edge_verdict[b, t] != -1]).reshape(-1, 4)
    if len(chosen):
        cs = ck.certified_sweep(*_edge_rows(q_nodes, chosen), resolution, max_samples=mx)
        at = (chosen[:, 0], chosen[:, 1])
        for f, g in (("edge_margin", "margin"), ("edge_lower_bound", "lower_bound"), ("edge_n_samples", "n_samples"), ("edge_verdict", "verdict")):
            np.testing.assert_array_equal(np.asarray(getattr(out, f))[at], getattr(cs, g), err_msg=f"{what}: {f} is certified_sweep's {g}")


def _against_reference(name, conditions, max_rows=4096):
    import mink_amd as mink
    c = lc.case(name)
    keep, st = c["keep"], c["stage"]
    conditions(c)
    q, q_nodes = c["q"][keep], c["q_nodes"][keep]
    cfg = mink.Configuration(c["model"], q.copy())
    ck = _checker(c["fixture"], max_rows)
    T = q_nodes.shape[1]
    for policy in (0, 1):
        want = c["select"][policy]
        out = mink.ladder_path(cfg, q_nodes, collision_check=ck, edge_resolution=c["resolution"], max_edge_samples=c["max_samples"],
                               require_certified=bool(policy))
        what = f"{name}, policy {policy}"
        assert isinstance(out, mink.CertifiedLadderPath) and out.edge_collision.dtype == bool
        assert out.edge_verdict.dtype == np.int32 and out.edge_n_samples.dtype == np.int32 and out.edge_lower_bound.dtype == np.float64
        for f in EXACT:
            np.testing.assert_array_equal(np.asarray(getattr(out, f)).astype(np.int64), want[f][keep].astype(np.int64), err_msg=f"{what}: {f}")
        np.testing.assert_array_equal(out.q, want["q_path"][keep], err_msg=f"{what}: q")
        assert np.abs(out.path_length / want["path_length"][keep] - 1.0).max() <= 1e-12
        for f in CLOSE:
            _close(getattr(out, f), want[f][keep], f"{what}: {f}")
        _device_invariants(out, ck, q_nodes, c["resolution"], c["max_samples"], policy, what)
        print("%s: n_tracked %s of %d, n_certified %s, n_edge_collisions %s" %
              (what, out.n_tracked.tolist(), T, out.n_certified.tolist(), out.n_edge_collisions.tolist()))
    ck.close()
    return c


def _verdicts(c):
    return set(c["stage"]["edge_verdict_all"][c["stage"]["swept"]].tolist())


def _differs(c):
    return (c["select"][0]["node_index"] != c["select"][1]["node_index"]).any(axis=1)


def test_case_a_four_edges_per_wavefront_at_their_own_counts(nat):
    def conditions(c):
        assert _verdicts(c) == {0, 1, 2}
        # (launch order is row-major over (b, t >= 1, s', s): with S = 4 a wavefront holds the four edges into one destination)
        n = c["stage"]["edge_n_samples_all"][:, 1:].reshape(-1, 4)
        assert ((n.max(axis=1) > n.min(axis=1)) & (n.min(axis=1) > 0)).any()
        assert n.max() == 16 and n[n > 0].min() == 1
        assert _differs(c)[0]
    _against_reference("A", conditions)


def test_case_b_a_ragged_last_wavefront(nat):
    def conditions(c):
        assert c["stage"]["swept"].sum() == 9                   # two full wavefronts and one edge in the third
    _against_reference("B", conditions)


def test_case_c_one_edge_per_wavefront(nat):
    def conditions(c):
        assert _verdicts(c) == {0, 1, 2}
        assert (~c["stage"]["swept"][:, 1:]).any()             # (wavefronts that sweep nothing, beside live ones)
    _against_reference("C", conditions)


def test_case_d_require_certified_loses_waypoints(nat):
    def conditions(c):
        T = c["q_nodes"].shape[1]
        assert _verdicts(c) == {0, 1, 2}
        assert (c["select"][1]["n_tracked"] < T).any() and (c["select"][0]["n_tracked"] == T).all()
    _against_reference("D", conditions)


# ------------------------------------------------------------------ the fused call
B, T, S, K, ITERS = 2, 3, 4, 3, 20
THR = (1e-4, 1e-4)
RULE = dict(edge_resolution=0.04, max_edge_samples=16)


def _world():
    """tests/test_gpu_ladder_free.py's set-up: the UR5e at `home`, a FrameTask whose waypoints are the end-effector poses of rows the
    reference finds free of collision."""
    import mink_amd as mink
    model, _, rows = cr.fixture("ur5e_all")
    free = rows[~cr.fixture_ref("ur5e_all").in_collision][:B * T]
    tg = mink.Configuration(model, free).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz.reshape(B, T, 7)
    home = np.tile(model.key_qpos[model.name2id("key", "home")], (B, 1))
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    return model, home, task, tg


def _call(model, home, task, tg, **kw):
    import mink_amd as mink
    cfg = mink.Configuration(model, home.copy())
    return cfg, mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, S, ITERS, *THR, limits=[mink.ConfigurationLimit(model)],
                                                damping=1e-3, rng_seed=5, update=False, return_all=True, **kw)


@pytest.mark.parametrize("n_nodes", [None, K])
@pytest.mark.parametrize("require", [False, True])
def test_fused_call_is_the_composition(nat, n_nodes, require):
    """solve_ik_trajectory_ladder(edge_resolution=...) bit for bit: the plain call's return_all, the clearance of those rows,
    (distinct_solutions on the free tracked results,) ladder_path(edge_resolution=...)."""
    import mink_amd as mink
    model, home, task, tg = _world()
    nq = model.nq
    ck = _checker("ur5e_all")
    cfg, plain = _call(model, home, task, tg)
    rule = dict(RULE, require_certified=require)
    _, got = _call(model, home, task, tg, collision_check=ck, **rule, **({} if n_nodes is None else dict(n_nodes=n_nodes)))
    assert isinstance(got, mink.CertifiedLadderResult if n_nodes is None else mink.CertifiedLadderNodesResult)
    clr = ck.clearance(plain.q_all)
    status = plain.status_all | np.where(clr.in_collision, mink.ST_IN_COLLISION, 0).astype(plain.status_all.dtype)
    trk = plain.converged_all & ((status & ~1) == 0)
    if n_nodes is None:
        np.testing.assert_array_equal(got.q_all, plain.q_all)
        np.testing.assert_array_equal(got.status_all, status)
        nodes, node_trk = plain.q_all, plain.converged_all & ((plain.status_all & ~1) == 0)
    else:
        bt = mink.Configuration(model, np.repeat(home, T, axis=0))
        sel = mink.distinct_solutions(bt, plain.q_all.reshape(B * T, S, nq), trk.reshape(B * T, S), n_solutions=K, min_distance=0.1)
        nodes, node_trk = sel.q.reshape(B, T, K, nq), (sel.seed_index >= 0).reshape(B, T, K)
        np.testing.assert_array_equal(got.q_all, nodes)
        np.testing.assert_array_equal(got.node_seed_index, sel.seed_index.reshape(B, T, K))
    path = mink.ladder_path(cfg, nodes, node_trk, collision_check=ck, **rule)
    for f in ("node_index", "n_tracked", "n_breaks", "path_length", "edge_break", "q", "edge_collision", "n_edge_collisions", "edge_margin",
              "edge_verdict", "edge_lower_bound", "edge_n_samples", "n_certified"):
        np.testing.assert_array_equal(getattr(got, f), getattr(path, f), err_msg=f)
    assert (got.edge_verdict[:, 1:] != -1).any()
    print("n_nodes %s, require_certified %s: n_tracked %s, n_certified %s, verdicts %s" %
          (n_nodes, require, got.n_tracked.tolist(), got.n_certified.tolist(), got.edge_verdict.tolist()))
    ck.close()


# ------------------------------------------------------------------ edge cases
def _small():
    """Case D's nodes: (model, q, q_nodes (3, 3, 2, nq), resolution, max_samples)."""
    c = lc.case("D")
    return c["model"], c["q"], c["q_nodes"], c["resolution"], c["max_samples"]


def test_a_single_waypoint(nat):
    import mink_amd as mink
    model, q, q_nodes, res, mx = _small()
    ck = _checker("ur5e_all")
    cfg = mink.Configuration(model, q.copy())
    nodes = np.ascontiguousarray(q_nodes[:, :1])
    out = mink.ladder_path(cfg, nodes, collision_check=ck, edge_resolution=res, max_edge_samples=mx, require_certified=True)
    sampled = mink.ladder_path(cfg, nodes, collision_check=ck)
    for f in ("node_index", "n_tracked", "n_breaks", "path_length", "q", "node_margin"):
        np.testing.assert_array_equal(getattr(out, f), getattr(sampled, f), err_msg=f)
    assert np.isposinf(out.edge_margin).all() and np.isposinf(out.edge_lower_bound).all() and (out.edge_verdict == -1).all()
    assert (out.edge_n_samples == 0).all() and (out.n_certified == 0).all() and not out.edge_collision.any()
    assert (out.edge_verdict_all == -1).all() and np.isnan(out.edge_margin_all).all()
    ck.close()


def test_a_non_finite_node(nat):
    """A NaN in node (1, 0) of instance 0: the node is not tracked and no edge into it is swept; the edges that LEAVE it into
    tracked nodes are swept and collide — margin NaN, one sample — under either policy; the other instances are untouched."""
    import mink_amd as mink
    model, q, q_nodes, res, mx = _small()
    ck = _checker("ur5e_all")
    cfg = mink.Configuration(model, q.copy())
    bad = q_nodes.copy()
    bad[0, 1, 0, 2] = np.nan
    for policy in (False, True):
        kw = dict(collision_check=ck, edge_resolution=res, max_edge_samples=mx, require_certified=policy)
        clean, out = mink.ladder_path(cfg, q_nodes, **kw), mink.ladder_path(cfg, bad, **kw)
        assert np.isnan(out.node_margin[0, 1, 0]) and (out.edge_verdict_all[0, 1, 0] == -1).all()
        into = out.node_margin[0, 2] >= 0.0                     # the tracked destinations behind the bad node
        assert into.any()
        assert (out.edge_verdict_all[0, 2, into, 0] == 2).all() and np.isnan(out.edge_margin_all[0, 2, into, 0]).all()
        for f in out._fields:
            np.testing.assert_array_equal(getattr(out, f)[1:], getattr(clean, f)[1:], err_msg=f)
        _device_invariants(out, ck, bad, res, mx, int(policy), "a NaN node")
    ck.close()


def test_sparse_tracked_flags_leave_wavefronts_with_nothing_to_sweep(nat):
    """Case A's nodes with the caller's flags cleared on whole rungs and on single nodes: a wavefront — the four edges into one
    destination — then sweeps nothing and leaves early, beside wavefronts that sweep; a rung without a tracked node."""
    import mink_amd as mink
    c = lc.case("A")
    q, q_nodes, res, mx = c["q"], c["q_nodes"], c["resolution"], c["max_samples"]
    trk = np.ones(q_nodes.shape[:3], dtype=bool)
    trk[:, 2] = False
    trk[0, 1, 1:] = False
    trk[1, 3, ::2] = False
    trk[2] = False
    ck = _checker("ur5e_all")
    cfg = mink.Configuration(c["model"], q.copy())
    full = mink.ladder_path(cfg, q_nodes, collision_check=ck, edge_resolution=res, max_edge_samples=mx)
    out = mink.ladder_path(cfg, q_nodes, trk, collision_check=ck, edge_resolution=res, max_edge_samples=mx)
    eff = trk & (out.node_margin >= 0.0)
    swept = out.edge_verdict_all != -1
    np.testing.assert_array_equal(swept[:, 1:], np.broadcast_to(eff[:, 1:, :, None], swept[:, 1:].shape))
    assert not swept[2].any() and (out.edge_verdict[2] == -1).all() and np.isnan(out.edge_margin[2, 1:]).all() and out.n_tracked[2] == 0
    # a swept edge does not depend on what else its wavefront, or the launch, sweeps
    np.testing.assert_array_equal(out.edge_verdict_all[swept], full.edge_verdict_all[swept])
    np.testing.assert_array_equal(out.edge_margin_all[swept], full.edge_margin_all[swept])
    np.testing.assert_array_equal(out.node_margin, full.node_margin)
    _device_invariants(out, ck, q_nodes, res, mx, 0, "sparse flags")
    ck.close()


def test_device_tensors_and_an_unbatched_configuration(nat):
    import torch
    import mink_amd as mink
    from mink_amd.tasks import PostureTask
    sik = importlib.import_module("mink_amd.solve_ik")         # (the package attribute of that name is the function)
    model, q, q_nodes, res, mx = _small()
    ck = _checker("ur5e_all")
    cfg = mink.Configuration(model, q.copy())
    kw = dict(collision_check=ck, edge_resolution=res, max_edge_samples=mx, require_certified=True)
    out = mink.ladder_path(cfg, q_nodes, **kw)
    one = mink.ladder_path(mink.Configuration(model, q[1].copy()), q_nodes[1], **kw)
    assert isinstance(one, mink.CertifiedLadderPath) and one.node_index.shape == (3,) and one.edge_verdict_all.shape == (3, 2, 2)
    assert np.ndim(one.n_certified) == 0 and one.edge_lower_bound.shape == (3,)
    for f in out._fields:
        np.testing.assert_array_equal(getattr(one, f), getattr(out, f)[1], err_msg=f)
    # device pointers: the native call on torch tensors, asynchronous on the current stream
    prob, layout = sik._compile(cfg, [PostureTask(model, cost=1.0)], None, 1, devices=cfg.devices[:1])
    with sik._pin(cfg, layout):
        path, more = prob.ladder_select_certified(torch.as_tensor(q.copy(), device="cuda"), torch.as_tensor(q_nodes.copy(), device="cuda"),
                                                  ck, resolution=res, max_samples=mx, require_certified=True, return_margins=True)
        torch.cuda.synchronize()
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in tuple(path) + tuple(more))
    assert more.edge_verdict_all.dtype == torch.int8 and more.edge_verdict.dtype == torch.int32 and more.edge_lower_bound.dtype == torch.float64
    np.testing.assert_array_equal(path.node_index.cpu().numpy(), out.node_index)
    np.testing.assert_array_equal(path.n_tracked.cpu().numpy(), out.n_tracked)
    for f in nat.LADDER_FREE_IO_FIELDS + nat.LADDER_CERTIFIED_IO_FIELDS:
        np.testing.assert_array_equal(getattr(more, f).cpu().numpy().astype(np.float64), np.asarray(getattr(out, f)).astype(np.float64), err_msg=f)
    ck.close()


# ------------------------------------------------------------------ refusals
def test_refusals_of_the_keywords(nat):
    import mink_amd as mink
    model, q, q_nodes, res, mx = _small()
    ck = _checker("ur5e_all")
    cfg = mink.Configuration(model, q.copy())
    with pytest.raises(ValueError, match="edge_samples"):
        mink.ladder_path(cfg, q_nodes, collision_check=ck, edge_resolution=res, edge_samples=4)
    with pytest.raises(ValueError, match="collision_check"):
        mink.ladder_path(cfg, q_nodes, edge_resolution=res)
    with pytest.raises(ValueError, match="edge_resolution"):
        mink.ladder_path(cfg, q_nodes, collision_check=ck, require_certified=True)
    for bad in (0.0, -0.02, np.nan, np.inf):
        with pytest.raises(ValueError, match="edge_resolution must be finite and > 0"):
            mink.ladder_path(cfg, q_nodes, collision_check=ck, edge_resolution=bad)
    for bad in (0, 4097):
        with pytest.raises(ValueError, match=r"max_edge_samples must be in \[1, 4096\]"):
            mink.ladder_path(cfg, q_nodes, collision_check=ck, edge_resolution=res, max_edge_samples=bad)
    wmodel, home, task, tg = _world()
    for refine in (True, "free"):
        with pytest.raises(ValueError, match="refinement pass still samples .* follow-up"):
            _call(wmodel, home, task, tg, collision_check=ck, refine=refine, **RULE)
    with pytest.raises(ValueError, match="edge_samples"):
        _call(wmodel, home, task, tg, collision_check=ck, edge_samples=5, **RULE)
    with pytest.raises(ValueError, match="collision_check"):
        _call(wmodel, home, task, tg, **RULE)
    # a checker with general convex pairs, whatever its sweep_rows
    cmodel, _, crow = cr.fixture("ur5e_convex")
    for rows in (0, 64):
        cck = mink.CollisionChecker(cmodel, cr.fixture_limits("ur5e_convex"), sweep_rows=rows)
        ccfg = mink.Configuration(cmodel, crow[:1].copy())
        with pytest.raises(nat.MinkHipError, match=r"error -1: mkh_ladder_select_certified: the checker has general convex pairs .* not certified yet"):
            mink.ladder_path(ccfg, crow[:6].reshape(1, 3, 2, -1), collision_check=cck, edge_resolution=res)
        cck.close()
    ck.close()


def test_refusals_of_the_entry_points(nat):
    import mink_amd as mink
    from mink_amd.tasks import PostureTask
    sik = importlib.import_module("mink_amd.solve_ik")
    model, q, q_nodes, res, mx = _small()
    Bn, Tn, Sn = q_nodes.shape[:3]
    ck = _checker("ur5e_all")
    cfg = mink.Configuration(model, q.copy())
    prob, layout = sik._compile(cfg, [PostureTask(model, cost=1.0)], None, 1, devices=cfg.devices[:1])
    native = ck._native_for(prob)
    L = nat.lib()
    buf = np.zeros(Bn * Tn * Sn * Sn + 8)
    io, fio, cio = nat.MkhLadderIO(), nat.MkhLadderFreeIO(), nat.MkhLadderCertifiedIO()
    for f in ("node_index", "n_tracked", "n_breaks", "path_length", "edge_break"):
        setattr(io, f, buf.ctypes.data)
    for f in ("edge_collision", "n_edge_collisions", "edge_margin"):
        setattr(fio, f, buf.ctypes.data)
    for f in ("edge_verdict", "edge_lower_bound", "edge_n_samples", "n_certified"):
        setattr(cio, f, buf.ctypes.data)
    trk = np.ones((Bn, Tn, Sn), np.int32)
    nodes = np.ascontiguousarray(q_nodes)

    def select(resolution=res, max_samples=mx, policy=0, cert=cio, S=Sn, flags=0):
        return L.mkh_ladder_select_certified(prob.handle, native.handle, Bn, Tn, S, q.ctypes.data, nodes.ctypes.data, trk.ctypes.data, None,
                                             float("inf"), resolution, max_samples, policy, ctypes.byref(io), ctypes.byref(fio),
                                             None if cert is None else ctypes.byref(cert), flags, None)
    with sik._pin(cfg, layout):
        assert select() == 0
        for policy in (-1, 2):
            assert select(policy=policy) == -1 and b"edge_policy = %d" % policy in L.mkh_last_error()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert select(resolution=bad) == -1 and b"must be finite and > 0" in L.mkh_last_error()
        for bad in (0, 4097):
            assert select(max_samples=bad) == -1 and b"must be in [1, 4096]" in L.mkh_last_error()
        assert select(cert=None) == -1 and b"certified_io and its outputs" in L.mkh_last_error()
        hole = nat.MkhLadderCertifiedIO()
        hole.edge_verdict = hole.edge_lower_bound = hole.edge_n_samples = buf.ctypes.data
        assert select(cert=hole) == -1 and b"n_certified are required" in L.mkh_last_error()
        assert select(S=257) != 0                                # (what mkh_ladder_select_free refuses: the shape)
        assert select(flags=nat.FLAG_UNWIND_TURNS) == -1
    # the fused entry point: a refinement, n_nodes without its outputs, a policy
    wmodel, home, task, tg = _world()
    wcfg = mink.Configuration(wmodel, home.copy())
    wprob, wlayout = sik._compile(wcfg, [task], None, 1, devices=wcfg.devices[:1])
    wnative = ck._native_for(wprob)
    tio, rio = nat.MkhTrajectoryLadderIO(), nat.MkhLadderRefineIO()
    args = lambda k, nodes_io, refine, policy: (wprob.handle, wnative.handle, B, T, S, k, 0.1, None, None, None, None, 1.0, 1e-3, ITERS, 1e-4,
                                                1e-4, 0, 0, 0.04, 16, policy, ctypes.byref(tio), nodes_io, refine, ctypes.byref(fio),
                                                ctypes.byref(cio), 0, None)
    with sik._pin(wcfg, wlayout):
        assert L.mkh_solve_trajectory_ladder_certified(*args(0, None, ctypes.byref(rio), 0)) == -1
        assert b"refinement pass still samples" in L.mkh_last_error() and b"refine must be NULL" in L.mkh_last_error()
        assert L.mkh_solve_trajectory_ladder_certified(*args(K, None, None, 0)) == -1 and b"n_nodes" in L.mkh_last_error()
        assert L.mkh_solve_trajectory_ladder_certified(*args(0, None, None, 7)) == -1 and b"edge_policy = 7" in L.mkh_last_error()
    ck.close()
