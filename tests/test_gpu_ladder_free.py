"""The checked ladder on the device (include/minkhip.h THE RULE "with a checker"): ladder_path(collision_check=...) against the
numpy reference of tests/ladder_free_ref.py on the shared case of tests/swept_cases.py, a rung beyond one destination pass, a
neutral checker against the plain call, and solve_ik_trajectory_ladder(collision_check=...) — plain and on distinct nodes —
against the composition of the calls it fuses.

Integers exactly; margins to 1e-9 absolute with the NaN placement exact; path_length to 1e-12 relative, the bound
tests/test_gpu_ladder.py holds it to.  The shared case keeps every reference margin more than 1e-6 away from zero
(tests/test_swept_cpu.py asserts it), so no flag is excluded."""

import numpy as np
import pytest

import clearance_ref as cr
import ladder_free_ref as lfref
import swept_cases as sc

pytestmark = pytest.mark.gpu
TOL = 1e-9
EXACT = ("node_index", "n_tracked", "n_breaks", "edge_break", "edge_collision", "n_edge_collisions")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _checker(neutral=False):
    import mink_amd as mink
    model, spec, _ = cr.fixture("ur5e_all")
    if neutral:                            # no configuration is closer than -10 m to anything
        spec = [dict(kw, minimum_distance_from_collisions=-10.0) for kw in spec]
    return mink.CollisionChecker(model, [mink.CollisionAvoidanceLimit(model, **kw) for kw in spec], max_rows=4096)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what}: NaN placement")
    np.testing.assert_array_equal(np.isinf(a), np.isinf(b), err_msg=f"{what}: inf placement")
    ok = np.isfinite(a)
    err = np.abs(a[ok] - b[ok]).max() if ok.any() else 0.0
    print("%s: max |device - ref| %.2e over %d finite entries" % (what, err, int(ok.sum())))
    assert err <= TOL, what


def _against_reference(out, want, what):
    for f in EXACT:
        np.testing.assert_array_equal(np.asarray(getattr(out, f)).astype(np.int64), want[f].astype(np.int64), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(out.q, want["q_path"], err_msg=f"{what}: q")
    assert np.abs(out.path_length / want["path_length"] - 1.0).max() <= 1e-12
    _close(out.edge_margin, want["edge_margin"], f"{what}: edge_margin")
    _close(out.node_margin, want["node_margin"], f"{what}: node_margin")
    _close(out.edge_margin_all, want["edge_margin_all"], f"{what}: edge_margin_all")


def test_ladder_path_against_the_reference(nat):
    """UR5e, B = 4, T = 5, S = 4, M = 7: colliding nodes, blocked and unswept edges, paths the mask changes, a lost waypoint."""
    import mink_amd as mink
    (model, limits, q, q_nodes), _, want = sc.ladder_ref()
    cfg = mink.Configuration(model, q.copy())
    ck = _checker()
    out = mink.ladder_path(cfg, q_nodes, collision_check=ck, edge_samples=7)
    assert isinstance(out, mink.FreeLadderPath) and out.edge_collision.dtype == bool and out.edge_margin_all.shape == (4, 5, 4, 4)
    _against_reference(out, want, "ladder_path")
    assert np.isposinf(out.edge_margin[:, 0]).all() and not out.edge_collision[:, 0].any()
    # a gate, weights and the caller's own tracked flags on top of the mask
    wts = np.random.default_rng(3).uniform(0.5, 2.0, size=model.nv)
    trk = np.random.default_rng(5).random(q_nodes.shape[:3]) < 0.8
    gate = 3.0
    want2 = lfref.select(model, limits, q, q_nodes, trk, wts, gate * gate, 7)
    out2 = mink.ladder_path(cfg, q_nodes, trk, max_step=gate, weights=wts, collision_check=ck, edge_samples=7)
    assert want2["n_breaks"].any()
    _against_reference(out2, want2, "ladder_path with tracked, weights and a gate")
    # one unbatched configuration
    c1 = mink.Configuration(model, q[0].copy())
    one = mink.ladder_path(c1, q_nodes[0], collision_check=ck, edge_samples=7)
    assert one.node_index.shape == (5,) and one.edge_margin_all.shape == (5, 4, 4) and np.ndim(one.n_edge_collisions) == 0
    np.testing.assert_array_equal(one.node_index, out.node_index[0])
    np.testing.assert_array_equal(one.edge_margin, out.edge_margin[0])
    ck.close()


def test_a_rung_beyond_one_destination_pass(nat):
    """B = 1, T = 3, S = 70, M = 2: the flags of 70 sources staged for destination passes of 64 and 6 nodes.  One node in seven
    of the first pass and every node of the second is tracked (an untracked destination's edges are not swept, which keeps the
    numpy reference of the 9 800 edges quick)."""
    import mink_amd as mink
    (model, limits, q, q_nodes), _, want = sc.ladder_ref(1, 3, 70, 2, seed=1, sparse=True)
    em = want["edge_margin_all"]
    assert np.abs(em[np.isfinite(em)]).min() > 1e-6 and np.abs(want["node_margin"]).min() > 1e-6
    assert want["blocked"][0, 1:, 64:].any() and want["blocked"][0, 1:, :64].any()
    cfg = mink.Configuration(model, q.copy())
    ck = _checker()
    out = mink.ladder_path(cfg, q_nodes, want["tracked_in"], collision_check=ck, edge_samples=2)
    ck.close()
    _against_reference(out, want, "S = 70")
    assert (out.node_index >= 64).any() and (out.node_index < 64).any(), out.node_index


def test_a_neutral_checker_is_the_plain_search(nat):
    import mink_amd as mink
    (model, limits, q, q_nodes), _, _ = sc.ladder_ref()
    cfg = mink.Configuration(model, q.copy())
    trk = np.random.default_rng(5).random(q_nodes.shape[:3]) < 0.8
    ck = _checker(neutral=True)
    for kw in (dict(), dict(tracked=trk, max_step=3.0)):
        plain = mink.ladder_path(cfg, q_nodes, **kw)
        out = mink.ladder_path(cfg, q_nodes, collision_check=ck, edge_samples=3, **kw)
        for f in plain._fields:
            np.testing.assert_array_equal(getattr(out, f), getattr(plain, f), err_msg=f)
        assert not out.edge_collision.any() and not out.n_edge_collisions.any() and (out.node_margin > 9.0).all()
    ck.close()


# ------------------------------------------------------------------ the fused call
B, T, S, K, M, ITERS = 4, 4, 8, 4, 5, 20
THR = (1e-4, 1e-4)


def _world():
    """The UR5e at `home`, a FrameTask on attachment_site whose waypoints are the end-effector poses of rows the reference finds
    free of collision (tests/test_gpu_collision_free_ik.py's set-up, with a T axis)."""
    import mink_amd as mink
    model, _, rows = cr.fixture("ur5e_all")
    ref = cr.fixture_ref("ur5e_all")
    free = rows[~ref.in_collision][:B * T]
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
def test_fused_call_is_the_composition(nat, n_nodes):
    """solve_ik_trajectory_ladder(collision_check=...) bit for bit: the plain call's return_all, MKH_ST_IN_COLLISION from
    checker.clearance on those rows, (distinct_solutions on the free tracked results,) ladder_path(collision_check=...)."""
    import mink_amd as mink
    model, home, task, tg = _world()
    nq = model.nq
    ck = _checker()
    cfg, plain = _call(model, home, task, tg)
    _, free = _call(model, home, task, tg, collision_check=ck, edge_samples=M, **({} if n_nodes is None else dict(n_nodes=n_nodes)))
    assert isinstance(free, mink.FreeLadderResult if n_nodes is None else mink.FreeLadderNodesResult)
    clr = ck.clearance(plain.q_all)
    status = plain.status_all | np.where(clr.in_collision, mink.ST_IN_COLLISION, 0).astype(plain.status_all.dtype)
    trk = plain.converged_all & ((status & ~1) == 0)
    # the verdict of the device against the numpy reference, where the device's own margin is not within 1e-6 of zero
    want = cr.clearance(model, cr.limits_of(cr.fixture_limits("ur5e_all")), plain.q_all.reshape(-1, nq))
    clear = np.abs(clr.margin.ravel()) > 1e-6
    print("nodes: %d of %d in collision, %d tracked and free, %d margins within 1e-6 of zero" %
          (int(clr.in_collision.sum()), clr.margin.size, int(trk.sum()), int((~clear).sum())))
    assert clear.mean() >= 0.98
    np.testing.assert_array_equal(clr.in_collision.ravel()[clear], want.in_collision[clear])
    assert np.abs(clr.margin.ravel() - want.margin).max() <= TOL
    if n_nodes is None:
        np.testing.assert_array_equal(free.q_all, plain.q_all)
        np.testing.assert_array_equal(free.status_all, status)                     # the bit exactly where the clearance says so
        for f in ("v_all", "iters_all", "converged_all", "seeds"):
            np.testing.assert_array_equal(getattr(free, f), getattr(plain, f), err_msg=f)
        nodes, node_trk = plain.q_all, plain.converged_all & ((plain.status_all & ~1) == 0)
    else:
        bt = mink.Configuration(model, np.repeat(home, T, axis=0))
        sel = mink.distinct_solutions(bt, plain.q_all.reshape(B * T, S, nq), trk.reshape(B * T, S), n_solutions=K, min_distance=0.1)
        nodes, node_trk = sel.q.reshape(B, T, K, nq), (sel.seed_index >= 0).reshape(B, T, K)
        np.testing.assert_array_equal(free.q_all, nodes)
        np.testing.assert_array_equal(free.node_seed_index, sel.seed_index.reshape(B, T, K))
        np.testing.assert_array_equal(free.n_converged, sel.n_valid.reshape(B, T))
        # a colliding candidate takes no slot (an empty slot holds candidate 0's rows, as in the plain call on nodes)
        assert ((free.status_all & mink.ST_IN_COLLISION) == 0)[free.node_seed_index >= 0].all()
        assert not clr.in_collision.reshape(B * T, S)[np.arange(B * T)[:, None], np.maximum(sel.seed_index, 0)][sel.seed_index >= 0].any()
    path = mink.ladder_path(cfg, nodes, node_trk, collision_check=ck, edge_samples=M)
    for f in ("node_index", "n_tracked", "n_breaks", "path_length", "edge_break", "q", "edge_collision", "n_edge_collisions",
              "edge_margin"):
        np.testing.assert_array_equal(getattr(free, f), getattr(path, f), err_msg=f)
    # the chosen rows are the chosen nodes', and a returned tracked waypoint is free of collision
    pick = free.node_index[..., None]
    np.testing.assert_array_equal(free.status, np.take_along_axis(free.status_all, pick, axis=2)[:, :, 0])
    chosen_trk = np.take_along_axis(node_trk & (path.node_margin >= 0.0), pick, axis=2)[:, :, 0]
    assert ((free.status[chosen_trk] & mink.ST_IN_COLLISION) == 0).all()
    assert not ck.clearance(free.q[chosen_trk]).in_collision.any()
    lost = (~chosen_trk | free.edge_collision).sum(axis=1)
    np.testing.assert_array_equal(free.n_tracked, T - lost)
    print("n_nodes %s: n_tracked %s, n_edge_collisions %s (plain call: n_tracked %s)" %
          (n_nodes, free.n_tracked.tolist(), free.n_edge_collisions.tolist(), plain.n_tracked.tolist()))
    ck.close()


@pytest.mark.parametrize("n_nodes", [None, K])
def test_fused_call_across_chunks_of_rungs_and_of_checker_rows(nat, n_nodes):
    """The same call on a handle whose max_batch holds 3 of the 16 rungs (six chunks of loops, the last of one rung) with a checker
    of 20 rows per launch (the clearance behind every chunk's loops walks its 24 candidate rows — or, in the plain ladder, all 128
    node rows — in ragged chunks of its own): every output equals the one-chunk call's, bit for bit."""
    import importlib
    import mink_amd as mink
    sik = importlib.import_module("mink_amd.solve_ik")         # (the package attribute of that name is the function)
    model, home, task, tg = _world()
    cfg = mink.Configuration(model, home.copy())
    limits = [mink.ConfigurationLimit(model)]
    ft = np.ascontiguousarray(tg.reshape(B, T, 1, 7))
    kw = dict(n_seeds=S, max_iters=ITERS, pos_threshold=THR[0], ori_threshold=THR[1], rng_seed=5, edge_samples=M, return_all=True,
              max_step_sq=4.0, qvel_dt=0.1)
    if n_nodes is not None:
        kw.update(n_nodes=n_nodes, min_distance=0.1, unwind_turns=True)
    results = []
    for max_batch, max_rows in ((B * T * S, 4096), (3 * S, 20)):
        prob, layout = sik._compile(cfg, [task], limits, max_batch, 1.0, devices=cfg.devices[:1])
        assert prob.max_batch == max_batch
        ck = mink.CollisionChecker(model, cr.fixture_limits("ur5e_all"), max_rows=max_rows)
        with sik._pin(cfg, layout):
            results.append(prob.solve_trajectory_ladder_free(home, ft, None, None, 1.0, 1e-3, checker=ck, **kw))
        ck.close()
    (whole, whole_free), (parts, parts_free) = results
    assert (whole.status_all & mink.ST_IN_COLLISION).any() or n_nodes is not None
    for a, b, what in ((whole, parts, "call"), (whole_free, parts_free, "free")):
        for f in a._fields:
            x, y = getattr(a, f), getattr(b, f)
            assert (x is None) == (y is None), f
            if x is not None:
                np.testing.assert_array_equal(x, y, err_msg=f"{what}: {f}")


def test_refusals_of_the_fused_call(nat):
    import mink_amd as mink
    model, home, task, tg = _world()
    ck = _checker()
    with pytest.raises(ValueError, match="refine"):
        _call(model, home, task, tg, collision_check=ck, refine=True)
    # the entry point itself: a refinement, and n_nodes without its outputs
    import importlib
    sik = importlib.import_module("mink_amd.solve_ik")         # (the package attribute of that name is the function)
    cfg = mink.Configuration(model, home.copy())
    prob, layout = sik._compile(cfg, [task], None, 1, devices=cfg.devices[:1])
    native = ck._native_for(prob)
    tio, fio, rio = nat.MkhTrajectoryLadderIO(), nat.MkhLadderFreeIO(), nat.MkhLadderRefineIO()
    import ctypes
    args = lambda k, nodes, refine: (prob.handle, native.handle, B, T, S, k, 0.1, None, None, None, None, 1.0, 1e-3, ITERS, 1e-4, 1e-4, 0, 0,
                                     M, ctypes.byref(tio), nodes, refine, ctypes.byref(fio), 0, None)
    assert nat.lib().mkh_solve_trajectory_ladder_free(*args(0, None, ctypes.byref(rio))) == -1
    assert b"refine must be NULL" in nat.lib().mkh_last_error()
    assert nat.lib().mkh_solve_trajectory_ladder_free(*args(K, None, None)) == -1
    assert b"n_nodes" in nat.lib().mkh_last_error()
    # a checker with general convex pairs
    cmodel, _, crow = cr.fixture("ur5e_convex")
    cck = mink.CollisionChecker(cmodel, cr.fixture_limits("ur5e_convex"))
    ccfg = mink.Configuration(cmodel, crow[:1].copy())
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        mink.ladder_path(ccfg, crow[:6].reshape(1, 3, 2, -1), collision_check=cck)
    cck.close(); ck.close()
