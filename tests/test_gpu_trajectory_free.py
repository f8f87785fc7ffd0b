"""Checked candidate tracking on the device (include/minkhip.h THE RULE "with a checker" of mkh_solve_trajectory_multistart):
candidate_path(collision_check=...) against the numpy reference of tests/trajectory_free_ref.py on the two shared cases of
tests/trajectory_free_cases.py, the plain selection against trajectory_multistart_ref, rows with a NaN or an infinity, and
solve_ik_trajectory_multistart(collision_check=...) against the unchecked call, the checker's own calls on its candidates and
the numpy rule applied to them.

Integers and the NaN / inf placement exactly; margins to 1e-9 absolute; path_length to 1e-12 relative.  The shared cases keep
every reference margin more than 1e-3 away from zero (tests/test_trajectory_free_cpu.py asserts it), so no flag is excluded."""

import numpy as np
import pytest

import clearance_ref as cr
import trajectory_free_cases as tc
import trajectory_free_ref as tfref
import trajectory_multistart_ref as tmref

pytestmark = pytest.mark.gpu
TOL = 1e-9
EXACT = ("seed_index", "n_tracked", "n_complete", "edge_collision", "n_edge_collisions", "tracked")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _checker(name="ur5e_all", neutral=False, **kw):
    import mink_amd as mink
    model, spec, _ = cr.fixture(name)
    if neutral:                            # no configuration is closer than -10 m to anything
        spec = [dict(s, minimum_distance_from_collisions=-10.0) for s in spec]
    return mink.CollisionChecker(model, [mink.CollisionAvoidanceLimit(model, **s) for s in spec], **kw)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what}: NaN placement")
    np.testing.assert_array_equal(np.isposinf(a), np.isposinf(b), err_msg=f"{what}: +inf placement")
    np.testing.assert_array_equal(np.isneginf(a), np.isneginf(b), err_msg=f"{what}: -inf placement")
    ok = np.isfinite(a)
    err = np.abs(a[ok] - b[ok]).max() if ok.any() else 0.0
    print("%s: max |device - ref| %.2e over %d finite entries" % (what, err, int(ok.sum())))
    assert err <= TOL, what


def _by_instance(x, B, S):
    return tmref.by_instance(x, B, S)


def _against_reference(out, want, B, S, what):
    for f in EXACT:
        np.testing.assert_array_equal(np.asarray(getattr(out, f)).astype(np.int64), np.asarray(want[f]).astype(np.int64), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(out.q, want["q_path"], err_msg=f"{what}: q")
    assert np.abs(out.path_length / want["path_length"] - 1.0).max() <= 1e-12
    _close(out.node_margin, want["node_margin"], f"{what}: node_margin")
    _close(out.edge_margin, want["edge_margin"], f"{what}: edge_margin")
    _close(out.node_margin_all, _by_instance(want["node_margin_all"], B, S), f"{what}: node_margin_all")
    _close(out.edge_margin_all, _by_instance(want["edge_margin_all"], B, S), f"{what}: edge_margin_all")


def _paths(q_all, B, S):
    """Time-major (T, B·S, nq) candidates as candidate_path takes them: (B, S, T, nq)."""
    return _by_instance(q_all, B, S)


def test_candidate_path_against_the_reference_on_the_shared_case(nat):
    """ur5e_all (four rows per wavefront), B = 3, S = 4, T = 5, M = 5: colliding nodes, blocked and unswept edges, picks that both
    masks change.  Then weights and a caller's tracked flags, and one unbatched configuration."""
    import mink_amd as mink
    (model, limits, q, q_all), want = tc.shared()
    B, S, T, M = (tc.SHARED[k] for k in "BSTM")
    cfg = mink.Configuration(model, q.copy())
    ck = _checker()
    paths = _paths(q_all, B, S)
    out = mink.candidate_path(cfg, paths, collision_check=ck, edge_samples=M)
    assert isinstance(out, mink.FreeCandidatePath) and out.edge_collision.dtype == bool and out.tracked.dtype == bool
    assert out.edge_margin_all.shape == (B, S, T) and out.q.shape == (B, T, model.nq)
    _against_reference(out, want, B, S, "candidate_path")
    assert out.seed_index.tolist() == [0, 3, 1]
    assert np.isposinf(out.edge_margin[:, 0]).all() and np.isposinf(out.edge_margin_all[:, :, 0]).all() and not out.edge_collision[:, 0].any()
    # weights and the caller's own flags on top
    wts = np.random.default_rng(3).uniform(0.5, 2.0, size=model.nv)
    trk = np.random.default_rng(5).random((T, B * S)) < 0.8
    want2 = tfref.rule(model, limits, q, q_all, trk.astype(np.int32), None, S, M, weights=wts)
    assert (want2["seed_index"] != want["seed_index"]).any() or (want2["n_tracked"] != want["n_tracked"]).any()
    out2 = mink.candidate_path(cfg, paths, _by_instance(trk, B, S), weights=wts, collision_check=ck, edge_samples=M)
    _against_reference(out2, want2, B, S, "candidate_path with tracked and weights")
    # one unbatched configuration
    one = mink.candidate_path(mink.Configuration(model, q[0].copy()), paths[0], collision_check=ck, edge_samples=M)
    assert one.q.shape == (T, model.nq) and one.edge_margin_all.shape == (S, T) and np.ndim(one.seed_index) == 0
    assert int(one.seed_index) == int(out.seed_index[0])
    np.testing.assert_array_equal(one.edge_margin, out.edge_margin[0])
    np.testing.assert_array_equal(one.node_margin_all, out.node_margin_all[0])
    np.testing.assert_array_equal(one.tracked, out.tracked[0])
    ck.close()


def test_candidate_path_against_the_reference_on_g1(nat):
    """g1 (46 pairs, a free joint): one row per wavefront, quaternion shortest arcs; B = 2, S = 3, T = 3, M = 3."""
    import mink_amd as mink
    (model, limits, q, q_all), want = tc.g1()
    B, S, T, M = (tc.G1[k] for k in "BSTM")
    ck = _checker("g1")
    out = mink.candidate_path(mink.Configuration(model, q.copy()), _paths(q_all, B, S), collision_check=ck, edge_samples=M)
    ck.close()
    _against_reference(out, want, B, S, "g1")
    assert out.seed_index.tolist() == [0, 1] and out.n_edge_collisions.sum() == want["n_edge_collisions"].sum()


def test_plain_rule_without_a_checker(nat):
    """candidate_path without a checker is THE RULE on the caller's flags: trajectory_multistart_ref.choose."""
    import mink_amd as mink
    (model, limits, q, q_all), _ = tc.shared()
    B, S, T = (tc.SHARED[k] for k in "BST")
    cfg = mink.Configuration(model, q.copy())
    trk = np.random.default_rng(11).random((T, B * S)) < 0.7
    wts = np.random.default_rng(3).uniform(0.5, 2.0, size=model.nv)
    for flags, w in ((None, None), (trk, wts)):
        cv = np.ones((T, B * S), np.int32) if flags is None else flags.astype(np.int32)
        seed, n_tracked, n_complete, length, _, _ = tmref.choose(model, q, q_all, cv, np.zeros_like(cv), S, w)
        out = mink.candidate_path(cfg, _paths(q_all, B, S), None if flags is None else _by_instance(flags, B, S), weights=w)
        assert isinstance(out, mink.CandidatePath) and not isinstance(out, mink.FreeCandidatePath)
        np.testing.assert_array_equal(out.seed_index, seed)
        np.testing.assert_array_equal(out.n_tracked, n_tracked)
        np.testing.assert_array_equal(out.n_complete, n_complete)
        assert np.abs(out.path_length / length - 1.0).max() <= 1e-12
        np.testing.assert_array_equal(out.q, tmref.chosen(q_all, seed, S))
    # nobody tracked anything: candidate 0
    none = mink.candidate_path(cfg, _paths(q_all, B, S), np.zeros((B, S, T), dtype=bool))
    assert none.seed_index.tolist() == [0] * B and none.n_tracked.tolist() == [0] * B and none.n_complete.tolist() == [0] * B


def test_rows_with_a_nan_or_an_infinity(nat):
    """A NaN row and an inf row among the candidates: the node's margin is NaN and the node in collision, the edge into it is not
    swept (NaN), the edge out of it is swept, NaN and collides."""
    import mink_amd as mink
    (model, limits, q, q_all), _ = tc.shared()
    B, S, T, M = (tc.SHARED[k] for k in "BSTM")
    free = cr.fixture("ur5e_all")[2][~cr.fixture_ref("ur5e_all").in_collision]
    q_all = np.ascontiguousarray(free[:T * B * S].reshape(T, B * S, model.nq)).copy()
    q_all[1, 0, 2] = np.nan                # candidate 0 of instance 0, waypoint 1
    q_all[2, 5, 0] = np.inf                # candidate 1 of instance 1, waypoint 2
    want = tfref.rule(model, limits, q, q_all, None, None, S, M)
    for t, i in ((1, 0), (2, 5)):
        assert np.isnan(want["node_margin_all"][t, i]) and np.isnan(want["edge_margin_all"][t, i]) and want["status_all"][t, i] == 64
        assert want["eligible"][t + 1, i] and np.isnan(want["edge_margin_all"][t + 1, i]) and not want["counted"][t + 1, i]
    ck = _checker()
    out = mink.candidate_path(mink.Configuration(model, q.copy()), _paths(q_all, B, S), collision_check=ck, edge_samples=M)
    ck.close()
    for f in EXACT:
        np.testing.assert_array_equal(np.asarray(getattr(out, f)).astype(np.int64), np.asarray(want[f]).astype(np.int64), err_msg=f)
    _close(out.node_margin_all, _by_instance(want["node_margin_all"], B, S), "node_margin_all")
    _close(out.edge_margin_all, _by_instance(want["edge_margin_all"], B, S), "edge_margin_all")
    assert np.isnan(out.node_margin_all[0, 0, 1]) and np.isnan(out.edge_margin_all[0, 0, 1]) and np.isnan(out.edge_margin_all[0, 0, 2])
    assert np.isnan(out.node_margin_all[1, 1, 2]) and np.isnan(out.edge_margin_all[1, 1, 2]) and np.isnan(out.edge_margin_all[1, 1, 3])
    assert out.seed_index[0] != 0 and out.seed_index[1] != 1


# ------------------------------------------------------------------ the fused call
B, T, S, M, ITERS = 4, 4, 8, 5, 20
THR = (1e-4, 1e-4)


def _world():
    """The UR5e at `home`, a FrameTask on attachment_site whose waypoints are the end-effector poses of rows the reference finds
    free of collision (tests/test_gpu_ladder_free.py's set-up, restated)."""
    import mink_amd as mink
    model, _, rows = cr.fixture("ur5e_all")
    ref = cr.fixture_ref("ur5e_all")
    free = rows[~ref.in_collision][:B * T]
    tg = mink.Configuration(model, free).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz.reshape(B, T, 7)
    home = np.tile(model.key_qpos[model.name2id("key", "home")], (B, 1))
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    return model, home, task, tg


def _call(model, home, task, tg, n_seeds=S, **kw):
    import mink_amd as mink
    cfg = mink.Configuration(model, home.copy())
    return cfg, mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: tg}, n_seeds, ITERS, *THR, limits=[mink.ConfigurationLimit(model)],
                                                    damping=1e-3, rng_seed=5, update=False, return_all=True, **kw)


def test_fused_call_against_the_unchecked_call_and_the_checker(nat):
    """UR5e, B = 4, T = 4, S = 8, M = 5, 20 iterations.  The loops' arrays are bitwise the unchecked call's; status_all is the plain
    one OR the bit where the device's own node margin is < 0; margins are checker.clearance's and checker.swept_clearance's where
    swept, NaN and +inf exactly placed; the choice is the numpy rule on the device's own candidates; chosen rows are rows of _all."""
    import mink_amd as mink
    model, home, task, tg = _world()
    nq = model.nq
    ck = _checker()
    _, plain = _call(model, home, task, tg)
    _, free = _call(model, home, task, tg, collision_check=ck, edge_samples=M)
    assert isinstance(free, mink.FreeTrajectoryMultistartResult) and free.tracked.dtype == bool and free.edge_collision.dtype == bool
    for f in ("q_all", "v_all", "iters_all", "converged_all", "seeds"):
        np.testing.assert_array_equal(getattr(free, f), getattr(plain, f), err_msg=f)
    hit = ~(free.node_margin_all >= 0.0)
    np.testing.assert_array_equal(free.status_all, plain.status_all | np.where(hit, mink.ST_IN_COLLISION, 0).astype(plain.status_all.dtype))
    # nodes and edges against the checker's own calls on the same rows
    clr = ck.clearance(plain.q_all)
    _close(free.node_margin_all, clr.margin, "node_margin_all against checker.clearance")
    eligible = plain.converged_all & ((free.status_all & ~1) == 0)
    swept = eligible.copy(); swept[:, :, 0] = False
    em = free.edge_margin_all
    assert np.isposinf(em[:, :, 0]).all() and (np.isnan(em[:, :, 1:]) == ~eligible[:, :, 1:]).all() and not np.isinf(em[:, :, 1:]).any()
    sw = ck.swept_clearance(plain.q_all[:, :, :-1], plain.q_all[:, :, 1:], n_samples=M)
    _close(em[:, :, 1:][swept[:, :, 1:]], sw.margin[swept[:, :, 1:]], "edge_margin_all against checker.swept_clearance")
    print("rows: %d of %d in collision, %d eligible, %d edges swept, %d of them collide; nearest margin to zero %.2e" %
          (int(hit.sum()), hit.size, int(eligible.sum()), int(swept.sum()), int((em[swept] < 0).sum()),
           float(min(np.abs(free.node_margin_all).min(), np.abs(em[swept]).min()))))
    assert hit.any() and (em[swept] < 0).any() and swept.sum() < (T - 1) * B * S       # the case has all three kinds of rows
    # the choice: the numpy rule on the device's own flags and margins
    tm = lambda x: np.ascontiguousarray(np.moveaxis(x, 2, 0)).reshape((T, B * S) + x.shape[3:])   # (B, S, T, ·) -> (T, B·S, ·)
    _, _, _, counted = tfref.flags(tm(plain.converged_all).astype(np.int32), tm(plain.status_all), tm(free.node_margin_all),
                                   lambda t, i: tm(em)[t, i])[:4]
    lengths = tfref.lengths_of(model, home, tm(plain.q_all), S)
    seed, n_tracked, n_complete, _ = tfref.pick(counted, lengths, S)
    np.testing.assert_array_equal(free.seed_index, seed)
    np.testing.assert_array_equal(free.n_tracked, n_tracked)
    np.testing.assert_array_equal(free.n_complete, n_complete)
    assert np.abs(free.path_length / lengths[np.arange(B), seed] - 1.0).max() <= 1e-12
    print("seed_index %s (unchecked %s), n_tracked %s (unchecked %s), n_complete %s (unchecked %s)" %
          (free.seed_index.tolist(), plain.seed_index.tolist(), free.n_tracked.tolist(), plain.n_tracked.tolist(),
           free.n_complete.tolist(), plain.n_complete.tolist()))
    # the chosen rows are rows of _all
    rows = np.arange(B)
    for f, g in (("q", "q_all"), ("v", "v_all"), ("status", "status_all"), ("iters", "iters_all"), ("converged", "converged_all"),
                 ("node_margin", "node_margin_all"), ("edge_margin", "edge_margin_all")):
        np.testing.assert_array_equal(getattr(free, f), getattr(free, g)[rows, free.seed_index], err_msg=f)
    chosen_el = eligible[rows, free.seed_index]
    np.testing.assert_array_equal(free.edge_collision, chosen_el & ~(free.edge_margin >= 0.0) & (np.arange(T) >= 1))
    np.testing.assert_array_equal(free.n_edge_collisions, free.edge_collision.sum(axis=1))
    np.testing.assert_array_equal(free.tracked, chosen_el & ((np.arange(T) == 0) | (np.nan_to_num(free.edge_margin, nan=-1.0) >= 0.0)))
    np.testing.assert_array_equal(free.tracked.sum(axis=1), free.n_tracked)
    ck.close()


def test_fused_call_in_both_layouts_on_numpy_and_torch(nat):
    """The native call batch-major and time-major, numpy arrays and torch tensors: four times the same result."""
    import importlib
    import torch
    import mink_amd as mink
    sik = importlib.import_module("mink_amd.solve_ik")         # (the package attribute of that name is the function)
    model, home, task, tg = _world()
    cfg = mink.Configuration(model, home.copy())
    prob, layout = sik._compile(cfg, [task], [mink.ConfigurationLimit(model)], B * S, 1.0, devices=cfg.devices[:1])
    ck = _checker()
    ft = np.ascontiguousarray(tg.reshape(B, T, 1, 7))
    kw = dict(checker=ck, edge_samples=M, n_seeds=S, n_steps=ITERS, pos_threshold=THR[0], ori_threshold=THR[1], rng_seed=5,
              return_all=True, qvel_dt=0.1)
    dev = torch.device("cuda:0")
    results = {}
    with sik._pin(cfg, layout):
        for tm in (False, True):
            f = np.ascontiguousarray(np.swapaxes(ft, 0, 1)) if tm else ft
            results["numpy", tm] = prob.solve_trajectory_multistart_free(home, f, None, None, 1.0, 1e-3, time_major=tm, **kw)
            o, more = prob.solve_trajectory_multistart_free(torch.as_tensor(home, device=dev), torch.as_tensor(f, device=dev), None, None,
                                                            1.0, 1e-3, time_major=tm, **kw)
            torch.cuda.synchronize()
            host = lambda r: type(r)(*[None if x is None else x.cpu().numpy() for x in r])
            results["torch", tm] = (host(o), host(more))
    ck.close()
    base, base_more = results["numpy", False]
    em = base_more.edge_margin_all
    assert (base.status_all & mink.ST_IN_COLLISION).any() and np.isnan(em).any() and (em[np.isfinite(em)] < 0.0).any()
    assert np.isnan(base_more.edge_margin).any() and np.isposinf(base_more.edge_margin[:, 0]).all()
    for (kind, tm), (o, more) in results.items():
        for r, want in ((o, base), (more, base_more)):
            for f in r._fields:
                x, y = getattr(r, f), getattr(want, f)
                assert (x is None) == (y is None), f
                if x is None:
                    continue
                if tm and x.ndim >= 2 and not f.endswith("_all") and f != "seeds":
                    x = np.swapaxes(x, 0, 1)                   # (T, B, ·) -> (B, T, ·); the *_all arrays are time-major either way
                np.testing.assert_array_equal(x, y, err_msg=f"{kind}, time_major={tm}: {f}")


def test_a_neutral_checker_is_the_unchecked_call(nat):
    """minimum_distance_from_collisions = -10 m: every shared field is bitwise the unchecked call's and nothing collides."""
    model, home, task, tg = _world()
    ck = _checker(neutral=True)
    _, plain = _call(model, home, task, tg)
    _, free = _call(model, home, task, tg, collision_check=ck, edge_samples=3)
    ck.close()
    for f in plain._fields:
        x, y = getattr(free, f), getattr(plain, f)
        assert (x is None) == (y is None), f
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg=f)
    assert not free.edge_collision.any() and not free.n_edge_collisions.any() and (free.node_margin_all > 9.0).all()
    el = plain.converged_all & ((plain.status_all & ~1) == 0)
    assert (free.edge_margin_all[:, :, 1:][el[:, :, 1:]] > 9.0).all() and np.isnan(free.edge_margin_all[:, :, 1:][~el[:, :, 1:]]).all()
    np.testing.assert_array_equal(free.tracked, el[np.arange(B), free.seed_index])


def test_one_seed_is_solve_ik_trajectory_plus_the_verdict(nat):
    import mink_amd as mink
    model, home, task, tg = _world()
    ck = _checker()
    cfg = mink.Configuration(model, home.copy())
    traj = mink.solve_ik_trajectory(cfg, [task], 1.0, {task: tg}, ITERS, pos_threshold=THR[0], ori_threshold=THR[1],
                                    limits=[mink.ConfigurationLimit(model)], damping=1e-3, update=False)
    _, free = _call(model, home, task, tg, n_seeds=1, collision_check=ck, edge_samples=M)
    for f in ("q", "v", "iters", "converged"):
        np.testing.assert_array_equal(getattr(free, f), getattr(traj, f), err_msg=f)
    clr = ck.clearance(traj.q)
    np.testing.assert_array_equal(free.status, traj.status | np.where(clr.in_collision, mink.ST_IN_COLLISION, 0).astype(traj.status.dtype))
    _close(free.node_margin, clr.margin, "node_margin")
    assert free.seed_index.tolist() == [0] * B and free.q_all.shape == (B, 1, T, model.nq)
    el = free.converged & ((free.status & ~1) == 0)
    sw = ck.swept_clearance(traj.q[:, :-1], traj.q[:, 1:], n_samples=M)
    assert np.isposinf(free.edge_margin[:, 0]).all() and (np.isnan(free.edge_margin[:, 1:]) == ~el[:, 1:]).all()
    _close(free.edge_margin[:, 1:][el[:, 1:]], sw.margin[el[:, 1:]], "edge_margin")
    np.testing.assert_array_equal(free.edge_collision[:, 1:], el[:, 1:] & sw.in_collision)
    ck.close()


def test_chunks_give_the_same_result(nat):
    """max_instances that holds one instance's candidates at a time (four chunks), and a checker of 20 rows per launch."""
    model, home, task, tg = _world()
    ck, small = _checker(), _checker(max_rows=20)
    _, whole = _call(model, home, task, tg, collision_check=ck, edge_samples=M)
    _, parts = _call(model, home, task, tg, collision_check=small, edge_samples=M, max_instances=S)
    ck.close(); small.close()
    for f in whole._fields:
        x, y = getattr(whole, f), getattr(parts, f)
        assert (x is None) == (y is None), f
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg=f)


def test_refusals(nat):
    import ctypes
    import importlib
    import mink_amd as mink
    sik = importlib.import_module("mink_amd.solve_ik")         # (the package attribute of that name is the function)
    model, home, task, tg = _world()
    cfg = mink.Configuration(model, home.copy())
    # a checker with general convex pairs
    cmodel, _, crow = cr.fixture("ur5e_convex")
    cck = mink.CollisionChecker(cmodel, cr.fixture_limits("ur5e_convex"))
    ccfg = mink.Configuration(cmodel, crow[:1].copy())
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        mink.candidate_path(ccfg, crow[:6].reshape(1, 2, 3, -1), collision_check=cck)
    ctask = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        mink.solve_ik_trajectory_multistart(ccfg, [ctask], 1.0, {ctask: tg[:1]}, 2, 3, *THR, update=False, collision_check=cck)
    cck.close()
    # an attached checker is still refused; a checker on another model handle
    ck = _checker()
    prob, layout = sik._compile(cfg, [task], None, B * S, 1.0, devices=cfg.devices[:1])
    native = ck._native_for(prob)
    ft = np.ascontiguousarray(tg.reshape(B, T, 1, 7))
    kw = dict(edge_samples=M, n_seeds=S, n_steps=ITERS, pos_threshold=THR[0], ori_threshold=THR[1])
    with sik._pin(cfg, layout):
        assert nat.lib().mkh_problem_set_collision_check(prob.handle, native.handle) == 0
        try:
            with pytest.raises(nat.MinkHipError, match="a collision checker is attached"):
                prob.solve_trajectory_multistart_free(home, ft, None, None, 1.0, 1e-3, checker=native, **kw)
        finally:
            assert nat.lib().mkh_problem_set_collision_check(prob.handle, None) == 0
        other_model = nat.NativeModel(model, device=0)
        other = nat.NativeProblem(other_model, collision_limits=ck._descs, max_batch=64)
        with pytest.raises(ValueError, match="another NativeModel"):
            prob.solve_trajectory_multistart_free(home, ft, None, None, 1.0, 1e-3, checker=other, **kw)
        cio, fio = nat.MkhTrajectoryCandidatesIO(), nat.MkhTrajectoryFreeIO()
        buf = np.zeros(4096)
        for io, names in ((cio, nat.TRAJECTORY_CANDIDATES_IO_FIELDS), (fio, nat.TRAJECTORY_FREE_IO_FIELDS[:4])):
            for n in names:
                setattr(io, n, buf.ctypes.data)
        assert nat.lib().mkh_select_trajectory_candidates(prob.handle, other.handle, 1, 2, 2, buf.ctypes.data, buf.ctypes.data, None, None, 3,
                                                          ctypes.byref(cio), ctypes.byref(fio), 0, None) == -1
        assert b"another MkhModel" in nat.lib().mkh_last_error()
        other.close(); other_model.close()
    ck.close()
