"""The refinement pass with a checker on the device (mkh_ladder_refine_free / mkh_solve_trajectory_ladder_free_refined and the
public calls on them; include/minkhip.h "THE RULE OF THE REFINEMENT, with a checker"): the pass is the stated rule — held against
its restatement (tests/ladder_refine_free_ref.py) with the solve kernels themselves as the restatement's loop and numpy's
margins —, it heals a designed colliding node and a designed blocked motion, a neutral checker leaves the plain pass, a checker
everything collides with leaves the input, the fused call is the checked ladder followed by the pass, and the refusals.

Discrete fields exactly; margins to 1e-9 absolute with the NaN / inf placement exact; path_length to (nv + T)·2^-52 relative."""

import ctypes
import importlib

import numpy as np
import pytest

import clearance_ref as cr
import ladder_ref as ref
import ladder_refine_free_ref as fref

pytestmark = pytest.mark.gpu
TOL = 1e-9
THR = (1e-4, 1e-4)
DAMPING = 1e-3
DISCRETE = ("q", "tracked", "repaired", "refined", "edge_break", "edge_collision", "n_tracked", "n_breaks", "n_edge_collisions")
NODE = ("v", "status", "iters", "converged")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _sik():
    return importlib.import_module("mink_amd.solve_ik")          # (the package attribute of that name is the function)


def _limit_objects(wide=False, dmin=None):
    """The `ur5e_all` limits; wide: its pair list three times with three minimum distances — 42 pairs, one instance per wavefront."""
    import mink_amd as mink
    model, spec, _ = cr.fixture("ur5e_all")
    if wide:
        spec = [dict(spec[0], minimum_distance_from_collisions=d) for d in (0.02, 0.0, 0.03)]
    if dmin is not None:
        spec = [dict(kw, minimum_distance_from_collisions=dmin) for kw in spec]
    return [mink.CollisionAvoidanceLimit(model, **kw) for kw in spec]


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what}: NaN placement")
    np.testing.assert_array_equal(np.isinf(a), np.isinf(b), err_msg=f"{what}: inf placement")
    np.testing.assert_array_equal(a[np.isinf(a)], b[np.isinf(b)], err_msg=f"{what}: inf sign")
    ok = np.isfinite(a)
    err = np.abs(a[ok] - b[ok]).max() if ok.any() else 0.0
    print("  %s: max |device - ref| %.2e over %d finite entries" % (what, err, int(ok.sum())))
    assert err <= TOL, what


def _handle(B, max_batch):
    """The UR5e at `home` (B rows), a FrameTask on attachment_site, and the native handle of that problem."""
    import mink_amd as mink
    sik = _sik()
    model = cr.fixture("ur5e_all")[0]
    home = np.tile(model.key_qpos[model.name2id("key", "home")], (B, 1))
    cfg = mink.Configuration(model, home.copy())
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    prob, layout = sik._compile(cfg, [task], [mink.ConfigurationLimit(model)], max_batch, 1.0, devices=cfg.devices[:1])
    return model, home, cfg, task, prob, layout


# ------------------------------------------------------------------ 1. the pass is the restatement
#        B,  T, M, wide, gate, low iterations, rng_seed, first fixture row of the targets
CASES = {"four_per_wavefront": (5, 6, 7, False, np.inf, 4, 1, 0),
         "many_wavefronts": (70, 3, 2, False, 16.0, 4, 2, 40),
         "no_edges": (1, 1, 3, False, 16.0, 2, 3, 7),
         "no_far_edge": (3, 2, 3, False, np.inf, 3, 4, 20),
         "one_per_wavefront": (3, 4, 3, True, np.inf, 4, 5, 100)}
_cases = {}


def _case(name):
    """The device's pass and the restatement's on the paths of a checked ladder at few iterations; computed once."""
    if name in _cases:
        return _cases[name]
    import mink_amd as mink
    sik = _sik()
    B, T, M, wide, gate, low, rng_seed, row0 = CASES[name]
    S, iters = 4, 40
    model, home, cfg, task, prob, layout = _handle(B, max(B, 8) * T * S)
    rows = cr.fixture("ur5e_all")[2]
    idx = (row0 + np.arange(B * T)) % len(rows)
    # the waypoints: the end-effector poses of fixture rows, free ones and colliding ones alike
    tg = mink.Configuration(model, rows[idx]).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz.reshape(B, T, 1, 7)
    tg = np.ascontiguousarray(tg)
    objs = _limit_objects(wide)
    limits = cr.limits_of(objs)
    ck = mink.CollisionChecker(model, objs, max_rows=64)
    with sik._pin(cfg, layout):
        lad, _ = prob.solve_trajectory_ladder_free(home, tg, None, None, 1.0, DAMPING, checker=ck, edge_samples=M, n_seeds=S,
                                                   max_iters=low, pos_threshold=THR[0], ori_threshold=THR[1], max_step_sq=gate,
                                                   rng_seed=rng_seed)
        trk = ref.tracked(lad.converged, lad.status)
        nodes = dict(v=lad.v, status=lad.status, iters=lad.iters, converged=lad.converged)

        def loop(t, start):
            return prob.solve(start, np.ascontiguousarray(tg[:, t]), None, None, 1.0, DAMPING, n_steps=iters, until=THR)

        judged, margins, counts = [], [], {}
        want = fref.refine(model, limits, loop, home, lad.q, trk, M, gate, judged=judged, margins=margins, counts=counts, **nodes)
        k_ref = prob.last_kernel()
        got = prob.ladder_refine_free(home, lad.q, ck, trk, tg, None, None, 1.0, DAMPING, max_iters=iters, pos_threshold=THR[0],
                                      ori_threshold=THR[1], edge_samples=M, max_step_sq=gate, **nodes)
        assert prob.last_kernel() == k_ref                        # the same kernel family served both
    ck.close()
    print(f"{name}: B={B} T={T} M={M} {len(cr.pair_list(limits)[0])} pairs, kernel {k_ref}; the ladder tracks {lad.n_tracked.tolist()}")
    print(f"  counters {counts}; refined {want['refined'].tolist()}; n_tracked {want['n_tracked'].tolist()}")
    _cases[name] = (model, B, T, gate, got, want, judged, margins, counts, lad)
    return _cases[name]


@pytest.mark.parametrize("name", list(CASES))
def test_pass_is_the_restatement(nat, name):
    model, B, T, gate, got, want, judged, margins, counts, lad = _case(name)
    # ---- the conditions under which the discrete choices are rounding-proof, on the reference alone
    mg = np.array([x for x in margins if np.isfinite(x)])
    c = np.array([x for _, x in judged if np.isfinite(x)])
    near = np.abs(c - gate) / gate if (np.isfinite(gate) and c.size) else np.array([np.inf])
    gaps = []
    for b in range(B):
        kp, kr = want["key_in"][b], want["key_work"][b]
        if kp[:2] == kr[:2] and want["work_repaired"][b].any():
            gaps.append(abs(kp[2] - kr[2]) / max(abs(kp[2]), abs(kr[2])))
    print(f"  {len(mg)} margins judged, nearest to zero {np.abs(mg).min() if mg.size else np.inf:.3e}; {len(c)} edge costs judged, nearest "
          f"to the gate {near.min():.3e} relative; tied keys with repairs: {len(gaps)}" + (f", nearest {min(gaps):.3e}" if gaps else ""))
    assert mg.size == 0 or np.abs(mg).min() > 1e-6
    assert near.min() > 1e-9
    assert all(g > 1e-9 for g in gaps)
    # ---- the device against the restatement
    for f in DISCRETE + NODE:
        np.testing.assert_array_equal(getattr(got, f), want[f], err_msg=f"{name}: {f}")
    _close(got.node_margin, want["node_margin"], "node_margin")
    _close(got.edge_margin, want["edge_margin"], "edge_margin")
    rel = np.abs(got.path_length - want["path_length"]) / np.maximum(np.abs(want["path_length"]), np.finfo(float).tiny)
    print(f"  path_length: worst relative |device - numpy| = {rel.max():.3e}")
    assert rel.max() <= (model.nv + T) * 2.0 ** -52
    # ---- never worse than the checked ladder's path, under its key
    for b in range(B):
        assert (T - got.n_tracked[b], got.n_breaks[b]) <= (T - lad.n_tracked[b], lad.n_breaks[b])
    assert np.isposinf(got.edge_margin[:, 0]).all() and not got.edge_collision[:, 0].any()


def test_the_cases_take_every_branch(nat):
    total = dict.fromkeys(fref.COUNTERS, 0)
    for name in CASES:
        for k, v in _case(name)[8].items():
            total[k] += v
    print(total)
    assert total["accepted_forward"] >= 1 and total["accepted_backward"] >= 1
    assert total["rejected_node"] >= 1 and total["rejected_edge"] >= 1


# ------------------------------------------------------------------ 2. designed paths
_T2, _B2, _M2 = 6, 3, 5
_KW2 = dict(max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, damping=DAMPING)
_designed = {}


def _line():
    """Joint-space lines qA (B, T, 6) far from `home`, steps of at most 0.08 rad per joint, free of collision as nodes and as
    motions by the reference; their site poses as targets; a colliding fixture row and a free one whose motion from the line the
    reference finds blocked."""
    import mink_amd as mink
    import swept_ref as sref
    model, _, rows = cr.fixture("ur5e_all")
    if not _designed:
        limits = cr.limits_of(_limit_objects())
        rng = np.random.default_rng(11)
        home = model.key_qpos[model.name2id("key", "home")]
        q0 = home + np.array([2.4, 1.0, -2.6, 1.2, 2.2, 1.5]) + rng.uniform(-0.2, 0.2, size=(_B2, 6))
        qA = q0[:, None, :] + np.arange(_T2)[None, :, None] * rng.uniform(0.02, 0.08, size=(_B2, 1, 6))
        fixture = cr.fixture_ref("ur5e_all")
        hit, free = rows[1], rows[0]
        assert fixture.margin[1] < -1e-3 and fixture.margin[0] > 1e-3
        assert cr.clearance(model, limits, qA.reshape(-1, 6)).margin.min() > 1e-3
        assert sref.sweep(model, limits, qA[:, :-1].reshape(-1, 6), qA[:, 1:].reshape(-1, 6), _M2).margin.min() > 1e-3
        assert sref.sweep(model, limits, qA[:, 2], np.tile(free, (_B2, 1)), _M2).margin.max() < -1e-3      # blocked for every line
        tg = mink.Configuration(model, qA.reshape(-1, 6)).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz
        _designed.update(qA=qA, home=home, tg=np.ascontiguousarray(tg.reshape(_B2, _T2, 7)), hit=hit, free=free)
    d = _designed
    cfg = mink.Configuration(model, np.tile(d["home"], (_B2, 1)))
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    return model, cfg, task, [mink.ConfigurationLimit(model)], d["tg"], d["qA"], d["hit"], d["free"]


@pytest.mark.parametrize("case", ["colliding_node", "blocked_motion"])
def test_designed_paths_are_healed(nat, case):
    import mink_amd as mink
    model, cfg, task, lims, tg, qA, hit, free = _line()
    T, B = _T2, _B2
    ck = mink.CollisionChecker(model, _limit_objects(), max_rows=256)
    path = qA.copy()
    if case == "colliding_node":                                 # a node in collision, flagged tracked
        path[:, 3] = hit
        kw = dict(_KW2, max_step=1.0)
    else:                                                        # a free node behind a blocked motion; no gate: only the sweep can call it bad
        path[:, 3] = free
        kw = dict(_KW2, max_step=None)
    out = mink.refine_path(cfg, [task], 1.0, {task: tg}, path, limits=lims, update=False, collision_check=ck, edge_samples=_M2, **kw)
    assert isinstance(out, mink.FreeRefinedPath) and out.q.shape == (B, T, model.nq) and out.edge_collision.dtype == bool
    print(f"{case}: repaired {out.repaired.tolist()}, n_tracked {out.n_tracked.tolist()}, edge margins {np.round(out.edge_margin, 3).tolist()}")
    assert out.refined.all() and (out.n_tracked == T).all() and out.tracked.all() and (out.repaired[:, 3] == 1).all()
    assert not out.edge_collision.any() and not out.n_edge_collisions.any() and not out.edge_break.any()
    assert (out.repaired[:, :3] == 0).all()
    # the checker finds nothing on what came back: nodes and motions
    assert not ck.clearance(out.q).in_collision.any()
    sw = ck.swept_clearance(out.q[:, :-1], out.q[:, 1:], n_samples=_M2)
    assert not sw.in_collision.any()
    _close(out.node_margin, ck.clearance(out.q).margin, "node_margin against checker.clearance")
    _close(out.edge_margin[:, 1:], sw.margin, "edge_margin against checker.swept_clearance")
    # ... and the plain pass knows nothing of it: the blocked motion stays, the colliding node is repaired only by the gate
    plain = mink.refine_path(cfg, [task], 1.0, {task: tg}, path, limits=lims, update=False, **kw)
    if case == "blocked_motion":
        assert not plain.refined.any()
    ck.close()


def test_a_neutral_checker_is_the_plain_pass(nat):
    import mink_amd as mink
    model, cfg, task, lims, tg, qA, hit, free = _line()
    ck = mink.CollisionChecker(model, _limit_objects(dmin=-10.0), max_rows=256)
    path, trk = qA.copy(), np.ones((_B2, _T2), dtype=bool)
    path[:, 3, [0, 2, 4]] += 2.0                                  # one node on another branch
    trk[:, 1] = False                                            # one node lost
    kw = dict(_KW2, max_step=1.0)
    plain = mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, **kw)
    out = mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, collision_check=ck, edge_samples=3, **kw)
    assert plain.refined.all()
    for f in plain._fields:
        np.testing.assert_array_equal(getattr(out, f), getattr(plain, f), err_msg=f)
    assert not out.edge_collision.any() and not out.n_edge_collisions.any() and (out.node_margin > 9.0).all()
    ck.close()


def test_a_checker_everything_collides_with(nat):
    import mink_amd as mink
    model, cfg, task, lims, tg, qA, hit, free = _line()
    ck = mink.CollisionChecker(model, _limit_objects(dmin=10.0), max_rows=256)
    path, trk = qA.copy(), np.ones((_B2, _T2), dtype=bool)
    trk[:, 1] = False
    out = mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, collision_check=ck, edge_samples=3,
                           **dict(_KW2, max_step=1.0))
    assert not out.refined.any() and not out.repaired.any() and not out.tracked.any() and (out.n_tracked == 0).all()
    np.testing.assert_array_equal(out.q, path)
    assert not out.v.any() and not out.status.any() and not out.iters.any() and not out.converged.any()
    assert not out.edge_collision.any() and np.isnan(out.edge_margin[:, 1:]).all() and (out.node_margin < 0).all()
    ck.close()


# ------------------------------------------------------------------ 3. fused = composition
B, T, S, K, M, ITERS = 4, 4, 8, 4, 5, 20


def _world():
    """tests/test_gpu_ladder_free.py::_world: the waypoints are the end-effector poses of free fixture rows."""
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
                                                damping=DAMPING, rng_seed=5, update=False, **kw)


@pytest.mark.parametrize("world,n_nodes", [("fixture", None), ("fixture", K), ("line", None)])
def test_fused_call_is_the_composition(nat, world, n_nodes):
    """`line`: the designed lines of part 2 as waypoints, far from `home` — consecutive targets are close, so the pass has
    something it can heal with the rungs' own 20 iterations, and both sides of the guard are in the comparison."""
    import mink_amd as mink
    if world == "fixture":
        model, home, task, tg = _world()
    else:
        model, cfg_line, task, _, tg, _, _, _ = _line()
        home = cfg_line.q_batch.copy()
    ck = mink.CollisionChecker(model, _limit_objects(), max_rows=4096)
    more = {} if n_nodes is None else dict(n_nodes=n_nodes)
    cfg, checked = _call(model, home, task, tg, collision_check=ck, edge_samples=M, **more)
    _, fused = _call(model, home, task, tg, collision_check=ck, edge_samples=M, refine="free", **more)
    assert isinstance(fused, mink.FreeRefinedLadderResult if n_nodes is None else mink.FreeRefinedLadderNodesResult)
    trk = checked.converged & ((checked.status & ~1) == 0)       # (a colliding node carries ST_IN_COLLISION: not tracked)
    sik = _sik()
    prob, layout = sik._compile(cfg, [task], [mink.ConfigurationLimit(model)], tg.shape[0] * tg.shape[1] * S, 1.0, devices=cfg.devices[:1])
    with sik._pin(cfg, layout):
        two = prob.ladder_refine_free(home, checked.q, ck, trk, np.ascontiguousarray(tg[:, :, None, :]), None, None, 1.0, DAMPING,
                                      max_iters=ITERS, pos_threshold=THR[0], ori_threshold=THR[1], edge_samples=M,
                                      v=checked.v, status=checked.status, iters=checked.iters, converged=checked.converged.astype(np.int32))
    for f in ("q", "v", "status", "iters", "repaired", "n_tracked", "n_breaks", "path_length", "n_edge_collisions", "edge_margin"):
        np.testing.assert_array_equal(getattr(fused, f), getattr(two, f), err_msg=f)
    for f in ("converged", "refined", "edge_break", "edge_collision"):
        np.testing.assert_array_equal(getattr(fused, f), getattr(two, f).astype(bool), err_msg=f)
    np.testing.assert_array_equal(fused.node_index, checked.node_index)      # the search's choice, repaired or not
    assert (fused.n_tracked >= checked.n_tracked).all()
    keep = ~fused.refined
    for f in checked._fields:
        if getattr(checked, f) is not None:
            np.testing.assert_array_equal(getattr(fused, f)[keep], getattr(checked, f)[keep], err_msg=f"kept: {f}")
    if world == "line":
        assert fused.refined.any()                               # (the case's condition: something was there to refine)
    print(f"{world}, n_nodes {n_nodes}: checked n_tracked {checked.n_tracked.tolist()}, refined {fused.refined.astype(int).tolist()}: "
          f"{fused.n_tracked.tolist()}, repaired {fused.repaired.tolist()}")
    ck.close()


def test_fused_call_across_chunks_and_pointer_kinds(nat):
    """A handle whose max_batch holds 3 of the 16 rungs with a checker of 20 rows per launch: bitwise the one-chunk call.  The
    pass alone on device pointers: bitwise the host-pointer call."""
    import torch
    import mink_amd as mink
    sik = _sik()
    model, home, task, tg = _world()
    cfg = mink.Configuration(model, home.copy())
    limits = [mink.ConfigurationLimit(model)]
    ft = np.ascontiguousarray(tg.reshape(B, T, 1, 7))
    kw = dict(n_seeds=S, max_iters=ITERS, pos_threshold=THR[0], ori_threshold=THR[1], rng_seed=5, edge_samples=M,
              qvel_dt=0.1, refine=True)
    results = []
    for max_batch, max_rows in ((B * T * S, 4096), (3 * S, 20)):
        prob, layout = sik._compile(cfg, [task], limits, max_batch, 1.0, devices=cfg.devices[:1])
        assert prob.max_batch == max_batch
        ck = mink.CollisionChecker(model, _limit_objects(), max_rows=max_rows)
        with sik._pin(cfg, layout):
            results.append(prob.solve_trajectory_ladder_free(home, ft, None, None, 1.0, DAMPING, checker=ck, **kw))
        if max_rows == 20:
            ck.close()
        else:
            whole_ck, whole_prob, whole_layout = ck, prob, layout
    (whole, whole_free), (parts, parts_free) = results
    for a, b, what in ((whole, parts, "call"), (whole_free, parts_free, "free")):
        for f in a._fields:
            x, y = getattr(a, f), getattr(b, f)
            assert (x is None) == (y is None), f
            if x is not None:
                np.testing.assert_array_equal(x, y, err_msg=f"{what}: {f}")
    assert whole.repaired is not None and whole.refined is not None
    # the pass alone: host arrays against device tensors
    dev = torch.device("cuda:0")
    on = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    path, trk = whole.q.copy(), np.ones((B, T), np.int32)
    path[:, 1] = cr.fixture("ur5e_all")[2][1]                     # a colliding fixture row
    trk[:, 2] = 0
    rkw = dict(max_iters=ITERS, pos_threshold=THR[0], ori_threshold=THR[1], edge_samples=M)
    with sik._pin(cfg, whole_layout):
        host = whole_prob.ladder_refine_free(home, path, whole_ck, trk, ft, None, None, 1.0, DAMPING, **rkw)
        devr = whole_prob.ladder_refine_free(on(home), on(path), whole_ck, on(trk), on(ft), None, None, 1.0, DAMPING, **rkw)
    assert all(x is None or (isinstance(x, torch.Tensor) and x.device.type == "cuda") for x in devr)
    for f in host._fields:
        if getattr(host, f) is not None:
            np.testing.assert_array_equal(getattr(devr, f).cpu().numpy(), getattr(host, f), err_msg=f"device pointers: {f}")
    whole_ck.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals(nat):
    import mink_amd as mink
    model, home, task, tg = _world()
    ck = mink.CollisionChecker(model, _limit_objects(), max_rows=64)
    cfg = mink.Configuration(model, home.copy())
    path = np.tile(home[:, None], (1, T, 1))
    lims = [mink.ConfigurationLimit(model)]
    with pytest.raises(ValueError, match="edge_samples must be >= 1"):
        mink.refine_path(cfg, [task], 1.0, {task: tg}, path, limits=lims, collision_check=ck, edge_samples=0)
    with pytest.raises(ValueError, match='refine="free" is the refinement pass with a checker'):
        _call(model, home, task, tg, refine="free")
    with pytest.raises(ValueError, match="refine"):
        _call(model, home, task, tg, collision_check=ck, refine=True)
    # a checker with general convex pairs; another model's checker
    cmodel, _, crow = cr.fixture("ur5e_convex")
    cck = mink.CollisionChecker(cmodel, cr.fixture_limits("ur5e_convex"))
    ccfg = mink.Configuration(cmodel, crow[0].copy())
    ctask = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    with pytest.raises(nat.MinkHipError, match="general convex pairs"):
        mink.refine_path(ccfg, [ctask], 1.0, {ctask: tg[0, :2]}, crow[:2], collision_check=cck)
    with pytest.raises(ValueError, match="another model"):
        mink.refine_path(cfg, [task], 1.0, {task: tg}, path, limits=lims, collision_check=cck)
    # the entry points themselves: n_samples, an attached checker, refine == NULL
    sik = _sik()
    prob, layout = sik._compile(cfg, [task], lims, B, 1.0, devices=cfg.devices[:1])
    native = ck._native_for(prob)
    L = nat.lib()
    f8, i4 = np.float64, np.int32
    out = dict(q_path_out=np.empty((B, T, model.nq), f8), tracked_out=np.empty((B, T), i4), repaired=np.empty((B, T), i4),
               refined=np.empty(B, i4), edge_break=np.empty((B, T), i4), n_tracked=np.empty(B, i4), n_breaks=np.empty(B, i4),
               path_length=np.empty(B, f8))
    rio, fio = nat.MkhLadderRefineIO(), nat.MkhLadderRefineFreeIO()
    for name, x in out.items():
        setattr(rio, name, x.ctypes.data)
    rio.max_step_sq = 4.0
    more = [np.empty((B, T), i4), np.empty(B, i4), np.empty((B, T), f8)]
    fio.edge_collision, fio.n_edge_collisions, fio.edge_margin = (x.ctypes.data for x in more)
    q, ft, trk = np.ascontiguousarray(home), np.ascontiguousarray(tg.reshape(B, T, 1, 7)), np.ones((B, T), i4)
    call = lambda checker, n: L.mkh_ladder_refine_free(prob.handle, checker, B, T, q.ctypes.data, path.ctypes.data, trk.ctypes.data,
                                                       ft.ctypes.data, None, None, 1.0, DAMPING, ITERS, 1e-4, 1e-4, n,
                                                       ctypes.byref(rio), ctypes.byref(fio), 0, None)
    with sik._pin(cfg, layout):
        assert call(native.handle, 0) == -1 and b"n_samples" in L.mkh_last_error()
        assert call(None, M) == -1 and b"null checker" in L.mkh_last_error()
        assert L.mkh_problem_set_collision_check(prob.handle, native.handle) == 0
        assert call(native.handle, M) == -1 and b"a collision checker is attached" in L.mkh_last_error()
        assert L.mkh_problem_set_collision_check(prob.handle, None) == 0
        assert call(native.handle, M) == 0, L.mkh_last_error()
        tio, lio = nat.MkhTrajectoryLadderIO(), nat.MkhLadderFreeIO()
        assert L.mkh_solve_trajectory_ladder_free_refined(prob.handle, native.handle, B, T, S, 0, 0.1, None, None, None, None, 1.0, 1e-3,
                                                          ITERS, 1e-4, 1e-4, 0, 0, M, ctypes.byref(tio), None, None, ctypes.byref(lio), 0,
                                                          None) == -1
        assert b"refine is required" in L.mkh_last_error()
    cck.close(); ck.close()
