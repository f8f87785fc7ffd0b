"""Checked candidate tracking and the checked refinement pass on checkers WITH general convex pairs (cylinder-box,
cylinder-cylinder, ellipsoid-*: `CollisionChecker(check_rows=)`, mkh_problem_set_check_rows, convex_check.hip and the _cv builds of
tmf_check_kernel and lr_check_kernel) against the numpy references tests/trajectory_free_ref.py and tests/ladder_refine_free_ref.py,
which work from clearance_ref and swept_ref and so take such pairs as they are.

Tolerance: margins to 1e-9 absolute, the bound tests/test_gpu_swept_convex.py uses; flags, indices, counts and the selection
exactly, on cases whose reference margins all lie more than 1e-6 from zero (asserted on the reference alone, here and in
tests/test_convex_checks_cpu.py).  Outputs must not depend on `check_rows` nor on the kind of pointers: every chunking is compared
bit for bit.  No margin is compared bit for bit with `clearance` / `swept_clearance`: those come from other kernels."""

import contextlib
import importlib

import numpy as np
import pytest

import clearance_ref as cr
import convex_check_cases as cc
import ladder_ref as lref
import ladder_refine_free_ref as fref
import swept_convex_cases as sc
import swept_ref as sref
import trajectory_free_ref as tfref
import trajectory_multistart_ref as tmref

pytestmark = pytest.mark.gpu
TOL = 1e-9
THR = (1e-4, 1e-4)
DAMPING = 1e-3
EXACT = ("seed_index", "n_tracked", "n_complete", "edge_collision", "n_edge_collisions", "tracked")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


def _sik():
    return importlib.import_module("mink_amd.solve_ik")          # (the package attribute of that name is the function)


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what}: NaN placement")
    np.testing.assert_array_equal(np.isinf(a), np.isinf(b), err_msg=f"{what}: inf placement")
    np.testing.assert_array_equal(a[np.isinf(a)], b[np.isinf(b)], err_msg=f"{what}: inf sign")
    ok = np.isfinite(a)
    err = np.abs(a[ok] - b[ok]).max() if ok.any() else 0.0
    print("  %s: max |device - ref| %.2e over %d finite entries" % (what, err, int(ok.sum())))
    assert err <= TOL, what


def _same(a, b, what):
    assert a._fields == b._fields
    for f in a._fields:
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f"{what}: {f}"
        if x is not None:
            x, y = [v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v) for v in (x, y)]
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {f}")


def _shapes_checker(check_rows, wide=False, sweep_rows=0):
    import mink_amd as mink
    model, spec = cc.shapes_spec(wide)
    return mink.CollisionChecker(model, sc.limit_objects(model, spec), max_rows=256, sweep_rows=sweep_rows, check_rows=check_rows)


def _against_tracking(out, want, B, S, what):
    by = lambda x: tmref.by_instance(x, B, S)
    for f in EXACT:
        np.testing.assert_array_equal(np.asarray(getattr(out, f)).astype(np.int64), np.asarray(want[f]).astype(np.int64), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(out.q, want["q_path"], err_msg=f"{what}: q")
    assert np.abs(out.path_length / want["path_length"] - 1.0).max() <= 1e-12
    _close(out.node_margin, want["node_margin"], f"{what}: node_margin")
    _close(out.edge_margin, want["edge_margin"], f"{what}: edge_margin")
    _close(out.node_margin_all, by(want["node_margin_all"]), f"{what}: node_margin_all")
    _close(out.edge_margin_all, by(want["edge_margin_all"]), f"{what}: edge_margin_all")


# ------------------------------------------------------------------ 1. candidate tracking
def test_candidate_path_on_convex_shapes(nat):
    """`convex_shapes`, T, B, S = 4, 2, 8, three samples per edge, 16-lane rows: 33 of the 64 nodes collide, 21 edges are swept and
    6 of them collide, and a general convex pair attains the margin of 44 nodes and 13 edges (tests/convex_check_cases.py pins the
    counts on the reference alone).  check_rows = 256 holds every row at once."""
    import mink_amd as mink
    (model, limits, q, q_all), want = cc.tracking()
    cc.tracking_counts(want)
    B, S, T, M = (cc.TRACK[k] for k in "BSTM")
    ck = _shapes_checker(256)
    out = mink.candidate_path(mink.Configuration(model, q.copy()), tmref.by_instance(q_all, B, S), collision_check=ck, edge_samples=M)
    ck.close()
    assert isinstance(out, mink.FreeCandidatePath) and out.edge_margin_all.shape == (B, S, T)
    _against_tracking(out, want, B, S, "convex_shapes")
    # the nodes in collision.  (Neither candidate_path nor the native selection returns the status words the check wrote — they
    # are the call's workspace —; the device's own status_all is held against the reference's in the fused test below.)
    hit = ~(out.node_margin_all >= 0.0)
    np.testing.assert_array_equal(hit, tmref.by_instance(want["status_all"], B, S) == tfref.ST_IN_COLLISION)
    assert int(hit.sum()) == 33


def _native_select(ck, q, q_all, M, device=None):
    """mkh_select_trajectory_candidates itself on host arrays or, `device` given, on torch tensors there."""
    import mink_amd as mink
    import torch
    sik = _sik()
    model = ck.model
    cfg = mink.Configuration(model, q.copy())
    prob, layout = sik._compile(cfg, [mink.PostureTask(model, cost=1.0)], None, 1, devices=cfg.devices[:1])
    on = (lambda x: torch.as_tensor(np.ascontiguousarray(x), device=device)) if device is not None else np.ascontiguousarray
    with sik._pin(cfg, layout):
        out, more = prob.select_trajectory_candidates(on(q), on(q_all), None, None, ck, M, True)
    if device is not None:
        torch.cuda.synchronize()
        assert all(x is None or (isinstance(x, torch.Tensor) and x.is_cuda) for x in tuple(out) + tuple(more))
    return out, more


def test_outputs_do_not_depend_on_the_chunking_nor_on_the_pointers(nat):
    """check_rows = 256 (one chunk of the 64 rows), 20 (five rows per chunk and a ragged last one) and 4 (one row per chunk), host
    arrays and device tensors: bit for bit.  R = 16 rows per waypoint: every boundary but the first few separates a row from its
    predecessor row g - R, which the pre-pass and the check read from the candidates, not from the chunk."""
    import torch
    (model, limits, q, q_all), _ = cc.tracking()
    M = cc.TRACK["M"]
    outs = {}
    for rows in (256, 20, 4):
        ck = _shapes_checker(rows)
        outs[rows] = _native_select(ck, q, q_all, M)
        dev = _native_select(ck, q, q_all, M, torch.device("cuda:0"))
        ck.close()
        for a, b in zip(dev, outs[rows]):
            _same(a, b, "device tensors, check_rows = %d" % rows)
    for rows in (20, 4):
        for a, b in zip(outs[rows], outs[256]):
            _same(a, b, "check_rows = %d against 256" % rows)
    assert np.isfinite(outs[256][1].edge_margin_all[1:]).sum() == 21


def test_one_row_per_wavefront(nat):
    """The fixture's pair list in three limits with three minimum distances: 45 pairs, 27 of them general convex — beyond 32 pairs
    a row takes a whole wavefront (the 64-lane builds).  check_rows = 28: seven rows per chunk."""
    import mink_amd as mink
    (model, limits, q, q_all), want = cc.tracking(wide=True)
    B, S, T, M = (cc.TRACK[k] for k in "BSTM")
    assert len(cr.pair_list(limits)[0]) == 45
    ck = _shapes_checker(28, wide=True)
    out = mink.candidate_path(mink.Configuration(model, q.copy()), tmref.by_instance(q_all, B, S), collision_check=ck, edge_samples=M)
    ck.close()
    _against_tracking(out, want, B, S, "45 pairs")


def test_non_finite_rows(nat):
    """Candidate 6: an infinity at waypoint 1 and a NaN at waypoint 2, its successor; candidate 3: an infinity at waypoint 1.
    Those nodes are NaN and in collision; the edges out of them into the free rows (3, 6) and (2, 3) are swept, NaN and collide —
    the pre-pass skips them, and the check must not read what it left out —; every other row is what it is without them."""
    import mink_amd as mink
    (model, limits, q, q_all), clean = cc.tracking()
    B, S, T, M = (cc.TRACK[k] for k in "BSTM")
    q_all = q_all.copy()
    q_all[1, 6, 0] = np.inf
    q_all[2, 6, 5] = np.nan
    q_all[1, 3, -1] = np.inf
    want = tfref.rule(model, limits, q, q_all, None, None, S, M)
    for t, i in ((1, 6), (2, 6), (1, 3)):
        assert np.isnan(want["node_margin_all"][t, i]) and np.isnan(want["edge_margin_all"][t, i]) and want["status_all"][t, i] == 64
    for t, i in ((3, 6), (2, 3)):
        assert want["eligible"][t, i] and np.isnan(want["edge_margin_all"][t, i]) and not want["counted"][t, i]
    ck = _shapes_checker(20)
    out = mink.candidate_path(mink.Configuration(model, q.copy()), tmref.by_instance(q_all, B, S), collision_check=ck, edge_samples=M)
    whole = mink.candidate_path(mink.Configuration(model, q.copy()), tmref.by_instance(cc.tracking()[0][3], B, S), collision_check=ck,
                                edge_samples=M)
    ck.close()
    _against_tracking(out, want, B, S, "non-finite rows")
    touched = np.zeros((T, B * S), dtype=bool)
    for t, i in ((1, 6), (2, 6), (3, 6), (1, 3), (2, 3)):
        touched[t, i] = True
    keep = ~tmref.by_instance(touched, B, S)
    for f in ("node_margin_all", "edge_margin_all"):
        np.testing.assert_array_equal(getattr(out, f)[keep], getattr(whole, f)[keep], err_msg=f)
    _close(whole.node_margin_all, tmref.by_instance(clean["node_margin_all"], B, S), "the clean rows again")


def test_fused_tracking_call_on_ur5e_convex(nat):
    """solve_ik_trajectory_multistart(collision_check=) on `ur5e_convex`, B = 2, T = 3, four seeds, the waypoints the poses of
    fixture rows by the wall (the cylinder-box distance in range) that are free: the
    loops' arrays are the unchecked call's bit for bit, the checked fields are candidate_path's on the returned candidates bit for
    bit, and the whole is the reference's on those rows."""
    import mink_amd as mink
    B, T, S, M, ITERS = 2, 3, 4, 3, 40
    model, _, _ = cr.fixture("ur5e_convex")
    objs = cr.fixture_limits("ur5e_convex")
    limits = cr.limits_of(objs)
    near = cc.ur5e_rows_by_the_wall(free=True)[:B * T]
    tg = mink.Configuration(model, near).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz.reshape(B, T, 7)
    home = np.tile(model.key_qpos[model.name2id("key", "home")], (B, 1))
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)

    def call(**kw):
        cfg = mink.Configuration(model, home.copy())
        return mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: tg}, S, ITERS, *THR, limits=[mink.ConfigurationLimit(model)],
                                                   damping=DAMPING, rng_seed=5, update=False, return_all=True, **kw)

    plain = call()
    ck = mink.CollisionChecker(model, objs, check_rows=2 * (1 + M))          # (two candidate rows per chunk)
    free = call(collision_check=ck, edge_samples=M)
    for f in ("q_all", "v_all", "iters_all", "converged_all", "seeds"):
        np.testing.assert_array_equal(getattr(free, f), getattr(plain, f), err_msg=f)
    assert ((free.status_all & ~mink.ST_IN_COLLISION) == plain.status_all).all()
    el = plain.converged_all & ((plain.status_all & ~1) == 0)
    path = mink.candidate_path(mink.Configuration(model, home.copy()), plain.q_all, el, collision_check=ck, edge_samples=M)
    ck.close()
    for f in ("seed_index", "n_tracked", "n_complete", "path_length", "node_margin", "edge_margin", "edge_collision", "n_edge_collisions",
              "tracked", "node_margin_all", "edge_margin_all", "q"):
        np.testing.assert_array_equal(getattr(free, f), getattr(path, f), err_msg=f)
    tm = lambda x: np.ascontiguousarray(np.moveaxis(x, 2, 0)).reshape((T, B * S) + x.shape[3:])       # (B, S, T, ·) -> (T, B·S, ·)
    want = tfref.rule(model, limits, home, tm(plain.q_all), tm(plain.converged_all).astype(np.int32), tm(plain.status_all), S, M)
    em = want["edge_margin_all"]
    judged = np.concatenate([want["node_margin_all"].ravel(), em[1:][np.isfinite(em[1:])]])
    print("  %d swept edges, nearest reference margin to zero %.2e" % (len(want["swept"]), np.abs(judged).min()))
    assert np.abs(judged).min() > 1e-6                          # (the reference alone separates)
    assert len(want["swept"]) >= 4 and (~(want["node_margin_all"] >= 0.0)).any()       # (the case has edges to sweep and nodes to drop)
    _against_tracking(free, want, B, S, "fused call")
    np.testing.assert_array_equal(tm(free.status_all), want["status_all"])


# ------------------------------------------------------------------ 2. the refinement pass
DISCRETE = ("q", "tracked", "repaired", "refined", "edge_break", "edge_collision", "n_tracked", "n_breaks", "n_edge_collisions")
NODE = ("v", "status", "iters", "converged")
_cases = {}


@contextlib.contextmanager
def _watched(conv, rec):
    """ladder_refine_free_ref's two margin functions, recording which kind of pair attains each margin judged BEHIND the first
    loop launch (the state of the input path comes before): rec["node"] (margin, convex) of every candidate node, rec["edge"]
    (source, destination, margin, convex) of every edge."""
    nm0, em0 = fref.node_margins, fref.edge_margin

    def node_margins(model, limits, rows):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, model.nq)
        if not len(rows):
            return np.zeros(0)
        c = cr.clearance(model, limits, rows)
        if rec["loops"]:
            rec["node"].extend((float(m), bool(conv[p])) for m, p in zip(c.margin, c.pair))
        return c.margin

    def edge_margin(model, limits, a, b, M):
        s = sref.sweep(model, limits, a[None], b[None], M)
        if rec["loops"]:
            rec["edge"].append((np.array(a), np.array(b), float(s.margin[0]), bool(conv[s.pair[0]]), rec["loops"][-1]))
        return float(s.margin[0])

    fref.node_margins, fref.edge_margin = node_margins, edge_margin
    try:
        yield
    finally:
        fref.node_margins, fref.edge_margin = nm0, em0


def _refine_case(name, params=None):
    """The device's pass and the restatement's — the device's loop its callable — on the paths of a checked ladder at few
    iterations; computed once."""
    if name in _cases:
        return _cases[name]
    import mink_amd as mink
    sik = _sik()
    world, B, T, M, gate, low, rng_seed, row0 = params or cc.REFINE[name]
    S, iters = 4, 40
    model, objs, rows, frame, home1 = cc.refine_world(world)
    limits = cr.limits_of(objs)
    conv = cc.convex_mask(model, limits)
    home = np.tile(home1, (B, 1))
    cfg = mink.Configuration(model, home.copy())
    task = mink.FrameTask(*frame, 1.0, 1.0, lm_damping=1.0)
    prob, layout = sik._compile(cfg, [task], [mink.ConfigurationLimit(model)], max(B, 8) * T * S, 1.0, devices=cfg.devices[:1])
    idx = (row0 + np.arange(B * T)) % len(rows)
    tg = np.ascontiguousarray(mink.Configuration(model, rows[idx]).get_transform_frame_to_world(*frame).wxyz_xyz.reshape(B, T, 1, 7))
    # room for all B instances in ONE launch of the check (B = 18 on 16-lane rows: five wavefronts, a ragged last one; one
    # instance per wavefront where the pair list is wide); the incoming path is swept two edges per chunk
    ck = mink.CollisionChecker(model, objs, max_rows=64, sweep_rows=2 * M, check_rows=B * (1 + 2 * M))
    per = 7 if B > 8 else 3                                      # instances per chunk of the second run: 7 + 7 + 4, or 3 + 2
    lean = cc.without_convex(model, limits)
    with sik._pin(cfg, layout):
        lad, _ = prob.solve_trajectory_ladder_free(home, tg, None, None, 1.0, DAMPING, checker=ck, edge_samples=M, n_seeds=S,
                                                   max_iters=low, pos_threshold=THR[0], ori_threshold=THR[1], max_step_sq=gate,
                                                   rng_seed=rng_seed)
        trk = lref.tracked(lad.converged, lad.status)
        nodes = dict(v=lad.v, status=lad.status, iters=lad.iters, converged=lad.converged)
        rec = dict(node=[], edge=[], loops=[])

        def loop(t, start):
            out = prob.solve(start, np.ascontiguousarray(tg[:, t]), None, None, 1.0, DAMPING, n_steps=iters, until=THR)
            rec["loops"].append((len(rec["loops"]) < T, np.array(out[0])))       # (forward?, x)
            return out

        judged, margins, counts = [], [], {}
        with _watched(conv, rec):
            want = fref.refine(model, limits, loop, home, lad.q, trk, M, gate, judged=judged, margins=margins, counts=counts, **nodes)
        # the same pass as a checker without its general convex pairs would run it
        rec_loops, rec["loops"] = rec["loops"], []
        lean_want = fref.refine(model, lean, loop, home, lad.q, trk, M, gate, **nodes) if lean else None
        rec["loops"] = rec_loops
        kw = dict(max_iters=iters, pos_threshold=THR[0], ori_threshold=THR[1], edge_samples=M, max_step_sq=gate, **nodes)
        got = prob.ladder_refine_free(home, lad.q, ck, trk, tg, None, None, 1.0, DAMPING, **kw)
        chunked = {}
        for n in (per, 1):                                       # (chunks behind the first start at an offset; one instance per chunk)
            part = mink.CollisionChecker(model, objs, max_rows=64, sweep_rows=64 * M, check_rows=n * (1 + 2 * M))
            chunked[n] = prob.ladder_refine_free(home, lad.q, part, trk, tg, None, None, 1.0, DAMPING, **kw)
            part.close()
    ck.close()
    print(f"{name}: {world} B={B} T={T} M={M}; the ladder tracks {lad.n_tracked.tolist()}; counters {counts}; refined "
          f"{want['refined'].tolist()}; n_tracked {want['n_tracked'].tolist()}")
    _cases[name] = dict(model=model, B=B, T=T, gate=gate, got=got, chunked=chunked, want=want, lean=lean_want, judged=judged,
                        margins=margins, counts=counts, lad=lad, rec=rec)
    return _cases[name]


def _convex_facts(c):
    """(rejected nodes whose margin a general convex pair attains, accepted repairs whose near-edge margin one attains): the near
    edge runs INTO the loop's result in the forward sweep and OUT of it in the backward sweep."""
    rec = c["rec"]
    nodes = sum(1 for m, cv in rec["node"] if not (m >= 0.0) and cv)
    near = 0
    for a, b, m, cv, (forward, x) in rec["edge"]:
        end = b if forward else a
        if cv and m >= 0.0 and (x == end[None, :]).all(axis=1).any():
            near += 1
    return nodes, near


@pytest.mark.parametrize("name", list(cc.REFINE))
def test_pass_is_the_restatement(nat, name):
    c = _refine_case(name)
    got, want, gate, B, T = c["got"], c["want"], c["gate"], c["B"], c["T"]
    # ---- the conditions under which the discrete choices are rounding-proof, on the reference alone
    mg = np.array([x for x in c["margins"] if np.isfinite(x)])
    cost = np.array([x for _, x in c["judged"] if np.isfinite(x)])
    near = np.abs(cost - gate) / gate if (np.isfinite(gate) and cost.size) else np.array([np.inf])
    gaps = []
    for b in range(B):
        kp, kr = want["key_in"][b], want["key_work"][b]
        if kp[:2] == kr[:2] and want["work_repaired"][b].any():
            gaps.append(abs(kp[2] - kr[2]) / max(abs(kp[2]), abs(kr[2])))
    print(f"  {len(mg)} margins judged, nearest to zero {np.abs(mg).min() if mg.size else np.inf:.3e}; {len(cost)} edge costs judged, "
          f"nearest to the gate {near.min():.3e} relative; tied keys with repairs: {len(gaps)}")
    assert mg.size == 0 or np.abs(mg).min() > 1e-6
    assert near.min() > 1e-9
    assert all(g > 1e-9 for g in gaps)
    # ---- the device against the restatement
    for f in DISCRETE + NODE:
        np.testing.assert_array_equal(getattr(got, f), want[f], err_msg=f"{name}: {f}")
    _close(got.node_margin, want["node_margin"], "node_margin")
    _close(got.edge_margin, want["edge_margin"], "edge_margin")
    rel = np.abs(got.path_length - want["path_length"]) / np.maximum(np.abs(want["path_length"]), np.finfo(float).tiny)
    assert rel.max() <= (c["model"].nv + T) * 2.0 ** -52
    # ---- three instances per chunk and one instance per chunk of the check against all of them in one launch: bit for bit
    for n, part in c["chunked"].items():
        _same(part, got, "check_rows = %d (1 + 2M)" % n)


def test_the_cases_take_every_branch(nat):
    """Over the cases every counter of the restatement is at least 1; a general convex pair attains the margin of a rejected node
    and the near-edge margin of an accepted repair; and without the general convex pairs some case repairs or tracks otherwise."""
    total = dict.fromkeys(fref.COUNTERS, 0)
    nodes = near = differs = 0
    for name in cc.REFINE:
        c = _refine_case(name)
        for k, v in c["counts"].items():
            total[k] += v
        n, e = _convex_facts(c)
        nodes, near = nodes + n, near + e
        if c["lean"] is not None:
            differs += int((c["lean"]["repaired"] != c["want"]["repaired"]).any() or (c["lean"]["n_tracked"] != c["want"]["n_tracked"]).any())
    print(total, "rejected nodes decided by a general convex pair:", nodes, "accepted near edges:", near, "cases that differ without:", differs)
    assert all(total[k] >= 1 for k in fref.COUNTERS), total
    assert nodes >= 1 and near >= 1 and differs >= 1


def test_more_instances_than_four_wavefronts(nat):
    """B = 18 on 16-lane rows, T = 2, against the restatement.  check_rows holds all 18 instances: ONE launch of the check on five
    wavefronts of four instances, the last one ragged; seven instances per chunk (two wavefronts, the chunks behind the first at
    an offset) and one instance per chunk are the same bit for bit."""
    c = _refine_case("many", cc.MANY)
    for f in DISCRETE + NODE:
        np.testing.assert_array_equal(getattr(c["got"], f), c["want"][f], err_msg=f)
    mg = np.array([x for x in c["margins"] if np.isfinite(x)])
    assert mg.size and np.abs(mg).min() > 1e-6
    _close(c["got"].node_margin, c["want"]["node_margin"], "node_margin")
    _close(c["got"].edge_margin, c["want"]["edge_margin"], "edge_margin")
    assert sorted(c["chunked"]) == [1, 7]
    for n, part in c["chunked"].items():
        _same(part, c["got"], "check_rows = %d (1 + 2M)" % n)


@pytest.mark.parametrize("n_nodes", [None, 2])
def test_fused_refined_call_is_the_composition(nat, n_nodes):
    """solve_ik_trajectory_ladder(collision_check=, refine="free") on `ur5e_convex` is the checked ladder followed by refine_path's
    native call on its path: bit for bit, with and without n_nodes."""
    import mink_amd as mink
    sik = _sik()
    B, T, S, M, ITERS = 3, 4, 4, 2, 12
    model, objs, _, frame, home1 = cc.refine_world("ur5e_convex")
    # waypoints close to each other by the wall: the poses along short joint-space lines out of free rows there, so that the pass
    # has something it can heal from a neighbour within the rungs' own iterations
    first = cc.ur5e_rows_by_the_wall(free=True)[:B]
    line = first[:, None, :] + np.arange(T)[None, :, None] * np.random.default_rng(11).uniform(-0.06, 0.06, size=(B, 1, model.nq))
    tg = mink.Configuration(model, line.reshape(-1, model.nq)).get_transform_frame_to_world(*frame).wxyz_xyz.reshape(B, T, 7)
    home = np.tile(home1, (B, 1))
    task = mink.FrameTask(*frame, 1.0, 1.0, lm_damping=1.0)
    ck = mink.CollisionChecker(model, objs, sweep_rows=5 * M, check_rows=1 + 2 * M)
    more = {} if n_nodes is None else dict(n_nodes=n_nodes)

    def call(**kw):
        cfg = mink.Configuration(model, home.copy())
        return cfg, mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, S, ITERS, *THR, limits=[mink.ConfigurationLimit(model)],
                                                    damping=DAMPING, rng_seed=5, update=False, collision_check=ck, edge_samples=M, **more, **kw)

    cfg, checked = call()
    _, fused = call(refine="free")
    trk = checked.converged & ((checked.status & ~1) == 0)
    prob, layout = sik._compile(cfg, [task], [mink.ConfigurationLimit(model)], B * T * S, 1.0, devices=cfg.devices[:1])
    with sik._pin(cfg, layout):
        two = prob.ladder_refine_free(home, checked.q, ck, trk, np.ascontiguousarray(tg[:, :, None, :]), None, None, 1.0, DAMPING,
                                      max_iters=ITERS, pos_threshold=THR[0], ori_threshold=THR[1], edge_samples=M,
                                      v=checked.v, status=checked.status, iters=checked.iters, converged=checked.converged.astype(np.int32))
    ck.close()
    for f in ("q", "v", "status", "iters", "repaired", "n_tracked", "n_breaks", "path_length", "n_edge_collisions", "edge_margin"):
        np.testing.assert_array_equal(getattr(fused, f), getattr(two, f), err_msg=f)
    for f in ("converged", "refined", "edge_break", "edge_collision"):
        np.testing.assert_array_equal(getattr(fused, f), getattr(two, f).astype(bool), err_msg=f)
    np.testing.assert_array_equal(fused.node_index, checked.node_index)
    assert (fused.n_tracked >= checked.n_tracked).all()
    assert fused.refined.any() and (fused.repaired != 0).any()  # (the case's condition: something was there to refine)
    print(f"n_nodes {n_nodes}: checked n_tracked {checked.n_tracked.tolist()}, refined {fused.refined.astype(int).tolist()}: "
          f"{fused.n_tracked.tolist()}, repaired {fused.repaired.tolist()}")


# ------------------------------------------------------------------ 3. limits, refusals, checkers without such pairs
def test_limits_and_refusals(nat):
    import mink_amd as mink
    (model, limits, q, q_all), _ = cc.tracking()
    B, S, T, M = (cc.TRACK[k] for k in "BSTM")
    cfg = mink.Configuration(model, q.copy())
    paths = tmref.by_instance(q_all, B, S)
    L = nat.lib()
    # ---- tracking: less than one item is a limit, one item serves
    ck = _shapes_checker(M)
    with pytest.raises(nat.MinkHipError, match=r"error -4: .*check_rows = 3 .*one item of 4 rows"):
        mink.candidate_path(cfg, paths, collision_check=ck, edge_samples=M)
    assert mink.candidate_path(cfg, paths, collision_check=ck, edge_samples=M - 1).edge_margin_all.shape == (B, S, T)
    # the handle itself: a refused size leaves the buffer alone; 0 restores the refusal, its message naming the way out
    prob = next(iter(ck._handles.values()))[1]
    assert L.mkh_problem_set_check_rows(prob.handle, -1) == -1
    assert L.mkh_problem_set_check_rows(prob.handle, 1 << 62) == -4
    assert mink.candidate_path(cfg, paths, collision_check=ck, edge_samples=M - 1).edge_margin_all.shape == (B, S, T)
    prob.set_check_rows(0)
    with pytest.raises(nat.MinkHipError, match=r"error -1: .*general convex pairs.*check_rows"):
        mink.candidate_path(cfg, paths, collision_check=ck, edge_samples=M - 1)
    assert L.mkh_problem_set_check_rows(None, 4) == -1 and b"null problem" in L.mkh_last_error()
    ck.close()
    # ---- refinement: check_rows without sweep_rows, 2M rows, and sweep_rows below one edge
    cmodel, objs, rows, frame, home1 = cc.refine_world("ur5e_convex")
    ccfg = mink.Configuration(cmodel, home1.copy())
    ctask = mink.FrameTask(*frame, 1.0, 1.0, lm_damping=1.0)
    tg = mink.Configuration(cmodel, rows[:2]).get_transform_frame_to_world(*frame).wxyz_xyz.reshape(2, 7)
    refine = lambda c, M_: mink.refine_path(ccfg, [ctask], 1.0, {ctask: tg}, rows[:2], collision_check=c, edge_samples=M_, update=False)
    fused = lambda c, M_: mink.solve_ik_trajectory_ladder(ccfg, [ctask], 1.0, {ctask: tg}, 2, 3, *THR, update=False, collision_check=c,
                                                          edge_samples=M_, refine="free")
    for call in (refine, fused):
        c = mink.CollisionChecker(cmodel, objs, check_rows=64)
        with pytest.raises(nat.MinkHipError, match=r"error -1: .*general convex pairs.*sweep_rows"):
            call(c, 2)
        c.close()
        c = mink.CollisionChecker(cmodel, objs, sweep_rows=64, check_rows=4)
        with pytest.raises(nat.MinkHipError, match=r"error -4: .*check_rows = 4 .*one item of 5 rows"):
            call(c, 2)
        c.close()
        c = mink.CollisionChecker(cmodel, objs, sweep_rows=1, check_rows=64)
        with pytest.raises(nat.MinkHipError, match=r"error -4: .*sweep_rows = 1 .*n_samples = 2"):
            call(c, 2)
        c.close()
    c = mink.CollisionChecker(cmodel, objs, sweep_rows=2, check_rows=5)
    assert refine(c, 2).q.shape == (2, cmodel.nq)
    c.close()


def test_check_rows_changes_nothing_without_general_convex_pairs(nat):
    """`ur5e_all`: 14 capsule pairs; one tracking call and one refinement call with check_rows = 64 against 0, bit for bit."""
    import mink_amd as mink
    model, spec, rows = cr.fixture("ur5e_all")
    B, S, T, M = 2, 3, 3, 2
    q = np.tile(model.key_qpos[model.name2id("key", "home")], (B, 1))
    paths = np.ascontiguousarray(rows[:B * S * T].reshape(B, S, T, model.nq))
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    tg = mink.Configuration(model, rows[40:40 + B * T]).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz.reshape(B, T, 7)
    outs = []
    for n in (0, 64):
        ck = mink.CollisionChecker(model, cr.fixture_limits("ur5e_all"), check_rows=n)
        cfg = mink.Configuration(model, q.copy())
        outs.append((mink.candidate_path(cfg, paths, collision_check=ck, edge_samples=M),
                     mink.refine_path(cfg, [task], 1.0, {task: tg}, paths[:, 0], limits=[mink.ConfigurationLimit(model)], update=False,
                                      collision_check=ck, edge_samples=M, max_iters=20, damping=DAMPING)))
        ck.close()
    for a, b in zip(outs[0], outs[1]):
        _same(a, b, "check_rows 64 against 0")
