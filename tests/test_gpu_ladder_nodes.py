"""The ladder on deduplicated nodes and the turn unwinding on the device (mkh_unwind_turns, MKH_FLAG_UNWIND_TURNS,
mkh_solve_trajectory_ladder_nodes and the public calls on them): the unwinding is the stated rule bit for bit, the fused call is
the three-call composition bit for bit and the numpy rule on the same loops, its invariants against the plain ladder hold, it
runs where the plain ladder's search cannot, and the result depends on neither chunks, the kind of array nor the seeds' source."""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import ladder_nodes_ref as lnref
import ladder_ref as ref
import test_gpu_ladder as tl
import test_gpu_multistart as tm
import test_gpu_trajectory_multistart as tms
import unwind_cases as uc
import unwind_ref as uw
from mink_amd import workloads

pytestmark = pytest.mark.gpu
CHOSEN = ("q", "v", "status", "iters", "converged")
SEARCH = ("node_index", "n_tracked", "n_breaks", "path_length", "edge_break")
SETS = ("node_seed_index", "node_multiplicity", "node_distance", "n_distinct", "n_converged", "n_uncovered", "seed_index")
R = 0.1


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _np(x):
    return None if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy())


def _same(got, want, what):
    """Bitwise, NaN rows included."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float64:
        got, want = np.ascontiguousarray(got).view(np.int64), np.ascontiguousarray(want).view(np.int64)
    np.testing.assert_array_equal(got, want, err_msg=what)


# ------------------------------------------------------------------ 1. the unwinding is the rule, bitwise
_plain_handles = {}


def _plain_handle(nat, name):
    """(model, handle): the unwinding only reads the model's joint table through the handle."""
    if name not in _plain_handles:
        m = uc.turns_model() if name == "turns" else workloads.load_robot(name)
        nm = nat.NativeModel(m, 0)
        prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "body", "frame_id": m.nbody - 1, "cost": [1.0] * 6}], max_batch=1)
        _plain_handles[name] = (m, nm, prob)
    return _plain_handles[name][0], _plain_handles[name][2]


@pytest.mark.parametrize("name", ["ur5e", "g1", "turns"])
def test_unwinding_is_the_rule_bitwise(nat, name):
    """64 rows x 3 references with the designed rows in front (tests/unwind_cases.py): UR5e (limited hinges of two turns and
    the elbow, which is not eligible), G1 (a free joint and limited hinges of less than a turn: every entry a bit copy) and the
    turns model (free joint, unlimited hinge, a hinge of three turns, short hinge, slide, ball)."""
    import torch
    m, prob = _plain_handle(nat, name)
    rows, q_ref = uc.designed_rows(m)
    want = uw.unwind(m, rows, q_ref, 64)
    got = prob.unwind_turns(rows, q_ref)
    _same(got, want, f"{name}: host arrays")
    moved = int((got.view(np.int64) != rows.view(np.int64)).sum())
    print(f"{name}: {len(uw.eligible(m))} eligible joints, {moved} of {rows.size} entries moved")
    assert (moved > 0) == (name != "g1")
    _same(prob.unwind_turns(got, q_ref), got, f"{name}: idempotent")
    three = prob.unwind_turns(rows.reshape(3, 64, m.nq), q_ref)                  # (B, S, nq) in, the same rows out
    _same(three.reshape(-1, m.nq), want, f"{name}: (B, S, nq)")
    in_place = rows.copy()
    assert prob.unwind_turns(in_place, q_ref, out=in_place) is in_place         # q_out == q_rows
    _same(in_place, want, f"{name}: in place")
    dev = torch.device("cuda:0")
    t_rows = torch.as_tensor(rows, device=dev)
    t_out = prob.unwind_turns(t_rows, torch.as_tensor(q_ref, device=dev))
    assert isinstance(t_out, torch.Tensor) and t_out.device.type == "cuda"
    _same(t_out, want, f"{name}: torch")
    _same(t_rows, rows, f"{name}: torch input untouched")
    assert prob.unwind_turns(t_rows, torch.as_tensor(q_ref, device=dev), out=t_rows) is t_rows
    _same(t_rows, want, f"{name}: torch in place")
    one = prob.unwind_turns(rows[:5], q_ref[:1])                                 # one block, a tail
    _same(one, want[:5], f"{name}: 5 rows")


# ------------------------------------------------------------------ 2. the fused call is the composition, bitwise
_far_handles = {}


def _far_world(nat, B, T, max_batch):
    """The far UR5e paths of tests/test_gpu_trajectory_multistart.py at the native level: one FrameTask on attachment_site
    (costs 1 / 1, lm_damping 1), ConfigurationLimit, every loop from `home`, dt = 1, damping 1e-3, thresholds 1e-4 / 1e-4, 40
    iterations.  Seeds drawn over the joints' two turns reach several IK branches, each on several turns."""
    from mink_amd.api_specs import configuration_limit_desc
    m, tg = tms._far_paths()
    if max_batch not in _far_handles:
        nm = nat.NativeModel(m, 0)
        prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "attachment_site"),
                                                   "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 1.0}],
                                 configuration_limits=[configuration_limit_desc(m)], max_batch=max_batch)
        _far_handles[max_batch] = (nm, prob)
    nm, prob = _far_handles[max_batch]
    q = np.tile(m.key_qpos[m.name2id("key", "home")], (B, 1))
    return SimpleNamespace(m=m, nm=nm, prob=prob, q=q, tg=np.ascontiguousarray(tg[:B, :T, None, :]), pt=None, ct=None, dt=1.0,
                           damping=1e-3, until=(1e-4, 1e-4), iters=40)


def _gather(rows, index, S):
    """rows (B, T, S, ...) through index (B, T, K) — -1 (an empty slot) reads candidate 0."""
    idx = np.maximum(index, 0)
    idx = idx.reshape(idx.shape + (1,) * (rows.ndim - 3))
    return np.take_along_axis(rows, idx, axis=2)


def _compose(w, S, K, r, gate, wts, unwind, plain):
    """The three host-composed calls on the plain ladder's rungs: (candidates, select_distinct's result, ladder_select's)."""
    B, T = plain.q_all.shape[:2]
    nq = w.m.nq
    trk = ref.tracked(plain.converged_all, plain.status_all)
    cand = plain.q_all
    if unwind:
        cand = w.prob.unwind_turns(np.ascontiguousarray(plain.q_all.reshape(B, T * S, nq)), w.q).reshape(B, T, S, nq)
    sel = w.prob.select_distinct(np.ascontiguousarray(cand.reshape(B * T, S, nq)), trk.reshape(B * T, S), np.repeat(w.q, T, axis=0), wts,
                                 n_solutions=K, min_distance=r)
    path = w.prob.ladder_select(w.q, sel.q.reshape(B, T, K, nq), (sel.seed_index >= 0).reshape(B, T, K), gate, wts)
    return trk, cand, sel, path


def _check_fused(nat, name, w, B, T, S, K, max_iters=None):
    m, prob = w.m, w.prob
    nq = m.nq
    wts = np.random.default_rng(2).uniform(0.5, 2.0, size=m.nv)
    gate = 1.0
    kw = tl._kw(w, S, rng_seed=8, weights=wts, max_step_sq=gate, qvel_dt=0.05)
    if max_iters is not None:
        kw["max_iters"] = max_iters
    args = (w.q, w.tg, w.pt, w.ct, w.dt, w.damping)
    plain = prob.solve_trajectory_ladder(*args, return_all=True, **kw)
    excluded = total = 0
    for unwind in (False, True):
        trk, cand, sel, path = _compose(w, S, K, R, gate, wts, unwind, plain)
        fused = prob.solve_trajectory_ladder_nodes(*args, n_nodes=K, min_distance=R, unwind_turns=unwind, return_all=True, **kw)
        what = f"{name} unwind={unwind}"
        if unwind:
            _same(cand.reshape(-1, nq), uw.unwind(m, plain.q_all.reshape(-1, nq), w.q, T * S), f"{what}: the unwound loop results")
        # the nodes are select_distinct's slots, their rows the loops' rows of those candidates
        si = sel.seed_index.reshape(B, T, K)
        _same(fused.q_all, sel.q.reshape(B, T, K, nq), f"{what}: q_all")
        _same(fused.q_all, _gather(cand, si, S), f"{what}: q_all are candidates")
        for f, src in (("v_all", plain.v_all), ("status_all", plain.status_all), ("iters_all", plain.iters_all),
                       ("converged_all", plain.converged_all)):
            _same(getattr(fused, f), _gather(src, si, S), f"{what}: {f}")
        _same(fused.seeds, plain.seeds, f"{what}: seeds")
        _same(fused.node_seed_index, si, f"{what}: node_seed_index")
        _same(fused.node_multiplicity, sel.multiplicity.reshape(B, T, K), f"{what}: node_multiplicity")
        _same(fused.node_distance, sel.distance.reshape(B, T, K), f"{what}: node_distance")
        _same(fused.n_distinct, sel.n_distinct.reshape(B, T), f"{what}: n_distinct")
        _same(fused.n_converged, sel.n_valid.reshape(B, T), f"{what}: n_converged")
        _same(fused.n_uncovered, sel.n_uncovered.reshape(B, T), f"{what}: n_uncovered")
        # the search is ladder_select on those nodes; the chosen rows are the chosen nodes'
        for f in SEARCH:
            _same(getattr(fused, f), getattr(path, f), f"{what}: {f}")
        _same(fused.q, path.q, f"{what}: q")
        pick = fused.node_index[..., None]
        for f, src in (("v", fused.v_all), ("status", fused.status_all), ("iters", fused.iters_all), ("converged", fused.converged_all),
                       ("seed_index", fused.node_seed_index)):
            idx = pick.reshape(pick.shape + (1,) * (src.ndim - 3))
            _same(getattr(fused, f), np.take_along_axis(src, idx, axis=2)[:, :, 0], f"{what}: {f}")
        assert fused.tracked is None and fused.repaired is None and fused.refined is None
        # the numpy rule on the same loop results, rungs with a decision within 1e-9 of a tie excluded
        nodes = lnref.nodes(m, w.q, plain.q_all, trk, K, R, wts, unwind)
        keep = ~nodes.near_tie
        excluded += int((~keep).sum()); total += keep.size
        for f, g in (("node_seed_index", "seed_index"), ("node_multiplicity", "multiplicity")):
            np.testing.assert_array_equal(getattr(fused, f)[keep], getattr(nodes, g)[keep], err_msg=f"{what}: numpy: {f}")
        for f in ("n_distinct", "n_converged", "n_uncovered"):
            np.testing.assert_array_equal(getattr(fused, f)[keep], getattr(nodes, f)[keep], err_msg=f"{what}: numpy: {f}")
        _same(fused.q_all[keep], nodes.q[keep], f"{what}: numpy: node rows")
        filled = keep[..., None] & (nodes.seed_index >= 0)
        assert np.isposinf(fused.node_distance[fused.node_seed_index < 0]).all()
        if filled.any():                                           # (the one computed double: 1e-12 relative, as the set's tests hold it)
            assert np.abs(fused.node_distance[filled] / nodes.distance[filled] - 1.0).max() <= 1e-12
        if keep.all():                                             # the search on numpy's nodes: the same keys
            want = ref.select(m, w.q, nodes.q, nodes.tracked, wts, gate)
            np.testing.assert_array_equal(fused.n_tracked, want["n_tracked"])
            np.testing.assert_array_equal(fused.n_breaks, want["n_breaks"])
            assert np.abs(fused.path_length / want["path_length"] - 1.0).max() <= 1e-12
        print(f"{what}: n_distinct {fused.n_distinct.ravel().tolist()}, n_uncovered {int(fused.n_uncovered.sum())}, "
              f"n_tracked {fused.n_tracked.tolist()}, n_breaks {fused.n_breaks.tolist()}, near ties {int((~keep).sum())}")
        # with refine: the pass alone on the fused search's path, bitwise
        fine = prob.solve_trajectory_ladder_nodes(*args, n_nodes=K, min_distance=R, unwind_turns=unwind, refine=True, **kw)
        chosen_trk = np.take_along_axis(fused.node_seed_index >= 0, pick, axis=2)[:, :, 0]
        two = prob.ladder_refine(w.q, fused.q, chosen_trk, w.tg, w.pt, w.ct, w.dt, w.damping, max_iters=kw["max_iters"],
                                 pos_threshold=kw["pos_threshold"], ori_threshold=kw["ori_threshold"], max_step_sq=gate, weights=wts,
                                 v=fused.v, status=fused.status, iters=fused.iters, converged=fused.converged)
        for f in ("q", "v", "status", "iters", "converged", "tracked", "repaired", "refined", "edge_break", "n_tracked", "n_breaks",
                  "path_length"):
            _same(getattr(fine, f), getattr(two, f), f"{what}: refined: {f}")
        for f in ("node_index",) + SETS:
            _same(getattr(fine, f), getattr(fused, f), f"{what}: refined: {f} is the search's")
        print(f"{what}: refined {fine.refined.tolist()}, repaired {int((fine.repaired > 0).sum())} waypoints")
    assert excluded <= 0.05 * total, (excluded, total)
    return w, plain


def test_fused_call_is_the_composition_ur5e(nat):
    """B = 3, T = 5, S = 16, K = 4 on the far UR5e paths: every output of the fused call against unwind_turns ->
    select_distinct -> ladder_select on the plain ladder's return_all, against the numpy rule on the same loops, and the
    refined call against ladder_refine on the fused search's path.

    CPU check of this fixture (the C oracle's solve + the numpy oracle's integration and error test, the loop of
    test_gpu_wide.py::_oracle_loop on the seeds of multistart_ref.draw_seeds, rng_seed 8, the test's weights): of the 15 rungs
    none has a decision within 1e-9 relative of a tie, raw or unwound — inside the 5 % the exclusion may take; n_distinct per
    rung [4, 4, 4, 4, 4, 1, 4, 3, 4, 4, 4, 4, 4, 4, 4] raw and [4, 4, 4, 4, 4, 1, 3, 3, 4, 3, 4, 4, 4, 4, 4] unwound, n_uncovered
    44 and 20: 13 rungs hold more candidates than slots.  The device gives the same figures."""
    B, T, S, K = 3, 5, 16, 4
    w, plain = _check_fused(nat, "ur5e far", _far_world(nat, B, T, B * T * S), B, T, S, K)
    per_rung = ref.tracked(plain.converged_all, plain.status_all).sum(axis=2)
    assert (per_rung > K).any() and (per_rung == 0).sum() <= 3, per_rung           # rungs with more candidates than slots


def test_fused_call_is_the_composition_g1(nat):
    """A free joint and 37 short hinges: B = 2, T = 3, S = 8, K = 3 (the unwinding is the identity on this robot)."""
    _check_fused(nat, "g1_c3", tl._real(nat, "g1_c3", 2, 3, 8), 2, 3, 8, 3)


# ------------------------------------------------------------------ 3. invariants against the plain ladder
def test_invariants_against_the_plain_ladder(nat):
    B, T, S, K = 6, 4, 16, 3
    w = _far_world(nat, B, T, B * T * S)
    wts, gate = None, 1.0
    kw = tl._kw(w, S, rng_seed=11, max_step_sq=gate)
    args = (w.q, w.tg, w.pt, w.ct, w.dt, w.damping)
    plain = w.prob.solve_trajectory_ladder(*args, return_all=True, **kw)
    trk = ref.tracked(plain.converged_all, plain.status_all)
    for unwind in (False, True):
        out = w.prob.solve_trajectory_ladder_nodes(*args, n_nodes=K, min_distance=R, unwind_turns=unwind, return_all=True, **kw)
        _same(out.n_tracked, plain.n_tracked, f"unwind={unwind}: n_tracked")
        for b in range(B):
            mine = (T - out.n_tracked[b], out.n_breaks[b], out.path_length[b])
            theirs = (T - plain.n_tracked[b], plain.n_breaks[b], plain.path_length[b])
            if not unwind:                                         # (unwound nodes are no subset of the raw candidates' rows)
                assert mine >= theirs, (b, mine, theirs)
        # the set rule's bookkeeping
        np.testing.assert_array_equal(out.n_converged, trk.sum(axis=2))
        np.testing.assert_array_equal(out.node_multiplicity.sum(axis=2) + out.n_uncovered, out.n_converged)
        np.testing.assert_array_equal((out.node_seed_index >= 0).sum(axis=2), out.n_distinct)
        np.testing.assert_array_equal(out.n_distinct, np.minimum(out.n_distinct, K))
        assert ((out.n_distinct == 0) == (out.n_converged == 0)).all()
        assert ((out.n_uncovered > 0) <= (out.n_distinct == K)).all()
        filled = out.node_seed_index >= 0
        d = np.where(filled, out.node_distance, np.inf)
        assert (d[..., 1:] >= d[..., :-1]).all() and np.isposinf(out.node_distance[~filled]).all()     # ascending d_ref, +inf behind
        assert trk[np.nonzero(filled)[0], np.nonzero(filled)[1], out.node_seed_index[filled]].all()
        print(f"unwind={unwind}: key (lost, breaks, length) per instance "
              f"{[(int(T - out.n_tracked[b]), int(out.n_breaks[b]), round(float(out.path_length[b]), 4)) for b in range(B)]}; plain "
              f"{[(int(T - plain.n_tracked[b]), int(plain.n_breaks[b]), round(float(plain.path_length[b]), 4)) for b in range(B)]}")
    # K >= S, r = 0, no unwinding: where every rung holds a tracked candidate the path is the plain ladder's (include/minkhip.h:
    # on a rung nobody tracked this call holds candidate 0's row only)
    S2 = 8
    kw2 = tl._kw(w, S2, rng_seed=11, max_step_sq=gate)
    plain2 = w.prob.solve_trajectory_ladder(*args, **kw2)
    same = w.prob.solve_trajectory_ladder_nodes(*args, n_nodes=S2 + 1, min_distance=0.0, **kw2)
    full = plain2.n_tracked == T
    assert full.sum() >= B // 2, plain2.n_tracked
    _same(same.n_tracked, plain2.n_tracked, "K >= S: n_tracked")
    for f in ("q", "n_breaks", "path_length", "v", "status", "iters", "converged", "edge_break"):
        _same(getattr(same, f)[full], getattr(plain2, f)[full], f"K >= S: {f}")
    _same(same.seed_index[full], plain2.node_index[full], "K >= S: the chosen candidates")
    for b in np.flatnonzero(~full):
        assert (same.n_breaks[b], same.path_length[b]) >= (plain2.n_breaks[b], plain2.path_length[b])


# ------------------------------------------------------------------ 4. beyond the search's limit
def test_more_candidates_than_the_search_holds(nat):
    """S = 320 candidates per rung: the plain call refuses (back-pointers are bytes), the fused call searches on K = 4 nodes."""
    B, T, S, K = 2, 3, 320, 4
    w = _far_world(nat, B, T, B * T * S)
    m, prob = w.m, w.prob
    f8, i4 = np.float64, np.int32
    out = {"q_traj": np.empty((B, T, m.nq), f8), "v_traj": np.empty((B, T, m.nv), f8), "status": np.empty((B, T), i4),
           "iters": np.empty((B, T), i4), "converged": np.empty((B, T), i4), "node_index": np.empty((B, T), i4),
           "n_tracked": np.empty(B, i4), "n_breaks": np.empty(B, i4), "path_length": np.empty(B, f8), "edge_break": np.empty((B, T), i4)}
    io = nat.MkhTrajectoryLadderIO()
    for name, x in out.items():
        setattr(io, name, x.ctypes.data)
    io.max_step_sq = float("inf")
    q, tg = np.ascontiguousarray(w.q), np.ascontiguousarray(w.tg)
    rc = nat.lib().mkh_solve_trajectory_ladder(prob.handle, B, T, S, q.ctypes.data, tg.ctypes.data, None, None, float(w.dt),
                                               float(w.damping), w.iters, w.until[0], w.until[1], 8, 0, ctypes.byref(io), 0, None)
    assert rc == -4 and b"at most 256" in nat.lib().mkh_last_error()              # MKH_E_LIMIT
    with pytest.raises(ValueError, match="at most 256"):
        prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, **tl._kw(w, S))
    got = prob.solve_trajectory_ladder_nodes(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, n_nodes=K, min_distance=R, rng_seed=8,
                                             **tl._kw(w, S))
    assert got.q.shape == (B, T, m.nq) and got.node_seed_index.shape == (B, T, K)
    assert (got.n_tracked >= 1).all() and (got.n_converged <= S).all() and got.node_seed_index.max() < S
    assert ((got.node_index >= 0) & (got.node_index < K)).all()
    np.testing.assert_array_equal((got.seed_index >= 0).sum(axis=1), got.n_tracked)
    # slot 0 of every rung is multi-start's choice on the flattened targets (the set's invariant), at S = 320
    ms = prob.solve_multistart(np.repeat(w.q, T, axis=0), w.tg.reshape(B * T, *w.tg.shape[2:]), w.pt, w.ct, w.dt, w.damping,
                               rng_seed=8, **tl._kw(w, S))
    some = ms.n_converged > 0
    np.testing.assert_array_equal(got.node_seed_index[:, :, 0].ravel()[some], ms.seed_index[some])
    assert (got.node_seed_index[:, :, 0].ravel()[~some] == -1).all()
    np.testing.assert_array_equal(got.n_converged.ravel(), ms.n_converged)
    print(f"S = {S}: tracked candidates per rung {got.n_converged.ravel().tolist()}, distinct {got.n_distinct.ravel().tolist()}, "
          f"uncovered {got.n_uncovered.ravel().tolist()}")


# ------------------------------------------------------------------ 5. the plumbing
def test_result_does_not_depend_on_the_plumbing(nat):
    import torch
    B, T, S, K = 3, 5, 16, 4
    w = _far_world(nat, B, T, B * T * S)
    m = w.m
    wts = np.random.default_rng(2).uniform(0.5, 2.0, size=m.nv)
    kw = dict(tl._kw(w, S, rng_seed=8, weights=wts, max_step_sq=1.0, qvel_dt=0.05), n_nodes=K, min_distance=R, unwind_turns=True,
              refine=True, return_all=True)
    args = (w.q, w.tg, w.pt, w.ct, w.dt, w.damping)
    whole = w.prob.solve_trajectory_ladder_nodes(*args, **kw)

    def same(other, what):
        for f in whole._fields:
            if getattr(whole, f) is not None:
                _same(getattr(other, f), getattr(whole, f), f"{what}: {f}")

    # max_batch: one rung per chunk, and two rungs per chunk with a tail (15 rungs)
    for mb in (S, 2 * S + 5):
        h = _far_world(nat, B, T, mb)
        same(h.prob.solve_trajectory_ladder_nodes(*args, **kw), f"max_batch = {mb}")
    # device tensors in, device tensors out
    dev = torch.device("cuda:0")
    on = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)
    tens = w.prob.solve_trajectory_ladder_nodes(*[on(x) if isinstance(x, np.ndarray) else x for x in args], **{**kw, "weights": on(wts)})
    assert all(x is None or (isinstance(x, torch.Tensor) and x.device.type == "cuda") for x in tens)
    same(tens, "torch")
    h = _far_world(nat, B, T, S)
    same(h.prob.solve_trajectory_ladder_nodes(*[on(x) if isinstance(x, np.ndarray) else x for x in args], **{**kw, "weights": on(wts)}),
         "torch, one rung per chunk")
    # the drawn seeds passed back in
    same(w.prob.solve_trajectory_ladder_nodes(*args, seeds=whole.seeds, **kw), "passed seeds")
    # the rows of a sharded caller: target_index0
    part = w.prob.solve_trajectory_ladder_nodes(w.q[1:], w.tg[1:], w.pt, w.ct, w.dt, w.damping, target_index0=1, **kw)
    for f in whole._fields:
        if getattr(whole, f) is not None:
            _same(getattr(part, f), getattr(whole, f)[1:], f"target_index0: {f}")
    # a seed table: chunks and the generator drop out
    table = nat.NativeSeedTable(w.prob, 64, w.q[0], rng_seed=3)
    try:
        kt = {k: v for k, v in kw.items() if k != "rng_seed"}
        a = w.prob.solve_trajectory_ladder_nodes(*args, seed_table=table, rng_seed=1, **kt)
        b = _far_world(nat, B, T, 2 * S + 5).prob.solve_trajectory_ladder_nodes(*args, seed_table=table, rng_seed=99, **kt)
        for f in a._fields:
            if getattr(a, f) is not None:
                _same(getattr(b, f), getattr(a, f), f"seed table: {f}")
        plain = w.prob.solve_trajectory_ladder(*args, seed_table=table, return_all=True, **tl._kw(w, S, max_step_sq=1.0))
        _same(a.seeds, plain.seeds, "seed table: the plain ladder's starts")
    finally:
        table.close()


def test_max_instances_chunks_of_the_public_call(nat):
    import mink_amd as mink
    m, cfg, tasks, lims, tg = tm._far_ur5e(4)
    T, S, K = 3, 8, 3
    task = tasks[0]
    line = np.repeat(tg[:, None, :], T, axis=1)
    line[:, :, 4:] += np.linspace(0.0, 0.02, T)[None, :, None]
    kw = dict(n_seeds=S, max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, max_step=1.0, damping=1e-3, rng_seed=5, limits=lims,
              update=False, n_nodes=K, unwind_turns=True, return_all=True)
    whole = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: line}, **kw)
    _, cfg2, tasks2, lims2, _ = tm._far_ur5e(4)
    parts = mink.solve_ik_trajectory_ladder(cfg2, tasks2, 1.0, {tasks2[0]: line}, **{**kw, "limits": lims2, "max_instances": T * S + 1})
    assert list(cfg2._problems.values())[-1].max_batch == T * S                   # one instance per chunk
    for f in whole._fields:
        if getattr(whole, f) is not None:
            _same(getattr(parts, f), getattr(whole, f), f"max_instances: {f}")


# ------------------------------------------------------------------ 6. the flag on mkh_solve_multistart_set
_far = {}


def _far_sets(nat):
    """32 far UR5e targets from `home`, S = 16, K = 8: (model, q, plain multi-start, the set, the set with the flag)."""
    if not _far:
        from mink_amd.api_specs import configuration_limit_desc
        m = workloads.load_robot("ur5e")
        nm = nat.NativeModel(m, 0)
        B, S = 32, 16
        prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "attachment_site"),
                                                   "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 1.0}],
                                 configuration_limits=[configuration_limit_desc(m)], max_batch=B * S)
        q = np.tile(m.key_qpos[0], (B, 1))
        args = (q, tm._far_targets(m, B)[:, None, :], None, None, 1.0, 1e-3)
        kw = dict(n_seeds=S, max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, rng_seed=8, return_all=True)
        _far.update(m=m, q=q, prob=prob, nm=nm, args=args, kw=kw,
                    plain=prob.solve_multistart(*args, **kw),
                    raw=prob.solve_multistart_set(*args, n_solutions=8, min_distance=R, **kw),
                    unw=prob.solve_multistart_set(*args, n_solutions=8, min_distance=R, unwind_turns=True, **kw))
    return _far


def test_flag_on_the_set_is_unwind_then_select(nat):
    """CPU check of the fixture (32 far UR5e targets from `home`, S = 16, K = 8, rng_seed 8; the oracle's loops as above):
    207 of 512 loops converge; n_uncovered 17 raw, 0 unwound — strictly smaller —, n_distinct 188 raw, 142 unwound, no near
    tie.  The device gives the same figures."""
    f = _far_sets(nat)
    m, q, prob, plain, raw, unw = f["m"], f["q"], f["prob"], f["plain"], f["raw"], f["unw"]
    B, S = plain.q_all.shape[:2]
    # the loops know nothing of the flag; q_all returns the unwound rows, the starts are unchanged
    for g in ("converged_all", "iters_all", "status_all", "seeds"):
        _same(getattr(unw, g), getattr(plain, g), g)
    _same(raw.q_all, plain.q_all, "q_all without the flag")
    want_rows = uw.unwind(m, plain.q_all.reshape(-1, m.nq), q, S).reshape(B, S, m.nq)
    _same(unw.q_all, want_rows, "q_all with the flag: the rule")
    _same(unw.q_all, prob.unwind_turns(plain.q_all, q), "q_all with the flag: mkh_unwind_turns")
    assert (unw.q_all.view(np.int64) != plain.q_all.view(np.int64)).any()
    # the selection is select_distinct on the unwound rows, bitwise
    ok = ref.tracked(plain.converged_all, plain.status_all)
    sel = prob.select_distinct(unw.q_all, ok, q, None, n_solutions=8, min_distance=R)
    for g, h in (("q", "q"), ("seed_index", "seed_index"), ("distance", "distance"), ("multiplicity", "multiplicity"),
                 ("n_distinct", "n_distinct"), ("n_converged", "n_valid"), ("n_uncovered", "n_uncovered")):
        _same(getattr(unw, g), getattr(sel, h), f"flag: {g}")
    si = np.maximum(unw.seed_index, 0)
    _same(unw.iters, np.take_along_axis(plain.iters_all, si, axis=1), "flag: iters")
    _same(unw.status, np.take_along_axis(plain.status_all, si, axis=1), "flag: status")
    # unwinding frees slots: fewer converged seeds are left without a slot
    print(f"32 far targets, S = 16, K = 8: n_uncovered raw {int(raw.n_uncovered.sum())} -> unwound {int(unw.n_uncovered.sum())}; "
          f"n_distinct raw {int(raw.n_distinct.sum())} -> unwound {int(unw.n_distinct.sum())}; truncated targets raw "
          f"{int((raw.n_uncovered > 0).sum())} -> unwound {int((unw.n_uncovered > 0).sum())}")
    assert unw.n_uncovered.sum() <= raw.n_uncovered.sum()
    np.testing.assert_array_equal(unw.n_converged, raw.n_converged)


def test_every_other_entry_point_refuses_the_flag(nat):
    import mink_amd as mink
    f = _far_sets(nat)
    m, prob, L = f["m"], f["prob"], nat.lib()
    B, T, S = 2, 2, 2
    q = np.ascontiguousarray(f["q"][:B])
    tg = np.ascontiguousarray(np.repeat(f["args"][1][:B, None], T, axis=1))      # (B, T, 1, 7)
    f8, i4 = np.float64, np.int32
    buf = lambda *shape, dtype=f8: np.zeros(shape, dtype=dtype)
    U = nat.FLAG_UNWIND_TURNS
    keep = []                                                      # (what the structs point to)

    def filled(cls, **shapes):
        io = cls()
        for n, (shape, dt) in shapes.items():
            a = np.zeros(shape, dtype=dt); keep.append(a)
            setattr(io, n, a.ctypes.data)
        return io

    v, st, it, cv = buf(B, m.nv), buf(B, dtype=i4), buf(B, dtype=i4), buf(B, dtype=i4)
    qo = buf(B, m.nq)
    P = lambda a: a.ctypes.data
    one = tg[:, 0]
    head = (prob.handle, B, P(q), P(one), None, None, 1.0, 1e-3)
    ms_io = filled(nat.MkhMultistartIO, q_best=((B, m.nq), f8), v_best=((B, m.nv), f8), iters=((B,), i4), status=((B,), i4),
                   converged=((B,), i4), seed_index=((B,), i4), n_converged=((B,), i4))
    set_io = filled(nat.MkhSolutionSetIO, q_set=((B, 2, m.nq), f8), seed_index=((B, 2), i4), multiplicity=((B, 2), i4),
                    distance=((B, 2), f8), n_distinct=((B,), i4), n_uncovered=((B,), i4))
    tj_io = filled(nat.MkhTrajectoryIO, q_traj=((B, T, m.nq), f8), v_traj=((B, T, m.nv), f8), status=((B, T), i4),
                   iters=((B, T), i4), converged=((B, T), i4))
    lad = dict(q_traj=((B, T, m.nq), f8), v_traj=((B, T, m.nv), f8), status=((B, T), i4), iters=((B, T), i4), converged=((B, T), i4),
               node_index=((B, T), i4), n_tracked=((B,), i4), n_breaks=((B,), i4), path_length=((B,), f8), edge_break=((B, T), i4))
    lad_io = filled(nat.MkhTrajectoryLadderIO, **lad)
    lad_io.max_step_sq = float("inf")
    sel_io = filled(nat.MkhLadderIO, node_index=((B, T), i4), n_tracked=((B,), i4), n_breaks=((B,), i4), path_length=((B,), f8),
                    edge_break=((B, T), i4))
    ref_io = filled(nat.MkhLadderRefineIO, q_path_out=((B, T, m.nq), f8), tracked_out=((B, T), i4), repaired=((B, T), i4),
                    refined=((B,), i4), edge_break=((B, T), i4), n_tracked=((B,), i4), n_breaks=((B,), i4), path_length=((B,), f8))
    ref_io.max_step_sq = float("inf")
    nodes_q, trk = buf(B, T, S, m.nq), np.ones((B, T, S), dtype=i4)
    path_q, path_trk, pose = buf(B, T, m.nq), np.ones((B, T), dtype=i4), buf(1, 7)
    nm = f["nm"]
    loop = (40, 1e-4, 1e-4)
    calls = {
        "mkh_solve": lambda: L.mkh_solve(*head, P(v), P(st), U, None),
        "mkh_solve_steps": lambda: L.mkh_solve_steps(*head, 2, P(qo), P(v), P(st), U, None),
        "mkh_solve_until": lambda: L.mkh_solve_until(*head, *loop, P(qo), P(v), P(st), P(it), P(cv), U, None),
        "mkh_eval": lambda: L.mkh_eval(*head, P(v), P(st), None, U, None),
        "mkh_solve_multistart": lambda: L.mkh_solve_multistart(*head, *loop, S, 0, 0, ctypes.byref(ms_io), U, None),
        "mkh_select_distinct": lambda: L.mkh_select_distinct(prob.handle, B, S, P(nodes_q), None, P(q), None, 2, 0.1,
                                                             ctypes.byref(set_io), U, None),
        "mkh_solve_trajectory": lambda: L.mkh_solve_trajectory(prob.handle, B, T, P(q), P(tg), None, None, 1.0, 1e-3, *loop,
                                                               ctypes.byref(tj_io), U, None),
        "mkh_ladder_select": lambda: L.mkh_ladder_select(prob.handle, B, T, S, P(q), P(nodes_q), P(trk), None, float("inf"),
                                                         ctypes.byref(sel_io), U, None),
        "mkh_solve_trajectory_ladder": lambda: L.mkh_solve_trajectory_ladder(prob.handle, B, T, S, P(q), P(tg), None, None, 1.0, 1e-3,
                                                                             *loop, 0, 0, ctypes.byref(lad_io), U, None),
        "mkh_solve_trajectory_ladder_refined": lambda: L.mkh_solve_trajectory_ladder_refined(
            prob.handle, B, T, S, P(q), P(tg), None, None, 1.0, 1e-3, *loop, 0, 0, ctypes.byref(lad_io), ctypes.byref(ref_io), U, None),
        "mkh_ladder_refine": lambda: L.mkh_ladder_refine(prob.handle, B, T, P(q), P(path_q), P(path_trk),
                                                         P(tg), None, None, 1.0, 1e-3, *loop, ctypes.byref(ref_io), U, None),
        "mkh_integrate": lambda: L.mkh_integrate(nm.handle, B, P(q), P(v), 1.0, P(qo), U, None),
        "mkh_lie_eval": lambda: L.mkh_lie_eval(0, 0, 1, P(pose), None, P(v), U, None),
        "mkh_unwind_turns": lambda: L.mkh_unwind_turns(prob.handle, B, 1, P(q), P(q), P(qo), U, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.mkh_last_error()
        assert b"MKH_FLAG_UNWIND_TURNS" in msg or (name == "mkh_unwind_turns" and b"only MKH_FLAG_DEVICE_PTRS" in msg), (name, msg)
    # the two that honour it accept it (the public calls exercise them above); the Python layer offers it nowhere else
    with pytest.raises(TypeError):
        prob.solve_multistart(*f["args"], unwind_turns=True, **f["kw"])


# ------------------------------------------------------------------ 7. the public API
def test_public_api(nat):
    import mink_amd as mink
    B, T, S, K = 4, 3, 8, 3
    m, cfg, tasks, lims, tg = tm._far_ur5e(B)
    task = tasks[0]
    home = cfg.q_batch.copy()
    line = np.repeat(tg[:, None, :], T, axis=1)
    line[:, :, 4:] += np.linspace(0.0, 0.02, T)[None, :, None]
    kw = dict(n_seeds=S, max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, max_step=1.0, damping=1e-3, rng_seed=5, limits=lims)
    plain = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: line}, update=False, return_all=True, **kw)
    assert type(plain) is mink.LadderResult                         # n_nodes None: today's call and type
    res = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: line}, update=False, return_all=True, n_nodes=K, **kw)
    assert type(res) is mink.LadderNodesResult
    assert res.q.shape == (B, T, m.nq) and res.q_all.shape == (B, T, K, m.nq) and res.seeds.shape == (B, T, S, m.nq)
    assert res.node_seed_index.shape == (B, T, K) and res.n_distinct.shape == (B, T) and res.seed_index.shape == (B, T)
    assert res.converged.dtype == bool and res.edge_break.dtype == bool and res.converged_all.dtype == bool
    _same(res.seeds, plain.seeds, "the starts are the plain ladder's")
    np.testing.assert_array_equal(res.n_tracked, plain.n_tracked)
    np.testing.assert_array_equal(cfg.q_batch, home)
    fine = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: line}, update=False, n_nodes=K, unwind_turns=True, refine=True, **kw)
    assert type(fine) is mink.RefinedLadderNodesResult and fine.repaired.shape == (B, T) and fine.refined.dtype == bool
    assert fine.q_all is None and fine.node_distance.shape == (B, T, K)
    raw = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: line}, update=False, n_nodes=K, unwind_turns=True, **kw)
    for b in range(B):                                             # the pass never makes the searched path worse
        assert (T - fine.n_tracked[b], fine.n_breaks[b], fine.path_length[b]) <= (T - raw.n_tracked[b], raw.n_breaks[b], raw.path_length[b])
    # update=True leaves the configuration at the chosen q[:, -1]
    moved = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: line}, n_nodes=K, **kw)
    _same(moved.q, res.q, "update: q")
    np.testing.assert_array_equal(cfg.q_batch, res.q[:, -1])
    cfg.update(home)
    # an unbatched configuration: unbatched fields
    c1 = mink.Configuration(m, home[0])
    r1 = mink.solve_ik_trajectory_ladder(c1, [task], 1.0, {task: line[2]}, n_nodes=K, return_all=True, update=False, **kw)
    assert r1.q.shape == (T, m.nq) and r1.q_all.shape == (T, K, m.nq) and r1.node_seed_index.shape == (T, K)
    assert r1.n_distinct.shape == (T,) and np.ndim(r1.path_length) == 0
    # unwind_turns, the function; solve_ik_solutions and distinct_solutions with the flag
    rows = plain.q_all.reshape(B, T * S, m.nq)
    un = mink.unwind_turns(cfg, rows)
    _same(un, uw.unwind(m, rows.reshape(-1, m.nq), home, T * S).reshape(rows.shape), "unwind_turns")
    u1 = mink.unwind_turns(c1, rows[0])
    _same(u1, un[0], "unwind_turns, unbatched")
    task.set_target(mink.SE3(tg))
    skw = dict(n_seeds=S, n_solutions=4, max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, damping=1e-3, rng_seed=5, limits=lims,
               return_all=True)
    s_raw = mink.solve_ik_solutions(cfg, [task], 1.0, **skw)
    s_unw = mink.solve_ik_solutions(cfg, [task], 1.0, unwind_turns=True, **skw)
    _same(s_unw.q_all, mink.unwind_turns(cfg, s_raw.q_all), "solve_ik_solutions: q_all")
    d_unw = mink.distinct_solutions(cfg, s_raw.q_all, s_raw.converged_all & ((s_raw.status_all & ~1) == 0), n_solutions=4,
                                    unwind_turns=True)
    for g in ("q", "seed_index", "distance", "multiplicity", "n_distinct", "n_uncovered"):
        _same(getattr(d_unw, g), getattr(s_unw, g), f"distinct_solutions(unwind_turns): {g}")
    with pytest.raises(ValueError, match="pass n_nodes"):
        mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: line}, unwind_turns=True, **kw)
    with pytest.raises(ValueError, match="n_solutions"):
        mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: line}, n_nodes=65, **kw)
