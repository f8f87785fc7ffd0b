"""Ladder-graph trajectory IK on the device (mkh_ladder_select / mkh_solve_trajectory_ladder and the public calls on them): the
search is the stated recurrence — exactly, where the arithmetic is exact, and optimal to rounding on real rungs —, the rungs are
multi-start's bit for bit, the chosen rows are rows of the rungs, and the result depends on neither chunks nor, with a seed
table, the generator."""

from types import SimpleNamespace

import numpy as np
import pytest

import ladder_ref as ref
import test_gpu_trajectory as tj
import test_gpu_trajectory_multistart as tms
import trajectory_ref as tref
from mink_amd import workloads

pytestmark = pytest.mark.gpu
ALL = ("q_all", "v_all", "status_all", "iters_all", "converged_all")
CHOSEN = ("q", "v", "status", "iters", "converged")
SEARCH = ("node_index", "n_tracked", "n_breaks", "path_length", "edge_break")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _np(x):
    return None if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy())


_handles = {}


def _handle(nat, name, max_batch):
    """A bench problem of `name` for `max_batch` loop rows (the search itself only reads the model's joint table through it)."""
    if (name, max_batch) not in _handles:
        m = workloads.load_bench_robot(name)
        nm = nat.NativeModel(m, 0)
        prob, dt, damping = workloads.bench_config(name, m, nm, max_batch)
        _handles[name, max_batch] = SimpleNamespace(m=m, nm=nm, prob=prob, dt=dt, damping=damping)
    return _handles[name, max_batch]


# ------------------------------------------------------------------ 1. the search, exact
def _dyadic_ladder(m, B, T, S, seed):
    """q (B, nq), q_nodes (B, T, S, nq), tracked (B, T, S) with hinge / slide / position entries on multiples of 1/8 in [-2, 2]
    and every quaternion the identity: each difference, square, product with a weight of 1 and sum is exact in float64 however
    the compiler contracts it, and the rotation terms are exactly 0.  Instance 0 carries the special cases: duplicated nodes
    (ties), a rung nobody tracked, NaN rows; instance 1 duplicates a whole rung; the last instance's last rung is out of any
    gate's reach."""
    rng = np.random.default_rng(seed)
    quat = np.zeros(m.nq, dtype=bool)
    base = np.zeros(m.nq)
    for j in range(m.njnt):
        jt, qa = int(m.jnt_type[j]), int(m.jnt_qposadr[j])
        if jt in (ref.JNT_FREE, ref.JNT_BALL):
            qa += 3 if jt == ref.JNT_FREE else 0
            quat[qa:qa + 4] = True
            base[qa] = 1.0
    draw = lambda shape: np.where(quat, base, rng.integers(-16, 17, size=shape + (m.nq,)) / 8.0)
    q, nodes = draw((B,)), draw((B, T, S))
    trk = rng.uniform(size=(B, T, S)) < 0.75
    if S >= 2:
        nodes[0, :, S - 1] = nodes[0, :, 0]                     # the last node a copy of the first, in every rung
        trk[0, :, S - 1] = trk[0, :, 0]
        nodes[0, T // 2, S // 2] = np.nan                       # a NaN row
        if B > 1:
            nodes[1, T - 1, :] = nodes[1, T - 1, 0]             # a rung of S equal nodes
            trk[1, T - 1, :] = True
    if S >= 7:
        nodes[0, 0, 3, 0] = np.nan
    if T >= 2:
        trk[0, 1] = False                                       # a rung with no tracked node
        nodes[B - 1, T - 1, :, 0] += 64.0                       # a rung far from the one before it: any finite gate breaks there
    return q, nodes, trk


def _reference(m, q, nodes, trk, gate):
    B, T, S, nq = nodes.shape
    out = dict(node_index=np.zeros((B, T), np.int32), n_tracked=np.zeros(B, np.int32), n_breaks=np.zeros(B, np.int32),
               path_length=np.zeros(B), edge_break=np.zeros((B, T), np.int32), q=np.zeros((B, T, nq)))
    for b in range(B):
        start, edges = ref.costs(m, q[b], nodes[b])
        # (the plain double loop up to a few thousand edges; beyond that its vectorised twin — tests/test_ladder_cpu.py holds
        #  the two against each other and against enumeration)
        path, key, brk = (ref.search if S * S * T <= 4000 else ref.search_fast)(start, edges, ~trk[b], gate)
        out["node_index"][b], out["edge_break"][b] = path, brk
        out["n_tracked"][b], out["n_breaks"][b], out["path_length"][b] = T - key[0], key[1], key[2]
        out["q"][b] = nodes[b, np.arange(T), path]
    return out


def _gate(m):
    """A dyadic gate near the middle of the ordinary edge costs: a difference of two draws has variance 2.83 per coordinate."""
    return 2.75 * _plain(m)


def _plain(m):
    """How many coordinates of q are no quaternion entries."""
    n = m.nq
    for j in range(m.njnt):
        if int(m.jnt_type[j]) in (ref.JNT_FREE, ref.JNT_BALL):
            n -= 4
    return n


def _check_exact(nat, w, q, nodes, trk, what):
    import torch
    m = w.m
    dev = torch.device("cuda:0")
    on = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    gate = _gate(m)
    seen_break = False
    for g in (np.inf, gate):
        want = _reference(m, q, nodes, trk, g)
        host = w.prob.ladder_select(q, nodes, trk, g)
        for f in want:
            np.testing.assert_array_equal(getattr(host, f), want[f], err_msg=f"{what}, gate {g}: {f}")
        tens = w.prob.ladder_select(on(q), on(nodes), on(trk.astype(np.int32)), g)
        assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in tens)
        for f in want:
            np.testing.assert_array_equal(_np(getattr(tens, f)), getattr(host, f), err_msg=f"{what}, gate {g}, torch: {f}")
        assert (host.edge_break[:, 0] == 0).all() and (host.edge_break.sum(axis=1) == host.n_breaks).all()
        seen_break = seen_break or bool((host.n_breaks > 0).any())
        if g == np.inf:
            assert (host.n_breaks == 0).all()
        elif nodes.shape[1] >= 2:
            assert host.n_breaks[-1] >= 1 and host.edge_break[-1, -1] == 1        # the forced break
    return seen_break


@pytest.mark.parametrize("T", [1, 2, 5, 33])
@pytest.mark.parametrize("S", [1, 2, 7, 64, 65, 130])
def test_search_is_the_recurrence_exactly(nat, S, T):
    w = _handle(nat, "ur5e_c2", 64)
    B = 3
    q, nodes, trk = _dyadic_ladder(w.m, B, T, S, seed=1000 * S + T)
    seen_break = _check_exact(nat, w, q, nodes, trk, f"ur5e S={S} T={T}")
    if T >= 2:
        want = _reference(w.m, q, nodes, trk, np.inf)
        assert want["n_tracked"][0] <= T - 1                     # the rung nobody tracked is lost on every path
        if S >= 2:
            assert want["node_index"][0].max() < S - 1           # the copy at S − 1 is never returned: ties go to the lowest index
            assert (want["node_index"][1][-1] == 0)              # a rung of equal nodes: node 0
    assert seen_break == (T >= 2)


def test_search_on_a_rung_beyond_one_lds_tile(nat):
    """G1 (the free joint's position enters the cost, its quaternion is the identity everywhere), S = 130: destination tile, keys
    and the whole source rung do not fit 64 KB of LDS — the sources pass in two tiles (ladder_source_tile in ladder.hip)."""
    w = _handle(nat, "g1_c3", 64)
    m, S, T, B = w.m, 130, 3, 3
    fixed = m.nq * 64 * 8 + 2 * S * 12
    assert fixed + S * m.nq * 8 > 64 * 1024 > fixed + (S // 2) * m.nq * 8
    q, nodes, trk = _dyadic_ladder(m, B, T, S, seed=7)
    assert _check_exact(nat, w, q, nodes, trk, "g1 S=130")


# ------------------------------------------------------------------ 2. the search on real rungs
def _real(nat, name, B, T, S):
    if name == "ballslide":
        w = tj._ballslide(nat, B * T * S, T)
        w.q, w.tg = np.ascontiguousarray(w.q[:B]), np.ascontiguousarray(w.tg[:B])
        return w
    h = _handle(nat, name, B * T * S)
    wl = tms._workload(nat, name, (B, T, S))                     # (its q and targets; the handle here holds B·T·S rows)
    until, iters = wl.until, wl.iters
    return SimpleNamespace(m=h.m, nm=h.nm, prob=h.prob, dt=h.dt, damping=h.damping, q=wl.q, tg=wl.tg, pt=wl.pt, ct=wl.ct,
                           until=until, iters=iters)


def _kw(w, S, **extra):
    return dict(n_seeds=S, max_iters=w.iters, pos_threshold=w.until[0], ori_threshold=w.until[1], **extra)


def _middle_gate(d):
    """The middle of the widest gap between consecutive sorted finite costs in the central half of their distribution."""
    d = np.sort(d[np.isfinite(d)])
    lo, hi = len(d) // 4, (3 * len(d)) // 4
    k = lo + int(np.argmax(np.diff(d[lo:hi + 1])))
    return 0.5 * (d[k] + d[k + 1])


@pytest.mark.parametrize("name", ["ur5e_c2", "ballslide"])
def test_search_on_real_rungs_is_optimal(nat, name):
    """Discrete choices may differ from numpy's at rounding-level ties, so the check is OPTIMALITY, no case excluded: the
    device path loses and breaks as little as the reference optimum, its length — recomputed in numpy — is the reported one and
    the reference optimum's, each within 1e-12 relative (the bound tests/test_gpu_trajectory_multistart.py holds path_length to)."""
    B, T, S = 12, 4, 8
    w = _real(nat, name, B, T, S)
    m = w.m
    assert tref.quaternion_dofs(m).any() == (name == "ballslide")
    weights = np.random.default_rng(1).uniform(0.1, 10.0, size=m.nv)
    seen_lost = seen_break = False
    for wts in (None, weights):
        rungs = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, return_all=True, rng_seed=8, weights=wts,
                                               **_kw(w, S))
        trk = ref.tracked(rungs.converged_all, rungs.status_all)
        cost = [ref.costs(m, w.q[b], rungs.q_all[b], wts) for b in range(B)]
        d = np.concatenate([e[1:].ravel() for _, e in cost])
        gate = _middle_gate(d)
        near = np.abs(d[np.isfinite(d)] - gate) / gate
        print(f"{name}{', weights' if wts is not None else ''}: {int(trk.sum())} of {trk.size} nodes tracked, gate {gate:.6g} "
              f"(median cost {np.median(d[np.isfinite(d)]):.6g}), nearest edge at {near.min():.3e} relative")
        assert near.min() > 1e-9
        for g in (np.inf, gate):
            out = w.prob.ladder_select(w.q, rungs.q_all, trk, g, wts)
            full = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, return_all=True, rng_seed=8, weights=wts,
                                                  max_step_sq=g, **_kw(w, S))
            np.testing.assert_array_equal(full.q_all, rungs.q_all)
            for f in SEARCH:                                     # the call's search is the search alone on its own rungs
                np.testing.assert_array_equal(getattr(full, f), getattr(out, f), err_msg=f)
            np.testing.assert_array_equal(full.q, out.q)
            worst_self = worst_opt = 0.0
            for b in range(B):
                start, edges = cost[b]
                lost = ~trk[b]
                _, best, _ = ref.search(start, edges, lost, g)
                mine = ref.path_key(start, edges, lost, out.node_index[b], g)
                assert (T - out.n_tracked[b], out.n_breaks[b]) == (best[0], best[1]) == (mine[0], mine[1]), (b, best, mine)
                brk = [0] + [int(edges[t][out.node_index[b, t]][out.node_index[b, t - 1]] > g) for t in range(1, T)]
                assert out.edge_break[b].tolist() == brk
                tiny = np.finfo(float).tiny
                worst_self = max(worst_self, abs(mine[2] - out.path_length[b]) / max(abs(out.path_length[b]), tiny))
                worst_opt = max(worst_opt, abs(mine[2] - best[2]) / max(abs(best[2]), tiny))
                seen_lost, seen_break = seen_lost or best[0] > 0, seen_break or best[1] > 0
            print(f"  gate {g:.6g}: path_length worst relative |numpy - device| = {worst_self:.3e}, |device path - optimum| = {worst_opt:.3e}")
            assert worst_self <= 1e-12 and worst_opt <= 1e-12
    print(f"{name}: lost nodes on an optimal path: {seen_lost}; breaks on an optimal path: {seen_break}")
    if name == "ballslide":
        w.prob.close(); w.nm.close()


# ------------------------------------------------------------------ 3. the rungs are multi-start's
def test_rungs_are_multistarts_bitwise(nat):
    B, T, S = 6, 4, 4
    w = _real(nat, "ur5e_c2", B, T, S)
    m = w.m
    flat_q = np.repeat(w.q, T, axis=0)                           # target row b·T + t starts from q[b]
    flat_tg = np.ascontiguousarray(w.tg.reshape(B * T, w.prob.n_frame, 7))
    for rng_seed, t0 in ((0, 0), (2 ** 40 + 12345, 1000003)):
        out = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, rng_seed=rng_seed, target_index0=t0,
                                             return_all=True, qvel_dt=0.05, **_kw(w, S))
        k = w.prob.last_kernel()
        ms = w.prob.solve_multistart(flat_q, flat_tg, w.pt, None, w.dt, w.damping, n_seeds=S, max_iters=w.iters,
                                     pos_threshold=w.until[0], ori_threshold=w.until[1], rng_seed=rng_seed, target_index0=t0 * T,
                                     return_all=True)
        assert w.prob.last_kernel() == k
        for f, g in (("q_all", "q_all"), ("converged_all", "converged_all"), ("status_all", "status_all"), ("iters_all", "iters_all"),
                     ("seeds", "seeds")):
            np.testing.assert_array_equal(getattr(out, f).reshape(getattr(ms, g).shape), getattr(ms, g), err_msg=f)
        np.testing.assert_array_equal(out.seeds[:, :, 0], np.broadcast_to(w.q[:, None], (B, T, m.nq)))     # seed 0 of every rung: q[b]
        rows, cols = np.arange(B)[:, None], np.arange(T)[None, :]
        for f, g in zip(ALL, CHOSEN):
            np.testing.assert_array_equal(getattr(out, g), getattr(out, f)[rows, cols, out.node_index], err_msg=g)
        trk = ref.tracked(out.converged_all, out.status_all)
        np.testing.assert_array_equal(out.n_tracked, trk.any(axis=2).sum(axis=1))
        assert (out.n_breaks == 0).all() and (out.edge_break == 0).all()
        print(f"rng_seed {rng_seed}: kernel {k}, {int(trk.sum())} of {trk.size} nodes tracked, n_tracked {out.n_tracked.tolist()}, "
              f"nodes {out.node_index.tolist()}")
    # the caller's own starts, row 0 of every rung replaced by q
    own = np.random.default_rng(3).uniform(-1.0, 1.0, size=(B, T, S, m.nq))
    mine = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, seeds=own, rng_seed=77, return_all=True, **_kw(w, S))
    want = own.copy(); want[:, :, 0] = w.q[:, None]
    np.testing.assert_array_equal(mine.seeds, want)
    ms = w.prob.solve_multistart(flat_q, flat_tg, w.pt, None, w.dt, w.damping, n_seeds=S, max_iters=w.iters, pos_threshold=w.until[0],
                                 ori_threshold=w.until[1], seeds=own.reshape(B * T, S, m.nq), return_all=True)
    np.testing.assert_array_equal(mine.q_all.reshape(B * T, S, m.nq), ms.q_all)
    # one node per rung: node 0 everywhere, each waypoint mkh_solve_until's loop from q[b]
    one = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, return_all=True, **_kw(w, 1))
    k1 = w.prob.last_kernel()
    loop = w.prob.solve(flat_q, flat_tg, w.pt, None, w.dt, w.damping, n_steps=w.iters, until=w.until)
    assert (one.node_index == 0).all() and w.prob.last_kernel() == k1
    for f, x in zip(CHOSEN, loop):
        np.testing.assert_array_equal(getattr(one, f).reshape(x.shape), x, err_msg=f"S = 1: {f}")
    np.testing.assert_array_equal(one.q_all[:, :, 0], one.q)
    # a handle too small for the whole ladder runs it in chunks of whole rungs: the same rungs when the same kernel serves them
    small = _handle(nat, "ur5e_c2", 5 * S)
    part = small.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, rng_seed=0, return_all=True, qvel_dt=0.05,
                                              **_kw(w, S))
    whole = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, rng_seed=0, return_all=True, qvel_dt=0.05, **_kw(w, S))
    np.testing.assert_array_equal(part.seeds, whole.seeds)
    assert small.prob.last_kernel() == w.prob.last_kernel()
    for f in whole._fields:
        np.testing.assert_array_equal(getattr(part, f), getattr(whole, f), err_msg=f"chunks of 5 rungs: {f}")
    with pytest.raises(nat.MinkHipError, match="exceeds max_batch"):
        small.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, **_kw(w, 5 * S + 1))


# ------------------------------------------------------------------ 4. invariants, through the public call
_KW = dict(n_seeds=tms._S5, max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, damping=1e-3, rng_seed=5)
_far = {}


def _far_ladder():
    if "whole" not in _far:
        import mink_amd as mink
        m, cfg, task, lims, tg = tms._far_setup()
        _far["whole"] = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, return_all=True,
                                                        qvel_dt=0.05, **_KW)
        _far["kernel"] = list(cfg._problems.values())[-1].last_kernel()
        for x in _far["whole"]:
            x.setflags(write=False)
    return _far["whole"]


def test_invariants_of_the_public_call(nat):
    import mink_amd as mink
    whole = _far_ladder()
    B, T, S = tms._B5, tms._T5, tms._S5
    m, cfg, task, lims, tg = tms._far_setup()
    home = cfg.q_batch.copy()
    assert isinstance(whole, mink.LadderResult)
    assert whole.q.shape == (B, T, m.nq) and whole.v.shape == (B, T, m.nv) and whole.qvel.shape == (B, T, m.nv)
    assert whole.q_all.shape == (B, T, S, m.nq) and whole.seeds.shape == (B, T, S, m.nq) and whole.node_index.shape == (B, T)
    assert whole.converged.dtype == bool and whole.converged_all.dtype == bool and whole.edge_break.dtype == bool
    # no gate: no breaks; a rung with a tracked node is never lost
    trk = ref.tracked(whole.converged_all, whole.status_all)
    assert (whole.n_breaks == 0).all() and not whole.edge_break.any()
    np.testing.assert_array_equal(whole.n_tracked, trk.any(axis=2).sum(axis=1))
    rows, cols = np.arange(B)[:, None], np.arange(T)[None, :]
    np.testing.assert_array_equal(whole.q, whole.q_all[rows, cols, whole.node_index])
    np.testing.assert_array_equal(whole.seeds[:, :, 0], np.broadcast_to(home[:, None], (B, T, m.nq)))
    print(f"far UR5e paths: ladder tracks {whole.n_tracked.tolist()} of {T} waypoints, nodes {whole.node_index.tolist()}")
    # the search alone, on these rungs: the same path
    alone = mink.ladder_path(cfg, whole.q_all, trk)
    assert isinstance(alone, mink.LadderPath)
    for f in ("node_index", "q", "n_tracked", "n_breaks", "path_length", "edge_break"):
        np.testing.assert_array_equal(getattr(alone, f), getattr(whole, f), err_msg=f)
    # a gate: the breaks are those of the chosen path's own steps
    gated = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, max_step=1.0, **_KW)
    step_sq = ((gated.q[:, 1:] - gated.q[:, :-1]) ** 2).sum(axis=2)
    # (steps at a distance from the gate: the comparison is the device's own rounding of the same sum)
    clear = np.abs(step_sq - 1.0) > 1e-9
    assert (gated.edge_break[:, 1:] == (step_sq > 1.0))[clear].all() and not gated.edge_break[:, 0].any()
    np.testing.assert_array_equal(gated.n_breaks, gated.edge_break.sum(axis=1))
    np.testing.assert_array_equal(cfg.q_batch, home)                       # update=False leaves the configuration alone
    assert gated.qvel is None and gated.q_all is None and gated.seeds is None

    def same(other, what):
        for f in whole._fields:
            np.testing.assert_array_equal(getattr(other, f), getattr(whole, f), err_msg=f"{what}: {f}")

    # chunks of 3 instances (15 rungs of 8 loops each)
    _, cfg_c, task_c, lims_c, _ = tms._far_setup()
    chunked = mink.solve_ik_trajectory_ladder(cfg_c, [task_c], 1.0, {task_c: tg}, limits=lims_c, update=False, return_all=True,
                                              qvel_dt=0.05, max_instances=3 * T * S + 7, **_KW)
    prob_c = list(cfg_c._problems.values())[-1]
    assert prob_c.max_batch == 3 * T * S and prob_c.last_kernel() == _far["kernel"]
    same(chunked, "max_instances")
    # two shards (the same device listed twice): 8 instances each, told their offset
    _, cfg_s, task_s, lims_s, _ = tms._far_setup(device=[0, 0])
    sharded = mink.solve_ik_trajectory_ladder(cfg_s, [task_s], 1.0, {task_s: tg}, limits=lims_s, update=False, return_all=True,
                                              qvel_dt=0.05, **_KW)
    shards = list(cfg_s._problems.values())[-1].shards
    assert len(shards) == 2 and all(p.max_batch == 8 * T * S and p.last_kernel() == _far["kernel"] for p in shards)
    same(sharded, "device=[0, 0]")
    # update=True: the configuration is left at the chosen q[:, -1]
    moved = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, **_KW)
    np.testing.assert_array_equal(moved.q, whole.q)
    np.testing.assert_array_equal(cfg.q_batch, whole.q[:, -1])
    cfg.update(home)
    # an unbatched configuration: unbatched fields
    c1 = mink.Configuration(m, home[0])
    r1 = mink.solve_ik_trajectory_ladder(c1, [task], 1.0, {task: tg[3]}, limits=lims, return_all=True, seeds=whole.seeds[3], **_KW)
    assert r1.q.shape == (T, m.nq) and r1.node_index.shape == (T,) and r1.q_all.shape == (T, S, m.nq) and np.ndim(r1.path_length) == 0
    np.testing.assert_array_equal(r1.q, whole.q[3])


def test_seed_table_makes_the_result_independent_of_the_generator(nat):
    import mink_amd as mink
    m, cfg, task, lims, tg = tms._far_setup()
    B, T, S = tms._B5, tms._T5, tms._S5
    table = mink.SeedTable(mink.Configuration(m, cfg.q_batch[0]), [task], 512, limits=lims)
    try:
        kw = {k: v for k, v in _KW.items() if k != "rng_seed"}
        a = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, return_all=True, seed_table=table,
                                            rng_seed=1, **kw)
        b = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, return_all=True, seed_table=table,
                                            rng_seed=2, **kw)
        for f in a._fields:
            if getattr(a, f) is not None:
                np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f)
        # every rung's rows 1 … S − 1 are the entries nearest to that waypoint's OWN target
        idx, _ = table.query(tg.reshape(B * T, 1, 7), S - 1)[:2]
        np.testing.assert_array_equal(a.seeds[:, :, 1:], table.q[np.asarray(idx)].reshape(B, T, S - 1, m.nq))
        plain = _far_ladder()
        print(f"far UR5e paths, complete: drawn seeds {int((plain.n_tracked == T).sum())} of {B}, seed table {int((a.n_tracked == T).sum())}")
    finally:
        table.close()


# ------------------------------------------------------------------ 5. qvel
@pytest.mark.parametrize("name", ["ur5e_c2", "ballslide"])
def test_qvel_is_the_stated_rule_on_the_returned_path(nat, name):
    B, T, S = 8, 4, 4
    w = _real(nat, name, B, T, S)
    wdt = 0.04
    out = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, qvel_dt=wdt, rng_seed=3, **_kw(w, S))
    want = tref.qvel(w.m, w.q, out.q, wdt)
    quat = tref.quaternion_dofs(w.m)
    np.testing.assert_array_equal(out.qvel[..., ~quat], want[..., ~quat])
    if quat.any():
        dev = np.abs(out.qvel[..., quat] - want[..., quat]) / np.maximum(1.0, np.abs(want[..., quat]))
        assert dev.max() <= 1e-9, dev.max()
    if name == "ballslide":
        w.prob.close(); w.nm.close()
