"""Ladder refinement on the device (mkh_ladder_refine / mkh_solve_trajectory_ladder_refined and the public calls on them): the
pass is the stated rule bit for bit — held against its restatement (tests/ladder_refine_ref.py) with the solve kernels themselves
as the restatement's loop —, it heals designed breaks and lost nodes, it never returns a worse path than it was given, the
composed call is the ladder followed by the pass, and the result depends on neither chunks nor the kind of array passed in."""

import ctypes
import logging
from types import SimpleNamespace

import numpy as np
import pytest

import ladder_ref as ref
import ladder_refine_ref as rref
import oracle_configs as oc
import test_gpu_ladder as tl
import test_gpu_trajectory_multistart as tms
import trajectory_ref as tref
from oracle import ik as oik

pytestmark = pytest.mark.gpu
GATE = 1.0                               # (1 rad)^2
NODE = ("q", "v", "status", "iters", "converged")
PATH = ("q", "tracked", "repaired", "refined", "edge_break", "n_tracked", "n_breaks")
_np = tl._np


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _loop(w, iters, until):
    """The restatement's loop: mkh_solve_until on the device through the same handle, on all B rows of the start array."""
    def loop(t, start):
        B = len(start)
        return w.prob.solve(start, np.ascontiguousarray(w.tg[:, t]), tref.waypoint_target(w.pt, t, w.prob.n_posture, w.m.nq, B),
                            tref.waypoint_target(w.ct, t, w.prob.n_com, 3, B), w.dt, w.damping, n_steps=iters, until=until)
    return loop


def _against_restatement(w, q, path, trk, gate, iters, until, rows, what):
    """ladder_refine against the restatement: everything array_equal, path_length within (nv + T)·2^-52 relative — the bound for
    a sum of non-negative terms under reordering or contraction.  The conditions under which discrete choices are rounding-proof
    are ASSERTED on every instance: no judged edge cost within 1e-9 relative of the gate; where lost and breaks tie and something
    was repaired, the two lengths differ by more than 1e-9 relative."""
    B, T, _ = path.shape
    judged = []
    want = rref.refine(w.m, _loop(w, iters, until), q, path, trk, gate, judged=judged, **rows)
    k_ref = w.prob.last_kernel()
    got = w.prob.ladder_refine(q, path, trk, w.tg, w.pt, w.ct, w.dt, w.damping, max_iters=iters, pos_threshold=until[0],
                               ori_threshold=until[1], max_step_sq=gate, **rows)
    assert w.prob.last_kernel() == k_ref                          # the same kernel family served both
    c = np.array([x for _, x in judged if np.isfinite(x)])
    near = np.abs(c - gate) / gate if (np.isfinite(gate) and c.size) else np.array([np.inf])
    gaps = []
    for b in range(B):
        kp, kr = want["key_in"][b], want["key_work"][b]
        if kp[:2] == kr[:2] and want["work_repaired"][b].any():
            gaps.append(abs(kp[2] - kr[2]) / max(abs(kp[2]), abs(kr[2])))
    print(f"{what}: kernel {k_ref}; {len(judged)} edges judged, nearest to the gate {near.min():.3e} relative; "
          f"{int((want['work_repaired'] != 0).sum())} repairs accepted on {int(want['work_repaired'].any(axis=1).sum())} of {B} paths, "
          f"{int(want['refined'].sum())} returned; keys tied in lost and breaks with repairs: {len(gaps)}"
          + (f", nearest lengths {min(gaps):.3e} relative" if gaps else ""))
    assert near.min() > 1e-9
    assert all(g > 1e-9 for g in gaps)
    for f in PATH + (NODE[1:] if rows else ()):                   # (the loops' rows come back only into arrays that went in)
        np.testing.assert_array_equal(getattr(got, f), want[f], err_msg=f"{what}: {f}")
    rel = np.abs(got.path_length - want["path_length"]) / np.maximum(np.abs(want["path_length"]), np.finfo(float).tiny)
    print(f"  path_length: worst relative |device - numpy| = {rel.max():.3e}")
    assert rel.max() <= (w.m.nv + T) * 2.0 ** -52
    return got, want


# ------------------------------------------------------------------ 1. bitwise against the restatement, real ladder paths
@pytest.mark.parametrize("name,B,T,low,rng_seed", [("ur5e_c2", 5, 6, 4, 1), ("ur5e_c2", 70, 3, 4, 2), ("ballslide", 4, 5, 2, 3),
                                                   ("g1_c3", 3, 4, 4, 4)])
def test_pass_is_the_restatement_bitwise(nat, name, B, T, low, rng_seed):
    S = 4
    w = tl._real(nat, name, B, T, S)
    # the rungs with `low` iterations: some nodes are lost; the pass with the workload's own loop length
    lad = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, n_seeds=S, max_iters=low, pos_threshold=w.until[0],
                                         ori_threshold=w.until[1], max_step_sq=GATE, rng_seed=rng_seed)
    trk = ref.tracked(lad.converged, lad.status)
    print(f"{name} B={B} T={T}: the ladder's paths track {lad.n_tracked.tolist()} of {T}, breaks {lad.n_breaks.tolist()}")
    rows = dict(v=lad.v, status=lad.status, iters=lad.iters, converged=lad.converged)
    got, want = _against_restatement(w, w.q, lad.q, trk, GATE, w.iters, w.until, rows, f"{name} B={B} T={T}")
    # the guard's view of the input path is the search's
    keep = got.refined == 0
    np.testing.assert_array_equal(got.n_tracked[keep], lad.n_tracked[keep])
    np.testing.assert_array_equal(got.n_breaks[keep], lad.n_breaks[keep])
    np.testing.assert_array_equal(got.path_length[keep], lad.path_length[keep])
    np.testing.assert_array_equal(got.edge_break[keep], lad.edge_break[keep])
    # no gate: only lost nodes are repaired
    free, _ = _against_restatement(w, w.q, lad.q, trk, np.inf, w.iters, w.until, rows, f"{name} B={B} T={T}, no gate")
    assert (free.n_breaks == 0).all() and (free.repaired[trk] == 0).all()
    if name == "ballslide":
        w.prob.close(); w.nm.close()


# ------------------------------------------------------------------ 2. designed paths on UR5e
_T2, _B2 = 6, 3
_KW2 = dict(max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, damping=1e-3, max_step=1.0)
_designed = {}


def _line():
    """Joint-space lines qA (B, T, 6) far from `home`, steps of at most 0.08 rad per joint — well under the gate —, their site
    poses as targets, a batched configuration at `home`, and a view of its handle for the restatement."""
    if not _designed:
        import mink_amd as mink
        m = tms._far_paths()[0]
        rng = np.random.default_rng(11)
        home = m.key_qpos[m.name2id("key", "home")]
        q0 = home + np.array([2.4, 1.0, -2.6, 1.2, 2.2, 1.5]) + rng.uniform(-0.2, 0.2, size=(_B2, 6))
        qA = q0[:, None, :] + np.arange(_T2)[None, :, None] * rng.uniform(0.02, 0.08, size=(_B2, 1, 6))
        assert (np.abs(qA[:, :, 2]) < 3.0).all() and (np.abs(qA - home).max(axis=2) > 2.0).all()      # inside the elbow's range, far from home
        tg = mink.Configuration(m, qA.reshape(-1, 6)).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz
        _designed.update(m=m, qA=qA, home=home, tg=np.ascontiguousarray(tg.reshape(_B2, _T2, 7)))
    d = _designed
    import mink_amd as mink
    cfg = mink.Configuration(d["m"], np.tile(d["home"], (_B2, 1)))
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    return d["m"], cfg, task, [mink.ConfigurationLimit(d["m"])], d["tg"], d["qA"]


def _solutions(m, q, tg, pth=1e-4, oth=1e-4):
    """Every node of q (B, T, nq) meets the thresholds at its target by the CPU oracle's kinematics."""
    mo = oc.model("ur5e")
    sid = mo.name2id("site", "attachment_site")
    worst_p = worst_o = 0.0
    for b in range(q.shape[0]):
        for t in range(q.shape[1]):
            e, _ = oik.task_error_jacobian(oik.Configuration(mo, q[b, t]), oik.FrameTaskSpec(sid, "site", np.ones(6), tg[b, t], lm_damping=1.0))
            worst_p, worst_o = max(worst_p, float(np.linalg.norm(e[:3]))), max(worst_o, float(np.linalg.norm(e[3:])))
    print(f"  worst error norms of the returned nodes by the oracle: position {worst_p:.3e}, orientation {worst_o:.3e}")
    assert worst_p <= pth + 1e-9 and worst_o <= oth + 1e-9


def _steps_sq(q):
    return ((q[:, 1:] - q[:, :-1]) ** 2).sum(axis=2)


@pytest.mark.parametrize("case", ["far", "lost", "head"])
def test_designed_paths_are_healed(nat, case):
    import mink_amd as mink
    m, cfg, task, lims, tg, qA = _line()
    T, B = _T2, _B2
    path, trk = qA.copy(), np.ones((B, T), dtype=bool)
    if case == "far":                                            # one node on another branch, flagged tracked
        path[:, 3, [0, 2, 4]] += 2.0
        touched = [3]
    elif case == "lost":                                         # one node flagged lost
        trk[:, 3] = False
        touched = [3]
    else:                                                        # the head of the path never left `home`
        path[:, :3] = cfg.q_batch[:, None, :]
        trk[:, :3] = False
        touched = [0, 1, 2]
    out = mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, **_KW2)
    assert isinstance(out, mink.RefinedPath) and out.q.shape == (B, T, m.nq) and out.refined.dtype == bool
    print(f"{case}: repaired {out.repaired.tolist()}, iterations of the repairs {out.iters[out.repaired != 0].tolist()}")
    assert out.refined.all() and (out.n_tracked == T).all() and (out.n_breaks == 0).all() and out.tracked.all()
    assert not out.edge_break.any()
    if case != "head":
        assert ((out.repaired != 0) == np.isin(np.arange(T), touched)[None, :]).all()
    else:
        assert (out.repaired[:, :3] != 0).all()
    _solutions(m, out.q, tg)
    assert _steps_sq(out.q).max() <= GATE                        # no step beyond the gate
    assert (out.converged[out.repaired != 0]).all() and not out.converged[out.repaired == 0].any()      # kept rows: zeros
    # ... and the same call on the native handle is the restatement, bit for bit
    prob = list(cfg._problems.values())[-1]
    w = SimpleNamespace(m=m, prob=prob, tg=np.ascontiguousarray(tg[:, :, None, :]), pt=None, ct=None, dt=1.0, damping=1e-3)
    got, _ = _against_restatement(w, cfg.q_batch, path, trk, GATE, 40, (1e-4, 1e-4), {}, f"designed, {case}")
    np.testing.assert_array_equal(got.q, out.q)
    np.testing.assert_array_equal(got.repaired, out.repaired)


def test_untouched_line_comes_back_bit_for_bit(nat):
    import mink_amd as mink
    m, cfg, task, lims, tg, qA = _line()
    home = cfg.q_batch.copy()
    out = mink.refine_path(cfg, [task], 1.0, {task: tg}, qA, limits=lims, update=False, **_KW2)
    assert not out.refined.any() and not out.repaired.any() and out.tracked.all()
    np.testing.assert_array_equal(out.q, qA)
    assert (out.n_tracked == _T2).all() and (out.n_breaks == 0).all() and not out.edge_break.any()
    np.testing.assert_array_equal(cfg.q_batch, home)
    # its length is the rule's, start edge from `home` included
    want = np.array([rref.key_of(m, home[b], qA[b], np.ones(_T2), GATE)[0][2] for b in range(_B2)])
    assert (np.abs(out.path_length - want) <= (m.nv + _T2) * 2.0 ** -52 * want).all()


# ------------------------------------------------------------------ 3. never worse
def test_refined_ladder_is_never_worse_than_the_search(nat):
    B, T, S = 12, 4, 8
    w = tl._real(nat, "ur5e_c2", B, T, S)
    seen = 0
    for low, gate in ((3, GATE), (5, 0.05), (w.iters, np.inf)):
        kw = dict(n_seeds=S, max_iters=low, pos_threshold=w.until[0], ori_threshold=w.until[1], max_step_sq=gate, rng_seed=8, qvel_dt=0.05)
        plain = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, **kw)
        fine = w.prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, refine=True, **kw)
        assert plain.refined is None and plain.repaired is None and plain.tracked is None
        for b in range(B):
            before = (T - plain.n_tracked[b], plain.n_breaks[b], plain.path_length[b])
            after = (T - fine.n_tracked[b], fine.n_breaks[b], fine.path_length[b])
            assert after <= before, (b, before, after)
            assert bool(fine.refined[b]) == (after < before)
        keep = fine.refined == 0
        for f in plain._fields[:11]:
            np.testing.assert_array_equal(getattr(fine, f)[keep], getattr(plain, f)[keep], err_msg=f"max_iters {low}: {f}")
        np.testing.assert_array_equal(fine.node_index, plain.node_index)           # the search's choice, repaired or not
        assert not fine.repaired[keep].any()
        np.testing.assert_array_equal(fine.tracked[keep], ref.tracked(plain.converged, plain.status)[keep])
        np.testing.assert_array_equal(fine.n_tracked, fine.tracked.sum(axis=1))
        np.testing.assert_array_equal(fine.n_breaks, fine.edge_break.sum(axis=1))
        seen += int(fine.refined.sum())
        print(f"max_iters {low}, gate {gate}: search lost {(T - plain.n_tracked).tolist()} breaks {plain.n_breaks.tolist()}; "
              f"refined {fine.refined.tolist()}: lost {(T - fine.n_tracked).tolist()} breaks {fine.n_breaks.tolist()}")
    assert seen > 0                                              # (the fixture's condition: something was there to refine)


# ------------------------------------------------------------------ 4. composition
def test_composed_call_is_the_ladder_followed_by_the_pass(nat):
    import torch
    B, T, S = 12, 4, 8
    w = tl._real(nat, "ur5e_c2", B, T, S)
    m, prob = w.m, w.prob
    kw = dict(n_seeds=S, max_iters=5, pos_threshold=w.until[0], ori_threshold=w.until[1], max_step_sq=0.05, rng_seed=8, qvel_dt=0.05,
              weights=np.random.default_rng(2).uniform(0.5, 2.0, size=m.nv))
    plain = prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, **kw)
    # (a) refine = NULL: the existing entry point, called as C callers call it, gives the same bits
    f8, i4 = np.float64, np.int32
    out = {"q_traj": np.empty((B, T, m.nq), f8), "v_traj": np.empty((B, T, m.nv), f8), "status": np.empty((B, T), i4),
           "iters": np.empty((B, T), i4), "converged": np.empty((B, T), i4), "node_index": np.empty((B, T), i4),
           "n_tracked": np.empty(B, i4), "n_breaks": np.empty(B, i4), "path_length": np.empty(B, f8),
           "edge_break": np.empty((B, T), i4), "qvel": np.empty((B, T, m.nv), f8)}
    io = nat.MkhTrajectoryLadderIO()
    for name, x in out.items():
        setattr(io, name, x.ctypes.data)
    io.weights, io.max_step_sq, io.waypoint_dt = kw["weights"].ctypes.data, 0.05, 0.05
    q, tg, pt = np.ascontiguousarray(w.q), np.ascontiguousarray(w.tg), np.ascontiguousarray(w.pt)
    assert pt.shape == (1, m.nq) and prob.n_posture <= 1 and w.ct is None        # (a held posture target: no flag)
    rc = nat.lib().mkh_solve_trajectory_ladder(prob.handle, B, T, S, q.ctypes.data, tg.ctypes.data, pt.ctypes.data, None, float(w.dt),
                                               float(w.damping), 5, w.until[0], w.until[1], 8, 0, ctypes.byref(io), 0, None)
    assert rc == 0, nat.lib().mkh_last_error()
    for name, f in zip(out, plain._fields[:11]):
        np.testing.assert_array_equal(out[name], getattr(plain, f), err_msg=f"refine = NULL: {f}")
    # (b) with refine: the ladder, then the pass on its outputs
    fine = prob.solve_trajectory_ladder(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, refine=True, **kw)
    trk = ref.tracked(plain.converged, plain.status)
    rkw = dict(max_iters=5, pos_threshold=w.until[0], ori_threshold=w.until[1], max_step_sq=0.05, weights=kw["weights"])
    two = prob.ladder_refine(w.q, plain.q, trk, w.tg, w.pt, w.ct, w.dt, w.damping, v=plain.v, status=plain.status, iters=plain.iters,
                             converged=plain.converged, **rkw)
    pairs = (("q", "q"), ("v", "v"), ("status", "status"), ("iters", "iters"), ("converged", "converged"), ("tracked", "tracked"),
             ("repaired", "repaired"), ("refined", "refined"), ("edge_break", "edge_break"), ("n_tracked", "n_tracked"),
             ("n_breaks", "n_breaks"), ("path_length", "path_length"))
    for f, g in pairs:
        np.testing.assert_array_equal(getattr(fine, f), getattr(two, g), err_msg=f"host arrays: {f}")
    assert fine.refined.any() and not fine.refined.all()          # (both sides of the guard are in the comparison)
    print(f"composition: refined {fine.refined.tolist()}, repaired {fine.repaired.tolist()}")
    # qvel follows the returned path
    want = tref.qvel(m, w.q, fine.q, 0.05)
    np.testing.assert_array_equal(fine.qvel, want)
    assert not np.array_equal(fine.qvel, plain.qvel)
    # (c) device tensors: the same bits, nothing on the host
    dev = torch.device("cuda:0")
    on = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)
    tkw = {**kw, "weights": on(kw["weights"])}
    fine_t = prob.solve_trajectory_ladder(on(w.q), on(w.tg), on(w.pt), on(w.ct), w.dt, w.damping, refine=True, **tkw)
    assert all(x is None or (isinstance(x, torch.Tensor) and x.device.type == "cuda") for x in fine_t)
    for f in fine._fields:
        if getattr(fine, f) is not None:
            np.testing.assert_array_equal(_np(getattr(fine_t, f)), getattr(fine, f), err_msg=f"torch, composed: {f}")
    plain_t = prob.solve_trajectory_ladder(on(w.q), on(w.tg), on(w.pt), on(w.ct), w.dt, w.damping, **tkw)
    two_t = prob.ladder_refine(on(w.q), plain_t.q, on(trk.astype(np.int32)), on(w.tg), on(w.pt), on(w.ct), w.dt, w.damping, v=plain_t.v,
                               status=plain_t.status, iters=plain_t.iters, converged=plain_t.converged,
                               **{**rkw, "weights": tkw["weights"]})
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in two_t)
    for f in two._fields:
        np.testing.assert_array_equal(_np(getattr(two_t, f)), getattr(two, f), err_msg=f"torch, the pass alone: {f}")
    np.testing.assert_array_equal(_np(plain_t.v), plain.v)        # (the caller's rows were copied, not written)


# ------------------------------------------------------------------ 5. plumbing, through the public calls
_KW5 = dict(n_seeds=tms._S5, max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, damping=1e-3, rng_seed=5, max_step=1.0)
_far = {}


def _far_refined():
    if "whole" not in _far:
        import mink_amd as mink
        m, cfg, task, lims, tg = tms._far_setup()
        _far["whole"] = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, qvel_dt=0.05,
                                                        refine=True, **_KW5)
        _far["kernel"] = list(cfg._problems.values())[-1].last_kernel()
    return _far["whole"]


def test_plumbing_of_the_refined_ladder(nat):
    import mink_amd as mink
    whole = _far_refined()
    B, T, S = tms._B5, tms._T5, tms._S5
    m, cfg, task, lims, tg = tms._far_setup()
    home = cfg.q_batch.copy()
    assert isinstance(whole, mink.RefinedLadderResult) and whole._fields[:17] == mink.LadderResult._fields
    assert whole.repaired.shape == (B, T) and whole.refined.shape == (B,) and whole.refined.dtype == bool
    plain = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, qvel_dt=0.05, **_KW5)
    assert isinstance(plain, mink.LadderResult) and not isinstance(plain, mink.RefinedLadderResult)
    np.testing.assert_array_equal(cfg.q_batch, home)
    print(f"far UR5e paths: search lost {(T - plain.n_tracked).tolist()} breaks {plain.n_breaks.tolist()}; "
          f"refined {whole.refined.astype(int).tolist()}: lost {(T - whole.n_tracked).tolist()} breaks {whole.n_breaks.tolist()}")
    for b in range(B):
        assert (T - whole.n_tracked[b], whole.n_breaks[b], whole.path_length[b]) <= (T - plain.n_tracked[b], plain.n_breaks[b], plain.path_length[b])

    def same(other, what):
        for f in whole._fields:
            if getattr(whole, f) is not None:
                np.testing.assert_array_equal(getattr(other, f), getattr(whole, f), err_msg=f"{what}: {f}")

    # two chunks of 8 instances: the same kernel family, the same result
    _, cfg_c, task_c, lims_c, _ = tms._far_setup()
    chunked = mink.solve_ik_trajectory_ladder(cfg_c, [task_c], 1.0, {task_c: tg}, limits=lims_c, update=False, qvel_dt=0.05, refine=True,
                                              max_instances=8 * T * S + 3, **_KW5)
    prob_c = list(cfg_c._problems.values())[-1]
    assert prob_c.max_batch == 8 * T * S and prob_c.last_kernel() == _far["kernel"]
    same(chunked, "max_instances")
    # update=True: the configuration is left at the returned q[:, -1]
    moved = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, refine=True, **_KW5)
    np.testing.assert_array_equal(moved.q, whole.q)
    np.testing.assert_array_equal(cfg.q_batch, whole.q[:, -1])
    cfg.update(home)
    # an unbatched configuration: unbatched fields
    c1 = mink.Configuration(m, home[0])
    r1 = mink.solve_ik_trajectory_ladder(c1, [task], 1.0, {task: tg[3]}, limits=lims, refine=True, **_KW5)
    assert r1.q.shape == (T, m.nq) and r1.repaired.shape == (T,) and np.ndim(r1.refined) == 0 and np.ndim(r1.path_length) == 0
    # T = 1 and no gate
    one = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg[:, :1]}, limits=lims, update=False, refine=True,
                                          **{**_KW5, "max_step": None})
    assert one.q.shape == (B, 1, m.nq) and not one.edge_break.any() and (one.repaired <= 1).all()
    free = mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, refine=True, **{**_KW5, "max_step": None})
    assert (free.n_breaks == 0).all() and (free.n_tracked >= plain.n_tracked).all()


def test_plumbing_of_the_pass_alone(nat, monkeypatch, caplog):
    import mink_amd as mink
    m, cfg, task, lims, tg, qA = _line()
    T, B = _T2, _B2
    home = cfg.q_batch.copy()
    path, trk = qA.copy(), np.ones((B, T), dtype=bool)
    trk[:, 3] = False
    whole = mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, **_KW2)
    kernel = list(cfg._problems.values())[-1].last_kernel()
    # chunks of 2 and 1 instances
    _, cfg_c, task_c, lims_c, _, _ = _line()
    chunked = mink.refine_path(cfg_c, [task_c], 1.0, {task_c: tg}, path, trk, limits=lims_c, update=False, max_instances=2, **_KW2)
    prob_c = list(cfg_c._problems.values())[-1]
    assert prob_c.max_batch == 2 and prob_c.last_kernel() == kernel
    for f in whole._fields:
        np.testing.assert_array_equal(getattr(chunked, f), getattr(whole, f), err_msg=f"max_instances: {f}")
    # update=True (the default) leaves the configuration at the returned q[:, -1]
    mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, **_KW2)
    np.testing.assert_array_equal(cfg.q_batch, whole.q[:, -1])
    cfg.update(home)
    # an unbatched configuration, a shared (T,) flag row; T = 1; no gate
    c1 = mink.Configuration(m, home[0])
    r1 = mink.refine_path(c1, [task], 1.0, {task: tg[1]}, path[1], trk[1], limits=lims, **_KW2)
    assert r1.q.shape == (T, m.nq) and r1.repaired.shape == (T,) and np.ndim(r1.refined) == 0
    np.testing.assert_array_equal(r1.q, whole.q[1])
    one = mink.refine_path(cfg, [task], 1.0, {task: tg[:, :1]}, path[:, :1], np.zeros((B, 1)), limits=lims, update=False, **_KW2)
    assert one.q.shape == (B, 1, m.nq) and set(one.repaired.ravel().tolist()) <= {0, 1} and not one.edge_break.any()
    free = mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, **{**_KW2, "max_step": None})
    assert free.refined.all() and (free.n_breaks == 0).all() and (free.repaired != 0).sum() == B
    # status bits count on the RETURNED nodes only: the loops of waypoints that were not bad are discarded with their bits
    from mink_amd import _native
    real = _native.NativeProblem.ladder_refine

    def with_bits(bits_repaired, bits_kept):
        def patched(self, *a, **k):
            r = real(self, *a, **k)
            st = np.where(r.repaired != 0, r.status | bits_repaired, r.status | bits_kept).astype(np.int32)
            return r._replace(status=st)
        return patched

    monkeypatch.setattr(_native.NativeProblem, "ladder_refine", with_bits(_native.ST_OUTSIDE_LIMITS, 0))
    with pytest.raises(mink.NotWithinConfigurationLimits, match=r"\(instance, waypoint\) = \(0, 3\)"):
        mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, safety_break=True, **_KW2)
    with caplog.at_level(logging.WARNING):
        mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, **_KW2)
    assert "outside their configuration limits" in caplog.text
    monkeypatch.setattr(_native.NativeProblem, "ladder_refine", with_bits(2, 0))
    with pytest.raises(mink.SolverError, match=r"QP failed at 3 of 18 returned nodes \(first: \(instance, waypoint\) = \(0, 3\)"):
        mink.refine_path(cfg, [task], 1.0, {task: tg}, path, trk, limits=lims, update=False, **_KW2)
    # an untouched line: nothing is returned from a loop, so no loop's bit can reach the caller
    monkeypatch.setattr(_native.NativeProblem, "ladder_refine", real)
    quiet = mink.refine_path(cfg, [task], 1.0, {task: tg}, qA, limits=lims, update=False, safety_break=True, **_KW2)
    assert not quiet.status.any() and not quiet.refined.any()
