"""Multi-start trajectory IK on the device (mkh_solve_trajectory_multistart / mink_amd.solve_ik_trajectory_multistart): the
candidates' loops are mkh_solve_trajectory's on the fanned-out instances — bitwise —, one seed is that call itself, the seeds
are multi-start's, the selection is the stated rule applied to the device's own candidates, the result does not depend on
chunks or shards, and it tracks paths a single start loses."""

from types import SimpleNamespace

import numpy as np
import pytest

import multistart_ref as msref
import oracle_configs as oc
import test_gpu_trajectory as tj
import trajectory_multistart_ref as ref
import trajectory_ref as tref
from mink_amd import workloads
from oracle import ik as oik

pytestmark = pytest.mark.gpu
ALL = ("q_all", "v_all", "status_all", "iters_all", "converged_all")
CHOSEN = ("q", "v", "status", "iters", "converged")
PER_INSTANCE = ("seed_index", "n_tracked", "n_complete", "path_length")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _np(x):
    return None if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy())


# B, T, S; thresholds, iterations per waypoint and the spread of the path are tests/test_gpu_trajectory.py's for the same config
_WORKLOADS = {"ur5e_c2": (6, 4, 4), "g1_c3": (4, 3, 3), "h1_full": (4, 3, 3)}
_cache = {}


def _workload(nat, name, shape=None):
    """tests/test_gpu_trajectory.py::_workload with a handle for B·S instances."""
    B, T, S = shape or _WORKLOADS[name]
    if (name, B, T, S) in _cache:
        return _cache[name, B, T, S]
    _, _, pth, oth, iters, sigma = tj._WORKLOADS[name]
    m = workloads.load_bench_robot(name)
    nm = nat.NativeModel(m, 0)
    prob, dt, damping = workloads.bench_config(name, m, nm, B * S)
    rng = np.random.default_rng(9)
    q, _, pt, _ = workloads.bench_batch(name, m, nm, prob, rng, B)
    taps = tj._taps_along(prob, tj._line(nm, q, T, rng, sigma), pt, ["frame_pose"] + (["subtree_com"] if prob.n_com else []))
    ct = np.ascontiguousarray(taps["subtree_com"][:, :, None, :] + 0.01) if prob.n_com else None      # (B, T, 1, 3)
    w = SimpleNamespace(name=name, m=m, nm=nm, prob=prob, dt=dt, damping=damping, q=q, tg=taps["frame_pose"], pt=pt, ct=ct, B=B, T=T,
                        S=S, until=(pth, oth), iters=iters)
    _cache[name, B, T, S] = w
    return w


def _kw(w, **extra):
    return dict(n_seeds=w.S, n_steps=w.iters, pos_threshold=w.until[0], ori_threshold=w.until[1], **extra)


def _repeated(x, B, S, held_ndim):
    """A (B, T, ...) target as solve_trajectory(time_major=True) takes it for the B·S candidates: (T, B·S, ...), the rows of
    instance b repeated S times; a held target keeps its shape, repeated when it has a B axis."""
    if x is None:
        return None
    if x.ndim == held_ndim:
        return x
    if x.ndim == held_ndim + 1:
        return np.repeat(x, S, axis=0) if x.shape[0] == B else x           # (B, n, w) held / (T, n, w): T leads already
    return np.ascontiguousarray(np.repeat(tref.to_time_major(x), S, axis=1))


def _loops_on_the_seeds(w, seeds, pt=None, ct=None):
    """The reference of tests 1, 2 and 5: solve_trajectory, time-major, on the B·S seeds with the targets repeated on the host."""
    pt, ct = w.pt if pt is None else pt, w.ct if ct is None else ct
    out = w.prob.solve_trajectory(seeds, _repeated(w.tg, w.B, w.S, 0), _repeated(pt, w.B, w.S, 2), _repeated(ct, w.B, w.S, 2), w.dt,
                                  w.damping, n_steps=w.iters, until=w.until, time_major=True)
    return out, w.prob.last_kernel()


def _same_all(out, want, what):
    for f, g in zip(ALL, CHOSEN):
        np.testing.assert_array_equal(_np(getattr(out, f)), _np(getattr(want, g)), err_msg=f"{what}: {f}")


def _chosen_rows_are_rows_of_all(out, S, time_major, what):
    pick = _np(out.seed_index)
    for f, g in zip(ALL, CHOSEN):
        np.testing.assert_array_equal(_np(getattr(out, g)), ref.chosen(_np(getattr(out, f)), pick, S, time_major), err_msg=f"{what}: {g}")


# ------------------------------------------------------------------ 1. composition
@pytest.mark.parametrize("name", list(_WORKLOADS))
def test_loops_are_the_existing_loops_bitwise(nat, name):
    """Same kernel, same seeds, the targets repeated on the host instead of fanned out on the device: a difference is a bug in
    the fan-out, the slabs or the gather.  Both caller layouts, numpy and torch."""
    import torch
    w = _workload(nat, name)
    B, T, S, m = w.B, w.T, w.S, w.m
    if name == "h1_full":
        assert w.ct is not None and w.ct.shape == (B, T, 1, 3)              # per waypoint AND per instance: fanned out per waypoint
    out = w.prob.solve_trajectory_multistart(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, return_all=True, rng_seed=4, **_kw(w))
    k = w.prob.last_kernel()
    assert out.q_all.shape == (T, B * S, m.nq) and out.v_all.shape == (T, B * S, m.nv) and out.status_all.shape == (T, B * S)
    assert out.seeds.shape == (B * S, m.nq) and out.q.shape == (B, T, m.nq) and out.seed_index.shape == (B,)
    np.testing.assert_array_equal(out.seeds[::S], w.q)                      # candidate 0: the caller's q, bit for bit
    want, k_ref = _loops_on_the_seeds(w, out.seeds)
    cv = want.converged != 0
    print(f"{name}: kernel {k}, {int(cv.sum())} of {cv.size} candidate waypoints converged, {int(((want.status & ~1) != 0).sum())} "
          f"with a failure bit, picks {out.seed_index.tolist()}, n_tracked {out.n_tracked.tolist()}, n_complete {out.n_complete.tolist()}")
    assert k and k_ref == k, (k, k_ref)
    _same_all(out, want, name)
    _chosen_rows_are_rows_of_all(out, S, False, name)
    # time-major caller arrays: the same candidates, the chosen outputs with T in front
    tm = w.prob.solve_trajectory_multistart(w.q, tref.to_time_major(w.tg), w.pt, tref.to_time_major(w.ct), w.dt, w.damping,
                                            return_all=True, rng_seed=4, time_major=True, **_kw(w))
    assert w.prob.last_kernel() == k and tm.q.shape == (T, B, m.nq) and tm.status.shape == (T, B)
    _same_all(tm, want, name + ", time-major")
    _chosen_rows_are_rows_of_all(tm, S, True, name + ", time-major")
    for f in PER_INSTANCE + ("seeds",):
        np.testing.assert_array_equal(getattr(tm, f), getattr(out, f), err_msg=f)
    # torch tensors on the device, both layouts: the loops write the caller's *_all directly
    dev = torch.device("cuda:0")
    on = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)
    for time_major in (False, True):
        lead = (lambda x: tref.to_time_major(x)) if time_major else (lambda x: x)
        tt = w.prob.solve_trajectory_multistart(on(w.q), on(lead(w.tg)), on(w.pt), on(lead(w.ct)), w.dt, w.damping, return_all=True,
                                                rng_seed=4, time_major=time_major, qvel_dt=0.05, **_kw(w))
        assert w.prob.last_kernel() == k
        assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in tt)
        what = f"{name}, torch, time_major={time_major}"
        _same_all(tt, want, what)
        _chosen_rows_are_rows_of_all(tt, S, time_major, what)
        for f in PER_INSTANCE + ("seeds",):
            np.testing.assert_array_equal(_np(getattr(tt, f)), getattr(out, f), err_msg=f"{what}: {f}")
        np.testing.assert_array_equal(_np(tt.q), tm.q if time_major else out.q)
    if name != "ur5e_c2":
        return
    # the same posture target in every shape the call takes: held per instance (fanned out once), with a T axis alone (read in
    # place), with both (fanned out per waypoint) — the candidates do not notice
    assert w.pt.shape == (1, m.nq) and T != B
    for what, pt in (("posture (B, n, nq)", np.ascontiguousarray(np.broadcast_to(w.pt, (B,) + w.pt.shape))),
                     ("posture (T, n, nq)", np.ascontiguousarray(np.broadcast_to(w.pt, (T,) + w.pt.shape))),
                     ("posture (B, T, n, nq)", np.ascontiguousarray(np.broadcast_to(w.pt, (B, T) + w.pt.shape)))):
        alt = w.prob.solve_trajectory_multistart(w.q, w.tg, pt, w.ct, w.dt, w.damping, return_all=True, rng_seed=4, **_kw(w))
        _same_all(alt, want, what)
        np.testing.assert_array_equal(alt.seed_index, out.seed_index)
        if pt.ndim == 4:
            alt_tm = w.prob.solve_trajectory_multistart(w.q, tref.to_time_major(w.tg), tref.to_time_major(pt), w.ct, w.dt, w.damping,
                                                        return_all=True, rng_seed=4, time_major=True, **_kw(w))
            _same_all(alt_tm, want, what + ", time-major")


# ------------------------------------------------------------------ 2. one seed
@pytest.mark.parametrize("name", list(_WORKLOADS))
def test_one_seed_is_solve_trajectory(nat, name):
    w = _workload(nat, name)
    kw = dict(n_steps=w.iters, qvel_dt=0.02)
    for time_major in (False, True):
        lead = (lambda x: tref.to_time_major(x)) if time_major else (lambda x: x)
        want = w.prob.solve_trajectory(w.q, lead(w.tg), w.pt, lead(w.ct), w.dt, w.damping, until=w.until, time_major=time_major, **kw)
        k = w.prob.last_kernel()
        one = w.prob.solve_trajectory_multistart(w.q, lead(w.tg), w.pt, lead(w.ct), w.dt, w.damping, n_seeds=1, pos_threshold=w.until[0],
                                                 ori_threshold=w.until[1], time_major=time_major, return_all=True, **kw)
        assert w.prob.last_kernel() == k
        for f in ("q", "v", "status", "iters", "converged", "qvel"):
            np.testing.assert_array_equal(getattr(one, f), getattr(want, f), err_msg=f"time_major={time_major}: {f}")
        assert (one.seed_index == 0).all()
        np.testing.assert_array_equal(one.seeds, w.q)
        t_axis = 0 if time_major else 1
        tracked = ref.tracked(want.converged, want.status)
        np.testing.assert_array_equal(one.n_tracked, tracked.sum(axis=t_axis))
        np.testing.assert_array_equal(one.n_complete, tracked.all(axis=t_axis).astype(np.int32))
        np.testing.assert_array_equal(one.q_all, want.q if time_major else tref.to_time_major(want.q))


# ------------------------------------------------------------------ 3. seeds
def test_seeds_are_multistarts(nat):
    w = _workload(nat, "ur5e_c2")
    B, S, m = w.B, w.S, w.m
    first = np.ascontiguousarray(w.tg[:, 0])
    for rng_seed, t0 in ((0, 0), (2 ** 40 + 12345, 1000003)):
        out = w.prob.solve_trajectory_multistart(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, rng_seed=rng_seed, target_index0=t0,
                                                 return_all=True, **_kw(w))
        ms = w.prob.solve_multistart(w.q, first, w.pt, None, w.dt, w.damping, n_seeds=S, max_iters=1, pos_threshold=w.until[0],
                                     ori_threshold=w.until[1], rng_seed=rng_seed, target_index0=t0, return_all=True)
        np.testing.assert_array_equal(out.seeds, ms.seeds.reshape(B * S, m.nq))
        np.testing.assert_array_equal(out.seeds, msref.draw_seeds(m, w.q, S, rng_seed=rng_seed, target_index0=t0).reshape(B * S, m.nq))
        assert len(np.unique(out.seeds[:, 0])) > B * (S - 1) // 2
    # the caller's own starts are honoured, row 0 of every instance replaced by q
    own = np.random.default_rng(3).uniform(-1.0, 1.0, size=(B, S, m.nq))
    out = w.prob.solve_trajectory_multistart(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, seeds=own, rng_seed=77, return_all=True, **_kw(w))
    want = own.copy(); want[:, 0] = w.q
    np.testing.assert_array_equal(out.seeds, want.reshape(B * S, m.nq))
    _same_all(out, _loops_on_the_seeds(w, out.seeds)[0], "user seeds")


# ------------------------------------------------------------------ 4. selection
def _selection_inputs(nat, name):
    if name == "ballslide":                       # ball joints: the quaternion dofs in the length
        B, T, S = 12, 3, 8
        w = tj._ballslide(nat, B * S, T)          # (a handle for B·S instances; its first B rows are the instances here)
        w.q, w.tg, w.B, w.S = np.ascontiguousarray(w.q[:B]), np.ascontiguousarray(w.tg[:B]), B, S
        return w
    return _workload(nat, name, (12, 4, 8))


def _check_selection(w, out, weights, what, wdt=0.04):
    """The restatement on the device's own candidates.  Returns what the inputs exercised."""
    B, S, T, m = w.B, w.S, w.T, w.m
    pick, n_tr, n_comp, length, counts, lengths = ref.choose(m, w.q, out.q_all, out.converged_all, out.status_all, S, weights)
    np.testing.assert_array_equal(out.seed_index, pick, err_msg=what)
    np.testing.assert_array_equal(out.n_tracked, n_tr, err_msg=what)
    np.testing.assert_array_equal(out.n_complete, n_comp, err_msg=what)
    rel = np.abs(out.path_length - length) / np.maximum(np.abs(length), np.finfo(float).tiny)
    print(f"{what}: picks {pick.tolist()}, n_tracked {n_tr.tolist()}, n_complete {n_comp.tolist()}, path_length worst relative "
          f"|device - numpy| = {rel.max():.3e} ({'bit-equal' if np.array_equal(out.path_length, length) else 'not bit-equal'})")
    assert rel.max() <= 1e-12
    _chosen_rows_are_rows_of_all(out, S, False, what)
    want = tref.qvel(m, w.q, out.q, wdt)
    quat = tref.quaternion_dofs(m)
    np.testing.assert_array_equal(out.qvel[..., ~quat], want[..., ~quat])
    if quat.any():
        dev = np.abs(out.qvel[..., quat] - want[..., quat]) / np.maximum(1.0, np.abs(want[..., quat]))
        assert dev.max() <= 1e-9, dev.max()
    best = counts == counts.max(axis=1, keepdims=True)
    return SimpleNamespace(
        what=what, equal_count_other_length=any(len(np.unique(lengths[b, counts[b] == c])) > 1 for b in range(B) for c in np.unique(counts[b])),
        pick_not_lowest_of_best=bool((pick != best.argmax(axis=1)).any()),
        untracked_waypoint=bool((counts < T).any()), near_tie=min(
            (np.sort(lengths[b, best[b]])[1] / max(np.sort(lengths[b, best[b]])[0], 1e-300) - 1.0 for b in range(B) if best[b].sum() > 1),
            default=np.inf))


def test_selection_is_the_stated_rule(nat):
    seen = []
    for name in ("ur5e_c2", "ballslide"):
        w = _selection_inputs(nat, name)
        B, S, m = w.B, w.S, w.m
        weights = np.random.default_rng(1).uniform(0.1, 10.0, size=m.nv)
        kw = dict(return_all=True, rng_seed=8, qvel_dt=0.04, **_kw(w))
        quat = tref.quaternion_dofs(m)
        assert quat.any() == (name == "ballslide")
        for wts, what in ((None, name), (weights, name + ", weights")):
            out = w.prob.solve_trajectory_multistart(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, weights=wts, **kw)
            seen.append(_check_selection(w, out, wts, what))
        # seed 3 a copy of seed 1: the same path, the same score — the tie goes to the lower index, 3 is never returned
        own = out.seeds.reshape(B, S, m.nq).copy()
        own[:, 3] = own[:, 1]
        dup = w.prob.solve_trajectory_multistart(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, seeds=own, weights=weights, **kw)
        by = ref.by_instance(dup.q_all, B, S)
        np.testing.assert_array_equal(by[:, 3], by[:, 1])
        assert (dup.seed_index != 3).all()
        seen.append(_check_selection(w, dup, weights, name + ", seed 3 = seed 1"))
        print(f"{name}: seed 1 chosen for {int((dup.seed_index == 1).sum())} of {B} instances with its copy at 3")
        if name == "ballslide":
            w.prob.close(); w.nm.close()
    # the far paths of test 5 through the public call: (B, S, T, ·) back to the time-major rows of the native call
    whole, (m5, _) = _far_whole(), _far_paths()
    rows = lambda x: np.ascontiguousarray(np.moveaxis(x, 2, 0).reshape((_T5, _B5 * _S5) + x.shape[3:]))
    w5 = SimpleNamespace(B=_B5, S=_S5, T=_T5, m=m5, q=np.tile(m5.key_qpos[m5.name2id("key", "home")], (_B5, 1)))
    out5 = SimpleNamespace(q_all=rows(whole.q_all), converged_all=rows(whole.converged_all), status_all=rows(whole.status_all),
                           v_all=rows(whole.v_all), iters_all=rows(whole.iters_all), **{f: getattr(whole, f) for f in CHOSEN + PER_INSTANCE},
                           qvel=whole.qvel)
    seen.append(_check_selection(w5, out5, None, "far UR5e paths", wdt=0.05))
    # the inputs exercise the rule
    assert any(s.equal_count_other_length for s in seen)
    assert any(s.pick_not_lowest_of_best for s in seen)
    assert any(s.untracked_waypoint for s in seen)
    print("smallest relative gap between the best and the runner-up length at the best count (without the copied seed):",
          min(s.near_tie for s in seen if "seed 3" not in s.what))


# ------------------------------------------------------------------ the fixture of 5, 6, 7
_B5, _T5, _S5 = 16, 5, 8
_KW5 = dict(n_seeds=_S5, n_steps=40, pos_threshold=1e-4, ori_threshold=1e-4, damping=1e-3, rng_seed=5)
_far = {}


def _far_paths():
    """UR5e paths whose first pose is far from `home`: the site poses along q_goal + t·delta, q_goal uniform in the joint ranges
    (clipped to ±π), delta ~ N(0, 0.05²) per joint.  CPU check of this fixture with the numpy oracle (one FrameTask, costs
    1 / 1, lm_damping 1, ConfigurationLimit, dt = 1, damping 1e-3, thresholds 1e-4 / 1e-4, 40 iterations per waypoint, 8 seeds,
    rng_seed 5): no QP failure; candidate 0 tracks [4, 1, 0, 5, 5, 5, 5, 5, 4, 0, 5, 0, 5, 4, 5, 5] waypoints — 9 of 16 paths
    complete —, the best of 8 candidates 13 of 16; picks [1, 1, 1, 0, 0, 0, 0, 0, 0, 4, 0, 2, 0, 0, 0, 0]."""
    if "tg" not in _far:
        import mink_amd as mink
        m = workloads.load_robot("ur5e")
        rng = np.random.default_rng(20261018)
        lo, hi = np.maximum(m.jnt_range[:, 0], -np.pi), np.minimum(m.jnt_range[:, 1], np.pi)
        q_goal = rng.uniform(lo, hi, size=(_B5, 6))
        delta = rng.normal(scale=0.05, size=(_B5, 6))
        qs = np.stack([np.clip(q_goal + t * delta, lo, hi) for t in range(_T5)], axis=1)             # (B, T, 6)
        tg = mink.Configuration(m, qs.reshape(_B5 * _T5, 6)).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz
        _far["m"], _far["tg"] = m, np.ascontiguousarray(tg.reshape(_B5, _T5, 7))
    return _far["m"], _far["tg"]


def _far_setup(device=0, B=_B5):
    import mink_amd as mink
    m, tg = _far_paths()
    cfg = mink.Configuration(m, np.tile(m.key_qpos[m.name2id("key", "home")], (B, 1)), device=device)
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    return m, cfg, task, [mink.ConfigurationLimit(m)], tg[:B]


def _far_whole():
    if "whole" not in _far:
        import mink_amd as mink
        m, cfg, task, lims, tg = _far_setup()
        _far["whole"] = mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, return_all=True,
                                                            waypoint_dt=0.05, **_KW5)
        _far["cfg"], _far["kernel"] = cfg, list(cfg._problems.values())[-1].last_kernel()
        for x in _far["whole"]:
            x.setflags(write=False)
    return _far["whole"]


# ------------------------------------------------------------------ 5. it tracks what single start loses
def test_multistart_tracks_paths_single_start_loses(nat):
    m, tg = _far_paths()
    res = _far_whole()
    B, T, S = _B5, _T5, _S5
    assert res.q_all.shape == (B, S, T, m.nq)
    tracked_all = ref.tracked(res.converged_all, res.status_all)                       # (B, S, T)
    n0 = tracked_all[:, 0].sum(axis=1)
    assert (res.n_tracked >= n0).all()
    # candidate 0 is the single start: solve_trajectory on the B instances alone, on the same handle
    prob = list(_far["cfg"]._problems.values())[-1]
    home = np.tile(m.key_qpos[m.name2id("key", "home")], (B, 1))
    single = prob.solve_trajectory(home, tg[:, :, None, :], None, None, 1.0, 1e-3, n_steps=40, until=(1e-4, 1e-4))
    k1 = prob.last_kernel()
    if k1 == _far["kernel"]:
        for f, g in zip(ALL, CHOSEN):
            np.testing.assert_array_equal(getattr(res, f)[:, 0], getattr(single, g) if g != "converged" else single.converged != 0,
                                          err_msg=f)
    else:
        np.testing.assert_allclose(res.q_all[:, 0], single.q, rtol=0, atol=1e-9)
    done1 = ref.tracked(single.converged, single.status).all(axis=1)
    complete = res.n_tracked == T
    print(f"UR5e, {B} far paths of {T} waypoints from home (kernels {k1} / {_far['kernel']}): single start tracks "
          f"{ref.tracked(single.converged, single.status).sum(axis=1).tolist()} waypoints, completes {int(done1.sum())}; multi-start "
          f"({S} seeds) tracks {res.n_tracked.tolist()}, completes {int(complete.sum())}; picks {res.seed_index.tolist()}, "
          f"n_complete {res.n_complete.tolist()}")
    # every waypoint of every chosen complete path is a solution by the CPU oracle's kinematics, inside the joint ranges
    mo = oc.model("ur5e")
    sid = mo.name2id("site", "attachment_site")
    worst_p = worst_o = 0.0
    for b in np.flatnonzero(complete):
        for t in range(T):
            c = oik.Configuration(mo, res.q[b, t])
            e, _ = oik.task_error_jacobian(c, oik.FrameTaskSpec(sid, "site", np.ones(6), tg[b, t], lm_damping=1.0))
            worst_p, worst_o = max(worst_p, float(np.linalg.norm(e[:3]))), max(worst_o, float(np.linalg.norm(e[3:])))
            assert np.linalg.norm(e[:3]) <= 1e-4 + 1e-9 and np.linalg.norm(e[3:]) <= 1e-4 + 1e-9, (b, t, e)
            assert c.limit_violations(1e-6) == [], (b, t)
    print(f"worst error norms of the chosen complete paths by the oracle: position {worst_p:.3e}, orientation {worst_o:.3e}")
    # the fixture's conditions, as the GPU sees them
    assert done1.sum() <= 12
    assert complete.sum() > done1.sum()


# ------------------------------------------------------------------ 6. independence
def test_result_does_not_depend_on_chunks_or_shards(nat):
    import mink_amd as mink
    whole, k = _far_whole(), _far["kernel"]
    assert (whole.seed_index > 0).any()

    def same(other, what):
        for f in whole._fields:
            np.testing.assert_array_equal(getattr(other, f), getattr(whole, f), err_msg=f"{what}: {f}")

    def run(device=0, **extra):
        m, cfg, task, lims, tg = _far_setup(device)
        return cfg, mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, return_all=True,
                                                        waypoint_dt=0.05, **_KW5, **extra)

    cfg_c, chunked = run(max_instances=4 * _S5 + 3)                      # chunks of 4 instances
    prob_c = list(cfg_c._problems.values())[-1]
    assert prob_c.max_batch == 4 * _S5 and prob_c.last_kernel() == k
    same(chunked, "max_instances")
    cfg_s, sharded = run(device=[0, 0])
    shards = list(cfg_s._problems.values())[-1].shards            # (the cached ShardedProblem's handles, one per listed device)
    assert len(shards) == 2 and all(p.max_batch == 8 * _S5 and p.last_kernel() == k for p in shards)
    same(sharded, "device=[0, 0]")


# ------------------------------------------------------------------ 7. public API
def test_public_api(nat):
    import mink_amd as mink
    whole = _far_whole()
    B, T, S = _B5, _T5, _S5
    m, cfg, task, lims, tg = _far_setup()
    home = cfg.q_batch.copy()
    assert isinstance(whole, mink.TrajectoryMultistartResult)
    assert whole.q.shape == (B, T, m.nq) and whole.v.shape == (B, T, m.nv) and whole.qvel.shape == (B, T, m.nv)
    for f in ("status", "iters", "converged"):
        assert getattr(whole, f).shape == (B, T), f
    for f in PER_INSTANCE:
        assert getattr(whole, f).shape == (B,), f
    assert whole.q_all.shape == (B, S, T, m.nq) and whole.v_all.shape == (B, S, T, m.nv) and whole.seeds.shape == (B, S, m.nq)
    for f in ("status_all", "iters_all", "converged_all"):
        assert getattr(whole, f).shape == (B, S, T), f
    assert whole.converged.dtype == bool and whole.converged_all.dtype == bool
    np.testing.assert_array_equal(whole.seeds[:, 0], home)
    rows = np.arange(B)
    np.testing.assert_array_equal(whole.q, whole.q_all[rows, whole.seed_index])
    np.testing.assert_array_equal(whole.qvel, tref.qvel(m, home, whole.q, 0.05))       # hinges only: exact
    # the native call on a handle of the same tasks: the same numbers
    res = mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: tg}, limits=lims, update=False, **_KW5)
    np.testing.assert_array_equal(cfg.q_batch, home)                       # update=False leaves the configuration alone
    assert res.qvel is None and res.q_all is None and res.seeds is None
    for f in CHOSEN + PER_INSTANCE:
        np.testing.assert_array_equal(getattr(res, f), getattr(whole, f), err_msg=f)
    prob = list(cfg._problems.values())[-1]
    native = prob.solve_trajectory_multistart(home, tg[:, :, None, :], None, None, 1.0, 1e-3, n_seeds=S, n_steps=40, pos_threshold=1e-4,
                                              ori_threshold=1e-4, rng_seed=5)
    np.testing.assert_array_equal(native.q, whole.q); np.testing.assert_array_equal(native.seed_index, whole.seed_index)
    np.testing.assert_array_equal(native.path_length, whole.path_length)
    # update=True: the configuration is left at the chosen q[:, -1]
    moved = mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: tg}, limits=lims, **_KW5)
    np.testing.assert_array_equal(moved.q, whole.q)
    np.testing.assert_array_equal(cfg.q_batch, whole.q[:, -1])
    # a (T, 7) sequence is every instance's; (S, nq) seeds are every instance's
    cfg.update(home)
    shared = mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: tg[3]}, limits=lims, update=False, return_all=True,
                                                 seeds=whole.seeds[3], **_KW5)
    np.testing.assert_array_equal(shared.seeds, np.repeat(whole.seeds[3:4], B, axis=0))
    np.testing.assert_array_equal(shared.q[5], whole.q[3]); np.testing.assert_array_equal(shared.seed_index, np.repeat(whole.seed_index[3], B))
    # unbatched configuration: unbatched fields
    c1 = mink.Configuration(m, home[0])
    r1 = mink.solve_ik_trajectory_multistart(c1, [task], 1.0, {task: tg[3]}, limits=lims, return_all=True, waypoint_dt=0.05,
                                             seeds=whole.seeds[3], **_KW5)
    assert r1.q.shape == (T, m.nq) and r1.converged.shape == (T,) and r1.qvel.shape == (T, m.nv) and r1.q_all.shape == (S, T, m.nq)
    assert r1.seeds.shape == (S, m.nq) and np.ndim(r1.seed_index) == 0 and np.ndim(r1.path_length) == 0
    np.testing.assert_array_equal(r1.q, whole.q[3]); np.testing.assert_array_equal(c1.q, whole.q[3, -1])
    assert int(r1.seed_index) == int(whole.seed_index[3]) and int(r1.n_tracked) == int(whole.n_tracked[3])

    # caller-defined tasks: the refusal of solve_ik_steps
    class Mine(mink.Task):
        def compute_error(self, configuration):
            return np.zeros((configuration.batch_size, 3))

        def compute_jacobian(self, configuration):
            return np.zeros((configuration.batch_size, 3, configuration.nv))

    with pytest.raises(mink.TaskDefinitionError, match="caller-defined Task / Limit"):
        mink.solve_ik_trajectory_multistart(cfg, [task, Mine(cost=np.ones(3))], 1.0, {task: tg}, limits=lims, **_KW5)
    # the handle is sized for B·S: a native call beyond it is refused, by the wrapper and by the library
    with pytest.raises(nat.MinkHipError, match="exceeds max_batch"):
        prob.solve_trajectory_multistart(home, tg[:, :, None, :], None, None, 1.0, 1e-3, n_seeds=S + 1, n_steps=5, pos_threshold=1e-4,
                                         ori_threshold=1e-4)
    import ctypes
    L = nat.lib()
    buf = np.zeros((B * (S + 1), T, 8))
    io = nat.MkhTrajectoryMultistartIO()
    for f in ("q_traj", "v_traj", "status", "iters", "converged", "seed_index", "n_tracked", "n_complete", "path_length"):
        setattr(io, f, buf.ctypes.data)
    rc = L.mkh_solve_trajectory_multistart(prob.handle, B, T, S + 1, buf.ctypes.data, buf.ctypes.data, None, None, 1.0, 1e-3, 5, 1e-4, 1e-4,
                                           0, 0, ctypes.byref(io), 0, None)
    assert rc == -1 and b"B * n_seeds" in L.mkh_last_error() and b"exceeds max_batch" in L.mkh_last_error()


# ------------------------------------------------------------------ 8. one handle, every outer loop
def _flat(out, prefix=""):
    """{field: numpy array} of a result, the trajectory inside a KeyframesOut included; fields that are None left out."""
    fields = {}
    for f, x in zip(out._fields, out):
        if hasattr(x, "_fields"):
            fields.update(_flat(x, prefix + f + "."))
        elif x is not None:
            fields[prefix + f] = _np(x)
    return fields


@pytest.mark.parametrize("name", ["ur5e_c2", "h1_full"])
def test_one_handle_serves_every_outer_loop_in_any_order(nat, name):
    """The four outer-loop entry points share one workspace per handle, by role.  ONE handle runs them interleaved, at changing
    sizes and with host and device arrays; every field of every call equals — bit for bit — the same call on a fresh handle of
    its own.  h1_full has per-instance, per-waypoint CoM targets: the CoM slabs are in use."""
    import torch
    w = _workload(nat, name)
    B, T, S, m = w.B, w.T, w.S, w.m
    rng = np.random.default_rng(21)
    seeds = rng.uniform(-1.0, 1.0, size=(B, S, m.nq))
    if m.nq != m.nv:                                                        # (a floating base: keep the caller's, as the seeder does)
        seeds[:, :, :7] = w.q[:, None, :7]
    reference = w.q + 0.05 * rng.standard_normal(w.q.shape)
    weights = rng.uniform(0.5, 2.0, size=m.nv)
    first = lambda x: None if x is None else np.ascontiguousarray(x[:, 0])  # waypoint 0's targets: a multi-start call's
    keys = lambda x: None if x is None else np.ascontiguousarray(x[:, :3])  # waypoints 0..2 as K = 3 keyframes
    kt, wt = np.array([0.0, 1.0, 2.0]), np.linspace(0.0, 2.0, T + 1)
    thr = dict(pos_threshold=w.until[0], ori_threshold=w.until[1])
    ms = dict(max_iters=w.iters, return_all=True, **thr)
    dev = torch.device("cuda:0")
    on = lambda x: x if not isinstance(x, np.ndarray) else torch.as_tensor(np.ascontiguousarray(x), device=dev)

    # (method, positional arrays, keywords) of calls 1 … 6; 5 is two calls, 6 is 1 again
    tms = ("solve_trajectory_multistart", (w.q, w.tg, w.pt, w.ct), dict(return_all=True, qvel_dt=0.05, rng_seed=4, **_kw(w)))
    calls = [tms,
             ("solve_multistart", (w.q, first(w.tg), w.pt, first(w.ct)),
              dict(n_seeds=S, seeds=seeds, reference=reference, weights=weights, **ms)),
             ("solve_keyframes", (w.q, kt, wt, keys(w.tg), w.pt, keys(w.ct)), dict(n_steps=w.iters, until=w.until, return_targets=True)),
             ("solve_trajectory", (w.q, w.tg, w.pt, w.ct), dict(n_steps=w.iters, until=w.until, qvel_dt=0.02)),
             ("solve_multistart", (w.q, first(w.tg), w.pt, first(w.ct)), dict(n_seeds=2, rng_seed=11, **ms)),
             ("solve_multistart", (w.q, first(w.tg), w.pt, first(w.ct)), dict(n_seeds=S, rng_seed=11, **ms)),
             tms]
    number = (1, 2, 3, 4, 5, 5, 6)

    def call(prob, method, args, kw, device):
        if device:
            args, kw = tuple(on(x) for x in args), {k: on(v) for k, v in kw.items()}
        return _flat(getattr(prob, method)(*args, w.dt, w.damping, **kw))

    def fresh(method, args, kw, device):
        prob, _, _ = workloads.bench_config(name, m, w.nm, B * S)
        try:
            return call(prob, method, args, kw, device)
        finally:
            prob.close()

    want = {}                                                               # (index of the call, device arrays) → its fields
    for torch_evens in (False, True):
        prob, _, _ = workloads.bench_config(name, m, w.nm, B * S)
        assert prob.max_batch == B * S
        try:
            got = []
            for i, (method, args, kw) in enumerate(calls):
                device = torch_evens and number[i] % 2 == 0
                if (i, device) not in want:
                    want[i, device] = fresh(method, args, kw, device)
                got.append(call(prob, method, args, kw, device))
                what = f"{name}, call {number[i]} ({method}{', torch' if device else ''})"
                assert set(got[-1]) == set(want[i, device]), what
                for f, x in got[-1].items():
                    np.testing.assert_array_equal(x, want[i, device][f], err_msg=f"{what}: {f}")
            assert set(got[6]) == set(got[0])
            for f, x in got[6].items():
                np.testing.assert_array_equal(x, got[0][f], err_msg=f"{name}: call 6 against call 1: {f}")
        finally:
            prob.close()
