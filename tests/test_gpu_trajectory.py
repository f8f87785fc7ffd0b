"""Trajectory IK on the device (mkh_solve_trajectory / mink_amd.solve_ik_trajectory): the call is the caller's loop of
mkh_solve_until / mkh_solve_steps over the waypoints — bitwise —, in either layout and with either kind of array; every
waypoint's loop is the oracle's loop from the device's own previous configuration; the waypoint velocity is the header's
rule; chunks, shards and warm starts do not change the answers."""

import os
from types import SimpleNamespace

import numpy as np
import pytest

import multistart_ref as msref
import native_configs as nc
import oracle_configs as oc
import trajectory_ref as ref
from mink_amd import workloads
from oracle import ik as oik

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("q", "v", "status", "iters", "converged", "qvel")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _np(x):
    return None if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy())


def _same(a, b, what, fields=FIELDS, swap_b=False):
    for f in fields:
        x, y = _np(getattr(a, f)), _np(getattr(b, f))
        assert (x is None) == (y is None), (what, f)
        if x is not None:
            np.testing.assert_array_equal(x, ref.to_batch_major(y) if swap_b else y, err_msg=f"{what}: {f}")


def _line(nm, q0, T, rng, sigma, jump=0.3):
    """(T, B, nq): configurations along a joint-space line from q0, T points per instance; for one instance in four the last
    point jumps away by a 0.3-rad scale (tests/test_gpu_steps.py's far targets), so that its loop does not converge."""
    B, nv = q0.shape[0], nm.model.nv
    delta = rng.normal(scale=sigma, size=(B, nv))
    pts = [nm.integrate(q0, delta * ((t + 1) / T), 1.0) for t in range(T)]
    far = nm.integrate(q0, delta + rng.normal(size=(B, nv)) * jump, 1.0)
    pts[-1][3::4] = far[3::4]
    return np.stack(pts, axis=0)


def _taps_along(prob, line, pt, names):
    """frame_pose / subtree_com taps of the (T, B, nq) configurations: (B, T, ...) arrays."""
    T, B = line.shape[:2]
    dummy = np.zeros((B, prob.n_frame, 7)); dummy[:, :, 0] = 1.0
    ct = np.zeros((prob.n_com, 3)) if prob.n_com else None
    rows = [prob.solve(line[t], dummy, pt, ct, 1.0, 1.0, taps=list(names), solve_qp=False)[2] for t in range(T)]
    return {n: np.ascontiguousarray(np.stack([r[n] for r in rows], axis=1)) for n in names}


# ------------------------------------------------------------------ 1. composition
# B, T, position / orientation thresholds, max_iters per waypoint, σ of the line's end point per dof.  Iterations and the
# humanoids' and the hand's thresholds are tests/test_gpu_multistart.py's (the velocity limits of these set-ups allow ~0.01 rad
# per step).  UR5e: the bench batch starts anywhere in the ±2π joint ranges, where the posture task holds the frame error above
# that file's 1e-3 / 1e-2 (CPU oracle, this seed: 41 of 288 waypoints converge); at 2e-2 / 5e-2 the oracle converges 276 of 288,
# 39 of 48 at the last waypoint — the device gave the oracle's counts waypoint for waypoint at the tighter pair.
# G1 (`g1_c3`), same check: the oracle converges 88 of 96 waypoints, 20 of 24 at the last one, in 2 … 44 iterations.
# Shadow hand (`shadow_c4`, position-only fingertip tasks, collision rows: no oracle loop cheap enough): a census of
# this input on the device (profiles/r11_trajectory.txt) — at that file's 2e-3 the collision rows and the posture task leave 28 of
# 96 waypoints converged, [14, 8, 5, 1] per waypoint; at 5e-3, 64 of 96, [21, 18, 15, 10], none of the six jumps.  `h1_full` at
# the humanoids' pair: 65 of 96, [19, 19, 15, 12].
_WORKLOADS = {"ur5e_c2": (48, 6, 2e-2, 5e-2, 60, 0.15), "g1_c3": (24, 4, 2e-2, 5e-2, 60, 0.15),
              "h1_full": (24, 4, 2e-2, 5e-2, 60, 0.15), "shadow_c4": (24, 4, 5e-3, 1.0, 60, 0.15)}
_cache = {}


def _workload(nat, name):
    if name in _cache:
        return _cache[name]
    B, T, pth, oth, iters, sigma = _WORKLOADS[name]
    m = workloads.load_bench_robot(name)
    nm = nat.NativeModel(m, 0)
    prob, dt, damping = workloads.bench_config(name, m, nm, B)
    rng = np.random.default_rng(9)
    q, _, pt, _ = workloads.bench_batch(name, m, nm, prob, rng, B)
    taps = _taps_along(prob, _line(nm, q, T, rng, sigma), pt, ["frame_pose"] + (["subtree_com"] if prob.n_com else []))
    ct = (taps["subtree_com"][:, :, None, :] + 0.01) if prob.n_com else None      # per waypoint AND per instance: (B, T, 1, 3)
    w = SimpleNamespace(name=name, m=m, nm=nm, prob=prob, dt=dt, damping=damping, q=q, tg=taps["frame_pose"], pt=pt,
                        ct=None if ct is None else np.ascontiguousarray(ct), B=B, T=T, until=(pth, oth), iters=iters, loops={})
    _cache[name] = w
    return w


def _callers_loop(w, until):
    """The reference of this file: prob.solve per waypoint from where the previous one ended, stacked by hand.  Computed once
    per workload and mode."""
    key = until is not None
    if key not in w.loops:
        q_prev, rows, kernels = w.q, [], set()
        for t in range(w.T):
            res = w.prob.solve(q_prev, np.ascontiguousarray(w.tg[:, t]), ref.waypoint_target(w.pt, t, w.prob.n_posture, w.m.nq, w.B),
                               ref.waypoint_target(w.ct, t, w.prob.n_com, 3, w.B), w.dt, w.damping, n_steps=w.iters, until=until)
            kernels.add(w.prob.last_kernel())
            rows.append(res)
            q_prev = res[0]
        stack = lambda k: np.stack([r[k] for r in rows], axis=1)
        w.loops[key] = (SimpleNamespace(q=stack(0), v=stack(1), status=stack(2), iters=stack(3) if key else None,
                                        converged=stack(4) if key else None, qvel=None), kernels)
        for x in vars(w.loops[key][0]).values():
            if x is not None:
                x.setflags(write=False)
    return w.loops[key]


@pytest.mark.parametrize("mode", ["until", "fixed"])
@pytest.mark.parametrize("name", list(_WORKLOADS))
def test_trajectory_is_the_callers_loop_bitwise(nat, name, mode):
    """Same kernel, same inputs, T launches in the same order: a difference is a bug in the slabs or the transposes."""
    w = _workload(nat, name)
    until = w.until if mode == "until" else None
    if name == "h1_full":
        assert w.ct is not None and w.ct.shape == (w.B, w.T, 1, 3)
    out = w.prob.solve_trajectory(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, n_steps=w.iters, until=until)
    k = w.prob.last_kernel()
    want, kernels = _callers_loop(w, until)
    assert k and kernels == {k}, (k, kernels)
    assert out.q.shape == (w.B, w.T, w.m.nq) and out.v.shape == (w.B, w.T, w.m.nv) and out.status.shape == (w.B, w.T)
    if mode == "until":
        cv = want.converged != 0
        print(f"{name}: kernel {k}, {int(cv.sum())} of {cv.size} waypoints converged, per waypoint {cv.sum(axis=0).tolist()}, "
              f"{int(((want.status & ~1) != 0).sum())} with a failure bit, iterations up to {int(want.iters.max())}")
        assert cv.sum() > cv.size // 2 and (~cv).any()          # neither all trivial nor all failed
        assert (~cv[:, -1]).any()
    else:
        assert out.iters is None and out.converged is None
    _same(out, want, f"{name} {mode}", fields=FIELDS[:5])


# ------------------------------------------------------------------ 2. layouts and array kinds
@pytest.mark.parametrize("name", ["ur5e_c2", "h1_full"])
def test_layouts_and_array_kinds_agree(nat, name):
    import torch
    w = _workload(nat, name)
    kw = dict(n_steps=w.iters, until=w.until, qvel_dt=0.02)
    bm = w.prob.solve_trajectory(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, **kw)
    _same(bm, _callers_loop(w, w.until)[0], "batch-major", fields=FIELDS[:5])
    tm = w.prob.solve_trajectory(w.q, ref.to_time_major(w.tg), w.pt, ref.to_time_major(w.ct), w.dt, w.damping, time_major=True, **kw)
    assert tm.q.shape == (w.T, w.B, w.m.nq) and tm.status.shape == (w.T, w.B) and tm.qvel.shape == (w.T, w.B, w.m.nv)
    _same(bm, tm, "time-major", swap_b=True)
    dev = torch.device("cuda:0")
    on = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)
    bm_t = w.prob.solve_trajectory(on(w.q), on(w.tg), on(w.pt), on(w.ct), w.dt, w.damping, **kw)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in bm_t)
    _same(bm, bm_t, "torch, batch-major")
    tm_t = w.prob.solve_trajectory(on(w.q), on(ref.to_time_major(w.tg)), on(w.pt), on(ref.to_time_major(w.ct)), w.dt, w.damping,
                                   time_major=True, **kw)
    assert tuple(tm_t.q.shape) == (w.T, w.B, w.m.nq)
    _same(bm, tm_t, "torch, time-major", swap_b=True)
    # fixed count: no iters / converged, the rest as before
    fx = w.prob.solve_trajectory(on(w.q), on(ref.to_time_major(w.tg)), on(w.pt), on(ref.to_time_major(w.ct)), w.dt, w.damping,
                                 n_steps=w.iters, time_major=True)
    assert fx.iters is None and fx.converged is None and fx.qvel is None
    _same(_callers_loop(w, None)[0], fx, "torch, time-major, fixed count", fields=FIELDS[:3], swap_b=True)
    # a target with a T axis against the same target held: posture (T, n, nq) / (B, T, n, nq), CoM (B, T, 1, 3)
    T, B = w.T, w.B
    held_ct = None if w.ct is None else np.ascontiguousarray(w.ct[:, 0])                       # (B, 1, 3), held
    base = w.prob.solve_trajectory(w.q, w.tg, w.pt, held_ct, w.dt, w.damping, **kw)
    rep_ct = None if w.ct is None else np.ascontiguousarray(np.repeat(w.ct[:, :1], T, axis=1))
    assert T != B
    for what, pt in (("posture (T, n, nq)", np.ascontiguousarray(np.repeat(w.pt[None], T, axis=0))),
                     ("posture (B, T, n, nq)", np.ascontiguousarray(np.broadcast_to(w.pt, (B, T) + w.pt.shape))),
                     ("posture (B, n, nq)", np.ascontiguousarray(np.broadcast_to(w.pt, (B,) + w.pt.shape)))):
        _same(base, w.prob.solve_trajectory(w.q, w.tg, pt, rep_ct, w.dt, w.damping, **kw), what)
        lead = lambda x: ref.to_time_major(x) if x is not None and x.ndim == 4 else x
        _same(base, w.prob.solve_trajectory(w.q, lead(w.tg), lead(pt), lead(rep_ct), w.dt, w.damping, time_major=True, **kw),
              what + ", time-major", swap_b=True)


def _ur5e_api(B, q=None, device=0):
    """UR5e with the tasks and limits of `ur5e_c2` through the public classes."""
    import mink_amd as mink
    m = workloads.load_robot("ur5e")
    home = m.key_qpos[m.name2id("key", "home")]
    cfg = mink.Configuration(m, np.tile(home, (B, 1)) if q is None else q, device=device)
    task = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    post = mink.PostureTask(m, cost=1e-2); post.set_target(home)
    lims = [mink.ConfigurationLimit(m), mink.VelocityLimit(m, {n: np.pi for n in m.jnt_names})]
    return m, cfg, task, post, lims


def test_one_waypoint_is_solve_ik_steps(nat):
    import mink_amd as mink
    w = _workload(nat, "ur5e_c2")
    m, cfg, task, post, lims = _ur5e_api(w.B, w.q)
    kw = dict(damping=w.damping, limits=lims, update=False, pos_threshold=w.until[0], ori_threshold=w.until[1])
    one = mink.solve_ik_trajectory(cfg, [task, post], w.dt, {task: w.tg[:, :1, 0]}, n_steps=w.iters, **kw)
    task.set_target(mink.SE3(w.tg[:, 0, 0]))
    q1, v1, it1, cv1 = mink.solve_ik_steps(cfg, [task, post], w.dt, w.iters, **kw)
    assert one.q.shape == (w.B, 1, m.nq)
    np.testing.assert_array_equal(one.q[:, 0], q1); np.testing.assert_array_equal(one.v[:, 0], v1)
    np.testing.assert_array_equal(one.iters[:, 0], it1); np.testing.assert_array_equal(one.converged[:, 0], cv1)
    assert 0 < cv1.sum()


# ------------------------------------------------------------------ 3. reference semantics
def test_every_waypoint_is_the_oracles_loop_from_the_devices_own_start(nat):
    """tests/test_gpu_steps.py::test_threshold_terminated_loop_matches_the_callers_loop per waypoint: one loop of at most
    max_iters steps from a common start — the device's own q[b, t - 1] —, hence that test's tolerances."""
    model = workloads.load_robot("ur5e")
    om = oc.model("ur5e")
    nm = nat.NativeModel(model)
    B, T, max_iters, pos_thr, ori_thr, dt = 8, 5, 20, 1e-4, 1e-4, 2e-2
    prob, _, damping = nc.build("ur5e_c2", nm, B)
    home = model.key_qpos[0]
    rng = np.random.default_rng(21)
    q0 = np.tile(home, (B, 1)) + rng.normal(scale=0.05, size=(B, model.nq))
    # (checked with the CPU oracle for this seed before the first GPU run: 36 of the 40 waypoints converge, in 2, 3 or 7
    #  iterations; instance 0 stops converging at its third waypoint and goes on from where its loop ended, instance 3's jump fails)
    tg = _taps_along(prob, _line(nm, q0, T, rng, 0.2), home[None, :], ["frame_pose"])["frame_pose"]
    out = prob.solve_trajectory(q0, tg, home[None, :], None, dt, damping, n_steps=max_iters, until=(pos_thr, ori_thr))
    assert prob.last_kernel() == "ik_quad_kernel_loop", prob.last_kernel()
    assert (out.status & ~1 == 0).all()
    cv = out.converged != 0
    print("iterations:", np.bincount(out.iters.reshape(-1), minlength=max_iters + 1).tolist(), "converged:", int(cv.sum()), "of", cv.size)
    assert cv.sum() > cv.size // 2 and (~cv).any()
    for b in range(B):
        for t in range(T):
            cfg = oik.Configuration(om, q0[b] if t == 0 else out.q[b, t - 1])
            _, tasks, limits, _, damp_o = oc.ur5e_c2(tg[b, t], home)
            done, n = False, 0
            for n in range(1, max_iters + 1):
                v_ref = oik.solve_ik(om, cfg, tasks, dt, damp_o, limits)
                cfg.update(cfg.integrate(v_ref, dt))
                err = oik.task_error_jacobian(cfg, tasks[0])[0]
                if np.linalg.norm(err[:3]) <= pos_thr and np.linalg.norm(err[3:]) <= ori_thr:
                    done = True
                    break
            assert (out.iters[b, t], bool(cv[b, t])) == (n, done), (b, t, out.iters[b, t], cv[b, t], n, done)
            np.testing.assert_allclose(out.q[b, t], cfg.q, rtol=0, atol=1e-10)
            np.testing.assert_allclose(out.v[b, t], v_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(v_ref).max()))
    prob.close(); nm.close()


# ------------------------------------------------------------------ 4. qvel
def _ballslide(nat, B, T):
    """A frame-task problem on the ball / slide / hinge chain (tests/test_gpu_multistart.py::test_selection_is_the_stated_rule)."""
    import mink_amd as mink
    from mink_amd.api_specs import configuration_limit_desc
    m = mink.load_mjcf(os.path.join(GOLDEN, "ballslide.xml"))
    nm = nat.NativeModel(m, 0)
    prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "tip"), "cost": [1.0] * 6,
                                               "gain": 1.0, "lm_damping": 0.1}],
                             configuration_limits=[configuration_limit_desc(m)], max_batch=B)
    rng = np.random.default_rng(4)
    q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (B, 1))
    for j in range(m.njnt):
        if m.jnt_type[j] in (ref.JNT_SLIDE, ref.JNT_HINGE):
            q[:, int(m.jnt_qposadr[j])] += rng.normal(scale=0.05, size=B)
    goal = msref.draw_seeds(m, q, T + 1, rng_seed=77)[:, 1:]                           # (B, T, nq): far apart, ball joints turned
    tg = mink.Configuration(m, goal.reshape(B * T, m.nq)).get_transform_frame_to_world("tip", "site").wxyz_xyz.reshape(B, T, 1, 7)
    return SimpleNamespace(m=m, nm=nm, prob=prob, q=q, tg=np.ascontiguousarray(tg), pt=None, ct=None, dt=1.0, damping=1e-3,
                           until=(1e-3, 1e-2), iters=40, B=B, T=T)


@pytest.mark.parametrize("name", ["h1_full", "ballslide"])
def test_qvel_is_the_stated_rule(nat, name):
    """Hinge / slide entries are EXACT (the kernel is compiled with contraction off: a rounded difference, a rounded quotient);
    quaternion entries within 1e-9 relative, the bound tests/test_gpu_multistart.py holds the same device quaternion
    difference to."""
    w = _workload(nat, name) if name == "h1_full" else _ballslide(nat, 16, 4)
    wdt = 0.04
    out = w.prob.solve_trajectory(w.q, w.tg, w.pt, w.ct, w.dt, w.damping, n_steps=w.iters, until=w.until, qvel_dt=wdt)
    want = ref.qvel(w.m, w.q, out.q, wdt)
    quat = ref.quaternion_dofs(w.m)
    assert quat.any() and (~quat).any()
    assert np.abs(want[..., quat]).max() > 1e-3 and np.abs(want[..., ~quat]).max() > 1e-3        # things moved
    np.testing.assert_array_equal(out.qvel[..., ~quat], want[..., ~quat])
    dev = np.abs(out.qvel[..., quat] - want[..., quat]) / np.maximum(1.0, np.abs(want[..., quat]))
    print(f"{name}: qvel of quaternion dofs, worst |device - numpy| / max(1, |numpy|) = {dev.max():.3e} "
          f"(largest |qvel| {np.abs(want[..., quat]).max():.3e})")
    assert dev.max() <= 1e-9
    tm = w.prob.solve_trajectory(w.q, ref.to_time_major(w.tg), w.pt, ref.to_time_major(w.ct), w.dt, w.damping, n_steps=w.iters,
                                 until=w.until, qvel_dt=wdt, time_major=True)
    np.testing.assert_array_equal(ref.to_batch_major(tm.qvel), out.qvel)
    if name == "ballslide":
        w.prob.close(); w.nm.close()


# ------------------------------------------------------------------ 5. chunks and shards
def _ur5e_line_targets(nat, B, T, seed=5):
    m = workloads.load_robot("ur5e")
    nm = nat.NativeModel(m, 0)
    prob, _, _ = nc.build("ur5e_c2", nm, B)
    home = m.key_qpos[0]
    rng = np.random.default_rng(seed)
    q0 = np.tile(home, (B, 1)) + rng.normal(scale=0.05, size=(B, m.nq))
    tg = _taps_along(prob, _line(nm, q0, T, rng, 0.05), home[None, :], ["frame_pose"])["frame_pose"][:, :, 0]
    prob.close(); nm.close()
    return q0, np.ascontiguousarray(tg)


def test_result_does_not_depend_on_chunks_or_shards(nat):
    import mink_amd as mink
    B, T = 256, 4                                  # whole, chunks of 64 and shards of 128: all on the row kernel's loop
    q0, tg = _ur5e_line_targets(nat, B, T)
    kw = dict(n_steps=20, damping=1e-3, pos_threshold=1e-4, ori_threshold=1e-4, waypoint_dt=0.05, update=False)

    def run(device=0, **extra):
        m, cfg, task, post, lims = _ur5e_api(B, q0, device)
        return cfg, mink.solve_ik_trajectory(cfg, [task, post], 2e-2, {task: tg}, limits=lims, **kw, **extra)

    cfg, whole = run()
    k = list(cfg._problems.values())[-1].last_kernel()
    assert k == "ik_quad_kernel_loop" and 0 < whole.converged.sum() < whole.converged.size
    cfg_c, chunked = run(max_instances=64)
    prob_c = list(cfg_c._problems.values())[-1]
    assert prob_c.max_batch == 64 and prob_c.last_kernel() == k
    _same(chunked, whole, "max_instances=64")
    cfg_s, sharded = run(device=[0, 0])
    shards = list(cfg_s._problems.values())[-1].shards            # (the cached ShardedProblem's handles, one per listed device)
    assert len(shards) == 2 and all(p.max_batch == 128 and p.last_kernel() == k for p in shards)
    _same(sharded, whole, "device=[0, 0]")


# ------------------------------------------------------------------ 6. warm start
def test_warm_started_trajectory_gives_the_cold_answers(nat):
    """tests/test_gpu_steps.py::test_warm_start_across_calls_gives_the_cold_answers per waypoint, from the warm run's own q."""
    model = workloads.load_robot("g1")
    nm = nat.NativeModel(model)
    B, T = 64, 8
    prob, dt, damping = nc.build("g1_c3", nm, B)
    cold, _, _ = nc.build("g1_c3", nm, B)
    stand = model.key_qpos[0]
    rng = np.random.default_rng(8)
    q0, _ = workloads.make_batch(model, nm, prob, rng, B, base_q=stand)
    delta = rng.normal(scale=0.1, size=(B, model.nv))
    line = np.stack([nm.integrate(q0, delta * ((t + 1) / T), 1.0) for t in range(T)])
    tg = _taps_along(prob, line, stand[None, :], ["frame_pose"])["frame_pose"]
    warm = prob.solve_trajectory(q0, tg, stand[None, :], None, dt, damping, n_steps=1, warm_start=True)      # tracking mode
    assert (warm.status & ~1 == 0).all()
    worst = 0.0
    for t in range(T):
        vc, stc = cold.solve(q0 if t == 0 else warm.q[:, t - 1], np.ascontiguousarray(tg[:, t]), stand[None, :], None, dt, damping)
        assert (stc & ~1 == 0).all()
        worst = max(worst, np.abs(warm.v[:, t] - vc).max() / max(1.0, np.abs(vc).max()))
        np.testing.assert_allclose(warm.q[:, t], nm.integrate(q0 if t == 0 else warm.q[:, t - 1], warm.v[:, t], dt), rtol=0, atol=1e-12)
    print("trajectory of %d warm-started waypoints vs cold solves: max rel |dv| = %.2e" % (T, worst))
    assert worst < 1e-9
    prob.close(); cold.close(); nm.close()


# ------------------------------------------------------------------ 7. public API
def test_public_api(nat):
    import mink_amd as mink
    w = _workload(nat, "ur5e_c2")
    B, T = w.B, w.T
    m, cfg, task, post, lims = _ur5e_api(B, w.q)
    start = cfg.q_batch.copy()
    kw = dict(n_steps=w.iters, damping=w.damping, limits=lims, pos_threshold=w.until[0], ori_threshold=w.until[1])
    res = mink.solve_ik_trajectory(cfg, [task, post], w.dt, {task: w.tg[:, :, 0]}, waypoint_dt=0.05, update=False, **kw)
    assert isinstance(res, mink.TrajectoryResult)
    np.testing.assert_array_equal(cfg.q_batch, start)                     # update=False leaves the configuration alone
    assert res.q.shape == (B, T, m.nq) and res.v.shape == (B, T, m.nv) and res.qvel.shape == (B, T, m.nv)
    for f in ("status", "iters", "converged"):
        assert getattr(res, f).shape == (B, T), f
    assert res.converged.dtype == bool
    # the native call on the same handle, and test 1's loop on the bench descriptors of the same tasks
    prob = list(cfg._problems.values())[-1]
    home = m.key_qpos[m.name2id("key", "home")]
    native = prob.solve_trajectory(w.q, w.tg, home[None, :], None, w.dt, w.damping, n_steps=w.iters, until=w.until, qvel_dt=0.05)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(res, f), getattr(native, f), err_msg=f)
    want, _ = _callers_loop(w, w.until)
    np.testing.assert_array_equal(res.q, want.q); np.testing.assert_array_equal(res.iters, want.iters)
    np.testing.assert_array_equal(res.qvel, ref.qvel(m, w.q, res.q, 0.05))             # hinges only: exact
    # an instance whose last waypoint is out of reach: not converged there, no exception, its earlier waypoints and the other
    # instances intact
    b = int(np.flatnonzero(res.converged.all(axis=1))[0])
    far = w.tg[:, :, 0].copy(); far[b, -1, 4:] = [5.0, 5.0, 5.0]
    un = mink.solve_ik_trajectory(cfg, [task, post], w.dt, {task: far}, update=False, **kw)
    assert not un.converged[b, -1] and un.iters[b, -1] == w.iters
    np.testing.assert_array_equal(un.q[b, :-1], res.q[b, :-1]); np.testing.assert_array_equal(un.converged[b, :-1], res.converged[b, :-1])
    others = np.arange(B) != b
    np.testing.assert_array_equal(un.q[others], res.q[others]); np.testing.assert_array_equal(un.converged[others], res.converged[others])
    plain = mink.solve_ik_trajectory(cfg, [task, post], w.dt, {task: w.tg[:, :, 0]}, **kw)
    assert plain.qvel is None
    np.testing.assert_array_equal(plain.q, res.q)
    np.testing.assert_array_equal(cfg.q_batch, res.q[:, -1])              # update=True: the configuration is left at q[:, -1]
    # fixed count: no iters / converged; a (T, 7) sequence is every instance's; a posture sequence beside a held frame target
    cfg.update(start)
    fx = mink.solve_ik_trajectory(cfg, [task, post], w.dt, {task: w.tg[0, :, 0]}, n_steps=3, damping=w.damping, limits=lims, update=False)
    assert fx.iters is None and fx.converged is None and fx.q.shape == (B, T, m.nq)
    ev = mink.solve_ik_trajectory(cfg, [task, post], w.dt, {task: np.repeat(w.tg[:1, :, 0], B, axis=0)}, n_steps=3, damping=w.damping,
                                  limits=lims, update=False)
    np.testing.assert_array_equal(fx.q, ev.q)
    task.set_target(mink.SE3(w.tg[:, 0, 0]))
    ps = mink.solve_ik_trajectory(cfg, [task, post], w.dt, {post: np.repeat(home[None, :], T, axis=0)}, n_steps=3, damping=w.damping,
                                  limits=lims, update=False)
    hd = mink.solve_ik_trajectory(cfg, [task, post], w.dt, {task: np.repeat(w.tg[:, :1, 0], T, axis=1)}, n_steps=3, damping=w.damping,
                                  limits=lims, update=False)
    np.testing.assert_array_equal(ps.q, hd.q)
    # unbatched configuration: unbatched fields
    c1 = mink.Configuration(m, start[0])
    r1 = mink.solve_ik_trajectory(c1, [task, post], w.dt, {task: w.tg[0, :, 0]}, waypoint_dt=0.05, **kw)
    assert r1.q.shape == (T, m.nq) and r1.converged.shape == (T,) and r1.qvel.shape == (T, m.nv)
    np.testing.assert_array_equal(r1.q, res.q[0]); np.testing.assert_array_equal(c1.q, res.q[0, -1])

    # caller-defined tasks: the refusal of solve_ik_steps
    class Mine(mink.Task):
        def compute_error(self, configuration):
            return np.zeros((configuration.batch_size, 3))

        def compute_jacobian(self, configuration):
            return np.zeros((configuration.batch_size, 3, configuration.nv))

    with pytest.raises(mink.TaskDefinitionError, match="caller-defined Task / Limit"):
        mink.solve_ik_trajectory(cfg, [task, post, Mine(cost=np.ones(3))], w.dt, {task: w.tg[:, :, 0]}, **kw)
    # a QP failure names its (instance, waypoint): instance 2 starts outside its limits under a velocity limit it cannot meet
    bad = start.copy(); bad[2, 0] = 7.0
    cfg.update(bad)
    tight = [mink.ConfigurationLimit(m), mink.VelocityLimit(m, {"shoulder_pan": 1e-3})]
    with pytest.raises(mink.SolverError, match=r"\(instance, waypoint\) = \(2, 0\)"):
        mink.solve_ik_trajectory(cfg, [task, post], w.dt, {task: w.tg[:, :, 0]}, n_steps=3, damping=w.damping, limits=tight)
    np.testing.assert_array_equal(cfg.q_batch, bad)                       # a failed call does not move the configuration


# ------------------------------------------------------------------ 8. refusals that need a handle
def test_refusals_of_the_native_call(nat):
    import ctypes
    w = _workload(nat, "ur5e_c2")
    with pytest.raises(nat.MinkHipError, match="exceeds max_batch"):
        w.prob.solve_trajectory(np.repeat(w.q, 2, axis=0), np.repeat(w.tg, 2, axis=0), w.pt, None, w.dt, w.damping)
    L = nat.lib()
    buf = np.zeros((2 * w.B, w.T, 8))
    io = nat.MkhTrajectoryIO()
    io.q_traj, io.v_traj, io.status = buf.ctypes.data, buf.ctypes.data, buf.ctypes.data
    rc = L.mkh_solve_trajectory(w.prob.handle, 2 * w.B, w.T, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, w.dt, w.damping,
                                3, -1.0, -1.0, ctypes.byref(io), 0, None)
    assert rc == -1 and b"exceeds max_batch" in L.mkh_last_error()
    # threshold mode needs a frame task to test the thresholds on
    only_posture = nat.NativeProblem(w.nm, posture_tasks=[{"cost": 1.0}], max_batch=4)
    rc = L.mkh_solve_trajectory(only_posture.handle, 4, 2, buf.ctypes.data, None, buf.ctypes.data, None, w.dt, w.damping, 3, 1e-3, 1e-3,
                                ctypes.byref(io), 0, None)
    assert rc == -1 and b"at least one frame task" in L.mkh_last_error()
    with pytest.raises(ValueError, match="at least one frame task"):
        only_posture.solve_trajectory(w.q[:4], None, np.repeat(w.pt[None], 2, axis=0), None, w.dt, w.damping, until=(1e-3, 1e-3))
    only_posture.close()
