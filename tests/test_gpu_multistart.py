"""Multi-start IK on the device (mkh_solve_multistart / mink_amd.solve_ik_multistart): the seeds are the header's rule, the loop
is mkh_solve_until's on the fanned-out instances — bitwise —, the selection is the stated rule, the result does not depend on
chunking, sharding or the kind of array passed in, and it finds solutions a single start misses."""

import os

import numpy as np
import pytest

import multistart_ref as ref
import oracle_configs as oc
from mink_amd import workloads
from oracle import ik as oik

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _mjcf(name):
    import mink_amd
    return mink_amd.load_mjcf(os.path.join(GOLDEN, name + ".xml"))


def _start(m, B, rng, base=None):
    q = np.tile(np.asarray(m.qpos0 if base is None else base, dtype=np.float64), (B, 1))
    for j in range(m.njnt):
        if m.jnt_type[j] in (ref.JNT_SLIDE, ref.JNT_HINGE):
            q[:, int(m.jnt_qposadr[j])] += rng.normal(scale=0.05, size=B)
    return q


# ------------------------------------------------------------------ 1. seeds
@pytest.mark.parametrize("name", ["ur5e", "g1", "shadow_left", "ballslide", "balllimit"])
def test_device_seeds_are_the_stated_rule(nat, name):
    """Hinge / slide entries are EXACT: the seed kernel is compiled with floating-point contraction off, so lo + width·u is a
    rounded product and a rounded sum like numpy's.  Ball quaternions agree to 1e-15 (sin / cos of the two libraries)."""
    m = _mjcf(name) if name.startswith("ball") else workloads.load_robot(name)
    nm = nat.NativeModel(m, 0)
    B, S = 37, 16
    rng = np.random.default_rng(2)
    base = m.key_qpos[0] if len(m.key_qpos) else None
    q = _start(m, B, rng, base)
    prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "body", "frame_id": m.nbody - 1, "cost": [1.0] * 6}], max_batch=B * S)
    tg = np.zeros((B, 1, 7)); tg[:, :, 0] = 1.0
    for rng_seed, t0 in ((0, 0), (2 ** 40 + 12345, 1000003)):
        out = prob.solve_multistart(q, tg, None, None, 1.0, 1e-3, n_seeds=S, max_iters=1, pos_threshold=1e-4, ori_threshold=1e-4,
                                    rng_seed=rng_seed, target_index0=t0, return_all=True)
        want = ref.draw_seeds(m, q, S, rng_seed=rng_seed, target_index0=t0)
        got = out.seeds
        assert got.shape == (B, S, m.nq)
        assert np.array_equal(got[:, 0], q)                                     # seed 0: bitwise the caller's q
        n_ball = 0
        for j in range(m.njnt):
            jt, a = int(m.jnt_type[j]), int(m.jnt_qposadr[j])
            if jt == ref.JNT_BALL:
                n_ball += 1
                err = np.abs(got[:, :, a:a + 4] - want[:, :, a:a + 4]).max()
                print(f"{name} ball joint {j}: max |device - numpy| = {err:.3e}")
                assert err <= 1e-15
                assert np.abs(np.linalg.norm(got[:, :, a:a + 4], axis=-1) - 1.0).max() < 4e-16
            elif jt == ref.JNT_FREE:
                assert np.array_equal(got[:, :, a:a + 7], np.repeat(q[:, None, a:a + 7], S, axis=1))   # the base stays
            else:
                assert np.array_equal(got[:, :, a], want[:, :, a]), (name, j)
        assert n_ball == sum(1 for j in range(m.njnt) if m.jnt_type[j] == ref.JNT_BALL)
    prob.close(); nm.close()


# ------------------------------------------------------------------ 2. composition
# B, S, position / orientation thresholds, max_iters (the velocity limits of these set-ups allow ~0.01 rad per step)
_WORKLOADS = {"ur5e_c2": (48, 8, 1e-3, 1e-2, 60), "g1_c3": (24, 4, 2e-2, 5e-2, 60), "h1_full": (24, 4, 2e-2, 5e-2, 60),
              "shadow_c4": (24, 8, 2e-3, 1.0, 60)}


def _workload(nat, name, seed=9):
    B, S, pth, oth, iters = _WORKLOADS[name]
    m = workloads.load_bench_robot(name)
    nm = nat.NativeModel(m, 0)
    prob, dt, damping = workloads.bench_config(name, m, nm, B * S)
    q, tg, pt, ct = workloads.bench_batch(name, m, nm, prob, np.random.default_rng(seed), B)
    return m, nm, prob, (q, tg, pt, ct), dt, damping, (B, S, pth, oth, iters)


def _rep(x, per, S):
    return None if x is None else (np.repeat(x, S, axis=0) if x.ndim == per + 1 else x)


@pytest.mark.parametrize("name", list(_WORKLOADS))
def test_loop_is_the_existing_loop_bitwise(nat, name):
    """The per-instance results are those of the threshold loop run on the device's own seeds with the targets repeated on the
    host: same kernel, same inputs — a difference is a bug in the fan-out."""
    m, nm, prob, (q, tg, pt, ct), dt, damping, (B, S, pth, oth, iters) = _workload(nat, name)
    if name == "h1_full":
        assert ct is not None and ct.shape == (B, 1, 3)                     # per-instance CoM targets: fanned out too
    out = prob.solve_multistart(q, tg, pt, ct, dt, damping, n_seeds=S, max_iters=iters, pos_threshold=pth, ori_threshold=oth,
                                rng_seed=4, return_all=True)
    k_multi = prob.last_kernel()
    seeds = out.seeds.reshape(B * S, m.nq)
    qn, vn, st, it, cv = prob.solve(seeds, _rep(tg, 2, S), _rep(pt, 2, S), _rep(ct, 2, S), dt, damping, n_steps=iters,
                                    until=(pth, oth))
    print(f"{name}: kernel {k_multi}, {int(cv.sum())} of {B * S} instances converged, {int(((st & ~1) != 0).sum())} failed, "
          f"{int(out.converged.sum())} of {B} targets")
    assert k_multi and prob.last_kernel() == k_multi
    np.testing.assert_array_equal(out.q_all.reshape(B * S, m.nq), qn)
    np.testing.assert_array_equal(out.iters_all.reshape(-1), it)
    np.testing.assert_array_equal(out.converged_all.reshape(-1), cv)
    np.testing.assert_array_equal(out.status_all.reshape(-1), st)
    # the chosen rows are rows of that loop
    pick = np.arange(B) * S + out.seed_index
    np.testing.assert_array_equal(out.q, qn[pick]); np.testing.assert_array_equal(out.v, vn[pick])
    np.testing.assert_array_equal(out.iters, it[pick]); np.testing.assert_array_equal(out.status, st[pick])
    prob.close(); nm.close()


def test_public_call_is_solve_ik_steps_on_the_same_seeds(nat):
    """The same through the public API on UR5e: solve_ik_steps on Configuration(model, seeds) with the targets repeated."""
    import mink_amd as mink
    m, cfg, tasks, lims, tg = _far_ur5e(64)
    S = 8
    res = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, rng_seed=3, update=False,
                                   return_all=True)
    k = list(cfg._problems.values())[-1].last_kernel()
    cfg2 = mink.Configuration(m, res.seeds.reshape(64 * S, m.nq))
    tasks[0].set_target(mink.SE3(np.repeat(tg, S, axis=0)))
    q2, v2, it2, cv2 = mink.solve_ik_steps(cfg2, tasks, 1.0, 40, damping=1e-3, limits=lims, pos_threshold=1e-4, ori_threshold=1e-4)
    assert list(cfg2._problems.values())[-1].last_kernel() == k
    np.testing.assert_array_equal(res.q_all.reshape(-1, m.nq), q2)
    np.testing.assert_array_equal(res.iters_all.reshape(-1), it2)
    np.testing.assert_array_equal(res.converged_all.reshape(-1), cv2)


# ------------------------------------------------------------------ 3. selection
def _check_selection(m, out, q_ref, weights=None):
    B, S = out.q_all.shape[:2]
    n_none = 0
    for b in range(B):
        d = np.array([ref.distance(m, out.q_all[b, s], q_ref[b], weights) for s in range(S)])
        ok = ref.eligible(out.converged_all[b], out.status_all[b])
        assert int(out.n_converged[b]) == int(ok.sum())
        s = int(out.seed_index[b])
        if not ok.any():
            n_none += 1
            assert s == 0 and not out.converged[b]
            assert np.array_equal(out.q[b], out.q_all[b, 0])                 # seed 0's row, bitwise
            continue
        assert out.converged[b] and ok[s]                                    # converged and failure-free
        dmin = d[ok].min()
        assert d[s] <= dmin * (1 + 1e-9) + 1e-12, (b, s, d[s], dmin)
        assert np.array_equal(out.q[b], out.q_all[b, s])
        if (np.sort(d[ok])[1:2] > dmin * (1 + 1e-9) + 1e-12).all():             # (no near-tie: exactly numpy's choice)
            assert s == ref.select(d, out.converged_all[b], out.status_all[b])[0]
    return n_none


def test_selection_is_the_stated_rule(nat):
    for name in ("ur5e_far", "shadow_c4", "ballslide"):
        if name == "ur5e_far":
            m = workloads.load_robot("ur5e")
            nm = nat.NativeModel(m, 0)
            B, S, iters, pth, oth, dt, damping = 96, 16, 40, 1e-4, 1e-4, 1.0, 1e-3
            from mink_amd.api_specs import configuration_limit_desc
            prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "attachment_site"),
                                                       "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 1.0}],
                                     configuration_limits=[configuration_limit_desc(m)], max_batch=B * S)
            q = np.tile(m.key_qpos[0], (B, 1))
            tg = _far_targets(m, B)[:, None, :]
            pt = ct = None
        elif name == "ballslide":                     # ball joints: the quaternion branch of the tangent-space difference
            import mink_amd as mink
            from mink_amd.api_specs import configuration_limit_desc
            m = _mjcf("ballslide")
            nm = nat.NativeModel(m, 0)
            B, S, iters, pth, oth, dt, damping = 32, 16, 40, 1e-3, 1e-2, 1.0, 1e-3
            prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "tip"),
                                                       "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 0.1}],
                                     configuration_limits=[configuration_limit_desc(m)], max_batch=B * S)
            q = _start(m, B, np.random.default_rng(4))
            goal = ref.draw_seeds(m, q, 2, rng_seed=77)[:, 1]
            tg = mink.Configuration(m, goal).get_transform_frame_to_world("tip", "site").wxyz_xyz[:, None, :]
            pt = ct = None
        else:
            m, nm, prob, (q, tg, pt, ct), dt, damping, (B, S, pth, oth, iters) = _workload(nat, name)
        kw = dict(n_seeds=S, max_iters=iters, pos_threshold=pth, ori_threshold=oth, rng_seed=8, return_all=True)
        out = prob.solve_multistart(q, tg, pt, ct, dt, damping, **kw)
        n_none = _check_selection(m, out, q)
        failed = int(((out.status_all & ~1) != 0).sum())
        print(f"{name}: {int(out.converged.sum())} of {B} targets converged, {n_none} with no converged seed, "
              f"{failed} failed instances, seed_index histogram {np.bincount(out.seed_index, minlength=S).tolist()}")
        if name == "ur5e_far":
            assert 0 < n_none < B and (out.n_converged > 1).sum() > B // 4   # both branches of the rule are exercised
        # reference= and weights= change the choice as numpy says
        rng = np.random.default_rng(1)
        q_ref = out.q_all[np.arange(B), rng.integers(0, S, size=B)].copy()
        w = rng.uniform(0.1, 10.0, size=m.nv)
        out_r = prob.solve_multistart(q, tg, pt, ct, dt, damping, reference=q_ref, weights=w, **kw)
        np.testing.assert_array_equal(out_r.q_all, out.q_all)                # (the loops do not know about the selection)
        _check_selection(m, out_r, q_ref, w)
        if name == "ur5e_far":
            assert (out_r.seed_index != out.seed_index).sum() > 0
        prob.close(); nm.close()


# ------------------------------------------------------------------ fixtures of 4, 5, 6
def _far_targets(m, B, seed=20261016):
    """End-effector poses of configurations drawn uniformly in the joint ranges (clipped to ±π): far from `home`.  CPU check of
    this fixture (seed 20261016, B = 1024, the C oracle's solve + the numpy oracle's error test, 40 iterations from `home`,
    thresholds 1e-4 / 1e-4): single start converges 635 of 1024 — 38 % unconverged, above the 5 % the test needs.  (The device
    gives the same 635, and 992 with 16 seeds: profiles/r08_multistart.txt.)"""
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(m.jnt_range[:, 0], -np.pi), np.minimum(m.jnt_range[:, 1], np.pi)
    q_goal = rng.uniform(lo, hi, size=(B, m.nq))
    import mink_amd as mink
    return mink.Configuration(m, q_goal).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz


def _far_ur5e(B, device=0):
    """The set-up of the issue: UR5e, one FrameTask on attachment_site (costs 1 / 1, lm_damping 1), ConfigurationLimit, every
    loop started at `home`; callers use dt = 1, damping = 1e-3, thresholds 1e-4 / 1e-4, 40 iterations."""
    import mink_amd as mink
    m = workloads.load_robot("ur5e")
    tg = _far_targets(m, B)
    cfg = mink.Configuration(m, np.tile(m.key_qpos[m.name2id("key", "home")], (B, 1)), device=device)
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    task.set_target(mink.SE3(tg))
    return m, cfg, [task], [mink.ConfigurationLimit(m)], tg


_KW = dict(damping=1e-3, rng_seed=5, update=False, return_all=True)


# ------------------------------------------------------------------ 4. independence
def test_result_does_not_depend_on_chunks_shards_or_array_kind(nat):
    import mink_amd as mink
    import torch
    B, S = 256, 16                               # 4 096 instances, chunks of 1 024, shards of 2 048: all on the row kernel's loop
    m, cfg, tasks, lims, tg = _far_ur5e(B)
    whole = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, limits=lims, **_KW)
    k = list(cfg._problems.values())[-1].last_kernel()
    assert 0 < whole.converged.sum() and (whole.seed_index > 0).sum() > 0

    def same(other, what):
        for f in ("q", "seed_index", "converged", "n_converged", "seeds", "q_all"):
            np.testing.assert_array_equal(getattr(other, f), getattr(whole, f), err_msg=f"{what}: {f}")

    _, cfg_c, tasks_c, lims_c, _ = _far_ur5e(B)
    chunked = mink.solve_ik_multistart(cfg_c, tasks_c, 1.0, S, 40, 1e-4, 1e-4, limits=lims_c, max_instances=1024, **_KW)
    prob_c = list(cfg_c._problems.values())[-1]
    assert prob_c.max_batch == 1024 and prob_c.last_kernel() == k
    same(chunked, "max_instances=1024")
    _, cfg_s, tasks_s, lims_s, _ = _far_ur5e(B, device=[0, 0])
    sharded = mink.solve_ik_multistart(cfg_s, tasks_s, 1.0, S, 40, 1e-4, 1e-4, limits=lims_s, **_KW)
    shards = list(cfg_s._problems.values())[-1].shards            # (the cached ShardedProblem's handles, one per listed device)
    assert len(shards) == 2 and all(p.max_batch == 2048 and p.last_kernel() == k for p in shards)
    same(sharded, "device=[0, 0]")
    # numpy against torch inputs, one level down (a Configuration holds its q on the host)
    prob = list(cfg._problems.values())[-1]
    q = cfg.q_batch
    args = dict(n_seeds=S, max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, rng_seed=5, return_all=True)
    o_np = prob.solve_multistart(q, tg[:, None, :], None, None, 1.0, 1e-3, **args)
    dev = torch.device("cuda:0")
    o_t = prob.solve_multistart(torch.as_tensor(q, device=dev), torch.as_tensor(np.ascontiguousarray(tg[:, None, :]), device=dev),
                                None, None, 1.0, 1e-3, **args)
    assert prob.last_kernel() == k
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in o_t)
    for f in o_np._fields:
        np.testing.assert_array_equal(getattr(o_t, f).cpu().numpy(), getattr(o_np, f), err_msg=f"torch: {f}")
    np.testing.assert_array_equal(o_np.q, whole.q); np.testing.assert_array_equal(o_np.seed_index, whole.seed_index)
    # user seeds and a reference as device tensors
    sd = torch.as_tensor(whole.seeds, device=dev)
    o_u = prob.solve_multistart(torch.as_tensor(q, device=dev), torch.as_tensor(np.ascontiguousarray(tg[:, None, :]), device=dev),
                                None, None, 1.0, 1e-3, seeds=sd, **{**args, "rng_seed": 99})
    np.testing.assert_array_equal(o_u.q.cpu().numpy(), whole.q)


# ------------------------------------------------------------------ 5. it finds what single start misses
def test_multistart_converges_targets_single_start_misses(nat):
    import mink_amd as mink
    B, S = 1024, 16
    m, cfg, tasks, lims, tg = _far_ur5e(B)
    q1, v1, it1, cv1 = mink.solve_ik_steps(cfg, tasks, 1.0, 40, damping=1e-3, limits=lims, update=False, pos_threshold=1e-4,
                                           ori_threshold=1e-4)
    res = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, rng_seed=0, update=False)
    print(f"UR5e, {B} far targets from home: single start converged {int(cv1.sum())}, multi-start ({S} seeds) {int(res.converged.sum())}")
    assert cv1.sum() <= 0.95 * B                                         # (the fixture's condition, as the GPU sees it)
    # (a) seed 0 is the single start: nothing it converged is lost
    assert res.converged[cv1].all()
    # (b) every returned converged q is a solution by the CPU oracle's kinematics, inside the joint ranges
    mo = oc.model("ur5e")
    sid = mo.name2id("site", "attachment_site")
    worst_p = worst_o = 0.0
    for b in np.flatnonzero(res.converged):
        c = oik.Configuration(mo, res.q[b])
        e, _ = oik.task_error_jacobian(c, oik.FrameTaskSpec(sid, "site", np.ones(6), tg[b], lm_damping=1.0))
        worst_p, worst_o = max(worst_p, float(np.linalg.norm(e[:3]))), max(worst_o, float(np.linalg.norm(e[3:])))
        assert np.linalg.norm(e[:3]) <= 1e-4 + 1e-9 and np.linalg.norm(e[3:]) <= 1e-4 + 1e-9, (b, e)
        assert c.limit_violations(1e-6) == [], b
    print(f"worst error norms of the converged results by the oracle: position {worst_p:.3e}, orientation {worst_o:.3e}")
    # (c) strictly more targets
    assert res.converged.sum() > cv1.sum()
    # what did not converge is seed 0's result: the single start's
    none = ~res.converged
    assert (res.seed_index[none] == 0).all()
    np.testing.assert_array_equal(res.q[none], q1[none])


# ------------------------------------------------------------------ 6. API
def test_public_api(nat):
    import mink_amd as mink
    B, S = 32, 6
    m, cfg, tasks, lims, tg = _far_ur5e(B)
    home = cfg.q_batch.copy()
    res = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, update=False, return_all=True)
    assert isinstance(res, mink.MultistartResult)
    np.testing.assert_array_equal(cfg.q_batch, home)                      # update=False leaves the configuration alone
    assert res.q.shape == (B, m.nq) and res.v.shape == (B, m.nv) and res.q_all.shape == (B, S, m.nq) and res.seeds.shape == (B, S, m.nq)
    for f in ("converged", "seed_index", "n_converged", "iters", "status"):
        assert getattr(res, f).shape == (B,), f
    for f in ("converged_all", "iters_all", "status_all"):
        assert getattr(res, f).shape == (B, S), f
    assert res.converged.dtype == bool and res.converged_all.dtype == bool
    plain = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims)
    assert plain.q_all is None and plain.seeds is None
    np.testing.assert_array_equal(plain.q, res.q)
    np.testing.assert_array_equal(cfg.q_batch, res.q)                     # update=True: the configuration takes q
    # user seeds, both shapes; row 0 is still the caller's q
    cfg.update(home)
    own = res.seeds.copy(); own[:, 0] = 123.0
    u = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, seeds=own, update=False, return_all=True)
    np.testing.assert_array_equal(u.seeds, res.seeds); np.testing.assert_array_equal(u.q, res.q)
    one = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, seeds=own[3], update=False, return_all=True)
    np.testing.assert_array_equal(one.seeds[:, 1:], np.repeat(res.seeds[3:4, 1:], B, axis=0))
    np.testing.assert_array_equal(one.seeds[:, 0], home)
    np.testing.assert_array_equal(one.q[3], res.q[3])
    # n_seeds = 1 is solve_ik_steps
    q1, v1, it1, cv1 = mink.solve_ik_steps(cfg, tasks, 1.0, 40, damping=1e-3, limits=lims, update=False, pos_threshold=1e-4, ori_threshold=1e-4)
    s1 = mink.solve_ik_multistart(cfg, tasks, 1.0, 1, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, update=False)
    np.testing.assert_array_equal(s1.q, q1); np.testing.assert_array_equal(s1.converged, cv1); np.testing.assert_array_equal(s1.iters, it1)
    # unbatched configuration: unbatched fields
    c1 = mink.Configuration(m, home[0])
    t1 = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0); t1.set_target(mink.SE3(tg[3]))
    r1 = mink.solve_ik_multistart(c1, [t1], 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, return_all=True)
    assert r1.q.shape == (m.nq,) and r1.v.shape == (m.nv,) and r1.q_all.shape == (S, m.nq) and r1.converged_all.shape == (S,)
    assert np.ndim(r1.converged) == 0 and np.ndim(r1.seed_index) == 0
    np.testing.assert_array_equal(c1.q, r1.q)
    # caller-defined tasks: the refusal of solve_ik_steps

    class Mine(mink.Task):
        def compute_error(self, configuration):
            return np.zeros((configuration.batch_size, 3))

        def compute_jacobian(self, configuration):
            return np.zeros((configuration.batch_size, 3, configuration.nv))

    with pytest.raises(mink.TaskDefinitionError, match="caller-defined Task / Limit"):
        mink.solve_ik_multistart(cfg, tasks + [Mine(cost=np.ones(3))], 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims)
    # an unreachable pose: not converged, seed 0, no exception
    far = tg.copy(); far[0, 4:] = [5.0, 5.0, 5.0]
    tasks[0].set_target(mink.SE3(far))
    cfg.update(home)
    un = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, update=False, return_all=True)
    assert not un.converged[0] and un.seed_index[0] == 0 and un.n_converged[0] == 0
    np.testing.assert_array_equal(un.q[0], un.q_all[0, 0])
    np.testing.assert_array_equal(un.q[1:], res.q[1:])                   # (the other targets do not notice)
    # the handle is sized for B·S; a native call beyond it is refused
    prob = list(cfg._problems.values())[-1]
    with pytest.raises(nat.MinkHipError, match="exceeds max_batch"):
        prob.solve_multistart(home, far[:, None, :], None, None, 1.0, 1e-3, n_seeds=S + 1, max_iters=5, pos_threshold=1e-4,
                              ori_threshold=1e-4)
