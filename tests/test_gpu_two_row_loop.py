"""The fused caller loop (mkh_solve_steps / mkh_solve_until) on the two-row build of the row kernel (quad_kernel.h,
`ik_quad_kernel<32, true, 32>`): 17 … 32 dofs or links, a floating base whose quaternion the kernel carries from step to step.
Against the host-driven loop of single solves + integrate, the wavefront kernel's fused loop (MKH_FLAG_WAVE_KERNEL), the
numpy oracle's loop and the real mink's closed loop (tests/golden/make_golden_loop.py).  The default dispatch takes the two-row loop
where it measured faster (ComTask / RelativeFrameTask problems, robots without a floating base); `quad_kernel=True`
(MKH_FLAG_QUAD_KERNEL) forces it for the others, which is how the H1 / Go1 task sets without a ComTask reach it here."""

import os

import numpy as np
import pytest

import oracle_configs as oc
from mink_amd import workloads
from mink_amd.flatmodel import FlatModel
from oracle import ik as oik

pytestmark = pytest.mark.gpu
LOOP = "ik_quad_kernel_32_loop"


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _h1(nat, name, B, seed=5, sigma=0.15):
    m = workloads.load_robot("h1")
    nm = nat.NativeModel(m)
    prob, dt, damping = workloads.bench_config(name, m, nm, B)
    stand = m.key_qpos[m.name2id("key", "stand")]
    q, tg = workloads.make_batch(m, nm, prob, np.random.default_rng(seed), B, base_q=stand, sigma=sigma)
    return m, nm, prob, dt, damping, stand, q, tg


def _h1_oracle_tasks(m, tg_i, stand):
    site = lambda s: m.name2id("site", s)
    c6 = lambda p, o: np.array([p] * 3 + [o] * 3, dtype=np.float64)
    fts = [oik.FrameTaskSpec(site(s), "site", c6(200.0, o), tg_i[k], lm_damping=1.0)
           for k, (s, o) in enumerate((("left_foot", 10.0), ("right_foot", 10.0), ("left_wrist", 0.0), ("right_wrist", 0.0)))]
    hinge = [int(m.jnt_dofadr[j]) for j in range(m.njnt) if m.jnt_type[j] != 0]
    lims = [oik.ConfigurationLimitSpec(), oik.VelocityLimitSpec(np.array(hinge), np.full(len(hinge), np.pi))]
    return fts + [oik.PostureTaskSpec(np.full(m.nv, 1.0), stand)], lims


def _quat_norms(m, q):
    free = [int(m.jnt_qposadr[j]) + 3 for j in range(m.njnt) if m.jnt_type[j] == 0]
    return np.concatenate([np.linalg.norm(q[:, a:a + 4], axis=1) for a in free])


def _same_loop(got, ref, q_tol=1e-10, v_tol=1e-7):
    np.testing.assert_array_equal(got[2], ref[2])                                    # status
    ok = (got[2] & 14) == 0
    np.testing.assert_allclose(got[0][ok], ref[0][ok], rtol=0, atol=q_tol)
    np.testing.assert_allclose(got[1][ok], ref[1][ok], rtol=0, atol=v_tol * max(1.0, np.abs(ref[1][ok]).max()))
    if len(got) > 3:
        np.testing.assert_array_equal(got[3], ref[3]); np.testing.assert_array_equal(got[4], ref[4])


def test_dispatch_and_the_fixed_loop(nat):
    m, nm, prob, dt, damping, stand, q0, tg = _h1(nat, "h1_c3", 64)
    K = 6
    qK, vK, st = prob.solve(q0, tg, stand[None, :], None, dt, damping, n_steps=K, quad_kernel=True)
    assert prob.last_kernel() == LOOP, prob.last_kernel()
    assert (st & ~1 == 0).all()
    # (a) the host-driven loop: single solves (the two-row single-solve build) + mkh_integrate
    q = q0.copy()
    for _ in range(K):
        v, _ = prob.solve(q, tg, stand[None, :], None, dt, damping)
        q = nm.integrate(q, v, dt)
    np.testing.assert_allclose(qK, q, rtol=0, atol=1e-10)
    np.testing.assert_allclose(vK, v, rtol=0, atol=1e-9 * max(1.0, np.abs(v).max()))
    # (b) the wavefront kernel's fused loop
    qw, vw, stw = prob.solve(q0, tg, stand[None, :], None, dt, damping, n_steps=K, wave_kernel=True)
    assert prob.last_kernel().startswith("ik_solve_kernel"), prob.last_kernel()
    np.testing.assert_array_equal(stw, st)
    np.testing.assert_allclose(qK, qw, rtol=0, atol=1e-10)
    np.testing.assert_allclose(vK, vw, rtol=0, atol=1e-9 * max(1.0, np.abs(vw).max()))
    # (c) the oracle's loop on a few instances
    for i in (0, 29, 63):
        cfg = oik.Configuration(m, q0[i])
        tasks, lims = _h1_oracle_tasks(m, tg[i], stand)
        for _ in range(K):
            v_ref = oik.solve_ik(m, cfg, tasks, dt, damping, lims)
            cfg.update(cfg.integrate(v_ref, dt))
        np.testing.assert_allclose(qK[i], cfg.q, rtol=0, atol=1e-10)
        np.testing.assert_allclose(vK[i], v_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(v_ref).max()))
    # the base quaternion stays a unit quaternion
    assert np.abs(_quat_norms(m, qK) - 1.0).max() < 1e-14


def test_real_mink_closed_loop_replay(nat):
    """tests/golden/ik_h1_loop.npz: the real mink's loop of examples/humanoid_h1.py (solve_ik + Configuration.integrate_inplace,
    8 ticks, ComTask with per-instance CoM targets) on 16 instances, through the public API's fused loop."""
    import mink_amd as mink
    d = np.load(os.path.join(oc.GOLDEN, "ik_h1_loop.npz"))
    m = FlatModel.load(os.path.join(oc.GOLDEN, "models", "all", "unitree_h1__scene.json"))
    B, K = d["q"].shape[0], d["v"].shape[1]
    cfg = mink.Configuration(m, d["q"][:, 0])
    fts = [mink.FrameTask("pelvis", "body", position_cost=0.0, orientation_cost=10.0)]
    fts += [mink.FrameTask(s, "site", position_cost=200.0, orientation_cost=10.0, lm_damping=1.0) for s in ("right_foot", "left_foot")]
    fts += [mink.FrameTask(s, "site", position_cost=200.0, orientation_cost=0.0, lm_damping=1.0) for s in ("right_wrist", "left_wrist")]
    for k, t in enumerate(fts):
        t.set_target(mink.SE3(d["frame_targets"][:, k]))
    post = mink.PostureTask(m, cost=1.0); post.set_target(d["posture_target"])
    com = mink.ComTask(cost=200.0); com.set_target(d["com_targets"])
    qf, vl = mink.solve_ik_steps(cfg, fts + [post, com], float(d["dt"]), K, damping=float(d["damping"]),
                                 limits=[mink.ConfigurationLimit(m)])
    assert list(cfg._problems.values())[-1].last_kernel() == LOOP
    print("h1 loop replay: |q - mink| %.1e, |v - mink| %.1e" % (np.abs(qf - d["q"][:, -1]).max(), np.abs(vl - d["v"][:, -1]).max()))
    np.testing.assert_allclose(qf, d["q"][:, -1], rtol=0, atol=1e-9)
    np.testing.assert_allclose(vl, d["v"][:, -1], rtol=0, atol=1e-9 * max(1.0, np.abs(d["v"][:, -1]).max()))
    np.testing.assert_allclose(cfg.q_batch, d["q"][:, -1], rtol=0, atol=1e-9)


def test_threshold_loop(nat):
    """mkh_solve_until: targets at spread distances — some instances converge within 2-3 iterations, some never — against the
    wavefront kernel's threshold loop and the oracle's (examples/arm_ur5e_actuators.py:88-97) per instance."""
    B, max_iters, pos_thr, ori_thr = 64, 20, 1e-3, 1e-2
    m, nm, prob, dt, damping, stand, q0, _ = _h1(nat, "h1_c3", B, seed=21)
    rng = np.random.default_rng(22)
    scale = np.repeat([1e-3, 1e-2, 0.05, 0.3], B // 4)[:, None]
    q_t = nm.integrate(q0, rng.normal(size=(B, m.nv)) * scale, 1.0)
    dummy = np.zeros((B, 4, 7)); dummy[:, :, 0] = 1
    _, _, t = prob.solve(q_t, dummy, stand[None, :], None, 1.0, 1.0, taps=["frame_pose"], solve_qp=False)
    tg = t["frame_pose"]
    kw = {"n_steps": max_iters, "until": (pos_thr, ori_thr)}
    got = prob.solve(q0, tg, stand[None, :], None, dt, damping, quad_kernel=True, **kw)
    assert prob.last_kernel() == LOOP, prob.last_kernel()
    ref = prob.solve(q0, tg, stand[None, :], None, dt, damping, wave_kernel=True, **kw)
    iters, conv = got[3], got[4]
    print("iterations:", np.bincount(iters, minlength=max_iters + 1).tolist(), "converged:", int(conv.sum()), "of", B)
    assert (got[2] & ~1 == 0).all() and conv.sum() >= B // 4 and (conv == 0).sum() >= 4 and len(set(iters[conv == 1].tolist())) >= 3
    _same_loop(got, ref)
    for i in range(0, B, 9):
        cfg = oik.Configuration(m, q0[i])
        tasks, lims = _h1_oracle_tasks(m, tg[i], stand)
        done, n, near = False, 0, False
        for n in range(1, max_iters + 1):
            v_ref = oik.solve_ik(m, cfg, tasks, dt, damping, lims)
            cfg.update(cfg.integrate(v_ref, dt))
            errs = [oik.task_error_jacobian(cfg, tk)[0] for tk in tasks[:4]]
            ep = max(np.linalg.norm(e[:3]) for e in errs); eo = max(np.linalg.norm(e[3:]) for e in errs[:2])
            near |= abs(ep - pos_thr) < 1e-9 * pos_thr or abs(eo - ori_thr) < 1e-9 * ori_thr
            if ep <= pos_thr and eo <= ori_thr:
                done = True
                break
        if near:                                       # (an error within 1e-9 relative of a threshold: rounding decides, excluded)
            continue
        assert (iters[i], bool(conv[i])) == (n, done), (i, iters[i], conv[i], n, done)
        np.testing.assert_allclose(got[0][i], cfg.q, rtol=0, atol=1e-10)
        np.testing.assert_allclose(got[1][i], v_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(v_ref).max()))


def _go1(nat, B):
    m = FlatModel.load(os.path.join(oc.GOLDEN, "models", "all", "unitree_go1__scene.json"))
    nm = nat.NativeModel(m)
    fts = [{"frame_type": "body", "frame_id": m.name2id("body", "trunk"), "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 0.0}]
    fts += [{"frame_type": "site", "frame_id": m.name2id("site", s), "cost": [1.0, 1.0, 1.0, 0.0, 0.0, 0.0], "gain": 1.0, "lm_damping": 0.0}
            for s in ("FL", "FR", "RR", "RL")]
    import native_configs as nc
    prob = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1e-5}], configuration_limits=[nc._cfg_limit(m)], max_batch=B)
    return m, nm, prob, 2e-3, 1e-5, m.key_qpos[m.name2id("key", "home")]


def _shadow(nat, B):
    m = workloads.load_robot("shadow_left")
    nm = nat.NativeModel(m)
    from mink_amd.api_specs import configuration_limit_desc
    fts = [workloads._frame_desc(m, f, "site", 1.0, 0.0, 1.0) for f in workloads.SHADOW_FINGERS]
    prob = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1e-2}], configuration_limits=[configuration_limit_desc(m)], max_batch=B)
    return m, nm, prob, 2e-3, 1e-5, m.key_qpos[m.name2id("key", "grasp hard")]


@pytest.mark.parametrize("robot", ["h1_full", "go1", "shadow"])
def test_breadth_against_the_wavefront_loop(nat, robot):
    B = 96
    if robot == "h1_full":
        m, nm, prob, dt, damping, key, q0, tg = _h1(nat, "h1_full", B, seed=31)
        ct = nm.integrate(q0, np.random.default_rng(32).normal(scale=0.1, size=(B, m.nv)), 1.0)
        _, _, t = prob.solve(ct, tg, key[None, :], np.zeros((B, 1, 3)), 1.0, 1.0, taps=["subtree_com"], solve_qp=False)
        com = t["subtree_com"].reshape(B, 1, 3)
    else:
        m, nm, prob, dt, damping, key = (_go1 if robot == "go1" else _shadow)(nat, B)
        q0, tg = workloads.make_batch(m, nm, prob, np.random.default_rng(33), B, base_q=key)
        com = None
    for kw in ({"n_steps": 5}, {"n_steps": 12, "until": (1e-3, 1e-2)}):
        got = prob.solve(q0, tg, key[None, :], com, dt, damping, quad_kernel=True, **kw)
        assert prob.last_kernel() == LOOP, prob.last_kernel()
        ref = prob.solve(q0, tg, key[None, :], com, dt, damping, wave_kernel=True, **kw)
        assert (got[2] & ~1 == 0).all()
        _same_loop(got, ref)
        if len(got) > 3:
            print(robot, "iterations:", np.bincount(got[3]).tolist(), "converged:", int(got[4].sum()), "of", B)
    if robot == "h1_full":
        assert np.abs(_quat_norms(m, got[0]) - 1.0).max() < 1e-14
    # host-stepped single solves of the same problem (the single-solve two-row build + mkh_integrate)
    q = q0.copy()
    for _ in range(5):
        v, _ = prob.solve(q, tg, key[None, :], com, dt, damping)
        q = nm.integrate(q, v, dt)
    q5 = prob.solve(q0, tg, key[None, :], com, dt, damping, n_steps=5, quad_kernel=True)[0]
    np.testing.assert_allclose(q5, q, rtol=0, atol=1e-10)


@pytest.mark.parametrize("seed", range(4))
def test_random_trees(nat, seed):
    """Random trees with a free root (even seeds) or 17 … 32 hinge / slide dofs, RelativeFrameTasks on seeds 1 and 2: the fused
    loops of the two-row build against the wavefront kernel's."""
    import mink_amd as mink
    from random_models import random_mjcf, rand_q
    rng = np.random.default_rng(9300 + seed)
    free = seed % 2 == 0
    for _ in range(200):
        nbody = int(rng.integers(4, 20))
        xml, sites = random_mjcf(rng, nbody, free_root=free, no_ball=True)
        m = mink.loads_mjcf(xml)
        if (free and 7 <= m.nv <= 32) or (not free and 17 <= m.nv <= 32):
            break
    else:
        pytest.skip("no draw in range")
    B = 37
    q = np.stack([rand_q(m, rng) for _ in range(B)])
    cfg = mink.Configuration(m, q)
    tgt_cfg = mink.Configuration(m, cfg.integrate(rng.normal(scale=0.2, size=(B, m.nv)), 1.0))
    frames = [(s, "site") for s in sites] + [(f"b{i}", "body") for i in range(nbody)]
    picks = [frames[i] for i in rng.choice(len(frames), size=min(int(rng.integers(1, 6)), len(frames)), replace=False)]
    tasks = []
    for name, typ in picks:
        if seed in (1, 2) and tasks and rng.uniform() < 0.7:
            rname, rtyp = picks[int(rng.integers(0, len(tasks)))]
            if (rname, rtyp) == (name, typ):
                rname, rtyp = "b0", "body"
            ft = mink.RelativeFrameTask(name, typ, rname, rtyp, position_cost=1.0, orientation_cost=0.5, lm_damping=0.1)
            ft.set_target(tgt_cfg.get_transform(name, typ, rname, rtyp))
        else:
            ft = mink.FrameTask(name, typ, position_cost=1.0, orientation_cost=0.5, lm_damping=0.1)
            ft.set_target(tgt_cfg.get_transform_frame_to_world(name, typ))
        tasks.append(ft)
    post = mink.PostureTask(m, cost=0.1); post.set_target(rand_q(m, rng))
    lims = [mink.ConfigurationLimit(m)]
    mink.solve_ik(cfg, tasks + [post], 1e-2, "mi355x", 1e-3, limits=lims)
    prob = list(cfg._problems.values())[-1]
    if prob.last_kernel().startswith("ik_solve_kernel"):
        pytest.skip("more than 32 links on the frames' chains: wavefront kernel")
    ftg = np.stack([(ft.transform_target_to_root if isinstance(ft, mink.RelativeFrameTask) else ft.transform_target_to_world).wxyz_xyz
                    for ft in tasks], axis=1)
    ptq = post.target_q[None, :]
    for kw in ({"n_steps": 4}, {"n_steps": 8, "until": (2e-2, 5e-2)}):
        got = prob.solve(q, ftg, ptq, None, 1e-2, 1e-3, quad_kernel=True, **kw)
        assert prob.last_kernel() == LOOP, prob.last_kernel()
        ref = prob.solve(q, ftg, ptq, None, 1e-2, 1e-3, wave_kernel=True, **kw)
        np.testing.assert_array_equal(got[2], ref[2])
        ok = (got[2] & 14) == 0
        np.testing.assert_allclose(got[0][ok], ref[0][ok], rtol=0, atol=1e-9)
        if len(got) > 3:
            # an instance may break one iteration apart only where the error that decided it lies within 1e-9 relative of a
            # threshold: the configuration at which the earlier of the two loops stopped (converged), its errors on the host
            diff = np.nonzero((got[3] != ref[3]) | (got[4] != ref[4]))[0]
            if len(diff):
                pos_thr, ori_thr = kw["until"]
                q_stop = np.where((got[3] <= ref[3])[:, None], got[0], ref[0])
                cs = mink.Configuration(m, q_stop)
                err = [np.atleast_2d(np.asarray(ft.compute_error(cs))) for ft in tasks]
                ep = np.max([np.linalg.norm(e[:, :3], axis=1) for e in err], axis=0)
                eo = np.max([np.linalg.norm(e[:, 3:], axis=1) for e in err], axis=0)
                for i in diff:
                    near = abs(ep[i] - pos_thr) <= 1e-9 * pos_thr or abs(eo[i] - ori_thr) <= 1e-9 * ori_thr
                    print("seed %d: instance %d breaks at %d / %d (pos %.17g, ori %.17g)" % (seed, i, got[3][i], ref[3][i], ep[i], eo[i]))
                    assert near and abs(int(got[3][i]) - int(ref[3][i])) == 1, (i, got[3][i], ref[3][i], ep[i], eo[i])


def test_edges(nat):
    """q_out in place, an odd batch (the last instance shares its wavefront with an idle row), an instance whose box becomes
    inconsistent (stops at its first failing step: NaN v, the wavefront loop's status), the outside-limits bit OR-ed over steps."""
    B = 33
    m, nm, prob, dt, damping, stand, q0, tg = _h1(nat, "h1_c3", B, seed=41)
    hinge = [j for j in range(m.njnt) if m.jnt_type[j] == 3 and m.jnt_limited[j]]
    j = hinge[0]; a = int(m.jnt_qposadr[j])
    q0[5, a] = m.jnt_range[j][1] + 0.5                  # far outside: the box is inconsistent at step 0
    j2 = hinge[3]; a2 = int(m.jnt_qposadr[j2])
    q0[9, a2] = m.jnt_range[j2][1] + 2e-6               # just outside: bit 1 at step 0, pulled back inside by the limit
    got = prob.solve(q0, tg, stand[None, :], None, dt, damping, n_steps=4, quad_kernel=True)
    assert prob.last_kernel() == LOOP
    ref = prob.solve(q0, tg, stand[None, :], None, dt, damping, n_steps=4, wave_kernel=True)
    np.testing.assert_array_equal(got[2], ref[2])
    assert got[2][5] & 2 and np.isnan(got[1][5]).all() and got[2][9] == 1
    ok = (got[2] & 14) == 0
    np.testing.assert_allclose(got[0][ok], ref[0][ok], rtol=0, atol=1e-10)
    # in place: q_out == q (host arrays and device tensors)
    qi = q0.copy()
    prob.solve(qi, tg, stand[None, :], None, dt, damping, n_steps=4, q_out=qi, quad_kernel=True)
    np.testing.assert_array_equal(qi[ok], got[0][ok])
    import torch
    qt = torch.tensor(q0, device="cuda")
    prob.solve(qt, torch.tensor(tg, device="cuda"), torch.tensor(stand[None, :], device="cuda"), None, dt, damping, n_steps=4, q_out=qt, quad_kernel=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(qt.cpu().numpy()[ok], got[0][ok])


def test_public_api(nat):
    """mink.solve_ik_steps on a batched H1 Configuration — the fixed loop and the threshold form — equals NativeProblem.solve
    bitwise and advances the configuration."""
    import mink_amd as mink
    m = workloads.load_robot("h1")
    B = 24
    stand = m.key_qpos[m.name2id("key", "stand")]
    rng = np.random.default_rng(51)
    q0 = workloads.sample_q(m, rng, B, stand)
    tgt = mink.Configuration(m, mink.Configuration(m, q0).integrate(rng.normal(scale=0.15, size=(B, m.nv)), 1.0))
    tasks = []
    for s, o in (("left_foot", 10.0), ("right_foot", 10.0), ("left_wrist", 0.0), ("right_wrist", 0.0)):
        t = mink.FrameTask(s, "site", 200.0, o, lm_damping=1.0)
        t.set_target(tgt.get_transform_frame_to_world(s, "site"))
        tasks.append(t)
    post = mink.PostureTask(m, cost=1.0); post.set_target(stand)
    com = mink.ComTask(cost=200.0)
    com_t = np.asarray(tgt.subtree_com())
    com.set_target(com_t)                              # (per-instance CoM targets: the default route is the two-row loop)
    tasks += [post, com]
    lims = [mink.ConfigurationLimit(m), mink.VelocityLimit(m, {m.jnt_names[j]: np.pi for j in range(m.njnt) if m.jnt_type[j] == 3})]
    cfg = mink.Configuration(m, q0.copy())
    q1, v1 = mink.solve_ik_steps(cfg, tasks, 5e-3, 5, damping=1e-1, limits=lims)
    prob = list(cfg._problems.values())[-1]
    assert prob.last_kernel() == LOOP
    np.testing.assert_array_equal(cfg.q_batch, q1)
    ftg = np.stack([t.transform_target_to_world.wxyz_xyz for t in tasks[:4]], axis=1)
    ctg = com_t.reshape(B, 1, 3)
    qn, vn, _ = prob.solve(q0, ftg, stand[None, :], ctg, 5e-3, 1e-1, n_steps=5)
    np.testing.assert_array_equal(q1, qn); np.testing.assert_array_equal(v1, vn)
    cfg2 = mink.Configuration(m, q0.copy())
    q2, v2, it2, cv2 = mink.solve_ik_steps(cfg2, tasks, 5e-3, 15, damping=1e-1, limits=lims, pos_threshold=1e-3, ori_threshold=1e-2)
    qu, vu, _, itu, cvu = prob.solve(q0, ftg, stand[None, :], ctg, 5e-3, 1e-1, n_steps=15, until=(1e-3, 1e-2))
    assert prob.last_kernel() == LOOP
    np.testing.assert_array_equal(q2, qu); np.testing.assert_array_equal(v2, vu)
    np.testing.assert_array_equal(it2, itu); np.testing.assert_array_equal(cv2, cvu.astype(bool))
    np.testing.assert_array_equal(cfg2.q_batch, q2)


def test_default_route(nat):
    """The default dispatch of fused loops follows profiles/r07_two_row_loop.txt: the two-row loop with a ComTask (H1 example as
    written) and without a floating base (Shadow hand); the wavefront kernel's loop for a floating base under frame / posture
    tasks alone (h1_c3, Go1); single solves stay on the two-row build."""
    B = 16
    for robot, expect in (("h1_full", LOOP), ("shadow", LOOP), ("h1_c3", "ik_solve_kernel"), ("go1", "ik_solve_kernel")):
        if robot.startswith("h1"):
            m, nm, prob, dt, damping, key, q0, tg = _h1(nat, robot, B, seed=61)
        else:
            m, nm, prob, dt, damping, key = (_go1 if robot == "go1" else _shadow)(nat, B)
            q0, tg = workloads.make_batch(m, nm, prob, np.random.default_rng(62), B, base_q=key)
        com = np.zeros((B, 1, 3)) if prob.n_com else None
        prob.solve(q0, tg, key[None, :], com, dt, damping, n_steps=3)
        assert prob.last_kernel().startswith(expect), (robot, prob.last_kernel())
        prob.solve(q0, tg, key[None, :], com, dt, damping)
        assert prob.last_kernel() == "ik_quad_kernel_32", (robot, prob.last_kernel())


def test_free_body_off_the_task_chains(nat):
    """A hand scene with a loose object (a free joint on no task chain: the two-row descriptor has no link for it).  Its fused loops
    run on the wavefront kernel — the default route with a RelativeFrameTask and under quad_kernel=True alike — so every
    coordinate of q comes back, the object's quaternion normalised as mj_integratePos does; device tensors, q_out left to the call."""
    import torch
    import mink_amd as mink
    m = FlatModel.load(os.path.join(oc.GOLDEN, "models", "all", "wonik_allegro__scene_left.json"))
    assert m.nq == m.nv + 1
    B = 21
    rng = np.random.default_rng(71)
    q0 = workloads.sample_q(m, rng, B)
    oq = int(m.jnt_qposadr[[j for j in range(m.njnt) if m.jnt_type[j] == 0][0]]) + 3
    q0[:, oq:oq + 4] *= 1.3                              # (an object quaternion that is not unit: the loop normalises it)
    cfg = mink.Configuration(m, q0.copy())
    tgt = mink.Configuration(m, cfg.integrate(rng.normal(scale=0.2, size=(B, m.nv)), 1.0))
    tasks = []
    for s in ("ff_tip", "mf_tip", "rf_tip"):
        t = mink.FrameTask(s, "site", position_cost=1.0, orientation_cost=0.0, lm_damping=1.0)
        t.set_target(tgt.get_transform_frame_to_world(s, "site"))
        tasks.append(t)
    rel = mink.RelativeFrameTask("th_tip", "site", "palm", "body", position_cost=1.0, orientation_cost=0.0, lm_damping=1.0)
    rel.set_target(tgt.get_transform("th_tip", "site", "palm", "body"))
    post = mink.PostureTask(m, cost=1e-2); post.set_target(q0[0])
    mink.solve_ik(cfg, tasks + [rel, post], 1e-2, "mi355x", 1e-3, limits=[mink.ConfigurationLimit(m)])
    prob = list(cfg._problems.values())[-1]
    assert prob.last_kernel() == "ik_quad_kernel_32", prob.last_kernel()          # (single solves: the two-row build)
    ftg = np.stack([t.transform_target_to_world.wxyz_xyz for t in tasks] + [rel.transform_target_to_root.wxyz_xyz], axis=1)
    dev = lambda x: torch.tensor(x, device="cuda")
    qd, fd, pd = dev(q0), dev(ftg), dev(post.target_q[None, :])
    for kw in ({"n_steps": 4}, {"n_steps": 8, "until": (1e-3, 1e-2)}):
        ref = [x.cpu().numpy() for x in prob.solve(qd, fd, pd, None, 1e-2, 1e-3, wave_kernel=True, **kw)]
        for extra in ({}, {"quad_kernel": True}):
            got = [x.cpu().numpy() for x in prob.solve(qd, fd, pd, None, 1e-2, 1e-3, **kw, **extra)]
            assert prob.last_kernel().startswith("ik_solve_kernel"), (kw, extra, prob.last_kernel())
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a, b)
        assert (ref[2] & ~1 == 0).all() and np.isfinite(ref[0]).all()
        np.testing.assert_allclose(np.linalg.norm(ref[0][:, oq:oq + 4], axis=1), 1.0, rtol=0, atol=1e-14)
        np.testing.assert_allclose(ref[0][:, oq:oq + 4], q0[:, oq:oq + 4] / 1.3, rtol=0, atol=1e-14)
