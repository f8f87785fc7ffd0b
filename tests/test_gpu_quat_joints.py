"""Quaternion joints at the edges of their representation, on the device (tests/quat_cases.py; its CPU side is
tests/test_quat_cases_cpu.py).  Every kernel family carries its own copy of the quaternion code around lie_dev.h's quat2vel /
qnormalize / axis_angle: the wavefront kernel (`mixed`, `balllimit`), the workgroup-per-problem kernel (`ballchain`, 68 dofs,
18 ball joints — the first ball joints this kernel sees in the suite), the two-row build of the row kernel (`h1`, free root)
and the stand-alone integrate kernel.  Each test pins the launch by name."""

import os

import numpy as np
import pytest

import quat_cases as qc
from oracle import ik as oik

pytestmark = pytest.mark.gpu
WAVE, WIDE, QUAD, LOOP = "ik_solve_kernel", "ik_wide_kernel", "ik_quad_kernel_32", "ik_quad_kernel_32_loop"
WITH_BALL = [n for n in qc.MODELS if n != "h1"]
EPS_NORM = 4.5e-16                                         # two ulps of 1: a unit quaternion after one rounding of a norm


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


_handles = {}


def _prob(nat, name):
    if name not in _handles:
        _handles[name] = qc.native_problem(nat, qc.problem(name), 64)
    return _handles[name]


def _pinned(name, kernel, loop=False):
    """The launch each model is there for."""
    if name == "ballchain":
        return kernel == WIDE
    if name == "h1":
        return kernel == (LOOP if loop else QUAD)
    return kernel.startswith(WAVE)


def _rel(v, v_ref):
    return np.abs(v - v_ref).max(axis=-1) / np.maximum(1.0, np.abs(v_ref).max(axis=-1))


def _quats(m, x):
    return np.stack([x[..., a:a + 4] for _, a in qc.quat_slices(m)], axis=-2)


# ------------------------------------------------------------------------------------------------ (a) the plain solve
@pytest.mark.parametrize("family", qc.FAMILIES)
@pytest.mark.parametrize("name", qc.MODELS)
def test_solve_against_both_oracles(nat, name, family):
    """Every instance against the plain-C oracle at 1e-8·max(1, ‖v‖∞), every 8th against the numpy oracle; the failure bits of
    the status are the C oracle's (none), its outside-limits bit is the reference's check_limits on the caller's q."""
    P, q, pt, tg = qc.case(name, family)
    _, prob = _prob(nat, name)
    v, st = prob.solve(q, tg, pt, None, P["dt"], P["damping"])
    assert _pinned(name, prob.last_kernel()), prob.last_kernel()
    v_c, st_c = qc.c_oracle(name, family)
    err = _rel(v, v_c)
    err_np = max(_rel(v[i], qc.numpy_oracle(P, q[i], tg[i], pt[i, 0])) for i in range(0, len(q), 8))
    outside = np.array([qc.outside_limits(P["m"], q[i]) for i in range(len(q))])
    print("(a) %-9s %-16s %s: max rel |v - C| %.2e, |v - numpy| %.2e; status %s" %
          (name, family, prob.last_kernel(), err.max(), err_np, dict(zip(*[x.tolist() for x in np.unique(st, return_counts=True)]))))
    np.testing.assert_array_equal(st & ~1, st_c)
    np.testing.assert_array_equal((st & 1).astype(bool), outside)
    assert err.max() <= 1e-8 and err_np <= 1e-8


# ------------------------------------------------------------------------------------------------ (b) the taps
def _box_from_rows(G, h, nv):
    lo, hi = np.full(nv, -np.inf), np.full(nv, np.inf)
    for r in range(len(h)):
        nz = np.flatnonzero(G[r])
        assert len(nz) == 1 and abs(G[r, nz[0]]) == 1.0
        if G[r, nz[0]] > 0:
            hi[nz[0]] = min(hi[nz[0]], h[r])
        else:
            lo[nz[0]] = max(lo[nz[0]], -h[r])
    return lo, hi


@pytest.mark.parametrize("family", qc.FAMILIES)
@pytest.mark.parametrize("name", WITH_BALL)
def test_taps_against_the_numpy_oracle(nat, name, family):
    """task_e / task_J of the frame rows and of the posture rows against oracle/ik.py::task_error_jacobian at
    1e-12·max(1, ‖e‖∞) and 1e-9·max(1, ‖J‖∞) (the bounds of test_gpu_wide.py); box_lo / box_hi on the dofs of the limited
    ball joints against the reference's rows at 1e-13.  The posture error on the ball dofs is where the wrap at π
    shows: its worst difference is printed."""
    P, q, pt, tg = qc.case(name, family)
    m = P["m"]
    _, prob = _prob(nat, name)
    n = 4
    _, _, taps = prob.solve(q[:n], tg[:n], pt[:n], None, P["dt"], P["damping"], taps=["task_e", "task_J", "box_lo", "box_hi"])
    assert _pinned(name, prob.last_kernel()), prob.last_kernel()
    lim_dofs = [d for j, va in qc.ball_dofs(m) if m.jnt_limited[j] for d in range(va, va + 3)]
    assert lim_dofs or name == "mixed"
    n_frame_rows = 6 * len(P["frames"])
    worst_e = worst_J = worst_ball = worst_box = 0.0
    for i in range(n):
        tasks, limits = qc.oracle_specs(P, tg[i], pt[i, 0])
        cfg = oik.Configuration(m, q[i])
        eJ = [oik.task_error_jacobian(cfg, t) for t in tasks]
        e_ref, J_ref = np.concatenate([e for e, _ in eJ]), np.vstack([J for _, J in eJ])
        assert taps["task_e"][i].shape == e_ref.shape
        se, sJ = max(1.0, np.abs(e_ref).max()), max(1.0, np.abs(J_ref).max())
        de, dJ = np.abs(taps["task_e"][i] - e_ref), np.abs(taps["task_J"][i] - J_ref)
        worst_e, worst_J = max(worst_e, de.max() / se), max(worst_J, dJ.max() / sJ)
        for _, va in qc.ball_dofs(m):
            worst_ball = max(worst_ball, de[n_frame_rows + va:n_frame_rows + va + 3].max())
        _, _, G, h = oik.build_ik(cfg, tasks, P["dt"], P["damping"], limits)
        lo, hi = _box_from_rows(G, h, m.nv)
        if lim_dofs:
            worst_box = max(worst_box, np.abs(taps["box_lo"][i][lim_dofs] - lo[lim_dofs]).max(),
                            np.abs(taps["box_hi"][i][lim_dofs] - hi[lim_dofs]).max())
        np.testing.assert_allclose(taps["task_e"][i], e_ref, rtol=0, atol=1e-12 * se)
        np.testing.assert_allclose(taps["task_J"][i], J_ref, rtol=0, atol=1e-9 * sJ)
    print("(b) %-9s %-16s rel |e| %.2e, rel |J| %.2e, posture error on the ball dofs |Δ| %.2e, limited-ball box |Δ| %.2e" %
          (name, family, worst_e, worst_J, worst_ball, worst_box))
    assert worst_box <= 1e-13


# ------------------------------------------------------------------------------------------------ (c) sign and scale
@pytest.mark.parametrize("name", qc.MODELS)
def test_sign_of_q_and_scale_of_the_target_leave_the_answer_alone(nat, name):
    """−q is the same rotation as q, and mju_quat2Vel does not see the norm of the posture target: the device on `neg_w` against
    the device on `plain`, and on `plain` with the posture target of `scaled` (same seed, so nothing else differs).  No oracle
    in the comparison; the bound is 16 × what the numpy oracle itself moves by on the same instances (16: the summation order of
    a 64-lane reduction against a serial sum), floor 1e-12, both relative to max(1, ‖v‖∞).
    Measured, oracle / device, for −q and for the scaled target: mixed 1.4e-16 / 2.6e-16 and 1.5e-16 / 1.9e-16; balllimit
    8.7e-16 / 1.6e-15 and 3.4e-16 / 6.6e-16; ballchain 1.2e-15 / 7.8e-16 and 7.8e-16 / 1.1e-15; h1 0 / 0 and 0 / 0 (a free
    root's quaternion enters through FK alone, and −q gives the same rotation matrix bit for bit).  16 × the oracle's figure
    is below the floor everywhere: the bound in force is 1e-12."""
    P, q, pt, tg = qc.case(name, "plain")
    _, q_neg, _, _ = qc.case(name, "neg_w")
    _, _, pt_sc, _ = qc.case(name, "scaled")
    _, prob = _prob(nat, name)
    v0, st0 = prob.solve(q, tg, pt, None, P["dt"], P["damping"])
    assert _pinned(name, prob.last_kernel()), prob.last_kernel()
    o0 = np.stack([qc.numpy_oracle(P, q[i], tg[i], pt[i, 0]) for i in range(len(q))])
    for what, q1, pt1 in (("-q", q_neg, pt), ("scaled target", q, pt_sc)):
        v1, st1 = prob.solve(q1, tg, pt1, None, P["dt"], P["damping"])
        assert _pinned(name, prob.last_kernel())
        o1 = np.stack([qc.numpy_oracle(P, q1[i], tg[i], pt1[i, 0]) for i in range(len(q))])
        moved_o, moved_d = _rel(o1, o0).max(), _rel(v1, v0).max()
        print("(c) %-9s %-13s numpy oracle moves by %.2e, device by %.2e" % (name, what, moved_o, moved_d))
        np.testing.assert_array_equal(st1 & ~1, st0 & ~1)
        assert moved_d <= max(16.0 * moved_o, 1e-12)


# ------------------------------------------------------------------------------------------------ (d) integration alone
AXIS = np.array([2.0, -1.0, 2.0]) / 3.0
OMEGA = (0.0, 1e-200, 1e-16, np.pi - 1e-9, np.pi, 2.0 * np.pi, 7.0, 1e3)          # rad/s at dt = 1: the angle itself


def _exact_quat_integrate(quat, omega, dt):
    """mju_quatIntegrate in 50-digit arithmetic: normalise(quat) ⊗ exp(axis·|ω|·dt), the zero quaternion the identity."""
    import mpmath as mp
    with mp.workdps(50):
        a = [mp.mpf(float(x)) for x in quat]
        n = mp.sqrt(sum(x * x for x in a))
        a = [mp.mpf(1), mp.mpf(0), mp.mpf(0), mp.mpf(0)] if n < mp.mpf("1e-15") else [x / n for x in a]
        w = [mp.mpf(float(x)) for x in omega]
        nw = mp.sqrt(sum(x * x for x in w))
        ax = [mp.mpf(1), mp.mpf(0), mp.mpf(0)] if nw < mp.mpf("1e-15") else [x / nw for x in w]
        half = nw * mp.mpf(float(dt)) / 2
        b = [mp.cos(half)] + [x * mp.sin(half) for x in ax]
        r = [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
             a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]]
        return np.array([float(x) for x in r])


@pytest.mark.parametrize("family", ["neg_w", "scaled", "f32", "zero"])
@pytest.mark.parametrize("name", qc.MODELS)
def test_integrate_on_its_own(nat, name, family):
    """mkh_integrate (Configuration.integrate and NativeModel.integrate) on designed velocities: the angular block of every
    ball and free joint of instance i is OMEGA[(i // 4) % 8]·AXIS, dt = 1.  Up to 2π: the oracle's Configuration.integrate
    at the atol = 1e-15 of test_gpu_joints.py.  7 and 1e3 rad, where the private sincos reduces its argument: as accurate as the
    numpy oracle against the 50-digit product, factor 4, floor 1e-15 (the rule of test_gpu_lie.py).  Every output quaternion is
    unit within 4.5e-16."""
    import mink_amd as mink
    P = qc.problem(name)
    m = P["m"]
    B = 32
    q, _ = qc.states(m, family, B)
    rng = np.random.default_rng(11)
    v = rng.normal(scale=0.3, size=(B, m.nv))
    ang = [int(m.jnt_dofadr[j]) + (3 if int(m.jnt_type[j]) == qc.JNT_FREE else 0) for j, _ in qc.quat_slices(m)]
    for i in range(B):
        for va in ang:
            v[i, va:va + 3] = OMEGA[(i // 4) % len(OMEGA)] * AXIS
    nm, _ = _prob(nat, name)
    qn = nm.integrate(q, v, 1.0)
    np.testing.assert_array_equal(mink.Configuration(m, q).integrate(v, 1.0), qn)
    ref = np.stack([oik.Configuration(m, q[i]).integrate(v[i], 1.0) for i in range(B)])
    small = np.array([OMEGA[(i // 4) % len(OMEGA)] <= 2.0 * np.pi for i in range(B)])
    norm_dev = np.abs(np.linalg.norm(_quats(m, qn), axis=-1) - 1.0).max()
    norm_ref = np.abs(np.linalg.norm(_quats(m, ref), axis=-1) - 1.0).max()
    err_d = err_o = 0.0
    for i in np.flatnonzero(~small):
        for (_, a), va in zip(qc.quat_slices(m), ang):
            exact = _exact_quat_integrate(q[i, a:a + 4], v[i, va:va + 3], 1.0)
            err_d = max(err_d, np.abs(qn[i, a:a + 4] - exact).max())
            err_o = max(err_o, np.abs(ref[i, a:a + 4] - exact).max())
    print("(d) %-9s %-7s |ω| ≤ 2π: max |q - oracle| %.2e; 7 and 1e3 rad against 50 digits: device %.2e, numpy oracle %.2e; "
          "| ‖quat‖ − 1 | device %.2e, oracle %.2e" % (name, family, np.abs(qn[small] - ref[small]).max(), err_d, err_o, norm_dev, norm_ref))
    np.testing.assert_allclose(qn[small], ref[small], rtol=0, atol=1e-15)
    assert err_d <= max(4.0 * err_o, 1e-15)
    assert norm_dev <= EPS_NORM


# ------------------------------------------------------------------------------------------------ (e) integration in the kernels
def _numpy_loop(P, q_i, tg_i, pt_i, n):
    """The callers' loop on the numpy oracle (as test_gpu_wide.py::_oracle_loop, which does not carry a posture gain)."""
    cfg = oik.Configuration(P["m"], q_i)
    tasks, limits = qc.oracle_specs(P, tg_i, pt_i)
    for _ in range(n):
        v = oik.solve_ik(P["m"], cfg, tasks, P["dt"], P["damping"], limits)
        cfg.update(cfg.integrate(v, P["dt"]))
    return cfg.q.copy(), v


def _c_loop(P, q, tg, pt, n):
    """The same loop on a whole batch: the C oracle's solve, the numpy oracle's mj_integratePos."""
    from oracle import cport
    tasks, limits = qc.oracle_specs(P, tg[0], pt[0, 0])
    cp = cport.CProblem(P["m"], tasks, limits)
    q = q.copy()
    for _ in range(n):
        v, st = cp.solve_batch(q, tg, pt, P["dt"], P["damping"], nthreads=4)
        assert (st == 0).all()
        q = np.stack([oik.Configuration(P["m"], q[k]).integrate(v[k], P["dt"]) for k in range(len(q))])
    return q, v


@pytest.mark.parametrize("family", ["neg_w", "scaled", "f32"])
@pytest.mark.parametrize("name", qc.MODELS)
def test_fused_steps(nat, name, family):
    """mkh_solve_steps.  One step: q_out against the oracle's integrate(v_device, dt) at 1e-14 — the kernel's integration apart
    from its solve.  Five steps on 4 instances against the callers' loop on the numpy oracle at the bounds of test_gpu_wide.py
    and test_gpu_steps.py, q 1e-10 and v 1e-7·max(1, ‖v‖∞).  The kernels multiply on the right by a small rotation, as the
    reference does, so the sign of w is the reference loop's on every quaternion of every instance (the C oracle's solve + the
    numpy integrate): from `neg_w` it stays negative, except where 5 steps at the velocity limit carry a joint through w = 0 —
    on `ballchain`, whose ball joints turn by up to 0.8 rad; the count is printed."""
    P, q, pt, tg = qc.case(name, family)
    m = P["m"]
    _, prob = _prob(nat, name)
    kw = {"quad_kernel": True} if name == "h1" else {}
    q1, v1, st1 = prob.solve(q, tg, pt, None, P["dt"], P["damping"], n_steps=1, **kw)
    assert _pinned(name, prob.last_kernel(), loop=True), prob.last_kernel()
    assert ((st1 & ~1) == 0).all(), st1
    ref1 = np.stack([oik.Configuration(m, q[i]).integrate(v1[i], P["dt"]) for i in range(len(q))])
    one = np.abs(q1 - ref1).max()
    q5, v5, st5 = prob.solve(q, tg, pt, None, P["dt"], P["damping"], n_steps=5, **kw)
    assert _pinned(name, prob.last_kernel(), loop=True) and ((st5 & ~1) == 0).all()
    dq = dv = 0.0
    for i in range(0, len(q), len(q) // 4):
        q_ref, v_ref = _numpy_loop(P, q[i], tg[i], pt[i, 0], 5)
        dq, dv = max(dq, np.abs(q5[i] - q_ref).max()), max(dv, _rel(v5[i], v_ref))
        np.testing.assert_allclose(q5[i], q_ref, rtol=0, atol=1e-10)
        np.testing.assert_allclose(v5[i], v_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(v_ref).max()))
    q_c, _ = _c_loop(P, q, tg, pt, 5)
    w_dev, w_ref = _quats(m, q5)[..., 0], _quats(m, q_c)[..., 0]
    crossed = int((np.sign(w_ref) != np.sign(_quats(m, q)[..., 0])).sum())
    print("(e) %-9s %-7s %s: one step |q_out - integrate(v)| %.2e; five steps |q - oracle| %.2e, rel |v - oracle| %.2e; "
          "w changes sign on %d of %d quaternions in the reference loop" %
          (name, family, prob.last_kernel(), one, dq, dv, crossed, w_ref.size))
    assert one <= 1e-14
    assert np.abs(w_ref).min() > 1e-9                         # (no quaternion ends on w = 0, where the sign is rounding)
    np.testing.assert_array_equal(np.sign(w_dev), np.sign(w_ref))
    if family == "neg_w":
        assert crossed <= w_ref.size // 20 and (name == "ballchain" or crossed == 0)


@pytest.mark.parametrize("name", ["mixed", "h1"])
def test_quaternion_norm_over_a_long_fused_loop(nat, name):
    """200 fused steps from the `scaled` starts (norms 0.5 … 2): every output quaternion stays unit within 4 × the deviation the
    reference's loop shows after the same 200 steps on 2 of the instances (the C oracle's solve, the numpy oracle's
    mj_integratePos), floor 4.5e-16.  Measured: device 2.2e-16 on both models; the reference loop 5.6e-16 (mixed), 6.7e-16
    (h1) — it normalises only what is off by more than 1e-15, the kernels normalise at every step."""
    P, q, pt, tg = qc.case(name, "scaled")
    m = P["m"]
    _, prob = _prob(nat, name)
    kw = {"quad_kernel": True} if name == "h1" else {}
    qK, vK, st = prob.solve(q, tg, pt, None, P["dt"], P["damping"], n_steps=200, **kw)
    assert _pinned(name, prob.last_kernel(), loop=True), prob.last_kernel()
    assert ((st & ~1) == 0).all(), st
    idx = np.arange(0, len(q), len(q) // 2)
    qo, _ = _c_loop(P, q[idx], tg[idx], pt[idx], 200)
    dev_d = np.abs(np.linalg.norm(_quats(m, qK), axis=-1) - 1.0).max()
    dev_o = np.abs(np.linalg.norm(_quats(m, qo), axis=-1) - 1.0).max()
    print("(e) %-9s 200 steps from `scaled`: | ‖quat‖ − 1 | device %.2e (all %d instances), oracle loop %.2e; |q - oracle loop| %.2e" %
          (name, dev_d, len(q), dev_o, np.abs(qK[idx] - qo).max()))
    assert dev_d <= max(4.0 * dev_o, EPS_NORM)


# ------------------------------------------------------------------------------------------------ (f) multi-start's distance
def test_multistart_distance_across_the_sign_of_q(nat):
    """ms_distance.h's tangent-space difference on `ballslide`.  The starts carry w < 0 on every odd seed (and on q itself), the
    reference is the unflipped twin of q: the loop keeps the sign, so the relative quaternion of a flipped result has w < 0 and
    the distance goes through the wrap.  Then `same`: the reference is a bit-identical copy of one seed's result (odd targets)
    or its negation (even ones) — distance 0 on both sides.  tests/multistart_ref.py's restatement applied to the device's own
    q_all reproduces the device's seed_index at test_gpu_multistart.py's 1e-12.  (The entry point validates shapes only: it
    takes these seeds.)"""
    import mink_amd
    import multistart_ref as ref
    from mink_amd.api_specs import configuration_limit_desc
    from test_gpu_multistart import _check_selection
    m = mink_amd.load_mjcf(os.path.join(qc.GOLDEN, "ballslide.xml"))
    nm = nat.NativeModel(m, 0)
    B, S, iters, pth, oth, dt, damping = 32, 8, 40, 1e-3, 1e-2, 1.0, 1e-3
    prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "tip"),
                                               "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 0.1}],
                             configuration_limits=[configuration_limit_desc(m)], max_batch=B * S)
    X, _ = qc.states(m, "plain", B * S, seed=qc.SEED + 7)
    F, _ = qc.states(m, "neg_w", B * S, seed=qc.SEED + 7)
    X, F = X.reshape(B, S, m.nq), F.reshape(B, S, m.nq)
    seeds = np.where((np.arange(S) % 2 == 1)[None, :, None], F, X)
    q, q_ref = F[:, 0].copy(), X[:, 0].copy()
    seeds[:, 0] = q
    goal = mink_amd.Configuration(m, X[:, 1]).integrate(np.random.default_rng(3).normal(scale=0.05, size=(B, m.nv)), 1.0)
    tg = mink_amd.Configuration(m, goal).get_transform_frame_to_world("tip", "site").wxyz_xyz[:, None, :]
    kw = dict(n_seeds=S, max_iters=iters, pos_threshold=pth, ori_threshold=oth, seeds=seeds, return_all=True)
    out = prob.solve_multistart(q, tg, None, None, dt, damping, reference=q_ref, **kw)
    assert prob.last_kernel()
    np.testing.assert_array_equal(out.seeds, seeds)
    ok = ref.eligible(out.converged_all, out.status_all)
    flipped = (_quats(m, out.q_all) * _quats(m, q_ref)[:, None]).sum(axis=-1).min(axis=-1) < 0          # (B, S)
    n_none = _check_selection(m, out, q_ref)
    print("(f) ballslide %s: %d of %d instances eligible, %d of them end with w < 0 against the reference; %d targets without one; "
          "seed_index %s" % (prob.last_kernel(), int(ok.sum()), B * S, int((ok & flipped).sum()), n_none,
                             np.bincount(out.seed_index, minlength=S).tolist()))
    assert (ok & flipped).sum() >= B // 2 and (ok & ~flipped).sum() >= B // 2 and n_none < B // 2
    # `same`: the reference is one eligible result itself (odd targets) or its negation (even ones)
    pick = np.array([np.flatnonzero(ok[b])[-1] if ok[b].any() else 0 for b in range(B)])
    twin = out.q_all[np.arange(B), pick].copy()
    for _, a in qc.quat_slices(m):
        twin[0::2, a:a + 4] *= -1.0
    out2 = prob.solve_multistart(q, tg, None, None, dt, damping, reference=twin, **kw)
    np.testing.assert_array_equal(out2.q_all, out.q_all)
    _check_selection(m, out2, twin)
    has = ok.any(axis=1)
    d_pick = np.array([ref.distance(m, out.q_all[b, pick[b]], twin[b]) for b in range(B)])
    d_chosen = np.array([ref.distance(m, out2.q[b], twin[b]) for b in range(B)])
    print("(f) `same`: restated distance of the twin ≤ %.1e, of the device's choice ≤ %.1e" % (d_pick[has].max(), d_chosen[has].max()))
    assert (d_chosen[has] <= 1e-12).all()
    prob.close(); nm.close()


# ------------------------------------------------------------------------------------------------ convex_pre.hip's own FK
FLOATING_CANS = """<mujoco><compiler angle="radian"/><worldbody>
  <geom name="crate" type="box" size=".1 .2 .2" pos="0.4 0 0" quat="0.98 0.1 0.05 0.1"/>
  <geom name="drum" type="cylinder" size=".1 .2" pos="-0.4 0 0" quat="0.95 0.2 0.1 0"/>
  <geom name="crate2" type="box" size=".2 .2 .1" pos="0 0 0.5" quat="0.97 0.05 0.2 0.1"/>
  <geom name="drum2" type="cylinder" size=".1 .2" pos="0 0.4 0" quat="0.7 0 0.7 0.1"/>
  <body name="base" pos="0 0 0"><freejoint name="root"/>
    <inertial pos="0 0 0" mass="1" diaginertia="1 1 1"/>
    <geom name="l_can" type="cylinder" size=".03 .04" pos="0.08 0 0" quat="1 0 1 0"/>
    <geom name="r_can" type="cylinder" size=".03 .04" pos="-0.08 0 0" quat="1 1 0 0"/>
    <body name="arm" pos="0 0 0.1"><joint name="elbow" type="hinge" axis="0 1 0" range="-1.5 1.5"/>
      <inertial pos="0 0 0.05" mass="0.3" diaginertia="1 1 1"/>
      <geom name="arm_can" type="cylinder" size=".025 .04" pos="0 0 0.08"/>
      <site name="tip" pos="0 0 0.13"/>
    </body>
  </body>
</worldbody></mujoco>"""
CAN_PAIRS = [("l_can", "crate"), ("l_can", "drum"), ("r_can", "crate"), ("r_can", "drum"), ("arm_can", "crate"), ("arm_can", "drum"),
             ("arm_can", "crate2"), ("l_can", "drum2")]


@pytest.mark.parametrize("family", ["neg_w", "f32"])
def test_convex_pairs_in_front_of_the_solve_see_the_same_base(nat, family):
    """convex_pre.hip walks the kinematic chains with an FK of its own, reached from 32 768 (instance, pair) items on: a
    floating body with three cylinders against two boxes and two cylinders (8 general convex pairs, every one separated — the
    base stays within 0.15 of the origin, the obstacles start at 0.3; d_min = 0.15 makes rows bind), B = 4 096.  Against the same
    instances below the threshold (the first 64: the routine inside the solve kernel) at 1e-12·max(1, ‖v‖∞) — the device's two
    routes must agree — and against the numpy oracle on 8 instances at 1e-8."""
    import mink_amd
    m = mink_amd.loads_mjcf(FLOATING_CANS)
    pairs = [(m.name2id("geom", a), m.name2id("geom", b)) for a, b in CAN_PAIRS]
    det, dmin, dt, damping = 0.35, 0.15, 0.1, 1e-3
    B, n = 4096, 64
    q, pt = qc.states(m, family, B)
    q[:, :3] *= 0.25
    nm = nat.NativeModel(m)
    tip = m.name2id("site", "tip")
    cost = np.array([1.0, 1.0, 1.0, 0.2, 0.2, 0.2])
    idx, lower, upper = oik.configuration_limit_arrays(m, oik.ConfigurationLimitSpec())
    prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": tip, "cost": list(cost), "gain": 1.0, "lm_damping": 0.0}],
                             posture_tasks=[{"cost": 1e-2}],
                             configuration_limits=[{"gain": 0.95, "lower": lower, "upper": upper, "indices": idx}],
                             collision_limits=[{"geom_id_pairs": np.array(pairs), "gain": 0.85, "minimum_distance_from_collisions": dmin,
                                                "collision_detection_distance": det, "bound_relaxation": 0.0}], max_batch=B)
    qt = nm.integrate(q, np.random.default_rng(3).normal(scale=0.3, size=(B, m.nv)), 1.0)
    dummy = np.zeros((B, 1, 7)); dummy[:, :, 0] = 1
    tg = prob.solve(qt, dummy, pt[:, None, :], None, 1.0, 1.0, taps=["frame_pose"], solve_qp=False)[2]["frame_pose"]
    v, st = prob.solve(q, tg, pt[:, None, :], None, dt, damping)
    split = prob.last_kernel()
    assert split.startswith("convex_pre+"), split
    assert ((st & ~1) == 0).all(), np.unique(st, return_counts=True)
    v_in, st_in = prob.solve(q[:n], tg[:n], pt[:n, None, :], None, dt, damping)
    inside = prob.last_kernel()
    assert not inside.startswith("convex_pre+") and inside.startswith(WAVE), inside
    routes = _rel(v[:n], v_in).max()
    spec = oik.CollisionAvoidanceLimitSpec(pairs, collision_detection_distance=det, minimum_distance_from_collisions=dmin)
    worst = binding = 0
    for i in range(0, n, 8):
        ts = [oik.FrameTaskSpec(tip, "site", cost, tg[i, 0], 1.0, 0.0), oik.PostureTaskSpec(np.full(m.nv, 1e-2), pt[i], 1.0)]
        v_ref, (_, _, G, h) = oik.solve_ik(m, q[i], ts, dt, damping, [oik.ConfigurationLimitSpec(), spec], return_problem=True)
        fin = np.isfinite(h[-len(pairs):])
        binding += int((np.abs(G[-len(pairs):][fin] @ (v_ref * dt) - h[-len(pairs):][fin]) < 1e-9).sum())
        worst = max(worst, _rel(v[i], v_ref))
    print("convex_pre %-5s %s / %s: the two routes differ by %.2e; against the numpy oracle %.2e (%d convex rows binding on the 8 instances)" %
          (family, split, inside, routes, worst, binding))
    np.testing.assert_array_equal(st[:n], st_in)
    assert binding > 0 and worst <= 1e-8
    assert routes <= 1e-12
    prob.close(); nm.close()
