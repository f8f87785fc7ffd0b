"""The workgroup-per-problem kernel (mink_amd/csrc/wide_kernel.h) past 100 dofs and on random trees.

Every model here plans a branch of plan_wide that no other test reaches — tests/test_problem_plan_cpu.py names that branch per
model on the host (tableau in LDS or in the workgroup's slice of device memory, 2 … 9 chain words, the block-pivot staging over
the poses / appended / absent, one to three dofs per thread, the largest model and the first refused one, the pair cull on a
wide-only model) and tests/test_wide_cases_cpu.py shows the reference itself good to 1e-13 on these inputs.  The device is held
to DESIGN.md §5: ‖v − v_ref‖∞ ≤ 1e-8·max(1, ‖v_ref‖∞), against the plain-C oracle on every instance and against the numpy
oracle (another pivot order) on some."""

import re

import numpy as np
import pytest

import quat_cases as qc
import wide_cases as wc
from oracle import cport
from oracle import ik as oik
from qp_certificate import certificate

pytestmark = pytest.mark.gpu
WIDE = "ik_wide_kernel"
TOL = 1e-8


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


_handles = {}


def _prob(nat, name, max_batch=wc.B):
    if (name, max_batch) not in _handles:
        _handles[(name, max_batch)] = qc.native_problem(nat, wc.problem(name), max_batch)
    return _handles[(name, max_batch)]


def _rel(v, v_ref):
    return np.abs(v - v_ref).max(axis=-1) / np.maximum(1.0, np.abs(v_ref).max(axis=-1))


def _chain_dofs(m, body):
    """Dofs that move `body`, from the parent array."""
    dofs = []
    while body > 0:
        dofs += range(int(m.body_dofadr[body]), int(m.body_dofadr[body]) + int(m.body_dofnum[body])) if m.body_dofnum[body] else []
        body = int(m.body_parentid[body])
    return sorted(dofs)


# ------------------------------------------------------------------------------------------------ sizes across the switches
@pytest.mark.parametrize("name", wc.SOLVED)
def test_solve_against_both_oracles_and_the_certificate(nat, name):
    """B = 8 instances of one model of tests/wide_cases.py: v of every instance against the C oracle, of instance 0 against the
    numpy oracle, and instance 0's v held to the optimality conditions of the numpy oracle's own (H, c, G, h)
    (tests/qp_certificate.py: nothing of the device's tableau enters).  A point within t = 1e-8·dt·max(1, ‖v‖∞) of the minimiser
    violates no box row (unit norm) by more than t, and — its active set (slack ≤ 1e-9 > t) containing the minimiser's — leaves a
    residual r with ‖P⁻¹r‖∞ ≤ ‖P⁻¹‖₂·‖P·δ‖₂ ≤ cond₂(P)·√nv·t: the two bounds asserted."""
    P, q, pt, tg = wc.case(name)
    m, dt = P["m"], P["dt"]
    _, prob = _prob(nat, name)
    v, st = prob.solve(q, tg, pt, None, dt, P["damping"])
    assert prob.last_kernel() == WIDE, prob.last_kernel()
    assert ((st & ~1) == 0).all(), np.unique(st, return_counts=True)
    v_c, st_c = wc.c_oracle(name)
    assert (st_c == 0).all()
    err = _rel(v, v_c)
    bound = wc.n_bound(P, v_c)
    tasks, limits = qc.oracle_specs(P, tg[0], pt[0, 0])
    v_np, (H, c, G, h) = oik.solve_ik(m, q[0], tasks, dt, P["damping"], limits, return_problem=True)
    err_np = _rel(v[0], v_np)
    t = TOL * dt * max(1.0, np.abs(v_np).max())
    primal, active, stat = certificate(H, c, G, h, v[0] * dt)
    cond = np.linalg.cond(H)
    print("%-10s nv %3d nbody %3d: max rel |v - C| %.2e, |v - numpy| %.2e; certificate primal %.1e stationarity %.1e "
          "(t = %.1e, cond(H) = %.0f, %d rows active); velocity bounds binding %s"
          % (name, m.nv, m.nbody, err.max(), err_np, primal, stat, t, cond, len(active), bound.tolist()))
    assert bound.mean() > 2 and bound.min() >= 1
    assert err.max() <= TOL and err_np <= TOL
    assert primal <= t and stat <= cond * np.sqrt(m.nv) * t


@pytest.mark.parametrize("name", wc.SOLVED)
def test_task_taps_read_every_chain_word(nat, name):
    """task_e / task_J of two instances against oik.task_error_jacobian at 1e-12 / 1e-9 — every frame task, the first site and
    the tip among them — and the columns beyond a site's own chain exactly 0.  A site past dof 128 has its columns in chain
    word 2 and beyond: a wrong word index zeroes them or lights columns off the chain."""
    P, q, pt, tg = wc.case(name)
    m = P["m"]
    _, prob = _prob(nat, name)
    pick = [0, len(q) - 1]
    _, _, taps = prob.solve(q[pick], tg[pick], pt[pick], None, P["dt"], P["damping"], taps=["task_e", "task_J"])
    assert prob.last_kernel() == WIDE
    worst_e = worst_J = 0.0
    for r, i in enumerate(pick):
        cfg = oik.Configuration(m, q[i])
        tasks, _ = qc.oracle_specs(P, tg[i], pt[i, 0])
        eJ = [oik.task_error_jacobian(cfg, t) for t in tasks]
        e_ref, J_ref = np.concatenate([e for e, _ in eJ]), np.vstack([J for _, J in eJ])
        assert e_ref.shape == taps["task_e"][r].shape and J_ref.shape == taps["task_J"][r].shape
        worst_e = max(worst_e, np.abs(taps["task_e"][r] - e_ref).max() / max(1.0, np.abs(e_ref).max()))
        worst_J = max(worst_J, np.abs(taps["task_J"][r] - J_ref).max() / max(1.0, np.abs(J_ref).max()))
        np.testing.assert_allclose(taps["task_e"][r], e_ref, rtol=0, atol=1e-12 * max(1.0, np.abs(e_ref).max()))
        np.testing.assert_allclose(taps["task_J"][r], J_ref, rtol=0, atol=1e-9 * max(1.0, np.abs(J_ref).max()))
        for k, (site, typ, _, _, _) in enumerate(P["frames"]):
            on = _chain_dofs(m, int(m.site_bodyid[m.name2id(typ, site)]))
            off = np.setdiff1d(np.arange(m.nv), on)
            Jk = taps["task_J"][r][6 * k:6 * k + 6]
            assert (Jk[:, off] == 0.0).all(), (name, site)
            for w in range(-(-m.nv // 64)):                           # every chain word the site's chain reaches carries columns
                cols = [d for d in on if d // 64 == w]
                assert not cols or np.abs(Jk[:, cols]).max() > 0.0, (name, site, w)
    tip = _chain_dofs(m, int(m.site_bodyid[m.name2id("site", P["frames"][-1][0])]))
    assert max(tip) == m.nv - 1 and len(P["frames"]) >= 2
    print("%-10s task_e %.1e task_J %.1e of their scale; tip chain reaches chain word %d" % (name, worst_e, worst_J, max(tip) // 64))


def test_second_problem_on_a_device_memory_tableau(nat):
    """chain124 (the first size whose tableau lives in the workgroup's slice of device memory) with 37 instances more than
    the launch has workgroups: some workgroups solve a second problem on the same slice."""
    name = "chain124"
    _, prob = _prob(nat, name, 1024)
    B = prob.launch_info(1024)["grid"] + 37
    assert B <= 1024
    info = prob.launch_info(B)
    assert info["block"] == 256 and 0 < info["grid"] < B, info
    P, q, pt, tg = wc.case(name, B)
    v, st = prob.solve(q, tg, pt, None, P["dt"], P["damping"])
    assert prob.last_kernel() == WIDE and ((st & ~1) == 0).all()
    v_c, st_c = wc.c_oracle(name, B)
    assert (st_c == 0).all()
    err = _rel(v, v_c)
    print("chain124, %d instances on %d workgroups: max rel |v - C| %.2e" % (B, info["grid"], err.max()))
    assert err.max() <= TOL


@pytest.mark.parametrize("name,picks", [("chain130", (0, 5, 7)), ("ball86", (0, 4, 7))])
def test_fused_loops(nat, name, picks):
    """mkh_solve_steps / mkh_solve_until inside the kernel with three chain words and the tableau in device memory (chain130) and
    without the block-pivot staging (ball86).

    n_steps = 3 against the same loop of single launches (q 1e-11, v 1e-9) on the per-model problem: the two loops hand each
    other q that differs in the last bit (q ⊕ Δq inside the kernel, q ⊕ (Δq/dt)·dt outside), so 1e-11 on q after three steps
    asks the QP's answer to be determined to 1e-11 / (3·dt) in v — which tests/test_wide_cases_cpu.py shows for these inputs
    on the reference (cond(H) ≈ 40), and does NOT show for the near targets below: there the frame errors and with them the
    Levenberg–Marquardt term vanish, cond(H) reaches 1e5, the reference itself moves by 7e-12 in v under one-ulp changes, and
    the device's v was measured 5e-10 … 9e-10 from the C oracle's (inside 1e-8, but two device runs then differ by 2e-11 in q).

    until= with reachable targets at very different distances (tests/wide_cases.py::loop_case) against the callers' loop on the
    numpy oracle on three instances: iteration counts and converged flags equal, q 1e-9."""
    P, q, qt, tg = wc.loop_case(name)
    m, dt, damping = P["m"], P["dt"], P["damping"]
    nm, prob = _prob(nat, name)
    _, q_far, pt, tg_far = wc.case(name)
    K = wc.LOOP_STEPS
    qK, vK, st = prob.solve(q_far, tg_far, pt, None, dt, damping, n_steps=K)
    assert prob.last_kernel() == WIDE and ((st & ~1) == 0).all()
    qs = q_far.copy()
    for _ in range(K):
        vs, _ = prob.solve(qs, tg_far, pt, None, dt, damping)
        qs = nm.integrate(qs, vs, dt)
    print("%s, %d fused steps against single launches: |q| %.1e, |v| %.1e" % (name, K, np.abs(qK - qs).max(), np.abs(vK - vs).max()))
    np.testing.assert_allclose(qK, qs, rtol=0, atol=1e-11)
    np.testing.assert_allclose(vK, vs, rtol=0, atol=1e-9 * max(1.0, np.abs(vs).max()))
    qU, vU, stU, it, cv = prob.solve(q, tg, qt[:, None, :].copy(), None, dt, damping, n_steps=wc.LOOP_MAX_ITERS, until=wc.LOOP_THRESHOLDS)
    assert prob.last_kernel() == WIDE and ((stU & ~1) == 0).all()
    print("%s, until: iterations %s converged %s" % (name, it.tolist(), cv.tolist()))
    assert cv.sum() >= 2 and (cv == 0).sum() >= 2
    for i in picks:
        q_ref, n, done = wc.oracle_loop(P, q[i], tg[i], qt[i], wc.LOOP_MAX_ITERS, wc.LOOP_THRESHOLDS)
        assert (it[i], bool(cv[i])) == (n, done), (i, it[i], cv[i], n, done)
        print("   instance %d: %d iterations, converged %s, |q - oracle loop| %.1e" % (i, n, done, np.abs(qU[i] - q_ref).max()))
        np.testing.assert_allclose(qU[i], q_ref, rtol=0, atol=1e-9)


def test_first_model_that_does_not_fit_is_refused(nat):
    """One link more than chain_last (which test_solve_against_both_oracles_and_the_certificate solves): MKH_E_LIMIT at problem
    creation, and the message carries the LDS the model would need."""
    assert wc.CHAINS["chain_last+1"] == wc.CHAINS["chain_last"] + 1
    with pytest.raises(nat.MinkHipError) as exc:
        qc.native_problem(nat, wc.problem("chain_last+1"), wc.B)
    msg = str(exc.value)
    assert "libminkhip error -4:" in msg and "model too large for the workgroup-per-problem kernel" in msg, msg      # MKH_E_LIMIT
    kb = re.search(r"(\d+) KB of LDS per problem, 158 KB available", msg)
    assert kb and int(kb.group(1)) >= 158, msg


def test_wide_route_by_body_count_alone(nat):
    """fixed30: 91 bodies on 30 dofs.  Against the C oracle on the model itself, and against the same chain without its
    jointless bodies (31 bodies: a wavefront kernel) at 1e-9 — the same kinematics."""
    P, q, pt, tg = wc.case("fixed30")
    _, prob = _prob(nat, "fixed30")
    v, st = prob.solve(q, tg, pt, None, P["dt"], P["damping"])
    assert prob.last_kernel() == WIDE and ((st & ~1) == 0).all()
    err = _rel(v, wc.c_oracle("fixed30")[0])
    P0, q0, pt0, tg0 = wc.case("fixed30_plain")
    assert (P["m"].nbody, P["m"].nv, P0["m"].nbody, P0["m"].nv) == (91, 30, 31, 30)
    _, prob0 = _prob(nat, "fixed30_plain")
    v0, st0 = prob0.solve(q0, tg0, pt0, None, P0["dt"], P0["damping"])
    assert "wide" not in prob0.last_kernel() and ((st0 & ~1) == 0).all(), prob0.last_kernel()
    print("fixed30: max rel |v - C| %.2e; against %s on the chain without jointless bodies %.2e" % (err.max(), prob0.last_kernel(), _rel(v, v0).max()))
    assert err.max() <= TOL and _rel(v, v0).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ random trees past one wavefront
@pytest.mark.parametrize("seed", wc.TREE_SEEDS)
def test_random_tree_past_one_wavefront(seed):
    """test_random_tree's draw on trees of 66 … 120 bodies (every joint kind, frames on sites and bodies with zeroed cost
    components, per-dof posture costs, a ComTask in half of them, ConfigurationLimit with a gain, VelocityLimit on a subset),
    B = 16 through the public solve_ik.  The seeds were picked on the CPU (tests/test_oracle_random_models.py holds the
    reference on them); no draw is skipped."""
    import mink_amd as mink
    T = wc.random_tree(seed)
    m, q, B = T["m"], T["q"], len(T["q"])
    assert m.nbody > 64 or m.nv > 64
    # among the six: a ball joint below a branching point, a body with two joints, a jointless body, nv > 128 — from the arrays
    everyone = [wc.tree_properties(wc.random_tree(s)["m"]) for s in wc.TREE_SEEDS]
    assert len(everyone) == 6 and all(any(p[key] for p in everyone) for key in ("ball_below_branch", "two_joints", "jointless", "nv_gt_128"))
    assert sum(wc.random_tree(s)["com"] is not None for s in wc.TREE_SEEDS) >= 2
    cfg = mink.Configuration(m, q)
    tasks = []
    for k, (name, typ, cost, gain, lm) in enumerate(T["frames"]):
        ft = mink.FrameTask(name, typ, position_cost=cost[:3], orientation_cost=cost[3], gain=gain, lm_damping=lm)
        ft.set_target(mink.SE3(T["tg"][:, k]))
        tasks.append(ft)
    post = mink.PostureTask(m, cost=T["post"][0], gain=T["post"][1])
    post.set_target(T["post"][2])
    extra = [post]
    if T["com"] is not None:
        com = mink.ComTask(cost=T["com"][0])
        com.set_target(T["com"][1])
        extra.append(com)
    lims = [mink.ConfigurationLimit(m, gain=T["cfg_gain"])] + ([mink.VelocityLimit(m, T["vel"])] if T["vel"] else [])
    v, st = mink.solve_ik(cfg, tasks + extra, T["dt"], "mi355x", T["damping"], limits=lims, return_status=True)
    assert np.isfinite(v).all() and ((st & ~1) == 0).all()
    v_c, st_c = wc.tree_c_oracle(T)
    assert (st_c == 0).all()
    err = _rel(v, v_c)
    err_np = 0.0
    for i in (0, B - 1):
        ts, ls = wc.tree_specs(T, i)
        err_np = max(err_np, _rel(v[i], oik.solve_ik(m, q[i], ts, T["dt"], T["damping"], ls)))
    print("tree %d: nbody %d nv %d, %d frame tasks %s, ComTask %s: max rel |v - C| %.2e, |v - numpy| %.2e"
          % (seed, m.nbody, m.nv, len(tasks), [t for _, t, _, _, _ in T["frames"]], T["com"] is not None, err.max(), err_np))
    assert err.max() <= TOL and err_np <= TOL
    # compute_error / compute_jacobian of each task on instance 0
    one = mink.Configuration(m, q[0])
    o = oik.Configuration(m, q[0])
    ts, _ = wc.tree_specs(T, 0)
    mine = []
    for task in tasks:
        t1 = mink.FrameTask(task.frame_name, task.frame_type, task.cost[:3], task.cost[3:], task.gain, task.lm_damping)
        t1.set_target(mink.SE3(task.transform_target_to_world.wxyz_xyz[0]))
        mine.append(t1)
    for t1, ot in zip(mine + extra, ts):
        e_ref, J_ref = oik.task_error_jacobian(o, ot)
        np.testing.assert_allclose(t1.compute_error(one), e_ref, rtol=0, atol=1e-12 * max(1.0, np.abs(e_ref).max()))
        np.testing.assert_allclose(t1.compute_jacobian(one), J_ref, rtol=0, atol=1e-9 * max(1.0, np.abs(J_ref).max()))


def test_random_trees_ran_on_the_wide_kernel(nat):
    """The public call above does not name its kernel: the same six models through a handle that does."""
    for seed in wc.TREE_SEEDS:
        T = wc.random_tree(seed)
        m = T["m"]
        nm = nat.NativeModel(m)
        fts = [{"frame_type": t, "frame_id": m.name2id(t, n), "cost": list(c), "gain": g, "lm_damping": lm} for n, t, c, g, lm in T["frames"]]
        idx, lower, upper = oik.configuration_limit_arrays(m, oik.ConfigurationLimitSpec(T["cfg_gain"]))
        kw = {}
        ts, ls = wc.tree_specs(T, 0)
        if T["vel"]:
            kw["velocity_limits"] = [{"indices": ls[1].indices, "limit": ls[1].limit}]
        if T["com"] is not None:
            kw["com_tasks"] = [{"cost": list(T["com"][0])}]
        prob = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": T["post"][0], "gain": T["post"][1]}],
                                 configuration_limits=[{"gain": T["cfg_gain"], "lower": lower, "upper": upper, "indices": idx}],
                                 max_batch=len(T["q"]), **kw)
        v, st = prob.solve(T["q"], T["tg"], T["post"][2][None, :], None if T["com"] is None else T["com"][1][None, :], T["dt"], T["damping"])
        assert prob.last_kernel() == WIDE, (seed, prob.last_kernel())
        assert _rel(v, wc.tree_c_oracle(T)[0]).max() <= TOL, seed


# ------------------------------------------------------------------------------------------------ collision rows on a wide-only model
def test_collision_rows_and_the_pair_cull_on_a_wide_only_model(nat):
    """hinge_chain_mjcf(80) with a CollisionAvoidanceLimit over 92 sphere pairs, 3 … 7 of them in range per instance: more than a
    wavefront of pairs, so the bounding-sphere cull runs in front of the distance routines (plan: use_cull, asserted on the
    host), with body poses at a stride beyond 64.  Every instance against the C oracle; the same call without the cull
    (MKH_DIAG_NO_PAIR_CULL) is bitwise equal."""
    H80 = wc.collision_case()
    m, q, tg = H80["m"], H80["q"], H80["tg"]
    assert (m.nv, m.nbody) == (80, 81) and len(wc.HINGE80_PAIRS) > 64

    def build(diag):
        nm = nat.NativeModel(m)
        idx, lower, upper = oik.configuration_limit_arrays(m, oik.ConfigurationLimitSpec(0.95))
        col = {"geom_id_pairs": np.array(wc.HINGE80_PAIRS), "gain": 0.85, "minimum_distance_from_collisions": wc.HINGE80_DMIN,
               "collision_detection_distance": wc.HINGE80_DETECT, "bound_relaxation": 0.0}
        with nat.diag_options(diag):
            return nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "tip"), "cost": list(H80["cost"]),
                                                       "gain": 1.0, "lm_damping": 0.5}],
                                     posture_tasks=[{"cost": 0.05}],
                                     configuration_limits=[{"gain": 0.95, "lower": lower, "upper": upper, "indices": idx}],
                                     velocity_limits=[{"indices": np.arange(m.nv), "limit": np.full(m.nv, 1.0)}],
                                     collision_limits=[col], max_batch=len(q))

    prob = build(0)
    v, st, taps = prob.solve(q, tg, np.array(m.qpos0)[None, :], None, H80["dt"], H80["damping"], taps=["coll_h"])
    assert prob.last_kernel() == WIDE, prob.last_kernel()
    assert ((st & ~1) == 0).all(), np.unique(st, return_counts=True)
    v_c, st_c = wc.collision_c_oracle()
    assert (st_c == 0).all()
    cp = cport.CProblem(m, *wc.collision_specs(H80, 0))
    for i in range(len(q)):
        h_ref = cp.collision_rows(q[i], H80["dt"])[1]
        np.testing.assert_array_equal(np.isfinite(taps["coll_h"][i]), np.isfinite(h_ref))
        fin = np.isfinite(h_ref)
        np.testing.assert_allclose(taps["coll_h"][i][fin], h_ref[fin], rtol=0, atol=1e-10)
    err = _rel(v, v_c)
    v1, st1 = prob.solve(q, tg, np.array(m.qpos0)[None, :], None, H80["dt"], H80["damping"])
    prob_nocull = build(nat.DIAG_NO_PAIR_CULL)
    v2, st2 = prob_nocull.solve(q, tg, np.array(m.qpos0)[None, :], None, H80["dt"], H80["damping"])
    assert prob_nocull.last_kernel() == WIDE
    print("hinge80 + %d pairs (%s in range): max rel |v - C| %.2e" % (len(wc.HINGE80_PAIRS), np.isfinite(taps["coll_h"]).sum(axis=1).tolist(), err.max()))
    assert err.max() <= TOL
    np.testing.assert_array_equal(v1, v)
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(st2, st)
