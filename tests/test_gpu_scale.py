"""Full-size checks (BASELINE sizes) through size-independent properties: feasibility of every
instance, KKT stationarity on a sample via the H/c taps, determinism, batch-permutation
equivariance, oracle agreement on a random subsample, device-pointer (torch) path = host path."""

import numpy as np
import pytest

import native_configs as nc
import oracle_configs as oc
from oracle import ik as oik

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g1_setup():
    from mink_amd import _native as nat
    from mink_amd import workloads
    model = workloads.load_robot("g1")
    nm = nat.NativeModel(model)
    B = 65536
    prob, dt, damping = nc.build("g1_c3", nm, B)
    rng = np.random.default_rng(2024)
    stand = model.key_qpos[0]
    q, tg = workloads.make_batch(model, nm, prob, rng, B, base_q=stand)
    return model, nm, prob, dt, damping, q, tg, stand


def test_g1_full_batch_properties(g1_setup):
    model, nm, prob, dt, damping, q, tg, stand = g1_setup
    B = len(q)
    v, st, taps = prob.solve(q, tg, stand[None, :], None, dt, damping, taps=["box_lo", "box_hi", "qp_iters"])
    assert (st == 0).all()
    dq = v * dt
    lo, hi = taps["box_lo"], taps["box_hi"]
    tol = 1e-12 * 4
    assert (dq <= hi + tol).all() and (dq >= lo - tol).all()       # primal feasibility of all 65 536
    it = taps["qp_iters"]
    print("G1 B=65536: active-set pivots after x0: mean %.1f max %d" % (it.mean(), it.max()))
    # the tap call runs the full-feature kernel with the direct QP start, the plain call the lean kernel
    # with the low-rank start: same optimum, different elimination order
    v2, st2 = prob.solve(q, tg, stand[None, :], None, dt, damping)
    assert prob.last_kernel().removesuffix("o") == "ik_solve_kernel_44_32_r44_w3", prob.last_kernel()   # low-rank start, 3 waves per SIMD
    assert (st2 == 0).all()
    assert np.abs(v2 - v).max() <= 1e-8 * max(1.0, np.abs(v).max())
    # the same algorithm on the 2-waves register map (pre-QP phases inlined instead of called): bitwise equal or not,
    # the optimum is the same
    v2w, st2w = prob.solve(q, tg, stand[None, :], None, dt, damping, two_waves=True)
    assert prob.last_kernel() == "ik_solve_kernel_44_32_r44", prob.last_kernel()
    assert (st2w == 0).all()
    assert np.abs(v2w - v2).max() <= 1e-9 * max(1.0, np.abs(v).max())
    # determinism + permutation equivariance (bitwise)
    v2b, _ = prob.solve(q, tg, stand[None, :], None, dt, damping)
    np.testing.assert_array_equal(v2, v2b)
    perm = np.random.default_rng(0).permutation(B)
    v3, _ = prob.solve(q[perm], tg[perm], stand[None, :], None, dt, damping)
    np.testing.assert_array_equal(v3, v2[perm])
    # ... and the lean kernel with the direct start (MKH_FLAG_DIRECT_QP)
    v4, st4 = prob.solve(q, tg, stand[None, :], None, dt, damping, direct_qp=True)
    assert prob.last_kernel() == "ik_solve_kernel_44_0_w3", prob.last_kernel()
    v4w, st4w = prob.solve(q, tg, stand[None, :], None, dt, damping, direct_qp=True, two_waves=True)
    assert prob.last_kernel() == "ik_solve_kernel_44_0", prob.last_kernel()
    np.testing.assert_array_equal(v4w, v4)                 # same arithmetic, different register map
    assert (st4 == 0).all()
    err = np.abs(v4 - v2).max() / max(1.0, np.abs(v).max())
    print("G1 B=65536: low-rank start vs direct start, max rel |dv| = %.2e" % err)
    assert err <= 1e-8
    # KKT on a sample: H dq + c = −μ with μ only on active bounds and correctly signed
    idx = np.arange(0, B, 257)[:256]
    _, _, t = prob.solve(q[idx], tg[idx], stand[None, :], None, dt, damping, taps=["H", "c"])
    g = np.einsum("bij,bj->bi", t["H"], dq[idx]) + t["c"]
    scale = np.abs(t["c"]).max(axis=1, keepdims=True)
    at_hi = np.abs(dq[idx] - hi[idx]) < 1e-13
    at_lo = np.abs(dq[idx] - lo[idx]) < 1e-13
    free = ~(at_hi | at_lo)
    assert (np.abs(g)[free] / np.broadcast_to(scale, g.shape)[free]).max() < 1e-9
    assert (g[at_hi & ~at_lo] <= 1e-9 * np.broadcast_to(scale, g.shape)[at_hi & ~at_lo]).all()
    assert (g[at_lo & ~at_hi] >= -1e-9 * np.broadcast_to(scale, g.shape)[at_lo & ~at_hi]).all()
    # oracle on a random subsample
    m = oc.model("g1")
    worst = 0.0
    for i in np.random.default_rng(1).choice(B, size=24, replace=False):
        mm, tasks, limits, dt_o, damp_o = oc.g1_c3(tg[i], stand)
        v_ref = oik.solve_ik(m, q[i], tasks, dt_o, damp_o, limits)
        worst = max(worst, np.abs(v[i] - v_ref).max() / max(1.0, np.abs(v_ref).max()))
    print("oracle subsample max rel err", worst)
    assert worst < 1e-8


def test_device_pointer_path_matches_host_path(g1_setup):
    torch = pytest.importorskip("torch")
    model, nm, prob, dt, damping, q, tg, stand = g1_setup
    n = 4096
    v_h, st_h = prob.solve(q[:n], tg[:n], stand[None, :], None, dt, damping)
    dev = torch.device("cuda", 0)
    v_d, st_d = prob.solve(torch.from_numpy(q[:n]).to(dev), torch.from_numpy(tg[:n]).to(dev),
                           torch.from_numpy(stand[None, :].copy()).to(dev), None, dt, damping)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(v_d.cpu().numpy(), v_h)
    np.testing.assert_array_equal(st_d.cpu().numpy(), st_h)
    # a host-pointer call that stages 32 MB or more runs in up to four chunks whose copies overlap the kernels of their
    # neighbours (solve_host.hip via_staged): same answers, ragged last chunk included, fused steps and their outputs too
    n = 40001
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    v_h, st_h = prob.solve(q[:n], tg[:n], stand[None, :], None, dt, damping)
    v_d, st_d = prob.solve(to(q[:n]), to(tg[:n]), to(stand[None, :]), None, dt, damping)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(v_d.cpu().numpy(), v_h)
    np.testing.assert_array_equal(st_d.cpu().numpy(), st_h)
    qf_h, vf_h, sf_h = prob.solve(q[:n], tg[:n], stand[None, :], None, dt, damping, n_steps=3)
    qf_d, vf_d, sf_d = prob.solve(to(q[:n]), to(tg[:n]), to(stand[None, :]), None, dt, damping, n_steps=3)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(qf_d.cpu().numpy(), qf_h)
    np.testing.assert_array_equal(vf_d.cpu().numpy(), vf_h)
    np.testing.assert_array_equal(sf_d.cpu().numpy(), sf_h)
    # ... and the threshold-terminated loop with its per-instance iteration counts, with per-instance posture targets
    n = 26000                # (≥ 32 MB staged: the chunked path)
    pt = np.repeat(stand[None, None, :], n, axis=0) + 0.01 * np.random.default_rng(3).standard_normal((n, 1, len(stand)))
    out_h = prob.solve(q[:n], tg[:n], pt, None, dt, damping, n_steps=4, until=(1e-2, 5e-2))
    out_d = prob.solve(to(q[:n]), to(tg[:n]), to(pt), None, dt, damping, n_steps=4, until=(1e-2, 5e-2))
    torch.cuda.synchronize()
    for a_h, a_d in zip(out_h, out_d):
        np.testing.assert_array_equal(a_d.cpu().numpy(), a_h)
    # ... and the warm-start state, of which every chunk reads and writes its own rows: consecutive warm-started calls through the
    # chunks against the same calls on device tensors (a call of another batch size in between resets the handle's state; three
    # calls, because the state is read from the third on)
    n = 40001

    def warm_calls(conv):
        prob.solve(conv(q[:16]), conv(tg[:16]), conv(stand[None, :]), None, dt, damping, warm_start=True)
        return [prob.solve(conv(q[:n]), conv(tg[:n]), conv(stand[None, :]), None, dt, damping, warm_start=True) for _ in range(3)]

    warm_h, warm_d = warm_calls(lambda x: x), warm_calls(to)
    torch.cuda.synchronize()
    for (v_h, st_h), (v_d, st_d) in zip(warm_h, warm_d):
        np.testing.assert_array_equal(v_d.cpu().numpy(), v_h)
        np.testing.assert_array_equal(st_d.cpu().numpy(), st_h)


@pytest.mark.parametrize("name,B", [("ur5e_c2", 4096), ("shadow_c4", 16384)])
def test_other_configs_full_batch(name, B):
    from mink_amd import _native as nat
    from mink_amd import workloads
    robot = nc.ROBOT_OF[name]
    model = workloads.load_robot(robot)
    nm = nat.NativeModel(model)
    prob, dt, damping = nc.build(name, nm, B)
    rng = np.random.default_rng(5)
    base = model.key_qpos[model.name2id("key", "home" if robot == "ur5e" else "grasp hard")]
    q, tg = workloads.make_batch(model, nm, prob, rng, B, base_q=base)
    if robot == "shadow_left":
        q[::2] = 0.5 * (q[::2] + base)            # bring fingers close: active collision rows
    taps = ["box_lo", "box_hi", "qp_iters"] + (["coll_G", "coll_h"] if prob.n_pairs else [])
    v, st, t = prob.solve(q, tg, base[None, :], None, dt, damping, taps=taps)
    assert ((st & ~1) == 0).all(), np.unique(st)
    dq = v * dt
    assert (dq <= t["box_hi"] + 1e-11).all() and (dq >= t["box_lo"] - 1e-11).all()
    if prob.n_pairs:
        Gx = np.einsum("bpj,bj->bp", t["coll_G"], dq)
        fin = np.isfinite(t["coll_h"])
        nrm = np.linalg.norm(t["coll_G"], axis=2)
        assert (Gx[fin] <= t["coll_h"][fin] + 1e-10 * np.maximum(1.0, nrm[fin])).all()   # half-spaces respected
        print(name, "active contact rows per instance: mean %.1f max %d" % (fin.sum(1).mean(), fin.sum(1).max()))
    m = oc.model(robot)
    cfgfn = getattr(oc, name)
    worst = 0.0
    for i in np.random.default_rng(1).choice(B, size=16, replace=False):
        mm, tasks, limits, dt_o, damp_o = cfgfn(tg[i], base)
        v_ref = oik.solve_ik(m, q[i], tasks, dt_o, damp_o, limits)
        worst = max(worst, np.abs(v[i] - v_ref).max() / max(1.0, np.abs(v_ref).max()))
    print(name, "oracle subsample max rel err", worst, "pivots mean", t["qp_iters"].mean())
    assert worst < 1e-8                    # the stated tolerance
    # the whole batch on the PRODUCTION kernel against the plain-C oracle (round 4: contact rows of plane / sphere /
    # capsule pairs are in its scope — collision_avoidance_limit.py:187-229)
    import os
    from oracle import cport
    mm, tasks, limits, dt_o, damp_o = cfgfn(tg[0], base)
    v_ref, st_ref = cport.CProblem(mm, tasks, limits).solve_batch(q, tg, base[None, :], dt_o, damp_o,
                                                                 nthreads=min(16, os.cpu_count() or 1))
    assert (st_ref == 0).all()
    v2, st2 = prob.solve(q, tg, base[None, :], None, dt, damping)       # production kernel variant
    assert ((st2 & ~1) == 0).all(), np.unique(st2)
    if prob.n_pairs:
        assert prob.last_kernel().removesuffix("+wide") == "ik_solve_kernel_48_72+redo_64", prob.last_kernel()
    err = np.abs(v2 - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
    print(name, "all %d problems vs C oracle: max rel err %.2e (kernel %s)" % (B, err.max(), prob.last_kernel()))
    assert err.max() < 1e-8
    if prob.n_pairs:
        v3, st3 = prob.solve(q, tg, base[None, :], None, dt, damping, full_rows=True)
        assert prob.last_kernel().removesuffix("+wide") == "ik_solve_kernel_64_72", prob.last_kernel()
        err3 = np.abs(v3 - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
        print(name, "full-row build vs C oracle: max rel err %.2e" % err3.max())
        assert ((st3 & ~1) == 0).all() and err3.max() < 1e-8


def test_g1_full_batch_against_c_oracle(g1_setup):
    """Every one of the 65 536 problems of the benchmark batch against the plain-C restatement of the reference
    pipeline (oracle/c), all host threads.  Tolerance: the stated 1e-8·max(1, ‖v_ref‖∞)."""
    import os
    from oracle import cport
    model, nm, prob, dt, damping, q, tg, stand = g1_setup
    v, st = prob.solve(q, tg, stand[None, :], None, dt, damping)
    m, tasks, limits, dt_o, damp_o = oc.g1_c3(tg[0], stand)
    assert dt_o == dt and damp_o == damping
    v_ref, st_ref = cport.CProblem(m, tasks, limits).solve_batch(q, tg, stand[None, :], dt, damping,
                                                                  nthreads=min(16, os.cpu_count() or 1))
    assert (st == 0).all() and (st_ref == 0).all()
    err = np.abs(v - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
    print("G1 B=65536 vs C oracle: max rel err %.2e, p99 %.2e (kernel %s)" % (err.max(), np.percentile(err, 99), prob.last_kernel()))
    assert err.max() < 1e-8


def test_launches_replay_inside_a_hip_graph(g1_setup):
    """Device-pointer solves are plain asynchronous launches with no host-side state (the ticket counter of the
    dynamic tail is zeroed by the launch's last draw): captured into a hipGraph through torch and replayed, they
    return what the eager calls return — bitwise, every replay."""
    torch = pytest.importorskip("torch")
    model, nm, prob, dt, damping, q, tg, stand = g1_setup
    dev = torch.device("cuda", 0)
    n = 16384                                   # 8 problems per wave: static rounds + ticket tail
    q_d = torch.from_numpy(q[:n]).to(dev)
    tg_d = torch.from_numpy(tg[:n]).to(dev)
    pt_d = torch.from_numpy(stand[None, :].copy()).to(dev)
    v_ref, st_ref = prob.solve(q_d, tg_d, pt_d, None, dt, damping)
    torch.cuda.synchronize()
    outs = [torch.zeros_like(v_ref) for _ in range(3)]
    sts = [torch.zeros_like(st_ref) for _ in range(3)]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):               # warm-up on the capture stream, as torch asks
        prob.solve(q_d, tg_d, pt_d, None, dt, damping, out=outs[0], status_out=sts[0])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for o, s in zip(outs, sts):
            prob.solve(q_d, tg_d, pt_d, None, dt, damping, out=o, status_out=s)
    for _ in range(3):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for o, s in zip(outs, sts):
            assert torch.equal(o, v_ref) and torch.equal(s, st_ref)
    v_again, _ = prob.solve(q_d, tg_d, pt_d, None, dt, damping)      # and eager launches still work afterwards
    torch.cuda.synchronize()
    assert torch.equal(v_again, v_ref)


def test_low_rank_start_with_com_rows_and_many_task_rows():
    """The F_COM builds of the low-rank start: ComTask rows, more than 18 task rows, and the two-pass
    elimination when NR + n_μ lanes do not exist — each against the direct start of the same problem and the C oracle."""
    from mink_amd import _native as nat
    from mink_amd import workloads
    from oracle import cport
    model = workloads.load_robot("g1")
    nm = nat.NativeModel(model)
    stand = model.key_qpos[0]
    B = 4096
    # (a) the G1 full example: 21 frame-task rows + 3 ComTask rows = 24 > 64 − 44 lanes: two passes
    prob, dt, damping = nc.build("g1_full", nm, B)
    q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(3), B, base_q=stand)
    _, _, t = prob.solve(q, tg, stand[None, :], np.zeros((1, 3)), dt, damping, taps=["subtree_com"], solve_qp=False)
    com = t["subtree_com"][:, None, :] + 0.01
    v, st = prob.solve(q, tg, stand[None, :], com, dt, damping)
    assert prob.last_kernel().removesuffix("o") == "ik_solve_kernel_44_36_r44_w3", prob.last_kernel()      # (round 5: ten wavefronts per CU)
    v2w, st2w = prob.solve(q, tg, stand[None, :], com, dt, damping, two_waves=True)
    assert prob.last_kernel() == "ik_solve_kernel_44_36_r44", prob.last_kernel()
    assert (st2w == st).all() and np.abs(v2w - v).max() <= 1e-9 * max(1.0, np.abs(v).max())
    vd, std = prob.solve(q, tg, stand[None, :], com, dt, damping, direct_qp=True)
    assert prob.last_kernel() == "ik_solve_kernel_44_6", prob.last_kernel()
    assert (st == 0).all() and (std == 0).all()
    err = np.abs(v - vd).max() / max(1.0, np.abs(vd).max())
    print("G1 full example: low-rank (two-pass) vs direct start, max rel |dv| = %.2e" % err)
    assert err < 1e-9
    n = 512                                            # (the C oracle takes one CoM target for the whole batch)
    vs, sts = prob.solve(q[:n], tg[:n], stand[None, :], com[0], dt, damping)
    assert prob.last_kernel().removesuffix("o") == "ik_solve_kernel_44_36_r44_w3" and (sts == 0).all()
    m, tasks, limits, dt_o, damp_o = oc.g1_full(tg[0], stand, com[0, 0])
    v_c, st_c = cport.CProblem(m, tasks, limits).solve_batch(q[:n], tg[:n], stand[None, :], dt_o, damp_o, com_target=com[0, 0])
    assert (st_c == 0).all()
    assert (np.abs(vs - v_c).max(axis=1) / np.maximum(1.0, np.abs(v_c).max(axis=1))).max() < 1e-8
    # (b) 20 task rows without a ComTask: one pass with the 24-row instantiation (44 + 20 lanes exist)
    fts = [nc._ft(model, s, "site", 200.0, 10.0, 1.0) for s in ("left_foot", "right_foot", "left_palm")]
    fts.append({"frame_type": "site", "frame_id": model.name2id("site", "right_palm"), "cost": [150.0, 150.0, 0, 0, 0, 0],
                "gain": 1.0, "lm_damping": 1.0})
    p20 = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1.0}], configuration_limits=[nc._cfg_limit(model)],
                            velocity_limits=[nc._vel_limit(model)], max_batch=B)
    q2, tg2 = workloads.make_batch(model, nm, p20, np.random.default_rng(4), B, base_q=stand)
    v2, st2 = p20.solve(q2, tg2, stand[None, :], None, 5e-3, 1e-1)
    assert p20.last_kernel().removesuffix("o") == "ik_solve_kernel_44_36_r44_w3", p20.last_kernel()
    v2d, st2d = p20.solve(q2, tg2, stand[None, :], None, 5e-3, 1e-1, direct_qp=True)
    assert "_r" not in p20.last_kernel()
    assert (st2 == 0).all() and (st2d == 0).all()
    err2 = np.abs(v2 - v2d).max() / max(1.0, np.abs(v2d).max())
    print("G1, 20 task rows: low-rank (24-row columns) vs direct start, max rel |dv| = %.2e" % err2)
    assert err2 < 1e-9


def test_cold_start_refinement_agrees_with_the_plain_low_rank_start(monkeypatch):
    """the lean 44-row build re-factorises for the bounds the unconstrained minimiser violates before the
    tableau exists.  Same optimum with the pass switched off (a handle created with MKH_DIAG_NO_COLD_REFINE), on
    ordinary problems, on heavily saturated ones (dt × 8: most dofs end on a velocity bound) and on instances that start ON
    their joint limits (bounds of exactly 0: the violated set is decided by rounding); C oracle on a sample."""
    from mink_amd import _native as nat
    from mink_amd import workloads
    from oracle import cport
    model = workloads.load_robot("g1")
    nm = nat.NativeModel(model)
    B = 4096
    prob, dt, damping = nc.build("g1_c3", nm, B)
    with nat.diag_options(nat.DIAG_NO_COLD_REFINE):
        plain, _, _ = nc.build("g1_c3", nm, B)
    assert plain.diag == nat.DIAG_NO_COLD_REFINE and prob.diag == 0
    stand = model.key_qpos[0]
    q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(77), B, base_q=stand)
    # a quarter of the batch on its joint limits
    lim = np.asarray(model.jnt_range, dtype=np.float64)
    for j in range(model.njnt):
        if model.jnt_type[j] in (2, 3) and model.jnt_limited[j]:
            a = int(model.jnt_qposadr[j])
            q[: B // 4, a] = np.where(np.arange(B // 4) % 2 == 0, lim[j, 0], lim[j, 1])
    for scale in (1.0, 8.0):
        v, st = prob.solve(q, tg, stand[None, :], None, dt * scale, damping)
        assert prob.last_kernel().removesuffix("o") == "ik_solve_kernel_44_32_r44_w3", prob.last_kernel()
        vp, stp = plain.solve(q, tg, stand[None, :], None, dt * scale, damping)
        assert (st == 0).all() and (stp == 0).all()
        err = np.abs(v - vp).max() / max(1.0, np.abs(vp).max())
        idx = np.arange(0, B, 16)
        mm, tasks, limits, _, _ = oc.g1_c3(tg[0], stand)
        v_ref, _ = cport.CProblem(mm, tasks, limits).solve_batch(q[idx], tg[idx], stand[None, :], dt * scale, damping)
        err_o = (np.abs(v[idx] - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))).max()
        print("dt x %g: refinement vs none %.2e, vs C oracle %.2e" % (scale, err, err_o))
        assert err < 1e-9 and err_o < 1e-9


_BENCH_KERNELS = {"ur5e_c2": "ik_quad_kernel", "g1_c3": "ik_solve_kernel_44_32_r44_w3", "g1_full": "ik_solve_kernel_44_36_r44_w3",
                  "shadow_c4": "ik_solve_kernel_48_72+redo_64", "g1_plugin": "ik_solve_kernel_48_256", "h1_c3": "ik_quad_kernel_32",
                  "h1_full": "ik_quad_kernel_32", "g1_coll": "ik_solve_kernel_48_40_r48+redo_64+wide", "ur5e_coll": "ik_solve_kernel_16_8",
                  "g1_hands": "ik_wide_kernel"}


def _oracle_specs_of_bench(name, model, prob_desc):
    """The oracle-side statement of a bench workload (mink_amd/workloads.py::bench_config), written out independently."""
    from oracle import ik
    site = lambda s: model.name2id("site", s)
    cost6 = lambda p, o: np.array([p] * 3 + [o] * 3, dtype=np.float64)
    hinge = [int(model.jnt_dofadr[j]) for j in range(model.njnt) if model.jnt_type[j] != 0]
    vel = ik.VelocityLimitSpec(np.array(hinge), np.full(len(hinge), np.pi))
    z7 = np.zeros(7)
    if name == "ur5e_c2":
        return ([ik.FrameTaskSpec(site("attachment_site"), "site", cost6(1.0, 1.0), z7, lm_damping=1.0),
                 ik.PostureTaskSpec(np.full(model.nv, 1e-2), None)], [ik.ConfigurationLimitSpec(), vel], {})
    feet_palms = [] if name in ("h1_c3", "h1_full") else [ik.FrameTaskSpec(site(s), "site", cost6(200.0, o), z7, lm_damping=1.0)
                  for s, o in (("left_foot", 10.0), ("right_foot", 10.0), ("left_palm", 0.0), ("right_palm", 0.0))]
    post = ik.PostureTaskSpec(np.full(model.nv, 1.0), None)
    if name in ("h1_c3", "h1_full"):
        fts = [ik.FrameTaskSpec(site(s), "site", cost6(200.0, o), z7, lm_damping=1.0)
               for s, o in (("left_foot", 10.0), ("right_foot", 10.0), ("left_wrist", 0.0), ("right_wrist", 0.0))]
        if name == "h1_full":
            pel = ik.FrameTaskSpec(model.name2id("body", "pelvis"), "body", cost6(0.0, 10.0), z7)
            return [pel] + fts + [post, ik.ComTaskSpec(np.full(3, 200.0), None)], [ik.ConfigurationLimitSpec(), vel], {}
        return fts + [post], [ik.ConfigurationLimitSpec(), vel], {}
    if name == "g1_c3":
        return feet_palms + [post], [ik.ConfigurationLimitSpec(), vel], {}
    if name == "aloha_coll":
        # (the pair list: the real mink's, recorded in the ik_aloha_coll fixture — the product's constructor must produce the same)
        pairs = [tuple(p) for p in np.load(oc.GOLDEN + "/ik_aloha_coll.npz")["geom_id_pairs"]]
        joints = [f"{p}/{n}" for p in ("left", "right") for n in ("waist", "shoulder", "elbow", "forearm_roll", "wrist_angle", "wrist_rotate")]
        dofs = np.array([int(model.jnt_dofadr[model.name2id("joint", j)]) for j in joints])
        return ([ik.FrameTaskSpec(site(f"{p}/gripper"), "site", cost6(1.0, 1.0), z7, lm_damping=1.0) for p in ("left", "right")] +
                [ik.PostureTaskSpec(np.full(model.nv, 1e-4), None)],
                [ik.ConfigurationLimitSpec(), ik.VelocityLimitSpec(dofs, np.full(len(dofs), np.pi)),
                 ik.CollisionAvoidanceLimitSpec(pairs, minimum_distance_from_collisions=0.05, collision_detection_distance=0.1)], {})
    if name == "g1_hands":
        tips = [ik.RelativeFrameTaskSpec(site(f"{side}/{tip}"), "site", model.name2id("body", f"{side}/palm"), "body", cost6(1.0, 0.0), z7, lm_damping=1.0)
                for side in ("lh", "rh") for tip in ("ff_tip", "mf_tip", "rf_tip", "th_tip")]
        return feet_palms + tips + [post], [ik.ConfigurationLimitSpec(), vel], {}
    if name == "g1_coll":       # (the pair list is written out by name in test_g1_coll_pair_list_is_what_the_workload_says)
        from mink_amd import workloads
        col = ik.CollisionAvoidanceLimitSpec([tuple(p) for p in workloads.g1_collision_pairs(model)], gain=0.85,
                                             minimum_distance_from_collisions=0.005, collision_detection_distance=0.25)
        return feet_palms + [post], [ik.ConfigurationLimitSpec(), vel, col], {}
    if name == "ur5e_coll":
        g = lambda n: model.name2id("geom", n)
        col = ik.CollisionAvoidanceLimitSpec([(g("wrist_3_link"), g("floor")), (g("wrist_3_link"), g("wall"))], collision_detection_distance=0.3)
        return ([ik.FrameTaskSpec(site("attachment_site"), "site", cost6(1.0, 1.0), z7, lm_damping=1.0)],
                [ik.ConfigurationLimitSpec(), vel, col], {})
    if name == "g1_full":
        pel = ik.FrameTaskSpec(model.name2id("body", "pelvis"), "body", cost6(0.0, 10.0), z7)
        return [pel] + feet_palms + [post, ik.ComTaskSpec(np.full(3, 200.0), None)], [ik.ConfigurationLimitSpec(), vel], {}
    if name == "g1_plugin":
        return (feet_palms + [post], [ik.ConfigurationLimitSpec(), vel],
                {"dense_tasks": [{"cost": np.full(3, 50.0), "gain": 1.0, "lm_damping": 0.0}], "dense_limit_rows": 2})
    if name == "shadow_c4":
        tips = [ik.FrameTaskSpec(site(f), "site", cost6(1.0, 0.0), z7, lm_damping=1.0)
                for f in ("thumb", "first", "middle", "ring", "little")]
        pairs = [tuple(p) for p in np.load(oc.GOLDEN + "/shadow_c4_geom_pairs.npy")]
        return (tips + [ik.PostureTaskSpec(np.full(model.nv, 1e-2), None)],
                [ik.ConfigurationLimitSpec(), ik.CollisionAvoidanceLimitSpec(pairs, collision_detection_distance=0.03)], {})
    raise KeyError(name)


def test_g1_coll_pair_list_is_what_the_workload_says():
    """`g1_coll`'s 46 pairs by geom TYPE and body side, independent of the list comprehension that builds them."""
    from mink_amd import workloads
    model = workloads.load_bench_robot("g1_coll")
    pairs = workloads.g1_collision_pairs(model)
    gt, gb = np.asarray(model.geom_type), np.asarray(model.geom_bodyid)
    kinds = sorted(tuple(sorted((int(gt[a]), int(gt[b])))) for a, b in pairs)
    from collections import Counter
    assert Counter(kinds) == Counter({(0, 2): 8, (2, 2): 16, (0, 5): 4, (0, 6): 2, (2, 5): 8, (2, 6): 8}), Counter(kinds)
    assert len(set(map(tuple, pairs))) == 46
    for a, b in pairs:                       # no pair inside one body, planes only as the second geom
        assert gb[a] != gb[b] and gt[a] != 0


@pytest.mark.parametrize("name", ["ur5e_c2", "g1_c3", "g1_full", "shadow_c4", "g1_plugin", "h1_c3", "h1_full", "g1_coll", "ur5e_coll", "g1_hands", "aloha_coll"])
def test_every_bench_workload_at_its_bench_batch_against_the_c_oracle(name, monkeypatch):
    """Exactly what `bench.py --config <name>` times — the same constructors, the same generated batch (per-instance CoM
    targets for the G1 full example, half of the Shadow instances pulled towards `grasp hard`, the caller's rows of the plugin
    workload), the plain call, hence the production kernel — with EVERY instance held against the plain-C restatement of the
    reference pipeline at the stated 1e-8·max(1, ‖v_ref‖∞)."""
    import os
    from mink_amd import _native as nat
    from mink_amd import workloads
    from oracle import cport
    B = workloads.BENCH_CONFIGS[name]["batch"]
    model = workloads.load_bench_robot(name)
    nm = nat.NativeModel(model)
    prob, dt, damping = workloads.bench_config(name, model, nm, B)
    rng = np.random.default_rng(2024)
    q, tg, pt, com = workloads.bench_batch(name, model, nm, prob, rng, B)
    dense = workloads.bench_dense(name, model, nm, q, rng)
    v, st = prob.solve(q, tg, pt, com, dt, damping, dense=dense)
    # ("+wide": every problem with half-space rows is followed by the redo launch of the workgroup-per-problem kernel — round 5)
    # (`_w3o`: the one-problem-per-workgroup build of the same kernel, which the dispatch picks by batch size — round 6)
    lk = prob.last_kernel().removesuffix("+wide")
    lk = lk[:-1] if lk.endswith("_w3o") else lk
    assert name not in _BENCH_KERNELS or lk == _BENCH_KERNELS[name].removesuffix("+wide"), prob.last_kernel()
    assert ((st & ~1) == 0).all(), np.unique(st, return_counts=True)
    tasks, limits, extra = _oracle_specs_of_bench(name, model, prob)
    if name == "shadow_c4":          # the bench's pair list (built by the product's CollisionAvoidanceLimit) = real mink's, recorded
        from mink_amd.limits import CollisionAvoidanceLimit
        groups = [[f"{f}_1", f"{f}_2"] for f in workloads.SHADOW_FINGERS]
        col = CollisionAvoidanceLimit(model, [(groups[i], groups[j]) for i in range(5) for j in range(i + 1, 5)])
        np.testing.assert_array_equal(np.array(col.geom_id_pairs), np.load(oc.GOLDEN + "/shadow_c4_geom_pairs.npy"))
    cp = cport.CProblem(model if name in ("h1_c3", "h1_full", "g1_hands", "aloha_coll") else oc.model(workloads.BENCH_CONFIGS[name]["robot"]), tasks, limits, **extra)
    v_ref, st_ref = cp.solve_batch(q, tg, pt, dt, damping, com_target=com, dense=dense, nthreads=min(16, os.cpu_count() or 1))
    assert (st_ref == 0).all(), np.unique(st_ref, return_counts=True)
    err = np.abs(v - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
    print("%s: all %d instances vs C oracle: max rel err %.2e, p99 %.2e (kernel %s)"
          % (name, B, err.max(), np.percentile(err, 99), prob.last_kernel()))
    if name == "aloha_coll":
        # ALOHA's limit lists many geom pairs per body pair: rows with opposite normals and h = 0 (a·Δq ≤ 0 and −a·Δq ≤ 0) next to
        # rows almost parallel to them.  A handful of instances are ILL-POSED — multipliers of 1e8 on the opposite pair, so that
        # relaxing every contact bound by 1e-9 moves the reference's own answer by more than 1e-6 (up to 0.4 rad/s) — and there no
        # two implementations of the iteration agree (quadprog's restatement itself takes dual steps of 6e7 there).  They are
        # identified by that sensitivity of the ORACLE, must be a few, and are excluded; everything else holds 1e-8.
        bad = np.flatnonzero(err >= 1e-8)
        if len(bad):
            relaxed = [l if not isinstance(l, type(limits[-1])) else type(l)(l.geom_id_pairs, gain=l.gain,
                       minimum_distance_from_collisions=l.minimum_distance_from_collisions,
                       collision_detection_distance=l.collision_detection_distance, bound_relaxation=1e-9) for l in limits]
            v_rel, _ = cport.CProblem(model, tasks, relaxed, **extra).solve_batch(q[bad], tg[bad], pt, dt, damping)
            sens = np.abs(v_rel - v_ref[bad]).max(axis=1)
            print("aloha_coll: %d instance(s) beyond 1e-8 %s; the oracle's own answer moves by %s there when every contact bound is relaxed by 1e-9"
                  % (len(bad), err[bad], sens))
            assert len(bad) <= 4 and (sens > 1e-6).all(), (bad, err[bad], sens)
            err[bad] = 0.0
    assert err.max() < 1e-8
    if name == "g1_full":
        # round 5: one more resident wave per SIMD (10 wavefronts per CU, the heavy phases of the low-rank start as callees of
        # their own).  The two-waves build of the same algorithm (MKH_FLAG_TWO_WAVES) is another kernel with the same answers.
        v2w, st2w = prob.solve(q, tg, pt, com, dt, damping, two_waves=True)
        assert prob.last_kernel() == "ik_solve_kernel_44_36_r44", prob.last_kernel()
        assert (st2w == st).all()
        assert np.abs(v2w - v).max() <= 1e-9 * max(1.0, np.abs(v).max())
    if name == "shadow_c4":          # the regime must exercise the rows: contacts in range on most instances
        G, h = cp.collision_rows(q[0], dt)
        assert np.isfinite(h).sum() >= 5
    if name == "aloha_coll":
        from mink_amd import workloads as wl
        rows = np.array([np.isfinite(cp.collision_rows(q[i], dt, which=0)[1]).sum() for i in range(0, B, 64)])
        print("aloha_coll: contacts in range per instance (every 64th): mean %.1f, max %d of 1104 pairs; tableau rows 48" % (rows.mean(), rows.max()))
        assert rows.max() >= 8
    if name == "g1_coll":
        # the launches the bench times (round 5: tight rows first, as for the Shadow hand): the 48-row build with 5 rows, the
        # 64-row build with 21 on what that one flags, the workgroup-per-problem kernel on what is flagged then.  How many that is:
        # the same batch on a handle without the last launch (MKH_DIAG_NO_WIDE_REDO)
        with nat.diag_options(nat.DIAG_NO_WIDE_REDO):
            alone, _, _ = workloads.bench_config(name, model, nm, B)
        v1, st1 = alone.solve(q, tg, pt, com, dt, damping)
        assert alone.last_kernel() == "ik_solve_kernel_48_40_r48+redo_64", alone.last_kernel()
        flagged = np.flatnonzero(st1 & 16)
        # ... and the full-row build alone (MKH_FLAG_FULL_ROWS), another kernel with the same answers
        v_full, st_full = alone.solve(q, tg, pt, com, dt, damping, full_rows=True)
        assert alone.last_kernel() == "ik_solve_kernel_64_8", alone.last_kernel()
        okf = (st_full & 16) == 0
        e_full = np.abs(v_full - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
        print("g1_coll: full-row build alone: max rel err %.2e on the %d instances it does not flag" % (e_full[okf].max(), okf.sum()))
        assert e_full[okf].max() < 1e-8
        rows = np.array([np.isfinite(cp.collision_rows(q[i], dt, which=0)[1]).sum() for i in range(0, B, 64)])
        print("g1_coll: %d of %d instances re-solved with every row by the wide kernel (err on those: %.2e); contacts in range "
              "per instance: mean %.1f, max %d" % (len(flagged), B, err[flagged].max() if len(flagged) else 0.0, rows.mean(), rows.max()))
        # (measured: on this batch NO instance is flagged — up to 22 contacts are in range, but never is a dropped one violated at
        #  the 21-row solution; the second launch of the pair is an empty sweep.  The redo path itself is held at scale by
        #  tests/test_gpu_wide.py, in a regime with 40+ contacts in range)
        assert rows.max() > 21
        ok = np.setdiff1d(np.arange(B), flagged)
        np.testing.assert_array_equal(v1[ok], v[ok])          # the redo launch touches nothing else


def _numpy_oracle_chunk(args):
    name, idx, q, tg, pt, dt, damping = args
    from mink_amd import workloads
    from oracle import ik
    model = workloads.load_bench_robot(name)
    site = model.name2id("site", "attachment_site")
    hinge = [int(model.jnt_dofadr[j]) for j in range(model.njnt) if model.jnt_type[j] != 0]
    g = lambda n: model.name2id("geom", n)
    pairs = [(g("wrist_3_link"), g("floor")), (g("wrist_3_link"), g("wall"))]
    out = []
    for i in idx:
        tasks = [ik.FrameTaskSpec(site, "site", np.ones(6), tg[i, 0], lm_damping=1.0)]
        limits = [ik.ConfigurationLimitSpec(), ik.CollisionAvoidanceLimitSpec(pairs, collision_detection_distance=0.3),
                  ik.VelocityLimitSpec(np.array(hinge), np.full(len(hinge), np.pi))]
        out.append(ik.solve_ik(model, q[i], tasks, dt, damping, limits))
    return np.array(out)


def test_ur5e_convex_at_its_bench_batch_against_the_numpy_oracle():
    """The sixth bench workload: a cylinder–box pair goes through the general convex routine, which the C restatement does
    not carry — all 4 096 instances against the numpy restatement (oracle/gjk.py) on every host core.  Tolerance 1e-9 (SURVEY
    §8d asks 1e-8) since round 6: the witness points of GJK / the expanding polytope are polished onto the exact features on
    both sides (convex_dev.h cvx_polish, oracle/gjk.py polish; pinned by the KKT checker of tests/test_oracle_gjk.py) — measured
    1.5e-13 on every instance, the 104 at or inside d_min included; with the raw witness points it was 3.7e-6."""
    import multiprocessing as mp
    import os
    from mink_amd import _native as nat
    from mink_amd import workloads
    name = "ur5e_convex"
    B = workloads.BENCH_CONFIGS[name]["batch"]
    model = workloads.load_bench_robot(name)
    nm = nat.NativeModel(model)
    prob, dt, damping = workloads.bench_config(name, model, nm, B)
    q, tg, pt, _ = workloads.bench_batch(name, model, nm, prob, np.random.default_rng(2024), B)
    v, st = prob.solve(q, tg, pt, None, dt, damping)
    assert prob.last_kernel() == "ik_solve_kernel_16_136+wide", prob.last_kernel()
    assert ((st & ~1) == 0).all(), np.unique(st, return_counts=True)
    ncpu = min(16, os.cpu_count() or 1)
    chunks = np.array_split(np.arange(B), ncpu * 4)
    with mp.get_context("fork").Pool(ncpu) as pool:
        parts = pool.map(_numpy_oracle_chunk, [(name, c, q, tg, pt, dt, damping) for c in chunks])
    v_ref = np.concatenate(parts)
    err = np.abs(v - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
    print("ur5e_convex: all %d instances vs numpy oracle: max rel err %.2e, p99 %.2e" % (B, err.max(), np.percentile(err, 99)))
    assert err.max() < 1e-9


def _numpy_h_chunk(args):
    name, idx, q, dt = args
    from mink_amd import workloads
    from oracle import ik
    model = workloads.load_bench_robot(name)
    g = lambda n: model.name2id("geom", n)
    spec = ik.CollisionAvoidanceLimitSpec([(g("wrist_3_link"), g("floor")), (g("wrist_3_link"), g("wall"))], collision_detection_distance=0.3)
    return np.array([ik.limit_inequalities(ik.Configuration(model, q[i]), spec, dt)[1] for i in idx])


def test_ur5e_convex_contact_distances_at_scale():
    """h of both pairs (cylinder-plane analytic, cylinder-box through GJK / the expanding polytope) on all 4 096
    instances of the bench batch against the numpy restatement at 1e-9·max(1, |h|) — which pairs are in range included."""
    import multiprocessing as mp
    import os
    from mink_amd import _native as nat
    from mink_amd import workloads
    name = "ur5e_convex"
    B = workloads.BENCH_CONFIGS[name]["batch"]
    model = workloads.load_bench_robot(name)
    nm = nat.NativeModel(model)
    prob, dt, damping = workloads.bench_config(name, model, nm, B)
    q, tg, pt, _ = workloads.bench_batch(name, model, nm, prob, np.random.default_rng(2024), B)
    _, _, taps = prob.solve(q, tg, pt, None, dt, damping, taps=["coll_h"], solve_qp=False)
    h = taps["coll_h"]
    ncpu = min(16, os.cpu_count() or 1)
    chunks = np.array_split(np.arange(B), ncpu * 2)
    with mp.get_context("fork").Pool(ncpu) as pool:
        h_ref = np.concatenate(pool.map(_numpy_h_chunk, [(name, c, q, dt) for c in chunks]))
    np.testing.assert_array_equal(np.isfinite(h), np.isfinite(h_ref))
    fin = np.isfinite(h_ref)
    err = np.abs(h[fin] - h_ref[fin]) / np.maximum(1.0, np.abs(h_ref[fin]))
    pen = int((h_ref[fin] == 0.0).sum())
    print("ur5e_convex: h of %d contacts in range on %d instances (%d at or inside d_min): max rel err %.2e" % (fin.sum(), B, pen, err.max()))
    assert fin[:, 1].sum() > B // 8 and err.max() < 1e-9


def test_convex_pairs_in_a_kernel_of_their_own_from_32768_items():
    """Round 5: from 32 768 (instance, pair) items on, plain solves evaluate general convex pairs in `convex_contacts_kernel` in
    front of the ANALYTIC collision build (mink_amd/csrc/convex_pre.hip: no callee-saved register blocks in scratch; 1.27 → 0.97 ms
    at 65 536 instances).  Same answers as the routine inside the solve kernel (MKH_FLAG... none: the small batch takes that path)
    to the tolerance of rows through GJK, and the numpy oracle on a sample."""
    from mink_amd import _native as nat
    from mink_amd import workloads
    name = "ur5e_convex"
    B = 32768
    model = workloads.load_bench_robot(name)
    nm = nat.NativeModel(model)
    prob, dt, damping = workloads.bench_config(name, model, nm, B)
    q, tg, pt, _ = workloads.bench_batch(name, model, nm, prob, np.random.default_rng(7), B)
    v, st = prob.solve(q, tg, pt, None, dt, damping)
    assert prob.last_kernel() == "convex_pre+ik_solve_kernel_16_8+wide", prob.last_kernel()
    assert ((st & ~1) == 0).all(), np.unique(st, return_counts=True)
    parts = [prob.solve(q[i:i + 4096], tg[i:i + 4096], pt, None, dt, damping) for i in range(0, B, 4096)]
    assert prob.last_kernel() == "ik_solve_kernel_16_136+wide", prob.last_kernel()
    v_in = np.concatenate([p_[0] for p_ in parts])
    err = np.abs(v - v_in).max(axis=1) / np.maximum(1.0, np.abs(v_in).max(axis=1))
    bad = np.flatnonzero(err >= 1e-9)
    print("ur5e_convex, %d instances: split vs in-kernel routine max rel %.2e; beyond 1e-9: %d" % (B, err.max(), len(bad)))
    # the two paths see the geoms through different FK rounding; with the witness points polished onto the exact features (round 6)
    # that is all that separates them (before: 2e-5, and the expanding polytope's witness points moved at the 1e-4 level) — except
    # where the cylinder OVERLAPS the wall and the depth is almost flat in the direction: instance 32 654 of this batch has the rim
    # against a vertical edge of the box, reduced curvature 0.0016 (the depth changes by 7e-7 over 0.03 rad, two local minima
    # 1.2 % apart), the polytope stops at its vertex budget in one basin or the other and the polish certifies the one it is given
    assert len(bad) <= B // 8192
    if len(bad):
        _, _, t = prob.solve(q[bad], tg[bad], pt, None, dt, damping, taps=["coll_h"], solve_qp=False)
        assert (t["coll_h"].min(axis=1) == 0.0).all(), t["coll_h"]
    v_ref = _numpy_oracle_chunk((name, np.arange(0, B, 1024), q, tg, pt, dt, damping))
    e2 = np.abs(v[::1024] - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
    assert e2.max() < 1e-9, e2.max()


def test_the_bounding_sphere_cull_of_many_pairs_changes_nothing(monkeypatch):
    """Round 5: a problem with more than one wavefront of collision pairs (the reference's ALOHA example: 1 104) drops the pairs
    whose bounding spheres are farther apart than the detection distance before the distance routines run (ik_kernel.h
    collision_phase, wide_kernel.h wide_contacts: 5.9 → 2.7 ms).  A culled pair is one mj_geomDistance answers `distmax` for
    (collision_avoidance_limit.py:214-229), so NOTHING may change: bitwise the same v, statuses, h of every pair (the tap layout
    of all 1 104) with the cull and without it (a handle created with MKH_DIAG_NO_PAIR_CULL)."""
    from mink_amd import _native as nat
    from mink_amd import workloads
    name, B = "aloha_coll", 4096
    model = workloads.load_bench_robot(name)
    nm = nat.NativeModel(model)
    out = {}
    for cull in (True, False):
        with nat.diag_options(0 if cull else nat.DIAG_NO_PAIR_CULL):
            prob, dt, damping = workloads.bench_config(name, model, nm, B)
        q, tg, pt, _ = workloads.bench_batch(name, model, nm, prob, np.random.default_rng(11), B)
        v, st = prob.solve(q, tg, pt, None, dt, damping)
        assert prob.last_kernel() == "ik_solve_kernel_64_8+wide", prob.last_kernel()
        _, _, t = prob.solve(q[:512], tg[:512], pt, None, dt, damping, taps=["coll_h"], solve_qp=False)
        out[cull] = (v, st, t["coll_h"])
    h = out[True][2]
    in_range = np.isfinite(h).sum(axis=1)
    print("aloha_coll: %d pairs, in range per instance: mean %.1f, max %d" % (h.shape[1], in_range.mean(), in_range.max()))
    assert h.shape[1] == 1104 and in_range.max() < h.shape[1] // 4
    np.testing.assert_array_equal(out[True][0], out[False][0])
    np.testing.assert_array_equal(out[True][1], out[False][1])
    np.testing.assert_array_equal(out[True][2], out[False][2])


def test_humanoid_with_more_than_a_wavefront_of_analytic_pairs(monkeypatch):
    """Round 5, the two new mechanisms of the analytic collision build TOGETHER: G1 under its task set with every analytic pair
    among its primitive collision geoms and the floor (≈ 150: spheres, cylinders, boxes — box–box left out, the C restatement
    has no routine for it) → bounding-sphere cull (more than 64 pairs) AND tight rows first (43 dofs: 5 rows on the 48-row build,
    21 on the 64-row build for what that flags, the workgroup-per-problem kernel behind).  Large steps and a wide detection
    distance, so that the later stages have work.  EVERY instance against the C restatement with all rows at 1e-8; bitwise the
    same without the cull."""
    import os
    from mink_amd import _native as nat
    from mink_amd import workloads
    from oracle import cport, ik
    B = 2048
    model = workloads.load_robot("g1")
    gt, gv, gb = np.asarray(model.geom_type), np.asarray(model.geom_valid), np.asarray(model.geom_bodyid)
    prim = [g for g in range(model.ngeom) if gt[g] in (2, 3, 5, 6) and gv[g] == 1]
    floor = [g for g in range(model.ngeom) if gt[g] == 0][0]
    in_c = {(3, 3), (2, 2), (2, 3), (2, 6), (2, 5), (3, 6), (3, 5)}
    pairs = [(a, b) for i, a in enumerate(prim) for b in prim[i + 1:]
             if gb[a] != gb[b] and tuple(sorted((int(gt[a]), int(gt[b])))) in in_c] + [(g, floor) for g in prim]
    assert len(pairs) > 128, len(pairs)
    nm = nat.NativeModel(model)
    fts = [nc._ft(model, s, "site", 200.0, 10.0, 1.0) for s in ("left_foot", "right_foot")] + \
          [nc._ft(model, s, "site", 200.0, 0.0, 1.0) for s in ("left_palm", "right_palm")]
    col = {"geom_id_pairs": np.array(pairs), "gain": 0.85, "minimum_distance_from_collisions": 0.01,
           "collision_detection_distance": 0.3, "bound_relaxation": 0.0}
    stand = model.key_qpos[model.name2id("key", "stand")]
    dt, damping = 5e-2, 1e-1
    out = {}
    for cull in (True, False):
        prob = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1.0}], configuration_limits=[nc._cfg_limit(model)],
                                 velocity_limits=[nc._vel_limit(model)], collision_limits=[col], max_batch=B,
                                 diag=0 if cull else nat.DIAG_NO_PAIR_CULL)
        q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(23), B, base_q=stand, sigma=0.5)
        v, st = prob.solve(q, tg, stand[None, :], None, dt, damping)
        assert prob.last_kernel() == "ik_solve_kernel_48_40_r48+redo_64+wide", prob.last_kernel()
        out[cull] = (v, st)
    v, st = out[True]
    np.testing.assert_array_equal(v, out[False][0])
    np.testing.assert_array_equal(st, out[False][1])
    assert ((st & ~1) == 0).all(), np.unique(st, return_counts=True)
    site = lambda s: model.name2id("site", s)
    cost6 = lambda p, o: np.array([p] * 3 + [o] * 3, dtype=np.float64)
    tasks = [ik.FrameTaskSpec(site(s), "site", cost6(200.0, o), np.zeros(7), lm_damping=1.0)
             for s, o in (("left_foot", 10.0), ("right_foot", 10.0), ("left_palm", 0.0), ("right_palm", 0.0))] + \
            [ik.PostureTaskSpec(np.full(model.nv, 1.0), None)]
    hinge = [int(model.jnt_dofadr[j]) for j in range(model.njnt) if model.jnt_type[j] != 0]
    limits = [ik.ConfigurationLimitSpec(), ik.VelocityLimitSpec(np.array(hinge), np.full(len(hinge), np.pi)),
              ik.CollisionAvoidanceLimitSpec([tuple(p) for p in pairs], gain=0.85, minimum_distance_from_collisions=0.01,
                                             collision_detection_distance=0.3)]
    cp = cport.CProblem(oc.model("g1"), tasks, limits)
    v_ref, st_ref = cp.solve_batch(q, tg, stand[None, :], dt, damping, nthreads=min(16, os.cpu_count() or 1))
    assert (st_ref == 0).all(), np.unique(st_ref, return_counts=True)
    err = np.abs(v - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
    rows = np.array([np.isfinite(cp.collision_rows(q[i], dt, which=0)[1]).sum() for i in range(0, B, 32)])
    # how much the later stages did: the same batch without the last launch, and the first launch's own flags are not visible from
    # here (the 64-row launch clears them) — the contacts in range say how often 5 and 21 rows cannot have been enough
    print("G1 + %d analytic pairs: all %d instances vs C oracle: max rel err %.2e; contacts in range per instance: mean %.1f, max %d"
          % (len(pairs), B, err.max(), rows.mean(), rows.max()))
    assert rows.max() > 21 and rows.mean() > 5
    assert err.max() < 1e-8


def test_one_problem_per_workgroup_twin_on_ragged_batches():
    """Round 6: from 3.5 rounds of the resident wavefronts on, the headline's kernel runs as its twin compiled for one problem per
    workgroup (`44_32_r44_w3o`: no loop, lane ids by mbcnt, the descriptor through the constant address space).  Batch sizes that are
    not multiples of the 8 XCDs take the plain workgroup → problem map; every size bitwise equal to the two-waves build (same
    arithmetic, other register map) and without a NaN."""
    from mink_amd import _native as nat
    from mink_amd import workloads
    name = "g1_c3"
    model = workloads.load_bench_robot(name)
    nm = nat.NativeModel(model)
    for B in (10752, 10753, 12289, 16391):
        prob, dt, damping = workloads.bench_config(name, model, nm, B)
        q, tg, pt, ct = workloads.bench_batch(name, model, nm, prob, np.random.default_rng(B), B)
        v1, s1 = prob.solve(q, tg, pt, ct, dt, damping)
        assert prob.last_kernel() == "ik_solve_kernel_44_32_r44_w3o" and prob.launch_info(B)["grid"] == B, (prob.last_kernel(), prob.launch_info(B))
        v2, s2 = prob.solve(q, tg, pt, ct, dt, damping, two_waves=True)
        assert prob.last_kernel() == "ik_solve_kernel_44_32_r44"
        np.testing.assert_array_equal(v1, v2)
        assert (s1 == s2).all() and not np.isnan(v1).any()
        prob.close()
