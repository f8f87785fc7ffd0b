"""The low-rank start with the host's lane tables (docs/HISTORY.md "Low-rank start: model constants out of the solve"): the
product lanes walk a packed list of their column's dofs instead of the bits of its chain mask, the right-hand side's place in
its chunk and the "every joint at its body's origin" flag come from the descriptor.  Every instance of every case against the
plain-C oracle and against the direct QP start (MKH_FLAG_DIRECT_QP) at the project's 1e-8·max(1, ‖v_ref‖∞), failure bits as the
oracle's, `last_kernel()` asserted so that each case names the build it ran on.  Batches of 64.

  (a) G1 with the bench task set: chains of 12 and 13 + 6 dofs in one problem — short lanes walk padding entries
  (b) serial chains of 16 dofs (a full list), 17 and 40 (past the capacity: the mask walk, on a small and on the headline-size
      build) and 63 (no spare lane, no low-rank build: the direct start)
  (c) row-mask gaps: position-only, orientation-only and 0b101101 on two tasks; 13 rows = chunks of 4 with the right-hand
      side alone in the last one
  (d) a predicted active set takes the mask walk: MKH_FLAG_WARM_START on a handle with history, a fused loop of 4 steps
  (e) the anchor flag: a chain with every joint at its body's origin, the same with one hinge moved (a body with two joints
      in both); body poses by tap
  (f) `g1_coll`: contact rows next to the low-rank start (their columns of Jh behind the dofs start from the filled zero)

The fixtures and their references are made on the CPU (tests/wood_list_cases.py; tests/test_wood_list_cases_cpu.py holds them
against the second oracle)."""

import re

import numpy as np
import pytest

import native_configs as nc
import wood_list_cases as wl
from oracle import ik as oik

pytestmark = pytest.mark.gpu

_nmodels = {}


def _nmodel(c):
    from mink_amd import _native as nat
    if id(c.model) not in _nmodels:
        _nmodels[id(c.model)] = nat.NativeModel(c.model)
    return _nmodels[id(c.model)]


def _problem(c, max_batch=wl.B):
    from mink_amd import _native as nat
    from mink_amd import workloads
    nm, m = _nmodel(c), c.model
    if c.collision is not None:                      # the bench workload's own constructor (46 analytic pairs)
        prob, dt, damping = workloads.bench_config("g1_coll", m, nm, max_batch)
        assert (dt, damping) == (c.dt, c.damping)
        return prob
    fts = [{"frame_type": f.kind, "frame_id": m.name2id(f.kind, f.name), "cost": list(f.cost), "gain": 1.0,
            "lm_damping": f.lm_damping} for f in c.frames]
    return nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": c.posture_cost}],
                             configuration_limits=[nc._cfg_limit(m)], velocity_limits=[nc._vel_limit(m)], max_batch=max_batch)


def _rel(v, v_ref):
    return np.abs(v - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))


def _check(name, prob=None, **flags):
    """One plain solve of a case on the wavefront kernel: the build, the failure bits, every instance against the C oracle and
    against the direct start.  Returns (v, kernel)."""
    c = wl.case(name)
    v_ref, st_ref = wl.reference(name)
    prob = prob or _problem(c)
    v, st = prob.solve(c.q, c.frame_targets, c.posture_target, None, c.dt, c.damping, wave_kernel=True, **flags)
    kernel = prob.last_kernel()
    assert kernel.startswith(c.kernel), (name, kernel)
    np.testing.assert_array_equal((st & wl.FAILURE_BITS) != 0, st_ref != 0)          # (the oracle solves every instance)
    err = _rel(v, v_ref)
    vd, std = prob.solve(c.q, c.frame_targets, c.posture_target, None, c.dt, c.damping, wave_kernel=True, direct_qp=True)
    assert not re.search(r"_r\d+", prob.last_kernel()), (name, prob.last_kernel())    # no low-rank build
    assert ((std & wl.FAILURE_BITS) == 0).all(), name
    errd = _rel(v, vd)
    print("%s: %d instances on %s: max rel err vs C oracle %.2e, vs direct start (%s) %.2e"
          % (name, len(v), kernel, err.max(), prob.last_kernel(), errd.max()))
    assert err.max() < 1e-8, (name, err.max(), int(err.argmax()))
    assert errd.max() < 1e-8, (name, errd.max(), int(errd.argmax()))
    return v, kernel


def test_chains_of_different_lengths_in_one_problem():
    """(a)"""
    _check("g1_bench")


@pytest.mark.parametrize("n", [16, 17, 40, 63])
def test_chains_around_the_list_capacity(n):
    """(b)"""
    _check("chain%d" % n)


@pytest.mark.parametrize("name", ["rows_pos_ori", "rows_ori_gaps", "rows_gaps_pos", "rows_13"])
def test_row_mask_gaps(name):
    """(c)"""
    c = wl.case(name)
    prob = _problem(c)
    assert prob.n_rows >= 0
    _check(name, prob)


def test_warm_start_across_calls_takes_the_predicted_set():
    """(d) the third call of a handle reads what the first left (a state at least two solves old)."""
    c = wl.case("g1_bench")
    v_ref, _ = wl.reference("g1_bench")
    prob = _problem(c)
    for call in range(3):
        v, st = prob.solve(c.q, c.frame_targets, c.posture_target, None, c.dt, c.damping, warm_start=True)
        assert prob.last_kernel().startswith(c.kernel), prob.last_kernel()
        assert ((st & wl.FAILURE_BITS) == 0).all()
        err = _rel(v, v_ref)
        print("warm-started call %d: max rel err vs C oracle %.2e" % (call, err.max()))
        assert err.max() < 1e-8, (call, err.max(), int(err.argmax()))


def test_fused_loop_of_four_steps():
    """(d) steps 3 and 4 start from the previous step's active set.  Against the host-driven loop and the oracle's loop, with
    the bounds of tests/test_gpu_two_row_loop.py."""
    c = wl.case("g1_bench")
    nm = _nmodel(c)
    prob = _problem(c)
    K = 4
    qK, vK, st = prob.solve(c.q, c.frame_targets, c.posture_target, None, c.dt, c.damping, n_steps=K)
    assert prob.last_kernel().startswith("ik_solve_kernel_44_48_r44_w3"), prob.last_kernel()
    assert ((st & wl.FAILURE_BITS) == 0).all()
    q = c.q.copy()
    for _ in range(K):
        v, _ = prob.solve(q, c.frame_targets, c.posture_target, None, c.dt, c.damping)
        q = nm.integrate(q, v, c.dt)
    np.testing.assert_allclose(qK, q, rtol=0, atol=1e-10)
    np.testing.assert_allclose(vK, v, rtol=0, atol=1e-9 * max(1.0, np.abs(v).max()))
    for i in (0, 17, 63):
        cfg = oik.Configuration(c.oracle_model, c.q[i])
        tasks, limits = wl.oracle_tasks(c, i)
        for _ in range(K):
            v_o = oik.solve_ik(c.oracle_model, cfg, tasks, c.dt, c.damping, limits)
            cfg.update(cfg.integrate(v_o, c.dt))
        np.testing.assert_allclose(qK[i], cfg.q, rtol=0, atol=1e-10)
        np.testing.assert_allclose(vK[i], v_o, rtol=0, atol=1e-7 * max(1.0, np.abs(v_o).max()))


def test_joint_anchor_flag_on_and_off():
    """(e)"""
    v_zero, _ = _check("anchors_zero")
    v_moved, _ = _check("anchors_moved")
    assert np.abs(v_zero - v_moved).max() > 1e-6             # the moved hinge matters: the flag must be off for that model
    for name in ("anchors_zero", "anchors_moved"):
        c = wl.case(name)
        prob = _problem(c)
        _, _, t = prob.solve(c.q[:4], c.frame_targets[:4], c.posture_target, None, c.dt, c.damping, taps=["xpos", "xquat"],
                             wave_kernel=True)
        # (taps come from the all-feature build, whose kinematics do not read the flag: what the poses of both models ARE —
        #  the low-rank builds answer for them through v above)
        assert prob.last_kernel().startswith("ik_solve_kernel_"), prob.last_kernel()
        for i in range(4):
            d = oik.Configuration(c.oracle_model, c.q[i]).data
            assert np.abs(t["xpos"][i] - d.xpos).max() <= 1e-12 * max(1.0, np.abs(d.xpos).max()), (name, i)
            dq = np.minimum(np.abs(t["xquat"][i] - d.xquat), np.abs(t["xquat"][i] + d.xquat)).max()   # (q and −q: one rotation)
            assert dq <= 1e-12, (name, i, dq)


def test_contact_rows_next_to_the_low_rank_start():
    """(f)"""
    _check("g1_coll")
