"""The paths of the headline G1 kernel (`ik_solve_kernel_44_32_r44_w3o`, one problem per workgroup) that its elimination
splits: every instance of every batch against the plain-C oracle and against the direct QP start (MKH_FLAG_DIRECT_QP), both at
the project's 1e-8·max(1, ‖v_ref‖∞), with `last_kernel()` asserted so that each case names the build it ran on.

  (i)   the bench task set: 18 task rows = the elimination's compiled capacity (every step guard true)
  (ii)  the same without the right-palm task: 15 rows < capacity (guards false for the last three steps, same build)
  (iii) targets = the current frame poses, posture target = q: x⁰ = 0 violates no bound, the refinement pass is skipped
  (iv)  dt ten times smaller: nearly every limited hinge saturates (large violated set in the refinement pass)
  (v)   ragged batch sizes on both sides of the launch-shape switch (3.5 rounds of the resident wavefronts) and 16 384 + 1

Inputs are seeded and generated here; each case also checks that its inputs do what they are for (the oracle solves every
instance, and the bounds active at the oracle's optimum are many / none as the case needs)."""

import os

import numpy as np
import pytest

import native_configs as nc
import oracle_configs as oc
from oracle import ik

pytestmark = pytest.mark.gpu

TWIN = "ik_solve_kernel_44_32_r44_w3o"
PERSISTENT = "ik_solve_kernel_44_32_r44_w3"
SITES = ("left_foot", "right_foot", "left_palm", "right_palm")
B_TWIN = 12288            # 4 rounds of the resident wavefronts: above the switch, the twin runs


@pytest.fixture(scope="module")
def g1():
    from mink_amd import _native as nat
    from mink_amd import workloads
    model = workloads.load_robot("g1")
    return model, nat.NativeModel(model), model.key_qpos[model.name2id("key", "stand")]


def _native_problem(nm, sites, max_batch):
    from mink_amd import _native as nat
    m = nm.model
    fts = [nc._ft(m, s, "site", 200.0, 10.0 if s.endswith("foot") else 0.0, 1.0) for s in sites]
    return nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1.0}], configuration_limits=[nc._cfg_limit(m)],
                             velocity_limits=[nc._vel_limit(m)], max_batch=max_batch)


def _oracle_problem(sites, frame_targets0, posture_target):
    from oracle import cport
    m = oc.model("g1")
    tasks = [ik.FrameTaskSpec(m.name2id("site", s), "site", oc._cost6(200.0, 10.0 if s.endswith("foot") else 0.0),
                              frame_targets0[k], lm_damping=1.0) for k, s in enumerate(sites)]
    tasks.append(ik.PostureTaskSpec(np.full(m.nv, 1.0), posture_target))
    return cport.CProblem(m, tasks, [ik.ConfigurationLimitSpec(), oc._hinge_velocity_limit(m)])


def _active_bounds(prob, q, tg, pt, dt, damping, v_ref):
    """Per instance: how many box bounds the oracle's optimum sits on (bounds from the kernel's own taps)."""
    _, _, taps = prob.solve(q, tg, pt, None, dt, damping, taps=["box_lo", "box_hi"])
    dq = v_ref * dt
    tol = 1e-9
    return ((np.abs(dq - taps["box_hi"]) <= tol) | (np.abs(dq - taps["box_lo"]) <= tol)).sum(axis=1), taps


def _check(prob, sites, q, tg, pt, dt, damping, kernel, label):
    v, st = prob.solve(q, tg, pt, None, dt, damping)
    assert prob.last_kernel() == kernel, (label, prob.last_kernel())
    assert (st == 0).all(), (label, np.unique(st, return_counts=True))
    cp = _oracle_problem(sites, tg[0], pt[0] if pt.ndim == 2 else pt[0, 0])
    v_ref, st_ref = cp.solve_batch(q, tg, pt, dt, damping, nthreads=min(16, os.cpu_count() or 1))
    assert (st_ref == 0).all(), (label, np.unique(st_ref, return_counts=True))       # the oracle alone solves all of them
    err = np.abs(v - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
    vd, std = prob.solve(q, tg, pt, None, dt, damping, direct_qp=True)
    assert "_r44" not in prob.last_kernel(), (label, prob.last_kernel())             # the direct start: no low-rank build
    assert (std == 0).all(), label
    errd = np.abs(v - vd).max(axis=1) / np.maximum(1.0, np.abs(vd).max(axis=1))
    print("%s: %d instances on %s: max rel err vs C oracle %.2e, vs direct start %.2e" % (label, len(q), kernel, err.max(), errd.max()))
    assert err.max() < 1e-8, (label, err.max(), int(err.argmax()))                   # EVERY instance
    assert errd.max() < 1e-8, (label, errd.max(), int(errd.argmax()))
    return v_ref


def _batch(g1, prob, B, seed):
    from mink_amd import workloads
    model, nm, stand = g1
    q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(seed), B, base_q=stand)
    return q, tg, stand[None, :]


def test_full_capacity_elimination(g1):
    """(i) 18 rows = K."""
    _, nm, _ = g1
    prob = _native_problem(nm, SITES, B_TWIN)
    q, tg, pt = _batch(g1, prob, B_TWIN, 901)
    v_ref = _check(prob, SITES, q, tg, pt, 5e-3, 1e-1, TWIN, "(i) bench task set")
    act, _ = _active_bounds(prob, q, tg, pt, 5e-3, 1e-1, v_ref)
    print("(i) bounds active at the optimum: mean %.1f" % act.mean())
    assert act.mean() > 5.0                    # a saturated workload: the refinement pass has a violated set to work on


def test_guarded_elimination_with_fewer_rows(g1):
    """(ii) 15 rows < K on the same build."""
    _, nm, _ = g1
    sites = SITES[:3]
    prob = _native_problem(nm, sites, B_TWIN)
    assert prob.n_frame == 3
    q, tg, pt = _batch(g1, prob, B_TWIN, 902)
    v_ref = _check(prob, sites, q, tg, pt, 5e-3, 1e-1, TWIN, "(ii) without the right-palm task")
    act, _ = _active_bounds(prob, q, tg, pt, 5e-3, 1e-1, v_ref)
    print("(ii) bounds active at the optimum: mean %.1f" % act.mean())
    assert act.mean() > 5.0


def test_refinement_pass_skipped(g1):
    """(iii) nothing to do: x⁰ = 0 inside every bound."""
    model, nm, stand = g1
    prob = _native_problem(nm, SITES, B_TWIN)
    q, _, _ = _batch(g1, prob, B_TWIN, 903)
    dummy = np.zeros((B_TWIN, prob.n_frame, 7))
    dummy[:, :, 0] = 1.0
    _, _, taps = prob.solve(q, dummy, np.zeros((1, model.nq)), None, 1.0, 1.0, taps=["frame_pose"], solve_qp=False)
    tg = taps["frame_pose"]                    # the frames where they are
    pt = q[:, None, :].copy()                  # the posture where it is (per instance)
    v_ref = _check(prob, SITES, q, tg, pt, 5e-3, 1e-1, TWIN, "(iii) targets = current poses")
    assert np.abs(v_ref).max() < 1e-9          # the unconstrained minimiser is 0 ...
    act, taps = _active_bounds(prob, q, tg, pt, 5e-3, 1e-1, v_ref)
    assert (taps["box_lo"] <= 0.0).all() and (taps["box_hi"] >= 0.0).all()           # ... and 0 violates no bound


def test_nearly_every_hinge_saturated(g1):
    """(iv) dt = 5e-4."""
    _, nm, _ = g1
    prob = _native_problem(nm, SITES, B_TWIN)
    q, tg, pt = _batch(g1, prob, B_TWIN, 904)
    v_ref = _check(prob, SITES, q, tg, pt, 5e-4, 1e-1, TWIN, "(iv) dt = 5e-4")
    act, _ = _active_bounds(prob, q, tg, pt, 5e-4, 1e-1, v_ref)
    print("(iv) bounds active at the optimum: mean %.1f of 37 limited hinges" % act.mean())
    assert act.mean() > 20.0


@pytest.mark.parametrize("B,kernel", [(10751, PERSISTENT), (10752, TWIN), (10753, TWIN), (16385, TWIN)])
def test_ragged_batches_around_the_launch_shape_switch(g1, B, kernel):
    """(v) 10 752 = 3.5 rounds of the 3 072 resident wavefronts: the twin takes over there."""
    _, nm, _ = g1
    prob = _native_problem(nm, SITES, B)
    q, tg, pt = _batch(g1, prob, B, 905 + B)
    _check(prob, SITES, q, tg, pt, 5e-3, 1e-1, kernel, "(v) B = %d" % B)
