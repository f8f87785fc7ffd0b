"""The product form of the low-rank builds (`ik_solve_kernel_44_32_r44`, `_w3`, `_w3o`: no dof block of the tableau — a row on
demand from the factors and a history of 13 pivots, refactorisation when it is full), on G1 config 3 as
`workloads.bench_config` builds it.  Every instance against the plain-C oracle and against the direct QP start
(MKH_FLAG_DIRECT_QP), both at the bound and measure of test_gpu_headline_paths.py: 1e-8·max(1, ‖v_ref‖∞).

  (a) the default handle: ≈ 2.6 pivots per solve, the history hardly ever fills
  (b) the same batch on a handle without the cold-start refinement (MKH_DIAG_NO_COLD_REFINE): ≈ 13 flips per solve, so the
      history fills on about half of the instances and the solve starts again from its active set — same bound, same statuses
      (tests/test_product_form_cpu.py holds the numpy replay to "more than 13 pivots on at least a quarter" of the B = 256
      fixture; a sample of 64 rows of each batch drawn on the device is replayed here, to the same condition)
  (c) dt ten times smaller (test_nearly_every_hinge_saturated's construction): no NaN, same bound

B = 256 (a grid of one workgroup per problem: the twin `44_32_r44_w3o`) and, with the two-waves switch, `44_32_r44`; B = 4 096,
between one and 3.5 rounds of the resident wavefronts, on the persistent `44_32_r44_w3`; B = 10 752 on the twin again, at the
launch-shape switch, as the ragged-batch test of test_gpu_scale.py has it.
The fused-loop builds keep the tableau (docs/HISTORY.md), so there is no fused case here."""

import os
import sys

import numpy as np
import pytest

import oracle_configs as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

TWIN = "ik_solve_kernel_44_32_r44_w3o"
PERSISTENT = "ik_solve_kernel_44_32_r44_w3"
TWO_WAVES = "ik_solve_kernel_44_32_r44"
B_SMALL, SEED_SMALL = 256, 1601          # (the fixture tests/test_product_form_cpu.py replays)
B_TWIN = 10752
B_PERSISTENT = 4096


@pytest.fixture(scope="module")
def g1():
    from mink_amd import _native as nat
    from mink_amd import workloads
    model = workloads.load_robot("g1")
    return model, nat.NativeModel(model), model.key_qpos[model.name2id("key", "stand")]


def _handles(g1, B):
    """(default handle, handle without the cold-start refinement, dt, damping)"""
    from mink_amd import _native as nat
    from mink_amd import workloads
    model, nm, _ = g1
    prob, dt, damping = workloads.bench_config("g1_c3", model, nm, B)
    with nat.diag_options(nat.DIAG_NO_COLD_REFINE):
        plain, _, _ = workloads.bench_config("g1_c3", model, nm, B)
    return prob, plain, dt, damping


def _oracle(q, tg, pt, dt, damping):
    from oracle import cport
    m, tasks, limits, _, _ = oc.g1_c3(tg[0], pt[0])
    cp = cport.CProblem(m, tasks, limits)
    v_ref, st_ref = cp.solve_batch(q, tg, pt, dt, damping, nthreads=min(16, os.cpu_count() or 1))
    assert (st_ref == 0).all(), np.unique(st_ref, return_counts=True)
    return v_ref


def _err(v, ref):
    return np.abs(v - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))


@pytest.fixture(scope="module")
def small(g1):
    """B = 256, generated on the host (tools/proto_product_form.py g1_batch): inputs, both handles, both references."""
    import proto_product_form as pf
    q, tg, stand = pf.g1_batch(B_SMALL, SEED_SMALL)
    pt = np.asarray(stand)[None, :].copy()
    prob, plain, dt, damping = _handles(g1, B_SMALL)
    v_ref = _oracle(q, tg, pt, dt, damping)
    vd, std = prob.solve(q, tg, pt, None, dt, damping, direct_qp=True)
    assert "_r44" not in prob.last_kernel() and (std == 0).all()
    return q, tg, pt, prob, plain, dt, damping, v_ref, vd


def _device_batch(g1, B, seed):
    """device FK for the targets, as in the bench"""
    from mink_amd import workloads
    model, nm, stand = g1
    prob, plain, dt, damping = _handles(g1, B)
    q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(seed), B, base_q=stand)
    pt = stand[None, :].copy()
    v_ref = _oracle(q, tg, pt, dt, damping)
    vd, std = prob.solve(q, tg, pt, None, dt, damping, direct_qp=True)
    assert "_r44" not in prob.last_kernel() and (std == 0).all()
    return q, tg, pt, prob, plain, dt, damping, v_ref, vd


def _history_fills(q, tg, pt, label, n=64):
    """The numpy statement of the kernel's rules on a sample of the batch, without the refinement: more than 13 pivots — a full
    history, a refactorisation — on at least a quarter of it, or case (b) below exercises nothing."""
    import proto_product_form as pf
    rows = np.linspace(0, len(q) - 1, n).astype(int)
    _, st, piv, ref = pf.replay(pf.g1_problems(q[rows], tg[rows], pt[0]), P=13, cold_refine=False)
    print("%s replay of %d rows without the refinement: more than 13 pivots on %d, %d refactorise" % (label, n, int((piv > 13).sum()), int((ref > 0).sum())))
    assert (st == 0).all() and (piv > 13).mean() >= 0.25 and (ref[piv > 13] > 0).all(), (label, piv.tolist())


def _both(fix, kernel, label, replay=False, **kw):
    q, tg, pt, prob, plain, dt, damping, v_ref, vd = fix
    if replay:
        _history_fills(q, tg, pt, label)
    # (a) default handle
    v, st = prob.solve(q, tg, pt, None, dt, damping, **kw)
    assert prob.last_kernel() == kernel, (label, prob.last_kernel())
    e, ed = _err(v, v_ref), _err(v, vd)
    print("%s (a) default handle on %s: max rel err vs C oracle %.2e, vs direct start %.2e" % (label, kernel, e.max(), ed.max()))
    assert (st == 0).all(), (label, np.unique(st, return_counts=True))
    assert e.max() < 1e-8, (label, e.max(), int(e.argmax()))
    assert ed.max() < 1e-8, (label, ed.max(), int(ed.argmax()))
    # (b) no cold-start refinement: the history fills, the solve refactorises
    vp, stp = plain.solve(q, tg, pt, None, dt, damping, **kw)
    assert plain.last_kernel() == kernel, (label, plain.last_kernel())
    e, ed = _err(vp, v_ref), _err(vp, vd)
    print("%s (b) without the refinement on %s: max rel err vs C oracle %.2e, vs direct start %.2e" % (label, kernel, e.max(), ed.max()))
    assert np.array_equal(stp, st), (label, np.unique(stp, return_counts=True))
    assert e.max() < 1e-8, (label, e.max(), int(e.argmax()))
    assert ed.max() < 1e-8, (label, ed.max(), int(ed.argmax()))


def test_small_batch_on_the_twin(small):
    _both(small, TWIN, "B = 256")


def test_two_waves_build(small):
    _both(small, TWO_WAVES, "B = 256, two waves", two_waves=True)


def test_persistent_three_waves_build(g1):
    _both(_device_batch(g1, B_PERSISTENT, 1604), PERSISTENT, "B = 4096", replay=True)


def test_one_problem_per_workgroup_twin(g1):
    _both(_device_batch(g1, B_TWIN, 1602), TWIN, "B = 10752", replay=True)


def test_nearly_every_hinge_saturated(g1):
    """(c) dt = 5e-4, B = 64."""
    from mink_amd import workloads
    model, nm, stand = g1
    prob, plain, _, damping = _handles(g1, 64)
    q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(1603), 64, base_q=stand)
    pt = stand[None, :].copy()
    dt = 5e-4
    v_ref = _oracle(q, tg, pt, dt, damping)
    vd, std = prob.solve(q, tg, pt, None, dt, damping, direct_qp=True)
    assert (std == 0).all()
    for h, label in ((prob, "default"), (plain, "without the refinement")):
        v, st = h.solve(q, tg, pt, None, dt, damping)
        assert h.last_kernel() == TWIN, h.last_kernel()
        e, ed = _err(v, v_ref), _err(v, vd)
        print("(c) dt = 5e-4, %s: max rel err vs C oracle %.2e, vs direct start %.2e" % (label, e.max(), ed.max()))
        assert not np.isnan(v).any() and (st == 0).all(), (label, np.unique(st, return_counts=True))
        assert e.max() < 1e-8 and ed.max() < 1e-8, (label, e.max(), ed.max())
