"""The headline's build on four waves per SIMD, `ik_solve_kernel_44_32_r44_w4o` (the product form alone below
128 VGPRs — 18 factor rows and 13 history slots of ONE double, the multiplier formed again from the pivot's σ_k² and 1/d; one LDS
union of everything that is dead after the pair lanes), on G1 config 3 as `workloads.bench_config` builds it.

B = 32 768 + 37: the build is taken from 3.5 rounds of its 4 096 resident wavefronts (14 336 instances) AND from the batch size at
which it measured clearly faster than the three-waves twin, 32 768 (minkhip.hip kW4MinBatch: a tie at 14 336, −0.8 % at 16 384, −6 %
at 32 768) — so that is the smallest batch that reaches it; ragged on purpose (not a multiple of the 8 XCDs).  Every instance
against the plain-C oracle and against the direct QP start (MKH_FLAG_DIRECT_QP), measure and bound of
tests/test_gpu_product_form.py: |v − v_ref|∞ / max(1, |v_ref|∞) < 1e-8; statuses equal.

The same instances in three parts run below the switch, on the three-waves build with its 13 two-double slots.  Both builds hold 13
slots and the re-formed multiplier has the stored one's bits, so they refactorise at the same pivots and do the same arithmetic: v
is bitwise equal on EVERY row (stricter than "every row that refactorises in neither build", which a map with fewer slots would
have needed) — a call's answers must not depend on how it is cut into launches (tests/test_gpu_scale.py: host-pointer chunks).

Without the cold-start refinement (MKH_DIAG_NO_COLD_REFINE: ≈ 13 flips per solve) about half of the solves refactorise, some twice
(a replayed sample of 64 rows is held to "at least a quarter"): same bounds, bitwise equal again; NaN-free at dt = 5e-4.
Two frame tasks (n_μ = 12: the guarded rows of load_gz, the union layout at other sizes) and per-instance posture targets."""

import os
import sys

import numpy as np
import pytest

import native_configs as nc
import oracle_configs as oc
from oracle import ik

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

pytestmark = pytest.mark.gpu

W4 = "ik_solve_kernel_44_32_r44_w4o"
W3_BUILDS = ("ik_solve_kernel_44_32_r44_w3", "ik_solve_kernel_44_32_r44_w3o")
B = 32768 + 37
SITES = ("left_foot", "right_foot", "left_palm", "right_palm")
P_SLOTS = 13


def _err(v, ref):
    return np.abs(v - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))


def _native_problem(nm, sites, max_batch, diag=0):
    from mink_amd import _native as nat
    m = nm.model
    fts = [nc._ft(m, s, "site", 200.0, 10.0 if s.endswith("foot") else 0.0, 1.0) for s in sites]
    with nat.diag_options(diag):
        return nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1.0}], configuration_limits=[nc._cfg_limit(m)],
                                 velocity_limits=[nc._vel_limit(m)], max_batch=max_batch)


def _oracle(sites, q, tg, pt, dt, damping):
    from oracle import cport
    m = oc.model("g1")
    tasks = [ik.FrameTaskSpec(m.name2id("site", s), "site", oc._cost6(200.0, 10.0 if s.endswith("foot") else 0.0), tg[0][k], lm_damping=1.0)
             for k, s in enumerate(sites)]
    tasks.append(ik.PostureTaskSpec(np.full(m.nv, 1.0), pt[0] if pt.ndim == 2 else pt[0, 0]))
    cp = cport.CProblem(m, tasks, [ik.ConfigurationLimitSpec(), oc._hinge_velocity_limit(m)])
    v_ref, st_ref = cp.solve_batch(q, tg, pt, dt, damping, nthreads=min(16, os.cpu_count() or 1))
    assert (st_ref == 0).all(), np.unique(st_ref, return_counts=True)                  # the oracle alone solves all of them
    return v_ref


def _halves(prob, q, tg, pt, dt, damping):
    """The same instances in three launches below the switch: the three-waves build."""
    n = len(q)
    out_v, out_s = [], []
    for a, b in ((0, n // 3), (n // 3, 2 * (n // 3)), (2 * (n // 3), n)):
        v, st = prob.solve(q[a:b], tg[a:b], pt if pt.shape[0] != len(q) else pt[a:b], None, dt, damping)
        assert prob.last_kernel() in W3_BUILDS, prob.last_kernel()
        out_v.append(v); out_s.append(st)
    return np.concatenate(out_v), np.concatenate(out_s)


def _checked(prob, q, tg, pt, dt, damping, v_ref, vd, label, device=False):
    """v, status of the default launch: on the new build, statuses 0 (as the oracle's and the direct start's), both bounds.
    device: through device pointers — a host-pointer call that stages 32 MB or more is cut into chunks, each a launch of its own size."""
    if device:
        import torch
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", 0))
        v, st = prob.solve(to(q), to(tg), to(pt), None, dt, damping)
        torch.cuda.synchronize()
        v, st = v.cpu().numpy(), st.cpu().numpy()
    else:
        v, st = prob.solve(q, tg, pt, None, dt, damping)
    assert prob.last_kernel() == W4, (label, prob.last_kernel())
    e, ed = _err(v, v_ref), _err(v, vd)
    print("%s on %s: max rel err vs C oracle %.2e, vs direct start %.2e" % (label, W4, e.max(), ed.max()))
    assert not np.isnan(v).any() and (st == 0).all(), (label, np.unique(st, return_counts=True))
    assert e.max() < 1e-8, (label, e.max(), int(e.argmax()))
    assert ed.max() < 1e-8, (label, ed.max(), int(ed.argmax()))
    return v, st


@pytest.fixture(scope="module")
def g1():
    from mink_amd import _native as nat
    from mink_amd import workloads
    model = workloads.load_robot("g1")
    return model, nat.NativeModel(model), model.key_qpos[model.name2id("key", "stand")]


@pytest.fixture(scope="module")
def batch(g1):
    """Inputs (device FK for the targets, as in the bench), both handles, both references — computed once, left unchanged."""
    from mink_amd import _native as nat
    from mink_amd import workloads
    model, nm, stand = g1
    prob, dt, damping = workloads.bench_config("g1_c3", model, nm, B)
    with nat.diag_options(nat.DIAG_NO_COLD_REFINE):
        plain, _, _ = workloads.bench_config("g1_c3", model, nm, B)
    q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(1701), B, base_q=stand)
    pt = stand[None, :].copy()
    v_ref = _oracle(SITES, q, tg, pt, dt, damping)
    vd, std = prob.solve(q, tg, pt, None, dt, damping, direct_qp=True)
    assert "_r44" not in prob.last_kernel() and (std == 0).all()
    return q, tg, pt, prob, plain, dt, damping, v_ref, vd


def test_default_handle_runs_the_four_waves_build(batch):
    q, tg, pt, prob, plain, dt, damping, v_ref, vd = batch
    v, st = _checked(prob, q, tg, pt, dt, damping, v_ref, vd, "B = %d, default handle" % B)
    assert prob.launch_info(B)["grid"] == B, prob.launch_info(B)
    # below the switch: the three-waves build
    v3, st3 = _halves(prob, q, tg, pt, dt, damping)
    assert np.array_equal(st3, st)
    differ = np.nonzero((v3 != v).any(axis=1))[0]
    print("rows that differ bitwise from the three-waves build: %d of %d" % (len(differ), B))
    assert len(differ) == 0, differ[:16].tolist()
    assert _err(v3, v_ref).max() < 1e-8


def test_without_the_refinement_most_solves_refactorise(batch):
    q, tg, pt, prob, plain, dt, damping, v_ref, vd = batch
    v, st = _checked(plain, q, tg, pt, dt, damping, v_ref, vd, "B = %d, without the refinement" % B)
    v3, st3 = _halves(plain, q, tg, pt, dt, damping)
    assert np.array_equal(st3, st)
    assert _err(v3, v_ref).max() < 1e-8
    np.testing.assert_array_equal(v, v3)
    import proto_product_form as pf
    rows = np.linspace(0, B - 1, 64).astype(int)
    _, s13, piv, ref13 = pf.replay(pf.g1_problems(q[rows], tg[rows], pt[0]), P=P_SLOTS, cold_refine=False, one_double=True)
    print("replay of 64 rows without the refinement: more than 13 pivots on %d, refactorise on %d (twice or more on %d)" % (
        int((piv > 13).sum()), int((ref13 > 0).sum()), int((ref13 > 1).sum())))
    assert (s13 == 0).all()
    assert (ref13 > 0).mean() >= 0.25                   # ... or this case exercises nothing (tests/test_gpu_product_form.py's condition)


def test_nearly_every_hinge_saturated(batch):
    """dt = 5e-4 (tests/test_gpu_product_form.py's construction): no NaN, same bounds, on both handles."""
    q, tg, pt, prob, plain, _, damping, _, _ = batch
    dt = 5e-4
    v_ref = _oracle(SITES, q, tg, pt, dt, damping)
    vd, std = prob.solve(q, tg, pt, None, dt, damping, direct_qp=True)
    assert (std == 0).all()
    for h, label in ((prob, "default"), (plain, "without the refinement")):
        _checked(h, q, tg, pt, dt, damping, v_ref, vd, "dt = 5e-4, %s" % label)


def test_two_frame_tasks(g1):
    """n_μ = 12: rows 12 … 17 of the factor are the guarded (zero) rows of load_gz; the union layout with two task blocks."""
    from mink_amd import workloads
    model, nm, stand = g1
    sites = SITES[:2]
    dt, damping = 5e-3, 1e-1
    for diag, label in ((0, "two frame tasks"), (4, "two frame tasks, without the refinement")):
        prob = _native_problem(nm, sites, B, diag)
        q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(1702), B, base_q=stand)
        pt = stand[None, :].copy()
        if diag == 0:
            v_ref = _oracle(sites, q, tg, pt, dt, damping)
        vd, std = prob.solve(q, tg, pt, None, dt, damping, direct_qp=True)
        assert "_r44" not in prob.last_kernel() and (std == 0).all()
        v, st = _checked(prob, q, tg, pt, dt, damping, v_ref, vd, label)
        v3, st3 = _halves(prob, q, tg, pt, dt, damping)
        assert np.array_equal(st3, st) and np.array_equal(v3, v)
        prob.close()


def test_per_instance_posture_targets(g1):
    pytest.importorskip("torch")
    from mink_amd import workloads
    model, nm, stand = g1
    dt, damping = 5e-3, 1e-1
    prob = _native_problem(nm, SITES, B)
    rng = np.random.default_rng(1703)
    q, tg = workloads.make_batch(model, nm, prob, rng, B, base_q=stand)
    pt = workloads.sample_q(model, rng, B, stand)[:, None, :].copy()      # (B, 1, nq): a posture of its own per instance
    v_ref = _oracle(SITES, q, tg, pt, dt, damping)
    vd, std = prob.solve(q, tg, pt, None, dt, damping, direct_qp=True)
    assert "_r44" not in prob.last_kernel() and (std == 0).all()
    v, st = _checked(prob, q, tg, pt, dt, damping, v_ref, vd, "per-instance posture targets", device=True)
    v3, st3 = _halves(prob, q, tg, pt, dt, damping)
    assert np.array_equal(st3, st) and np.array_equal(v3, v)
    prob.close()
