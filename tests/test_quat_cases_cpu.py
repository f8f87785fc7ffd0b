"""The designed quaternion states of tests/quat_cases.py do what they are for — on the reference side alone (no device).

Per family and model: both oracles (numpy, `oracle/ik.py`, on every 8th instance; the plain-C restatement behind
`oracle/cport.py` on all) solve every instance and agree; the answer does not move under a one-ulp change of every
quaternion entry by more than 1 % of the tolerance the device is held to (the rule of
tests/test_qp_cases_cpu.py::test_minimiser_is_well_conditioned); and each family is what its name says."""

import numpy as np
import pytest

import quat_cases as qc
from oracle import ik as oik
from oracle import mjmath

EVERY = 8
WITH_BALL = [n for n in qc.MODELS if n != "h1"]           # (the H1 has a free root and hinges: no posture error on a quaternion)


def _quats(m, x):
    """(B, n_quat, 4) quaternion slices of a batch of configurations."""
    return np.stack([x[:, a:a + 4] for _, a in qc.quat_slices(m)], axis=1)


def _posture_error(P, q_i, pt_i):
    return oik.task_error_jacobian(oik.Configuration(P["m"], q_i), oik.PostureTaskSpec(P["posture"][0], pt_i, P["posture"][1]))[0]


@pytest.mark.parametrize("family", qc.FAMILIES)
@pytest.mark.parametrize("name", qc.MODELS)
def test_oracles_agree_and_the_answer_is_well_conditioned(name, family):
    """Agreement ≤ 1e-12·max(1, ‖v‖∞), no Infeasible anywhere (limited ball joints are drawn with σ = 0.15 for that), and
    the numpy oracle's v moves by ≤ 1e-10·max(1, ‖v‖∞) when every quaternion entry of q and of the posture target changes
    by one ulp (random signs)."""
    P, q, pt, tg = qc.case(name, family)
    m = P["m"]
    v_c, st_c = qc.c_oracle(name, family)
    assert (st_c == 0).all(), np.unique(st_c, return_counts=True)
    rng = np.random.default_rng(5)
    eps = np.finfo(float).eps
    agree = moved = 0.0
    for i in range(0, len(q), EVERY):
        v = qc.numpy_oracle(P, q[i], tg[i], pt[i, 0])                   # (raises qp_gi.Infeasible if it is)
        sc = max(1.0, np.abs(v).max())
        agree = max(agree, np.abs(v - v_c[i]).max() / sc)
        q2, pt2 = q[i].copy(), pt[i, 0].copy()
        for _, a in qc.quat_slices(m):
            q2[a:a + 4] *= 1.0 + eps * rng.choice([-1.0, 1.0], size=4)
            pt2[a:a + 4] *= 1.0 + eps * rng.choice([-1.0, 1.0], size=4)
        moved = max(moved, np.abs(qc.numpy_oracle(P, q2, tg[i], pt2) - v).max() / sc)
    print("%-9s %-16s oracles agree %.1e, one-ulp sensitivity %.1e" % (name, family, agree, moved))
    assert agree <= 1e-12 and moved <= 1e-10


@pytest.mark.parametrize("name", qc.MODELS)
def test_purpose_signs(name):
    """neg_w: w < 0 on every quaternion of q.  antipodal_target: dot(q, target) < 0.  zero: exactly one zero quaternion per
    instance.  Every family leaves the hinge / slide entries and the frame targets of `plain` alone."""
    P, q0, pt0, tg0 = qc.case(name, "plain")
    m = P["m"]
    assert (_quats(m, q0)[..., 0] > 0).all()                            # what the suite fed the kernels before
    _, q, _, _ = qc.case(name, "neg_w")
    assert (_quats(m, q)[..., 0] < 0).all()
    _, q, pt, _ = qc.case(name, "antipodal_target")
    assert ((_quats(m, q) * _quats(m, pt[:, 0])).sum(axis=-1) < 0).all()
    _, q, _, _ = qc.case(name, "zero")
    assert ((_quats(m, q) == 0).all(axis=-1).sum(axis=1) == 1).all()
    rest = np.ones(m.nq, bool)
    for _, a in qc.quat_slices(m):
        rest[a:a + 4] = False
    for family in qc.FAMILIES:
        _, q, pt, tg = qc.case(name, family)
        assert np.array_equal(q[:, rest], q0[:, rest]) and np.array_equal(pt[:, 0][:, rest], pt0[:, 0][:, rest]) and tg is tg0


@pytest.mark.parametrize("family", [f for f in qc.FAMILIES if f.startswith(("near_pi_", "tiny_"))])
@pytest.mark.parametrize("name", WITH_BALL)
def test_purpose_angle_to_the_target(name, family):
    """The reference's posture error on every ball joint has norm within 1e-12 of π − δ (near_pi) resp. δ (tiny); for
    near_pi the even instances (π − δ) and the odd ones (π + δ, wrapped) point in opposite directions along the axis."""
    P, q, pt, _ = qc.case(name, family)
    m = P["m"]
    _, _, ax = qc.plain(m, len(q), qc.SEED)
    k_of = {j: k for k, (j, _) in enumerate(qc.quat_slices(m))}
    d = qc.family_delta(family)
    want = np.pi - d if family.startswith("near_pi_") else d
    worst = 0.0
    for i in range(len(q)):
        e = _posture_error(P, q[i], pt[i, 0])
        for j, va in qc.ball_dofs(m):
            worst = max(worst, abs(np.linalg.norm(e[va:va + 3]) - want))
            along = e[va:va + 3] @ ax[i, k_of[j]]
            assert along > 0 if (i % 2 == 0 or family.startswith("tiny_")) else along < 0, (i, j, along)
    print("%-9s %-14s | ‖e_ball‖ − %.17g | ≤ %.1e" % (name, family, want, worst))
    assert qc.ball_dofs(m) and worst <= 1e-12


@pytest.mark.parametrize("name", WITH_BALL)
def test_purpose_same_is_exact(name):
    """`same`: the relative quaternion conj(q)·target is (±|q|², 0) up to the rounding of its own products (+ on odd
    instances, − on even ones) — a vector part below mju_normalize3's 1e-15, so mju_quat2Vel takes its zero-axis branch
    (exactly 0 on 118 of the 432 quaternions of the three models, one rounding of a sum of two products, ≤ 6e-17, on the
    others) — and the reference's error on the ball dofs is 0 to 1e-15 on both sides of the wrap."""
    P, q, pt, _ = qc.case(name, "same")
    m = P["m"]
    exact = total = 0
    for i in range(len(q)):
        for _, a in qc.quat_slices(m):
            neg, dif = np.empty(4), np.empty(4)
            mjmath.mju_negQuat(neg, q[i, a:a + 4])
            mjmath.mju_mulQuat(dif, neg, pt[i, 0, a:a + 4])
            assert np.linalg.norm(dif[1:]) < mjmath.mjMINVAL and abs(abs(dif[0]) - 1.0) <= 4.5e-16 and (dif[0] > 0) == (i % 2 == 1)
            exact += int((dif[1:] == 0).all()); total += 1
        e = _posture_error(P, q[i], pt[i, 0])
        for _, va in qc.ball_dofs(m):
            assert np.abs(e[va:va + 3]).max() <= 1e-15
    print("%-9s same: vector part exactly 0 on %d of %d quaternions" % (name, exact, total))
    assert exact > 0


@pytest.mark.parametrize("name", qc.MODELS)
def test_purpose_f32_and_scaled_norms(name):
    """f32: the round trip moves the norm of a quaternion by 1e-9 … 1e-6 — off by more than mju_normalize4's 1e-15, by less
    than anything a caller would notice.  That holds for the bulk (median 1.2e-8 … 1.6e-8, max 4.0e-8), not for every single
    quaternion: four rounding errors sometimes cancel (min 5.2e-11), so the lower end is asserted on the median and every
    quaternion is held to > 1e-15.  scaled: the norms are the stated factors."""
    P, q, pt, _ = qc.case(name, "f32")
    m = P["m"]
    dev = np.abs(np.linalg.norm(np.concatenate([_quats(m, q), _quats(m, pt[:, 0])]), axis=-1) - 1.0)
    print("%-9s f32: | ‖q‖ − 1 | min %.1e median %.1e max %.1e" % (name, dev.min(), np.median(dev), dev.max()))
    assert dev.max() <= 1e-6 and np.median(dev) >= 1e-9 and (dev > 1e-15).all()
    _, q, pt, _ = qc.case(name, "scaled")
    for i in range(len(q)):
        np.testing.assert_allclose(np.linalg.norm(_quats(m, q)[i], axis=-1), qc.Q_SCALES[i % 4], rtol=1e-15)
        np.testing.assert_allclose(np.linalg.norm(_quats(m, pt[:, 0])[i], axis=-1), qc.TARGET_SCALES[i % 4], rtol=1e-15)


@pytest.mark.parametrize("family", qc.FAMILIES)
def test_ballchain_velocity_bounds_bind_on_some_dofs(family):
    """The 68-dof chain (free root, 18 ball joints, 4 of them limited, 8 hinges) with VelocityLimit 8 rad/s on its 50 hinge and
    unlimited-ball dofs, posture cost 0.3, dt 0.02: on the C oracle between 2 and nv / 2 = 34 velocity bounds bind per instance
    on average in every family — 2.1 (`same`, `tiny`), 3.0 (`antipodal_target`), 7.3 (`zero`), 13.6 (`plain`, `neg_w`, `scaled`,
    `f32`), 27.2 (`near_pi`).  (Limit 1.0 at dt 0.02 bound 420 of 544: a clamp, not a solve.)"""
    P, q, _, _ = qc.case("ballchain", family)
    m = P["m"]
    assert 65 <= m.nv <= 70 and sum(1 for j, _ in qc.ball_dofs(m) if m.jnt_limited[j]) >= 2
    v, st = qc.c_oracle("ballchain", family)
    idx, lim = P["vel"]
    bind = (np.abs(np.abs(v[:, idx]) - lim) < 1e-9).sum(axis=1).mean()
    print("ballchain %-16s velocity bounds binding per instance: mean %.1f" % (family, bind))
    assert 2.0 <= bind <= m.nv / 2
