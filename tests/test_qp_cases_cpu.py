"""The designed QP families of tests/qp_cases.py do what they are for — on the reference side alone (no device).

Both oracles (numpy Goldfarb–Idnani, `oracle/qp_gi.py`, and the plain-C restatement behind `oracle/cport.py`) solve every
feasible instance, agree, pass the optimality certificate of tests/qp_certificate.py, refuse exactly the infeasible
families — and the degeneracy each family was drawn for is present at the optimum.  The problems are the ones the device
tests solve on the UR5e (nv = 6, every row) and the G1 (nv = 43, 21 half-space rows per wavefront): box rows of the
built-in limits first, then the family (tests/qp_cases.py::stacked_qp)."""

import numpy as np
import pytest

import oracle_configs as oc
import qp_cases as qc
from oracle import cport, qp_gi
from oracle import ik as oik
from qp_certificate import ACTIVE_TOL, certificate

B = 16
MODELS = {"ur5e": None, "g1": 21}                      # model → half-space rows its wavefront path holds (None: every row)
_solved = {}


def _solve(robot, fam):
    """Every instance of one family by both oracles, once per session: list of (P, c, G, h, x_gi, x_c, n_box_rows)."""
    if (robot, fam) not in _solved:
        m = oc.model(robot)
        cfg = oik.Configuration(m, qc.mid_range_q(m))
        case = qc.FAMILIES[fam](m.nv, B, budget=MODELS[robot], scale=qc.SCALE)
        out = []
        for i in range(B):
            P, c, G, h = qc.stacked_qp(cfg, case, i)
            xs = []
            for solve in (qp_gi.solve_qp, cport.solve_qp):
                try:
                    xs.append(solve(P, c, G, h))
                except qp_gi.Infeasible:
                    xs.append(None)
            out.append((P, c, G, h, xs[0], xs[1], len(h) - case[4].shape[1]))
        _solved[(robot, fam)] = (case, out)
    return _solved[(robot, fam)]


@pytest.mark.parametrize("fam", list(qc.FAMILIES))
@pytest.mark.parametrize("robot", list(MODELS))
def test_oracles_agree_and_pass_the_certificate(robot, fam):
    _, out = _solve(robot, fam)
    agree = primal = stat = 0.0
    for P, c, G, h, x_gi, x_c, _ in out:
        if fam in qc.INFEASIBLE:
            assert x_gi is None and x_c is None
            continue
        assert x_gi is not None and x_c is not None      # (barely_feasible among them: a slab 1e-6·SCALE wide is solved)
        sc = max(1.0, np.abs(x_gi).max())
        agree = max(agree, np.abs(x_gi - x_c).max() / sc)
        for x in (x_gi, x_c):
            p, _, s = certificate(P, c, G, h, x)
            primal, stat = max(primal, p), max(stat, s / max(1.0, np.abs(x).max()))
    print("%s %-24s oracles agree %.1e, certificate primal %.1e stationarity %.1e" % (robot, fam, agree, primal, stat))
    assert agree <= 1e-10 and primal <= 1e-11 and stat <= 1e-11


@pytest.mark.parametrize("fam", [f for f in qc.FAMILIES if f not in qc.INFEASIBLE])
@pytest.mark.parametrize("robot", list(MODELS))
def test_minimiser_is_well_conditioned(robot, fam):
    """The device is held to 1e-8·max(1, ‖v‖∞) on these problems, i.e. 1e-8·max(dt, ‖x‖∞) in x.  That is only fair where the
    minimiser does not move under rounding of the inputs: every entry of G and h changed by a relative 2.2e-16 (random signs)
    moves the C oracle's x by less than 1 % of that bound.  (`touching` and the slabs of zero width stay feasible: the
    oracle's own violation tolerance is 1e-12.)"""
    _, out = _solve(robot, fam)
    rng = np.random.default_rng(5)
    worst = 0.0
    for P, c, G, h, _, x, _ in out:
        eps = np.finfo(float).eps
        G2 = G * (1.0 + eps * rng.choice([-1.0, 1.0], size=G.shape))
        h2 = h * (1.0 + eps * rng.choice([-1.0, 1.0], size=h.shape))
        worst = max(worst, np.abs(cport.solve_qp(P, c, G2, h2) - x).max() / max(qc.DT, np.abs(x).max()))
    print("%s %-24s x moves by %.1e·max(dt, |x|) under one-ulp changes of G, h" % (robot, fam, worst))
    assert worst <= 1e-10


def _active_family_rows(robot, fam):
    """Per instance: (active rows of the family at the C oracle's optimum, as indices into the family; their matrix)."""
    _, out = _solve(robot, fam)
    res = []
    for P, c, G, h, _, x, nb in out:
        _, act, _ = certificate(P, c, G, h, x)
        a = act[act >= nb]
        res.append((a - nb, G[a]))
    return res


@pytest.mark.parametrize("robot", list(MODELS))
def test_purpose_vertex(robot):
    """UR5e: nv + 4 rows through the minimiser, more than nv active in EVERY instance.  G1: cut to the 21 rows a wavefront
    holds (fewer than nv, so the minimiser leaves x_s along the weakly curved directions and may meet a joint limit first):
    every tableau row active in at least half of the instances."""
    m = oc.model(robot)
    n_act = [len(a) for a, _ in _active_family_rows(robot, "vertex")]
    print("%s vertex: active family rows per instance %s" % (robot, n_act))
    if MODELS[robot] is None:
        assert min(n_act) > m.nv
    else:
        assert sum(n == MODELS[robot] for n in n_act) >= B // 2


@pytest.mark.parametrize("fam", ["duplicate", "combination", "equality_pairs"])
@pytest.mark.parametrize("robot", list(MODELS))
def test_purpose_rank_deficient_active_set(robot, fam):
    deficient = sum(len(a) > 0 and np.linalg.matrix_rank(GA) < len(a) for a, GA in _active_family_rows(robot, fam))
    print("%s %s: active rows rank deficient in %d of %d instances" % (robot, fam, deficient, B))
    assert deficient >= B // 2


@pytest.mark.parametrize("fam", ["near_parallel_1e-4", "near_parallel_1e-7"])
@pytest.mark.parametrize("robot", list(MODELS))
def test_purpose_near_parallel_pairs_active(robot, fam):
    both = sum(any(k in a and k + 3 in a for k in range(3)) for a, _ in _active_family_rows(robot, fam))
    print("%s %s (pull %.1f): both rows of a pair active in %d of %d instances" % (robot, fam, qc.NEAR_PARALLEL_PULL, both, B))
    assert both >= B // 4


@pytest.mark.parametrize("nv", [6, 43])
def test_purpose_touching_is_exact(nv):
    e, J, cost, G, h = qc.touching(nv, B, scale=qc.SCALE)
    H, c = qc.objective(e, J, cost)
    x0 = np.linalg.solve(H, -c[..., None])[..., 0]
    assert (np.abs(np.einsum("bmi,bi->bm", G, x0) - h) == 0.0).all()


def test_scale_is_an_equivariance():
    """`scale` only places x against the robot's box: the rows G do not change, e and h scale with it."""
    for fam, fn in qc.FAMILIES.items():
        a, b = fn(6, 4, scale=1.0), fn(6, 4, scale=0.5)          # (a power of two: exact)
        np.testing.assert_array_equal(a[3], b[3])
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_allclose(0.5 * a[0], b[0], rtol=1e-15, atol=0)
        fin = np.isfinite(a[4])
        np.testing.assert_allclose(0.5 * a[4][fin], b[4][fin], rtol=1e-9, atol=1e-15)


def test_lstsq_multipliers_misjudge_a_dependent_active_set():
    """Why tests/qp_certificate.py exists: the oracle's x is optimal (NNLS finds λ ≥ 0 with zero residual), but
    `kkt_residual` takes minimum-norm multipliers from lstsq on the dependent active rows and reports one of them negative —
    a 'dual infeasibility' of the size of the multiplier itself.  Exact copies of one row do not show it (the minimum-norm
    split between equal rows is even, so it is non-negative whenever their sum is): `duplicate` is searched first and has
    none; `combination` — rows a₀, a₁, a₀ + a₁ with multipliers (c₀ − t, c₁ − t, t), minimum norm at t = (c₀ + c₁)/3 — has
    one wherever c₁ > 2·c₀ or c₀ > 2·c₁."""
    found = None
    for fam in ("duplicate", "combination"):
        for robot in MODELS:
            _, out = _solve(robot, fam)
            for i, (P, c, G, h, x, _, _) in enumerate(out):
                _, act, stat = certificate(P, c, G, h, x)
                lam = np.linalg.lstsq(G[act].T, -(P @ x + c), rcond=None)[0]
                if found is None and lam.min() < -1e-3 * np.abs(lam).max() and stat <= 1e-11:
                    found = (robot, fam, i, float(lam.min()), qp_gi.kkt_residual(P, c, G, h, x), stat)
        if fam == "duplicate":
            assert found is None
    assert found is not None, "no instance with a negative lstsq multiplier"
    print("%s %s[%d]: lstsq multiplier %.3e, kkt_residual %.3e, certificate stationarity %.1e" % found)
    assert found[4] >= -found[3] * (1 - 1e-6) and found[4] > 1e6 * found[5]


def test_certificate_rejects_a_wrong_answer():
    """The certificate is not vacuous: a feasible point 1e-6 off the minimiser fails stationarity, a point across a row
    fails primal, and a row of zeros counts as violated iff h < 0."""
    _, out = _solve("ur5e", "duplicate")
    P, c, G, h, x, _, nb = out[0]
    p, act, s = certificate(P, c, G, h, x)
    a = G[nb] / np.linalg.norm(G[nb])
    assert nb in act and s <= 1e-11
    p_in, _, s_in = certificate(P, c, G, h, x - 1e-6 * a)         # inside: feasible, no longer optimal
    assert p_in <= 1e-6 + 1e-9 and s_in > 1e-8
    p_out, _, _ = certificate(P, c, G, h, x + 1e-6 * a)
    assert abs(p_out - 1e-6) < 1e-9
    Z, hz = np.zeros((1, len(x))), np.array([-0.5])
    assert certificate(P, c, Z, hz, x)[0] == 0.5 and certificate(P, c, Z, -hz, x)[0] == -np.inf
