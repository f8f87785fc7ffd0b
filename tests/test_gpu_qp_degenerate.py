"""The in-wave QP on half-space rows that are duplicate, dependent, almost dependent, contradictory or of zero norm
(tests/qp_cases.py) — every instance against the C oracle, every 8th against the numpy one, and the device's own x through
the optimality certificate of tests/qp_certificate.py.

A strictly convex QP has ONE minimiser however degenerate its constraints are, so the device is held to the project's
tolerance on all of them: ‖v − v_ref‖∞ ≤ 1e-8·max(1, ‖v_ref‖∞), primal violation ≤ 1e-9 (the slack the suite
grants in Gx ≤ h + 1e-9), stationarity ≤ 1e-8·max(1, ‖v_ref‖∞)·dt in Δq units.  Four launch paths:

(a) UR5e, nv = 6, public API (a mink.Task and a mink.Limit subclass): every row fits the tableau; the single-entry families,
    which the host folds into the per-dof box, run here only;
(b) G1, nv = 43: 21 half-space rows per wavefront; `vertex` cut to 21 rows, `duplicate` / `near_parallel` also padded to 30
    rows so that the all-rows redo behind the wavefront kernel runs;
(c) a 63-hinge chain: ONE tableau row — every family with two rows active comes back from the workgroup-per-problem redo;
(d) a 70-hinge chain: the workgroup-per-problem kernel as the model's own path;
(e) (a) and (b) on a handle without the redo launch: an instance is right or carries a status bit, never silently wrong;
(f) infeasible families are reported instance by instance, and a failing neighbour leaves no trace in a feasible one.

Every model stands at the middle of its joint ranges with ConfigurationLimit and a VelocityLimit of ±0.2 per step as the
built-in box (tests/qp_cases.py: DT, VMAX, SCALE).  docs/HISTORY.md has the figures of the run these tests were pinned on."""

import numpy as np
import pytest

import mink_amd as mink
import oracle_configs as oc
import qp_cases as qc
from mink_amd import _native as nat
from oracle import cport, qp_gi
from oracle import ik as oik
from qp_certificate import certificate
from random_models import hinge_chain_mjcf

pytestmark = pytest.mark.gpu

DT, DAMPING = qc.DT, qc.DAMPING
ST_DEGENERATE = 32
FAILURE_BITS = nat.ST_INFEASIBLE | nat.ST_NOT_PD | nat.ST_ITER_LIMIT
# path → (batch, half-space rows the generator may draw: None = every row)
PATHS = {"ur5e": (64, None), "g1": (64, 21), "chain63": (32, None), "chain70": (32, None)}
G1_PADDED_ROWS = 30
WIDE_FAMILIES = ("duplicate", "near_parallel_1e-4", "near_parallel_1e-7", "equality_pairs", "vertex", "infeasible",
                 "barely_feasible")
_models, _refs, _handles, _cfgs = {}, {}, {}, {}


def _model(path):
    if path not in _models:
        _models[path] = oc.model(path) if path in ("ur5e", "g1") else mink.loads_mjcf(hinge_chain_mjcf(int(path[5:])))
    return _models[path]


def _reference(path, fam, padded=False):
    """One family on one path, solved once per session: the rows, the stacked QP of every instance, the C oracle's x
    (None: infeasible) — and the numpy oracle's on every 8th instance."""
    key = (path, fam, padded)
    if key not in _refs:
        m = _model(path)
        B, budget = PATHS[path]
        case = qc.FAMILIES[fam](m.nv, B, budget=budget, scale=qc.SCALE)
        if padded:
            e, J, cost, G, h = case
            case = (e, J, cost) + qc.pad_rows(fam, G, h, e, J, cost, G1_PADDED_ROWS, scale=qc.SCALE)
        cfg = oik.Configuration(m, qc.mid_range_q(m))
        qps, xs = [], []
        for i in range(B):
            P, c, G, h = qc.stacked_qp(cfg, case, i)
            try:
                x = cport.solve_qp(P, c, G, h)
            except qp_gi.Infeasible:
                x = None
            if i % 8 == 0:
                try:
                    x_gi = qp_gi.solve_qp(P, c, G, h)
                except qp_gi.Infeasible:
                    x_gi = None
                assert (x is None) == (x_gi is None), (path, fam, i)
                if x is not None:
                    assert np.abs(x - x_gi).max() <= 1e-10 * max(1.0, np.abs(x).max()), (path, fam, i)
            qps.append((P, c, G, h)); xs.append(x)
        _refs[key] = (case, qps, xs)
    return _refs[key]


def _hinge_dofs(m):
    return np.array([int(m.jnt_dofadr[j]) for j in range(m.njnt) if m.jnt_type[j] != 0])


def _handle(path, M, diag=0):
    """Raw ABI: the built-in box, one dense task of K rows and M dense limit rows — one handle per (model, M, diag)."""
    key = (path, M, diag)
    if key not in _handles:
        m = _model(path)
        idx = _hinge_dofs(m)
        _handles[key] = nat.NativeProblem(
            nat.NativeModel(m), configuration_limits=[mink.ConfigurationLimit(m)._native_desc()[1]],
            velocity_limits=[{"indices": idx, "limit": np.full(len(idx), qc.VMAX)}],
            dense_tasks=[{"cost": np.ones(max(2, m.nv // 2))}], dense_limit_rows=M, max_batch=PATHS[path][0], diag=diag)
    return _handles[key]


def _solve_raw(path, case, diag=0, rows=None):
    e, J, cost, G, h = case
    rows = np.arange(len(e)) if rows is None else rows
    m = _model(path)
    prob = _handle(path, G.shape[1], diag)
    q = np.tile(qc.mid_range_q(m), (len(rows), 1))
    dense = {"task_e": e[rows], "task_J": J[rows], "limit_G": G[rows], "limit_h": h[rows]}
    v, st = prob.solve(q, None, None, None, DT, DAMPING, dense={k: np.ascontiguousarray(x) for k, x in dense.items()})
    return v, st, prob.last_kernel()


class RowsTask(mink.Task):
    """A caller-defined task that returns given rows (e, J) for the whole batch."""

    def __init__(self, e, J, cost):
        super().__init__(cost=cost)
        self.e, self.J = e, J

    def compute_error(self, configuration):
        return self.e

    def compute_jacobian(self, configuration):
        return self.J


class RowsLimit(mink.Limit):
    """A caller-defined limit that returns given rows G·Δq ≤ h for the whole batch."""

    def __init__(self, G, h):
        self.G, self.h = G, h

    def compute_qp_inequalities(self, configuration, dt):
        return mink.Constraint(G=self.G, h=self.h)


def _solve_public(path, case):
    """mink.solve_ik(..., return_status=True) → (v, status, kernel); SolverError propagates."""
    e, J, cost, G, h = case
    m = _model(path)
    if path not in _cfgs:
        _cfgs[path] = mink.Configuration(m, np.tile(qc.mid_range_q(m), (len(e), 1)))
    cfg = _cfgs[path]
    names = [m.jnt_names[j] for j in range(m.njnt) if m.jnt_type[j] != 0]
    lims = [mink.ConfigurationLimit(m), mink.VelocityLimit(m, {n: qc.VMAX for n in names}), RowsLimit(G, h)]
    try:
        v, st = mink.solve_ik(cfg, [RowsTask(e, J, cost)], DT, "mi355x", DAMPING, limits=lims, return_status=True)
    finally:
        kernel = list(cfg._problems.values())[-1].last_kernel() if cfg._problems else None
    return v, st, kernel


def _judge(qps, xs, v, st):
    """Per instance: None when it meets every bound of this file, else a string saying which it misses.  Also the worst
    figures over the instances the reference solves: (error against the C oracle, primal, stationarity / (max(1, |v_ref|)·dt))."""
    verdict, worst = [], np.zeros(3)
    worst[1] = -np.inf
    for i, ((P, c, G, h), x_ref) in enumerate(zip(qps, xs)):
        if x_ref is None:
            ok = bool(st[i] & nat.ST_INFEASIBLE) and np.isnan(v[i]).all()
            verdict.append(None if ok else "reference infeasible, device status %d" % st[i])
            continue
        if st[i] & ~nat.ST_OUTSIDE_LIMITS:
            verdict.append("status %d on a feasible instance" % st[i])
            continue
        v_ref = x_ref / DT
        sc = max(1.0, np.abs(v_ref).max())
        err = np.abs(v[i] - v_ref).max() / sc
        primal, _, stat = certificate(P, c, G, h, v[i] * DT)
        worst = np.maximum(worst, [err, primal, stat / (sc * DT)])
        bad = [n for n, x, b in (("error", err, 1e-8), ("primal", primal, 1e-9), ("stationarity", stat / (sc * DT), 1e-8))
               if not x <= b]
        verdict.append(None if not bad else "%s beyond the bound (err %.2e primal %.2e stat %.2e)" % (
            "/".join(bad), err, primal, stat / (sc * DT)))
    return verdict, worst


def _report(tag, fam, kernel, worst, st, verdict):
    bad = [(i, w) for i, w in enumerate(verdict) if w is not None]
    print("%-8s %-24s %-34s err %.1e primal %.1e stat %.1e status %s wrong %d" % (
        tag, fam, kernel, worst[0], worst[1], worst[2], dict(zip(*np.unique(st, return_counts=True))), len(bad)))
    return bad


# The launch of every case, from the run these tests were pinned on (NativeProblem.last_kernel): the lean plugin build
# `_256` with the smallest tableau that holds nv + M indices, the all-rows redo behind it ("+wide": the handle has that
# launch; which instances it re-solved is in the status census of test_without_the_redo_launch_never_silently_wrong).
_W8, _W16, _W48, _W64 = ("ik_solve_kernel_%d_256+wide" % n for n in (8, 16, 48, 64))
KERNELS = {
    "ur5e": {"duplicate": _W16, "scaled": _W16, "near_parallel_1e-4": _W16, "near_parallel_1e-7": _W16, "equality_pairs": _W16,
             "vertex": _W16, "zero_and_inf": _W16, "combination": _W16, "touching": _W16, "infeasible": _W8,
             "barely_feasible": _W8, "single_entry": _W8},
    "g1": {"duplicate": _W64, "scaled": _W64, "near_parallel_1e-4": _W64, "near_parallel_1e-7": _W64, "equality_pairs": _W48,
           "vertex": _W64, "zero_and_inf": _W64, "combination": _W48, "touching": _W48, "infeasible": _W48,
           "barely_feasible": _W48},
    "g1+pad": {"duplicate": _W64, "near_parallel_1e-4": _W64, "near_parallel_1e-7": _W64},
    "chain63": {f: _W64 for f in qc.GENERAL},
    "chain70": {f: "ik_wide_kernel" for f in WIDE_FAMILIES},
}


def _expect_kernel(path, fam, kernel):
    assert kernel == KERNELS[path][fam], "launch of %s %s: %r" % (path, fam, kernel)


# ------------------------------------------------------------------ (a) UR5e, public API
@pytest.mark.parametrize("fam", list(qc.FAMILIES))
def test_ur5e_public_api(fam):
    case, qps, xs = _reference("ur5e", fam)
    if fam in qc.INFEASIBLE:
        assert all(x is None for x in xs)
        with pytest.raises(mink.SolverError, match="%d of %d instances.*inconsistent" % (len(xs), len(xs))):
            _solve_public("ur5e", case)
        return
    v, st, kernel = _solve_public("ur5e", case)
    verdict, worst = _judge(qps, xs, v, st)
    assert not _report("ur5e", fam, kernel, worst, st, verdict)
    _expect_kernel("ur5e", fam, kernel)


# ------------------------------------------------------------------ (b) G1, 21 rows per wavefront
@pytest.mark.parametrize("fam,padded", [(f, False) for f in qc.GENERAL] +
                         [(f, True) for f in ("duplicate", "near_parallel_1e-4", "near_parallel_1e-7")])
def test_g1_wavefront_rows(fam, padded):
    case, qps, xs = _reference("g1", fam, padded)
    assert case[3].shape[1] == G1_PADDED_ROWS if padded else case[3].shape[1] <= 21
    v, st, kernel = _solve_raw("g1", case)
    verdict, worst = _judge(qps, xs, v, st)
    assert not _report("g1" + ("+pad" if padded else ""), fam, kernel, worst, st, verdict)
    _expect_kernel("g1+pad" if padded else "g1", fam, kernel)
    if padded:
        assert kernel.endswith("+wide")                              # some instance went to the all-rows redo


# ------------------------------------------------------------------ (c) 63-hinge chain: one tableau row
@pytest.mark.parametrize("fam", list(qc.GENERAL))
def test_chain63_one_tableau_row(fam):
    case, qps, xs = _reference("chain63", fam)
    v, st, kernel = _solve_raw("chain63", case)
    verdict, worst = _judge(qps, xs, v, st)
    assert not _report("chain63", fam, kernel, worst, st, verdict)
    _expect_kernel("chain63", fam, kernel)


# ------------------------------------------------------------------ (d) 70-hinge chain: the wide kernel itself
@pytest.mark.parametrize("fam", list(WIDE_FAMILIES))
def test_chain70_wide_kernel(fam):
    case, qps, xs = _reference("chain70", fam)
    v, st, kernel = _solve_raw("chain70", case)
    verdict, worst = _judge(qps, xs, v, st)
    assert not _report("chain70", fam, kernel, worst, st, verdict)
    _expect_kernel("chain70", fam, kernel)


# ------------------------------------------------------------------ (e) never silently wrong
@pytest.mark.parametrize("path", ["ur5e", "g1"])
def test_without_the_redo_launch_never_silently_wrong(path):
    """The wavefront kernel by itself (MKH_DIAG_NO_WIDE_REDO): an instance meets the bounds or carries MKH_ST_ROW_OVERFLOW,
    MKH_ST_DEGENERATE or a failure bit.  (The single-entry families need the host's folding: public API only.)"""
    silent = []
    cases = [(f, False) for f in qc.GENERAL]
    if path == "g1":
        cases += [(f, True) for f in ("duplicate", "near_parallel_1e-4", "near_parallel_1e-7")]
    for fam, padded in cases:
        case, qps, xs = _reference(path, fam, padded)
        v, st, kernel = _solve_raw(path, case, diag=nat.DIAG_NO_WIDE_REDO)
        assert kernel == KERNELS[path + ("+pad" if padded else "")][fam].removesuffix("+wide"), kernel
        verdict, worst = _judge(qps, xs, v, st)
        flagged = (st & (nat.ST_ROW_OVERFLOW | ST_DEGENERATE | FAILURE_BITS)) != 0
        census = {b: int(((st & b) != 0).sum()) for b in (2, 4, 8, 16, 32)}
        print("%-5s%s %-24s %-30s bits %s; wrong %d, of them unflagged %d" % (
            path, "+pad" if padded else "", fam, kernel, census, sum(w is not None for w in verdict),
            sum(w is not None and not flagged[i] for i, w in enumerate(verdict))))
        silent += [(fam, padded, i, w) for i, w in enumerate(verdict) if w is not None and not flagged[i]]
    assert not silent, silent


# ------------------------------------------------------------------ (f) status
@pytest.mark.parametrize("path", ["ur5e", "g1", "chain63", "chain70"])
def test_infeasible_is_reported_and_leaves_no_trace(path):
    """`infeasible` instance by instance (MKH_ST_INFEASIBLE, v NaN), `barely_feasible` solved — and a batch that alternates
    the two: its feasible rows are bit-equal to the same instances solved in a batch of their own."""
    (case_i, qps_i, xs_i), (case_f, qps_f, xs_f) = _reference(path, "infeasible"), _reference(path, "barely_feasible")
    assert all(x is None for x in xs_i) and all(x is not None for x in xs_f)
    v, st, _ = _solve_raw(path, case_i)
    assert ((st & nat.ST_INFEASIBLE) != 0).all() and np.isnan(v).all()
    B = len(xs_f)
    odd = (np.arange(B) % 2 == 1)
    mixed = tuple(case_f[k] if k == 2 else np.where(odd.reshape((B,) + (1,) * (case_f[k].ndim - 1)), case_i[k], case_f[k])
                  for k in range(5))
    vm, stm, kernel = _solve_raw(path, mixed)
    verdict, worst = _judge([qps_i[i] if odd[i] else qps_f[i] for i in range(B)],
                            [xs_i[i] if odd[i] else xs_f[i] for i in range(B)], vm, stm)
    assert not _report(path, "mixed", kernel, worst, stm, verdict)
    _expect_kernel(path, "barely_feasible", kernel)
    assert ((stm[odd] & nat.ST_INFEASIBLE) != 0).all() and (stm[~odd] & ~nat.ST_OUTSIDE_LIMITS == 0).all()
    va, sta, _ = _solve_raw(path, case_f, rows=np.flatnonzero(~odd))
    np.testing.assert_array_equal(vm[~odd], va)
    np.testing.assert_array_equal(stm[~odd], sta)
