"""The inputs the checked candidate-tracking tests share (tests/test_trajectory_free_cpu.py, tests/test_gpu_trajectory_free.py)
and their references by tests/trajectory_free_ref.py — computed once per process and handed out read-only."""

import numpy as np

import clearance_ref as cr
import trajectory_free_ref as tfref

_cache = {}


def candidates(name, B, S, T, seed=0):
    """(model, limits, q (B, nq), q_all (T, B·S, nq)) on fixture `name`: the rows drawn as swept_cases.ladder_case draws its
    nodes — three quarters from the fixture's rows the reference finds free, one quarter from all of them —, time-major; q the
    model's qpos0."""
    model, _, rows = cr.fixture(name)
    ref = cr.fixture_ref(name)
    rng = np.random.default_rng(seed)
    free = np.nonzero(~ref.in_collision)[0]
    n = B * T * S
    any_row = np.arange(n) % 4 == 3
    rng.shuffle(any_row)
    pick = np.where(any_row, rng.integers(0, len(rows), size=n), free[rng.integers(0, len(free), size=n)])
    q_all = np.ascontiguousarray(rows[pick].reshape(T, B * S, model.nq))
    q = np.tile(np.asarray(model.qpos0, dtype=np.float64), (B, 1))
    return model, cr.limits_of(cr.fixture_limits(name)), q, q_all


def _frozen(case, ref):
    for a in [x for x in ref.values() if isinstance(x, np.ndarray)] + [case[2], case[3]]:
        a.setflags(write=False)
    return case, ref


SHARED = dict(B=3, S=4, T=5, M=5)


def shared():
    """(case, ref): `ur5e_all` (14 pairs: four rows per wavefront), B = 3, S = 4, T = 5, M = 5, every row tracked."""
    if "shared" not in _cache:
        case = candidates("ur5e_all", SHARED["B"], SHARED["S"], SHARED["T"])
        model, limits, q, q_all = case
        _cache["shared"] = _frozen(case, tfref.rule(model, limits, q, q_all, None, None, SHARED["S"], SHARED["M"]))
    return _cache["shared"]


G1 = dict(B=2, S=3, T=3, M=3)
G1_REPLACED = (0, 1)               # (t, i): the node that is replaced by a row in collision — waypoint 0 of a candidate that would win


def g1():
    """(case, ref): `g1` (46 pairs, a free joint: one row per wavefront, quaternion shortest arcs), B = 2, S = 3, T = 3, M = 3,
    node G1_REPLACED replaced by the fixture row the reference finds deepest in collision."""
    if "g1" not in _cache:
        model, limits, q, q_all = candidates("g1", G1["B"], G1["S"], G1["T"])
        _, _, rows = cr.fixture("g1")
        q_all = q_all.copy()
        q_all[G1_REPLACED] = rows[int(np.argmin(cr.fixture_ref("g1").margin))]
        case = (model, limits, q, q_all)
        _cache["g1"] = _frozen(case, tfref.rule(model, limits, q, q_all, None, None, G1["S"], G1["M"]))
    return _cache["g1"]
