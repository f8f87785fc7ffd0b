"""The inputs the swept-clearance and checked-ladder tests share (tests/test_swept_cpu.py, tests/test_gpu_swept.py,
tests/test_gpu_ladder_free.py), and their references by tests/swept_ref.py and tests/ladder_free_ref.py — computed once per
process and handed out read-only."""

import numpy as np

import clearance_ref as cr
import ladder_free_ref as lfref

_cache = {}


def ladder_case(B=4, T=5, S=4, seed=0):
    """(model, limits, q (B, nq), q_nodes (B, T, S, nq)) on the UR5e with the `ur5e_all` checker (14 capsule pairs against floor and
    wall): three quarters of the nodes drawn from the fixture's free rows, one quarter from all of its rows; q the model's qpos0."""
    model, _, rows = cr.fixture("ur5e_all")
    ref = cr.fixture_ref("ur5e_all")
    rng = np.random.default_rng(seed)
    free = np.nonzero(~ref.in_collision)[0]
    n = B * T * S
    any_row = np.arange(n) % 4 == 3
    rng.shuffle(any_row)
    pick = np.where(any_row, rng.integers(0, len(rows), size=n), free[rng.integers(0, len(free), size=n)])
    q_nodes = np.ascontiguousarray(rows[pick].reshape(B, T, S, model.nq))
    q = np.tile(np.asarray(model.qpos0, dtype=np.float64), (B, 1))
    return model, cr.limits_of(cr.fixture_limits("ur5e_all")), q, q_nodes


def ladder_ref(B=4, T=5, S=4, M=7, seed=0, sparse=False):
    """(case, stage, select): ladder_free_ref.margins and ladder_free_ref.select of ladder_case, no gate.  Every node tracked —
    or, `sparse`, about one in seven and every node from 64 on (select["tracked_in"]): a wide rung whose reference stays quick,
    an untracked destination's edges not being swept."""
    key = (B, T, S, M, seed, sparse)
    if key not in _cache:
        case = ladder_case(B, T, S, seed)
        model, limits, q, q_nodes = case
        trk = None
        if sparse:
            trk = np.random.default_rng(seed + 1000).random((B, T, S)) < 0.15
            trk[:, :, 64:] = True
        stage = lfref.margins(model, limits, q_nodes, trk, M)
        sel = lfref.select(model, limits, q, q_nodes, trk, None, np.inf, M, stage=stage)
        sel["tracked_in"] = trk
        for a in list(stage) + [x for x in sel.values() if isinstance(x, np.ndarray)] + [q, q_nodes]:
            a.setflags(write=False)
        _cache[key] = (case, stage, sel)
    return _cache[key]
