"""Fixtures shared by tests/test_goalset_cpu.py (which checks their conditions with the CPU oracle) and
tests/test_gpu_goalset.py (which relies on them)."""

import numpy as np

FAR_SEED = 20261016               # (tests/test_gpu_multistart.py::_far_targets: the same generator, the same draws)


def far_goal_joints(m, B, G, seed=FAR_SEED):
    """(B·G, nq) joint vectors drawn uniformly in the joint ranges (clipped to ±π): the end-effector poses of rows
    b·G … b·G + G − 1 are the G goals of target b — far from `home`, and from each other."""
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(m.jnt_range[:, 0], -np.pi), np.minimum(m.jnt_range[:, 1], np.pi)
    return rng.uniform(lo, hi, size=(B * G, m.nq))


def designed_candidates(m, rng, B, G, S, n_max=40):
    """Candidates of a hinge / slide model whose every decision is exact: q_ref on a grid of 1/16, candidate (b, g, s) = q_ref[b]
    moved by n/8 along one joint, n an integer in 1 … n_max — so d_ref = n²/64 with no rounding anywhere, and equal n tie
    exactly.  Returns (q_cand (B, G, S, nq), q_ref (B, nq), d (B, G, S))."""
    assert m.nq == m.nv
    q_ref = rng.integers(-16, 17, size=(B, m.nq)) / 16.0
    n = rng.integers(1, n_max + 1, size=(B, G, S))
    joint = rng.integers(0, m.nq, size=(B, G, S))
    q = np.repeat(np.repeat(q_ref[:, None, None, :], G, axis=1), S, axis=2)
    bi, gi, si = np.meshgrid(np.arange(B), np.arange(G), np.arange(S), indexing="ij")
    q[bi, gi, si, joint] += n / 8.0
    return np.ascontiguousarray(q), q_ref, (n * n) / 64.0
