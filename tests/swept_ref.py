"""numpy restatement of THE RULE OF THE SWEEP (include/minkhip.h): the interior samples of an edge by keyframe_ref.blend_posture,
each judged by clearance_ref.clearance, and numpy's min / argmin over them.  Written from the header's text, not from the kernel.
The reference of tests/test_gpu_swept.py; tests/test_swept_cpu.py holds its pieces against each other."""

from typing import NamedTuple

import numpy as np

import clearance_ref as cr
import keyframe_ref as kf


class RefSweep(NamedTuple):
    margin: np.ndarray         # (N,)
    sample: np.ndarray         # (N,) int32
    pair: np.ndarray           # (N,) int32
    in_collision: np.ndarray   # (N,) bool
    samples: np.ndarray        # (N, M): every sample's margin


def sample_rows(model, a, b, n_samples):
    """q(u_i) = a (+) u_i (b (-) a) for u_i = i / (M + 1), i = 1 .. M: (M, nq)."""
    M = int(n_samples)
    assert M >= 1
    return np.stack([kf.blend_posture(model, a, b, float(i) / float(M + 1)) for i in range(1, M + 1)])


def sweep(model, limits, q_from, q_to, n_samples):
    """The rule on N edges: q_from, q_to (N, nq); `limits` as clearance_ref.clearance takes them."""
    q_from = np.asarray(q_from, dtype=np.float64).reshape(-1, model.nq)
    q_to = np.asarray(q_to, dtype=np.float64).reshape(-1, model.nq)
    N, M = len(q_from), int(n_samples)
    margins, pairs = np.full((N, M), np.nan), np.zeros((N, M), np.int32)
    finite = np.isfinite(q_from).all(axis=1) & np.isfinite(q_to).all(axis=1)       # (a NaN or an infinity: every sample NaN, pair 0)
    if finite.any():
        rows = np.concatenate([sample_rows(model, q_from[e], q_to[e], M) for e in np.nonzero(finite)[0]])
        ref = cr.clearance(model, limits, rows)
        margins[finite], pairs[finite] = ref.margin.reshape(-1, M), ref.pair.reshape(-1, M)
    sample = margins.argmin(axis=1).astype(np.int32)            # (numpy: the first NaN, else the lowest index of the minimum)
    margin = margins[np.arange(N), sample]
    return RefSweep(margin, sample, pairs[np.arange(N), sample].astype(np.int32), ~(margin >= 0.0), margins)
