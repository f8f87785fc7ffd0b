"""numpy restatement of the seed table's metric and K-best rule, written from the text of include/minkhip.h "Seed tables" (not
from the kernel): every product and sum below is one rounded numpy operation, in the header's order, so nothing is fused."""

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)


def default_weights(frame_tasks):
    """(position weights, orientation weights) of a list of frame-task descriptors ({"cost": 6 numbers, optional "root_type"}):
    1 where a plain FrameTask has a cost of that kind > 0, else 0; a RelativeFrameTask 0 / 0."""
    wp = np.array([1.0 if t.get("root_type") is None and any(float(c) > 0.0 for c in t["cost"][:3]) else 0.0 for t in frame_tasks])
    wo = np.array([1.0 if t.get("root_type") is None and any(float(c) > 0.0 for c in t["cost"][3:6]) else 0.0 for t in frame_tasks])
    return wp, wo


def _norm2(q):
    return ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]


def distances(targets, keys, wp, wo):
    """d (B, N) between targets (B, F, 7) and the keys (N, F, 7) of the entries (wxyz, xyz); a non-finite d counts as DBL_MAX."""
    targets, keys = np.asarray(targets, dtype=np.float64), np.asarray(keys, dtype=np.float64)
    B, F = targets.shape[:2]
    N = keys.shape[0]
    assert targets.shape == (B, F, 7) and keys.shape == (N, F, 7) and len(wp) == F and len(wo) == F
    d = np.zeros((B, N))
    with np.errstate(all="ignore"):
        for f in range(F):
            T, E = targets[:, None, f, :], keys[None, :, f, :]
            dx, dy, dz = E[..., 4] - T[..., 4], E[..., 5] - T[..., 5], E[..., 6] - T[..., 6]
            pos = (dx * dx + dy * dy) + dz * dz
            dot = ((T[..., 0] * E[..., 0] + T[..., 1] * E[..., 1]) + T[..., 2] * E[..., 2]) + T[..., 3] * E[..., 3]
            c = dot / np.sqrt(_norm2(T) * _norm2(E))
            ori = 4.0 * (1.0 - c * c)
            ori = np.where(ori < 0.0, 0.0, ori)                 # max(0, .) that keeps a NaN
            d = d + (wp[f] * pos + wo[f] * ori)
        bad = ~(d >= 0.0) | (d > DBL_MAX)
    return np.where(bad, DBL_MAX, d)


def k_best(d, K):
    """(index (B, K), distance (B, K)): per row the K smallest (d, j) in lexicographic order, ascending."""
    d = np.asarray(d)
    assert 1 <= K <= d.shape[1]
    order = np.argsort(d, axis=1, kind="stable")[:, :K]         # stable: equal distances keep ascending j
    return order.astype(np.int32), np.take_along_axis(d, order, axis=1)


def query(targets, keys, K, wp, wo):
    return k_best(distances(targets, keys, wp, wo), K)


def relative_gaps(d, K):
    """Per row the relative gaps (d[r + 1] − d[r]) / d[r + 1] between ranks 1 … K + 1 of the sorted distances: (B, K)."""
    s = np.sort(d, axis=1)[:, :K + 1]
    with np.errstate(all="ignore"):
        return (s[:, 1:] - s[:, :-1]) / s[:, 1:]
