"""numpy restatement of multi-start trajectory IK's device-side rules (include/minkhip.h, mkh_solve_trajectory_multistart):
the score of a candidate path, the selection among an instance's candidates, and where a candidate's rows sit in the
time-major `*_all` arrays and in the chosen outputs.  Written from the header's text, not from the kernels, on
multistart_ref's distance, eligibility test and seeds."""

import numpy as np

import multistart_ref as msref

draw_seeds = msref.draw_seeds


def tracked(converged, status):
    """Waypoint t is tracked when its loop converged and its status carries no bit but MKH_ST_OUTSIDE_LIMITS."""
    return msref.eligible(converged, status)


def score(model, q0, q_path, converged, status, weights=None):
    """(n_tracked, length) of ONE candidate: q0 (nq,) the caller's start — not the seed —, q_path (T, nq), converged and
    status (T,).  length = sum over ascending t of d(q_t, q_{t-1}), q_{-1} = q0."""
    q_path = np.asarray(q_path, dtype=np.float64)
    length, prev = 0.0, np.asarray(q0, dtype=np.float64)
    for t in range(q_path.shape[0]):
        length = length + msref.distance(model, q_path[t], prev, weights)
        prev = q_path[t]
    return int(tracked(converged, status).sum()), float(length)


def select(n_tracked, length):
    """The chosen candidate of ONE instance from its candidates' counts and lengths (S,): the largest count, then the
    smallest length (NaN / inf behind every finite one), then the lowest index; nobody tracked anything: candidate 0."""
    n = np.asarray(n_tracked)
    if n.max() == 0:
        return 0
    length = np.asarray(length, dtype=np.float64)
    key = np.where(np.isfinite(length), length, np.inf)
    best = n == n.max()
    return int(np.flatnonzero(best & (key == key[best].min()))[0])


def by_instance(x_all, B, S):
    """(T, B·S, ...) time-major rows t·(B·S) + b·S + s  ->  (B, S, T, ...)."""
    x = np.asarray(x_all)
    return np.ascontiguousarray(np.moveaxis(x.reshape((x.shape[0], B, S) + x.shape[2:]), 0, 2))


def choose(model, q0, q_all, converged_all, status_all, S, weights=None):
    """(seed_index, n_tracked, n_complete, path_length), each (B,), and the (B, S) tables of counts and lengths they come
    from, out of the time-major results of the B·S candidates."""
    q0 = np.asarray(q0, dtype=np.float64)
    B, T = q0.shape[0], np.asarray(q_all).shape[0]
    q, cv, st = by_instance(q_all, B, S), by_instance(converged_all, B, S), by_instance(status_all, B, S)
    counts, lengths = np.zeros((B, S), dtype=np.int64), np.zeros((B, S))
    for b in range(B):
        for s in range(S):
            counts[b, s], lengths[b, s] = score(model, q0[b], q[b, s], cv[b, s], st[b, s], weights)
    pick = np.array([select(counts[b], lengths[b]) for b in range(B)])
    rows = np.arange(B)
    return pick, counts[rows, pick], (counts == T).sum(axis=1), lengths[rows, pick], counts, lengths


def chosen(x_all, seed_index, S, time_major=False):
    """The chosen candidate's rows of a time-major `*_all` array in the caller's layout: out[b, t] = all[t, b·S + seed_index[b]]
    — (B, T, ...), or (T, B, ...) time-major."""
    x = np.asarray(x_all)
    pick = np.asarray(seed_index)
    rows = np.arange(len(pick)) * S + pick
    out = x[:, rows]
    return np.ascontiguousarray(out if time_major else np.swapaxes(out, 0, 1))
