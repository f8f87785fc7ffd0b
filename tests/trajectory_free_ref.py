"""numpy restatement of THE RULE "with a checker" of candidate tracking (include/minkhip.h, mkh_select_trajectory_candidates /
mkh_solve_trajectory_multistart_free), written from the header's text, not from the kernels: nodes by clearance_ref, edges by
swept_ref, count / length / selection by trajectory_multistart_ref.  The flag logic (`flags`, `pick`) takes margins as they
come, so that tests/test_trajectory_free_cpu.py can hold it on hand-made tables; `rule` puts the geometry in front of it."""

import numpy as np

import clearance_ref as cr
import swept_ref as swref
import trajectory_multistart_ref as tmref

ST_OUTSIDE_LIMITS, ST_IN_COLLISION = 1, 64


def flags(converged_all, status_all, node_margin_all, edge_margin_of):
    """Nodes, edges and score flags of (T, R) candidates rows.  edge_margin_of(t, i) is asked for the edges that ARE swept, and
    for no other.  Returns (status_all with the bit, eligible, edge_margin_all, counted)."""
    cv, st, nm = np.asarray(converged_all), np.asarray(status_all), np.asarray(node_margin_all, dtype=np.float64)
    T, R = nm.shape
    status = st | np.where(~(nm >= 0.0), ST_IN_COLLISION, 0).astype(st.dtype)              # a NaN decides: in collision
    eligible = (cv != 0) & ((status & ~ST_OUTSIDE_LIMITS) == 0)                            # evaluated after that OR
    edge = np.full((T, R), np.nan)
    edge[0] = np.inf                                                                       # the start edge is never swept
    for t in range(1, T):
        for i in range(R):
            if eligible[t, i]:
                edge[t, i] = edge_margin_of(t, i)
    counted = eligible.copy()
    counted[1:] &= edge[1:] >= 0.0
    return status, eligible, edge, counted


def pick(counted, lengths, S):
    """Selection per instance from the counted flags (T, B·S) and the (B, S) lengths: (seed_index, n_tracked, n_complete)."""
    T, R = counted.shape
    B = R // S
    counts = counted.sum(axis=0).reshape(B, S)
    seed = np.array([tmref.select(counts[b], lengths[b]) for b in range(B)])
    return seed, counts[np.arange(B), seed], (counts == T).sum(axis=1), counts


def lengths_of(model, q, q_all, S, weights=None):
    """(B, S) path lengths by trajectory_multistart_ref.score, q_{-1} = q[b]."""
    q_all = np.asarray(q_all, dtype=np.float64)
    T, R = q_all.shape[:2]
    B = R // S
    paths = tmref.by_instance(q_all, B, S)
    one, zero = np.ones(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
    return np.array([[tmref.score(model, q[b], paths[b, s], one, zero, weights)[1] for s in range(S)] for b in range(B)])


def rule(model, limits, q, q_all, converged_all, status_all, S, M, weights=None, edges=True):
    """The whole rule on time-major candidates q_all (T, B·S, nq); converged_all None: every row, status_all None: zeros (the
    selection alone).  `edges` False: the nodes' verdict only (what a caller gets from the status bit without a sweep)."""
    q, q_all = np.asarray(q, dtype=np.float64), np.asarray(q_all, dtype=np.float64)
    T, R, nq = q_all.shape
    B = R // S
    cv = np.ones((T, R), np.int32) if converged_all is None else np.asarray(converged_all)
    st = np.zeros((T, R), np.int32) if status_all is None else np.asarray(status_all)
    finite = np.isfinite(q_all).all(axis=2)
    nm = np.full((T, R), np.nan)                               # (a row with a NaN or an infinite entry: margin NaN)
    nm[finite] = cr.clearance(model, limits, q_all[finite]).margin
    swept = []

    def edge_margin_of(t, i):
        swept.append((t, i))
        return swref.sweep(model, limits, q_all[t - 1, i], q_all[t, i], M).margin[0] if edges else np.inf

    status, eligible, edge, counted = flags(cv, st, nm, edge_margin_of)
    lengths = lengths_of(model, q, q_all, S, weights)
    seed, n_tracked, n_complete, counts = pick(counted, lengths, S)
    rows = np.arange(B)
    ch = lambda x: tmref.chosen(x, seed, S)
    ch_el, ch_edge = ch(eligible), ch(edge)
    collision = ch_el & ~(ch_edge >= 0.0)                      # swept and colliding
    collision[:, 0] = False
    return dict(seed_index=seed, n_tracked=n_tracked, n_complete=n_complete, path_length=lengths[rows, seed], q_path=ch(q_all),
                node_margin=ch(nm), edge_margin=ch_edge, edge_collision=collision, n_edge_collisions=collision.sum(axis=1),
                tracked=ch(counted), node_margin_all=nm, edge_margin_all=edge, status_all=status, eligible=eligible,
                counted=counted, counts=counts, lengths=lengths, swept=swept)
