"""numpy restatement of the ladder on deduplicated nodes (include/minkhip.h, mkh_solve_trajectory_ladder_nodes), composed from the
restatements of its parts: the unwinding (unwind_ref), the rule of the set per rung (solution_set_ref.select_cover) and the
ladder's recurrence on the (B, T, K) nodes (ladder_ref.select).  It starts from the loops' results, which are multi-start's."""

from typing import NamedTuple

import numpy as np

import ladder_ref
import solution_set_ref as ss
import unwind_ref


class Nodes(NamedTuple):
    """The nodes of every rung: `q` (B, T, K, nq), `tracked` (B, T, K), the slots' `seed_index`, `multiplicity`, `distance`
    (B, T, K), the rungs' `n_distinct`, `n_converged`, `n_uncovered` (B, T), `near_tie` (B, T): a decision of the rung's
    selection lay within 1e-9 relative of a tie, and `candidates` (B, T, S, nq): the rows the selection ran on."""
    q: np.ndarray
    tracked: np.ndarray
    seed_index: np.ndarray
    multiplicity: np.ndarray
    distance: np.ndarray
    n_distinct: np.ndarray
    n_converged: np.ndarray
    n_uncovered: np.ndarray
    near_tie: np.ndarray
    candidates: np.ndarray


def nodes(model, q, q_all, tracked_all, K, r, weights=None, unwind=False) -> Nodes:
    """q (B, nq), the loops' q_all (B, T, S, nq) and tracked flags (B, T, S) -> the K nodes of every rung."""
    q_all = np.asarray(q_all, dtype=np.float64)
    B, T, S, nq = q_all.shape
    trk = np.asarray(tracked_all) != 0
    cand = q_all.copy()
    if unwind:
        cand = unwind_ref.unwind(model, q_all.reshape(B * T * S, nq), q, T * S).reshape(B, T, S, nq)
    out = Nodes(np.empty((B, T, K, nq)), np.zeros((B, T, K), bool), np.empty((B, T, K), np.int32), np.empty((B, T, K), np.int32),
                np.empty((B, T, K)), *[np.zeros((B, T), np.int32) for _ in range(3)], np.zeros((B, T), bool), cand)
    for b in range(B):
        for t in range(T):
            sel = ss.select_cover(model, cand[b, t], trk[b, t], q[b], K, r, weights)
            out.seed_index[b, t], out.multiplicity[b, t], out.distance[b, t] = sel.seed_index, sel.multiplicity, sel.distance
            out.n_distinct[b, t], out.n_converged[b, t], out.n_uncovered[b, t] = sel.n_distinct, sel.n_eligible, sel.n_uncovered
            out.near_tie[b, t] = ss.near_tie(sel)
            for j in range(K):
                out.q[b, t, j] = cand[b, t, sel.seed_index[j] if j < sel.n_distinct else 0]     # (an empty slot: candidate 0)
            out.tracked[b, t] = np.arange(K) < sel.n_distinct
    return out


def solve(model, q, q_all, tracked_all, K, r, weights=None, max_step_sq=np.inf, unwind=False):
    """(Nodes, ladder_ref.select's dict on them, seed_index (B, T) of the chosen nodes)."""
    n = nodes(model, q, q_all, tracked_all, K, r, weights, unwind)
    path = ladder_ref.select(model, q, n.q, n.tracked, weights, max_step_sq)
    B, T = path["node_index"].shape
    chosen = n.seed_index[np.arange(B)[:, None], np.arange(T)[None, :], path["node_index"]]
    return n, path, chosen
