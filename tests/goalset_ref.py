"""numpy restatement of the goal-set rule (include/minkhip.h "THE RULE OF THE GOAL SET": mkh_select_goalset,
mkh_solve_goalset).  Written from the header's text, not from the kernel, on top of multi-start's restatement
(tests/multistart_ref.py: draw_seeds, distance, eligible, select).  Level 2 is written twice: as the two-level reduction the
header states, and — for a call without costs and masks — as multi-start's selection over the G·S candidates of a target taken
as one flat list, which the header's third invariant says is the same thing."""

from typing import NamedTuple

import numpy as np

import multistart_ref as ms

DBL_MAX = np.finfo(np.float64).max


class Choice(NamedTuple):
    """One target's result: `goal_index` (nothing reached: the lowest valid goal, −1 when none is valid), `seed_index`,
    `converged`, `n_reached`, `score` (+inf); per goal `seed_index_goal`, `reached`, `n_eligible_goal`, `distance_goal` (+inf)."""
    goal_index: int
    seed_index: int
    converged: bool
    n_reached: int
    score: float
    seed_index_goal: np.ndarray
    reached: np.ndarray
    n_eligible_goal: np.ndarray
    distance_goal: np.ndarray


def draw_seeds(model, q, n_goals, n_seeds, rng_seed=0, target_index0=0):
    """(B, G, S, nq): multi-start's seeds of the B·G flattened pairs — q[b] repeated G times, global target index
    (target_index0 + b)·G + g."""
    q = np.asarray(q, dtype=np.float64)
    B = q.shape[0]
    flat = ms.draw_seeds(model, np.repeat(q, n_goals, axis=0), n_seeds, rng_seed=rng_seed, target_index0=target_index0 * n_goals)
    return flat.reshape(B, n_goals, n_seeds, -1)


def d_ref(model, q_cand, q_ref, weights=None):
    """(G, S) d(q_gs, q_ref), a NaN or infinite value replaced by DBL_MAX."""
    G, S = q_cand.shape[:2]
    d = np.array([[ms.distance(model, q_cand[g, s], q_ref, weights) for s in range(S)] for g in range(G)], dtype=np.float64)
    return np.where(np.isfinite(d), d, DBL_MAX)


def level1(d, eligible):
    """(seed, has) of one goal: the eligible seed with the smallest d, ties to the lowest s — multi-start's select()."""
    s, has, _ = ms.select(d, eligible, np.zeros(len(d), dtype=np.int32))
    return s, has


def select(d, eligible, goal_cost=None, goal_valid=None) -> Choice:
    """The two levels for one target: d (G, S) = d_ref with NaN / inf already replaced, eligible (G, S), goal_cost (G,) or
    None (zeros), goal_valid (G,) or None (every goal)."""
    d = np.asarray(d, dtype=np.float64)
    eligible = np.asarray(eligible) != 0
    G, S = d.shape
    cost = np.zeros(G) if goal_cost is None else np.asarray(goal_cost, dtype=np.float64)
    valid = np.ones(G, dtype=bool) if goal_valid is None else np.asarray(goal_valid) != 0
    seed_goal, reached = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=bool)
    dist_goal = np.full(G, np.inf)
    for g in range(G):
        s, has = level1(d[g], eligible[g])
        if valid[g] and has:
            seed_goal[g], reached[g], dist_goal[g] = s, True, d[g, s]
    best, best_score = -1, np.inf
    for g in range(G):                                     # ascending g: ties keep the lower index; a NaN score never wins
        if not reached[g]:
            continue
        score = np.float64(cost[g]) + np.float64(dist_goal[g])              # one rounded addition
        if score == score and (best < 0 or score < best_score):
            best, best_score = g, score
    if best >= 0:
        return Choice(best, int(seed_goal[best]), True, int(reached.sum()), float(best_score), seed_goal, reached,
                      eligible.sum(axis=1).astype(np.int32), dist_goal)
    lowest = int(np.flatnonzero(valid)[0]) if valid.any() else -1
    return Choice(lowest, 0, False, int(reached.sum()), float("inf"), seed_goal, reached, eligible.sum(axis=1).astype(np.int32),
                  dist_goal)


def select_flat(d, eligible):
    """(goal_index, seed_index, converged) without costs and masks: multi-start's selection over the G·S candidates as one
    flat list, index g·S + s.  Nothing eligible: (0, 0, False) — goal 0 is the lowest valid goal."""
    d = np.asarray(d, dtype=np.float64)
    G, S = d.shape
    i, has, _ = ms.select(d.reshape(-1), (np.asarray(eligible) != 0).reshape(-1), np.zeros(G * S, dtype=np.int32))
    return (i // S, i % S, True) if has else (0, 0, False)
