"""numpy restatement of the distinct-set rule (include/minkhip.h "THE RULE OF THE SET": mkh_select_distinct,
mkh_solve_multistart_set), twice: the cover formulation the header states and the sorted greedy walk it says this equals.
Written from the header's text, not from the kernel; distances and eligibility are multi-start's (tests/multistart_ref.py)."""

from typing import NamedTuple

import numpy as np

import multistart_ref as ms

DBL_MAX = np.finfo(np.float64).max


class Selection(NamedTuple):
    """One target's set for K slots: per slot `seed_index` (−1: empty), `multiplicity` (0), `distance` (+inf); `n_distinct`,
    `n_eligible`, `n_uncovered`; `margin`: the smallest relative distance of any decision of the walk from a tie (inf: no
    decision was made) — see near_tie()."""
    seed_index: np.ndarray
    multiplicity: np.ndarray
    distance: np.ndarray
    n_distinct: int
    n_eligible: int
    n_uncovered: int
    margin: float


def d_ref(model, q_cand, q_ref, weights=None):
    """(S,) d(q_s, q_ref), a NaN or infinite value replaced by DBL_MAX."""
    d = np.array([ms.distance(model, q, q_ref, weights) for q in q_cand], dtype=np.float64)
    return np.where(np.isfinite(d), d, DBL_MAX)


def _same_row(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


class _Pairs:
    """d(q_s, q_t) on demand, each pair priced once."""

    def __init__(self, model, q_cand, weights):
        self.model, self.q, self.w, self.memo = model, q_cand, weights, {}

    def __call__(self, s, t):
        if (s, t) not in self.memo:
            self.memo[(s, t)] = ms.distance(self.model, self.q[s], self.q[t], self.w)
        return self.memo[(s, t)]


def _rel_gap(a, b):
    m = max(abs(a), abs(b))
    return np.inf if m == 0.0 or not np.isfinite(m) else abs(a - b) / m


def _empty(K):
    return np.full(K, -1, dtype=np.int32), np.zeros(K, dtype=np.int32), np.full(K, np.inf)


def select_cover(model, q_cand, ok, q_ref, K, r, weights=None, dref=None):
    """The rule as the header states it: per slot the uncovered eligible candidate with the smallest d_ref (ties: the lowest
    index) becomes the representative and covers what lies within r of it."""
    q_cand = np.asarray(q_cand, dtype=np.float64)
    ok = np.asarray(ok, dtype=bool)
    S = len(q_cand)
    dr = d_ref(model, q_cand, q_ref, weights) if dref is None else np.asarray(dref, dtype=np.float64)
    pair = _Pairs(model, q_cand, weights)
    seed_index, mult, dist = _empty(K)
    uncovered = ok.copy()
    r2, margin, j = r * r, np.inf, 0
    while j < K and uncovered.any():
        idx = np.flatnonzero(uncovered)
        dmin = dr[idx].min()
        rep = int(idx[dr[idx] == dmin][0])
        others = np.sort(dr[idx])[1:2]
        if len(others):
            margin = min(margin, _rel_gap(float(others[0]), float(dmin)))
        n = 0
        for s in idx:
            d = 0.0 if s == rep else pair(int(s), rep)
            if s != rep:
                margin = min(margin, _rel_gap(d, r2) if r2 > 0.0 or d > 0.0 else np.inf)
            if s == rep or d <= r2 or _same_row(q_cand[s], q_cand[rep]):
                uncovered[s] = False
                n += 1
        seed_index[j], mult[j], dist[j] = rep, n, dmin
        j += 1
    return Selection(seed_index, mult, dist, j, int(ok.sum()), int(uncovered.sum()), float(margin))


def select_walk(model, q_cand, ok, q_ref, K, r, weights=None, dref=None):
    """The same set by the greedy walk: the eligible candidates in ascending (d_ref, index); one is kept iff it is farther than r
    from every candidate kept before it (and a slot is left), else it counts for the first kept one within r."""
    q_cand = np.asarray(q_cand, dtype=np.float64)
    ok = np.asarray(ok, dtype=bool)
    dr = d_ref(model, q_cand, q_ref, weights) if dref is None else np.asarray(dref, dtype=np.float64)
    pair = _Pairs(model, q_cand, weights)
    seed_index, mult, dist = _empty(K)
    order = sorted(np.flatnonzero(ok), key=lambda s: (dr[s], s))
    r2, kept, left = r * r, [], 0
    for s in order:
        s = int(s)
        home = next((j for j, k in enumerate(kept) if pair(s, k) <= r2 or _same_row(q_cand[s], q_cand[k])), None)
        if home is not None:
            mult[home] += 1
        elif len(kept) < K:
            seed_index[len(kept)], mult[len(kept)], dist[len(kept)] = s, 1, dr[s]
            kept.append(s)
        else:
            left += 1
    return Selection(seed_index, mult, dist, len(kept), int(ok.sum()), left, np.inf)


def near_tie(sel: Selection, rel: float = 1e-9) -> bool:
    """Whether a decision of select_cover lay within a relative `rel` of a tie: two d_ref of uncovered candidates, or a d
    against r²."""
    return sel.margin <= rel
