"""numpy restatement of THE RULE "with a checker" (include/minkhip.h, mkh_ladder_select_free): ladder_ref.search with the amended
first component of the key — waypoint t is lost when its node is not tracked by the effective flag or the edge into it collides
— and the nodes / edges stage in front of it (clearance_ref, swept_ref).  Written from the header's text."""

import itertools

import numpy as np

import clearance_ref as cr
import ladder_ref as lref
import swept_ref as sref


def search(start, edges, lost, blocked, max_step_sq=np.inf):
    """ladder_ref.search on ONE instance with the mask: blocked (T, S, S), blocked[t][s'][s] = 1 where the edge from node
    (t - 1, s) to node (t, s') collides (blocked[0] unused).  Returns (node_index (T,), (lost, breaks, length), edge_break (T,),
    edge_collision (T,))."""
    T, S = np.asarray(lost).shape
    K = [(int(lost[0][s]), 0, float(start[s])) for s in range(S)]
    pred = [[0] * S]
    for t in range(1, T):
        new, back = [], []
        for s1 in range(S):
            best, arg = None, 0
            for s in range(S):
                c = float(edges[t][s1][s])
                gone = int(lost[t][s1]) | int(blocked[t][s1][s])
                cand = (K[s][0] + gone, K[s][1] + (1 if c > max_step_sq else 0), K[s][2] + c)
                if best is None or cand < best:                 # strict: a tie keeps the lowest s
                    best, arg = cand, s
            new.append(best); back.append(arg)
        K = new
        pred.append(back)
    end = min(range(S), key=lambda s: (K[s], s))
    path = [end]
    for t in range(T - 1, 0, -1):
        path.append(pred[t][path[-1]])
    path = path[::-1]
    brk = [0] + [1 if float(edges[t][path[t]][path[t - 1]]) > max_step_sq else 0 for t in range(1, T)]
    col = [0] + [int(blocked[t][path[t]][path[t - 1]]) for t in range(1, T)]
    return np.array(path, dtype=np.int32), K[end], np.array(brk, dtype=np.int32), np.array(col, dtype=np.int32)


def brute_force(start, edges, lost, blocked, max_step_sq=np.inf):
    """The same answer by enumeration of all S^T paths under the amended key (ladder_ref.brute_force's tie order)."""
    T, S = np.asarray(lost).shape
    best = None
    for path in itertools.product(range(S), repeat=T):
        n_lost, n_brk, length = int(lost[0][path[0]]), 0, float(start[path[0]])
        for t in range(1, T):
            c = float(edges[t][path[t]][path[t - 1]])
            n_lost += int(lost[t][path[t]]) | int(blocked[t][path[t]][path[t - 1]])
            n_brk += 1 if c > max_step_sq else 0
            length = length + c
        cand = ((n_lost, n_brk, length), path[::-1])
        if best is None or cand < best:
            best = cand
    path = best[1][::-1]
    brk = [0] + [1 if float(edges[t][path[t]][path[t - 1]]) > max_step_sq else 0 for t in range(1, T)]
    col = [0] + [int(blocked[t][path[t]][path[t - 1]]) for t in range(1, T)]
    return np.array(path, dtype=np.int32), best[0], np.array(brk, dtype=np.int32), np.array(col, dtype=np.int32)


def margins(model, limits, q_nodes, tracked_nodes, n_samples):
    """The stage in front of the search on (B, T, S, nq) nodes: node_margin (B, T, S), the effective flags (B, T, S) and
    edge_margin_all (B, T, S, S) [b, t, s', s] — NaN for t = 0 and for an edge whose destination is not effectively tracked."""
    q_nodes = np.asarray(q_nodes, dtype=np.float64)
    B, T, S, nq = q_nodes.shape
    trk = np.ones((B, T, S), dtype=bool) if tracked_nodes is None else np.asarray(tracked_nodes) != 0
    node_margin = cr.clearance(model, limits, q_nodes.reshape(-1, nq)).margin.reshape(B, T, S)
    eff = trk & (node_margin >= 0.0)
    em = np.full((B, T, S, S), np.nan)
    idx = [(b, t, s1, s) for b in range(B) for t in range(1, T) for s1 in range(S) if eff[b, t, s1] for s in range(S)]
    if idx:
        a = np.stack([q_nodes[b, t - 1, s] for b, t, s1, s in idx])
        c = np.stack([q_nodes[b, t, s1] for b, t, s1, s in idx])
        sw = sref.sweep(model, limits, a, c, n_samples)
        for (b, t, s1, s), m in zip(idx, sw.margin):
            em[b, t, s1, s] = m
    return node_margin, eff, em


def select(model, limits, q, q_nodes, tracked_nodes=None, weights=None, max_step_sq=np.inf, n_samples=8, stage=None):
    """mkh_ladder_select_free on host arrays.  `stage`: margins() of the same nodes, computed before.  Returns ladder_ref.select's
    dict and edge_collision (B, T), n_edge_collisions (B,), edge_margin (B, T), node_margin, edge_margin_all."""
    q_nodes = np.asarray(q_nodes, dtype=np.float64)
    B, T, S, nq = q_nodes.shape
    node_margin, eff, em = stage if stage is not None else margins(model, limits, q_nodes, tracked_nodes, n_samples)
    swept = np.zeros((B, T, S, S), dtype=bool)
    swept[:, 1:] = eff[:, 1:, :, None]
    blocked = swept & ~(em >= 0.0)
    out = dict(node_index=np.zeros((B, T), np.int32), n_tracked=np.zeros(B, np.int32), n_breaks=np.zeros(B, np.int32),
               path_length=np.zeros(B), edge_break=np.zeros((B, T), np.int32), q_path=np.zeros((B, T, nq)),
               edge_collision=np.zeros((B, T), np.int32), n_edge_collisions=np.zeros(B, np.int32), edge_margin=np.zeros((B, T)),
               node_margin=node_margin, edge_margin_all=em, blocked=blocked, tracked=eff)
    for b in range(B):
        start, edges = lref.costs(model, q[b], q_nodes[b], weights)
        path, key, brk, col = search(start, edges, ~eff[b], blocked[b], max_step_sq)
        out["node_index"][b], out["edge_break"][b], out["edge_collision"][b] = path, brk, col
        out["n_tracked"][b], out["n_breaks"][b], out["path_length"][b] = T - key[0], key[1], key[2]
        out["n_edge_collisions"][b] = col.sum()
        out["q_path"][b] = q_nodes[b, np.arange(T), path]
        out["edge_margin"][b, 0] = np.inf
        for t in range(1, T):
            out["edge_margin"][b, t] = em[b, t, path[t], path[t - 1]]
    return out
