"""numpy restatement of the ladder-graph search (include/minkhip.h, mkh_ladder_select "THE RULE"): the edge cost, the break gate,
the three-level key, the recurrence with its tie order, the back-trace and the outputs.  Written from the header's text, not
from the kernel.  The edge cost is multistart_ref.distance's arithmetic, vectorised over a whole rung (edge_costs; the CPU
tests hold the two against each other); everything else is plain Python on tuples, so that the tie order can be read off."""

import itertools

import numpy as np

import multistart_ref as msref

JNT_FREE, JNT_BALL = 0, 1
DBL_MAX = np.finfo(np.float64).max

tracked = msref.eligible          # converged and no status bit but MKH_ST_OUTSIDE_LIMITS


def _rotation_difference(a, b):
    """mju_subQuat per pair: the rotation vector of conj(b)·a — a (n, 4), b (m, 4) -> (n, m, 3)."""
    aw, ax, ay, az = (a[:, None, k] for k in range(4))
    bw, bx, by, bz = b[None, :, 0], -b[None, :, 1], -b[None, :, 2], -b[None, :, 3]         # conj(b)
    w = bw * aw - bx * ax - by * ay - bz * az
    x = bw * ax + bx * aw + by * az - bz * ay
    y = bw * ay - bx * az + by * aw + bz * ax
    z = bw * az + bx * ay - by * ax + bz * aw
    with np.errstate(invalid="ignore", divide="ignore"):
        sn = np.sqrt(x * x + y * y + z * z)
        small = sn < 1e-15
        inv = np.where(small, 1.0, sn)
        axis = np.stack([np.where(small, 1.0, x / inv), np.where(small, 0.0, y / inv), np.where(small, 0.0, z / inv)], axis=-1)
        speed = 2.0 * np.arctan2(sn, w)
        speed = np.where(speed > np.pi, speed - 2.0 * np.pi, speed)
    return axis * speed[..., None]


def edge_costs(model, dst, src, weights=None):
    """c[i, j] of the edges from src[j] to dst[i] — dst (n, nq), src (m, nq): d = sum_k w_k ((dst (-) src)_k)^2 with
    mj_differentiatePos at dt = 1, accumulated joint by joint as the device function does; c = d when 0 <= d <= DBL_MAX, else +inf."""
    dst, src = np.asarray(dst, dtype=np.float64), np.asarray(src, dtype=np.float64)
    w = np.ones(model.nv) if weights is None else np.asarray(weights, dtype=np.float64)
    d = np.zeros((dst.shape[0], src.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(model.njnt):
            jt, qa, va = int(model.jnt_type[j]), int(model.jnt_qposadr[j]), int(model.jnt_dofadr[j])
            if jt not in (JNT_FREE, JNT_BALL):
                dv = dst[:, None, qa] - src[None, :, qa]
                d = d + w[va] * dv * dv
                continue
            if jt == JNT_FREE:
                for k in range(3):
                    dv = dst[:, None, qa + k] - src[None, :, qa + k]
                    d = d + w[va + k] * dv * dv
                qa, va = qa + 3, va + 3
            dw = _rotation_difference(dst[:, qa:qa + 4], src[:, qa:qa + 4])
            d = d + (w[va] * dw[..., 0] * dw[..., 0] + w[va + 1] * dw[..., 1] * dw[..., 1] + w[va + 2] * dw[..., 2] * dw[..., 2])
        ok = (d >= 0.0) & (d <= DBL_MAX)
    return np.where(ok, d, np.inf)


def costs(model, q0, q_nodes, weights=None):
    """Every edge cost of ONE instance: start (S,) from q0 (nq,), and edges (T, S, S) with edges[t, s', s] the cost from node
    (t - 1, s) to node (t, s') (edges[0] is unused and zero)."""
    q_nodes = np.asarray(q_nodes, dtype=np.float64)
    T, S = q_nodes.shape[:2]
    start = edge_costs(model, q_nodes[0], np.asarray(q0, dtype=np.float64)[None], weights)[:, 0]
    edges = np.zeros((T, S, S))
    for t in range(1, T):
        edges[t] = edge_costs(model, q_nodes[t], q_nodes[t - 1], weights)
    return start, edges


def search(start, edges, lost, max_step_sq=np.inf):
    """The recurrence on ONE instance's costs: start (S,), edges (T, S, S), lost (T, S) (1 where a node is NOT tracked).
    Returns (node_index (T,), (lost, breaks, length), edge_break (T,))."""
    T, S = np.asarray(lost).shape
    K = [(int(lost[0][s]), 0, float(start[s])) for s in range(S)]
    pred = [[0] * S]
    for t in range(1, T):
        new, back = [], []
        for s1 in range(S):
            best, arg = None, 0
            for s in range(S):
                c = float(edges[t][s1][s])
                cand = (K[s][0] + int(lost[t][s1]), K[s][1] + (1 if c > max_step_sq else 0), K[s][2] + c)
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
    return np.array(path, dtype=np.int32), K[end], np.array(brk, dtype=np.int32)


def brute_force(start, edges, lost, max_step_sq=np.inf):
    """The same answer by enumeration of all S^T paths: the smallest (key, path) — among paths of equal key the recurrence's
    tie order (lowest end node, then lowest predecessor walking back) is the smallest path read from the END."""
    T, S = np.asarray(lost).shape
    best = None
    for path in itertools.product(range(S), repeat=T):
        n_lost, n_brk, length = int(lost[0][path[0]]), 0, float(start[path[0]])
        for t in range(1, T):
            c = float(edges[t][path[t]][path[t - 1]])
            n_lost += int(lost[t][path[t]])
            n_brk += 1 if c > max_step_sq else 0
            length = length + c
        cand = ((n_lost, n_brk, length), path[::-1])
        if best is None or cand < best:
            best = cand
    path = best[1][::-1]
    brk = [0] + [1 if float(edges[t][path[t]][path[t - 1]]) > max_step_sq else 0 for t in range(1, T)]
    return np.array(path, dtype=np.int32), best[0], np.array(brk, dtype=np.int32)


def select(model, q, q_nodes, tracked_nodes=None, weights=None, max_step_sq=np.inf):
    """mkh_ladder_select on host arrays: q (B, nq), q_nodes (B, T, S, nq), tracked_nodes (B, T, S) or None (every node).
    Returns dict(node_index (B, T), n_tracked, n_breaks, path_length (B,), edge_break (B, T), q_path (B, T, nq))."""
    q_nodes = np.asarray(q_nodes, dtype=np.float64)
    B, T, S, nq = q_nodes.shape
    trk = np.ones((B, T, S), dtype=bool) if tracked_nodes is None else np.asarray(tracked_nodes) != 0
    out = dict(node_index=np.zeros((B, T), np.int32), n_tracked=np.zeros(B, np.int32), n_breaks=np.zeros(B, np.int32),
               path_length=np.zeros(B), edge_break=np.zeros((B, T), np.int32), q_path=np.zeros((B, T, nq)))
    for b in range(B):
        start, edges = costs(model, q[b], q_nodes[b], weights)
        path, key, brk = search(start, edges, ~trk[b], max_step_sq)
        out["node_index"][b], out["edge_break"][b] = path, brk
        out["n_tracked"][b], out["n_breaks"][b], out["path_length"][b] = T - key[0], key[1], key[2]
        out["q_path"][b] = q_nodes[b, np.arange(T), path]
    return out


def path_key(start, edges, lost, path, max_step_sq=np.inf):
    """(lost, breaks, length) of a GIVEN path of one instance, accumulated as the rule says."""
    n_lost, n_brk, length = int(lost[0][path[0]]), 0, float(start[path[0]])
    for t in range(1, len(path)):
        c = float(edges[t][path[t]][path[t - 1]])
        n_lost += int(lost[t][path[t]])
        n_brk += 1 if c > max_step_sq else 0
        length = length + c
    return n_lost, n_brk, length


def search_fast(start, edges, lost, max_step_sq=np.inf):
    """search(), the loop over (s', s) vectorised in numpy — what a host caller would write around solve_multistart (the bench
    tool's host composition).  Same key, same tie order."""
    lost = np.asarray(lost).astype(np.int64)
    T, S = lost.shape
    cnt = lost[0] << 16
    length = np.asarray(start, dtype=np.float64).copy()
    pred = np.zeros((T, S), dtype=np.int64)
    for t in range(1, T):
        c = edges[t]                                                        # (s', s)
        cand_cnt = cnt[None, :] + (c > max_step_sq)
        cand_len = length[None, :] + c
        lowest = cand_cnt.min(axis=1, keepdims=True)
        masked = np.where(cand_cnt == lowest, cand_len, np.inf)
        shortest = masked.min(axis=1, keepdims=True)
        arg = ((cand_cnt == lowest) & (masked == shortest)).argmax(axis=1)  # the first True: the lowest s
        rows = np.arange(S)
        cnt, length, pred[t] = cand_cnt[rows, arg] + (lost[t] << 16), cand_len[rows, arg], arg
    end = int(np.lexsort((np.arange(S), length, cnt))[0])
    path = [end]
    for t in range(T - 1, 0, -1):
        path.append(int(pred[t][path[-1]]))
    path = np.array(path[::-1], dtype=np.int32)
    brk = np.array([0] + [int(edges[t][path[t]][path[t - 1]] > max_step_sq) for t in range(1, T)], dtype=np.int32)
    return path, (int(cnt[end] >> 16), int(cnt[end] & 0xffff), float(length[end])), brk
