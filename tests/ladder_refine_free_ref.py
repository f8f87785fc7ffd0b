"""Restatement of the ladder refinement pass with a checker (include/minkhip.h, "THE RULE OF THE REFINEMENT, with a checker"): the
state of a path — node margins, effective flags, swept edge margins —, the two sweeps with their amended bad and acceptance
tests, the margins a commit maintains, and the guard on the checked ladder's key.  Written from the header's text, not from the
kernels.  It extends ladder_refine_ref.refine's shape: the loop is a CALLABLE loop(t, start (B, nq)) -> (x, v, status, iters,
converged), one call per waypoint of a sweep on ALL instances.  Margins are clearance_ref.clearance's and swept_ref.sweep's;
`limits` as those take them."""

import numpy as np

import clearance_ref as cr
import ladder_refine_ref as rref
import swept_ref as sref

COUNTERS = ("accepted_forward", "accepted_backward", "rejected_node", "rejected_edge", "rejected_gate", "far_edges")


def node_margins(model, limits, rows):
    """margin of every row, (N, nq) -> (N,)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, model.nq)
    return cr.clearance(model, limits, rows).margin if len(rows) else np.zeros(0)


def edge_margin(model, limits, a, b, M):
    """The swept margin of ONE edge a -> b."""
    return float(sref.sweep(model, limits, a[None], b[None], M).margin[0])


def path_state(model, limits, path, tracked, M, margins=None):
    """(node_margin (T,), effective (T,) int32, edge_margin (T,)) of ONE path (T, nq): the edge into t is swept iff t >= 1 and
    waypoint t is effectively tracked, else NaN; entry 0 is +inf."""
    T = len(path)
    nm = node_margins(model, limits, path)
    eff = ((np.asarray(tracked) != 0) & (nm >= 0.0)).astype(np.int32)
    em = np.full(T, np.nan)
    em[0] = np.inf
    for t in range(1, T):
        if eff[t]:
            em[t] = edge_margin(model, limits, path[t - 1], path[t], M)
    if margins is not None:
        margins.extend(float(x) for x in nm[np.asarray(tracked) != 0])
        margins.extend(float(x) for x in em[1:][eff[1:] != 0])
    return nm, eff, em


def collides(eff_dst, em):
    """An edge collides iff it was swept — its destination is effectively tracked — and !(margin >= 0)."""
    return bool(eff_dst) and not (em >= 0.0)


def key_of(model, q0, path, eff, em, max_step_sq, weights=None):
    """((lost, breaks, length), edge_break (T,), edge_collision (T,)) of ONE path under the amended key."""
    (lost0, breaks, length), brk = rref.key_of(model, q0, path, eff, max_step_sq, weights)
    T = len(path)
    col = np.array([0] + [1 if collides(eff[t], em[t]) else 0 for t in range(1, T)], dtype=np.int32)
    lost = int(((np.asarray(eff) == 0) | (col != 0)).sum())
    assert lost == lost0 + int(col.sum())                            # (a colliding edge enters a tracked node: the two are disjoint)
    return (lost, breaks, length), brk, col


def refine(model, limits, loop, q, q_path, tracked, n_samples, max_step_sq=np.inf, weights=None, v=None, status=None, iters=None,
           converged=None, judged=None, margins=None, counts=None):
    """mkh_ladder_refine_free on host arrays; the arguments of ladder_refine_ref.refine with the checker's `limits` and n_samples.
    `judged`: every edge cost held against the gate, with its instance; `margins`: every margin held against zero; `counts`: a
    dict that receives COUNTERS.  Returns a dict."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(q_path, dtype=np.float64)
    B, T, nq = p.shape
    M = int(n_samples)
    assert M >= 1
    cnt = dict.fromkeys(COUNTERS, 0)
    p_flag = np.ones((B, T), dtype=np.int32) if tracked is None else (np.asarray(tracked) != 0).astype(np.int32)
    p_nm, p_eff, p_em = np.empty((B, T)), np.empty((B, T), np.int32), np.empty((B, T))
    for b in range(B):
        p_nm[b], p_eff[b], p_em[b] = path_state(model, limits, p[b], p_flag[b], M, margins)
    r, r_eff, r_nm, r_em = p.copy(), p_eff.copy(), p_nm.copy(), p_em.copy()
    rep = np.zeros((B, T), dtype=np.int32)
    rows = {}
    gate = float(max_step_sq)

    def note(c, who):
        if judged is not None:
            judged.extend((int(b), float(c[b])) for b in who)

    def held(x):
        if margins is not None:
            margins.append(float(x))

    def sweep(ts, direction):
        for t in ts:
            if direction > 0:
                frm = r[:, t - 1] if t else q
                c = rref.row_costs(model, frm, r[:, t], weights) if t else np.zeros(B)
                blocked = np.array([t >= 1 and collides(r_eff[b, t], r_em[b, t]) for b in range(B)])
            else:
                frm = r[:, t + 1]
                c = rref.row_costs(model, r[:, t], frm, weights)
                blocked = np.array([collides(r_eff[b, t + 1], r_em[b, t + 1]) for b in range(B)])
            judge = (r_eff[:, t] != 0) & (t >= 1 or direction < 0)
            note(c, np.flatnonzero(judge))
            bad = (r_eff[:, t] == 0) | (judge & (c > gate)) | blocked
            start = np.where(bad[:, None], frm, r[:, t])
            x, xv, xst, xit, xcv = loop(t, np.ascontiguousarray(start))
            cand = np.flatnonzero(bad & rref.tracks(xst, xcv))
            if direction > 0:
                cx = rref.row_costs(model, frm, x, weights) if t else np.zeros(B)
                gated = t >= 1
            else:
                cx = rref.row_costs(model, x, frm, weights)
                gated = True
            if gated:
                note(cx, cand)
            mx = np.full(B, np.nan)
            mx[cand] = node_margins(model, limits, x[cand])
            for b in cand:
                held(mx[b])
                if not (mx[b] >= 0.0):
                    cnt["rejected_node"] += 1
                    continue
                if gated and cx[b] > gate:
                    cnt["rejected_gate"] += 1
                    continue
                # the near edge: forward r_{t-1} -> x (its destination x is free: swept); backward x -> r_{t+1}
                near = np.nan
                if direction > 0 and t >= 1:
                    near = edge_margin(model, limits, r[b, t - 1], x[b], M)
                elif direction < 0 and r_eff[b, t + 1]:
                    near = edge_margin(model, limits, x[b], r[b, t + 1], M)
                swept = (direction > 0 and t >= 1) or (direction < 0 and r_eff[b, t + 1] != 0)
                if swept:
                    held(near)
                    if not (near >= 0.0):
                        cnt["rejected_edge"] += 1
                        continue
                # accepted
                cnt["accepted_forward" if direction > 0 else "accepted_backward"] += 1
                r[b, t], r_eff[b, t], rep[b, t] = x[b], 1, (1 if direction > 0 else 2)
                rows[(int(b), t)] = (np.array(xv[b]), int(xst[b]), int(xit[b]), int(xcv[b]))
                r_nm[b, t] = mx[b]
                if direction > 0:
                    if t >= 1:
                        r_em[b, t] = near
                    if t + 1 < T:                                    # the far edge x -> r_{t+1}
                        r_em[b, t + 1] = edge_margin(model, limits, x[b], r[b, t + 1], M) if r_eff[b, t + 1] else np.nan
                        if r_eff[b, t + 1]:
                            cnt["far_edges"] += 1
                            held(r_em[b, t + 1])
                else:
                    r_em[b, t + 1] = near
                    if t >= 1:                                       # the far edge r_{t-1} -> x: its destination is tracked
                        r_em[b, t] = edge_margin(model, limits, r[b, t - 1], x[b], M)
                        cnt["far_edges"] += 1
                        held(r_em[b, t])

    sweep(range(T), +1)
    sweep(range(T - 2, -1, -1), -1)
    nv = model.nv
    out = dict(q=np.empty_like(p), tracked=np.empty((B, T), np.int32), repaired=np.zeros((B, T), np.int32),
               refined=np.zeros(B, np.int32), edge_break=np.zeros((B, T), np.int32), n_tracked=np.zeros(B, np.int32),
               n_breaks=np.zeros(B, np.int32), path_length=np.zeros(B),
               v=np.zeros((B, T, nv)) if v is None else np.array(v, dtype=np.float64),
               status=np.zeros((B, T), np.int32) if status is None else np.array(status, dtype=np.int32),
               iters=np.zeros((B, T), np.int32) if iters is None else np.array(iters, dtype=np.int32),
               converged=np.zeros((B, T), np.int32) if converged is None else np.array(converged, dtype=np.int32),
               edge_collision=np.zeros((B, T), np.int32), n_edge_collisions=np.zeros(B, np.int32), edge_margin=np.empty((B, T)),
               node_margin=np.empty((B, T)), key_in=[], key_work=[], work_repaired=rep)
    for b in range(B):
        key_p, brk_p, col_p = key_of(model, q[b], p[b], p_eff[b], p_em[b], gate, weights)
        key_r, brk_r, col_r = key_of(model, q[b], r[b], r_eff[b], r_em[b], gate, weights)
        out["key_in"].append(key_p); out["key_work"].append(key_r)
        take = key_r < key_p                                         # strictly smaller, lexicographically
        key, brk, col = (key_r, brk_r, col_r) if take else (key_p, brk_p, col_p)
        out["q"][b] = r[b] if take else p[b]
        out["tracked"][b] = r_eff[b] if take else p_eff[b]
        out["refined"][b] = int(take)
        out["edge_break"][b] = brk
        out["edge_collision"][b], out["n_edge_collisions"][b] = col, int(col.sum())
        out["edge_margin"][b] = r_em[b] if take else p_em[b]
        out["node_margin"][b] = r_nm[b] if take else p_nm[b]
        out["n_tracked"][b], out["n_breaks"][b], out["path_length"][b] = T - key[0], key[1], key[2]
        if take:
            out["repaired"][b] = rep[b]
            for t in np.flatnonzero(rep[b]):
                out["v"][b, t], out["status"][b, t], out["iters"][b, t], out["converged"][b, t] = rows[(b, int(t))]
    if counts is not None:
        counts.update(cnt)
    return out
