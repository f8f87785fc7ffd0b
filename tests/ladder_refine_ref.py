"""Restatement of the ladder refinement pass (include/minkhip.h, "THE RULE OF THE REFINEMENT"): the two sweeps over a working
copy of the path, the acceptance of a repair, and the guard that returns the working copy only on a strictly smaller key.
Written from the header's text, not from the kernels.  The loop is a CALLABLE — loop(t, start (B, nq)) -> (x (B, nq), v (B, nv),
status (B,), iters (B,), converged (B,)), one call per waypoint of a sweep on ALL instances, as the device launches it — so that
the CPU tests can run the rule against a table of canned results and the GPU tests against the solve kernels themselves.  The
edge cost is ladder_ref.edge_costs, row by row."""

import numpy as np

import ladder_ref as ref


def row_costs(model, a, b, weights=None):
    """c(a[i] -> b[i]) for every row i: a, b (B, nq) -> (B,)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array([ref.edge_costs(model, b[i:i + 1], a[i:i + 1], weights)[0, 0] for i in range(len(a))])


def tracks(status, converged):
    """A loop result tracks: converged, and no status bit but MKH_ST_OUTSIDE_LIMITS."""
    return (np.asarray(converged) != 0) & ((np.asarray(status) & ~1) == 0)


def key_of(model, q0, path, trk, max_step_sq, weights=None):
    """((lost, breaks, length), edge_break (T,)) of ONE instance's path (T, nq) from q0 (nq,), length accumulated in ascending t."""
    T = len(path)
    prev = np.concatenate([np.asarray(q0, dtype=np.float64)[None], path[:-1]], axis=0)
    c = row_costs(model, prev, path, weights)
    brk = np.array([0] + [1 if c[t] > max_step_sq else 0 for t in range(1, T)], dtype=np.int32)
    length = 0.0
    for t in range(T):
        length = length + float(c[t])
    return (int((np.asarray(trk) == 0).sum()), int(brk.sum()), length), brk


def refine(model, loop, q, q_path, tracked, max_step_sq=np.inf, weights=None, v=None, status=None, iters=None, converged=None,
           judged=None):
    """mkh_ladder_refine on host arrays: q (B, nq), q_path (B, T, nq), tracked (B, T) or None (every node).  v, status, iters,
    converged: the caller's rows (zeros when None); the rows of repaired nodes of a returned working path are replaced.
    `judged`: a list that collects every edge cost held against the gate, with the instance it belongs to.  Returns a dict."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(q_path, dtype=np.float64)
    B, T, nq = p.shape
    p_trk = np.ones((B, T), dtype=np.int32) if tracked is None else (np.asarray(tracked) != 0).astype(np.int32)
    r, r_trk, rep = p.copy(), p_trk.copy(), np.zeros((B, T), dtype=np.int32)
    rows = {}                                                        # (b, t) -> the loop's (v, status, iters, converged)
    gate = float(max_step_sq)

    def note(c, who):
        if judged is not None:
            judged.extend((int(b), float(c[b])) for b in who)

    def sweep(ts, direction):
        for t in ts:
            if direction > 0:
                frm = r[:, t - 1] if t else q
                c = row_costs(model, frm, r[:, t], weights) if t else np.zeros(B)
            else:
                frm = r[:, t + 1]
                c = row_costs(model, r[:, t], frm, weights)
            judge = (r_trk[:, t] != 0) & (t >= 1 or direction < 0)   # (a lost node is bad whatever its edge; the start edge is exempt)
            note(c, np.flatnonzero(judge))
            bad = (r_trk[:, t] == 0) | (judge & (c > gate))
            start = np.where(bad[:, None], frm, r[:, t])
            x, xv, xst, xit, xcv = loop(t, np.ascontiguousarray(start))
            ok = bad & tracks(xst, xcv)
            if direction > 0:
                cx = row_costs(model, frm, x, weights) if t else np.zeros(B)
                gated = t >= 1
            else:
                cx = row_costs(model, x, frm, weights)
                gated = True
            if gated:
                note(cx, np.flatnonzero(ok))
                ok = ok & ~(cx > gate)
            for b in np.flatnonzero(ok):
                r[b, t], r_trk[b, t], rep[b, t] = x[b], 1, (1 if direction > 0 else 2)
                rows[(int(b), t)] = (np.array(xv[b]), int(xst[b]), int(xit[b]), int(xcv[b]))

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
               key_in=[], key_work=[], work_repaired=rep)         # (the last three: what the guard saw, for the tests' conditions)
    for b in range(B):
        key_p, brk_p = key_of(model, q[b], p[b], p_trk[b], gate, weights)
        key_r, brk_r = key_of(model, q[b], r[b], r_trk[b], gate, weights)
        out["key_in"].append(key_p); out["key_work"].append(key_r)
        take = key_r < key_p                                         # strictly smaller, lexicographically
        key, brk = (key_r, brk_r) if take else (key_p, brk_p)
        out["q"][b] = r[b] if take else p[b]
        out["tracked"][b] = r_trk[b] if take else p_trk[b]
        out["refined"][b] = int(take)
        out["edge_break"][b] = brk
        out["n_tracked"][b], out["n_breaks"][b], out["path_length"][b] = T - key[0], key[1], key[2]
        if take:
            out["repaired"][b] = rep[b]
            for t in np.flatnonzero(rep[b]):
                out["v"][b, t], out["status"][b, t], out["iters"][b, t], out["converged"][b, t] = rows[(b, int(t))]
    return out
