"""Numpy statement of the product-form active set of the low-rank builds (design aid, not product).

The low-rank start (proto_woodbury.py) leaves the dof block of the sweep tableau as R₀[i][j] = Σ_r Z[r][i]·Z[r][j]/d_r with
the true entry σ_i·σ_j·R[i][j] and the diagonal carried apart.  The kernel used to BUILD that block (n_μ rank-1 updates of 44
rows) and then update all of it in every pivot, although the active set only ever reads one row per pivot.  Here — as in the
kernel's product-form builds (ik_kernel.h kProduct) — the block stays in its factors:

    row col for index j   =   Σ_r Z[r][col]·gz[r][j]   −   Σ_{q < npiv} own_q[col]·g_q[j]        gz[r][j] = Z[r][j]/d_r

with one history slot (g_q, own_q) per past pivot, P slots.  A slot of ONE double (`one_double`) keeps own_q per lane and the
pivot's two wave-uniform scalars (σ_k², 1/d) apart, and re-forms g_q[j] = ((σ_k²)·own_q[j])·(1/d) — the multiplications of the
pivot, in the pivot's order — whenever a row is asked for: the same bits as the stored multiplier (counted in
stats["reformed_unequal"], which must stay 0), at half the registers per slot.  When the history is full the solve starts again from the active
set it has reached — the predicted-active-set start of a warm start — which rebuilds Z and d for that set; nothing is ever
materialised.  Iterations keep counting across such refactorisations (one counts as the P pivots it closes).

The rules are the kernel's: cold-start refinement (the bounds x⁰ violates become the first active set), block steps while each
at least halves the infeasibilities (≤ 3), hand-over releases, Goldfarb–Idnani.

    python tools/proto_product_form.py [n=512] [seed=0] [P=13]   histogram of pivots per solve, share of solves that refactorise
                                                                 at P (two-double slots, then one-double slots)
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

P_DEFAULT = 13            # history slots of the 44-row builds: (44 − 18) / 2


def solve(Dg, c_d, Jw, r, lo, hi, P=P_DEFAULT, cold_refine=True, stats=None, one_double=False):
    """min ½xᵀ(Dg + JwᵀJw)x + (c_d − Jwᵀr)ᵀx, lo ≤ x ≤ hi.  Returns (x, status): 0 solved, 2 infeasible, 4 bad pivot, 8 iteration cap."""
    nv = len(Dg)
    # (the start takes the posture part c_d and the residuals apart: Jw·z̃ − r)
    Jw = np.asarray(Jw, float)

    def start(bound):
        # fold −Jwᵀr into the linear term through the right-hand side, as the kernel does: ω from (Jw·z̃ − r)
        nm = Jw.shape[0]
        free = bound == 0
        dsq = 1.0 / np.sqrt(Dg)
        Jh = Jw * dsq[None, :]
        S = np.eye(nm) + Jh[:, free] @ Jh[:, free].T
        L = np.linalg.cholesky(S)
        dd = np.diag(L).copy()
        L = L / dd[None, :]
        d = dd * dd
        Z = np.linalg.solve(L, Jh)
        quad = (Z * Z / d[:, None]).sum(axis=0)
        beta = np.where(bound == 2, hi, np.where(bound == 1, lo, 0.0))
        zt = np.where(free, -c_d / Dg, beta)
        om = np.linalg.solve(L, Jw @ zt - r)
        zw = (Z * (om / d)[:, None]).sum(axis=0)
        sg = np.where(free, dsq, Dg * dsq)
        D = np.where(free, dsq * dsq * (quad - 1.0), Dg * (1.0 + quad))
        x = np.where(free, -c_d * dsq * dsq - dsq * zw, Dg * beta + c_d + Dg * dsq * zw)
        return Z, d, sg, D, x

    hdiag = Dg + (Jw * Jw).sum(axis=0)
    hmax = hdiag.max()
    tolw = 1e-16 * hmax
    thr = 1e-13 / (hmax * nv)
    max_iters = 8 * (nv + 8)
    if np.any(lo > hi + 1e-12):
        return np.full(nv, np.nan), 2
    bound = np.zeros(nv, int)
    iters = 0
    n_piv = n_refac = n_unequal = 0
    best, outer = 4 * 64, 0                            # block steps: carried across refactorisations (the state is the same state)
    while True:                                        # one pass = one factorisation
        Z, d, sg, D, x = start(bound)
        # (the kernel refines whenever the start has no prediction: also after a refactorisation that reached an empty active set)
        if cold_refine and not bound.any():
            viol = np.where(x > hi, 2, np.where(x < lo, 1, 0))
            if viol.any():
                bound = viol
                Z, d, sg, D, x = start(bound)
        gz = Z / d[:, None]
        basic = bound == 0
        at_hi = bound == 2
        hist = []                                       # (g_q, own_q, σ_k², 1/d): a one-double slot keeps own_q, the scalars are the pivot's
        refac = False

        def row(col):
            nonlocal n_unequal
            acc = Z[:, col] @ gz                        # Σ_r Z[r][col]·gz[r][j]
            for g, own, sk2, inv in hist:
                if one_double:
                    g2 = (sk2 * own) * inv              # the pivot's own multiplications, in its order
                    n_unequal += int((g2 != g).sum())
                    g = g2
                acc = acc - own[col] * g
            acc[col] = 0.0
            return acc

        def pivot(k, own, reverse):
            nonlocal D, sg, n_piv
            dk, sk = D[k], sg[k]
            inv = 1.0 / dk
            ck = sg * sk * own
            sk2 = sk * sk
            g = sk2 * own * inv
            hist.append((g, own, sk2, inv))
            Dn = D - ck * inv * ck
            Dn[k] = -inv
            D = Dn
            sg = sg.copy()
            sg[k] = (-sk if reverse else sk) * inv
            n_piv += 1

        def flip(k, kb, up):
            """clamp a basic dof onto its violated bound (kb) / release a bound dof into the basis"""
            nonlocal x
            own = row(k)
            dk = D[k]
            if not ((-dk if kb else dk) > 0.0):
                return 4
            tau = sg * sg[k] * own
            tau[k] = dk
            beta = hi[k] if up else lo[k]
            alpha = (x[k] - beta) / dk if kb else -x[k] / dk
            x = x + np.where(basic, -alpha, alpha) * tau
            if kb:
                x[k] = alpha; basic[k] = False; at_hi[k] = up
            else:
                x[k] = (hi[k] if at_hi[k] else lo[k]) + alpha; basic[k] = True; at_hi[k] = False
            pivot(k, own, kb)
            return 0

        def wrong():
            y = np.where(at_hi, -x, x)
            return (~basic) & (y < -tolw)

        status = 0
        need_gi = False
        while True:                                     # block steps
            over = basic & (x - hi > 1e-12)
            under = basic & (lo - x > 1e-12)
            todo = over | under | wrong()
            cnt = int(todo.sum())
            if cnt == 0:
                break
            if 2 * cnt > best or outer >= 3:
                need_gi = True
                break
            best = cnt
            for k in np.nonzero(todo)[0]:
                if len(hist) == P:
                    refac = True
                    break
                status |= flip(k, bool(over[k] | under[k]), bool(over[k]))
                if status:
                    break
            outer += 1                                  # (an interrupted block step counts)
            if status or refac:
                break
        while need_gi and not status and not refac:    # hand-over
            w = wrong()
            if not w.any():
                break
            if len(hist) == P:
                refac = True
                break
            iters += 1
            if iters > max_iters:
                status |= 8
                break
            status |= flip(int(np.nonzero(w)[0][0]), False, False)
        p, pend, pend_rev = -1, -1, False
        upper, sgn, acc = False, 1.0, 0.0
        while need_gi and not status and not refac:    # Goldfarb–Idnani
            if pend >= 0:
                col = pend
            else:
                if p < 0:
                    viol = np.maximum(x - hi, lo - x)
                    cand = basic & (viol > 1e-12)
                    if not cand.any():
                        break
                    # (the kernel compares the high words of the violations; "most violated" only steers the path)
                    vh = np.where(cand, viol, -1.0).astype(np.float64).view(np.uint64) >> np.uint64(32)
                    vh = np.where(cand, vh, 0)
                    p = int(np.nonzero(cand & (vh == vh.max()))[0][0])
                    upper = bool(x[p] - hi[p] > lo[p] - x[p])
                    sgn = -1.0 if upper else 1.0
                    acc = 0.0
                iters += 1
                if iters > max_iters:
                    status |= 8
                    break
                col = p
            own = row(col)
            dk = D[col]
            inv = 1.0 / dk
            if pend >= 0:
                rev = pend_rev
                pend = -1
            else:
                tau = sg * sg[col] * own
                tau[col] = dk
                beta = hi[col] if upper else lo[col]
                t2 = abs((x[col] - beta) * inv) if abs(dk) > thr else np.inf
                rr = sgn * tau
                rr = np.where(at_hi, rr, -rr)           # rate of decrease of the multiplier that must stay ≥ 0
                y = np.where(at_hi, -x, x)
                cnd = (~basic) & (rr > 0.0)
                cnd[col] = False
                t = np.where(cnd, np.maximum(y, 0.0) / np.where(cnd, rr, 1.0), np.inf)
                t1 = t.min() if cnd.any() else np.inf
                if not min(t1, t2) < np.inf:
                    status |= 2
                    break
                full = t2 <= t1
                alpha = sgn * (t2 if full else t1)
                x = x + np.where(basic, -alpha, alpha) * tau
                acc += alpha
                if full:
                    x[p] = acc; basic[p] = False; at_hi[p] = upper
                    rev = True
                    p = -1
                else:
                    pend = int(np.nonzero(cnd & (t == t1))[0][0])
                    pend_rev = False
                    x[pend] = hi[pend] if at_hi[pend] else lo[pend]
                    basic[pend] = True; at_hi[pend] = False
                    continue
            if len(hist) == P:
                refac = True
                break
            pivot(col, own, rev)
        if refac:
            iters += P
            if iters > max_iters:
                status |= 8
            else:
                n_refac += 1
                bound = np.where(basic, 0, np.where(at_hi, 2, 1))
                continue
        break
    if stats is not None:
        stats["pivots"] = n_piv
        stats["refactorisations"] = n_refac
        stats["reformed_unequal"] = n_unequal
    if status:
        return np.full(nv, np.nan), status
    return np.where(basic, x, np.where(at_hi, hi, lo)), 0


def g1_problem(q, frame_targets, posture_target):
    """(Dg, c_d, Jw, r, lo, hi, dt) of one G1 config-3 instance, from the numpy oracle's own task and limit code."""
    import oracle_configs as oc
    from oracle import ik
    m, tasks, limits, dt, damping = oc.g1_c3(frame_targets, posture_target)
    cfg = ik.Configuration(m, q)
    nv = m.nv
    Dg = np.full(nv, damping)
    c_d = np.zeros(nv)
    rows, rhs = [], []
    for t in tasks:
        e, J = ik.task_error_jacobian(cfg, t)
        W = np.asarray(t.cost, float)
        we = W * (-t.gain * e)
        Dg += t.lm_damping * (we @ we)
        Jw = W[:, None] * J
        if isinstance(t, ik.PostureTaskSpec):
            Dg += np.diag(Jw.T @ Jw)
            c_d += -we @ Jw
        else:
            keep = W != 0
            rows.append(Jw[keep])
            rhs.append(we[keep])
    lo, hi = np.full(nv, -np.inf), np.full(nv, np.inf)
    for lim in limits:
        G, h = ik.limit_inequalities(cfg, lim, dt)
        if G is None:
            continue
        for g, hh in zip(G, h):                          # single-entry rows: ±e_k·x ≤ h
            k = int(np.nonzero(g)[0][0])
            if g[k] > 0:
                hi[k] = min(hi[k], hh / g[k])
            else:
                lo[k] = max(lo[k], hh / g[k])
    return Dg, c_d, np.vstack(rows), np.hstack(rhs), lo, hi, dt


def g1_batch(n, seed, sigma=0.15):
    """Benchmark-like G1 config-3 instances on the host: q as mink_amd.workloads.sample_q draws it around `stand`, frame targets =
    the frames at q ⊕ δ, δ ~ N(0, σ²) per dof (workloads.make_batch's distribution, with the numpy oracle's kinematics)."""
    import oracle_configs as oc
    from oracle import ik
    from mink_amd import workloads
    m = oc.model("g1")
    stand = np.asarray(m.key_qpos[m.name2id("key", "stand")], float)
    rng = np.random.default_rng(seed)
    q = workloads.sample_q(m, rng, n, stand)
    delta = rng.normal(scale=sigma, size=(n, m.nv))
    sites = [m.name2id("site", s) for s in ("left_foot", "right_foot", "left_palm", "right_palm")]
    tg = np.empty((n, 4, 7))
    cfg = ik.Configuration(m, q[0])
    for i in range(n):
        cfg.update(q[i])
        cfg.update(cfg.integrate(delta[i], 1.0))
        for k, s in enumerate(sites):
            tg[i, k] = cfg.get_transform_frame_to_world(s, "site")
    return q, tg, stand


def g1_problems(q, tg, stand):
    return [g1_problem(q[i], tg[i], stand) for i in range(len(q))]


def replay(problems, P=P_DEFAULT, cold_refine=True, one_double=False, unequal=None):
    """v, status, pivots, refactorisations per instance.  unequal: a list that receives, per instance, the count of re-formed
    multiplier entries that differ from the stored ones (one_double)."""
    n = len(problems)
    v = np.empty((n, len(problems[0][0])))
    st = np.zeros(n, int)
    piv = np.zeros(n, int)
    ref = np.zeros(n, int)
    for i, (Dg, c_d, Jw, r, lo, hi, dt) in enumerate(problems):
        s = {}
        x, st[i] = solve(Dg, c_d, Jw, r, lo, hi, P=P, cold_refine=cold_refine, stats=s, one_double=one_double)
        if unequal is not None:
            unequal.append(s["reformed_unequal"])
        v[i] = x / dt
        piv[i], ref[i] = s["pivots"], s["refactorisations"]
    return v, st, piv, ref


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    P = int(sys.argv[3]) if len(sys.argv) > 3 else P_DEFAULT
    problems = g1_problems(*g1_batch(n, seed))
    for cold in (True, False):
        v, st, piv, ref = replay(problems, P=P, cold_refine=cold)
        print("cold-start refinement %s: %d instances, status != 0: %d, pivots per solve mean %.2f max %d" % (
            "on" if cold else "off", n, int((st != 0).sum()), piv.mean(), piv.max()))
        print("  histogram of pivots per solve:", np.bincount(piv).tolist())
        print("  solves that refactorise at P = %d: %d (%.2f %%)" % (P, int((ref > 0).sum()), 100.0 * (ref > 0).mean()))
        uneq = []
        v1, st1, piv1, ref1 = replay(problems, P=P, cold_refine=cold, one_double=True, unequal=uneq)
        print("  one-double slots: re-formed multiplier entries unequal to the stored ones: %d; v bitwise equal: %s; statuses equal: %s" % (
            sum(uneq), np.array_equal(v1, v), np.array_equal(st1, st)))


if __name__ == "__main__":
    main()
