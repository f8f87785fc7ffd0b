#!/usr/bin/env python
"""Checked candidate tracking (mkh_solve_trajectory_multistart_free, mkh_select_trajectory_candidates): what the check costs.

    python tools/bench_trajectory_free.py [rounds=5] [parts=abc] [T=64] [shapes=all] > profiles/r24_trajectory_free.txt

`shapes`: "all", or a comma-separated choice of ur5e:256, ur5e:4096, g1_c3:256, g1_c3:4096 (the profile is four runs' lines).

Wall clock around each leg with a device synchronisation at its end; the legs of a part ALTERNATE, `rounds` times after a
warm-up round; reported: the median and the (max - min) of each leg's rounds (tools/bench_swept.py's method and workloads).
S = 16 candidates per instance, M = 8 samples per motion; UR5e and G1 (g1_c3, 46 pairs) at 256 and 4 096 instances.
  (a) the checked call against the unchecked one at the same shape on the same build, device tensors in and out: the cost of
      the check, per call and per row of the T·B·S·(1 + M) the check can evaluate at the most.
  (b) the check alone on the device-resident q_all of (a), two ways behind the same rule:
        (k) tmf_check_kernel — timed as mkh_select_trajectory_candidates with the checker minus the same call without one
            (the score and the gather of q are in both; the two margin gathers and the edge flags stay in the difference)
        (2) the two launches that existed: mkh_clearance on the T·B·S rows, mkh_swept_clearance on the (T - 1)·B·S edges
            from = q_all[:-1], to = q_all[1:], and the masking of the edges into rows that are not eligible (torch.where)
      Their margins must agree: asserted, NaN and +inf placement included.
  (c) the checked call against the host composition it replaces, numpy in and out on both sides, UR5e at 256 instances:
      solve_trajectory_multistart with return_all, checker.clearance and checker.swept_clearance with host arrays, and the
      selection vectorised in numpy.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

ST_IN_COLLISION = 64


def numpy_selection(q, q_all, converged_all, status_all, node_margin, edge_margin, S):
    """THE RULE "with a checker" on host arrays of a model with hinge and slide joints only (the UR5e): (seed_index, n_tracked)."""
    T, R, nq = q_all.shape
    B = R // S
    status = status_all | np.where(~(node_margin >= 0.0), ST_IN_COLLISION, 0).astype(status_all.dtype)
    eligible = (converged_all != 0) & ((status & ~1) == 0)
    free_edge = np.ones((T, R), dtype=bool)
    free_edge[1:] = np.nan_to_num(edge_margin, nan=-1.0) >= 0.0
    counts = (eligible & free_edge).sum(axis=0).reshape(B, S)
    prev = np.concatenate([np.repeat(q, S, axis=0)[None], q_all[:-1]])
    length = ((q_all - prev) ** 2).sum(axis=2).sum(axis=0).reshape(B, S)
    key = np.where(np.isfinite(length), length, np.inf)
    order = np.lexsort((np.tile(np.arange(S), (B, 1)), key, -counts), axis=1)[:, 0]
    seed = np.where(counts.max(axis=1) > 0, order, 0)
    return seed, counts[np.arange(B), seed]


def main():
    import torch

    import mink_amd as mink
    from bench_clearance import checker
    from bench_swept import M, S, cell, ladder_workload
    from mink_amd import _native as nat
    from mink_amd import workloads

    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    parts = sys.argv[2] if len(sys.argv) > 2 else "abc"
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    only = sys.argv[4].split(",") if len(sys.argv) > 4 and sys.argv[4] != "all" else None
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_trajectory_free needs a GPU")
    dev = torch.device("cuda:0")
    to = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def alternate(legs, n=rounds):
        for fn in legs.values():
            wall(fn)
        ts = {k: [] for k in legs}
        for _ in range(n):
            for k, fn in legs.items():
                ts[k].append(wall(fn)[0])
        return {k: np.array(v) for k, v in ts.items()}

    print(f"# tools/bench_trajectory_free.py {' '.join(sys.argv[1:])}   ({rounds} alternating rounds; median [max - min]; "
          f"S = {S} candidates, M = {M} samples per motion, T = {T})")
    for name, ck_name, B in (("ur5e", "ur5e", 256), ("ur5e", "ur5e", 4096), ("g1_c3", "g1", 256), ("g1_c3", "g1", 4096)):
        if only is not None and f"{name}:{B}" not in only:
            continue
        m, nm, prob, q, tg, pt, dt, damping, iters, thr = ladder_workload(nat, workloads, name, B, T)
        _, ck = checker(mink, workloads, ck_name, model=m, max_rows=1 << 20)
        native = ck._native_for(prob)
        kw = dict(n_seeds=S, n_steps=iters, pos_threshold=thr[0], ori_threshold=thr[1], rng_seed=3)
        dq, dtg, dpt = to(q), to(tg), to(pt)
        rows_max = T * B * S * (1 + M)
        plain = lambda: prob.solve_trajectory_multistart(dq, dtg, dpt, None, dt, damping, return_all=True, **kw)
        free = lambda: prob.solve_trajectory_multistart_free(dq, dtg, dpt, None, dt, damping, checker=native, edge_samples=M,
                                                             return_all=True, **kw)
        rp, (rf, mf) = plain(), free()
        for f in ("q_all", "v_all", "iters_all", "converged_all"):
            assert torch.equal(getattr(rp, f), getattr(rf, f)), f
        eligible = (rf.converged_all != 0) & ((rf.status_all & ~1) == 0)
        n_rows = T * B * S + M * int(eligible[1:].sum().item())          # rows the check DID evaluate
        if "a" in parts:
            ts = alternate({"p": plain, "f": free})
            mp, mc = np.median(ts["p"]), np.median(ts["f"])
            print(f"(a) {name:6s} B={B:5d} T={T} ({ck.n_pairs} pairs, loop kernel {prob.last_kernel()}): unchecked {cell(ts['p'])}   checked "
                  f"{cell(ts['f'])}   added {mc - mp:+9.3f} ms = {100.0 * (mc - mp) / mp:+6.1f} % = {1e6 * (mc - mp) / rows_max:7.3f} ns per row "
                  f"of T*B*S*(1+M) = {rows_max}, {1e6 * (mc - mp) / n_rows:7.3f} ns per row of the {n_rows} evaluated   [complete candidates "
                  f"{int(rp.n_complete.sum().item())} -> {int(rf.n_complete.sum().item())} of {B * S}; instances with one "
                  f"{int((rp.n_tracked == T).sum().item())} -> {int((rf.n_tracked == T).sum().item())} of {B}; rows in collision "
                  f"{int(((rf.status_all & ST_IN_COLLISION) != 0).sum().item())} of {T * B * S}]", flush=True)
        if "b" in parts:
            q_all, cv_all = rp.q_all, rp.converged_all
            trk = ((cv_all != 0) & ((rp.status_all & ~1) == 0)).to(torch.int32)          # the loops' verdict as the caller's flags
            nq = q_all.shape[2]
            with_ck = lambda: prob.select_trajectory_candidates(dq, q_all, trk, None, native, M, True)
            without = lambda: prob.select_trajectory_candidates(dq, q_all, trk)

            def two_launches():
                node = native.clearance(q_all.reshape(-1, nq)).margin.reshape(T, B * S)
                edge = torch.full((T, B * S), float("inf"), dtype=torch.float64, device=dev)
                if T > 1:
                    sw = native.swept_clearance(q_all[:-1].reshape(-1, nq), q_all[1:].reshape(-1, nq), M).margin.reshape(T - 1, B * S)
                    ok = (trk[1:] != 0) & (node[1:] >= 0.0)
                    edge[1:] = torch.where(ok, sw, torch.full_like(sw, float("nan")))
                return node, edge

            ts = alternate({"k": with_ck, "s": without, "2": two_launches})
            (_, more), (node2, edge2) = with_ck(), two_launches()
            assert torch.equal(torch.isnan(more.edge_margin_all), torch.isnan(edge2)) and torch.equal(torch.isinf(more.edge_margin_all), torch.isinf(edge2))
            fin = torch.isfinite(edge2)
            assert float((more.edge_margin_all[fin] - edge2[fin]).abs().max().item()) <= 1e-9
            assert float((more.node_margin_all - node2).abs().max().item()) <= 1e-9
            mk, ms, m2 = (np.median(ts[k]) for k in "ks2")
            swept = int(fin[1:].sum().item())
            print(f"(b) {name:6s} B={B:5d} T={T}: selection with the checker {cell(ts['k'])}, without {cell(ts['s'])}: the one launch "
                  f"{mk - ms:9.3f} ms = {1e6 * (mk - ms) / (T * B * S + M * swept):7.3f} ns per evaluated row   the two launches "
                  f"{cell(ts['2'])} = {m2 / (mk - ms):5.2f} x   [{swept} of {(T - 1) * B * S} edges swept by the one launch, all of them by "
                  f"the two]", flush=True)
        if "c" in parts and name == "ur5e" and B <= 256:
            def fused():
                return prob.solve_trajectory_multistart_free(q, tg, pt, None, dt, damping, checker=native, edge_samples=M, **kw)

            def host():
                out = prob.solve_trajectory_multistart(q, tg, pt, None, dt, damping, return_all=True, **kw)
                nqh = out.q_all.shape[2]
                node = ck.clearance(out.q_all.reshape(-1, nqh)).margin.reshape(T, B * S)
                edge = ck.swept_clearance(out.q_all[:-1].reshape(-1, nqh), out.q_all[1:].reshape(-1, nqh), n_samples=M).margin
                return numpy_selection(q, out.q_all, out.converged_all, out.status_all, node, edge.reshape(T - 1, B * S), S)

            ts = alternate({"c": fused, "h": host}, n=max(3, rounds // 2))
            (rc, _), (seed_h, n_h) = fused(), host()
            assert (rc.n_tracked == n_h).all()         # (the lengths are summed in another order on the host: a near-tie may fall the other way)
            print(f"(c) {name:6s} B={B:5d} T={T} S={S}, numpy in and out: the fused call {cell(ts['c'])}; host composition {cell(ts['h'])} = "
                  f"{np.median(ts['h']) / np.median(ts['c']):6.2f} x   [the same counts on both sides: asserted; the same candidate at "
                  f"{int((rc.seed_index == seed_h).sum())} of {B} instances]", flush=True)
        ck.close(); prob.close(); nm.close()


if __name__ == "__main__":
    main()
