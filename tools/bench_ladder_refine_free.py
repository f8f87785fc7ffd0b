#!/usr/bin/env python
"""The refinement pass with a checker (mkh_ladder_refine_free, mkh_solve_trajectory_ladder_free_refined): what the check costs.

    python tools/bench_ladder_refine_free.py [rounds=7] [parts=ab] [T=64] > profiles/r23_refine_free.txt

Wall clock around each leg with a device synchronisation at its end; the legs of a part ALTERNATE, `rounds` times after a
warm-up round; reported: the median and the (max - min) of each leg's rounds (tools/bench_swept.py's method and workloads).
  (a) the checked pass against the plain one on the same device-resident paths — the chosen paths of the checked ladder on K = 8
      distinct nodes of S = 16 solutions per waypoint, M = 8 samples per motion: (p) mkh_ladder_refine, (f) mkh_ladder_refine_free.
      UR5e at 256 and 4 096 instances, G1 (g1_c3, 46 pairs) at 256.  Reported per call and per waypoint step (2T - 1 steps).
  (b) the fused checked-and-refined call against the host composition it replaces, numpy in and out on both sides, UR5e at 256
      instances: the checked ladder, refine_path's pass WITHOUT a checker, then checker.clearance and checker.swept_clearance
      with host arrays on what came back.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import torch

    import mink_amd as mink
    from bench_clearance import checker
    from bench_swept import K, M, S, cell, ladder_workload
    from mink_amd import _native as nat
    from mink_amd import workloads

    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    parts = sys.argv[2] if len(sys.argv) > 2 else "ab"
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_ladder_refine_free needs a GPU")
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

    print(f"# tools/bench_ladder_refine_free.py {' '.join(sys.argv[1:])}   ({rounds} alternating rounds; median [max - min]; "
          f"M = {M} samples per motion, T = {T})")
    for name, ck_name, B in (("ur5e", "ur5e", 256), ("ur5e", "ur5e", 4096), ("g1_c3", "g1", 256)):
        m, nm, prob, q, tg, pt, dt, damping, iters, thr = ladder_workload(nat, workloads, name, B, T)
        _, ck = checker(mink, workloads, ck_name, model=m, max_rows=1 << 20)
        native = ck._native_for(prob)
        kw = dict(n_seeds=S, n_nodes=K, max_iters=iters, pos_threshold=thr[0], ori_threshold=thr[1], rng_seed=3)
        rkw = dict(max_iters=iters, pos_threshold=thr[0], ori_threshold=thr[1])
        dq, dtg, dpt = to(q), to(tg), to(pt)
        if "a" in parts:
            lad, _ = prob.solve_trajectory_ladder_free(dq, dtg, dpt, None, dt, damping, checker=native, edge_samples=M, **kw)
            trk = ((lad.converged != 0) & ((lad.status & ~1) == 0)).to(torch.int32)
            plain = lambda: prob.ladder_refine(dq, lad.q, trk, dtg, dpt, None, dt, damping, **rkw)
            free = lambda: prob.ladder_refine_free(dq, lad.q, native, trk, dtg, dpt, None, dt, damping, edge_samples=M, **rkw)
            ts = alternate({"p": plain, "f": free})
            rp, rf = plain(), free()
            mp, mf = np.median(ts["p"]), np.median(ts["f"])
            steps = 2 * T - 1
            print(f"(a) {name:6s} B={B:5d} T={T} ({ck.n_pairs} pairs, loop kernel {prob.last_kernel()}): plain pass {cell(ts['p'])} = "
                  f"{1e3 * mp / steps:8.2f} us/step   checked pass {cell(ts['f'])} = {1e3 * mf / steps:8.2f} us/step   added "
                  f"{mf - mp:+9.3f} ms = {1e3 * (mf - mp) / steps:+8.2f} us/step = {100.0 * (mf - mp) / mp:+7.1f} %   [free tracked waypoints "
                  f"in {int(lad.n_tracked.sum().item())}, plain pass (by its own key) {int(rp.n_tracked.sum().item())}, checked pass "
                  f"{int(rf.n_tracked.sum().item())} of {B * T}; repairs {int((rp.repaired != 0).sum().item())} / "
                  f"{int((rf.repaired != 0).sum().item())}; edge collisions left {int(rf.n_edge_collisions.sum().item())}]", flush=True)
        if "b" in parts and name == "ur5e" and B <= 256:
            def fused():
                return prob.solve_trajectory_ladder_free(q, tg, pt, None, dt, damping, checker=native, edge_samples=M, refine=True, **kw)

            def host():
                out, _ = prob.solve_trajectory_ladder_free(q, tg, pt, None, dt, damping, checker=native, edge_samples=M, **kw)
                trk_h = (out.converged != 0) & ((out.status & ~1) == 0)
                r = prob.ladder_refine(q, out.q, trk_h, tg, pt, None, dt, damping, v=out.v, status=out.status, iters=out.iters,
                                       converged=out.converged, **rkw)
                nodes_free = ~ck.clearance(r.q).in_collision
                moves_free = ~ck.swept_clearance(r.q[:, :-1], r.q[:, 1:], n_samples=M).in_collision
                ok = (r.tracked != 0) & nodes_free
                ok[:, 1:] &= moves_free
                return ok.sum(axis=1)

            ts = alternate({"c": fused, "h": host}, n=max(3, rounds // 2))
            (rc, _), hn = fused(), host()
            print(f"(b) {name:6s} B={B:5d} T={T} S={S} K={K}, numpy in and out: the fused call {cell(ts['c'])}; host composition "
                  f"{cell(ts['h'])} = {np.median(ts['h']) / np.median(ts['c']):6.2f} x   [free tracked waypoints: fused "
                  f"{int(rc.n_tracked.sum())}, host composition (unchecked repairs, judged afterwards) {int(hn.sum())} of {B * T}]",
                  flush=True)
        ck.close(); prob.close(); nm.close()


if __name__ == "__main__":
    main()
