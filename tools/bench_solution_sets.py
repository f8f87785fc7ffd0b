#!/usr/bin/env python
"""Distinct solution sets (mkh_solve_multistart_set): what the selection costs on top of multi-start's, what the one call saves
over the host composition it replaces, and what the ladder search gains from deduplicated rungs.

    python tools/bench_solution_sets.py [workloads=ur5e:65536,ur5e:1048576,g1_c3:65536] [reps=20] [seeds=16] [solutions=8]

Per workload (robot : B·S instances, S seeds per target, K slots, min_distance 0.1), median of `reps` after warm-up with the
spread (min … max) of the repetitions; the device legs are timed twice, interleaved, and both medians are printed:
  (i)   the set    NativeProblem.solve_multistart_set, device-resident inputs and outputs — HIP events around the call
  (ii)  one result NativeProblem.solve_multistart on the same B, S — the same seeds, fan-out and loops, multi-start's selection
  (iii) host       what a caller writes without the entry point: solve_multistart(return_all=True) with numpy in and out (B·S
                   rows over the bus), then the rule in numpy — vectorised over the targets, squared differences of qpos (UR5e:
                   the rule itself; G1: the base quaternion's components stand in for its rotation vector — what a caller would
                   write; the share of targets on which it picks the device's seeds is printed) — wall clock
  (iv)  ladder     UR5e only: NativeProblem.ladder_select on (P, T, K) deduplicated rungs against (P, T, S) raw ones, 256 lines
                   of 16 waypoints solved as P·T targets, device-resident — HIP events
The workloads are those of tools/bench_multistart.py.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def host_rule(q_all, ok, q0, K, r):
    """The rule in numpy over (B, S, nq) candidates of hinge / slide joints: K rounds, each vectorised over the targets."""
    B, S, _ = q_all.shape
    d_ref = np.where(ok, ((q_all - q0[:, None, :]) ** 2).sum(axis=2), np.inf)
    left = ok.copy()
    seed_index, mult = np.full((B, K), -1, dtype=np.int32), np.zeros((B, K), dtype=np.int32)
    rows = np.arange(B)
    for j in range(K):
        d = np.where(left, d_ref, np.inf)
        rep = d.argmin(axis=1)                                             # (ties: the lowest index)
        live = left[rows, rep]
        if not live.any():
            break
        near = ((q_all - q_all[rows, rep][:, None, :]) ** 2).sum(axis=2) <= r * r
        cover = left & near & live[:, None]
        seed_index[live, j] = rep[live]
        mult[:, j] = cover.sum(axis=1)
        left &= ~cover
    return seed_index, mult, left.sum(axis=1)


def spread(ts):
    return f"{np.median(ts):8.3f} ms ({np.min(ts):.3f} … {np.max(ts):.3f})"


def main():
    import torch

    from bench_multistart import workload
    from mink_amd import _native as nat
    from mink_amd import workloads

    specs = (sys.argv[1] if len(sys.argv) > 1 else "ur5e:65536,ur5e:1048576,g1_c3:65536").split(",")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    S = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    K = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    r = 0.1
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_solution_sets needs a GPU")
    dev = torch.device("cuda:0")
    to = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)

    def events(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return np.array(ts)

    print(f"# tools/bench_solution_sets.py {' '.join(sys.argv[1:])}   (median of {reps} (min … max), S = {S}, K = {K}, min_distance = {r})")
    for spec in specs:
        name, N = spec.split(":")
        N = int(N)
        B = N // S
        m, nm, prob, (q, tg, pt, ct), dt, damping, iters, thr = workload(nat, workloads, name, N, S)
        dq, dtg, dpt, dct = to(q), to(tg), to(pt), to(ct)
        kw = dict(n_seeds=S, max_iters=iters, pos_threshold=thr[0], ori_threshold=thr[1], rng_seed=0)
        the_set = lambda: prob.solve_multistart_set(dq, dtg, dpt, dct, dt, damping, n_solutions=K, min_distance=r, **kw)
        one_result = lambda: prob.solve_multistart(dq, dtg, dpt, dct, dt, damping, **kw)
        # alternate the two device legs so that neither owns a quiet moment of a shared machine
        t_i, t_ii, t_i2, t_ii2 = events(the_set), events(one_result), events(the_set), events(one_result)
        k_loop = prob.last_kernel()

        def host():
            out = prob.solve_multistart(q, tg, pt, ct, dt, damping, return_all=True, **kw)
            ok = (out.converged_all != 0) & ((out.status_all & ~1) == 0)
            return host_rule(out.q_all, ok, q, K, r)

        host(); host()
        th = []
        for _ in range(max(5, reps // 4)):
            t0 = time.perf_counter(); host(); th.append(1e3 * (time.perf_counter() - t0))
        th = np.array(th)
        res = the_set()
        nd = res.n_distinct.cpu().numpy()
        hs, hm, hu = host()
        agree = float((hs == res.seed_index.cpu().numpy()).all(axis=1).mean())
        mi, mii = 0.5 * (np.median(t_i) + np.median(t_i2)), 0.5 * (np.median(t_ii) + np.median(t_ii2))
        print(f"{name:8s} B*S={N:8d} (B={B}, S={S}, K={K}) loop kernel {k_loop}:\n"
              f"    (i)   the set          {spread(t_i)}   again {spread(t_i2)}\n"
              f"    (ii)  one result       {spread(t_ii)}   again {spread(t_ii2)}\n"
              f"    (i)-(ii) {mi - mii:+7.3f} ms = {100.0 * (mi - mii) / mii:+5.1f} % of (ii)\n"
              f"    (iii) host composition {spread(th)} = {np.median(th) / mi:5.1f} x (i)\n"
              f"    [{1e-6 * B / (1e-3 * mi):.2f} M targets/s; distinct solutions per target 0 … {K}: {np.bincount(nd, minlength=K + 1).tolist()}; "
              f"targets with uncovered seeds {int((res.n_uncovered > 0).sum().item())}; host rule picks the same seeds on {100 * agree:.1f} % of the targets]",
              flush=True)
        prob.close(); nm.close()

    # ---- (iv) the ladder search on deduplicated rungs
    P, T = 256, 16
    m, nm, prob, (q, tg, _, _), dt, damping, iters, thr = workload(nat, workloads, "ur5e", P * T * S, S)
    dq, dtg = to(q), to(tg)
    rungs = prob.solve_multistart_set(dq, dtg, None, None, dt, damping, n_seeds=S, n_solutions=K, min_distance=r, max_iters=iters,
                                      pos_threshold=thr[0], ori_threshold=thr[1], rng_seed=0, return_all=True)
    q0 = dq[:P].contiguous()
    few_nodes = rungs.q.reshape(P, T, K, m.nq).contiguous()
    few_trk = (rungs.seed_index >= 0).to(torch.int32).reshape(P, T, K).contiguous()
    all_nodes = rungs.q_all.reshape(P, T, S, m.nq).contiguous()
    all_trk = ((rungs.converged_all != 0) & ((rungs.status_all & ~1) == 0)).to(torch.int32).reshape(P, T, S).contiguous()
    few = lambda: prob.ladder_select(q0, few_nodes, few_trk)
    full = lambda: prob.ladder_select(q0, all_nodes, all_trk)
    t_f, t_a, t_f2, t_a2 = events(few), events(full), events(few), events(full)
    same = bool((few().n_tracked == full().n_tracked).all().item())
    print(f"ur5e     ladder search, {P} instances of {T} rungs (independent far targets as rungs):\n"
          f"    (iv)  K = {K:3d} nodes per rung {spread(t_f)}   again {spread(t_f2)}\n"
          f"          S = {S:3d} nodes per rung {spread(t_a)}   again {spread(t_a2)}\n"
          f"    = {0.5 * (np.median(t_a) + np.median(t_a2)) / (0.5 * (np.median(t_f) + np.median(t_f2))):.2f} x   [the same n_tracked: {same}]", flush=True)
    prob.close(); nm.close()


if __name__ == "__main__":
    main()
