#!/usr/bin/env python
"""Goal sets (mkh_solve_goalset): what the seeds, the fan-out and the two-level selection cost on top of the loops they frame,
and what the one call saves over the host composition it replaces.

    python tools/bench_goalset.py [workloads=ur5e:256,ur5e:4096,g1_c3:256] [reps=20] [goals=8] [seeds=8]

Per workload (robot : B targets, G goals per target, S seeds per goal), median of `reps` after warm-up with the spread
(min … max) of the repetitions; the device legs are timed twice, interleaved, and both medians are printed:
  (i)   the call   NativeProblem.solve_goalset, device-resident inputs and outputs — HIP events around the call
  (ii)  bare loop  the threshold-terminated loop launch alone on the same B·G·S device-resident instances (the call's own seeds,
                   the targets repeated beforehand) — HIP events
  (iii) host       what a caller writes without the entry point: solve_multistart(return_all=True) on the B·G flattened pairs
                   with numpy in and out (B·G·S rows over the bus), then the two levels in numpy — vectorised over the targets,
                   squared differences of qpos (UR5e: the rule itself; G1: the base quaternion's components stand in for its
                   rotation vector — what a caller would write; the share of targets on which it makes the device's choice is
                   printed) — wall clock
The targets are those of tools/bench_multistart.py, G consecutive ones forming one target's goals.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def host_rule(q_all, ok, q0):
    """The two levels in numpy over (B, G, S, nq) candidates, no costs and no masks: (goal_index, seed_index, converged)."""
    B, G, S, _ = q_all.shape
    d = np.where(ok, ((q_all - q0[:, None, None, :]) ** 2).sum(axis=3), np.inf)
    seed_goal = d.argmin(axis=2)                                            # (ties: the lowest index)
    d_goal = np.take_along_axis(d, seed_goal[..., None], 2)[..., 0]
    goal = d_goal.argmin(axis=1)
    rows = np.arange(B)
    hit = np.isfinite(d_goal[rows, goal])
    return np.where(hit, goal, 0), np.where(hit, seed_goal[rows, goal], 0), hit


def spread(ts):
    return f"{np.median(ts):8.3f} ms ({np.min(ts):.3f} … {np.max(ts):.3f})"


def main():
    import torch

    from bench_multistart import workload
    from mink_amd import _native as nat
    from mink_amd import workloads

    specs = (sys.argv[1] if len(sys.argv) > 1 else "ur5e:256,ur5e:4096,g1_c3:256").split(",")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    G = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    S = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_goalset needs a GPU")
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

    print(f"# tools/bench_goalset.py {' '.join(sys.argv[1:])}   (median of {reps} (min … max), G = {G}, S = {S})")
    for spec in specs:
        name, B = spec.split(":")
        B = int(B)
        R, N = B * G, B * G * S
        m, nm, prob, (qq, tg, pt, ct), dt, damping, iters, thr = workload(nat, workloads, name, N, S)      # R rows of targets
        q = np.ascontiguousarray(qq[::G])
        per_goal = lambda x: None if x is None else (x.reshape(B, G, *x.shape[1:]) if x.ndim == 3 and x.shape[0] == R else x)
        goals, gpt, gct = tg.reshape(B, G, *tg.shape[1:]), per_goal(pt), per_goal(ct)
        flat = lambda x: None if x is None else (x.reshape(R, *x.shape[2:]) if x.ndim == 4 else x)
        rep = lambda x: None if x is None else (np.repeat(flat(x), S, axis=0) if x.ndim == 4 else x)
        dq, dgoals, dpt, dct = to(q), to(goals), to(gpt), to(gct)
        kw = dict(n_seeds=S, max_iters=iters, pos_threshold=thr[0], ori_threshold=thr[1], rng_seed=0)
        first = prob.solve_goalset(dq, dgoals, dpt, dct, dt, damping, return_all=True, **kw)
        seeds = first.seeds.reshape(N, m.nq).contiguous()
        rtg, rpt, rct = to(rep(goals)), to(rep(gpt)), to(rep(gct))
        the_call = lambda: prob.solve_goalset(dq, dgoals, dpt, dct, dt, damping, **kw)
        bare_loop = lambda: prob.solve(seeds, rtg, rpt, rct, dt, damping, n_steps=iters, until=thr)
        # alternate the two device legs so that neither owns a quiet moment of a shared machine
        t_i = events(the_call)
        k_loop = prob.last_kernel()
        t_ii, t_i2, t_ii2 = events(bare_loop), events(the_call), events(bare_loop)
        q_rep = np.repeat(q, G, axis=0)

        def host():
            out = prob.solve_multistart(q_rep, flat(goals), flat(gpt), flat(gct), dt, damping, return_all=True, **kw)
            ok = (out.converged_all != 0) & ((out.status_all & ~1) == 0)
            return host_rule(out.q_all.reshape(B, G, S, m.nq), ok.reshape(B, G, S), q)

        host(); host()
        th = []
        for _ in range(max(5, reps // 4)):
            t0 = time.perf_counter(); host(); th.append(1e3 * (time.perf_counter() - t0))
        th = np.array(th)
        res = the_call()
        hg, hs, hc = host()
        gi, si, cv = res.goal_index.cpu().numpy(), res.seed_index.cpu().numpy(), res.converged.cpu().numpy() != 0
        agree = float(((hg == gi) & (hs == si) & (hc == cv)).mean())
        one = int((first.reached[:, 0] != 0).sum().item())
        mi, mii = 0.5 * (np.median(t_i) + np.median(t_i2)), 0.5 * (np.median(t_ii) + np.median(t_ii2))
        print(f"{name:8s} B={B:6d} (G={G}, S={S}: {N} loops) loop kernel {k_loop}:\n"
              f"    (i)   the call         {spread(t_i)}   again {spread(t_i2)}\n"
              f"    (ii)  bare loop        {spread(t_ii)}   again {spread(t_ii2)}\n"
              f"    (i)-(ii) {mi - mii:+7.3f} ms = {100.0 * (mi - mii) / mii:+5.1f} % of (ii)\n"
              f"    (iii) host composition {spread(th)} = {np.median(th) / mi:5.1f} x (i)\n"
              f"    [{1e-3 * B / (1e-3 * mi):.1f} k targets/s; targets reached {int(cv.sum())} of {B}, by goal 0 alone {one}; goal_index "
              f"histogram {np.bincount(gi[cv], minlength=G).tolist()}; host rule makes the same choice on {100 * agree:.1f} % of the targets]",
              flush=True)
        prob.close(); nm.close()


if __name__ == "__main__":
    main()
