#!/usr/bin/env python
"""Seed tables (mkh_seed_table_*): what the query in front of the seed kernel costs next to the multi-start call it feeds.

    python tools/bench_seed_table.py [workloads=ur5e:4096:16:16384,g1_c3:4096:4:16384] [reps=20] [--tree PATH ...]

Per workload (robot : B targets : S seeds per target : N table entries), device-resident inputs and outputs, HIP events around
every call, legs alternated over two passes so that none owns a quiet moment of a shared machine; printed per leg: the median
of 2·`reps` timings [max − min]:
  (a) table    NativeProblem.solve_multistart(seed_table=): query, seed kernel, target fan-out, the threshold loop, selection
  (b) random   the same call with seeds drawn by the stateless generator — the call as it is without a table
  (c) query    NativeSeedTable.query alone: indices, distances and the K = S − 1 rows of every target
and (a) − (b), (c) against (b)'s own spread, the keys a query reads (N·n_frame·56 bytes per pass, one pass per 16 targets),
and the converged targets of (a) and (b).
UR5e: the far-target set-up of examples/batched_global_ik_ur5e.py, table drawn around `home`; g1_c3: the bench workload
(targets 0.15 rad away), table drawn around `stand`, 20 iterations, thresholds 1e-3 / 1e-2.

--tree PATH (repeatable): run the workloads once per source tree, each in a child process that imports mink_amd from PATH —
a tree that has no seed tables (a build of an earlier commit) runs leg (b) only, so the same command measures this tree's
random-seed call against that tree's.
"""
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def workload(nat, workloads, name, B, S):
    from mink_amd.api_specs import configuration_limit_desc
    rng = np.random.default_rng(1)
    if name == "ur5e":
        m = workloads.load_robot("ur5e")
        nm = nat.NativeModel(m)
        prob = nat.NativeProblem(nm, frame_tasks=[workloads._frame_desc(m, "attachment_site", "site", 1.0, 1.0, 1.0)],
                                 configuration_limits=[configuration_limit_desc(m)], max_batch=B * S)
        lo, hi = np.maximum(m.jnt_range[:, 0], -np.pi), np.minimum(m.jnt_range[:, 1], np.pi)
        goal = rng.uniform(lo, hi, size=(B, m.nq))
        dummy = np.zeros((B, 1, 7)); dummy[:, :, 0] = 1.0
        _, _, t = prob.solve(goal, dummy, None, None, 1.0, 1.0, taps=["frame_pose"], solve_qp=False)
        home = np.array(m.key_qpos[m.name2id("key", "home")])
        return m, nm, prob, (np.tile(home, (B, 1)), t["frame_pose"], None, None), 1.0, 1e-3, 40, (1e-4, 1e-4), home
    m = workloads.load_bench_robot(name)
    nm = nat.NativeModel(m)
    prob, dt, damping = workloads.bench_config(name, m, nm, B * S)
    q, tg, pt, ct = workloads.bench_batch(name, m, nm, prob, rng, B)
    base = np.array(m.key_qpos[m.name2id("key", workloads.BENCH_CONFIGS[name]["key"])])
    return m, nm, prob, (q, tg, pt, ct), dt, damping, 20, (1e-3, 1e-2), base


def run(specs, reps):
    import torch

    from mink_amd import _native as nat
    from mink_amd import workloads

    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_seed_table needs a GPU")
    has_tables = hasattr(nat, "NativeSeedTable")
    dev = torch.device("cuda:0")
    tree = os.path.dirname(os.path.dirname(os.path.abspath(nat.__file__)))
    print(f"# tools/bench_seed_table.py on {tree}   (median of {2 * reps} [max - min], ms)"
          + ("" if has_tables else "   -- no seed tables in this tree: leg (b) only"))
    for spec in specs:
        name, B, S, N = spec.split(":")
        B, S, N = int(B), int(S), int(N)
        m, nm, prob, (q, tg, pt, ct), dt, damping, iters, thr, q0 = workload(nat, workloads, name, B, S)
        to = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)
        dq, dtg, dpt, dct = to(q), to(tg), to(pt), to(ct)
        kw = dict(n_seeds=S, max_iters=iters, pos_threshold=thr[0], ori_threshold=thr[1])
        legs = {"b": lambda: prob.solve_multistart(dq, dtg, dpt, dct, dt, damping, rng_seed=0, **kw)}
        if has_tables:
            tab = nat.NativeSeedTable(prob, N, q0, rng_seed=11)
            legs["a"] = lambda: prob.solve_multistart(dq, dtg, dpt, dct, dt, damping, seed_table=tab, **kw)
            legs["c"] = lambda: tab.query(dtg, S - 1)
        times = {k: [] for k in legs}
        for _ in range(2):                                 # two passes over the legs, alternating
            for k, fn in sorted(legs.items()):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                for _ in range(reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); fn(); b.record()
                    b.synchronize()
                    times[k].append(a.elapsed_time(b))
        med = {k: float(np.median(v)) for k, v in times.items()}
        spread = {k: float(np.max(v) - np.min(v)) for k, v in times.items()}
        conv = {k: int(legs[k]().converged.sum().item()) for k in legs if k != "c"}
        line = f"{name:6s} B={B} S={S} N={N} loop kernel {prob.last_kernel()}: (b) random {med['b']:8.3f} [{spread['b']:.3f}]"
        if has_tables:
            n_frame = tg.shape[1]
            passes = -(-B // 16)
            line += (f"  (a) table {med['a']:8.3f} [{spread['a']:.3f}]  (c) query {med['c']:8.3f} [{spread['c']:.3f}]  "
                     f"(a)-(b) {med['a'] - med['b']:+.3f}  (c) = {med['c'] / spread['b'] if spread['b'] else float('inf'):.2f} x (b)'s spread, "
                     f"{100.0 * med['c'] / med['b']:.1f} % of (b)   [keys {N * n_frame * 56 / 1e6:.2f} MB x {passes} workgroups = "
                     f"{N * n_frame * 56 * passes / 1e6:.0f} MB through L2; converged: table {conv['a']}, random {conv['b']} of {B}]")
            tab.close()
        else:
            line += f"   [converged: random {conv['b']} of {B}]"
        print(line, flush=True)
        prob.close(); nm.close()


def main():
    args = sys.argv[1:]
    trees = []
    while "--tree" in args:
        i = args.index("--tree")
        trees.append(os.path.abspath(args[i + 1]))
        del args[i:i + 2]
    child = "--child" in args
    if child:
        args.remove("--child")
    specs = (args[0] if args else "ur5e:4096:16:16384,g1_c3:4096:4:16384").split(",")
    reps = int(args[1]) if len(args) > 1 else 20
    if trees and not child:
        for tree in trees:                                 # one fresh process per tree: each imports its own package and library
            env = dict(os.environ, PYTHONPATH=tree)
            subprocess.run([sys.executable, os.path.abspath(__file__), ",".join(specs), str(reps), "--child"], env=env, check=True)
        return
    if not child:
        sys.path.insert(0, REPO)
    run(specs, reps)


if __name__ == "__main__":
    main()
