#!/usr/bin/env python
"""The certifying ladder search (mkh_ladder_select_certified) against the sampled one (mkh_ladder_select_free at 8 samples per
edge) on the same device-resident graph.

    python tools/bench_certified_ladder.py [rounds=5] [robot ...] > profiles/r30_certified_ladder.txt
    python tools/bench_certified_ladder.py once ur5e 256          # one call of each kind, for a kernel trace around it

Graph: UR5e (14 pairs, four edges per wavefront) and G1 (46 pairs, one per wavefront), T = 64 waypoints, 8 nodes per rung, 256 and
4 096 instances; every node is its instance's base posture with its hinge and slide joints moved by N(0, 0.05) (a free joint stays,
so the motion is the scalars'), all nodes flagged tracked; resolution 0.02 m, max_samples 64.  Wall clock around each call with a
device synchronisation at its end; the legs ALTERNATE, `rounds` times after a warm-up round; reported: the median and the
(max - min) of each leg's rounds.
  (s)  ladder_select_free, edge_samples = 8: the parent commit's call, unchanged — the baseline.  8 rows per swept edge.
  (c)  ladder_select_certified, colliding edges blocked; (r) the same with require_certified.
       sum(n_samples + 2) rows over the swept edges; the counts come from certified_sweep on the same edges, outside the clock.
The whole call is the node clearance (B T S rows), the launch over all edges, the search, and the launch over the B T chosen edges:
the launch over all edges is S = 8 times the rest in rows, so ns per row of the whole call bounds the launch's from above.  The
launches alone are a kernel trace's to report: the `once` form runs each call once behind a warm-up for that."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

RESOLUTION, MAX_SAMPLES, M_FIXED, T, S, SIGMA = 0.02, 64, 8, 64, 8, 0.05


def cell(ts):
    return f"{np.median(ts):9.3f} [{np.max(ts) - np.min(ts):7.3f}] ms"


def graph(model, workloads, name, B, rng):
    """(q (B, nq), q_nodes (B, T, S, nq)) on the host."""
    key = {"g1": "stand"}.get(name)
    base = workloads.sample_q(model, rng, B, base_q=None if key is None else model.key_qpos[model.name2id("key", key)])
    nodes = np.repeat(base[:, None, None, :], T, axis=1).repeat(S, axis=2)
    for j in range(model.njnt):
        if int(model.jnt_type[j]) in (2, 3):                       # slide, hinge
            qa = int(model.jnt_qposadr[j])
            nodes[..., qa] += rng.normal(scale=SIGMA, size=(B, T, S))
            if model.jnt_limited[j]:
                lo, hi = np.asarray(model.jnt_range).reshape(-1, 2)[j]
                nodes[..., qa] = np.clip(nodes[..., qa], lo, hi)
    return base, np.ascontiguousarray(nodes)


def main():
    import importlib

    import torch

    import mink_amd as mink
    from bench_clearance import checker
    from mink_amd import _native as nat
    from mink_amd import workloads
    from mink_amd.tasks import PostureTask
    sik = importlib.import_module("mink_amd.solve_ik")

    argv = sys.argv[1:]
    once = bool(argv) and argv[0] == "once"
    if once:
        robots, sizes, rounds = [argv[1]], [int(argv[2])], 1
    else:
        rounds = int(argv[0]) if argv else 5
        robots, sizes = (argv[1:] or ["ur5e", "g1"]), [256, 4096]
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_certified_ladder needs a GPU")
    dev = torch.device("cuda:0")
    to = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    print(f"# tools/bench_certified_ladder.py {' '.join(argv)}   ({rounds} alternating rounds; median [max - min]; T {T}, {S} nodes per rung, "
          f"resolution {RESOLUTION} m, max_samples {MAX_SAMPLES}, sampled rule at {M_FIXED} samples)")
    for name in robots:
        for B in sizes:
            model, ck = checker(mink, workloads, name, max_rows=1 << 16)
            q, nodes = graph(model, workloads, name, B, np.random.default_rng(3))
            cfg = mink.Configuration(model, q.copy())
            prob, layout = sik._compile(cfg, [PostureTask(model, cost=1.0)], None, 1, devices=cfg.devices[:1])
            dq, dn = to(q), to(nodes)
            with sik._pin(cfg, layout):
                legs = {"s": lambda: prob.ladder_select_free(dq, dn, ck, edge_samples=M_FIXED, return_margins=True),
                        "c": lambda: prob.ladder_select_certified(dq, dn, ck, resolution=RESOLUTION, max_samples=MAX_SAMPLES,
                                                                  return_margins=True),
                        "r": lambda: prob.ladder_select_certified(dq, dn, ck, resolution=RESOLUTION, max_samples=MAX_SAMPLES,
                                                                  require_certified=True, return_margins=True)}
                for fn in legs.values():
                    wall(fn)
                ts = {k: [] for k in legs}
                for _ in range(rounds):
                    for k, fn in legs.items():
                        ts[k].append(wall(fn)[0])
                out = {k: fn() for k, fn in legs.items()}
                torch.cuda.synchronize()
            # ---- the rows each rule evaluated: the swept edges are the same (the gating is), the counts are certified_sweep's
            va = out["c"][1].edge_verdict_all
            swept = va != -1
            assert bool((swept == ~torch.isnan(out["s"][1].edge_margin_all)).all())
            idx = torch.nonzero(swept)
            rows_c, n_min, n_max = 0, MAX_SAMPLES, 0
            for lo in range(0, len(idx), 1 << 20):
                b, t, s1, s0 = idx[lo:lo + (1 << 20)].T
                n = ck.certified_sweep(dn[b, t - 1, s0], dn[b, t, s1], RESOLUTION, max_samples=MAX_SAMPLES).n_samples
                rows_c += int((n + 2).sum().item()); n_min = min(n_min, int(n.min().item())); n_max = max(n_max, int(n.max().item()))
            edges = int(swept.sum().item())
            rows_s = M_FIXED * edges
            v = va[swept]
            ns = {k: 1e6 * np.median(ts[k]) / (rows_s if k == "s" else rows_c) for k in legs}
            tracked = {k: int(out[k][0].n_tracked.sum().item()) for k in legs}
            print(f"{name:5s} {ck.n_pairs:4d} pairs {B:5d} instances, {edges} swept edges, n_samples {n_min} .. {n_max} (mean {rows_c / edges - 2:.1f}); "
                  f"verdicts certified / undecided / colliding {int((v == 1).sum())} / {int((v == 0).sum())} / {int((v == 2).sum())}\n"
                  f"    (s) {cell(ts['s'])} = {ns['s']:7.3f} ns/row of {rows_s}   (c) {cell(ts['c'])} = {ns['c']:7.3f} ns/row of {rows_c}   "
                  f"(r) {cell(ts['r'])} = {ns['r']:7.3f} ns/row   (c)/(s) per row = {ns['c'] / ns['s']:5.3f}, per call = "
                  f"{np.median(ts['c']) / np.median(ts['s']):5.3f}; tracked waypoints of {B * T}: (s) {tracked['s']} (c) {tracked['c']} (r) {tracked['r']}, "
                  f"certified chosen edges (c) {int(out['c'][1].n_certified.sum().item())} (r) {int(out['r'][1].n_certified.sum().item())}", flush=True)
            ck.close()


if __name__ == "__main__":
    main()
