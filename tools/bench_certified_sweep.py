#!/usr/bin/env python
"""Certified sweep (mkh_certified_sweep): what an evaluated sample row costs, against mkh_swept_clearance on the same edges.

    python tools/bench_certified_sweep.py [rounds=7] > profiles/r29_certified_sweep.txt

Wall clock around each leg with a device synchronisation at its end; the legs ALTERNATE, `rounds` times after a warm-up round;
reported: the median and the (max - min) of each leg's rounds.  mkh_swept_clearance is the parent commit's entry point, unchanged:
it is the baseline.  UR5e 14 pairs (four edges per wavefront), G1 46 pairs, ALOHA 1 104 pairs (one per wavefront), at 2 048 and
16 384 edges, device-resident; resolution 0.02 m, max_samples 64.  The ends differ in hinge and slide joints only, so an edge
scaled by s has s times the motion, and its sample count is the tool's to choose:
  (equal)  every edge scaled to motion = 16.5 resolution: n_samples = 16 on every edge, asserted.
             (c) mkh_certified_sweep: 18 evaluated rows per edge (the ends are points)
             (s) mkh_swept_clearance at n_samples = 16: 16 rows per edge
           per-row cost of each, and (c)/(s).  What (c) pays beyond the sweep: two LDS rows of pairs per point — the cone of every
           pair against the previous point — and the L_k pass over (pairs x joints) once per edge.
  (mixed)  the same edges scaled to n_samples drawn uniformly from 2 .. 62 (mean 32), in random order: the groups of a wavefront
           walk to the largest count among them (four edges per wavefront), and wavefronts finish at different times.
             (c) as drawn; (o) the same edges ORDERED by count, so that the four groups of a wavefront agree
             (s) mkh_swept_clearance at n_samples = 32 on the same edges: the fixed count with the same total
           per evaluated row; (c)/(o) is the cost of the imbalance inside wavefronts, (o)/(s) what is left.
The margins of (c) and (s) are held against each other where they must agree: min(ends, sweep at the same count) on the equal
edges, to 1e-9."""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

RESOLUTION, MAX_SAMPLES, M_EQUAL, M_MIX = 0.02, 64, 16, (2, 62)


def cell(ts):
    return f"{np.median(ts):9.3f} [{np.max(ts) - np.min(ts):7.3f}] ms"


def main():
    import torch

    import mink_amd as mink
    from bench_clearance import checker
    from mink_amd import _native as nat
    from mink_amd import workloads

    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_certified_sweep needs a GPU")
    dev = torch.device("cuda:0")
    to = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def alternate(legs):
        for fn in legs.values():
            wall(fn)
        ts = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                ts[k].append(wall(fn)[0])
        return {k: np.array(v) for k, v in ts.items()}

    print(f"# tools/bench_certified_sweep.py {' '.join(sys.argv[1:])}   ({rounds} alternating rounds; median [max - min]; resolution "
          f"{RESOLUTION} m, max_samples {MAX_SAMPLES})")
    for name in ("ur5e", "g1", "aloha"):
        for N in (2048, 16384):
            model, ck = checker(mink, workloads, name, max_rows=1 << 16)
            key = {"g1": "stand", "aloha": "neutral_pose"}.get(name)
            base = None if key is None else model.key_qpos[model.name2id("key", key)]
            rng = np.random.default_rng(2)
            a, b0 = (workloads.sample_q(model, rng, N, base_q=base) for _ in range(2))
            for j in range(model.njnt):                                     # a free or ball joint stays where it is: the motion is the scalars'
                jt, qa = int(model.jnt_type[j]), int(model.jnt_qposadr[j])
                if jt in (0, 1):
                    b0[:, qa:qa + (7 if jt == 0 else 4)] = a[:, qa:qa + (7 if jt == 0 else 4)]
            motion0 = ck.certified_sweep(a, b0, RESOLUTION, max_samples=MAX_SAMPLES).motion
            assert np.isfinite(motion0).all() and (motion0 > 0).all()

            def scaled(counts):
                """The edges scaled so that edge e gets n_samples = counts[e]: motion = (counts + 0.5) resolution."""
                s = (counts + 0.5) * RESOLUTION / motion0
                return a + s[:, None] * (b0 - a)

            # ---- equal lengths
            b = scaled(np.full(N, M_EQUAL))
            da, db = to(a), to(b)
            cert = lambda: ck.certified_sweep(da, db, RESOLUTION, max_samples=MAX_SAMPLES)
            sweep = lambda: ck.swept_clearance(da, db, n_samples=M_EQUAL)
            ts = alternate({"c": cert, "s": sweep})
            c, s = cert(), sweep()
            assert (c.n_samples == M_EQUAL).all() and not c.capped.any()
            ends = torch.minimum(ck.clearance(da).margin, ck.clearance(db).margin)
            worst = float((torch.minimum(ends, s.margin) - c.margin).abs().max().item())
            assert worst <= 1e-9, worst
            rows_c, rows_s = N * (M_EQUAL + 2), N * M_EQUAL
            ns_c, ns_s = 1e6 * np.median(ts["c"]) / rows_c, 1e6 * np.median(ts["s"]) / rows_s
            v = c.verdict.cpu().numpy()
            print(f"(equal) {name:6s} {ck.n_pairs:5d} pairs {N:6d} edges, n_samples {M_EQUAL}: (c) {cell(ts['c'])} = {ns_c:8.3f} ns/row of {rows_c}   "
                  f"(s) {cell(ts['s'])} = {ns_s:8.3f} ns/row of {rows_s}   (c)/(s) per row = {ns_c / ns_s:5.3f}   [certified / undecided / "
                  f"colliding {int((v == 1).sum())} / {int((v == 0).sum())} / {int((v == 2).sum())}; max |min(ends, (s)) - (c)| {worst:.1e}]", flush=True)
            # ---- a mix of lengths
            counts = rng.integers(M_MIX[0], M_MIX[1] + 1, size=N)
            b = scaled(counts)
            order = np.argsort(counts, kind="stable")
            da, db, oa, ob = to(a), to(b), to(a[order]), to(b[order])
            M_mean = int(round(counts.mean()))
            legs = {"c": lambda: ck.certified_sweep(da, db, RESOLUTION, max_samples=MAX_SAMPLES),
                    "o": lambda: ck.certified_sweep(oa, ob, RESOLUTION, max_samples=MAX_SAMPLES),
                    "s": lambda: ck.swept_clearance(da, db, n_samples=M_mean)}
            ts = alternate(legs)
            got = legs["c"]().n_samples.cpu().numpy()
            assert (got == counts).all(), (got[:8], counts[:8])
            rows_c, rows_s = int((counts + 2).sum()), N * M_mean
            ns = {k: 1e6 * np.median(ts[k]) / (rows_s if k == "s" else rows_c) for k in legs}
            print(f"(mixed) {name:6s} {ck.n_pairs:5d} pairs {N:6d} edges, n_samples {counts.min()} .. {counts.max()} (mean {counts.mean():.1f}): "
                  f"(c) {cell(ts['c'])} = {ns['c']:8.3f} ns/row of {rows_c}   (o) ordered {cell(ts['o'])} = {ns['o']:8.3f} ns/row   "
                  f"(s) n_samples {M_mean} {cell(ts['s'])} = {ns['s']:8.3f} ns/row of {rows_s}   (c)/(o) = {ns['c'] / ns['o']:5.3f}   "
                  f"(o)/(s) = {ns['o'] / ns['s']:5.3f}   (c)/(s) = {ns['c'] / ns['s']:5.3f}", flush=True)
            ck.close()


if __name__ == "__main__":
    main()
