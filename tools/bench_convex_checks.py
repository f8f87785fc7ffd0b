#!/usr/bin/env python
"""Checked candidate tracking and the checked refinement pass on checkers WITH general convex pairs
(CollisionChecker(check_rows=), convex_check.hip): what they cost.

    python tools/bench_convex_checks.py [rounds=5] [parts=tur] > profiles/r27_convex_checks.txt

Wall clock around each leg with a device synchronisation at its end; the legs of a part ALTERNATE, `rounds` times after a
warm-up round; reported: the median and the (max - min) of each leg's rounds.  Device tensors in and out, but for (u).  T = 64 waypoints,
M = 8 samples per edge, on `ur5e_convex` (the wrist cylinder against floor and box wall: one general convex pair of two) and on
`convex_shapes` (tests/swept_convex_cases.py: nine of fifteen).
  (t) the tracking check, mkh_select_trajectory_candidates on B = 16 instances of S = 16 device-resident candidates (16 384 rows) —
        (f) with the checker, check_rows holding every row: one convex_check_kernel and one tmf_check_cv_kernel launch
        (c) the same with check_rows = 16 384: chunks of 1 820 rows
        (n) the same call on the checker WITHOUT its general convex pairs: the price of those pairs is (f) - (n)
        (o) the composition that existed before on the same candidates: clearance on all rows, swept_clearance (sweep_rows) on all
            edges, and a mask — no selection, so it flatters (o)
      and the share of the pre-pass's evaluations the check never read: the samples of rows whose node collides.
  (u) the checked tracking CALL, solve_ik_trajectory_multistart(collision_check=) — loops, check, selection; host arrays, the
      public call's interface: the copies are the same in all legs — on B = 64 instances of 16 candidates, 20 iterations per waypoint:
        (f) with the checker, check_rows holding every row, (n) the checker without its general convex pairs, (p) no checker.
  (r) the checked refinement pass, mkh_ladder_refine_free on B = 64 random paths, every second waypoint flagged lost —
        (f) with the checker (check_rows and sweep_rows holding everything), (n) without its general convex pairs.
"""
import importlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

M, T = 8, 64


def cell(ts):
    return f"{np.median(ts):9.3f} [{np.max(ts) - np.min(ts):7.3f}] ms"


def world(mink, name):
    """(model, limit kwargs with the general convex pairs, without them, n_cv, frame of the task, home)."""
    import clearance_ref as cr
    import swept_convex_cases as sc
    if name == "ur5e_convex":
        model, spec, _ = cr.fixture("ur5e_convex")
        lean = [dict(spec[0], geom_pairs=[(["wrist_3_link"], ["floor"])])]
        return model, spec, lean, 1, ("attachment_site", "site"), np.asarray(model.key_qpos[model.name2id("key", "home")], dtype=np.float64)
    model, spec, _ = sc.shapes()
    lean = [dict(spec[0], geom_pairs=[p for p, (_, _, g) in zip(spec[0]["geom_pairs"], sc.PAIRS) if not g])]
    return model, spec, lean, sum(1 for _, _, g in sc.PAIRS if g), ("s8", "body"), np.asarray(model.qpos0, dtype=np.float64)


def main():
    import torch

    import clearance_ref as cr
    import mink_amd as mink
    from mink_amd import _native as nat

    sik = importlib.import_module("mink_amd.solve_ik")
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    parts = sys.argv[2] if len(sys.argv) > 2 else "tur"
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_convex_checks needs a GPU")
    dev = torch.device("cuda:0")
    to = lambda x: torch.as_tensor(np.array(x), device=dev)

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

    mk = lambda model, s, **kw: mink.CollisionChecker(model, [mink.CollisionAvoidanceLimit(model, **x) for x in s], **kw)
    print(f"# tools/bench_convex_checks.py {' '.join(sys.argv[1:])}   ({rounds} alternating rounds; median [max - min]; T = {T} waypoints, "
          f"M = {M} samples per edge; library {os.path.basename(nat._LIB_PATH)})")
    for name in ("ur5e_convex", "convex_shapes"):
        model, spec, lean_spec, n_cv, frame, home1 = world(mink, name)
        nq = model.nq
        if "t" in parts:
            B, S = 16, 16
            R, N = B * S, T * B * S
            ck = mk(model, spec, max_rows=N, check_rows=N * (1 + M), sweep_rows=N * M)
            ck_c = mk(model, spec, max_rows=N, check_rows=16384)
            lean = mk(model, lean_spec, max_rows=N)
            rng = np.random.default_rng(2)
            # candidates that move a little from waypoint to waypoint, as tracked ones do
            first = cr._uniform_in_ranges(model, rng, R)
            q_all = to(first[None] + 0.02 * np.cumsum(rng.normal(size=(T, R, nq)), axis=0))
            q = to(np.tile(home1, (B, 1)))
            cfg = mink.Configuration(model, np.tile(home1, (B, 1)))
            prob, layout = sik._compile(cfg, [mink.PostureTask(model, cost=1.0)], None, 1, devices=cfg.devices[:1])
            with sik._pin(cfg, layout):
                sel = lambda c: (lambda: prob.select_trajectory_candidates(q, q_all, None, None, c, M, True))

                def composed():
                    nodes = ck.clearance(q_all.reshape(N, nq))
                    edges = ck.swept_clearance(q_all[:-1].reshape(N - R, nq), q_all[1:].reshape(N - R, nq), n_samples=M)
                    free = nodes.margin.reshape(T, R) >= 0.0
                    return torch.where(free[1:], edges.margin.reshape(T - 1, R), torch.full_like(edges.margin.reshape(T - 1, R), float("nan")))

                ts = alternate({"f": sel(ck), "c": sel(ck_c), "n": sel(lean), "o": composed})
                (_, more), (_, more_c), edge_o = sel(ck)(), sel(ck_c)(), composed()
            torch.cuda.synchronize()
            nm, em = more.node_margin_all, more.edge_margin_all
            assert bool((nm == more_c.node_margin_all).all().item()) and bool((em[1:].nan_to_num(7.0) == more_c.edge_margin_all[1:].nan_to_num(7.0)).all().item())
            # ((o)'s margins come from other kernels: compared where both swept, to 1e-9)
            worst = float((em[1:] - edge_o).nan_to_num(0.0).abs().max().item())
            assert worst <= 1e-9 and int((em[1:].isnan() != edge_o.isnan()).sum().item()) <= 2, worst
            hit = int((~(nm >= 0.0)).sum().item())
            # the pre-pass: every node, and M samples of every row with a predecessor (all converged, status 0); the check reads the
            # nodes and the samples behind a free node
            pre, read = N + (N - R) * M, N + int((nm[1:] >= 0.0).sum().item()) * M
            md = {k: np.median(v) for k, v in ts.items()}
            print(f"(t) {name:13s} {ck.n_pairs:2d} pairs ({n_cv} general convex) {N} rows: (f) {cell(ts['f'])}   (c) {cell(ts['c'])}   "
                  f"(n) {cell(ts['n'])}   (o) {cell(ts['o'])}   the pairs cost (f) - (n) = {md['f'] - md['n']:8.3f} ms   (f)/(o) = {md['f'] / md['o']:5.3f}   "
                  f"[{hit} of {N} nodes collide; the pre-pass evaluates {pre} rows, the check reads {read}: {100.0 * (pre - read) / pre:4.1f} % never read; "
                  f"max |(f) - (o)| {worst:.1e}]", flush=True)
            for x in (ck, ck_c, lean):
                x.close()
        if "u" in parts:
            B, S = 64, 16
            N = T * B * S
            ck = mk(model, spec, max_rows=N, check_rows=N * (1 + M))
            lean = mk(model, lean_spec, max_rows=N)
            rng = np.random.default_rng(4)
            first = cr._uniform_in_ranges(model, rng, B)
            path = first[:, None] + 0.02 * np.cumsum(rng.normal(size=(B, T, nq)), axis=1)
            task = mink.FrameTask(*frame, 1.0, 1.0, lm_damping=1.0)
            tg = mink.Configuration(model, path.reshape(-1, nq)).get_transform_frame_to_world(*frame).wxyz_xyz.reshape(B, T, 7)
            cfg = mink.Configuration(model, np.tile(home1, (B, 1)))
            call = lambda **kw: (lambda: mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: tg}, S, 20, 1e-4, 1e-4, damping=1e-3,
                                                                            limits=[mink.ConfigurationLimit(model)], rng_seed=5,
                                                                            update=False, **kw))
            ts = alternate({"f": call(collision_check=ck, edge_samples=M), "n": call(collision_check=lean, edge_samples=M), "p": call()})
            out = call(collision_check=ck, edge_samples=M)()
            md = {k: np.median(v) for k, v in ts.items()}
            print(f"(u) {name:13s} {ck.n_pairs:2d} pairs ({n_cv} general convex) B = {B}, {S} candidates, {N} rows: (f) {cell(ts['f'])}   (n) {cell(ts['n'])}   "
                  f"(p) {cell(ts['p'])}   the pairs cost (f) - (n) = {md['f'] - md['n']:8.3f} ms, the check (f) - (p) = {md['f'] - md['p']:8.3f} ms   "
                  f"[free tracked waypoints {int(out.n_tracked.sum())} of {B * T}]", flush=True)
            ck.close(); lean.close()
        if "r" in parts:
            B = 64
            ck = mk(model, spec, max_rows=B * T, check_rows=B * (1 + 2 * M), sweep_rows=B * T * M)
            lean = mk(model, lean_spec, max_rows=B * T)
            rng = np.random.default_rng(3)
            first = cr._uniform_in_ranges(model, rng, B)
            path = first[:, None] + 0.02 * np.cumsum(rng.normal(size=(B, T, nq)), axis=1)
            trk = np.ones((B, T), np.int32)
            trk[:, 1::2] = 0
            cfg = mink.Configuration(model, np.tile(home1, (B, 1)))
            task = mink.FrameTask(*frame, 1.0, 1.0, lm_damping=1.0)
            tg = mink.Configuration(model, path.reshape(-1, nq)).get_transform_frame_to_world(*frame).wxyz_xyz.reshape(B, T, 1, 7)
            prob, layout = sik._compile(cfg, [task], [mink.ConfigurationLimit(model)], B, 1.0, devices=cfg.devices[:1])
            d = [to(np.tile(home1, (B, 1))), to(path), to(trk), to(tg)]
            with sik._pin(cfg, layout):
                leg = lambda c: (lambda: prob.ladder_refine_free(d[0], d[1], c, d[2], d[3], None, None, 1.0, 1e-3, max_iters=20,
                                                                 pos_threshold=1e-4, ori_threshold=1e-4, edge_samples=M))
                ts = alternate({"f": leg(ck), "n": leg(lean)})
                out = leg(ck)()
            torch.cuda.synchronize()
            md = {k: np.median(v) for k, v in ts.items()}
            print(f"(r) {name:13s} {ck.n_pairs:2d} pairs ({n_cv} general convex) B = {B}: (f) {cell(ts['f'])}   (n) {cell(ts['n'])}   the pairs cost "
                  f"(f) - (n) = {md['f'] - md['n']:8.3f} ms = {1e3 * (md['f'] - md['n']) / (2 * T - 1):7.1f} us per step of the pass   "
                  f"[{int((out.repaired != 0).sum().item())} of {B * T // 2} lost waypoints repaired]", flush=True)
            ck.close(); lean.close()


if __name__ == "__main__":
    main()
