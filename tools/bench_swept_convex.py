#!/usr/bin/env python
"""Swept clearance on checkers WITH general convex pairs (CollisionChecker(sweep_rows=), convex_sweep.hip): what it costs.

    python tools/bench_swept_convex.py [rounds=7] [parts=asi] > profiles/r26_swept_convex.txt

Wall clock around each leg with a device synchronisation at its end; the legs of a part ALTERNATE, `rounds` times after a
warm-up round; reported: the median and the (max - min) of each leg's rounds.  Device tensors in and out, but for (s).
  (a) per SAMPLE ROW, N = 2 048 and 16 384 edges of M = 8 samples, on `ur5e_convex` (the wrist cylinder against floor and box wall:
      one general convex pair of two) and on `convex_shapes` (tests/swept_convex_cases.py: nine of fifteen) —
        (f) the checked sweep, sweep_rows = N·M: one convex_sweep_kernel launch and one sweep_kernel launch
        (c) the same with sweep_rows = 16 384: chunks of 2 048 edges
        (m) what a caller could do before: the N·M sample rows materialised on the device (timed), then mkh_clearance on them
        (n) the sweep on the same checker WITHOUT its general convex pairs: the price of the routine is (f) - (n)
      (f)'s margin must be the minimum of (m)'s over each edge's rows: asserted to 1e-9.
  (s) the sparse checked ladder: ladder_path on `convex_shapes` nodes, B = 64, T = 16, S = 8, M = 8, with a checker no node
      collides with (minimum distance -10 m), every node tracked against one node in seven: the pre-pass skips the edges into
      the others; and the same two calls on the checker without general convex pairs.  Host arrays (ladder_path's interface):
      the copies are the same in all four legs.
  (i) items per wavefront of the pre-pass, leg (f) again: the launch's own choice (0) against fixed values.  Needs an experiment
      build (MKH_BUILD_TAG=dbg MKH_EXTRA_FLAGS=-DMKH_DEBUG_SWITCHES python -m mink_amd.csrc.build; run with MKH_LIB_TAG=dbg): the
      product library does not read the environment, and the part says so instead of measuring nothing.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

M = 8


def cell(ts):
    return f"{np.median(ts):9.3f} [{np.max(ts) - np.min(ts):7.3f}] ms"


def checkers(mink, name, sweep_rows, max_rows, dmin=None):
    """(model, checker with its general convex pairs, checker without them, n_cv)."""
    import clearance_ref as cr
    import swept_convex_cases as sc
    if name == "ur5e_convex":
        model, spec, _ = cr.fixture("ur5e_convex")
        lean = [dict(spec[0], geom_pairs=[(["wrist_3_link"], ["floor"])])]
        n_cv = 1
    else:
        model, spec, _ = sc.shapes()
        lean = [dict(spec[0], geom_pairs=[p for p, (_, _, g) in zip(spec[0]["geom_pairs"], sc.PAIRS) if not g])]
        n_cv = sum(1 for _, _, g in sc.PAIRS if g)
    if dmin is not None:
        spec, lean = [dict(kw, minimum_distance_from_collisions=dmin) for kw in spec], [dict(kw, minimum_distance_from_collisions=dmin) for kw in lean]
    mk = lambda s, rows: mink.CollisionChecker(model, [mink.CollisionAvoidanceLimit(model, **kw) for kw in s], max_rows=max_rows, sweep_rows=rows)
    return model, mk(spec, sweep_rows), mk(lean, 0), n_cv


def main():
    import torch

    import clearance_ref as cr
    import mink_amd as mink
    import swept_convex_cases as sc
    from mink_amd import _native as nat

    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    parts = sys.argv[2] if len(sys.argv) > 2 else "asi"
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_swept_convex needs a GPU")
    dev = torch.device("cuda:0")
    to = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)

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

    def edges(model, N):
        rng = np.random.default_rng(2)
        return to(cr._uniform_in_ranges(model, rng, N)), to(cr._uniform_in_ranges(model, rng, N))

    u = to((np.arange(1, M + 1, dtype=np.float64) / float(M + 1))[None, :, None])
    print(f"# tools/bench_swept_convex.py {' '.join(sys.argv[1:])}   ({rounds} alternating rounds; median [max - min]; M = {M} samples per edge; "
          f"library {os.path.basename(nat._LIB_PATH)})")
    if "a" in parts:
        print("(a) per sample row: (f) checked sweep, one chunk; (c) chunks of 2 048 edges; (m) rows materialised + mkh_clearance; (n) without the general convex pairs")
        for name in ("ur5e_convex", "convex_shapes"):
            for N in (2048, 16384):
                model, ck, lean, n_cv = checkers(mink, name, N * M, N * M)
                _, ck_c, _, _ = checkers(mink, name, 16384, 256)
                da, db = edges(model, N)
                rows = lambda: (da[:, None, :] + u * (db - da)[:, None, :]).reshape(N * M, model.nq)     # (hinges and slides only)
                ts = alternate({"f": lambda: ck.swept_clearance(da, db, n_samples=M), "c": lambda: ck_c.swept_clearance(da, db, n_samples=M),
                                "m": lambda: ck.clearance(rows()), "n": lambda: lean.swept_clearance(da, db, n_samples=M)})
                f, c, mm = ck.swept_clearance(da, db, n_samples=M), ck_c.swept_clearance(da, db, n_samples=M), ck.clearance(rows())
                worst = float((f.margin - mm.margin.reshape(N, M).min(dim=1).values).abs().max().item())
                assert worst <= 1e-9, worst
                assert bool((f.margin == c.margin).all().item()) and bool((f.pair == c.pair).all().item())
                ns = {k: 1e6 * np.median(v) / (N * M) for k, v in ts.items()}
                print(f"  {name:13s} {ck.n_pairs:2d} pairs ({n_cv} general convex) {N:6d} edges = {N * M:7d} rows: (f) {cell(ts['f'])} = {ns['f']:7.2f} ns/row   "
                      f"(c) {cell(ts['c'])} = {ns['c']:7.2f}   (m) {cell(ts['m'])} = {ns['m']:7.2f}   (n) {cell(ts['n'])} = {ns['n']:7.2f}   "
                      f"(f)/(m) = {ns['f'] / ns['m']:5.3f}   routine (f) - (n) = {ns['f'] - ns['n']:7.2f} ns/row   "
                      f"[max |(f) - min (m)| {worst:.1e}; {int(f.in_collision.sum().item())} edges collide]", flush=True)
                for x in (ck, ck_c, lean):
                    x.close()
    if "s" in parts:
        B, T, S = 64, 16, 8
        model, ck, lean, _ = checkers(mink, "convex_shapes", B * T * S * S * M, B * T * S, dmin=-10.0)
        rng = np.random.default_rng(5)
        nodes = cr._uniform_in_ranges(model, rng, B * T * S).reshape(B, T, S, model.nq)
        cfg = mink.Configuration(model, np.tile(np.asarray(model.qpos0, dtype=np.float64), (B, 1)))
        dense = np.ones((B, T, S), dtype=bool)
        sparse = rng.random((B, T, S)) < 1.0 / 7.0
        call = lambda c, trk: (lambda: mink.ladder_path(cfg, nodes, trk, collision_check=c, edge_samples=M))
        ts = alternate({"cd": call(ck, dense), "cs": call(ck, sparse), "ad": call(lean, dense), "as": call(lean, sparse)})
        n_d, n_s = B * (T - 1) * S * S * M, int(sparse[:, 1:].sum()) * S * M
        md = {k: np.median(v) for k, v in ts.items()}
        print(f"(s) convex_shapes ladder B={B} T={T} S={S}: every node tracked ({n_d} swept sample rows): with general convex pairs {cell(ts['cd'])}, "
              f"without {cell(ts['ad'])}: the pairs add {md['cd'] - md['ad']:8.3f} ms;  one node in seven tracked ({n_s} rows): with "
              f"{cell(ts['cs'])}, without {cell(ts['as'])}: they add {md['cs'] - md['as']:8.3f} ms — a pre-pass that did not skip unswept "
              f"edges would add the first figure to both", flush=True)
        ck.close(); lean.close()
    if "i" in parts:
        if os.environ.get("MKH_LIB_TAG", "") == "":
            print("(i) items per wavefront: skipped — the product library does not read MKH_DEBUG_CONVEX_SWEEP_IPW (run an experiment build)")
            return
        print("(i) items per wavefront of convex_sweep_kernel, leg (f): 0 = the launch's own choice (about 4 096 wavefronts, at most 64 items each)")
        for name in ("ur5e_convex", "convex_shapes"):
            for N in (2048, 16384):
                model, ck, lean, n_cv = checkers(mink, name, N * M, 256)
                da, db = edges(model, N)

                def leg(ipw):
                    def run():
                        os.environ["MKH_DEBUG_CONVEX_SWEEP_IPW"] = str(ipw)
                        return ck.swept_clearance(da, db, n_samples=M)
                    return run

                ts = alternate({ipw: leg(ipw) for ipw in (0, 1, 2, 4, 8, 16, 32, 64)})
                os.environ.pop("MKH_DEBUG_CONVEX_SWEEP_IPW", None)
                auto = min(64, max(1, (N * M * n_cv + 4095) // 4096))
                print(f"  {name:13s} {N:6d} edges x {M} x {n_cv} items (own choice: {auto}): " +
                      "   ".join(f"ipw {k:2d}: {np.median(v):8.3f} [{np.max(v) - np.min(v):6.3f}]" for k, v in ts.items()) + "  ms", flush=True)
                ck.close(); lean.close()


if __name__ == "__main__":
    main()
