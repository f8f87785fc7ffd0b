#!/usr/bin/env python
"""Ladder-graph trajectory IK (mkh_solve_trajectory_ladder): what the search costs next to the loops whose rungs it reads, and
the whole call next to the two things a caller would do instead.

    python tools/bench_ladder.py [workloads=ur5e_c2:256:8,...] [rounds=5] [T=64] [nohost] > profiles/r15_ladder.txt

Per workload (bench config : B instances : S nodes per waypoint; T waypoints along a joint-space line from the bench batch's
start; the threshold-terminated loop, up to 20 steps per node), device tensors in and out unless said otherwise:
  (a) the call: q fanned out, the multi-start launch(es) over the B·T flattened targets (chunks of whole rungs beyond the
      handle's max_batch), tracked flags, the search, five gathers
  (s) the search alone on (a)'s rungs: mkh_ladder_select (the dynamic program and one gather) — its share of (a) is (s) / (a)
  (h) the host composition (a) replaces: solve_multistart(return_all) with HOST arrays over the flattened targets — B·T·S rows
      of q, status, converged and iterations over the bus, in chunks of max_batch — and the dynamic program vectorised in
      numpy over (s', s), instance by instance (tests/ladder_ref.py: costs + search_fast)
  (m) solve_trajectory_multistart at the same B, T, S: S whole candidates tracked through T stream-ordered loop launches of
      B·S rows (its kernels are the parent commit's: adding the ladder moved no code_sha256 of kernel_resources.json)
  (r) the refined call: (a) with the refinement pass behind its search (mkh_solve_trajectory_ladder_refined) — 2T − 1 loop
      launches on the B chosen paths, one small kernel between two of them, the guard; (r) − (a) is what the pass costs
  (t) what those loop launches should cost: solve_trajectory on the B instances, TWICE (2T loop launches of B rows between
      time-major slabs, no kernel in between); ((r) − (a)) − (t) is the gap the pass leaves to it
Wall clock around the leg with a device synchronisation at its end, ms per call.  The legs ALTERNATE, `rounds` times after a
warm-up round ((h): one round beyond 256 instances — it runs for seconds); reported: the median and the (max - min) of each
leg's rounds.  Complete paths (every waypoint tracked) of (a), (r) and (m) are printed with them: the calls answer different
questions on the same targets.  `nohost` leaves leg (h) out (it runs for tens of seconds at 4 096 instances).
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from bench_trajectory import MAX_ITERS, THRESHOLDS  # noqa: E402

DEFAULT = ",".join(f"{n}:{b}:{s}" for n in ("ur5e_c2", "g1_c3") for b in (256, 4096) for s in (8, 16, 64))
MAX_BATCH = 1 << 20         # loop rows per launch of this tool's handles: larger ladders run in chunks of whole rungs


def host_composition(prob, model, q, tg_flat, pt, dt, damping, S, T, until, ladder_ref):
    """Leg (h): the rungs over the bus, then the dynamic program in numpy.  Returns (node_index (B, T), n_tracked (B,))."""
    B = len(q)
    per = max(1, prob.max_batch // S)
    flat_q = np.repeat(q, T, axis=0)
    parts = []
    for r0 in range(0, B * T, per):
        r1 = min(B * T, r0 + per)
        parts.append(prob.solve_multistart(flat_q[r0:r1], tg_flat[r0:r1], pt, None, dt, damping, n_seeds=S, max_iters=MAX_ITERS,
                                           pos_threshold=until[0], ori_threshold=until[1], rng_seed=3, target_index0=r0, return_all=True))
    q_all = np.concatenate([p.q_all for p in parts]).reshape(B, T, S, model.nq)
    trk = ladder_ref.tracked(np.concatenate([p.converged_all for p in parts]), np.concatenate([p.status_all for p in parts])).reshape(B, T, S)
    nodes, n_tracked = np.zeros((B, T), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        start, edges = ladder_ref.costs(model, q[b], q_all[b])
        nodes[b], key, _ = ladder_ref.search_fast(start, edges, ~trk[b])
        n_tracked[b] = T - key[0]
    return nodes, n_tracked


def main():
    import torch

    import ladder_ref
    from mink_amd import _native as nat
    from mink_amd import workloads

    specs = (sys.argv[1] if len(sys.argv) > 1 else DEFAULT).split(",")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    host = not (len(sys.argv) > 4 and sys.argv[4] == "nohost")
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_ladder needs a GPU")
    dev = torch.device("cuda:0")
    print(f"# tools/bench_ladder.py {' '.join(sys.argv[1:])}   (T = {T} waypoints, up to {MAX_ITERS} steps per node, {rounds} alternating "
          f"rounds; ms per call: median [max - min])", flush=True)
    for spec in specs:
        name, B, S = spec.split(":")
        B, S = int(B), int(S)
        N = B * T * S
        m = workloads.load_bench_robot(name)
        nm = nat.NativeModel(m)
        prob, dt, damping = workloads.bench_config(name, m, nm, min(N, MAX_BATCH))
        cand, _, _ = workloads.bench_config(name, m, nm, B * S)                   # leg (m)'s handle: B·S rows
        rng = np.random.default_rng(1)
        q, _, pt, _ = workloads.bench_batch(name, m, nm, cand, rng, B)
        delta = rng.normal(scale=0.15, size=(B, m.nv))
        dummy = np.zeros((B, cand.n_frame, 7)); dummy[:, :, 0] = 1.0
        tg = np.ascontiguousarray(np.stack([cand.solve(nm.integrate(q, delta * ((t + 1) / T), 1.0), dummy, pt, None, 1.0, 1.0,
                                                       taps=["frame_pose"], solve_qp=False)[2]["frame_pose"] for t in range(T)], axis=1))
        tg_flat = tg.reshape(B * T, cand.n_frame, 7)
        to = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        dq, dpt, d_tg = to(q), to(pt), to(tg)
        until = THRESHOLDS[name]
        kw = dict(n_seeds=S, pos_threshold=until[0], ori_threshold=until[1], rng_seed=3)
        first = prob.solve_trajectory_ladder(dq, d_tg, dpt, None, dt, damping, max_iters=MAX_ITERS, return_all=True, **kw)
        k_loop = prob.last_kernel()
        d_nodes = first.q_all
        d_trk = ((first.converged_all != 0) & ((first.status_all & ~1) == 0)).to(torch.int32)
        n_bad = int(((first.status_all & ~1) != 0).sum().item())
        del first

        def leg_a():
            return prob.solve_trajectory_ladder(dq, d_tg, dpt, None, dt, damping, max_iters=MAX_ITERS, **kw)

        def leg_s():
            return prob.ladder_select(dq, d_nodes, d_trk)

        def leg_h():
            return host_composition(prob, m, q, tg_flat, pt, dt, damping, S, T, until, ladder_ref)

        def leg_m():
            return cand.solve_trajectory_multistart(dq, d_tg, dpt, None, dt, damping, n_steps=MAX_ITERS, **kw)

        def leg_r():
            return prob.solve_trajectory_ladder(dq, d_tg, dpt, None, dt, damping, max_iters=MAX_ITERS, refine=True, **kw)

        def leg_t():
            for _ in range(2):
                out = cand.solve_trajectory(dq, d_tg, dpt, None, dt, damping, n_steps=MAX_ITERS, until=until)
            return out

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0), out

        ra, rs = leg_a(), leg_s()
        assert torch.equal(ra.node_index, rs.node_index) and torch.equal(ra.q, rs.q), "the call's path is not the search's on its rungs"
        for fn in (leg_a, leg_s, leg_m, leg_r, leg_t):           # warm-up round
            wall(fn)
        ts = {k: [] for k in "ashmrt"}
        rh = None
        for r in range(rounds):
            ts["a"].append(wall(leg_a)[0]); ts["s"].append(wall(leg_s)[0]); ts["m"].append(wall(leg_m)[0])
            ts["r"].append(wall(leg_r)[0]); ts["t"].append(wall(leg_t)[0])
            if host and (r == 0 or B <= 256):
                t, rh = wall(leg_h)
                ts["h"].append(t)
        if not host:
            ts["h"].append(float("nan"))
        rm, rr = leg_m(), leg_r()
        assert rh is None or np.array_equal(rh[1], ra.n_tracked.cpu().numpy()), "the host composition tracks other waypoints than the call"
        worse = ((T - rr.n_tracked > T - ra.n_tracked) | ((rr.n_tracked == ra.n_tracked) & (rr.n_breaks > ra.n_breaks))).any().item()
        assert not worse, "the refined call returned a path worse than the search's"
        med = {k: float(np.median(v)) for k, v in ts.items()}
        spread = {k: float(np.max(v) - np.min(v)) for k, v in ts.items()}
        cell = lambda k: f"{med[k]:10.3f} [{spread[k]:8.3f}]"
        print(f"{name:8s} B={B:5d} S={S:3d} ({N} loops in {-(-N // prob.max_batch)} launch(es) of kernel {k_loop}): (a) ladder call {cell('a')}  "
              f"(s) search alone {cell('s')} = {100.0 * med['s'] / med['a']:5.2f} % of (a)  (h) host composition {cell('h')} = "
              f"{med['h'] / med['a']:6.2f} x (a)  (m) candidate tracking {cell('m')} = {med['m'] / med['a']:6.2f} x (a)  |  complete paths of {B}: "
              f"ladder {int((ra.n_tracked == T).sum().item())}, refined {int((rr.n_tracked == T).sum().item())}, candidate tracking "
              f"{int((rm.n_tracked == T).sum().item())}; "
              f"[{n_bad} nodes with a failure bit]", flush=True)
        pass_ms = med["r"] - med["a"]
        print(f"{'':8s} refinement: (r) refined call {cell('r')} = {med['r'] / med['a']:6.3f} x (a); the pass (r) - (a) = {pass_ms:10.3f} ms; "
              f"(t) two trajectory calls on B {cell('t')}; the pass is {pass_ms / med['t']:6.3f} x (t), gap {pass_ms - med['t']:10.3f} ms; "
              f"{int(rr.refined.sum().item())} of {B} paths returned re-tracked, {int((rr.repaired != 0).sum().item())} waypoints repaired",
              flush=True)
        prob.close(); cand.close(); nm.close()


if __name__ == "__main__":
    main()
