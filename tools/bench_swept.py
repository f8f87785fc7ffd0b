#!/usr/bin/env python
"""Swept clearance (mkh_swept_clearance) and the checked ladder call (mkh_solve_trajectory_ladder_free): what they cost.

    python tools/bench_swept.py [rounds=7] [parts=abc] [T=64] > profiles/r22_swept.txt

Wall clock around each leg with a device synchronisation at its end; the legs of a part ALTERNATE, `rounds` times after a
warm-up round; reported: the median and the (max - min) of each leg's rounds.
  (a) the sweep against its yardstick, per SAMPLE ROW: N edges of M = 8 samples, device-resident —
        (f) mkh_swept_clearance: reads 2 nq doubles per edge, builds the M rows in LDS
        (m) mkh_clearance on the same N·M rows MATERIALISED beforehand (the interpolation itself is not timed)
      UR5e 14 pairs (four edges / rows per wavefront), G1 46 pairs, ALOHA 1 104 pairs (one per wavefront).  The ends differ in
      hinge and slide joints only, so the materialised rows are a + u (b - a) and (f)'s margin must be the minimum of (m)'s over
      each edge's rows: asserted to 1e-9.
  (b) the checked ladder call against the plain one at the same B, T, S, K: the ladder on K = 8 distinct nodes of S = 16
      solutions per waypoint, M = 8 — UR5e and G1 (g1_c3) at 256 and 4 096 instances, device tensors in and out.  The waypoints
      follow a joint-space line (UR5e: far from `home`, as in the example; G1: from the bench batch's start, as in bench_ladder).
  (c) the checked call against the host composition it replaces, numpy in and out on both sides, UR5e at 256 instances: the
      plain ladder on S = 8 nodes per waypoint with return_all, numpy interpolation of the B·(T-1)·S²·M rows, checker.clearance
      with host arrays on nodes and rows, and the masked dynamic program vectorised in numpy over (s', s).
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

M, S, K = 8, 16, 8
MAX_BATCH = 1 << 20


def cell(ts):
    return f"{np.median(ts):10.3f} [{np.max(ts) - np.min(ts):8.3f}] ms"


def masked_search_fast(start, edges, lost, blocked, max_step_sq=np.inf):
    """tests/ladder_ref.py's search_fast under THE RULE "with a checker": (node_index (T,), lost count)."""
    lost = np.asarray(lost).astype(np.int64)
    T, n = lost.shape
    cnt = lost[0] << 16
    length = np.asarray(start, dtype=np.float64).copy()
    pred = np.zeros((T, n), dtype=np.int64)
    for t in range(1, T):
        c = edges[t]
        cand_cnt = cnt[None, :] + (c > max_step_sq) + ((lost[t][:, None] | blocked[t].astype(np.int64)) << 16)
        cand_len = length[None, :] + c
        lowest = cand_cnt.min(axis=1, keepdims=True)
        masked = np.where(cand_cnt == lowest, cand_len, np.inf)
        shortest = masked.min(axis=1, keepdims=True)
        arg = ((cand_cnt == lowest) & (masked == shortest)).argmax(axis=1)
        rows = np.arange(n)
        cnt, length, pred[t] = cand_cnt[rows, arg], cand_len[rows, arg], arg
    end = int(np.lexsort((np.arange(n), length, cnt))[0])
    path = [end]
    for t in range(T - 1, 0, -1):
        path.append(int(pred[t][path[-1]]))
    return np.array(path[::-1], dtype=np.int32), int(cnt[end] >> 16)


def ladder_workload(nat, workloads, name, B, T):
    """(model, native model, handle, q (B, nq), targets (B, T, n_frame, 7), posture target, dt, damping, iterations, thresholds)."""
    from mink_amd.api_specs import configuration_limit_desc
    rng = np.random.default_rng(1)
    cap = min(B * T * S, MAX_BATCH)
    if name == "ur5e":
        m = workloads.load_robot("ur5e")
        nm = nat.NativeModel(m)
        prob = nat.NativeProblem(nm, frame_tasks=[workloads._frame_desc(m, "attachment_site", "site", 1.0, 1.0, 1.0)],
                                 configuration_limits=[configuration_limit_desc(m)], max_batch=cap)
        lo, hi = np.maximum(m.jnt_range[:, 0], -np.pi), np.minimum(m.jnt_range[:, 1], np.pi)
        first = rng.uniform(lo, hi, size=(B, 1, m.nq))
        last = np.clip(first + rng.normal(scale=0.25, size=(B, 1, m.nq)), lo, hi)
        goal = (first + (last - first) * (np.arange(T)[None, :, None] / max(T - 1, 1))).reshape(B * T, m.nq)
        dummy = np.zeros((B * T, 1, 7)); dummy[:, :, 0] = 1.0
        tg = np.concatenate([prob.solve(goal[i:i + cap], dummy[i:i + cap], None, None, 1.0, 1.0, taps=["frame_pose"],
                                        solve_qp=False)[2]["frame_pose"] for i in range(0, B * T, cap)])
        q = np.tile(m.key_qpos[m.name2id("key", "home")], (B, 1))
        return m, nm, prob, q, tg.reshape(B, T, 1, 7), None, 1.0, 1e-3, 40, (1e-4, 1e-4)
    m = workloads.load_bench_robot(name)
    nm = nat.NativeModel(m)
    prob, dt, damping = workloads.bench_config(name, m, nm, cap)
    q, _, pt, _ = workloads.bench_batch(name, m, nm, prob, rng, B)
    delta = rng.normal(scale=0.15, size=(B, m.nv))                       # (tools/bench_ladder.py's joint-space lines from the start)
    dummy = np.zeros((B, prob.n_frame, 7)); dummy[:, :, 0] = 1.0
    tg = np.stack([prob.solve(nm.integrate(q, delta * ((t + 1) / T), 1.0), dummy, pt, None, 1.0, 1.0, taps=["frame_pose"],
                              solve_qp=False)[2]["frame_pose"] for t in range(T)], axis=1)
    return m, nm, prob, q, np.ascontiguousarray(tg), pt, dt, damping, 20, (1e-3, 1e-2)


def main():
    import torch

    import ladder_ref
    import mink_amd as mink
    from bench_clearance import checker
    from mink_amd import _native as nat
    from mink_amd import workloads

    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    parts = sys.argv[2] if len(sys.argv) > 2 else "abc"
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_swept needs a GPU")
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

    print(f"# tools/bench_swept.py {' '.join(sys.argv[1:])}   ({rounds} alternating rounds; median [max - min]; M = {M} samples per edge)")
    if "a" in parts:
        print("(a) per sample row: (f) the fused sweep, (m) mkh_clearance on the same rows materialised beforehand")
        for name, N in (("ur5e", 65536), ("ur5e", 1 << 18), ("g1", 16384), ("aloha", 2048), ("aloha", 16384)):
            model, ck = checker(mink, workloads, name, max_rows=1 << 20)
            key = {"g1": "stand", "aloha": "neutral_pose"}.get(name)
            base = None if key is None else model.key_qpos[model.name2id("key", key)]
            rng = np.random.default_rng(2)
            a, b = (workloads.sample_q(model, rng, N, base_q=base) for _ in range(2))
            for j in range(model.njnt):                                     # both ends on one quaternion: (m)'s rows are linear blends
                if int(model.jnt_type[j]) in (0, 1):
                    qa = int(model.jnt_qposadr[j]) + (3 if int(model.jnt_type[j]) == 0 else 0)
                    b[:, qa:qa + 4] = a[:, qa:qa + 4]
            u = (np.arange(1, M + 1, dtype=np.float64) / float(M + 1))[None, :, None]
            rows = a[:, None, :] + u * (b - a)[:, None, :]                 # (quaternions of both ends are the base's: b - a = 0 there)
            da, db, drows = to(a), to(b), to(rows.reshape(N * M, model.nq))
            ts = alternate({"f": lambda: ck.swept_clearance(da, db, n_samples=M), "m": lambda: ck.clearance(drows)})
            f, mm = ck.swept_clearance(da, db, n_samples=M), ck.clearance(drows)
            worst = float((f.margin - mm.margin.reshape(N, M).min(dim=1).values).abs().max().item())
            assert worst <= 1e-9, worst
            ns = {k: 1e6 * np.median(v) / (N * M) for k, v in ts.items()}
            print(f"  {name:6s} {ck.n_pairs:5d} pairs {N:7d} edges = {N * M:8d} rows: (f) {cell(ts['f'])} = {ns['f']:7.3f} ns/row   (m) "
                  f"{cell(ts['m'])} = {ns['m']:7.3f} ns/row   (f)/(m) = {ns['f'] / ns['m']:5.3f}   [max |(f) - min (m)| {worst:.1e}; "
                  f"{int(f.in_collision.sum().item())} edges collide]", flush=True)
            ck.close()
    for name, ck_name, B in (("ur5e", "ur5e", 256), ("ur5e", "ur5e", 4096), ("g1_c3", "g1", 256), ("g1_c3", "g1", 4096)):
        if "b" not in parts and "c" not in parts:
            break
        m, nm, prob, q, tg, pt, dt, damping, iters, thr = ladder_workload(nat, workloads, name, B, T)
        _, ck = checker(mink, workloads, ck_name, model=m, max_rows=1 << 20)
        native = ck._native_for(prob)
        kw = dict(n_seeds=S, n_nodes=K, max_iters=iters, pos_threshold=thr[0], ori_threshold=thr[1], rng_seed=3)
        dq, dtg, dpt = to(q), to(tg), to(pt)
        if "b" in parts:
            plain = lambda: prob.solve_trajectory_ladder_nodes(dq, dtg, dpt, None, dt, damping, **kw)
            checked = lambda: prob.solve_trajectory_ladder_free(dq, dtg, dpt, None, dt, damping, checker=native, edge_samples=M, **kw)
            ts = alternate({"p": plain, "c": checked})
            rp, (rc, more) = plain(), checked()
            mp, mc = np.median(ts["p"]), np.median(ts["c"])
            swept = int(((rc.node_seed_index[:, 1:] >= 0).sum().item())) * K * M
            print(f"(b) {name:6s} B={B:5d} T={T} S={S} K={K} ({ck.n_pairs} pairs, loop kernel {prob.last_kernel()}): plain {cell(ts['p'])}   "
                  f"checked {cell(ts['c'])}   added {mc - mp:+9.3f} ms = {100.0 * (mc - mp) / mp:+7.1f} %   [{swept} swept sample rows = "
                  f"{1e6 * (mc - mp) / max(swept, 1):6.3f} ns each; complete paths {int((rp.n_tracked == T).sum().item())} -> "
                  f"{int((rc.n_tracked == T).sum().item())} of {B}; edge collisions on the chosen paths {int(more.n_edge_collisions.sum().item())}]",
                  flush=True)
        if "c" in parts and name == "ur5e" and B <= 256:
            ckw = dict(kw, n_seeds=K)
            del ckw["n_nodes"]

            def the_call():
                return prob.solve_trajectory_ladder_free(q, tg, pt, None, dt, damping, checker=native, edge_samples=M, **ckw)

            def host():
                out = prob.solve_trajectory_ladder(q, tg, pt, None, dt, damping, return_all=True, **ckw)
                nodes = out.q_all                                                        # (B, T, K, nq)
                trk = (out.converged_all != 0) & ((out.status_all & ~1) == 0) & ~ck.clearance(nodes).in_collision
                u = (np.arange(1, M + 1, dtype=np.float64) / float(M + 1))[:, None]
                src, dst = nodes[:, :-1, None, :, None, :], nodes[:, 1:, :, None, None, :]   # (b, t, s', s, i, nq)
                rows = src + u * (dst - src)
                blocked = np.zeros((B, T, K, K), dtype=bool)
                blocked[:, 1:] = ck.clearance(rows).in_collision.any(axis=-1) & trk[:, 1:, :, None]
                path, n_tracked = np.zeros((B, T), np.int32), np.zeros(B, np.int32)
                for i in range(B):
                    start, edges = ladder_ref.costs(m, q[i], nodes[i])
                    path[i], lost = masked_search_fast(start, edges, ~trk[i], blocked[i])
                    n_tracked[i] = T - lost
                return path, n_tracked

            ts = alternate({"c": the_call, "h": host}, n=max(3, rounds // 2))
            (rc, _), (hp, hn) = the_call(), host()
            same = float((hn == rc.n_tracked).mean())
            print(f"(c) {name:6s} B={B:5d} T={T} S={K} (plain ladder), numpy in and out: the checked call {cell(ts['c'])}; host composition "
                  f"{cell(ts['h'])} = {np.median(ts['h']) / np.median(ts['c']):6.1f} x   [same n_tracked on {100 * same:.1f} % of the paths]",
                  flush=True)
        ck.close(); prob.close(); nm.close()


if __name__ == "__main__":
    main()
