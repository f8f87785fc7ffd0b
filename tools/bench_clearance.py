#!/usr/bin/env python
"""Clearance (mkh_clearance) and the collision check behind multi-start's loops: what they cost.

    python tools/bench_clearance.py [reps=20] [seeds=16] [parts=abc]

Median of `reps` after warm-up with the spread (min … max); device legs are timed with HIP events on device-resident inputs and
outputs, twice, interleaved with their counterpart, and both medians are printed.
  (a) mkh_clearance alone: a checker of 65 536 rows per launch (CollisionChecker's default), rows drawn by workloads.sample_q —
      UR5e, its 14 link capsules against floor and wall, at 4 096 / 65 536 / 1 048 576 rows; G1, the 46 pairs of
      workloads.g1_collision_pairs, at 65 536; `ur5e_convex` (wrist cylinder against floor and wall: the general convex routine
      in a kernel of its own in front) at 65 536; ALOHA's 1 104 pairs at 16 384.
  (b) NativeProblem.solve_multistart with and without `collision_check=` on the same B·S instances (tools/bench_multistart.py's
      workloads): UR5e 4 096 × S and 65 536 × S, G1 (g1_c3) 4 096 × S.
  (c) the checked call against the host composition it replaces, numpy in and out on both sides (wall clock): return_all down,
      clearance of the B·S rows with host arrays, then the selection in numpy (squared differences of qpos).
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def spread(ts):
    return f"{np.median(ts):9.3f} ms ({np.min(ts):.3f} … {np.max(ts):.3f})"


def checker(mink, workloads, name, model=None, max_rows=65536):
    """(model, CollisionChecker) of one of the bench's pair lists; `model`: the robot as the caller already loaded it."""
    if name in ("ur5e", "ur5e_convex"):
        model = model or (workloads.load_bench_robot("ur5e_convex") if name == "ur5e_convex" else workloads.load_robot("ur5e"))
        if name == "ur5e":
            caps = [g for g in range(model.ngeom) if int(model.geom_type[g]) == 3 and model.geom_valid[g]]
            lim = mink.CollisionAvoidanceLimit(model, [(caps, ["floor", "wall"])], minimum_distance_from_collisions=0.02,
                                               collision_detection_distance=0.2)
        else:
            lim = mink.CollisionAvoidanceLimit(model, [(["wrist_3_link"], ["floor", "wall"])], minimum_distance_from_collisions=0.05,
                                               collision_detection_distance=0.3)
    elif name == "g1":
        model = model or workloads.load_robot("g1")
        lim = mink.CollisionAvoidanceLimit(model, [([a], [b]) for a, b in workloads.g1_collision_pairs(model)],
                                           minimum_distance_from_collisions=0.06, collision_detection_distance=0.25)
    elif name == "aloha":
        model = model or workloads.load_robot("aloha")
        sub = lambda b: mink.get_subtree_geom_ids(model, model.name2id("body", b))
        frame = mink.get_body_geom_ids(model, model.name2id("body", "metal_frame"))
        lim = mink.CollisionAvoidanceLimit(model, [(sub("left/wrist_link"), sub("right/wrist_link")),
                                                   (sub("left/upper_arm_link") + sub("right/upper_arm_link"), frame + ["table"])],
                                           minimum_distance_from_collisions=0.05, collision_detection_distance=0.1)
    else:
        raise KeyError(name)
    return model, mink.CollisionChecker(model, [lim], max_rows=max_rows)


def main():
    import torch

    import mink_amd as mink
    from bench_multistart import workload
    from mink_amd import _native as nat
    from mink_amd import workloads

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    parts = sys.argv[3] if len(sys.argv) > 3 else "abc"
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_clearance needs a GPU")
    dev = torch.device("cuda:0")
    to = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)

    def events(fn, n=reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return np.array(ts)

    print(f"# tools/bench_clearance.py {' '.join(sys.argv[1:])}   (median of {reps} (min … max), S = {S})")
    if "a" in parts:
        print("(a) mkh_clearance alone, device-resident rows, 65 536 rows per launch")
        for name, N in (("ur5e", 4096), ("ur5e", 65536), ("ur5e", 1 << 20), ("g1", 65536), ("ur5e_convex", 65536), ("aloha", 16384)):
            model, ck = checker(mink, workloads, name)
            key = {"g1": "stand", "aloha": "neutral_pose"}.get(name)
            base = None if key is None else model.key_qpos[model.name2id("key", key)]
            q = to(workloads.sample_q(model, np.random.default_rng(2), N, base_q=base))
            run = lambda: ck.clearance(q)
            t1, t2 = events(run), events(run)
            out = run()
            med = 0.5 * (np.median(t1) + np.median(t2))
            print(f"  {name:12s} {ck.n_pairs:5d} pairs {N:8d} rows: {spread(t1)}   again {spread(t2)}   = {1e3 * med / N:8.4f} us/row "
                  f"[{int(out.in_collision.sum().item())} rows in collision]", flush=True)
            ck.close()
    for name, ck_name, B in (("ur5e", "ur5e", 4096), ("ur5e", "ur5e", 65536), ("g1_c3", "g1", 4096)):
        if "b" not in parts and "c" not in parts:
            break
        N = B * S
        m, nm, prob, (q, tg, pt, ct), dt, damping, iters, thr = workload(nat, workloads, name, N, S)
        _, ck = checker(mink, workloads, ck_name, model=m)
        kw = dict(n_seeds=S, max_iters=iters, pos_threshold=thr[0], ori_threshold=thr[1], rng_seed=0)
        dq, dtg, dpt, dct = to(q), to(tg), to(pt), to(ct)
        plain = lambda: prob.solve_multistart(dq, dtg, dpt, dct, dt, damping, **kw)
        checked = lambda: prob.solve_multistart(dq, dtg, dpt, dct, dt, damping, collision_check=ck, **kw)
        if "b" in parts:
            t_p, t_c, t_p2, t_c2 = events(plain), events(checked), events(plain), events(checked)
            mp, mc = 0.5 * (np.median(t_p) + np.median(t_p2)), 0.5 * (np.median(t_c) + np.median(t_c2))
            a, b = plain(), checked()
            print(f"(b) {name:6s} B={B:6d} x S={S} ({N} loops, {ck.n_pairs} pairs, loop kernel {prob.last_kernel()}):\n"
                  f"    plain    {spread(t_p)}   again {spread(t_p2)}\n"
                  f"    checked  {spread(t_c)}   again {spread(t_c2)}\n"
                  f"    added {mc - mp:+8.3f} ms = {100.0 * (mc - mp) / mp:+6.1f} %   [converged {int(a.converged.sum().item())} -> "
                  f"{int(b.converged.sum().item())} of {B}; eligible seeds {int(a.n_converged.sum().item())} -> "
                  f"{int(b.n_converged.sum().item())}]", flush=True)
        if "c" in parts and B <= 4096:
            def the_call():
                return prob.solve_multistart(q, tg, pt, ct, dt, damping, collision_check=ck, **kw)

            def host():
                out = prob.solve_multistart(q, tg, pt, ct, dt, damping, return_all=True, **kw)
                free = ~ck.clearance(out.q_all.reshape(N, m.nq)).in_collision.reshape(B, S)
                ok = (out.converged_all != 0) & ((out.status_all & ~1) == 0) & free
                d = np.where(ok, ((out.q_all - q[:, None, :]) ** 2).sum(axis=2), np.inf)
                s = d.argmin(axis=1)
                return np.where(ok.any(axis=1), s, 0), ok.any(axis=1)

            def wall(fn, n=max(5, reps // 4)):
                fn(); fn()
                ts = []
                for _ in range(n):
                    t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
                return np.array(ts)

            t_call, t_host = wall(the_call), wall(host)
            res, (hs, hc) = the_call(), host()
            agree = float(((hs == res.seed_index) & (hc == (res.converged != 0))).mean())
            print(f"(c) {name:6s} B={B:6d} x S={S}, numpy in and out: the checked call {spread(t_call)}; host composition "
                  f"{spread(t_host)} = {np.median(t_host) / np.median(t_call):5.1f} x   [same choice on {100 * agree:.1f} % of the targets]",
                  flush=True)
        ck.close(); prob.close(); nm.close()


if __name__ == "__main__":
    main()
