#!/usr/bin/env python
"""Trajectory IK (mkh_solve_trajectory): what the one call costs next to the compositions it replaces, and what a waypoint
loop inside the kernels could still win.

    python tools/bench_trajectory.py [workloads=ur5e_c2:64,ur5e_c2:4096,ur5e_c2:65536,g1_c3:64,g1_c3:4096] [rounds=7] [T=64]

Per workload (bench config : B instances, T waypoints each along a joint-space line from the bench batch's start) and mode
(tracking: n_steps = 1, one differential step per waypoint; threshold: the threshold-terminated loop, up to 20 steps):
  (a) the call, time-major, device tensors in and out: the T loop launches read and write the caller's slabs directly
  (b) the call, batch-major, device tensors: the same plus the target transpose in front and the result transposes behind
  (c) a Python loop of NativeProblem.solve per waypoint on device tensors, outputs written into preallocated time-major
      slabs — the fastest way to do the same thing without the entry point
  (d) the public solve_ik_steps loop: Task.set_target + solve_ik_steps per waypoint, numpy arrays over the bus both ways
  (e) the sum over the T loop launches of leg (c) of the HIP-event time around each launch: what the device spends
(a)-(d): wall clock around the leg with a device synchronisation at its end, ms per trajectory call.  The legs ALTERNATE
(a, b, c, d, e, a, b, ...), `rounds` times after a warm-up round; reported: the median and the (max - min) of each leg's
rounds.  (a) - (e) per waypoint is the lead the one-launch-per-waypoint design leaves to a waypoint loop inside the kernels.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

THRESHOLDS = {"ur5e_c2": (1e-3, 1e-2), "g1_c3": (2e-2, 5e-2)}
MAX_ITERS = 20


def public_problem(mink, name, model, q):
    """The bench config's tasks and limits through the public classes: (configuration, tasks, frame tasks, limits)."""
    cfg = mink.Configuration(model, q)
    hinge = {model.jnt_names[j]: np.pi for j in range(model.njnt) if model.jnt_type[j] != 0}
    limits = [mink.ConfigurationLimit(model), mink.VelocityLimit(model, hinge)]
    if name == "ur5e_c2":
        frames = [mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)]
        post = mink.PostureTask(model, cost=1e-2)
    else:
        frames = [mink.FrameTask(s, "site", 200.0, o, lm_damping=1.0)
                  for s, o in (("left_foot", 10.0), ("right_foot", 10.0), ("left_palm", 0.0), ("right_palm", 0.0))]
        post = mink.PostureTask(model, cost=1.0)
    return cfg, frames + [post], frames, post, limits


def main():
    import torch

    import mink_amd as mink
    from mink_amd import _native as nat
    from mink_amd import workloads

    specs = (sys.argv[1] if len(sys.argv) > 1 else "ur5e_c2:64,ur5e_c2:4096,ur5e_c2:65536,g1_c3:64,g1_c3:4096").split(",")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_trajectory needs a GPU")
    dev = torch.device("cuda:0")
    print(f"# tools/bench_trajectory.py {' '.join(sys.argv[1:])}   (T = {T}, {rounds} alternating rounds; ms per trajectory call: "
          f"median [max - min])", flush=True)
    for spec in specs:
        name, B = spec.split(":")
        B = int(B)
        m = workloads.load_bench_robot(name)
        nm = nat.NativeModel(m)
        prob, dt, damping = workloads.bench_config(name, m, nm, B)
        rng = np.random.default_rng(1)
        q, _, pt, _ = workloads.bench_batch(name, m, nm, prob, rng, B)
        delta = rng.normal(scale=0.15, size=(B, m.nv))
        dummy = np.zeros((B, prob.n_frame, 7)); dummy[:, :, 0] = 1.0
        tg_tm = np.stack([prob.solve(nm.integrate(q, delta * ((t + 1) / T), 1.0), dummy, pt, None, 1.0, 1.0, taps=["frame_pose"],
                                     solve_qp=False)[2]["frame_pose"] for t in range(T)])                 # (T, B, n_frame, 7)
        tg_bm = np.ascontiguousarray(np.swapaxes(tg_tm, 0, 1))
        to = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        dq, dpt, d_tm, d_bm = to(q), to(pt), to(tg_tm), to(tg_bm)
        cfg, tasks, frames, post, limits = public_problem(mink, name, m, q)
        post.set_target(pt[0])
        # preallocated time-major slabs of leg (c)
        cq = torch.empty((T, B, m.nq), dtype=torch.float64, device=dev)
        cv = torch.empty((T, B, m.nv), dtype=torch.float64, device=dev)
        cs = torch.empty((T, B), dtype=torch.int32, device=dev)
        for mode, n_steps, until in (("tracking", 1, None), ("threshold", MAX_ITERS, THRESHOLDS[name])):
            thr = {} if until is None else dict(pos_threshold=until[0], ori_threshold=until[1])

            def leg_a():
                return prob.solve_trajectory(dq, d_tm, dpt, None, dt, damping, n_steps=n_steps, until=until, time_major=True)

            def leg_b():
                return prob.solve_trajectory(dq, d_bm, dpt, None, dt, damping, n_steps=n_steps, until=until)

            def leg_c(events=None):
                prev, extra = dq, []
                for t in range(T):
                    if events is not None:
                        events[t][0].record()
                    res = prob.solve(prev, d_tm[t], dpt, None, dt, damping, n_steps=n_steps, until=until, q_out=cq[t], out=cv[t],
                                     status_out=cs[t])
                    if events is not None:
                        events[t][1].record()
                    extra.append(res[3:])
                    prev = cq[t]
                return cq, cv, cs, extra

            def leg_d():
                cfg.update(q)
                qs = []
                for t in range(T):
                    for k, task in enumerate(frames):
                        task.set_target(mink.SE3(tg_tm[t, :, k]))
                    qs.append(mink.solve_ik_steps(cfg, tasks, dt, n_steps, damping=damping, limits=limits, **thr)[0])
                return np.stack(qs, axis=1)

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            def leg_e():
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(T)]
                torch.cuda.synchronize()
                leg_c(ev)
                torch.cuda.synchronize()
                return float(sum(a.elapsed_time(b) for a, b in ev))

            # the legs compute the same thing
            ra, rb, rc = leg_a(), leg_b(), leg_c()
            k_loop = prob.last_kernel()
            assert torch.equal(ra.q, rc[0]) and torch.equal(rb.q, rc[0].transpose(0, 1)), "legs disagree"
            n_bad = int(((ra.status & ~1) != 0).sum().item())
            run_d = n_bad == 0                                   # (the public loop raises SolverError on a QP failure)
            d_dev = float(np.abs(leg_d() - rb.q.cpu().numpy()).max()) if run_d else float("nan")
            conv = "" if until is None else f", {int(ra.converged.sum().item())} of {B * T} waypoints converged"
            for fn in (leg_a, leg_b, leg_c):                     # warm-up round
                wall(fn)
            ts = {k: [] for k in "abcde"}
            for r in range(rounds):
                ts["a"].append(wall(leg_a)); ts["b"].append(wall(leg_b)); ts["c"].append(wall(leg_c))
                if run_d and r < max(3, rounds // 2):            # (the public loop is the slow leg: fewer rounds)
                    ts["d"].append(wall(leg_d))
                ts["e"].append(leg_e())
            med = {k: float(np.median(v)) if v else float("nan") for k, v in ts.items()}
            spread = {k: float(np.max(v) - np.min(v)) if v else float("nan") for k, v in ts.items()}
            cell = lambda k: f"{med[k]:9.3f} [{spread[k]:7.3f}]"
            print(f"{name:8s} B={B:6d} {mode:9s} n_steps={n_steps:2d} loop kernel {k_loop}: (a) time-major {cell('a')}  (b) batch-major "
                  f"{cell('b')}  (c) solve loop {cell('c')}  (d) public loop {cell('d')}  (e) launches, event-timed {cell('e')}  |  "
                  f"(a)-(c) {med['a'] - med['c']:+8.3f} ms, (c)/(a) {med['c'] / med['a']:5.2f} x, (d)/(a) {med['d'] / med['a']:6.1f} x, "
                  f"((a)-(e))/T {1e3 * (med['a'] - med['e']) / T:+7.1f} us per waypoint, (a)/T {1e3 * med['a'] / T:7.1f} us per waypoint, "
                  f"{1e-6 * B * T / (1e-3 * med['a']):8.2f} M waypoints/s  [{n_bad} waypoints with a failure bit{conv}; max |public loop - call| in q {d_dev:.1e}]", flush=True)
        prob.close(); nm.close()


if __name__ == "__main__":
    main()
