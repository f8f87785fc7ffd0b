#!/usr/bin/env python
"""Keyframed trajectory IK (mkh_solve_keyframes): what interpolating the waypoint targets on the device costs next to the
trajectory call on targets that are already there, and next to the composition it replaces.

    python tools/bench_keyframes.py [workloads=ur5e_c2:64,ur5e_c2:4096,g1_c3:64,g1_c3:4096] [rounds=7] [T=64]

Per workload (bench config : B instances; K = T / 16 keyframes along a joint-space line from the bench batch's start, uniform
key times, T waypoints at uniform times up to the last keyframe) and mode (tracking: n_steps = 1; threshold: the
threshold-terminated loop, up to 20 steps):
  (a) the keyframed call, time-major, device tensors in and out: T x (one small interpolation launch + the loop launch)
  (b) mkh_solve_trajectory, time-major, on (a)'s own interpolated targets held on the device: the T loop launches alone
  (c) the composition the call replaces: a vectorised numpy interpolation of the keyframes on the host (slerp + lerp), then
      solve_ik_trajectory with host arrays
Wall clock around the leg with a device synchronisation at its end, ms per call.  The legs ALTERNATE (a, b, c, a, b, ...),
`rounds` times after a warm-up round; reported: the median and the (max - min) of each leg's rounds.  (a) - (b) is the cost
of the T small launches; it is printed next to (b)'s own spread, which is the resolution of the comparison.

Target workspace (bytes, from the sizes the handle's buffers are grown to — minkhip.hip, trajectory_core): (a) holds one
(B, n_frame, 7) slab whatever T is and reads B·K poses of the caller's; (b) time-major holds nothing but reads B·T poses of
the caller's; (b) batch-major would hold a transposed copy of those B·T poses.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_trajectory import MAX_ITERS, THRESHOLDS, public_problem  # noqa: E402


def _qmul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def numpy_interpolate(keys, key_times, waypoint_times):
    """(B, K, n, 7) -> (B, T, n, 7) on the host, vectorised over instances and tasks: the shortest-arc slerp of the rotations
    and the lerp of the translations — what a caller of solve_ik_trajectory writes today."""
    kt, wt = np.asarray(key_times), np.asarray(waypoint_times)
    k = np.clip(np.searchsorted(kt, wt, side="right") - 1, 0, len(kt) - 2)
    u = ((wt - kt[k]) / (kt[k + 1] - kt[k]))[None, :, None, None]
    a, b = keys[:, k], keys[:, k + 1]                                       # (B, T, n, 7)
    d = _qmul(a[..., :4] * np.array([1.0, -1.0, -1.0, -1.0]), b[..., :4])
    d = np.where(d[..., :1] < 0.0, -d, d)
    s = np.linalg.norm(d[..., 1:], axis=-1, keepdims=True)
    ang = 2.0 * np.arctan2(s, d[..., :1])
    axis = d[..., 1:] / np.where(s < 1e-12, 1.0, s)
    h = 0.5 * u * ang
    q = _qmul(a[..., :4], np.concatenate([np.cos(h), np.sin(h) * axis], axis=-1))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([q, a[..., 4:] + u * (b[..., 4:] - a[..., 4:])], axis=-1))


def main():
    import torch

    import mink_amd as mink
    from mink_amd import _native as nat
    from mink_amd import workloads

    specs = (sys.argv[1] if len(sys.argv) > 1 else "ur5e_c2:64,ur5e_c2:4096,g1_c3:64,g1_c3:4096").split(",")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    K = max(2, T // 16)
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_keyframes needs a GPU")
    dev = torch.device("cuda:0")
    print(f"# tools/bench_keyframes.py {' '.join(sys.argv[1:])}   (K = {K} keyframes, T = {T} waypoints, {rounds} alternating rounds; "
          f"ms per call: median [max - min])", flush=True)
    kt = np.linspace(0.0, 1.0, K)
    wt = np.linspace(0.0, 1.0, T + 1)[1:]
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
        keys_tm = np.stack([prob.solve(nm.integrate(q, delta * (k / (K - 1)), 1.0), dummy, pt, None, 1.0, 1.0, taps=["frame_pose"],
                                       solve_qp=False)[2]["frame_pose"] for k in range(K)])               # (K, B, n_frame, 7)
        keys_bm = np.ascontiguousarray(np.swapaxes(keys_tm, 0, 1))
        to = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        dq, dpt, d_keys = to(q), to(pt), to(keys_tm)
        cfg, tasks, frames, post, limits = public_problem(mink, name, m, q)
        post.set_target(pt[0])
        f8 = 8 * prob.n_frame * 7
        print(f"{name:8s} B={B:6d} target workspace of the handle / targets the caller holds [bytes]: (a) {B * f8} / {B * K * f8}   "
              f"(b) time-major 0 / {B * T * f8}   (b) batch-major {B * T * f8} / {B * T * f8}", flush=True)
        for mode, n_steps, until in (("tracking", 1, None), ("threshold", MAX_ITERS, THRESHOLDS[name])):
            thr = {} if until is None else dict(pos_threshold=until[0], ori_threshold=until[1])
            first = prob.solve_keyframes(dq, kt, wt, d_keys, dpt, None, dt, damping, n_steps=n_steps, until=until, time_major=True,
                                         return_targets=True)
            d_targets = first.frame_targets                                  # (T, B, n_frame, 7), on the device

            def leg_a():
                return prob.solve_keyframes(dq, kt, wt, d_keys, dpt, None, dt, damping, n_steps=n_steps, until=until,
                                            time_major=True).trajectory

            def leg_b():
                return prob.solve_trajectory(dq, d_targets, dpt, None, dt, damping, n_steps=n_steps, until=until, time_major=True)

            def leg_c():
                cfg.update(q)
                seq = numpy_interpolate(keys_bm, kt, wt)
                return mink.solve_ik_trajectory(cfg, tasks, dt, {task: seq[:, :, k] for k, task in enumerate(frames)},
                                                n_steps=n_steps, damping=damping, limits=limits, update=False, **thr)

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0)

            # the legs compute the same thing
            ra, rb = leg_a(), leg_b()
            k_loop = prob.last_kernel()
            assert torch.equal(ra.q, rb.q) and torch.equal(ra.v, rb.v), "legs (a) and (b) disagree"
            d_interp = float(np.abs(numpy_interpolate(keys_bm, kt, wt) - d_targets.transpose(0, 1).cpu().numpy()).max())
            n_bad = int(((ra.status & ~1) != 0).sum().item())
            run_c = n_bad == 0                                   # (the public call raises SolverError on a QP failure)
            d_c = float(np.abs(leg_c().q - ra.q.transpose(0, 1).cpu().numpy()).max()) if run_c else float("nan")
            conv = "" if until is None else f", {int(ra.converged.sum().item())} of {B * T} waypoints converged"
            for fn in (leg_a, leg_b):                            # warm-up round
                wall(fn)
            ts = {k: [] for k in "abc"}
            for r in range(rounds):
                ts["a"].append(wall(leg_a)); ts["b"].append(wall(leg_b))
                if run_c:
                    ts["c"].append(wall(leg_c))
            med = {k: float(np.median(v)) if v else float("nan") for k, v in ts.items()}
            spread = {k: float(np.max(v) - np.min(v)) if v else float("nan") for k, v in ts.items()}
            cell = lambda k: f"{med[k]:9.3f} [{spread[k]:7.3f}]"
            print(f"{name:8s} B={B:6d} {mode:9s} n_steps={n_steps:2d} loop kernel {k_loop}: (a) keyframed {cell('a')}  (b) trajectory on "
                  f"device targets {cell('b')}  (c) numpy + host arrays {cell('c')}  |  (a)-(b) {med['a'] - med['b']:+8.3f} ms = "
                  f"{1e3 * (med['a'] - med['b']) / T:+7.2f} us per waypoint against (b)'s spread of {spread['b']:.3f} ms, "
                  f"(c)/(a) {med['c'] / med['a']:6.2f} x  [{n_bad} waypoints with a failure bit{conv}; max |numpy - device| in the "
                  f"targets {d_interp:.1e}, max |(c) - (a)| in q {d_c:.1e}]", flush=True)
        prob.close(); nm.close()


if __name__ == "__main__":
    main()
