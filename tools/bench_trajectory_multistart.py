#!/usr/bin/env python
"""Multi-start trajectory IK (mkh_solve_trajectory_multistart): what seeding, fanning out the targets, scoring and gathering
on the device cost next to the bare loops of the same candidates, and next to the host composition the call replaces.

    python tools/bench_trajectory_multistart.py [workloads=ur5e_c2:256:16,ur5e_c2:64:16,g1_c3:256:16,g1_c3:64:16] [rounds=7] [T=64]

Per workload (bench config : B instances : S candidates each; T waypoints along a joint-space line from the bench batch's
start; the threshold-terminated loop, up to 20 steps per waypoint):
  (a) the call, time-major, device tensors in and out, without the candidates' own results: the seed kernel, T x (one fan-out
      launch per batched target group + the loop launch on B·S rows), the score / selection, five gathers
  (b) mkh_solve_trajectory, time-major, on B·S instances: (a)'s own seeds and the targets already repeated S times on the
      device — the T loop launches alone.  It is the yardstick, not the code under test
  (c) the host composition the call replaces: numpy seeds, np.repeat of the targets, solve_ik_trajectory with host arrays on
      B·S instances, a numpy score over the waypoints, argmin and gather
Wall clock around the leg with a device synchronisation at its end, ms per call.  The legs ALTERNATE (a, b, c, a, b, ...),
`rounds` times after a warm-up round; reported: the median and the (max - min) of each leg's rounds.  (a) - (b) per waypoint
is printed next to (b)'s own spread, which is the resolution of the comparison.

Workspace (bytes, include/minkhip.h): (a) without *_all holds T·B·S·((nq + nv)·8 + 12) for the candidates' results; (b) writes
the same number of bytes into the caller's arrays.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_trajectory import MAX_ITERS, THRESHOLDS, public_problem  # noqa: E402


def numpy_seeds(model, q, S, rng):
    """(B, S, nq) on the host: row 0 the caller's q, limited hinges / slides uniform in their range — what a caller draws."""
    out = np.repeat(q[:, None, :], S, axis=1)
    for j in range(model.njnt):
        if model.jnt_type[j] in (2, 3) and model.jnt_limited[j]:
            a = int(model.jnt_qposadr[j])
            out[:, 1:, a] = rng.uniform(model.jnt_range[j, 0], model.jnt_range[j, 1], size=(len(q), S - 1))
    return out


def _qmul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def numpy_difference(model, cur, prev):
    """(..., nv): cur (-) prev in the tangent space, vectorised over the leading axes (mj_differentiatePos at dt = 1)."""
    out = np.zeros(cur.shape[:-1] + (model.nv,))
    for j in range(model.njnt):
        jt, qa, va = int(model.jnt_type[j]), int(model.jnt_qposadr[j]), int(model.jnt_dofadr[j])
        if jt in (2, 3):
            out[..., va] = cur[..., qa] - prev[..., qa]
            continue
        if jt == 0:
            out[..., va:va + 3] = cur[..., qa:qa + 3] - prev[..., qa:qa + 3]
            qa += 3; va += 3
        d = _qmul(prev[..., qa:qa + 4] * np.array([1.0, -1.0, -1.0, -1.0]), cur[..., qa:qa + 4])
        s = np.linalg.norm(d[..., 1:], axis=-1)
        ang = 2.0 * np.arctan2(s, d[..., 0])
        ang = np.where(ang > np.pi, ang - 2.0 * np.pi, ang)
        out[..., va:va + 3] = d[..., 1:] * (ang / np.where(s < 1e-15, 1.0, s))[..., None]
    return out


def numpy_score_select(model, q0, q, converged, status, S):
    """The host's half of the composition: q (B·S, T, nq), converged / status (B·S, T), q0 (B, nq) -> the chosen row of every
    instance by (most tracked waypoints, shortest path from q0, lowest index) and the (B, T, nq) gather."""
    B = len(q0)
    prev = np.concatenate([np.repeat(q0, S, axis=0)[:, None, :], q[:, :-1]], axis=1)
    step = numpy_difference(model, q, prev)
    length = (step * step).sum(axis=(1, 2)).reshape(B, S)
    n = (converged & ((status & ~1) == 0)).sum(axis=1).reshape(B, S)
    key = np.where(n == n.max(axis=1, keepdims=True), np.where(np.isfinite(length), length, np.inf), np.inf)
    pick = np.where(n.max(axis=1) > 0, key.argmin(axis=1), 0)
    return pick, q[np.arange(B) * S + pick]


def main():
    import torch

    import mink_amd as mink
    from mink_amd import _native as nat
    from mink_amd import workloads

    specs = (sys.argv[1] if len(sys.argv) > 1 else "ur5e_c2:256:16,ur5e_c2:64:16,g1_c3:256:16,g1_c3:64:16").split(",")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_trajectory_multistart needs a GPU")
    dev = torch.device("cuda:0")
    print(f"# tools/bench_trajectory_multistart.py {' '.join(sys.argv[1:])}   (T = {T} waypoints, up to {MAX_ITERS} steps each, {rounds} "
          f"alternating rounds; ms per call: median [max - min])", flush=True)
    for spec in specs:
        name, B, S = spec.split(":")
        B, S = int(B), int(S)
        R = B * S
        m = workloads.load_bench_robot(name)
        nm = nat.NativeModel(m)
        prob, dt, damping = workloads.bench_config(name, m, nm, R)
        rng = np.random.default_rng(1)
        q, _, pt, _ = workloads.bench_batch(name, m, nm, prob, rng, B)
        delta = rng.normal(scale=0.15, size=(B, m.nv))
        dummy = np.zeros((B, prob.n_frame, 7)); dummy[:, :, 0] = 1.0
        tg_tm = np.stack([prob.solve(nm.integrate(q, delta * ((t + 1) / T), 1.0), dummy, pt, None, 1.0, 1.0, taps=["frame_pose"],
                                     solve_qp=False)[2]["frame_pose"] for t in range(T)])                 # (T, B, n_frame, 7)
        tg_bm = np.ascontiguousarray(np.swapaxes(tg_tm, 0, 1))
        to = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
        dq, dpt, d_tg = to(q), to(pt), to(tg_tm)
        until = THRESHOLDS[name]
        kw = dict(n_seeds=S, n_steps=MAX_ITERS, pos_threshold=until[0], ori_threshold=until[1], rng_seed=3, time_major=True)
        first = prob.solve_trajectory_multistart(dq, d_tg, dpt, None, dt, damping, return_all=True, **kw)
        d_seeds = first.seeds                                                 # (B·S, nq), on the device
        d_tg_rep = d_tg.repeat_interleave(S, dim=1).contiguous()              # (T, B·S, n_frame, 7): the targets pre-fanned out
        n_bad = int(((first.status_all & ~1) != 0).sum().item())
        ws = T * R * ((m.nq + m.nv) * 8 + 12)
        print(f"{name:8s} B={B:5d} S={S:3d}: workspace of the candidates' results {ws} bytes ({ws / 2 ** 20:.1f} MiB) + starts "
              f"{R * m.nq * 8} + one frame-target slab {R * prob.n_frame * 7 * 8}; (b) reads {T * R * prob.n_frame * 7 * 8} bytes of "
              f"repeated targets the caller holds", flush=True)
        cfg, tasks, frames, post, limits = public_problem(mink, name, m, np.repeat(q, S, axis=0))
        post.set_target(pt[0])
        host_rng = np.random.default_rng(4)

        def leg_a():
            return prob.solve_trajectory_multistart(dq, d_tg, dpt, None, dt, damping, **kw)

        def leg_b():
            return prob.solve_trajectory(d_seeds, d_tg_rep, dpt, None, dt, damping, n_steps=MAX_ITERS, until=until, time_major=True)

        def leg_c():
            seeds = numpy_seeds(m, q, S, host_rng).reshape(R, m.nq)
            seq = np.repeat(tg_bm, S, axis=0)
            cfg.update(seeds)
            res = mink.solve_ik_trajectory(cfg, tasks, dt, {task: seq[:, :, k] for k, task in enumerate(frames)}, n_steps=MAX_ITERS,
                                           damping=damping, limits=limits, update=False, pos_threshold=until[0], ori_threshold=until[1])
            return numpy_score_select(m, q, res.q, res.converged, res.status, S)

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        # (a) picks rows of (b)
        ra, rb = leg_a(), leg_b()
        k_loop = prob.last_kernel()
        rows = torch.arange(B, device=dev) * S + ra.seed_index.long()
        assert torch.equal(ra.q, rb.q[:, rows]) and torch.equal(ra.v, rb.v[:, rows]), "leg (a) is not rows of leg (b)"
        try:
            leg_c()
            run_c = True
        except mink.SolverError as e:                            # (the public call raises on a QP failure of any candidate)
            run_c = False
            print(f"{name:8s} B={B:5d} S={S:3d}: leg (c) not run: {e}", flush=True)
        for fn in (leg_a, leg_b):                                # warm-up round
            wall(fn)
        ts = {k: [] for k in "abc"}
        for r in range(rounds):
            ts["a"].append(wall(leg_a)); ts["b"].append(wall(leg_b))
            if run_c:
                ts["c"].append(wall(leg_c))
        med = {k: float(np.median(v)) if v else float("nan") for k, v in ts.items()}
        spread = {k: float(np.max(v) - np.min(v)) if v else float("nan") for k, v in ts.items()}
        cell = lambda k: f"{med[k]:9.3f} [{spread[k]:7.3f}]"
        done = int((ra.n_tracked == T).sum().item())
        done0 = int(((first.converged_all != 0) & ((first.status_all & ~1) == 0))[:, ::S].all(dim=0).sum().item())
        print(f"{name:8s} B={B:5d} S={S:3d} loop kernel {k_loop}: (a) multi-start call {cell('a')}  (b) bare loops on B·S rows {cell('b')}  "
              f"(c) host composition {cell('c')}  |  (a)-(b) {med['a'] - med['b']:+8.3f} ms = {1e3 * (med['a'] - med['b']) / T:+7.2f} us per "
              f"waypoint against (b)'s spread of {spread['b']:.3f} ms, (c)/(a) {med['c'] / med['a']:6.2f} x  [{n_bad} candidate waypoints "
              f"with a failure bit; complete paths: candidate 0 {done0}, chosen {done} of {B}; picks other than 0: "
              f"{int((ra.seed_index != 0).sum().item())}]", flush=True)
        prob.close(); nm.close()


if __name__ == "__main__":
    main()
