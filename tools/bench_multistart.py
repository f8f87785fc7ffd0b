#!/usr/bin/env python
"""Multi-start IK (mkh_solve_multistart): what the one call costs next to the loop it wraps and to the host composition it replaces.

    python tools/bench_multistart.py [workloads=ur5e:65536,ur5e:1048576,g1_c3:65536] [reps=20] [seeds=16]

Per workload (robot : B·S instances, S seeds per target), median of `reps` after warm-up:
  (i)   one call   NativeProblem.solve_multistart with device-resident inputs and outputs: seed kernel, target fan-out, the
                   threshold loop, selection — HIP events around the call
  (ii)  bare loop  NativeProblem.solve(n_steps=, until=) on the same B·S pre-seeded instances with the targets already repeated
                   on the device: the mkh_solve_until launch alone, unchanged kernels — HIP events around the call
  (iii) host       what a caller writes without the entry point: numpy seeds, np.repeat of the targets, the loop with numpy in
                   and out (B·S rows over the bus both ways), numpy selection — wall clock (the call is synchronous)
UR5e: the far-target set-up of examples/batched_global_ik_ur5e.py (one FrameTask, ConfigurationLimit, dt 1, damping 1e-3,
40 iterations, thresholds 1e-4).  g1_c3: the bench workload (targets 0.15 rad away), 20 iterations, thresholds 1e-3 / 1e-2.
Also printed: the bytes the seed, fan-out and selection kernels move, and (i) − (ii) as a share of (ii).
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def draw_host_seeds(m, q, S, rng):
    """Host seeding as a user would write it: uniform in the ranges of limited hinges / slides, the rest kept; row 0 = q."""
    out = np.repeat(q[:, None, :], S, axis=1)
    for j in range(m.njnt):
        if m.jnt_type[j] in (2, 3) and m.jnt_limited[j]:
            lo, hi = m.jnt_range[j]
            out[:, 1:, int(m.jnt_qposadr[j])] = rng.uniform(lo, hi, size=(len(q), S - 1))
    return out


def host_select(q_all, q0, conv, status):
    """argmin over the converged, failure-free seeds of |q − q0|² (hinge / slide coordinates; a free base is the same in every seed)."""
    d = ((q_all - q0[:, None, :]) ** 2).sum(axis=2)
    d = np.where((conv != 0) & ((status & ~1) == 0), d, np.inf)
    best = np.argmin(d, axis=1)
    best[~np.isfinite(d.min(axis=1))] = 0
    return best


def workload(nat, workloads, name, N, S):
    from mink_amd.api_specs import configuration_limit_desc
    B = N // S
    rng = np.random.default_rng(1)
    if name == "ur5e":
        m = workloads.load_robot("ur5e")
        nm = nat.NativeModel(m)
        prob = nat.NativeProblem(nm, frame_tasks=[workloads._frame_desc(m, "attachment_site", "site", 1.0, 1.0, 1.0)],
                                 configuration_limits=[configuration_limit_desc(m)], max_batch=N)
        lo, hi = np.maximum(m.jnt_range[:, 0], -np.pi), np.minimum(m.jnt_range[:, 1], np.pi)
        goal = rng.uniform(lo, hi, size=(B, m.nq))
        dummy = np.zeros((B, 1, 7)); dummy[:, :, 0] = 1.0
        _, _, t = prob.solve(goal, dummy, None, None, 1.0, 1.0, taps=["frame_pose"], solve_qp=False)
        q = np.tile(m.key_qpos[m.name2id("key", "home")], (B, 1))
        return m, nm, prob, (q, t["frame_pose"], None, None), 1.0, 1e-3, 40, (1e-4, 1e-4)
    m = workloads.load_bench_robot(name)
    nm = nat.NativeModel(m)
    prob, dt, damping = workloads.bench_config(name, m, nm, N)
    q, tg, pt, ct = workloads.bench_batch(name, m, nm, prob, rng, B)
    return m, nm, prob, (q, tg, pt, ct), dt, damping, 20, (1e-3, 1e-2)


def main():
    import torch

    from mink_amd import _native as nat
    from mink_amd import workloads

    specs = (sys.argv[1] if len(sys.argv) > 1 else "ur5e:65536,ur5e:1048576,g1_c3:65536").split(",")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    S = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_multistart needs a GPU")
    dev = torch.device("cuda:0")
    print(f"# tools/bench_multistart.py {' '.join(sys.argv[1:])}   (median of {reps}, S = {S})")
    for spec in specs:
        name, N = spec.split(":")
        N = int(N)
        B = N // S
        m, nm, prob, (q, tg, pt, ct), dt, damping, iters, thr = workload(nat, workloads, name, N, S)
        to = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)
        rep = lambda x, per: None if x is None else (np.repeat(x, S, axis=0) if x.ndim == per + 1 else x)
        dq, dtg, dpt, dct = to(q), to(tg), to(pt), to(ct)
        kw = dict(n_seeds=S, max_iters=iters, pos_threshold=thr[0], ori_threshold=thr[1], rng_seed=0)
        first = prob.solve_multistart(dq, dtg, dpt, dct, dt, damping, return_all=True, **kw)
        seeds = first.seeds.reshape(N, m.nq).contiguous()
        rtg, rpt, rct = to(rep(tg, 2)), to(rep(pt, 2)), to(rep(ct, 2))

        def one_call():
            return prob.solve_multistart(dq, dtg, dpt, dct, dt, damping, **kw)

        def bare_loop():
            return prob.solve(seeds, rtg, rpt, rct, dt, damping, n_steps=iters, until=thr)

        def events(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); fn(); b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            return float(np.median(ts)), float(np.min(ts))

        # alternate the two device legs so that neither owns a quiet moment of a shared machine
        t_i, lo_i = events(one_call)
        k_loop = prob.last_kernel()
        t_ii, lo_ii = events(bare_loop)
        t_i2, lo_i2 = events(one_call)
        t_ii2, lo_ii2 = events(bare_loop)
        t_i, t_ii = 0.5 * (t_i + t_i2), 0.5 * (t_ii + t_ii2)
        rng = np.random.default_rng(2)

        def host():
            hs = draw_host_seeds(m, q, S, rng).reshape(N, m.nq)
            qa, _, st, _, cv = prob.solve(hs, rep(tg, 2), rep(pt, 2), rep(ct, 2), dt, damping, n_steps=iters, until=thr)
            best = host_select(qa.reshape(B, S, m.nq), q, cv.reshape(B, S), st.reshape(B, S))
            return qa.reshape(B, S, m.nq)[np.arange(B), best]

        host(); host()
        th = []
        for _ in range(max(5, reps // 4)):
            t0 = time.perf_counter(); host(); th.append(1e3 * (time.perf_counter() - t0))
        t_iii = float(np.median(th))
        res = one_call()
        n_conv = int(res.converged.sum().item())
        single = int(first.converged_all[:, 0].sum().item())
        moved = 8 * (2 * N * m.nq + 2 * N * tg.shape[1] * 7 + N * (m.nq + m.nv)) + 12 * N       # seed w, fan-out r+w, select r
        print(f"{name:8s} B*S={N:8d} (B={B}, S={S}) loop kernel {k_loop}: (i) one call {t_i:8.3f} ms  (ii) bare loop {t_ii:8.3f} ms  "
              f"(i)-(ii) {t_i - t_ii:+7.3f} ms = {100.0 * (t_i - t_ii) / t_ii:+5.1f} %  (iii) host composition {t_iii:9.2f} ms "
              f"= {t_iii / t_i:5.1f} x (i)   [{1e-6 * B / (1e-3 * t_i):.2f} M targets/s one call; fastest (i) {min(lo_i, lo_i2):.3f} "
              f"(ii) {min(lo_ii, lo_ii2):.3f}; seed+fan-out+select traffic ~{moved / 1e6:.1f} MB; converged targets {n_conv} of {B}, "
              f"seed 0 alone {single}]", flush=True)
        prob.close(); nm.close()


if __name__ == "__main__":
    main()
