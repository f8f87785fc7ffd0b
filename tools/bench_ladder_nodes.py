#!/usr/bin/env python
"""The ladder on deduplicated nodes (mkh_solve_trajectory_ladder_nodes): what the one call costs next to the plain ladder call
and next to the three-call host composition it replaces, what the handle holds after each, and what K distinct nodes out of S
seeds — raw, and unwound to the turn nearest the start — do for the far Cartesian lines of examples/batched_ladder_ur5e.py.

    python tools/bench_ladder_nodes.py [workloads=ur5e_c2:256:16,...] [reps=20] [T=64] [K=8] [noquality] > profiles/r19_ladder_nodes.txt

Time, per workload (bench config : B instances : S seeds per waypoint; T waypoints along a joint-space line from the bench
batch's start, the threshold-terminated loop of tools/bench_ladder.py), device tensors in and out unless said otherwise, HIP
events around the call, median of `reps` (min … max) after a warm-up; every device leg is timed twice, the legs interleaved:
  (f)  the fused call, K nodes out of S seeds per rung, min_distance 0.1
  (fu) the same with unwind_turns
  (a)  the plain ladder call at the same B, T, S — unchanged by this tool's subject, in the same process
  (s)  the search alone on (a)'s S raw nodes per rung (ladder_select), and (sk) on (f)'s K nodes: the search's share of each call
  (d)  the selection alone on (a)'s rungs (select_distinct over the B·T flattened rungs): what (f) adds in front of the search
  (h)  the host composition (f) replaces: solve_trajectory_ladder(return_all) -> select_distinct -> ladder_select with HOST
       arrays — B·T·S rows down, up and the K nodes up once more; wall clock, `reps` / 4 repetitions (one beyond 256 instances)
Workspace: device bytes the handle holds after its first call ((a) and (f) on a fresh handle each): the drop of free device
memory across handle creation and call, less what torch reserved meanwhile for the outputs.  Reported, not asserted on.
Quality (UR5e, 256 far Cartesian lines of 16 waypoints, 40 iterations per waypoint, break: a joint step beyond 1 rad; the
set-up of examples/batched_ladder_ur5e.py): lines complete / complete and break-free for S = 8 raw, S = 64 -> K = 8, the same
with unwinding, and each of the three with refine=True.
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "examples"))

from bench_trajectory import MAX_ITERS, THRESHOLDS  # noqa: E402

DEFAULT = "ur5e_c2:256:16,ur5e_c2:256:64,ur5e_c2:4096:16,ur5e_c2:4096:64,g1_c3:256:16,g1_c3:256:64"
MAX_BATCH = 1 << 20         # loop rows per launch of this tool's handles: larger ladders run in chunks of whole rungs
R = 0.1


def spread(ts):
    return f"{np.median(ts):9.3f} ms ({np.min(ts):.3f} … {np.max(ts):.3f})"


def quality(K):
    import mink_amd as mink
    from batched_global_trajectory_ur5e import cartesian_lines
    from batched_ladder_ur5e import complete_and_break_free

    B, T, max_step = 256, 16, 1.0
    rng = np.random.default_rng(20261018)
    model = mink.load_robot("ur5e")
    home = mink.custom_configuration_vector(model, "home")
    lo, hi = np.maximum(model.jnt_range[:, 0], -np.pi), np.minimum(model.jnt_range[:, 1], np.pi)
    q_first = rng.uniform(lo, hi, size=(B, model.nq))
    q_last = np.clip(q_first + rng.normal(scale=0.25, size=(B, model.nq)), lo, hi)
    pose = lambda q: mink.Configuration(model, q).get_transform_frame_to_world("attachment_site", "site")
    lines = cartesian_lines(pose(q_first), pose(q_last), T)
    task = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    cfg = mink.Configuration(model, np.tile(home, (B, 1)))
    kw = dict(damping=1e-3, limits=[mink.ConfigurationLimit(model)], pos_threshold=1e-4, ori_threshold=1e-4, update=False,
              max_step=max_step, rng_seed=5)
    print(f"# quality: UR5e, {B} far Cartesian lines of {T} waypoints, 40 iterations per waypoint, break: a joint step beyond {max_step} rad "
          f"(examples/batched_ladder_ur5e.py); wall clock of the second call, numpy in and out")
    for label, S, extra in ((f"S = 8 raw", 8, {}), (f"S = 64 raw", 64, {}), (f"S = 64 -> K = {K}", 64, dict(n_nodes=K, min_distance=R)),
                            (f"S = 64 -> K = {K}, unwound", 64, dict(n_nodes=K, min_distance=R, unwind_turns=True)),
                            (f"S = 8 -> K = {K}", 8, dict(n_nodes=K, min_distance=R)),
                            (f"S = 8 -> K = {K}, unwound", 8, dict(n_nodes=K, min_distance=R, unwind_turns=True))):
        for refine in (False, True):
            call = lambda: mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: lines}, S, 40, refine=refine, **kw, **extra)
            call()
            t0 = time.perf_counter(); res = call(); ms = 1e3 * (time.perf_counter() - t0)
            tracked = res.converged & ((res.status & ~1) == 0)
            complete, clean = complete_and_break_free(res.q, tracked, max_step)
            tail = ""
            if "n_nodes" in extra:
                tail = (f"; rungs with uncovered seeds {int((res.n_uncovered > 0).sum())} of {B * T}, distinct nodes per rung "
                        f"{float(res.n_distinct.mean()):.2f}")
            print(f"  {label + (' + refine' if refine else ''):38s}: {int(complete.sum()):4d} complete, {int(clean.sum()):4d} complete and "
                  f"break-free of {B} (first 32 lines: {int(complete[:32].sum())} / {int(clean[:32].sum())}); {int(tracked.sum()):5d} of "
                  f"{B * T} waypoints; breaks on the chosen paths {int(res.n_breaks.sum()):4d}   ({ms:8.2f} ms){tail}", flush=True)


def main():
    import torch

    from mink_amd import _native as nat
    from mink_amd import workloads

    argv = [a for a in sys.argv[1:] if a != "noquality"]
    specs = (argv[0] if len(argv) > 0 else DEFAULT).split(",")
    reps = int(argv[1]) if len(argv) > 1 else 20
    T = int(argv[2]) if len(argv) > 2 else 64
    K = int(argv[3]) if len(argv) > 3 else 8
    if nat.lib().mkh_device_count() < 1:
        raise SystemExit("bench_ladder_nodes needs a GPU")
    dev = torch.device("cuda:0")
    to = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)

    def events(fn, n):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return np.array(ts)

    def held(make, call):
        """Device bytes a fresh handle holds after `call`: free memory lost, less what torch reserved for the outputs."""
        torch.cuda.synchronize()
        free0, res0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
        prob = make()
        out = call(prob)
        torch.cuda.synchronize()
        free1, res1 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
        del out
        return prob, (free0 - free1) - (res1 - res0)

    print(f"# tools/bench_ladder_nodes.py {' '.join(sys.argv[1:])}   (T = {T} waypoints, up to {MAX_ITERS} steps per node, K = {K} nodes, "
          f"min_distance = {R}; median of {reps} (min … max), every device leg timed twice, interleaved)", flush=True)
    for spec in specs:
        name, B, S = spec.split(":")
        B, S = int(B), int(S)
        N = B * T * S
        m = workloads.load_bench_robot(name)
        nm = nat.NativeModel(m)
        small, dt, damping = workloads.bench_config(name, m, nm, B)                # (targets along the line: FK taps on B rows)
        rng = np.random.default_rng(1)
        q, _, pt, _ = workloads.bench_batch(name, m, nm, small, rng, B)
        delta = rng.normal(scale=0.15, size=(B, m.nv))
        dummy = np.zeros((B, small.n_frame, 7)); dummy[:, :, 0] = 1.0
        tg = np.ascontiguousarray(np.stack([small.solve(nm.integrate(q, delta * ((t + 1) / T), 1.0), dummy, pt, None, 1.0, 1.0,
                                                        taps=["frame_pose"], solve_qp=False)[2]["frame_pose"] for t in range(T)], axis=1))
        small.close()
        dq, dpt, d_tg = to(q), to(pt), to(tg)
        until = THRESHOLDS[name]
        kw = dict(n_seeds=S, max_iters=MAX_ITERS, pos_threshold=until[0], ori_threshold=until[1], rng_seed=3)
        nkw = dict(n_nodes=K, min_distance=R)
        make = lambda: workloads.bench_config(name, m, nm, min(N, MAX_BATCH))[0]
        plain, held_a = held(make, lambda p: p.solve_trajectory_ladder(dq, d_tg, dpt, None, dt, damping, **kw))
        prob, held_f = held(make, lambda p: p.solve_trajectory_ladder_nodes(dq, d_tg, dpt, None, dt, damping, **kw, **nkw))
        k_loop = prob.last_kernel()

        first = plain.solve_trajectory_ladder(dq, d_tg, dpt, None, dt, damping, return_all=True, **kw)
        d_nodes = first.q_all
        d_trk = ((first.converged_all != 0) & ((first.status_all & ~1) == 0)).to(torch.int32)
        flat_nodes, flat_trk = d_nodes.reshape(B * T, S, m.nq), d_trk.reshape(B * T, S)
        flat_ref = dq.repeat_interleave(T, dim=0).contiguous()
        n_tracked_a = first.n_tracked.clone()
        del first
        fused = prob.solve_trajectory_ladder_nodes(dq, d_tg, dpt, None, dt, damping, return_all=True, **kw, **nkw)
        k_nodes, k_trk = fused.q_all.clone(), (fused.node_seed_index >= 0).to(torch.int32)
        assert torch.equal(fused.n_tracked, n_tracked_a), "the fused call tracks other waypoints than the plain ladder"
        nd = fused.n_distinct.cpu().numpy().ravel()
        unc = int((fused.n_uncovered > 0).sum().item())
        complete_f = int((fused.n_tracked == T).sum().item())
        del fused

        leg = {"f": lambda: prob.solve_trajectory_ladder_nodes(dq, d_tg, dpt, None, dt, damping, **kw, **nkw),
               "fu": lambda: prob.solve_trajectory_ladder_nodes(dq, d_tg, dpt, None, dt, damping, unwind_turns=True, **kw, **nkw),
               "a": lambda: plain.solve_trajectory_ladder(dq, d_tg, dpt, None, dt, damping, **kw),
               "s": lambda: plain.ladder_select(dq, d_nodes, d_trk),
               "sk": lambda: prob.ladder_select(dq, k_nodes, k_trk),
               "d": lambda: plain.select_distinct(flat_nodes, flat_trk, flat_ref, None, n_solutions=K, min_distance=R)}
        ts = {k: [] for k in leg}
        for _ in range(2):                                         # interleaved: no leg owns a quiet moment of a shared machine
            for k, fn in leg.items():
                ts[k].append(events(fn, reps))
        med = {k: 0.5 * (np.median(v[0]) + np.median(v[1])) for k, v in ts.items()}

        def host():
            o = plain.solve_trajectory_ladder(q, tg, pt, None, dt, damping, return_all=True, **kw)
            ok = (o.converged_all != 0) & ((o.status_all & ~1) == 0)
            sel = plain.select_distinct(np.ascontiguousarray(o.q_all.reshape(B * T, S, m.nq)), ok.reshape(B * T, S), np.repeat(q, T, axis=0),
                                        None, n_solutions=K, min_distance=R)
            return plain.ladder_select(q, sel.q.reshape(B, T, K, m.nq), (sel.seed_index >= 0).reshape(B, T, K))

        th = []
        if N <= (1 << 22):
            host()
            for _ in range(max(3, reps // 4) if B <= 256 else 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); hres = host(); th.append(1e3 * (time.perf_counter() - t0))
            same = np.array_equal(hres.n_tracked, n_tracked_a.cpu().numpy())
            h_line = f"{spread(th)} = {np.median(th) / med['f']:6.1f} x (f)   [tracks the same waypoints: {same}]"
        else:
            h_line = f"not run ({N} rows of q, v, status, iterations and flags over the bus three times)"
        print(f"{name:8s} B={B:5d} S={S:3d} K={K} ({N} loops in {-(-N // prob.max_batch)} launch(es) of kernel {k_loop}):\n"
              f"    (f)  fused call         {spread(ts['f'][0])}   again {spread(ts['f'][1])}\n"
              f"    (fu) fused, unwinding   {spread(ts['fu'][0])}   again {spread(ts['fu'][1])}\n"
              f"    (a)  plain ladder call  {spread(ts['a'][0])}   again {spread(ts['a'][1])}\n"
              f"    (f) / (a) = {med['f'] / med['a']:.3f}   (f) - (a) = {med['f'] - med['a']:+.3f} ms   (fu) - (f) = {med['fu'] - med['f']:+.3f} ms\n"
              f"    (s)  search on S = {S:3d}  {spread(ts['s'][0])}   again {spread(ts['s'][1])} = {100 * med['s'] / med['a']:5.1f} % of (a)\n"
              f"    (sk) search on K = {K:3d}  {spread(ts['sk'][0])}   again {spread(ts['sk'][1])} = {100 * med['sk'] / med['f']:5.1f} % of (f)\n"
              f"    (d)  selection alone    {spread(ts['d'][0])}   again {spread(ts['d'][1])} = {100 * med['d'] / med['f']:5.1f} % of (f); "
              f"(d) + (sk) - (s) = {med['d'] + med['sk'] - med['s']:+.3f} ms\n"
              f"    (h)  host composition   {h_line}\n"
              f"    workspace held by the handle after one call: (a) {held_a / 2 ** 20:9.1f} MiB   (f) {held_f / 2 ** 20:9.1f} MiB   "
              f"[node rows alone: B·T·S·((nq+nv)·8+16) = {N * ((m.nq + m.nv) * 8 + 16) / 2 ** 20:.1f} MiB, "
              f"B·T·K·… = {B * T * K * ((m.nq + m.nv) * 8 + 16) / 2 ** 20:.1f} MiB]\n"
              f"    [distinct nodes per rung 0 … {K}: {np.bincount(nd, minlength=K + 1).tolist()}; rungs with uncovered seeds {unc} of {B * T}; "
              f"complete paths {complete_f} of {B}, the plain ladder's {int((n_tracked_a == T).sum().item())}]", flush=True)
        prob.close(); plain.close(); nm.close()
        del d_nodes, d_trk, flat_nodes, flat_trk, k_nodes, k_trk
        torch.cuda.empty_cache()
    if "noquality" not in sys.argv:
        quality(K)


if __name__ == "__main__":
    main()
