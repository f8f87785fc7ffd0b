#!/usr/bin/env python
"""Distinct IK solution sets: the far targets of batched_global_ik_ur5e.py, every one solved from many starts, and instead of
the one result closest to `home` up to `--solutions` DIFFERENT converged results per target — the IK branches multi-start
found, deduplicated on the device (`solve_ik_solutions`, one call).

    python examples/batched_solution_sets_ur5e.py --targets 1024 --seeds 16 --solutions 8

UR5e, one FrameTask on `attachment_site` (costs 1 / 1, lm_damping 1), ConfigurationLimit, dt = 1, damping = 1e-3, thresholds
1e-4 / 1e-4, 40 iterations, every loop from `home`; two results within `--min-distance` (rad, Euclidean in joint space) are the
same solution.  Printed: how many distinct solutions the targets have and how many seeds a solution stands for.

Then the composition with the ladder search, on the far Cartesian lines of batched_ladder_ur5e.py: the waypoints of all lines
solved as B·T independent targets, their K deduplicated solutions reshaped to (B, T, K, nq) rungs for `ladder_path`, next to
`solve_ik_trajectory_ladder`, which searches all S loop results of every waypoint.  The composition stays here as an
illustration of the two calls; `solve_ik_trajectory_ladder(..., n_nodes=K)` does the same in one call on the device, without
the B·T·S rows crossing the bus (examples/batched_ladder_ur5e.py --n-nodes).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a source checkout
import mink_amd as mink  # noqa: E402
from batched_global_trajectory_ur5e import cartesian_lines  # noqa: E402
from batched_ladder_ur5e import complete_and_break_free  # noqa: E402


def timed(call):
    call()                                                                   # (first call: builds the handle)
    t0 = time.perf_counter()
    out = call()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--solutions", type=int, default=8)
    ap.add_argument("--min-distance", type=float, default=0.1)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--rng-seed", type=int, default=0)
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--waypoints", type=int, default=16)
    ap.add_argument("--max-step", type=float, default=1.0, help="joint-space step between waypoints that counts as a break (rad)")
    args = ap.parse_args()
    B, S, K = args.targets, args.seeds, args.solutions

    model = mink.load_robot("ur5e")
    home = mink.custom_configuration_vector(model, "home")
    lo, hi = np.maximum(model.jnt_range[:, 0], -np.pi), np.minimum(model.jnt_range[:, 1], np.pi)
    pose = lambda q: mink.Configuration(model, q).get_transform_frame_to_world("attachment_site", "site")
    end_effector = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    tasks, limits = [end_effector], [mink.ConfigurationLimit(model)]
    kw = dict(damping=1e-3, limits=limits, rng_seed=args.rng_seed)

    # ---- the solutions of far targets
    end_effector.set_target(pose(np.random.default_rng(20261016).uniform(lo, hi, size=(B, model.nq))))
    configuration = mink.Configuration(model, np.tile(home, (B, 1)))
    sets, ms = timed(lambda: mink.solve_ik_solutions(configuration, tasks, 1.0, S, K, args.max_iters, 1e-4, 1e-4,
                                                     min_distance=args.min_distance, **kw))
    one = mink.solve_ik_multistart(configuration, tasks, 1.0, S, args.max_iters, 1e-4, 1e-4, update=False, **kw)
    assert np.array_equal(sets.q[:, 0], one.q) and np.array_equal(sets.valid[:, 0], one.converged)   # slot 0 is multi-start's
    print(f"UR5e, {B} far targets, {S} starts each from `home`, at most {K} solutions {args.min_distance} rad apart ({ms:.2f} ms, numpy in and out):")
    print(f"  distinct solutions per target (0 … {K}): {np.bincount(sets.n_distinct, minlength=K + 1).tolist()}; "
          f"{int((sets.n_uncovered > 0).sum())} targets have more than {K}")
    mult = sets.multiplicity[sets.valid]
    print(f"  converged seeds a solution stands for (1 … {int(mult.max()) if len(mult) else 0}): {np.bincount(mult)[1:].tolist()}; "
          f"{int(sets.n_converged.sum())} converged seeds in {int(sets.valid.sum())} solutions")
    flat = mink.Configuration(model, sets.q[sets.valid])
    end_effector.set_target(mink.SE3(np.repeat(end_effector.transform_target_to_world.wxyz_xyz, K, axis=0).reshape(B, K, 7)[sets.valid]))
    err = end_effector.compute_error(flat)
    print(f"  worst pose error over all solutions: position {np.linalg.norm(err[:, :3], axis=1).max():.2e}, "
          f"orientation {np.linalg.norm(err[:, 3:], axis=1).max():.2e}")

    # ---- the sets as the rungs of a ladder
    P, T = args.paths, args.waypoints
    rng = np.random.default_rng(20261018)
    q_first = rng.uniform(lo, hi, size=(P, model.nq))
    q_last = np.clip(q_first + rng.normal(scale=0.25, size=(P, model.nq)), lo, hi)
    lines = cartesian_lines(pose(q_first), pose(q_last), T)                 # (P, T, 7)
    line_start = mink.Configuration(model, np.tile(home, (P, 1)))
    end_effector.set_target(mink.SE3(np.ascontiguousarray(lines.reshape(P * T, 7))))
    waypoints = mink.Configuration(model, np.tile(home, (P * T, 1)))
    rungs, ms_sets = timed(lambda: mink.solve_ik_solutions(waypoints, tasks, 1.0, S, K, args.max_iters, 1e-4, 1e-4,
                                                           min_distance=args.min_distance, **kw))
    nodes, tracked = rungs.q.reshape(P, T, K, model.nq), rungs.valid.reshape(P, T, K)
    few, ms_few = timed(lambda: mink.ladder_path(line_start, nodes, tracked, max_step=args.max_step))
    full, ms_full = timed(lambda: mink.solve_ik_trajectory_ladder(line_start, tasks, 1.0, {end_effector: lines}, S, args.max_iters, 1e-4, 1e-4,
                                                                  max_step=args.max_step, update=False, return_all=True, **kw))
    full_trk = full.converged_all & ((full.status_all & ~1) == 0)
    _, ms_search = timed(lambda: mink.ladder_path(line_start, full.q_all, full_trk, max_step=args.max_step))
    print(f"UR5e, {P} far Cartesian lines of {T} waypoints; a break is a joint step beyond {args.max_step} rad:")
    for name, q, trk, ms in ((f"solution sets ({K} nodes per waypoint) + ladder_path", few.q, np.take_along_axis(tracked, few.node_index[..., None], 2)[..., 0], ms_sets + ms_few),
                             (f"solve_ik_trajectory_ladder ({S} nodes per waypoint)", full.q, full.converged & ((full.status & ~1) == 0), ms_full)):
        complete, clean = complete_and_break_free(q, trk, args.max_step)
        print(f"  {name:58s}: {int(complete.sum()):5d} complete, {int(clean.sum()):5d} complete and break-free of {P}   ({ms:.2f} ms)")
    print(f"  the search alone, numpy in and out: {ms_few:.2f} ms on {K} nodes per waypoint, {ms_search:.2f} ms on {S}")
    assert (few.n_tracked == full.n_tracked).all()                           # a waypoint with a converged seed keeps slot 0


if __name__ == "__main__":
    main()
