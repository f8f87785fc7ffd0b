#!/usr/bin/env python
"""Collision-free ladder paths: the far Cartesian lines of batched_ladder_ur5e.py with the floor and a wall in the scene, tracked
by the ladder on 8 distinct unwound nodes per waypoint — once as it is, once with `collision_check=`: every IK solution is
checked on the device behind its loop, every joint-space motion between consecutive nodes is swept (`--edge-samples` interior
samples), and the dynamic program picks the path whose waypoints AND motions are free.

    python examples/batched_collision_free_ladder_ur5e.py --paths 256 [--refine] [--convex]

With `--refine` a third call adds `refine="free"`: behind the checked search the refinement pass re-solves lost waypoints, breaks
and waypoints entered through collision from their neighbours on the path, every repair checked as a node and the motions on
both sides of it swept, on the device.

With `--convex` the arm is the `ur5e_convex` workload's: its wrist is a CYLINDER, and a cylinder against the box wall has no
analytic distance routine — a general convex pair (GJK, the expanding polytope).  The checker then holds the wrist beside the
link capsules and is built with `sweep_rows=`: room for those pairs' distances at that many swept samples, which is what lets
the checked ladder sweep such a checker's motions (in chunks of sweep_rows // edge_samples edges).  Together with `--refine`
it is also built with `check_rows=`: room for those pairs' distances on the rows the refinement pass judges inside its own
launches — a repaired node and the samples of the two motions beside it, 1 + 2 edge_samples rows per line and step.

UR5e, one FrameTask on `attachment_site` (costs 1 / 1, lm_damping 1), ConfigurationLimit, dt = 1, damping = 1e-3, thresholds
1e-4 / 1e-4, 40 iterations per waypoint, every path started at `home`.  The checker holds every link capsule of the arm against
the floor and the wall.  Both results are judged the same way, by `checker.clearance` on the returned waypoints and
`checker.swept_clearance` on the returned motions: a line counts when it is complete (every waypoint tracked), free of breaks
(no joint step beyond `--max-step`), free of node collisions and free of swept collisions.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a source checkout
import mink_amd as mink  # noqa: E402
from batched_global_trajectory_ur5e import cartesian_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--waypoints", type=int, default=16)
    ap.add_argument("--seeds", type=int, default=64, help="IK solutions per waypoint the nodes are picked from")
    ap.add_argument("--n-nodes", type=int, default=8)
    ap.add_argument("--edge-samples", type=int, default=8)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--max-step", type=float, default=1.0, help="joint-space step between waypoints that counts as a break (rad)")
    ap.add_argument("--min-distance", type=float, default=0.02, help="clearance every capsule keeps from floor and wall (m)")
    ap.add_argument("--rng-seed", type=int, default=5)
    ap.add_argument("--refine", action="store_true", help='also run the checked call with refine="free"')
    ap.add_argument("--convex", action="store_true", help="the ur5e_convex arm: a cylinder wrist against the box wall (a general convex pair)")
    ap.add_argument("--sweep-rows", type=int, default=1 << 16, help="with --convex: swept samples the checker holds distances for")
    ap.add_argument("--check-rows", type=int, default=1 << 14, help="with --convex --refine: judged rows the checker holds distances for")
    args = ap.parse_args()
    B, T, S, K, M = args.paths, args.waypoints, args.seeds, args.n_nodes, args.edge_samples
    rng = np.random.default_rng(20261018)

    if args.convex:
        from mink_amd import workloads
        model = workloads.load_bench_robot("ur5e_convex")
    else:
        model = mink.load_robot("ur5e")
    home = mink.custom_configuration_vector(model, "home")
    lo, hi = np.maximum(model.jnt_range[:, 0], -np.pi), np.minimum(model.jnt_range[:, 1], np.pi)
    q_first = rng.uniform(lo, hi, size=(B, model.nq))
    q_last = np.clip(q_first + rng.normal(scale=0.25, size=(B, model.nq)), lo, hi)
    pose = lambda q: mink.Configuration(model, q).get_transform_frame_to_world("attachment_site", "site")
    lines = cartesian_lines(pose(q_first), pose(q_last), T)

    capsules = [g for g in range(model.ngeom) if int(model.geom_type[g]) == 3 and model.geom_valid[g]]
    pairs = [(capsules, ["floor", "wall"])] if capsules else []
    if args.convex:
        pairs.append((["wrist_3_link"], ["floor", "wall"]))                  # (its cylinder: analytic against the floor, GJK against the wall)
    scene = mink.CollisionAvoidanceLimit(model, pairs, minimum_distance_from_collisions=args.min_distance,
                                         collision_detection_distance=0.2)
    checker = mink.CollisionChecker(model, [scene], sweep_rows=args.sweep_rows if args.convex else 0,
                                    check_rows=args.check_rows if args.convex and args.refine else 0)

    end_effector = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    configuration = mink.Configuration(model, np.tile(home, (B, 1)))
    ladder = lambda **extra: mink.solve_ik_trajectory_ladder(
        configuration, [end_effector], 1.0, {end_effector: lines}, S, args.max_iters, pos_threshold=1e-4, ori_threshold=1e-4,
        max_step=args.max_step, rng_seed=args.rng_seed, damping=1e-3, limits=[mink.ConfigurationLimit(model)], update=False,
        n_nodes=K, unwind_turns=True, **extra)

    def timed(call):
        call()                                                               # (first call: builds the handles)
        t0 = time.perf_counter()
        out = call()
        return out, 1e3 * (time.perf_counter() - t0)

    plain, ms_plain = timed(ladder)
    checked, ms_checked = timed(lambda: ladder(collision_check=checker, edge_samples=M))
    rows = [("plain ladder", plain, ms_plain), ("with collision_check", checked, ms_checked)]
    if args.refine:
        refined, ms_refined = timed(lambda: ladder(collision_check=checker, edge_samples=M, refine="free"))
        rows.append(('... and refine="free"', refined, ms_refined))

    def judge(res):
        """Per line: complete, + free of breaks, + free of node collisions, + free of swept collisions — by the checker alone."""
        tracked = res.converged & ((res.status & ~1) == 0)
        steps = np.sqrt((np.diff(res.q, axis=1) ** 2).sum(axis=2))
        nodes_free = ~checker.clearance(res.q).in_collision
        moves_free = ~checker.swept_clearance(res.q[:, :-1], res.q[:, 1:], n_samples=M).in_collision
        complete = tracked.all(axis=1)
        clean = complete & (steps <= args.max_step).all(axis=1)
        still = clean & nodes_free.all(axis=1)
        return complete, clean, still, still & moves_free.all(axis=1), nodes_free, moves_free

    print(f"UR5e{' (cylinder wrist)' if args.convex else ''}, {B} Cartesian lines of {T} waypoints, floor and wall; the ladder on {K} distinct unwound nodes of {S} solutions per "
          f"waypoint, {M} samples per motion:")
    for name, res, ms in rows:
        complete, clean, still, free, nodes_free, moves_free = judge(res)
        print(f"  {name:22s}: {int(complete.sum()):5d} complete, {int(clean.sum()):5d} + free of breaks, {int(still.sum()):5d} + free of "
              f"node collisions, {int(free.sum()):5d} + free of swept collisions of {B}; {int((~nodes_free).sum()):5d} colliding waypoints, "
              f"{int((~moves_free).sum()):5d} colliding motions   ({ms:.2f} ms)")
    # what the checked call reports is what the checker finds on the returned path
    _, _, _, _, nodes_free, moves_free = judge(checked)
    tracked = checked.converged & ((checked.status & ~1) == 0)
    # (an empty slot of a rung with fewer than n_nodes distinct free solutions holds candidate 0's rows and is not a node)
    tracked &= np.take_along_axis(checked.node_seed_index, checked.node_index[..., None], axis=2)[..., 0] >= 0
    assert nodes_free[tracked].all()
    entered = tracked[:, 1:]                                                 # (a motion into a lost waypoint is not swept)
    assert (checked.edge_collision[:, 1:][entered] == ~moves_free[entered]).all()
    assert (checked.n_tracked == (tracked & ~checked.edge_collision).sum(axis=1)).all()
    if args.refine:
        # the guard: no line comes back with fewer free tracked waypoints than the checked search found
        assert (refined.n_tracked >= checked.n_tracked).all()
        print(f"  refined {int(refined.refined.sum())} of {B} lines, {int((refined.repaired != 0).sum())} waypoints repaired; free tracked "
              f"waypoints {int(checked.n_tracked.sum())} -> {int(refined.n_tracked.sum())} of {B * T}")
    checker.close()


if __name__ == "__main__":
    main()
