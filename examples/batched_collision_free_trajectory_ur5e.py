#!/usr/bin/env python
"""Collision-free candidate tracking: the far Cartesian lines of batched_collision_free_ladder_ur5e.py, floor and wall in the
scene, tracked by `solve_ik_trajectory_multistart` — `--seeds` continuous candidate paths per line, the best one returned —
once as it is, once with `collision_check=`: every waypoint of every candidate is checked on the device behind the loops, the
joint-space motion into every waypoint that still counts is swept (`--edge-samples` interior samples), and the candidate with
the most waypoints that are tracked, free and entered by a free motion wins.  A third step hands the checked result to
`refine_path(..., tracked=res.tracked, collision_check=checker)`, which re-solves the waypoints that did not count from their
neighbours on the path, every repair checked and swept.

    python examples/batched_collision_free_trajectory_ur5e.py --paths 256 [--convex]

With `--convex` the arm is the `ur5e_convex` workload's, whose wrist is a CYLINDER — against the box wall a general convex pair
(GJK, the expanding polytope), held beside the link capsules.  Both calls judge rows they produce themselves, so the checker is
built with `check_rows=` (room for those pairs' distances on that many judged rows: a candidate's node and the samples of the
motion into it) and, for refine_path's sweep of the incoming path, `sweep_rows=`.

UR5e, one FrameTask on `attachment_site` (costs 1 / 1, lm_damping 1), ConfigurationLimit, dt = 1, damping = 1e-3, thresholds
1e-4 / 1e-4, 40 iterations per waypoint, every path started at `home`.  The checker holds every link capsule of the arm against
the floor and the wall.  All results are judged the same way, by `checker.clearance` on the returned waypoints and
`checker.swept_clearance` on the returned motions: a line counts as complete when every waypoint is tracked, and as free when in
addition no waypoint and no motion between waypoints collides.
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
    ap.add_argument("--seeds", type=int, default=64, help="candidate paths per line")
    ap.add_argument("--edge-samples", type=int, default=8)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--min-distance", type=float, default=0.02, help="clearance every capsule keeps from floor and wall (m)")
    ap.add_argument("--rng-seed", type=int, default=5)
    ap.add_argument("--convex", action="store_true", help="the ur5e_convex arm: a cylinder wrist against the box wall (a general convex pair)")
    ap.add_argument("--check-rows", type=int, default=1 << 22, help="with --convex: judged rows the checker holds distances for (8 bytes per "
                    "general convex pair and row; the candidates' rows go in chunks of check_rows // (1 + edge_samples), and chunks cost)")
    ap.add_argument("--sweep-rows", type=int, default=1 << 14, help="with --convex: swept samples the checker holds distances for")
    args = ap.parse_args()
    B, T, S, M = args.paths, args.waypoints, args.seeds, args.edge_samples
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
    checker = mink.CollisionChecker(model, [scene], check_rows=args.check_rows if args.convex else 0,
                                    sweep_rows=args.sweep_rows if args.convex else 0)

    end_effector = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    limits = [mink.ConfigurationLimit(model)]
    configuration = mink.Configuration(model, np.tile(home, (B, 1)))
    track = lambda **extra: mink.solve_ik_trajectory_multistart(
        configuration, [end_effector], 1.0, {end_effector: lines}, S, args.max_iters, pos_threshold=1e-4, ori_threshold=1e-4,
        rng_seed=args.rng_seed, damping=1e-3, limits=limits, update=False, **extra)

    def timed(call):
        call()                                                               # (first call: builds the handles)
        t0 = time.perf_counter()
        out = call()
        return out, 1e3 * (time.perf_counter() - t0)

    plain, ms_plain = timed(track)
    checked, ms_checked = timed(lambda: track(collision_check=checker, edge_samples=M))
    refined, ms_refined = timed(lambda: mink.refine_path(
        configuration, [end_effector], 1.0, {end_effector: lines}, checked.q, tracked=checked.tracked, max_iters=args.max_iters,
        pos_threshold=1e-4, ori_threshold=1e-4, damping=1e-3, limits=limits, update=False, collision_check=checker, edge_samples=M))

    def judge(q, tracked):
        """Per line: complete, and complete + free of node and swept collisions — by the checker alone."""
        nodes_free = ~checker.clearance(q).in_collision
        moves_free = ~checker.swept_clearance(q[:, :-1], q[:, 1:], n_samples=M).in_collision
        complete = tracked.all(axis=1)
        return complete, complete & nodes_free.all(axis=1) & moves_free.all(axis=1), nodes_free, moves_free

    print(f"UR5e{' (cylinder wrist)' if args.convex else ''}, {B} Cartesian lines of {T} waypoints, floor and wall; {S} candidate paths per line, {M} samples per motion:")
    rows = [("plain candidate tracking", plain.q, plain.converged & ((plain.status & ~1) == 0), ms_plain),
            ("with collision_check", checked.q, checked.converged & ((checked.status & ~1) == 0), ms_checked),
            ("... then refine_path", refined.q, refined.tracked, ms_refined)]
    for name, q, tracked, ms in rows:
        complete, free, nodes_free, moves_free = judge(q, tracked)
        print(f"  {name:26s}: {int(complete.sum()):5d} complete, {int(free.sum()):5d} of them free of {B}; {int((~nodes_free).sum()):5d} "
              f"colliding waypoints, {int((~moves_free).sum()):5d} colliding motions   ({ms:.2f} ms)")
    # what the checked call reports is what the checker finds on the returned path
    _, _, nodes_free, moves_free = judge(checked.q, checked.tracked)
    eligible = checked.converged & ((checked.status & ~1) == 0)
    assert nodes_free[eligible].all()
    assert (checked.edge_collision[:, 1:][eligible[:, 1:]] == ~moves_free[eligible[:, 1:]]).all()   # (a motion into a waypoint that does not count is not swept)
    assert (checked.n_tracked == checked.tracked.sum(axis=1)).all()
    assert (refined.n_tracked >= checked.n_tracked).all()                    # the refinement's guard
    print(f"  complete AND free by the calls' own counts: checked {int((checked.n_tracked == T).sum())}, refined "
          f"{int((refined.n_tracked == T).sum())} of {B}; free tracked waypoints {int(checked.n_tracked.sum())} -> "
          f"{int(refined.n_tracked.sum())} of {B * T}; {int(refined.refined.sum())} lines refined, {int((refined.repaired != 0).sum())} "
          f"waypoints repaired")
    if args.convex:
        # what the speculative pre-pass of the general convex pairs evaluated and the check then never read: the samples of the
        # motions into candidate rows that converged and whose node then turned out to collide
        every = track(collision_check=checker, edge_samples=M, return_all=True)
        held = every.converged_all & ((every.status_all & ~(1 | mink.ST_IN_COLLISION)) == 0)
        held[:, :, 0] = False
        read = held & ((every.status_all & mink.ST_IN_COLLISION) == 0)
        n_rows = held.size
        pre, used = n_rows + M * int(held.sum()), n_rows + M * int(read.sum())
        print(f"  general convex pairs: the pre-pass evaluated {pre} rows ({n_rows} nodes, {int(held.sum())} motions of {M} samples), the check "
              f"read {used}: {100.0 * (pre - used) / pre:.1f} % never read")
    checker.close()


if __name__ == "__main__":
    main()
