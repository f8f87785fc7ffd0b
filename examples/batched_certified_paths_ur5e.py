#!/usr/bin/env python
"""Certified paths: the free lines of batched_collision_free_ladder_ur5e.py — complete, free of breaks, free of node collisions and
free of swept collisions at 8 samples per motion — judged once more by `CollisionChecker.certified_sweep`, which picks the sample
count of every motion from a bound on how far it moves the arm's capsules and says whether the space BETWEEN the samples is free
as well.

    python examples/batched_certified_paths_ur5e.py --paths 256

For each `--resolution` (metres a pair of geoms may move against each other between two neighbouring points) it prints how many
of those motions are certified free, undecided and colliding, how many lines are certified along their whole length, and how the
sample counts are distributed.  "Free at 8 samples" is a statement about eight postures; "certified" is one about the motion.  A
motion that ends close to the floor or the wall cannot be certified at a coarse resolution — certification takes margins of
about resolution / 2 at the points — and comes out undecided, not colliding.

The scene, the arm, the task and the ladder call are that example's: UR5e, one FrameTask on `attachment_site`, every link capsule
against the floor and the wall at a minimum distance of 0.02 m, the ladder on 8 distinct unwound nodes of 64 solutions per
waypoint with `collision_check=`.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a source checkout
import mink_amd as mink  # noqa: E402
from batched_global_trajectory_ur5e import cartesian_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--waypoints", type=int, default=16)
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--n-nodes", type=int, default=8)
    ap.add_argument("--edge-samples", type=int, default=8, help="samples per motion of the checked ladder (the sampled statement)")
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--max-step", type=float, default=1.0)
    ap.add_argument("--min-distance", type=float, default=0.02)
    ap.add_argument("--rng-seed", type=int, default=5)
    ap.add_argument("--resolution", type=float, nargs="+", default=[0.01, 0.02, 0.05])
    ap.add_argument("--max-samples", type=int, default=64)
    args = ap.parse_args()
    B, T, S, K, M = args.paths, args.waypoints, args.seeds, args.n_nodes, args.edge_samples
    rng = np.random.default_rng(20261018)

    model = mink.load_robot("ur5e")
    home = mink.custom_configuration_vector(model, "home")
    lo, hi = np.maximum(model.jnt_range[:, 0], -np.pi), np.minimum(model.jnt_range[:, 1], np.pi)
    q_first = rng.uniform(lo, hi, size=(B, model.nq))
    q_last = np.clip(q_first + rng.normal(scale=0.25, size=(B, model.nq)), lo, hi)
    pose = lambda q: mink.Configuration(model, q).get_transform_frame_to_world("attachment_site", "site")
    lines = cartesian_lines(pose(q_first), pose(q_last), T)

    capsules = [g for g in range(model.ngeom) if int(model.geom_type[g]) == 3 and model.geom_valid[g]]
    scene = mink.CollisionAvoidanceLimit(model, [(capsules, ["floor", "wall"])], minimum_distance_from_collisions=args.min_distance,
                                         collision_detection_distance=0.2)
    checker = mink.CollisionChecker(model, [scene])
    end_effector = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    configuration = mink.Configuration(model, np.tile(home, (B, 1)))
    res = mink.solve_ik_trajectory_ladder(
        configuration, [end_effector], 1.0, {end_effector: lines}, S, args.max_iters, pos_threshold=1e-4, ori_threshold=1e-4,
        max_step=args.max_step, rng_seed=args.rng_seed, damping=1e-3, limits=[mink.ConfigurationLimit(model)], update=False,
        n_nodes=K, unwind_turns=True, collision_check=checker, edge_samples=M)

    # the free lines, judged as that example judges them: by the checker alone
    tracked = res.converged & ((res.status & ~1) == 0)
    steps = np.sqrt((np.diff(res.q, axis=1) ** 2).sum(axis=2))
    nodes_free = ~checker.clearance(res.q).in_collision
    moves_free = ~checker.swept_clearance(res.q[:, :-1], res.q[:, 1:], n_samples=M).in_collision
    free = tracked.all(axis=1) & (steps <= args.max_step).all(axis=1) & nodes_free.all(axis=1) & moves_free.all(axis=1)
    paths = res.q[free]
    print(f"UR5e, {B} Cartesian lines of {T} waypoints, floor and wall: {int(free.sum())} lines free at {M} samples per motion, "
          f"{len(paths) * (T - 1)} motions")
    if not len(paths):
        checker.close()
        return
    reach = checker.motion_reach()
    print(f"  reach of the {checker.n_pairs} pairs per joint (m / rad): {np.array2string(reach[..., 1].max(axis=0), precision=2)}")
    for resolution in args.resolution:
        out = checker.certified_sweep(paths[:, :-1], paths[:, 1:], resolution, max_samples=args.max_samples)
        n = out.n_samples.ravel()
        q = np.percentile(n, [0, 25, 50, 75, 100]).astype(int)
        whole = out.certified.all(axis=1)
        print(f"  resolution {resolution:5.3f} m: {int(out.certified.sum()):5d} certified, {int((out.verdict == 0).sum()):5d} undecided, "
              f"{int(out.in_collision.sum()):5d} colliding motions; {int(whole.sum()):4d} lines certified whole; n_samples min / quartiles / max "
              f"{q[0]} / {q[1]} {q[2]} {q[3]} / {q[4]}, {int(out.capped.sum())} capped, {int(n.sum() + 2 * n.size)} points in all "
              f"(against {M * n.size} samples of the fixed sweep)")
        # a certified motion is free at the fixed sweep's samples too, and nothing the fixed sweep found free at its ends collides there
        assert not (out.certified & ~moves_free[free]).any()
        assert (out.lower_bound <= out.margin + 1e-12)[np.isfinite(out.lower_bound)].all()
    checker.close()


if __name__ == "__main__":
    main()
