#!/usr/bin/env python
"""Collision-free global IK: multi-start whose picks are checked against the scene on the device — a seed that ends with a link
through the floor or the wall is not eligible, and the closest of the free ones wins (`collision_check=`).

    python examples/batched_collision_free_ik_ur5e.py --targets 1024 --seeds 16

UR5e, one FrameTask on `attachment_site` (costs 1 / 1, lm_damping 1), ConfigurationLimit, dt = 1, damping = 1e-3, thresholds
1e-4 / 1e-4, 40 iterations, every loop from `home`.  The targets are the end-effector poses of collision-free configurations drawn
in the joint ranges, so each has at least one free solution.  The checker holds every link capsule of the arm against the floor
and the wall (`--min-distance`, default 20 mm).  Printed: how many of the plain picks collide, how many of the checked ones, and
what the check costs.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a source checkout
import mink_amd as mink  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--min-distance", type=float, default=0.02)
    ap.add_argument("--rng-seed", type=int, default=0)
    args = ap.parse_args()
    B, S = args.targets, args.seeds

    model = mink.load_robot("ur5e")
    capsules = [g for g in range(model.ngeom) if int(model.geom_type[g]) == 3 and model.geom_valid[g]]
    scene = mink.CollisionAvoidanceLimit(model, [(capsules, ["floor", "wall"])], minimum_distance_from_collisions=args.min_distance,
                                         collision_detection_distance=0.2)
    checker = mink.CollisionChecker(model, [scene])

    # targets: poses of free configurations (drawn until B of them are free)
    rng = np.random.default_rng(20261020)
    lo, hi = np.maximum(model.jnt_range[:, 0], -np.pi), np.minimum(model.jnt_range[:, 1], np.pi)
    drawn = rng.uniform(lo, hi, size=(4 * B, model.nq))
    free = drawn[~checker.clearance(drawn).in_collision][:B]
    if len(free) < B:
        raise SystemExit(f"only {len(free)} of {4 * B} drawn configurations are free")
    targets = mink.Configuration(model, free).get_transform_frame_to_world("attachment_site", "site")

    end_effector = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    end_effector.set_target(targets)
    tasks, limits = [end_effector], [mink.ConfigurationLimit(model)]
    home = mink.custom_configuration_vector(model, "home")
    configuration = mink.Configuration(model, np.tile(home, (B, 1)))
    call = lambda check: mink.solve_ik_multistart(configuration, tasks, 1.0, S, args.max_iters, 1e-4, 1e-4, damping=1e-3, limits=limits,
                                                  rng_seed=args.rng_seed, update=False, collision_check=check)
    out, ms = {}, {}
    for name, check in (("plain", None), ("checked", checker)):
        call(check)                                                          # (first call: builds the handles)
        t0 = time.perf_counter()
        out[name] = call(check)
        ms[name] = 1e3 * (time.perf_counter() - t0)
    print(f"UR5e, {B} targets, {S} starts per target from `home`, {checker.n_pairs} geom pairs (numpy in and out):")
    for name in ("plain", "checked"):
        r = out[name]
        c = checker.clearance(r.q)
        hit = c.in_collision & r.converged
        print(f"  {name:8s} {ms[name]:8.2f} ms: {int(r.converged.sum())} of {B} converged, {int(hit.sum())} of them in collision"
              + (f" (worst margin {c.margin[hit].min() * 1e3:.1f} mm)" if hit.any() else "")
              + f"; eligible seeds per target: median {int(np.median(r.n_converged))}")
    lost = out["plain"].converged & ~out["checked"].converged
    moved = out["plain"].converged & out["checked"].converged & (out["plain"].seed_index != out["checked"].seed_index)
    print(f"  the check moved {int(moved.sum())} picks to another seed and left {int(lost.sum())} targets without a free solution "
          f"among their {S} seeds")
    pair, count = np.unique(checker.clearance(out["plain"].q).pair[checker.clearance(out["plain"].q).in_collision], return_counts=True)
    names = lambda k: " x ".join(model.geom_names[g] or f"geom {g}" for g in checker.geom_id_pairs[k])
    print("  what the plain picks hit: " + ", ".join(f"{names(k)}: {n}" for k, n in zip(pair, count)))
    checker.close()


if __name__ == "__main__":
    main()
