#!/usr/bin/env python
"""Goal sets: a batch of objects, each with `--goals` candidate approach poses, and for every object the pose the arm reaches
with the configuration closest to `home` — which of the poses are within reach, and the best of them, in one call
(`solve_ik_goalset`), picked on the device.

    python examples/batched_goalset_ur5e.py --targets 1024 --goals 8 --seeds 4

UR5e, one FrameTask on `attachment_site` (costs 1 / 1, lm_damping 1), ConfigurationLimit, dt = 1, damping = 1e-3, thresholds
1e-4 / 1e-4, 40 iterations, every loop from `home`.  Object b sits at a random position around the base; its approach pose —
the tool's z axis horizontal, pointing at the object from `--standoff` metres away — is rotated about the world z axis through
the object in `--goals` equal steps from a random first yaw: a tool that may come from any side.  Printed: how many objects the
first pose alone reaches, how many the set reaches, and which poses were chosen.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a source checkout
import mink_amd as mink  # noqa: E402


def qmul(a, b):
    """Hamilton product of wxyz quaternions, broadcasting."""
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def approach_poses(objects, yaw0, G, standoff):
    """(B, G, 7) wxyz_xyz: the pose that looks along +x at the object from `standoff` away, rotated about the world z axis
    through the object by yaw0[b] + 2π g / G."""
    yaw = yaw0[:, None] + 2.0 * np.pi * np.arange(G)[None, :] / G
    about_z = np.stack([np.cos(0.5 * yaw), np.zeros_like(yaw), np.zeros_like(yaw), np.sin(0.5 * yaw)], axis=-1)
    z_to_x = np.array([np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0])              # tool z → world x
    back = -standoff * np.stack([np.cos(yaw), np.sin(yaw), np.zeros_like(yaw)], axis=-1)
    return np.concatenate([qmul(about_z, z_to_x), objects[:, None, :] + back], axis=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--goals", type=int, default=8)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--standoff", type=float, default=0.1)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--rng-seed", type=int, default=0)
    args = ap.parse_args()
    B, G, S = args.targets, args.goals, args.seeds

    model = mink.load_robot("ur5e")
    home = mink.custom_configuration_vector(model, "home")
    rng = np.random.default_rng(20261020)
    radius, bearing = rng.uniform(0.35, 0.75, size=B), rng.uniform(-np.pi, np.pi, size=B)
    objects = np.stack([radius * np.cos(bearing), radius * np.sin(bearing), rng.uniform(0.1, 0.6, size=B)], axis=1)
    goals = approach_poses(objects, rng.uniform(-np.pi, np.pi, size=B), G, args.standoff)

    end_effector = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    end_effector.set_target(mink.SE3(goals[:, 0]))
    tasks, limits = [end_effector], [mink.ConfigurationLimit(model)]
    configuration = mink.Configuration(model, np.tile(home, (B, 1)))
    call = lambda: mink.solve_ik_goalset(configuration, tasks, 1.0, {end_effector: goals}, S, args.max_iters, 1e-4, 1e-4,
                                         damping=1e-3, limits=limits, rng_seed=args.rng_seed, update=False)
    call()                                                                   # (first call: builds the handle)
    t0 = time.perf_counter()
    res = call()
    ms = 1e3 * (time.perf_counter() - t0)
    print(f"UR5e, {B} objects, {G} approach poses each, {S} starts per pose from `home` ({ms:.2f} ms, numpy in and out):")
    print(f"  reached by pose 0 alone: {int(res.reached[:, 0].sum())} of {B}; by the set: {int(res.converged.sum())}")
    print(f"  poses within reach per object (0 … {G}): {np.bincount(res.n_reached, minlength=G + 1).tolist()}")
    print(f"  chosen pose (goal_index 0 … {G - 1}): {np.bincount(res.goal_index[res.converged], minlength=G).tolist()}")
    chosen = np.flatnonzero(res.converged)
    end_effector.set_target(mink.SE3(goals[chosen, res.goal_index[chosen]]))
    err = end_effector.compute_error(mink.Configuration(model, res.q[chosen]))
    print(f"  worst pose error of the chosen configurations against their chosen poses: position "
          f"{np.linalg.norm(err[:, :3], axis=1).max():.2e}, orientation {np.linalg.norm(err[:, 3:], axis=1).max():.2e}")
    away = np.sqrt(res.score[chosen])
    print(f"  joint-space distance from `home` to the chosen configuration: median {np.median(away):.2f} rad, max {away.max():.2f}")


if __name__ == "__main__":
    main()
