#!/usr/bin/env python
"""Motion tracking for a batch of G1 instances in ONE call: the task set of mink's examples/humanoid_g1.py (:13-94) — pelvis
orientation, posture, CoM, feet and palm frame tasks with configuration limits — with both palms tracing closed curves
over T frames, a different size and phase per instance.

    python examples/batched_trajectory_g1.py --batch 1024 --frames 120

`solve_ik_trajectory` takes the whole (B, T, 7) target sequences, runs one differential-IK step per frame (tracking mode,
n_steps = 1) from where the previous frame ended, and returns every frame's configuration; nothing crosses the bus between
frames.  The tracking error of a frame is Task.compute_error at that frame's configuration.
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--fps", type=float, default=60.0, help="frame rate of the clip: waypoint_dt = 1 / fps")
    args = ap.parse_args()
    B, T = args.batch, args.frames
    rng = np.random.default_rng(0)

    model = mink.load_robot("g1")
    stand = mink.custom_configuration_vector(model, "stand")
    configuration = mink.Configuration(model, np.tile(stand, (B, 1)))

    feet, hands = ["right_foot", "left_foot"], ["right_palm", "left_palm"]
    tasks = [
        pelvis := mink.FrameTask("pelvis", "body", position_cost=0.0, orientation_cost=10.0),
        posture := mink.PostureTask(model, cost=1.0),
        com := mink.ComTask(cost=200.0),
    ]
    feet_tasks = [mink.FrameTask(f, "site", position_cost=200.0, orientation_cost=10.0, lm_damping=1.0) for f in feet]
    hand_tasks = [mink.FrameTask(h, "site", position_cost=200.0, orientation_cost=0.0, lm_damping=1.0) for h in hands]
    tasks += feet_tasks + hand_tasks
    limits = [mink.ConfigurationLimit(model)]

    # held targets: everything but the hands stays where it is
    posture.set_target_from_configuration(configuration)
    pelvis.set_target_from_configuration(configuration)
    com.set_target_from_configuration(configuration)
    for t in feet_tasks:
        t.set_target_from_configuration(configuration)

    # the clip: each palm on an ellipse in a tilted plane through its start pose — radius, tilt and phase per instance
    phase = 2.0 * np.pi * (np.arange(1, T + 1) / T)[None, :]                      # (1, T): the curve closes at frame T
    targets = {}
    for side, task in zip((-1.0, 1.0), hand_tasks):
        pose = configuration.get_transform_frame_to_world(task.frame_name, task.frame_type).wxyz_xyz      # (B, 7)
        radius = rng.uniform(0.03, 0.10, size=(B, 1))
        tilt = rng.uniform(-0.5, 0.5, size=(B, 1))
        ph = phase + rng.uniform(0.0, 2.0 * np.pi, size=(B, 1))
        ph0 = ph[:, :1] - phase[:, :1]                                            # the curve passes through the start pose
        seq = np.repeat(pose[:, None, :], T, axis=1)
        seq[:, :, 4] += 0.5 * radius * (np.cos(ph) - np.cos(ph0))
        seq[:, :, 5] += side * radius * np.cos(tilt) * (np.sin(ph) - np.sin(ph0))
        seq[:, :, 6] += radius * np.sin(tilt) * (np.sin(ph) - np.sin(ph0)) + 0.5 * radius * (np.cos(ph) - np.cos(ph0))
        targets[task] = seq

    dt, damping = 1.0 / args.fps, 1e-1
    mink.solve_ik_trajectory(configuration, tasks, dt, targets, n_steps=1, damping=damping, limits=limits, update=False)   # warm-up
    t0 = time.perf_counter()
    res = mink.solve_ik_trajectory(configuration, tasks, dt, targets, n_steps=1, damping=damping, limits=limits,
                                   waypoint_dt=dt, update=False)
    el = time.perf_counter() - t0
    print(f"{B} instances x {T} frames in {el * 1e3:.1f} ms: {B * T / el / 1e6:.2f} M frames/s, {T / el:.0f} clip frames/s per call "
          f"(host arrays in and out)")

    # tracking error per frame: compute_error of the hand tasks at q[:, t] against frame t's targets
    err = np.zeros((T, B))
    for t in range(T):
        cfg_t = mink.Configuration(model, res.q[:, t])
        for task in hand_tasks:
            task.set_target(mink.SE3(targets[task][:, t]))
            err[t] = np.maximum(err[t], np.linalg.norm(task.compute_error(cfg_t)[:, :3], axis=-1))
    print("frame   worst [mm]  median [mm]   (palm position error; one IK step per frame lags the target by about a frame)")
    for t in sorted(set(list(range(0, T, max(1, T // 12))) + [T - 1])):
        print(f"{t:5d}   {err[t].max() * 1e3:9.2f}   {np.median(err[t]) * 1e3:10.2f}")
    print(f"all frames: worst {err.max() * 1e3:.2f} mm, median {np.median(err) * 1e3:.2f} mm; "
          f"largest joint speed between frames {np.abs(res.qvel[:, :, 6:]).max():.2f} rad/s")


if __name__ == "__main__":
    main()
