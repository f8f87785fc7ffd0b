#!/usr/bin/env python
"""A Cartesian move for a batch of UR5e arms from TWO poses and a duration: every arm moves its tool from where it is to a
pose 5 cm along x, 10 cm up and 0.4 rad about the tool's own z, in `--duration` seconds, tracked at the control rate.

    python examples/batched_keyframes_ur5e.py --batch 1024 --duration 1.5 --rate 100

`solve_ik_trajectory(..., keyframe_times=..., waypoint_times=...)` takes the two poses as keyframes and interpolates the
T = duration * rate waypoint targets on the device: the straight line between the positions and the shortest arc between the
orientations (rotation and translation apart, not the SE3 screw).  Only the keyframes cross the bus; `return_targets=True`
gives the interpolated path back, here to measure the tracking error against it.
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
    ap.add_argument("--duration", type=float, default=1.5, help="seconds from the first pose to the second")
    ap.add_argument("--rate", type=float, default=100.0, help="control rate in Hz: one waypoint per period")
    args = ap.parse_args()
    B = args.batch
    T = max(1, int(round(args.duration * args.rate)))
    rng = np.random.default_rng(0)

    model = mink.load_robot("ur5e")
    home = mink.custom_configuration_vector(model, "home")
    configuration = mink.Configuration(model, np.tile(home, (B, 1)) + rng.normal(scale=0.05, size=(B, model.nq)))
    tasks = [
        tool := mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0),
        posture := mink.PostureTask(model, cost=1e-2),
    ]
    posture.set_target(home)
    limits = [mink.ConfigurationLimit(model), mink.VelocityLimit(model, {n: np.pi for n in model.jnt_names})]

    # two keyframes per arm: its own tool pose, and that pose moved and turned
    start = configuration.get_transform_frame_to_world("attachment_site", "site")
    turned = start.rotation() @ mink.SO3.from_z_radians(0.4)                          # about the tool's own z
    goal = mink.SE3(np.concatenate([turned.wxyz, start.translation() + np.array([0.05, 0.0, 0.1])], axis=1))
    keyframes = np.stack([start.wxyz_xyz, goal.wxyz_xyz], axis=1)                   # (B, 2, 7)
    keyframe_times = [0.0, args.duration]
    waypoint_times = np.arange(1, T + 1) * (args.duration / T)
    waypoint_times[-1] = args.duration                                               # (inside the keyframes' range, exactly)

    dt = args.duration / T
    kw = dict(n_steps=20, damping=1e-3, limits=limits, pos_threshold=1e-3, ori_threshold=1e-3, keyframe_times=keyframe_times,
              waypoint_times=waypoint_times, waypoint_dt=dt, update=False)
    mink.solve_ik_trajectory(configuration, tasks, dt, {tool: keyframes}, **kw)                           # warm-up
    t0 = time.perf_counter()
    res, path = mink.solve_ik_trajectory(configuration, tasks, dt, {tool: keyframes}, return_targets=True, **kw)
    el = time.perf_counter() - t0
    print(f"{B} arms x {T} waypoints from 2 keyframes in {el * 1e3:.1f} ms: {B * T / el / 1e6:.2f} M waypoints/s; "
          f"{keyframes.nbytes / 1e3:.0f} kB of keyframes instead of {path[tool].nbytes / 1e6:.1f} MB of waypoint targets")
    print(f"converged at {int(res.converged.sum())} of {res.converged.size} waypoints, at most {int(res.iters.max())} iterations; "
          f"largest joint speed {np.abs(res.qvel).max():.2f} rad/s")

    # tracking error along the path: compute_error of the tool task at q[:, t] against the interpolated target of waypoint t
    print("waypoint  time [s]  worst position error [mm]  worst orientation error [mrad]")
    for t in sorted(set(list(range(0, T, max(1, T // 10))) + [T - 1])):
        tool.set_target(mink.SE3(path[tool][:, t]))
        err = tool.compute_error(mink.Configuration(model, res.q[:, t]))
        print(f"{t:8d}  {waypoint_times[t]:8.3f}  {np.linalg.norm(err[:, :3], axis=-1).max() * 1e3:25.3f}  "
              f"{np.linalg.norm(err[:, 3:], axis=-1).max() * 1e3:30.3f}")


if __name__ == "__main__":
    main()
