#!/usr/bin/env python
"""Global trajectory IK by multi-start: Cartesian lines whose FIRST pose lies far from the current posture, tracked from one
start (`solve_ik_trajectory`) and from several (`solve_ik_trajectory_multistart`, one call: candidate paths seeded, tracked,
scored over the whole path and chosen on the device).

    python examples/batched_global_trajectory_ur5e.py --paths 256 --seeds 8

UR5e, one FrameTask on `attachment_site` (costs 1 / 1, lm_damping 1), ConfigurationLimit, dt = 1, damping = 1e-3, thresholds
1e-4 / 1e-4, 40 iterations per waypoint, every path started at `home`.  Every path is a straight line of `--waypoints` poses:
the end-effector poses of two configurations — one drawn uniformly in the joint ranges (clipped to ±π), one a small joint step
away — with the translation interpolated linearly and the rotation along the shortest arc between them.  A single start loses
the path when waypoint 0 is out of the local method's reach, or when the branch it lands on runs into a joint limit half-way;
a candidate that tracks the whole line is continuous by construction, and among those the shortest from `home` is returned.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a source checkout
import mink_amd as mink  # noqa: E402


def cartesian_lines(first, last, T):
    """(B, T, 7) wxyz_xyz: T poses from `first` to `last` (both mink.SE3 of B poses), translation and rotation blended apart."""
    u = np.linspace(0.0, 1.0, T)
    a, b = first.wxyz_xyz, last.wxyz_xyz
    step = first.rotation().inverse().multiply(last.rotation()).log()                       # (B, 3) rotation vector a -> b
    out = np.empty((len(a), T, 7))
    for t in range(T):
        out[:, t, :4] = first.rotation().multiply(mink.SO3.exp(u[t] * step)).wxyz
        out[:, t, 4:] = a[:, 4:] + u[t] * (b[:, 4:] - a[:, 4:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--waypoints", type=int, default=16)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--rng-seed", type=int, default=5)
    args = ap.parse_args()
    B, S, T = args.paths, args.seeds, args.waypoints
    rng = np.random.default_rng(20261018)

    model = mink.load_robot("ur5e")
    home = mink.custom_configuration_vector(model, "home")
    lo, hi = np.maximum(model.jnt_range[:, 0], -np.pi), np.minimum(model.jnt_range[:, 1], np.pi)
    q_first = rng.uniform(lo, hi, size=(B, model.nq))
    q_last = np.clip(q_first + rng.normal(scale=0.25, size=(B, model.nq)), lo, hi)
    pose = lambda q: mink.Configuration(model, q).get_transform_frame_to_world("attachment_site", "site")
    lines = cartesian_lines(pose(q_first), pose(q_last), T)

    end_effector = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    tasks, limits = [end_effector], [mink.ConfigurationLimit(model)]
    kw = dict(damping=1e-3, limits=limits, pos_threshold=1e-4, ori_threshold=1e-4, update=False)
    configuration = mink.Configuration(model, np.tile(home, (B, 1)))

    single = mink.solve_ik_trajectory(configuration, tasks, 1.0, {end_effector: lines}, n_steps=args.max_iters, **kw)
    multi = lambda **extra: mink.solve_ik_trajectory_multistart(configuration, tasks, 1.0, {end_effector: lines}, S, args.max_iters,
                                                                 rng_seed=args.rng_seed, **kw, **extra)
    multi()                                                                  # (first call: builds the handle)
    t0 = time.perf_counter()
    res = multi(return_all=True)
    t1 = time.perf_counter()
    tracked1 = single.converged & ((single.status & ~1) == 0)
    print(f"UR5e, {B} Cartesian lines of {T} waypoints whose first pose is far from `home`, at most {args.max_iters} iterations per waypoint:")
    print(f"  single start : {int(tracked1.all(axis=1).sum()):5d} of {B} lines tracked completely, {int(tracked1.sum()):6d} of {B * T} waypoints")
    print(f"  {S:3d} starts   : {int((res.n_tracked == T).sum()):5d} of {B} lines tracked completely, {int(res.n_tracked.sum()):6d} of {B * T} "
          f"waypoints   ({1e3 * (t1 - t0):.2f} ms, numpy in and out)")
    assert (res.n_tracked >= tracked1.sum(axis=1)).all()                     # candidate 0 is the single start
    many = np.flatnonzero(res.n_complete > 1)
    if len(many):
        ok = (res.converged_all & ((res.status_all & ~1) == 0)).all(axis=2)  # (B, S): complete candidates
        first = ok[many].argmax(axis=1)
        print(f"  {len(many)} lines with several complete candidates ({res.n_complete[many].mean():.1f} of {S} on average): the chosen one "
              f"is not the lowest-indexed for {int((res.seed_index[many] != first).sum())} of them")
    # the chosen paths are continuous: the largest joint step between consecutive waypoints of the complete ones
    done = res.n_tracked == T
    if done.any():
        steps = np.abs(np.diff(res.q[done], axis=1)).max()
        end_effector.set_target(mink.SE3(lines[done][:, -1]))
        err = end_effector.compute_error(mink.Configuration(model, res.q[done][:, -1]))
        print(f"  complete paths: largest joint step between waypoints {steps:.3f} rad; worst pose error at the last waypoint: position "
              f"{np.linalg.norm(err[:, :3], axis=1).max():.2e}, orientation {np.linalg.norm(err[:, 3:], axis=1).max():.2e}")


if __name__ == "__main__":
    main()
