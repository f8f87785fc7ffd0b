#!/usr/bin/env python
"""Global IK by multi-start: targets FAR from the current posture, where the local method stops at a joint limit or a
singularity for a good share of them, solved from many starts per target with the best solution picked on the device —
`solve_ik_multistart`, one call.

    python examples/batched_global_ik_ur5e.py --targets 1024 --seeds 16

UR5e, one FrameTask on `attachment_site` (costs 1 / 1, lm_damping 1), ConfigurationLimit, dt = 1, damping = 1e-3, thresholds
1e-4 / 1e-4, 40 iterations; every target is the end-effector pose of a configuration drawn uniformly in the joint ranges
(clipped to ±π), every loop starts at `home`.  Printed: how many targets converge from the single start (`solve_ik_steps`)
and from `--seeds` starts (seed 0 is the single start, so multi-start never converges fewer), and how far the chosen
solutions are from `home` next to the first converged seed's.

    python examples/batched_global_ik_ur5e.py --targets 256 --seeds 4 --seed-table 4096

`--seed-table N` also builds a `SeedTable` of N postures drawn around `home`, keyed on the site pose each one reaches, and
solves once more with seeds 1 … S − 1 taken from the table's entries nearest to each target: converged counts for random and
for table seeds at the same S.
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
    ap.add_argument("--rng-seed", type=int, default=0)
    ap.add_argument("--seed-table", type=int, default=0, metavar="N", help="also solve with seeds from a table of N stored postures")
    args = ap.parse_args()
    B, S = args.targets, args.seeds
    rng = np.random.default_rng(20261016)

    model = mink.load_robot("ur5e")
    home = mink.custom_configuration_vector(model, "home")
    lo, hi = np.maximum(model.jnt_range[:, 0], -np.pi), np.minimum(model.jnt_range[:, 1], np.pi)
    goal = mink.Configuration(model, rng.uniform(lo, hi, size=(B, model.nq)))
    end_effector = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    end_effector.set_target(goal.get_transform_frame_to_world("attachment_site", "site"))
    tasks, limits = [end_effector], [mink.ConfigurationLimit(model)]
    dt, damping, pos_thr, ori_thr = 1.0, 1e-3, 1e-4, 1e-4

    configuration = mink.Configuration(model, np.tile(home, (B, 1)))
    _, _, _, single = mink.solve_ik_steps(configuration, tasks, dt, args.max_iters, damping=damping, limits=limits, update=False,
                                          pos_threshold=pos_thr, ori_threshold=ori_thr)
    mink.solve_ik_multistart(configuration, tasks, dt, S, args.max_iters, pos_thr, ori_thr, damping=damping, limits=limits,
                             rng_seed=args.rng_seed, update=False)          # (first call: builds the handle)
    t0 = time.perf_counter()
    res = mink.solve_ik_multistart(configuration, tasks, dt, S, args.max_iters, pos_thr, ori_thr, damping=damping, limits=limits,
                                   rng_seed=args.rng_seed, update=False, return_all=True)
    t1 = time.perf_counter()
    print(f"UR5e, {B} far targets, every loop from `home`, at most {args.max_iters} iterations:")
    print(f"  single start : {int(single.sum()):6d} of {B} converged")
    print(f"  {S:3d} starts   : {int(res.converged.sum()):6d} of {B} converged   ({1e3 * (t1 - t0):.2f} ms, numpy in and out)")
    assert res.converged[single].all()
    if args.seed_table:
        table = mink.SeedTable(mink.Configuration(model, home), tasks, args.seed_table, limits=limits, rng_seed=11)
        near = mink.solve_ik_multistart(configuration, tasks, dt, S, args.max_iters, pos_thr, ori_thr, damping=damping,
                                        limits=limits, update=False, seed_table=table)
        index, distance, _ = table.query(end_effector.transform_target_to_world.wxyz_xyz, max(1, S - 1))
        print(f"  {S:3d} starts, seeds 1 … {S - 1} the nearest of {args.seed_table} stored postures: {int(near.converged.sum()):6d} of {B} "
              f"converged (random seeds: {int(res.converged.sum())}); median distance of the nearest entry "
              f"{np.median(distance[:, 0]):.3f} (m² + rad²)")
        assert near.converged[single].all()
        table.close()
    # the selection: closest to `home` among the converged seeds, against taking the first one that converged
    ok = res.converged_all & ((res.status_all & ~1) == 0)
    many = np.flatnonzero(ok.sum(axis=1) > 1)
    if len(many):
        first = ok[many].argmax(axis=1)
        d_first = np.linalg.norm(res.q_all[many, first] - home, axis=1)
        d_best = np.linalg.norm(res.q[many] - home, axis=1)
        print(f"  {len(many)} targets with several converged seeds: mean |q - home| {d_best.mean():.3f} rad for the chosen seed, "
              f"{d_first.mean():.3f} for the first converged one; converged seeds per target {ok.sum(axis=1).mean():.1f} of {S}")
    # every returned solution reaches its target
    configuration.update(res.q)
    err = end_effector.compute_error(configuration)[res.converged]
    print(f"  worst pose error of the converged results: position {np.linalg.norm(err[:, :3], axis=1).max():.2e}, "
          f"orientation {np.linalg.norm(err[:, 3:], axis=1).max():.2e}")


if __name__ == "__main__":
    main()
