#!/usr/bin/env python
"""Ladder-graph trajectory IK: the far Cartesian lines of batched_global_trajectory_ur5e.py, tracked four ways — from one start
(`solve_ik_trajectory`), from several whole candidates (`solve_ik_trajectory_multistart`), and through a ladder graph
(`solve_ik_trajectory_ladder`: several IK solutions per waypoint, the path picked by a dynamic program on the device) with
drawn seeds and, with `--seed-table`, with seeds looked up in a table of stored postures by every waypoint's own pose.  With
`--refine` every ladder runs a second time with the refinement pass behind its search (`refine=True`): the chosen path is
re-tracked across its breaks and lost waypoints, and kept only where that makes it better.  With `--n-nodes K` the drawn
ladder also runs on K distinct nodes per waypoint, deduplicated on the device out of `--node-seeds` solutions (`n_nodes=K`:
the search and the device's node rows then do not grow with the seeds), and with `--unwind` those solutions are first moved to
the full turn of every long-range joint that lies nearest `home` (`unwind_turns=True`).

    python examples/batched_ladder_ur5e.py --paths 256 --seeds 8 --seed-table --refine
    python examples/batched_ladder_ur5e.py --paths 256 --n-nodes 8 --node-seeds 64 --unwind

UR5e, one FrameTask on `attachment_site` (costs 1 / 1, lm_damping 1), ConfigurationLimit, dt = 1, damping = 1e-3, thresholds
1e-4 / 1e-4, 40 iterations per waypoint, every path started at `home`.  A path counts as COMPLETE when every waypoint is tracked
(its loop converged without a QP failure) and as BREAK-FREE when no joint-space step between consecutive waypoints exceeds
`--max-step` (Euclidean, rad): candidate tracking is continuous by construction, a ladder has to be asked — its rungs are solved
independently of each other, so two consecutive solutions may sit on different IK branches; the search avoids that where it can
and reports it where it cannot.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))   # run from a source checkout
import mink_amd as mink  # noqa: E402
from batched_global_trajectory_ur5e import cartesian_lines  # noqa: E402


def complete_and_break_free(q, tracked, max_step):
    """(complete, complete and break-free) per path from its configurations (B, T, nq) and tracked flags (B, T)."""
    steps = np.sqrt((np.diff(q, axis=1) ** 2).sum(axis=2))
    complete = tracked.all(axis=1)
    return complete, complete & (steps <= max_step).all(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--waypoints", type=int, default=16)
    ap.add_argument("--max-iters", type=int, default=40)
    ap.add_argument("--max-step", type=float, default=1.0, help="joint-space step between waypoints that counts as a break (rad)")
    ap.add_argument("--rng-seed", type=int, default=5)
    ap.add_argument("--seed-table", action="store_true", help="also run the ladder seeded from a table of stored postures")
    ap.add_argument("--table-entries", type=int, default=16384)
    ap.add_argument("--refine", action="store_true", help="also run every ladder with the refinement pass behind its search")
    ap.add_argument("--n-nodes", type=int, default=0, help="also run the drawn ladder on this many distinct nodes per waypoint")
    ap.add_argument("--node-seeds", type=int, default=64, help="solutions per waypoint the nodes of --n-nodes are picked from")
    ap.add_argument("--min-distance", type=float, default=0.1, help="two solutions closer than this are one node (rad)")
    ap.add_argument("--unwind", action="store_true", help="with --n-nodes: move the solutions to the turn nearest `home` first")
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
    targets = {end_effector: lines}

    def timed(call):
        call()                                                               # (first call: builds the handle)
        t0 = time.perf_counter()
        out = call()
        return out, 1e3 * (time.perf_counter() - t0)

    rows = []
    single, ms = timed(lambda: mink.solve_ik_trajectory(configuration, tasks, 1.0, targets, n_steps=args.max_iters, **kw))
    rows.append(("trajectory (one start)", single.q, single.converged & ((single.status & ~1) == 0), ms))
    multi, ms = timed(lambda: mink.solve_ik_trajectory_multistart(configuration, tasks, 1.0, targets, S, args.max_iters,
                                                                  rng_seed=args.rng_seed, **kw))
    rows.append((f"trajectory multi-start ({S} candidates)", multi.q, multi.converged & ((multi.status & ~1) == 0), ms))
    ladder = lambda **extra: mink.solve_ik_trajectory_ladder(configuration, tasks, 1.0, targets, S, args.max_iters,
                                                             max_step=args.max_step, rng_seed=args.rng_seed, **kw, **extra)
    drawn, ms = timed(ladder)
    rows.append((f"ladder ({S} nodes per waypoint, drawn)", drawn.q, drawn.converged & ((drawn.status & ~1) == 0), ms))
    results, notes = [drawn], []
    if args.refine:
        fine, ms = timed(lambda: ladder(refine=True))
        rows.append((f"ladder ({S} nodes per waypoint, drawn) + refinement", fine.q, fine.converged & ((fine.status & ~1) == 0), ms))
        results.append(fine)
    if args.unwind and not args.n_nodes:
        ap.error("--unwind works in front of the selection of --n-nodes")
    if args.n_nodes:
        K, S2 = args.n_nodes, args.node_seeds
        nodes_kw = dict(n_nodes=K, min_distance=args.min_distance, unwind_turns=args.unwind)
        few = lambda **extra: mink.solve_ik_trajectory_ladder(configuration, tasks, 1.0, targets, S2, args.max_iters,
                                                              max_step=args.max_step, rng_seed=args.rng_seed, **kw, **nodes_kw, **extra)
        label = f"ladder ({K} distinct of {S2} solutions{', unwound' if args.unwind else ''})"
        picked, ms = timed(few)
        rows.append((label, picked.q, picked.converged & ((picked.status & ~1) == 0), ms))
        results.append(picked)
        if args.refine:
            fine, ms = timed(lambda: few(refine=True))
            rows.append((label + " + refinement", fine.q, fine.converged & ((fine.status & ~1) == 0), ms))
            results.append(fine)
        notes.append(f"  nodes: {float(picked.n_distinct.mean()):.2f} distinct solutions per waypoint on average, "
                     f"{int((picked.n_uncovered > 0).sum())} of {B * T} waypoints hold more than {K}")
    if args.seed_table:
        table = mink.SeedTable(mink.Configuration(model, home), tasks, args.table_entries, limits=limits)
        looked_up, ms = timed(lambda: ladder(seed_table=table))
        rows.append((f"ladder ({S} nodes per waypoint, seed table of {args.table_entries})", looked_up.q,
                     looked_up.converged & ((looked_up.status & ~1) == 0), ms))
        results.append(looked_up)
        if args.refine:
            fine, ms = timed(lambda: ladder(seed_table=table, refine=True))
            rows.append((f"ladder ({S} nodes per waypoint, seed table of {args.table_entries}) + refinement", fine.q,
                         fine.converged & ((fine.status & ~1) == 0), ms))
            results.append(fine)
        table.close()

    print(f"UR5e, {B} Cartesian lines of {T} waypoints whose first pose is far from `home`, at most {args.max_iters} iterations per "
          f"waypoint; a break is a joint step beyond {args.max_step} rad:")
    for name, q, tracked, ms in rows:
        complete, clean = complete_and_break_free(q, tracked, args.max_step)
        print(f"  {name:71s}: {int(complete.sum()):5d} complete, {int(clean.sum()):5d} complete and break-free of {B}; "
              f"{int(tracked.sum()):6d} of {B * T} waypoints   ({ms:.2f} ms)")
    for res in results:                                                      # what the search reports is what the path shows
        steps_sq = (np.diff(res.q, axis=1) ** 2).sum(axis=2)
        clear = np.abs(steps_sq - args.max_step ** 2) > 1e-9
        assert (res.edge_break[:, 1:] == (steps_sq > args.max_step ** 2))[clear].all()
        assert (res.n_tracked == (res.converged & ((res.status & ~1) == 0)).sum(axis=1)).all()
    print("\n".join(notes), end="\n" if notes else "")
    for plain, fine in zip(results[0::2], results[1::2]) if args.refine else ():     # the pass never returns a worse path
        worse = [(T - f_t, f_b, f_l) > (T - p_t, p_b, p_l) for f_t, f_b, f_l, p_t, p_b, p_l in
                 zip(fine.n_tracked, fine.n_breaks, fine.path_length, plain.n_tracked, plain.n_breaks, plain.path_length)]
        assert not any(worse)
        print(f"  refinement: {int(fine.refined.sum())} of {B} paths returned re-tracked, {int((fine.repaired != 0).sum())} waypoints repaired "
              f"({int((fine.repaired == 1).sum())} forward, {int((fine.repaired == 2).sum())} backward)")


if __name__ == "__main__":
    main()
