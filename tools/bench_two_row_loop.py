#!/usr/bin/env python
"""Fused IK loops (mkh_solve_steps / mkh_solve_until) of the 17 … 32-dof robots, device-resident, timed with events: the row
kernel's two-row build (`ik_quad_kernel_32_loop`, forced with quad_kernel=True) against the wavefront kernel's loop
(wave_kernel=True), and which of the two the default dispatch takes.

    python tools/bench_two_row_loop.py [batches=4096,16384,65536] [reps=5] [robots=h1_c3,h1_full,h1_rel,go1,shadow]

Legs: a fixed loop of 10 steps, and the threshold loop (at most 20 iterations, pos 1e-3, ori 1e-2).  Robots: H1 with the
`h1_c3` and `h1_full` task sets (mink_amd/workloads.py) and `h1_rel` (`h1_c3` with the wrists as RelativeFrameTasks measured in the
pelvis frame: a floating base with RelativeFrameTasks and no ComTask), Go1 with the task set of the `ik_go1_c` fixture (trunk pose, four
feet, posture 1e-5, ConfigurationLimit), the Shadow hand without contacts (five fingertips, posture 1e-2, ConfigurationLimit).
Per line: kernel ms (median of `reps`), M targets/s (instances whose loop completes per second), converged fraction, the
two-row build's speedup and the default dispatch's kernel.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _rel_pose(root, frame):
    """T_root⁻¹ · T_frame of (B, 7) wxyz_xyz poses"""
    def qmul(a, b):
        w1, x1, y1, z1 = a.T; w2, x2, y2, z2 = b.T
        return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                         w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)
    qc = root[:, :4] * np.array([1.0, -1.0, -1.0, -1.0])
    d = np.concatenate([np.zeros((len(root), 1)), frame[:, 4:] - root[:, 4:]], axis=1)
    return np.concatenate([qmul(qc, frame[:, :4]), qmul(qmul(qc, d), root[:, :4])[:, 1:]], axis=1)


def problem(nat, workloads, name, B):
    """(model, native model, problem, dt, damping, key q, frame targets or None)"""
    from mink_amd.api_specs import configuration_limit_desc, velocity_limit_desc
    from mink_amd.flatmodel import FlatModel

    if name in ("h1_c3", "h1_full"):
        m = workloads.load_robot("h1")
        nm = nat.NativeModel(m)
        prob, dt, damping = workloads.bench_config(name, m, nm, B)
        return m, nm, prob, dt, damping, m.key_qpos[m.name2id("key", "stand")], None
    if name == "h1_rel":
        m = workloads.load_robot("h1")
        nm = nat.NativeModel(m)
        key = m.key_qpos[m.name2id("key", "stand")]
        plain = [workloads._frame_desc(m, s, "site", 200.0, o, 1.0) for s, o in (("left_foot", 10.0), ("right_foot", 10.0), ("left_wrist", 0.0), ("right_wrist", 0.0))]
        lims = {"configuration_limits": [configuration_limit_desc(m)],
                "velocity_limits": [velocity_limit_desc(m, workloads._hinge_velocities(m))]}
        twin = nat.NativeProblem(nm, frame_tasks=plain + [workloads._frame_desc(m, "pelvis", "body", 1.0, 1.0)], posture_tasks=[{"cost": 1.0}],
                                 max_batch=B, **lims)
        q, tg = workloads.make_batch(m, nm, twin, np.random.default_rng(5), B, base_q=key)
        twin.close()
        fts = plain[:2]
        for d in plain[2:]:
            d = dict(d); d.update(root_type="body", root_id=m.name2id("body", "pelvis")); fts.append(d)
        tgr = np.concatenate([tg[:, :2], np.stack([_rel_pose(tg[:, 4], tg[:, k]) for k in (2, 3)], axis=1)], axis=1)
        prob = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1.0}], max_batch=B, **lims)
        return m, nm, prob, 5e-3, 1e-1, key, (q, tgr)
    if name == "go1":
        m = FlatModel.load(os.path.join(REPO, "tests", "golden", "models", "all", "unitree_go1__scene.json"))
        nm = nat.NativeModel(m)
        fts = [workloads._frame_desc(m, "trunk", "body", 1.0, 1.0)] + [workloads._frame_desc(m, s, "site", 1.0, 0.0) for s in ("FL", "FR", "RR", "RL")]
        prob = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1e-5}], configuration_limits=[configuration_limit_desc(m)],
                                 max_batch=B)
        return m, nm, prob, 2e-3, 1e-5, m.key_qpos[m.name2id("key", "home")], None
    if name == "shadow":
        m = workloads.load_robot("shadow_left")
        nm = nat.NativeModel(m)
        fts = [workloads._frame_desc(m, f, "site", 1.0, 0.0, 1.0) for f in workloads.SHADOW_FINGERS]
        prob = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 1e-2}], configuration_limits=[configuration_limit_desc(m)],
                                 max_batch=B)
        return m, nm, prob, 2e-3, 1e-5, m.key_qpos[m.name2id("key", "grasp hard")], None
    raise KeyError(name)


def main():
    import torch

    from mink_amd import _native as nat
    from mink_amd import workloads

    batches = [int(b) for b in (sys.argv[1] if len(sys.argv) > 1 else "4096,16384,65536").split(",")]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    robots = (sys.argv[3] if len(sys.argv) > 3 else "h1_c3,h1_full,h1_rel,go1,shadow").split(",")
    dev = torch.device("cuda", 0)
    legs = (("steps10", {"n_steps": 10}), ("until20", {"n_steps": 20, "until": (1e-3, 1e-2)}))
    print("%-8s %6s %-8s | %-24s %9s %9s %6s | %-28s %9s %9s %6s | %-7s | %s" % ("robot", "B", "leg", "quad_kernel=True", "ms", "Mtgt/s",
          "conv", "wave_kernel=True", "ms", "Mtgt/s", "conv", "speedup", "default"), flush=True)
    for name in robots:
        for B in batches:
            m, nm, prob, dt, damping, key, batch = problem(nat, workloads, name, B)
            q, tg = batch if batch is not None else workloads.make_batch(m, nm, prob, np.random.default_rng(5), B, base_q=key)
            ct = None
            if prob.n_com:
                # per-instance CoM targets: the subtree CoM of a perturbed configuration (the wavefront kernel's tap)
                qc = nm.integrate(q, np.random.default_rng(6).normal(scale=0.1, size=(B, m.nv)), 1.0)
                _, _, t = prob.solve(qc, tg, key[None, :], np.zeros((B, 1, 3)), 1.0, 1.0, taps=["subtree_com"], solve_qp=False)
                ct = torch.from_numpy(t["subtree_com"].reshape(B, 1, 3).copy()).to(dev)
            qd, tgd = torch.from_numpy(q).to(dev), torch.from_numpy(tg).to(dev)
            pt = torch.from_numpy(key[None, :].copy()).to(dev)
            for leg, kw in legs:
                row = []
                for wave in (False, True):
                    ms = []
                    for r in range(reps + 2):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        out = prob.solve(qd, tgd, pt, ct, dt, damping, wave_kernel=wave, quad_kernel=not wave, **kw)
                        e1.record()
                        torch.cuda.synchronize()
                        if r >= 2:
                            ms.append(e0.elapsed_time(e1))
                    st = out[2].cpu().numpy()
                    conv = float(out[4].float().mean().item()) if len(out) > 4 else float("nan")
                    t = float(np.median(ms))
                    row.append((prob.last_kernel(), t, B / t / 1e3, conv, int(((st & ~1) != 0).sum())))
                a, b = row
                prob.solve(qd, tgd, pt, ct, dt, damping, **kw)
                torch.cuda.synchronize()
                print("%-8s %6d %-8s | %-24s %9.3f %9.2f %6.3f | %-28s %9.3f %9.2f %6.3f | %6.2fx | %s%s" % (
                    name, B, leg, a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], b[1] / a[1], prob.last_kernel(),
                    "" if a[4] == b[4] == 0 else "  (failed: %d / %d)" % (a[4], b[4])), flush=True)
            del prob


if __name__ == "__main__":
    main()
