"""Closed-loop fixture from the REAL reference for the fused loop of the row kernel's two-row build (floating base; build
container only; same method as make_golden_mid.py — /root/reference/mink on top of oracle/stubs):

    python tests/golden/make_golden_loop.py

  ik_h1_loop.npz  Unitree H1 (examples/unitree_h1/scene.xml, free joint + 19 hinges), the tasks of examples/humanoid_h1.py:22-52
                  as written — pelvis orientation (body frame), feet (pos 200 / ori 10, lm 1), wrists (pos 200 / ori 0, lm 1),
                  PostureTask(1), ComTask(200) with a per-instance CoM target — and its loop (humanoid_h1.py:87-89): 8 iterations
                  of solve_ik(dt = 5e-3, damping 1e-1, default limits) + Configuration.integrate_inplace, on 16 instances.
                  q: (16, 9, nq) — the start and every integrated configuration; v: (16, 8, nv) — every step's velocity.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ext as mg  # noqa: E402

mink, mujoco = mg.mink, mg.mujoco
EX = "/root/reference/examples/"


def h1_loop(rng, n=16, steps=8):
    m = mujoco.MjModel.from_xml_path(EX + "unitree_h1/scene.xml")
    fts = [mink.FrameTask("pelvis", "body", position_cost=0.0, orientation_cost=10.0)]
    fts += [mink.FrameTask(s, "site", position_cost=200.0, orientation_cost=10.0, lm_damping=1.0) for s in ("right_foot", "left_foot")]
    fts += [mink.FrameTask(s, "site", position_cost=200.0, orientation_cost=0.0, lm_damping=1.0) for s in ("right_wrist", "left_wrist")]
    post = mink.PostureTask(m, cost=1.0)
    com = mink.ComTask(cost=200.0)
    q0 = np.array(m.key_qpos[m.key("stand").id])
    post.set_target(q0)
    tasks = fts + [post, com]
    dt, damping = 5e-3, 1e-1
    rec = {k: [] for k in ("q", "v", "frame_targets", "com_targets")}
    for q in mg.sample_q(m, rng, n, base_q=q0):
        ct = mink.Configuration(m, mg.perturbed(m, q, rng, 0.15))
        for t in fts:
            t.set_target(ct.get_transform_frame_to_world(t.frame_name, t.frame_type))
        com.set_target(ct.data.subtree_com[1].copy())
        cfg = mink.Configuration(m, q)
        qs, vs = [cfg.q.copy()], []
        for _ in range(steps):
            v = mink.solve_ik(cfg, tasks, dt, "quadprog", damping)
            cfg.integrate_inplace(v, dt)
            qs.append(cfg.q.copy()); vs.append(v)
        rec["q"].append(qs); rec["v"].append(vs)
        rec["frame_targets"].append([t.transform_target_to_world.wxyz_xyz for t in fts])
        rec["com_targets"].append(np.array(com.target_com))
    out = {k: np.array(v) for k, v in rec.items()}
    out.update({"dt": np.array(dt), "damping": np.array(damping), "posture_target": q0.copy()})
    np.savez_compressed(os.path.join(HERE, "ik_h1_loop.npz"), **out)
    print("ik_h1_loop.npz", {k: v.shape for k, v in out.items()}, "max|v|", float(np.abs(out["v"]).max()))


if __name__ == "__main__":
    h1_loop(np.random.default_rng(47))
