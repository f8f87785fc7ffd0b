"""Fixtures of tests/test_gpu_wood_lists.py (the low-rank start's host tables: dof lists of the product lanes, the chunk
entry of the right-hand side, the joint-anchor flag), generated and solved on the CPU: seeded configurations, frame targets
from the numpy oracle's forward kinematics at a perturbed configuration, the C oracle's answer on every instance.
tests/test_wood_list_cases_cpu.py holds every case against the numpy oracle before any device sees it."""

import functools
import os
from typing import NamedTuple, Optional, Sequence

import numpy as np

import mink_amd as mink
import oracle_configs as oc
from mink_amd import workloads
from oracle import cport
from oracle import ik as oik

B = 64
FAILURE_BITS = 2 | 4 | 8          # MKH_ST_INFEASIBLE | MKH_ST_NOT_PD | MKH_ST_ITER_LIMIT
FEET_PALMS = (("left_foot", 10.0), ("right_foot", 10.0), ("left_palm", 0.0), ("right_palm", 0.0))
# cost vectors of case (c): bit r of a task's rowmask is set iff cost[r] > 0
POS_ONLY = (200.0, 200.0, 200.0, 0.0, 0.0, 0.0)      # 0b000111
ORI_ONLY = (0.0, 0.0, 0.0, 10.0, 10.0, 10.0)         # 0b111000
GAPS = (200.0, 0.0, 150.0, 10.0, 0.0, 5.0)           # 0b101101
FULL = (200.0, 200.0, 200.0, 10.0, 10.0, 10.0)


class Frame(NamedTuple):
    name: str
    kind: str
    cost: Sequence[float]
    lm_damping: float = 1.0


class Case(NamedTuple):
    label: str
    model: object                 # FlatModel of the product (NativeModel is built from it)
    oracle_model: object          # the oracle's FlatModel of the same robot
    frames: Sequence[Frame]
    posture_cost: float
    dt: float
    damping: float
    q: np.ndarray                 # (B, nq)
    frame_targets: np.ndarray     # (B, n_frame, 7)
    posture_target: np.ndarray    # (1, nq)
    collision: Optional[object]   # oracle CollisionAvoidanceLimitSpec, or None
    kernel: str                   # prefix of the build a plain solve of this case runs on


def anchor_chain_mjcf(n_links=12, seed=0, moved=None, two_joints_at=5):
    """A serial chain of hinges about random axes, body `two_joints_at` with TWO hinges, a site `tip` on the last link.  Every
    joint sits at its body's origin, except joint `moved` (a body index) when given."""
    rng = np.random.default_rng(seed)
    xml = ['<mujoco><compiler angle="radian"/><worldbody>']
    for i in range(n_links):
        xml.append(f'<body name="b{i}" pos="{0.04 + 0.02 * rng.uniform():.4f} {0.01 * rng.normal():.4f} {0.01 * rng.normal():.4f}">')
        for k in range(2 if i == two_joints_at else 1):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            pos = ' pos="0.013 -0.021 0.017"' if (i == moved and k == 0) else ""
            xml.append(f'<joint name="j{i}_{k}" type="hinge" axis="{ax[0]:.5f} {ax[1]:.5f} {ax[2]:.5f}" range="-1.5 1.5"{pos}/>')
        xml.append('<geom type="sphere" size="0.01" mass="0.1"/>')
    xml.append('<site name="tip" pos="0.02 0 0"/>')
    xml.append("</body>" * n_links)
    xml.append("</worldbody></mujoco>")
    return "".join(xml)


def _inputs(model, oracle_model, frames, seed, base_q=None, sigma=0.15):
    """q inside the ranges; targets = the frames' poses at q ⊕ δ, δ ~ N(0, σ²) per dof (workloads.make_batch's distribution,
    with the oracle's kinematics instead of the device's)."""
    rng = np.random.default_rng(seed)
    q = workloads.sample_q(model, rng, B, base_q)
    delta = rng.normal(scale=sigma, size=(B, model.nv))
    tg = np.empty((B, len(frames), 7))
    for i in range(B):
        cfg = oik.Configuration(oracle_model, q[i])
        cfg.update(cfg.integrate(delta[i], 1.0))
        for k, f in enumerate(frames):
            tg[i, k] = cfg.get_transform_frame_to_world(oracle_model.name2id(f.kind, f.name), f.kind)
    return q, tg


def _g1(label, frames, seed, kernel="ik_solve_kernel_44_32_r44_w3", robot="g1", collision=None):
    model = workloads.load_bench_robot("g1_coll") if collision else workloads.load_robot(robot)
    om = model if collision else oc.model(robot)
    stand = model.key_qpos[model.name2id("key", "stand")]
    q, tg = _inputs(model, om, frames, seed, base_q=stand)
    col = None
    if collision:
        col = oik.CollisionAvoidanceLimitSpec([tuple(p) for p in workloads.g1_collision_pairs(model)], gain=0.85,
                                              minimum_distance_from_collisions=0.005, collision_detection_distance=0.25)
    return Case(label, model, om, frames, 1.0, 5e-3, 1e-1, q, tg, np.array(stand)[None, :], col, kernel)


def _chain(n, seed, kernel):
    from random_models import hinge_chain_mjcf
    model = mink.loads_mjcf(hinge_chain_mjcf(n, seed=n))
    frames = [Frame("tip", "site", (1.0, 1.0, 1.0, 0.5, 0.5, 0.5))]
    q, tg = _inputs(model, model, frames, seed)
    return Case("chain%d" % n, model, model, frames, 1e-2, 1e-2, 1e-3, q, tg, np.zeros((1, model.nq)), None, kernel)


def _anchor(label, moved, seed=41):
    model = mink.loads_mjcf(anchor_chain_mjcf(moved=moved))
    frames = [Frame("tip", "site", (1.0, 1.0, 1.0, 0.5, 0.5, 0.5))]
    q, tg = _inputs(model, model, frames, seed)      # (the same seed: q of both models alike, the targets differ with the anchor)
    return Case(label, model, model, frames, 1e-2, 1e-2, 1e-3, q, tg, np.zeros((1, model.nq)), None, "ik_solve_kernel_16_32_r16")


def _bench_frames():
    return [Frame(s, "site", (200.0,) * 3 + (o,) * 3) for s, o in FEET_PALMS]


BUILDERS = {
    # (a) chains of different lengths in one problem: the legs' 12 dofs, the arms' 13 (waist + arm) on the floating base's 6
    "g1_bench": lambda: _g1("g1_bench", _bench_frames(), 11),
    # (b) the packed capacity (16 dofs), one past it, a long chain on the headline-size build, and no low-rank build at all
    "chain16": lambda: _chain(16, 21, "ik_solve_kernel_16_32_r16"),
    "chain17": lambda: _chain(17, 22, "ik_solve_kernel_24_32_r24"),
    "chain40": lambda: _chain(40, 23, "ik_solve_kernel_44_32_r44"),
    "chain63": lambda: _chain(63, 24, "ik_solve_kernel_64_"),
    # (c) row-mask gaps on two tasks (6 / 7 / 7 rows), and 13 rows = three chunks of 4 + 1: the right-hand side alone in a chunk
    "rows_pos_ori": lambda: _g1("rows_pos_ori", [Frame("left_foot", "site", POS_ONLY), Frame("right_palm", "site", ORI_ONLY)], 31),
    "rows_ori_gaps": lambda: _g1("rows_ori_gaps", [Frame("left_foot", "site", ORI_ONLY), Frame("right_palm", "site", GAPS)], 32),
    "rows_gaps_pos": lambda: _g1("rows_gaps_pos", [Frame("right_foot", "site", GAPS), Frame("left_palm", "site", POS_ONLY)], 33),
    "rows_13": lambda: _g1("rows_13", [Frame("left_foot", "site", FULL), Frame("right_palm", "site", GAPS),
                                       Frame("left_palm", "site", POS_ONLY)], 34),
    # (e) the anchor flag: every joint at its body's origin / one hinge moved (a body with two joints in both)
    "anchors_zero": lambda: _anchor("anchors_zero", None),
    "anchors_moved": lambda: _anchor("anchors_moved", 3),
    # (f) contact rows next to the low-rank start
    "g1_coll": lambda: _g1("g1_coll", _bench_frames(), 51, kernel="ik_solve_kernel_48_40_r48", collision=True),
}


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    return BUILDERS[name]()


def oracle_tasks(c: Case, i: int):
    """Specs of instance i for the numpy oracle (and, with i = 0, the task list of the C oracle's problem)."""
    om = c.oracle_model
    tasks = [oik.FrameTaskSpec(om.name2id(f.kind, f.name), f.kind, np.array(f.cost, dtype=np.float64), c.frame_targets[i, k],
                               lm_damping=f.lm_damping) for k, f in enumerate(c.frames)]
    tasks.append(oik.PostureTaskSpec(np.full(om.nv, c.posture_cost), c.posture_target[0]))
    limits = [oik.ConfigurationLimitSpec(), oc._hinge_velocity_limit(om)]
    if c.collision is not None:
        limits.append(c.collision)
    return tasks, limits


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """(v_ref, status) of the C oracle on every instance of a case — computed once per session, shared, never written to."""
    c = case(name)
    tasks, limits = oracle_tasks(c, 0)
    cp = cport.CProblem(c.oracle_model, tasks, limits)
    v, st = cp.solve_batch(c.q, c.frame_targets, c.posture_target, c.dt, c.damping, nthreads=min(16, os.cpu_count() or 1))
    v.setflags(write=False)
    st.setflags(write=False)
    return v, st
