"""Designed quaternion states for ball and free joints (mink_amd/csrc/lie_dev.h: quat2vel, qnormalize, axis_angle and every
kernel family's copy of the code around them): quaternions at the edges of their representation.

Random draws so3_exp(N(0, σ)), σ ≤ 1, are unit to the last bit, have w > 0 and sit 1–2 rad from the posture target: they
never reach the wrap of mju_quat2Vel at π, its zero-axis branch, mju_normalize4's branches, or a quaternion of norm
1 ± 6e-8 (a caller's float32 tensor widened to float64).  `states(m, family, B, seed)` draws a batch "as today" —
`random_models.rand_q`, limited ball joints with σ = 0.15 — and applies one family to every quaternion slice of q
(free joints [a+3:a+7], ball joints [a:a+4]) and of the per-instance posture target.  The plain draw depends on the seed
alone, so two families of one seed differ only in what the family did.

σ = 0.15 on limited ball joints: the reference differentiates the quaternion against (u, u, u, u) and (l, l, l, l)
(mink/limits/configuration_limit.py:100,110), a box with lo = 0 whose hi turns negative further out — the reference's own QP
is then infeasible.  tests/test_quat_cases_cpu.py asserts that no instance is.

`MODELS` are the four problems the device tests solve; `problem(name)` states each once (frames, costs, limits, dt,
damping) for both oracles and for the native descriptor."""

import os

import numpy as np

import random_models as rm
from oracle import ik as oik
from oracle import lie as olie

MIXED = """
<mujoco>
  <compiler angle="radian"/>
  <worldbody>
    <body name="b1" pos="0 0 0.1">
      <inertial pos="0 0 0.05" mass="1" diaginertia="1 1 1"/>
      <joint name="hinge" type="hinge" axis="0 1 0" range="-1.2 1.2" pos="0 0 0.02"/>
      <body name="b2" pos="0.1 0 .3" quat="0.9 0.1 0 0.4">
        <inertial pos="0 0.02 0" mass="0.7" diaginertia="1 1 1"/>
        <joint name="ball" type="ball" pos="0.01 0 0"/>
        <body name="b3" pos="0 0.05 .3">
          <inertial pos="0.03 0 0" mass="0.4" diaginertia="1 1 1"/>
          <joint name="slide" type="slide" axis="1 0.2 0" range="-0.2 0.3"/>
          <site name="tip" pos="0.02 0.01 0.1" quat="0.8 0 0.6 0"/>
          <body name="b4" pos="0 0 .2">
            <inertial pos="0 0 0.1" mass="0.3" diaginertia="1 1 1"/>
            <joint name="px" type="slide" axis="1 0 0"/>
            <joint name="py" type="slide" axis="0 1 0"/>
            <joint name="yaw" type="hinge" axis="0 0 1" pos="0.01 0.02 0"/>
            <joint name="pitch" type="hinge" axis="0 1 0" range="-1 1"/>
            <site name="multi" pos="0.05 0 0.05"/>
          </body>
        </body>
      </body>
    </body>
    <body name="floating" pos="1 0 0.5" quat="0.7 0.1 0.2 0.3">
      <inertial pos="0.01 0.02 0.03" mass="2" diaginertia="1 1 1"/>
      <freejoint name="free"/>
      <site name="fs" pos="0.1 0 0" quat="0.5 0.5 0.5 0.5"/>
      <body name="arm" pos="0 0 0.2">
        <inertial pos="0 0 0.1" mass="0.5" diaginertia="1 1 1"/>
        <joint name="elbow" type="hinge" axis="1 0 0" range="-2 2"/>
        <site name="hand" pos="0 0 0.25"/>
      </body>
    </body>
  </worldbody>
</mujoco>
"""

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JNT_FREE, JNT_BALL = 0, 1
LIMITED_BALL_SIGMA = 0.15
NEAR_PI = (1e-3, 1e-6, 1e-9)
TINY = (1e-6, 1e-9, 1e-13)
FAMILIES = ("plain", "neg_w", "antipodal_target") + tuple("near_pi_%g" % d for d in NEAR_PI) + ("same",) + \
    tuple("tiny_%g" % d for d in TINY) + ("scaled", "f32", "zero")
Q_SCALES = (0.5, 1.0 - 1e-3, 1.0 + 1e-7, 2.0)
TARGET_SCALES = (3.0, 1.0 + 1e-3, 1.0 - 1e-7, 0.25)
SEED = 20261018


def family_delta(family):
    """δ of a near_pi_δ / tiny_δ family name."""
    return float(family.rsplit("_", 1)[1])


def quat_slices(m):
    """[(joint, first qpos index of its quaternion)] of every free and ball joint."""
    out = []
    for j in range(m.njnt):
        a, t = int(m.jnt_qposadr[j]), int(m.jnt_type[j])
        if t == JNT_FREE:
            out.append((j, a + 3))
        elif t == JNT_BALL:
            out.append((j, a))
    return out


def ball_dofs(m):
    """[(joint, first dof)] of the ball joints: where the posture error sees a quaternion (a free joint's is zeroed)."""
    return [(j, int(m.jnt_dofadr[j])) for j in range(m.njnt) if int(m.jnt_type[j]) == JNT_BALL]


def qmul(a, b):
    """Hamilton product, wxyz."""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _as_today(m, rng):
    q = rm.rand_q(m, rng)
    for j, a in quat_slices(m):
        if int(m.jnt_type[j]) == JNT_BALL and m.jnt_limited[j]:
            q[a:a + 4] = olie.so3_exp(rng.normal(scale=LIMITED_BALL_SIGMA, size=3))
    return q


def plain(m, B, seed):
    """(q, posture_target, axes): the draw every family starts from; axes (B, n_quat, 3) are the unit axes `a` of the
    near_pi / tiny families, drawn here so that every δ turns about the same ones."""
    rng = np.random.default_rng(seed)
    q = np.stack([_as_today(m, rng) for _ in range(B)])
    pt = np.stack([_as_today(m, rng) for _ in range(B)])
    ax = rng.normal(size=(B, len(quat_slices(m)), 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    return q, pt, ax


def states(m, family, B, seed=SEED):
    """(q, posture_target), both (B, nq), of one family (the table in docs/HISTORY.md)."""
    q, pt, ax = plain(m, B, seed)
    rng = np.random.default_rng(seed + 1)
    sl = quat_slices(m)
    for i in range(B):
        for k, (j, a) in enumerate(sl):
            s = slice(a, a + 4)
            if family == "neg_w":
                q[i, s] = -q[i, s]
            elif family == "antipodal_target":
                pt[i, s] = -qmul(q[i, s], olie.so3_exp(rng.normal(scale=0.3, size=3)))
            elif family.startswith("near_pi_"):
                d = family_delta(family)
                pt[i, s] = qmul(q[i, s], _exp_about(ax[i, k], np.pi - d if i % 2 == 0 else np.pi + d))
            elif family == "same":
                pt[i, s] = q[i, s] if i % 2 else -q[i, s]
            elif family.startswith("tiny_"):
                pt[i, s] = qmul(q[i, s], _exp_about(ax[i, k], family_delta(family)))
            elif family == "scaled":
                q[i, s] = q[i, s] * Q_SCALES[i % 4]
                pt[i, s] = pt[i, s] * TARGET_SCALES[i % 4]
            elif family == "f32":
                q[i, s] = q[i, s].astype(np.float32).astype(np.float64)
                pt[i, s] = pt[i, s].astype(np.float32).astype(np.float64)
            elif family == "zero":
                if k == i % len(sl):
                    q[i, s] = 0.0
            elif family != "plain":
                raise KeyError(family)
    return q, pt


def _exp_about(axis, angle):
    """exp(axis·angle) with the half angle taken before sin / cos (so3_exp of a vector of norm π ± 1e-9 would round it)."""
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * axis])


# ----------------------------------------------------------------------------------------------------------- the problems
MODELS = ("mixed", "balllimit", "ballchain", "h1")
BATCH = {"mixed": 32, "balllimit": 32, "ballchain": 16, "h1": 32}
# ballchain: velocity limit (rad/s on every hinge and unlimited ball dof) and posture cost, chosen on the C oracle so that the box
# binds on some dofs and not on most (tests/test_quat_cases_cpu.py::test_ballchain_velocity_bounds_bind_on_some_dofs)
BALLCHAIN_VMAX, BALLCHAIN_POSTURE_COST, BALLCHAIN_DT = 8.0, 0.3, 0.02
_problems = {}


def _c6(p, o):
    return np.array([p] * 3 + [o] * 3, dtype=np.float64)


def problem(name):
    """One of MODELS as a dict: m, frames [(name, type, cost6, gain, lm_damping)], posture (cost (nv,), gain), cfg_gain,
    vel (indices, limit) or None, dt, damping."""
    if name in _problems:
        return _problems[name]
    import mink_amd
    from mink_amd.flatmodel import FlatModel
    vel = None
    if name == "mixed":
        m = mink_amd.loads_mjcf(MIXED)
        c = np.array([1.0, 2.0, 0.5, 0.3, 0.3, 0.3])
        frames = [(s, "site", c, 0.7, 0.5) for s in ("tip", "fs", "hand")]
        posture, cfg_gain, dt, damping = (np.linspace(0.1, 0.5, m.nv), 0.5), 0.8, 1e-2, 1e-4
    elif name == "balllimit":
        m = FlatModel.load(os.path.join(GOLDEN, "models", "balllimit.json"))
        frames = [("tip", "site", _c6(2.0, 0.5), 1.0, 0.1)]
        posture, cfg_gain, dt, damping = (np.full(m.nv, 0.1), 1.0), 0.9, 1e-2, 1e-4
    elif name == "ballchain":
        xml, sites = rm.ball_chain_mjcf(seed=3)
        m = mink_amd.loads_mjcf(xml)
        frames = [(s, "site", _c6(1.0, 0.3), 1.0, 0.5) for s in sites]
        posture, cfg_gain, dt, damping = (np.full(m.nv, BALLCHAIN_POSTURE_COST), 1.0), 0.95, BALLCHAIN_DT, 1e-4
        # (not on the limited ball joints: their box is then the ConfigurationLimit's alone, which the taps hold to 1e-13)
        idx = np.array([d for j in range(m.njnt) if int(m.jnt_type[j]) != JNT_FREE and not (int(m.jnt_type[j]) == JNT_BALL and m.jnt_limited[j])
                        for d in range(int(m.jnt_dofadr[j]), int(m.jnt_dofadr[j]) + (3 if int(m.jnt_type[j]) == JNT_BALL else 1))])
        vel = (idx, np.full(len(idx), BALLCHAIN_VMAX))
    elif name == "h1":
        from mink_amd import workloads
        m = workloads.load_robot("h1")
        frames = [(s, "site", _c6(200.0, o), 1.0, 1.0) for s, o in (("left_foot", 10.0), ("right_foot", 10.0), ("left_wrist", 0.0), ("right_wrist", 0.0))]
        posture, cfg_gain, dt, damping = (np.full(m.nv, 1.0), 1.0), 0.95, 5e-3, 1e-1
        idx = np.array([int(m.jnt_dofadr[j]) for j in range(m.njnt) if int(m.jnt_type[j]) != JNT_FREE])
        vel = (idx, np.full(len(idx), np.pi))
    else:
        raise KeyError(name)
    _problems[name] = {"name": name, "m": m, "frames": frames, "posture": posture, "cfg_gain": cfg_gain, "vel": vel,
                       "dt": dt, "damping": damping}
    return _problems[name]


def oracle_specs(P, tg_i, pt_i):
    """(tasks, limits) of one instance for oracle/ik.py and oracle/cport.py: frame tasks, then the posture task."""
    m = P["m"]
    tasks = [oik.FrameTaskSpec(m.name2id(t, n), t, c, tg_i[k], g, lm) for k, (n, t, c, g, lm) in enumerate(P["frames"])]
    tasks.append(oik.PostureTaskSpec(P["posture"][0], pt_i, P["posture"][1]))
    limits = [oik.ConfigurationLimitSpec(P["cfg_gain"])]
    if P["vel"] is not None:
        limits.append(oik.VelocityLimitSpec(P["vel"][0], P["vel"][1]))
    return tasks, limits


def native_problem(nat, P, max_batch):
    """(NativeModel, NativeProblem) of the same problem."""
    m = P["m"]
    nm = nat.NativeModel(m)
    fts = [{"frame_type": t, "frame_id": m.name2id(t, n), "cost": list(c), "gain": g, "lm_damping": lm} for n, t, c, g, lm in P["frames"]]
    idx, lower, upper = oik.configuration_limit_arrays(m, oik.ConfigurationLimitSpec(P["cfg_gain"]))
    kw = {}
    if P["vel"] is not None:
        kw["velocity_limits"] = [{"indices": P["vel"][0], "limit": P["vel"][1]}]
    prob = nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": P["posture"][0], "gain": P["posture"][1]}],
                             configuration_limits=[{"gain": P["cfg_gain"], "lower": lower, "upper": upper, "indices": idx}],
                             max_batch=max_batch, **kw)
    return nm, prob


_targets = {}


def frame_targets(P, B, seed=SEED):
    """(B, n_frame, 7): the frames' poses at plain q ⊕ N(0, 0.2) — the same for every family of one seed."""
    key = (P["name"], B, seed)
    if key not in _targets:
        m = P["m"]
        q, _, _ = plain(m, B, seed)
        rng = np.random.default_rng(seed + 2)
        tg = np.empty((B, len(P["frames"]), 7))
        for i in range(B):
            cfg = oik.Configuration(m, q[i])
            cfg.update(cfg.integrate(rng.normal(scale=0.2, size=m.nv), 1.0))
            for k, (n, t, _, _, _) in enumerate(P["frames"]):
                tg[i, k] = cfg.get_transform_frame_to_world(m.name2id(t, n), t)
        _targets[key] = tg
    return _targets[key]


_cases = {}


def case(name, family, B=None, seed=SEED):
    """(P, q, posture_target (B, 1, nq), frame_targets) of one model and family."""
    B = BATCH[name] if B is None else B
    key = (name, family, B, seed)
    if key not in _cases:
        P = problem(name)
        q, pt = states(P["m"], family, B, seed)
        _cases[key] = (P, q, pt[:, None, :].copy(), frame_targets(P, B, seed))
    return _cases[key]


_c_solved = {}


def c_oracle(name, family, B=None, seed=SEED, q=None, pt=None):
    """(v, status) of every instance on the plain-C oracle, once per session (q / pt override the family's, uncached)."""
    from oracle import cport
    P, q0, pt0, tg = case(name, family, B, seed)
    key = (name, family, len(q0), seed)
    if q is not None or pt is not None or key not in _c_solved:
        tasks, limits = oracle_specs(P, tg[0], pt0[0, 0])
        res = cport.CProblem(P["m"], tasks, limits).solve_batch(q0 if q is None else q, tg, pt0 if pt is None else pt,
                                                                P["dt"], P["damping"], nthreads=4)
        if q is not None or pt is not None:
            return res
        _c_solved[key] = res
    return _c_solved[key]


def numpy_oracle(P, q_i, tg_i, pt_i):
    tasks, limits = oracle_specs(P, tg_i, pt_i)
    return oik.solve_ik(P["m"], q_i, tasks, P["dt"], P["damping"], limits)


def outside_limits(m, q_i):
    """The reference's check_limits on one configuration (mink/configuration.py:86-110): MKH_ST_OUTSIDE_LIMITS."""
    return len(oik.Configuration(m, q_i).limit_violations()) > 0
