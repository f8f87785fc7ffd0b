"""Models and problems that put the workgroup-per-problem kernel (mink_amd/csrc/wide_kernel.h) on every branch of its layout
(mink_amd/csrc/problem_plan.hip plan_wide), shared by the host plan cases (tests/test_problem_plan_cpu.py), the reference's own
sensitivity test (tests/test_wide_cases_cpu.py) and the device tests (tests/test_gpu_wide_sizes.py).

| name            | model                                        | reaches                                              |
|-----------------|----------------------------------------------|------------------------------------------------------|
| chain123 / 124  | chain_mjcf                                   | last size with the tableau in LDS / first without    |
| chain130        | chain_mjcf                                   | three chain words                                    |
| chain300        | chain_mjcf                                   | two dofs per thread, five chain words                |
| chain_last      | chain_mjcf(CHAIN_LAST)                       | the largest chain whose per-problem state fits LDS   |
| chain_last+1    | chain_mjcf(CHAIN_LAST + 1)                   | refused: MKH_E_LIMIT                                 |
| ball80 / 86 / 92| ball_chain_mjcf(22 / 24 / 26 ball, 8 hinge)  | block-pivot staging appended / absent / appended     |
| fixed30         | fixed_chain_mjcf(30, 2)                      | 91 bodies on 30 dofs: the wide route by body count   |
| hinge80         | hinge_chain_mjcf(80) + sphere pairs          | more than 64 pairs on a wide-only model: the cull    |

A problem is the dict of tests/quat_cases.py::problem (m, frames, posture, cfg_gain, vel, dt, damping), so that its oracle_specs /
native_problem build both sides.  Chains: the problem of tests/test_gpu_wide.py::_chain_problem (frame tasks on the sites, posture
cost 0.05 towards qpos0, ConfigurationLimit 0.95, VelocityLimit 1.0 on every dof, dt 0.02, damping 1e-4, targets the frames' poses
at another random configuration — so far away that the velocity bounds bind).  Ball chains: the settings of quat_cases' `ballchain`.
"""

import numpy as np

import quat_cases as qc
import random_models as rm
from oracle import ik as oik

CHAIN_LAST = 560                   # found with tests/host/plan_cases.cpp (test_problem_plan_cpu.py holds it to the plan)
CHAINS = {"chain123": 123, "chain124": 124, "chain130": 130, "chain300": 300, "chain_last": CHAIN_LAST, "chain_last+1": CHAIN_LAST + 1}
BALLS = {"ball80": (22, 8), "ball86": (24, 8), "ball92": (26, 8)}
SOLVED = ["chain123", "chain124", "chain130", "chain300", "chain_last", "ball80", "ball86", "ball92", "fixed30"]   # per-model checks
HOST_MODELS = SOLVED + ["chain_last+1", "hinge80"]
SEED, BALL_SEED = 3, 3
DT, DAMPING = 0.02, 1e-4
B = 8

# collision case: spheres of radius 0.01 on the links of hinge_chain_mjcf(80), pairs (i, j) with j − i ≥ 6
HINGE80_PAIRS = [(i, i + 6 + (i % 5)) for i in range(0, 74) if i + 6 + (i % 5) < 80] + [(i, i + 40) for i in range(0, 40, 2)]
HINGE80_DETECT, HINGE80_DMIN = 0.17, 0.13

_models, _problems, _cases = {}, {}, {}


def sites_every(ndof):
    """chain_mjcf's site spacing: at most 16 frame tasks (kMaxFrameTasks) at every size."""
    return 25 if ndof <= 375 else 40


def mjcf_text(name):
    """(MJCF text, site names) of one model of the table."""
    if name in CHAINS:
        return rm.chain_mjcf(CHAINS[name], seed=SEED, sites_every=sites_every(CHAINS[name]))
    if name in BALLS:
        return rm.ball_chain_mjcf(BALLS[name][0], BALLS[name][1], seed=BALL_SEED)
    if name == "fixed30":
        return rm.fixed_chain_mjcf(30, 2, seed=SEED)
    if name == "fixed30_plain":
        return rm.fixed_chain_mjcf(30, 0, seed=SEED)
    if name == "hinge80":
        return rm.hinge_chain_mjcf(80), ["tip"]
    raise KeyError(name)


def model(name):
    if name not in _models:
        from mink_amd.mjcf import loads_mjcf
        _models[name] = loads_mjcf(mjcf_text(name)[0])
    return _models[name]


def problem(name):
    if name in _problems:
        return _problems[name]
    m, sites = model(name), mjcf_text(name)[1]
    if name in BALLS:
        frames = [(s, "site", qc._c6(1.0, 0.3), 1.0, 0.5) for s in sites]
        posture, cfg_gain = (np.full(m.nv, qc.BALLCHAIN_POSTURE_COST), 1.0), 0.95
        idx = np.array([d for j in range(m.njnt)
                        if int(m.jnt_type[j]) != qc.JNT_FREE and not (int(m.jnt_type[j]) == qc.JNT_BALL and m.jnt_limited[j])
                        for d in range(int(m.jnt_dofadr[j]), int(m.jnt_dofadr[j]) + (3 if int(m.jnt_type[j]) == qc.JNT_BALL else 1))])
        vel, dt = (idx, np.full(len(idx), qc.BALLCHAIN_VMAX)), qc.BALLCHAIN_DT
    else:
        frames = [(s, "site", np.array([1.0, 1.0, 1.0, 0.3, 0.3, 0.3]), 1.0, 0.5) for s in sites]
        posture, cfg_gain = (np.full(m.nv, 0.05), 1.0), 0.95
        vel, dt = (np.arange(m.nv), np.full(m.nv, 1.0)), DT
    _problems[name] = {"name": "wide:" + name, "m": m, "frames": frames, "posture": posture, "cfg_gain": cfg_gain, "vel": vel,
                       "dt": dt, "damping": DAMPING}
    return _problems[name]


def case(name, B=B, seed=SEED):
    """(P, q (B, nq), posture target (B, 1, nq), frame targets (B, n_frame, 7)) — fixed30_plain shares fixed30's draw (same nq)."""
    key = (name, B, seed)
    if key not in _cases:
        P = problem(name)
        m = P["m"]
        if name in BALLS:
            q, pt, _ = qc.plain(m, B, seed)
            _cases[key] = (P, q, pt[:, None, :].copy(), qc.frame_targets(P, B, seed))
        else:
            rng = np.random.default_rng(seed)
            q = np.array([rm.rand_q(m, rng) for _ in range(B)])
            tg = np.empty((B, len(P["frames"]), 7))
            for i in range(B):
                cfg = oik.Configuration(m, rm.rand_q(m, rng))
                for k, (n, t, _, _, _) in enumerate(P["frames"]):
                    tg[i, k] = cfg.get_transform_frame_to_world(m.name2id(t, n), t)
            _cases[key] = (P, q, np.repeat(np.array(m.qpos0)[None, None, :], B, axis=0), tg)
    return _cases[key]


_c_solved = {}


def c_oracle(name, B=B, seed=SEED):
    """(v, status) of every instance of case(name) on the plain-C oracle, once per session."""
    from oracle import cport
    key = (name, B, seed)
    if key not in _c_solved:
        P, q, pt, tg = case(name, B, seed)
        tasks, limits = qc.oracle_specs(P, tg[0], pt[0, 0])
        _c_solved[key] = cport.CProblem(P["m"], tasks, limits).solve_batch(q, tg, pt, P["dt"], P["damping"], nthreads=min(B, 8))
    return _c_solved[key]


def n_bound(P, v):
    """Velocity bounds binding per instance: dofs of the VelocityLimit whose |v| sits on the limit."""
    idx, lim = P["vel"]
    return (np.abs(np.abs(v[:, idx]) - lim[None, :]) < 1e-9 * lim[None, :]).sum(axis=1)


# ---- the host plan cases: the models as (parent, kind) lists for tests/host/plan_cases.cpp
FIXED, HINGE, HINGE2, BALL, FREE, SLIDE = range(6)


def body_kinds(m):
    """Per moving body (parent id, kind) from the loaded model's arrays."""
    out = []
    for b in range(1, m.nbody):
        n, a = int(m.body_jntnum[b]), int(m.body_jntadr[b])
        if n == 0:
            kind = FIXED
        elif n == 2:
            kind = HINGE2
        else:
            kind = {0: FREE, 1: BALL, 2: SLIDE, 3: HINGE}[int(m.jnt_type[a])]
        out.append((int(m.body_parentid[b]), kind))
    return out


def spec_line(name):
    """One line of the description file of tests/host/plan_cases.cpp: the model, its frame tasks' bodies, ComTasks, geom pairs."""
    m, sites = model(name), mjcf_text(name)[1]
    kinds = body_kinds(m)
    bodies = [int(m.site_bodyid[m.name2id("site", s)]) for s in sites]
    pairs = HINGE80_PAIRS if name == "hinge80" else []
    words = [name, "1" if name == "hinge80" else "0", str(len(kinds))] + ["%d %d" % pk for pk in kinds]
    words += [str(len(bodies))] + [str(b) for b in bodies] + ["0", str(len(pairs))] + ["%d %d" % p for p in pairs]
    return " ".join(words)


def chain_spec_line(ndof, n_tasks):
    """A serial hinge chain of ndof links with n_tasks frame tasks (the sweep for CHAIN_LAST)."""
    words = ["sweep%d" % ndof, "0", str(ndof)] + ["%d %d" % (i, HINGE) for i in range(ndof)]
    words += [str(n_tasks)] + [str(ndof)] * n_tasks + ["0", "0"]
    return " ".join(words)


# ---- random trees past one wavefront: the draw of tests/test_gpu_random_models.py::test_random_tree with 66 … 120 bodies, as plain
# data (the device test builds the public API's tasks from it, the CPU test the oracles' specs)
TREE_SEEDS = (0, 1, 2, 3, 4, 5)
TREE_FORCE_COM = (0, 1)             # (a ComTask whatever the draw says; seed 4 draws one of its own)
TREE_B = 16
_trees = {}


def random_tree(seed, B=TREE_B):
    """dict: m, nbody, q (B, nq), frames [(name, type, cost6, gain, lm)], tg (B, n_frame, 7), post (cost, gain, target q), com (cost,
    target) or None, vel {joint name: limit}, cfg_gain, dt, damping."""
    if (seed, B) in _trees:
        return _trees[(seed, B)]
    from mink_amd.mjcf import loads_mjcf
    rng = np.random.default_rng(7000 + seed)
    nbody = int(rng.integers(66, 121))
    xml, sites = rm.random_mjcf(rng, nbody, free_root=bool(seed % 2))
    m = loads_mjcf(xml)
    q = np.stack([rm.rand_q(m, rng) for _ in range(B)])
    delta = rng.normal(scale=0.15, size=(B, m.nv))
    goal = [oik.Configuration(m, oik.Configuration(m, q[i]).integrate(delta[i], 1.0)) for i in range(B)]
    names = [(s, "site") for s in sites] + [(f"b{i}", "body") for i in range(nbody)]
    n_ft = int(rng.integers(1, 4))
    picks = [names[i] for i in rng.choice(len(names), size=min(n_ft, len(names)), replace=False)]
    frames = []
    for name, typ in picks:
        pc = rng.uniform(0.5, 20.0) * (rng.uniform(size=3) < 0.85)
        oc_ = rng.uniform(0.1, 5.0) * (rng.uniform() < 0.6)
        if not pc.any() and oc_ == 0.0:
            pc = np.ones(3)
        gain, lm = float(rng.uniform(0.3, 1.0)), float(rng.uniform(0.0, 1.0))
        frames.append((name, typ, np.concatenate([pc, np.full(3, oc_)]), gain, lm))
    tg = np.array([[g.get_transform_frame_to_world(m.name2id(typ, name), typ) for name, typ, _, _, _ in frames] for g in goal])
    post = (rng.uniform(0.05, 1.0, size=m.nv), float(rng.uniform(0.2, 1.0)))
    post += (rm.rand_q(m, rng),)
    use_com = bool(rng.uniform() < 0.4) or seed in TREE_FORCE_COM
    com = (rng.uniform(0.5, 5.0, size=3), rng.normal(scale=0.3, size=3)) if use_com else None
    vel = {}
    for j in range(m.njnt):
        if m.jnt_type[j] in (2, 3) and rng.uniform() < 0.7:
            vel[m.jnt_names[j]] = float(rng.uniform(0.5, 3.0))
    cfg_gain = float(rng.uniform(0.5, 1.0))
    dt, damping = float(rng.choice([2e-3, 1e-2, 5e-2])), float(rng.choice([1e-6, 1e-3, 1e-1]))
    _trees[(seed, B)] = {"m": m, "nbody": nbody, "q": q, "frames": frames, "tg": tg, "post": post, "com": com, "vel": vel,
                         "cfg_gain": cfg_gain, "dt": dt, "damping": damping}
    return _trees[(seed, B)]


def tree_specs(T, i):
    """(tasks, limits) of instance i for oracle/ik.py and oracle/cport.py."""
    m = T["m"]
    ts = [oik.FrameTaskSpec(m.name2id(typ, name), typ, cost, T["tg"][i, k], gain, lm) for k, (name, typ, cost, gain, lm) in enumerate(T["frames"])]
    ts.append(oik.PostureTaskSpec(T["post"][0], T["post"][2], T["post"][1]))
    if T["com"] is not None:
        ts.append(oik.ComTaskSpec(T["com"][0], T["com"][1]))
    ls = [oik.ConfigurationLimitSpec(T["cfg_gain"])]
    if T["vel"]:
        idx = np.array([int(m.jnt_dofadr[m.jnt_names.index(n)]) for n in T["vel"]])
        ls.append(oik.VelocityLimitSpec(idx, np.array(list(T["vel"].values()))))
    return ts, ls


def tree_c_oracle(T):
    from oracle import cport
    ts, ls = tree_specs(T, 0)
    ctg = T["com"][1][None, :] if T["com"] is not None else None
    return cport.CProblem(T["m"], ts, ls).solve_batch(T["q"], T["tg"], T["post"][2][None, :], T["dt"], T["damping"], com_target=ctg,
                                                      nthreads=8)


def tree_properties(m):
    """From the model's arrays: a ball joint in the middle of the tree, below a branching point (a body with a ball joint that
    has a child and an ancestor with two or more children); a body with two joints; a jointless moving body; nv > 128."""
    parent = [int(p) for p in m.body_parentid]
    nchild = [0] * m.nbody
    for b in range(1, m.nbody):
        nchild[parent[b]] += 1
    ball_mid = False
    for b in range(1, m.nbody):
        a, n = int(m.body_jntadr[b]), int(m.body_jntnum[b])
        if any(int(m.jnt_type[a + k]) == 1 for k in range(n)) and nchild[b] > 0:
            p = parent[b]
            while p > 0 and nchild[p] < 2:
                p = parent[p]
            ball_mid = ball_mid or p > 0
    return {"ball_below_branch": ball_mid, "two_joints": any(int(m.body_jntnum[b]) == 2 for b in range(1, m.nbody)),
            "jointless": any(int(m.body_jntnum[b]) == 0 for b in range(1, m.nbody)), "nv_gt_128": m.nv > 128,
            "slide_next_to_ball": any(int(m.jnt_type[int(m.body_jntadr[b])]) == 2 and int(m.body_jntnum[parent[b]]) > 0
                                      and int(m.jnt_type[int(m.body_jntadr[parent[b]])]) == 1
                                      for b in range(1, m.nbody) if int(m.body_jntnum[b]) > 0)}


# ---- collision rows on a wide-only model: hinge80
_collision = {}


def collision_case(B=B):
    """dict: m, q, tg (B, 1, 7), dt, damping — q folded (large joint angles) so that links far apart along the chain come close."""
    if B not in _collision:
        m = model("hinge80")
        rng = np.random.default_rng(SEED + 40)
        q = rng.uniform(-1.4, 1.4, size=(B, m.nq))
        tg = np.empty((B, 1, 7))
        sid = m.name2id("site", "tip")
        for i in range(B):
            cfg = oik.Configuration(m, q[i])
            cfg.update(cfg.integrate(rng.normal(scale=0.1, size=m.nv), 1.0))
            tg[i, 0] = cfg.get_transform_frame_to_world(sid, "site")
        _collision[B] = {"m": m, "q": q, "tg": tg, "dt": DT, "damping": DAMPING, "cost": np.array([1.0, 1.0, 1.0, 0.3, 0.3, 0.3])}
    return _collision[B]


def collision_specs(H80, i):
    m = H80["m"]
    tasks = [oik.FrameTaskSpec(m.name2id("site", "tip"), "site", H80["cost"], H80["tg"][i, 0], lm_damping=0.5),
             oik.PostureTaskSpec(np.full(m.nv, 0.05), np.array(m.qpos0))]
    limits = [oik.ConfigurationLimitSpec(0.95), oik.VelocityLimitSpec(np.arange(m.nv), np.full(m.nv, 1.0)),
              oik.CollisionAvoidanceLimitSpec([tuple(p) for p in HINGE80_PAIRS], collision_detection_distance=HINGE80_DETECT,
                                              minimum_distance_from_collisions=HINGE80_DMIN)]
    return tasks, limits


def collision_c_oracle(B=B):
    from oracle import cport
    H80 = collision_case(B)
    m = H80["m"]
    if "v_c" not in H80:
        H80["v_c"] = cport.CProblem(m, *collision_specs(H80, 0)).solve_batch(H80["q"], H80["tg"], np.array(m.qpos0)[None, :], H80["dt"],
                                                                            H80["damping"], nthreads=min(B, 8))
    return H80["v_c"]


# ---- the fused loops: reachable targets at very different distances (tests/test_gpu_wide.py::test_fused_loops_beyond_one_wavefront)
LOOP_SCALES = (2e-4, 2e-3, 0.02, 0.2)
LOOP_STEPS, LOOP_MAX_ITERS, LOOP_THRESHOLDS = 3, 6, (2e-3, 2e-3)
_loops = {}


def loop_case(name, B=B):
    """(P, q, qt, tg): tg the frames' poses at qt = q ⊕ δ, δ ~ N(0, 1)·scale with the four scales spread over the batch; qt is also
    the posture target of the threshold-terminated loop (consistent targets)."""
    if (name, B) not in _loops:
        P, q, _, _ = case(name, B)
        m = P["m"]
        rng = np.random.default_rng(4)
        scale = np.repeat(LOOP_SCALES, B // 4)[:, None]
        delta = rng.normal(size=(B, m.nv)) * scale
        qt = np.stack([oik.Configuration(m, q[i]).integrate(delta[i], 1.0) for i in range(B)])
        tg = np.array([[oik.Configuration(m, qt[i]).get_transform_frame_to_world(m.name2id(t, n), t) for n, t, _, _, _ in P["frames"]]
                       for i in range(B)])
        _loops[(name, B)] = (P, q, qt, tg)
    return _loops[(name, B)]


def oracle_loop(P, q_i, tg_i, pt_i, max_iters, thresholds):
    """The callers' loop (solve, integrate, stop when every frame task is within the thresholds) on the numpy oracle →
    (q, iterations, converged)."""
    m = P["m"]
    cfg = oik.Configuration(m, q_i)
    tasks, limits = qc.oracle_specs(P, tg_i, pt_i)
    n, done = 0, False
    for n in range(1, max_iters + 1):
        v = oik.solve_ik(m, cfg, tasks, P["dt"], P["damping"], limits)
        cfg.update(cfg.integrate(v, P["dt"]))
        errs = [oik.task_error_jacobian(cfg, t)[0] for t in tasks if isinstance(t, oik.FrameTaskSpec)]
        if all(np.linalg.norm(e[:3]) <= thresholds[0] and np.linalg.norm(e[3:]) <= thresholds[1] for e in errs):
            done = True
            break
    return cfg.q.copy(), n, done
