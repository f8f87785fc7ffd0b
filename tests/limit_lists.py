"""Lists of limits and posture tasks: terms, inputs and reference of tests/test_gpu_limit_lists.py, device-free (numpy oracle only),
so that the conditions on the inputs are checked on the CPU (tests/test_limit_lists_cpu.py) before a kernel sees them.

One list, defined once and cut per model (L: the model's limited dofs in dof order; D: every dof that is not a free joint's):

  cfg0  gain 0.95, every limited joint
        (the last limited hinge / slide dof is left out of cfg1 and cfg2: on the other dofs one of those two is always the tighter
        — cfg1 by its gain and margin, cfg2 wherever the band lies inside the range — and cfg0, with its copy cfg3, would never bind)
  cfg1  gain 0.5, min_distance_from_limits 0.02, the odd entries of L (not joints narrower than 0.1: 2 x 0.02 would close them)
  cfg2  gain 1.0, lower / upper overridden to reference posture -/+ BAND, the even entries of L
  cfg3  a copy of cfg0
  vel0  every dof of D at 0.3
  vel1  the first half of D at 0.5, one of them at exactly 0.0: lo = hi = 0, a frozen dof
  vel2  the second half of D at 0.2
  vel3  one dof at 0.05: tighter than every other term

A limited ball joint keeps its three dofs together and goes to cfg1 with the joint's range itself in its four qpos slots, not the
range narrowed by the margin: the reference differentiates against the quaternion (u, u, u, u), whose direction does not depend on
u > 0, so a margin would turn lower and upper into the same rotation and pin the step, lo = hi up to rounding — on the
inconsistency gate by construction.  With lower = 0 the lower bound is 0 and the upper one is gain x X, X the rotation left to
(u, u, u, u): the joint sits in cfg0 (0.95) and cfg1 (0.5), and cfg1's is the tighter, which binds once X is small.  (A band of
its own for a ball joint would need four different slot values; the device holds one value per dof and refuses such a
descriptor.)  Its dofs are in the second half of D: vel0 and vel2.  `balllimit` is the model of tests/golden/ik_balllimit.npz with
inputs sampled here like every other family's (the fixture's 16 instances meet none of the conditions below).  Every problem carries two posture tasks with their own target slots: a DampingTask
(a PostureTask with gain 0) and a PostureTask with a cost per dof and a target per instance."""

import functools
import os

import numpy as np

import oracle_configs as oc
import random_models as rm
from mink_amd.flatmodel import FlatModel
from oracle import ik as oik
from oracle import qp_gi

COUNTS = [(2, 2), (4, 4), (3, 0), (0, 3)]
BAND, DT = 0.4, 5e-2
ST_OUTSIDE, ST_INFEASIBLE = 1, 2


def _scene(name):
    return FlatModel.load(os.path.join(oc.GOLDEN, "models", "all", name + ".json"))


def _chain70():
    from mink_amd import mjcf
    xml, sites = rm.chain_mjcf(70, seed=3)
    return mjcf.loads_mjcf(xml), sites


def _humanoid_frames(hands):
    return [("site", s, 200.0, 10.0, 1.0) for s in ("left_foot", "right_foot")] + [("site", s, 200.0, 0.0, 1.0) for s in hands]


# name → model, frame tasks (type, name, position cost, orientation cost, lm_damping), keyframe of the reference posture, batch,
# damping, base posture cost, and how many instances go to the oracle
FAMILIES = {
    "ur5e": dict(model=lambda: oc.model("ur5e"), frames=[("site", "attachment_site", 1.0, 1.0, 1.0)], key="home", B=67, damping=1e-3,
                 pcost=1e-2),
    "leap": dict(model=lambda: _scene("leap_hand__scene_right"), frames=[("site", s, 1.0, 0.0, 1.0) for s in ("tip_1", "tip_2", "tip_3", "th_tip")],
                 key=None, B=35, damping=1e-3, pcost=1e-2),
    "h1": dict(model=lambda: _scene("unitree_h1__scene"), frames=_humanoid_frames(("left_wrist", "right_wrist")), key="stand", B=35,
               damping=1e-1, pcost=1.0),
    "g1": dict(model=lambda: oc.model("g1"), frames=_humanoid_frames(("left_palm", "right_palm")), key="stand", B=70, damping=1e-1,
               pcost=1.0, sample=16),
    "balllimit": dict(model=lambda: oc.model("balllimit"), frames=[("site", "tip", 2.0, 0.5, 0.1)], key=None, ref=lambda m: _ball_reference(m),
                      B=32, damping=1e-4, pcost=0.1),
    "chain70": dict(model=lambda: _chain70()[0], frames=[("site", s, 1.0, 0.3, 0.5) for s in ("s24", "s49", "s69")], key=None, B=12,
                    damping=1e-4, pcost=5e-2),
}


BALL_AXIS = np.ones(3) / np.sqrt(3.0)


BALL_END = 2.0 * np.pi / 3.0        # the rotation the quaternion (u, u, u, u) stands for: 120 degrees about (1, 1, 1)


def _ball_reference(m):
    """`balllimit`'s reference posture: the fixture's hinge, the slide at -0.1 (the band's upper end, 0.3, then lies inside its
    range), and the limited ball joint turned 1.8 rad about (1, 1, 1): its w inside the joint's range [0, 0.8] as the reference's
    check_limits reads it, and 0.29 rad short of BALL_END, so that the upper bounds on its three dofs are positive."""
    q = np.array(m.qpos0, dtype=np.float64)
    q[int(m.jnt_qposadr[m.name2id("joint", "hinge")])] = 0.2
    q[int(m.jnt_qposadr[m.name2id("joint", "slide")])] = -0.1
    v = np.zeros(m.nv)
    a = int(m.jnt_dofadr[m.name2id("joint", "ball2")])
    v[a:a + 3] = 1.8 * BALL_AXIS
    return oik.Configuration(m, q).integrate(v, 1.0)


@functools.lru_cache(maxsize=None)
def model_of(family):
    return FAMILIES[family]["model"]()


def reference_posture(m, key):
    return np.array(m.qpos0 if key is None else m.key_qpos[m.name2id("key", key)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ the list
def dof_sets(m):
    """L, D, and per dof: joint id, qpos address, joint type, range width (inf: not limited)."""
    L = [int(d) for d in oik.configuration_limit_arrays(m, oik.ConfigurationLimitSpec())[0]]
    jid = np.zeros(m.nv, dtype=int)
    for j in range(m.njnt):
        jid[int(m.jnt_dofadr[j]):int(m.jnt_dofadr[j]) + oik._DW[int(m.jnt_type[j])]] = j
    D = [d for d in range(m.nv) if m.jnt_type[jid[d]] != oik.JNT_FREE]
    return L, D, jid


def plain_dof(m):
    """The last limited hinge / slide dof: in cfg0 (and its copy cfg3) alone.  None on a model with fewer than four such dofs."""
    L, _, jid = dof_sets(m)
    scalar = [d for d in L if m.jnt_type[jid[d]] != 1]
    return scalar[-1] if len(scalar) >= 4 else None


def subsets(m):
    """(odd, even) of L as cfg1 / cfg2 take them."""
    L, _, jid = dof_sets(m)
    ball = [d for d in L if m.jnt_type[jid[d]] == 1]
    scalar = [d for d in L if m.jnt_type[jid[d]] != 1 and d != plain_dof(m)]
    width = lambda d: float(m.jnt_range[jid[d], 1] - m.jnt_range[jid[d], 0])
    if len(scalar) < 4:        # (two or three such dofs: cfg2 takes them all, cfg1 the ball joints alone; cfg0 binds at a range end
        return ball, scalar    #  outside the band)
    return sorted([d for d in scalar[1::2] if width(d) >= 0.1] + ball), scalar[0::2]


def frozen_dof(m):
    """The dof vel1 freezes: the first one of its half that a tightened configuration term (cfg1, else cfg2) names too."""
    _, D, _ = dof_sets(m)
    odd, even = subsets(m)
    half = D[:len(D) // 2]
    return next((d for d in half if d in odd), next((d for d in half if d in even), None))


def tight_dof(m):
    """vel3's dof: the second half's first dof that cfg2 bounds; on a model with fewer than four limited hinge / slide dofs, where
    that one is all the band has left to bind on beside the frozen dof, the half's first dof outside cfg2."""
    _, D, jid = dof_sets(m)
    _, even = subsets(m)
    half = D[len(D) // 2:]
    return next(d for d in half if (d in even) == (plain_dof(m) is not None))


def limit_list(m, q_ref):
    """All eight terms: ([(name, oracle spec, native descriptor)] for cfg0..3, the same for vel0..3)."""
    L, D, jid = dof_sets(m)
    odd, even = subsets(m)
    qadr = lambda d: int(m.jnt_qposadr[jid[d]])
    cfg, vel = [], []

    def add_cfg(name, spec):
        idx, lower, upper = oik.configuration_limit_arrays(m, spec)
        cfg.append((name, spec, {"gain": spec.gain, "lower": lower, "upper": upper, "indices": idx}))

    add_cfg("cfg0", oik.ConfigurationLimitSpec(0.95))
    _, lower, upper = oik.configuration_limit_arrays(m, oik.ConfigurationLimitSpec(0.5, 0.02))
    for j in range(m.njnt):                              # a ball joint's slots: the range itself (see the module's docstring)
        if m.jnt_type[j] == 1 and m.jnt_limited[j]:
            a = int(m.jnt_qposadr[j])
            lower[a:a + 4], upper[a:a + 4] = m.jnt_range[j, 0], m.jnt_range[j, 1]
    add_cfg("cfg1", oik.ConfigurationLimitSpec(0.5, 0.02, lower=lower, upper=upper, indices=np.array(odd)))
    _, lower, upper = oik.configuration_limit_arrays(m, oik.ConfigurationLimitSpec())
    for d in even:
        lower[qadr(d)], upper[qadr(d)] = q_ref[qadr(d)] - BAND, q_ref[qadr(d)] + BAND
    add_cfg("cfg2", oik.ConfigurationLimitSpec(1.0, lower=lower, upper=upper, indices=np.array(even)))
    add_cfg("cfg3", oik.ConfigurationLimitSpec(0.95))

    def add_vel(name, idx, lim):
        idx, lim = np.array(idx, dtype=np.int64), np.array(lim, dtype=np.float64)
        vel.append((name, oik.VelocityLimitSpec(idx, lim), {"indices": idx, "limit": lim}))

    half = len(D) // 2
    add_vel("vel0", D, np.full(len(D), 0.3))
    add_vel("vel1", D[:half], [0.0 if d == frozen_dof(m) else 0.5 for d in D[:half]])
    add_vel("vel2", D[half:], np.full(len(D) - half, 0.2))
    add_vel("vel3", [tight_dof(m)], [0.05])
    return cfg, vel


def folded_velocity(m, vel):
    """The velocity terms as ONE term of per-dof minima (native descriptor)."""
    v = np.full(m.nv, np.inf)
    for _, _, d in vel:
        np.minimum.at(v, d["indices"], d["limit"])
    idx = np.flatnonzero(np.isfinite(v))
    return {"indices": idx, "limit": v[idx]}


# -------------------------------------------------------------------------------------------------------------------- inputs
class Case:
    """One family's inputs: model, q (B, nq), frame targets (B, F, 7), posture targets (B, 2, nq), the two posture tasks, the
    list, and which instances were built to be infeasible under vel1 / outside the model's range."""


@functools.lru_cache(maxsize=None)
def case(family):
    c = Case()
    c.family = family
    m = c.m = model_of(family)
    rng = np.random.default_rng(sum(map(ord, family)))
    L, D, jid = dof_sets(m)
    odd, even = subsets(m)
    f = FAMILIES[family]
    c.frames, c.B, c.damping, pcost = f["frames"], f["B"], f["damping"], f["pcost"]
    c.sample = f.get("sample", c.B)
    c.q_ref = f["ref"](m) if "ref" in f else reference_posture(m, f["key"])
    c.q, c.tg, c.made_infeasible, c.made_outside, pulls = _sample_inputs(c, rng)
    B = c.B
    c.dt = DT
    c.frame_ids = [(t, m.name2id(t, n)) for t, n, _, _, _ in c.frames]
    c.frame_cost = [np.array([p] * 3 + [o] * 3) for _, _, p, o, _ in c.frames]
    # DampingTask, then a PostureTask with a cost per dof and a target per instance
    c.post = [dict(cost=np.full(m.nv, 0.3 * pcost), gain=0.0, lm_damping=0.0),
              dict(cost=pcost * rng.uniform(0.5, 1.5, size=m.nv), gain=1.0, lm_damping=0.0)]
    c.pt = np.empty((B, 2, m.nq))
    c.pt[:, 0] = c.q_ref
    for i in range(B):
        c.pt[i, 1] = oik.Configuration(m, c.q_ref).integrate(rng.normal(scale=0.05, size=m.nv) * np.isin(np.arange(m.nv), D), 1.0)
    for i, a, sign in pulls:                             # the posture target pulls the same way as the frame targets push
        c.pt[i, 1, a] = c.q[i, a] + 0.3 * sign
    c.cfg, c.vel = limit_list(m, c.q_ref)
    return c


def _sample_inputs(c, rng):
    """q inside the band and the ranges, then per instance one odd dof close enough to a range end for cfg1 to bind and one even dof
    close enough to the band (or the range, where that is nearer) for cfg2 / cfg0 to bind; targets = FK(q + delta) with delta
    pushing those two outwards.  Three instances put the frozen dof where a tightened term excludes a zero step (infeasible
    under vel1, inside the model's range: no MKH_ST_OUTSIDE_LIMITS); two put a dof 2e-3 outside its range (that bit, still
    solved)."""
    m, B = c.m, c.B
    L, D, jid = dof_sets(m)
    odd, even = subsets(m)
    qadr = lambda d: int(m.jnt_qposadr[jid[d]])
    rlo = lambda d: float(m.jnt_range[jid[d], 0]) if m.jnt_limited[jid[d]] else -np.pi
    rhi = lambda d: float(m.jnt_range[jid[d], 1]) if m.jnt_limited[jid[d]] else np.pi
    q = np.tile(c.q_ref, (B, 1))
    delta = rng.normal(scale=0.15, size=(B, m.nv))
    for j in range(m.njnt):
        if m.jnt_type[j] == oik.JNT_FREE:
            delta[:, int(m.jnt_dofadr[j]):int(m.jnt_dofadr[j]) + 6] *= 0.2
    scalar = lambda ds: [d for d in ds if m.jnt_type[jid[d]] in (2, 3)]
    for d in scalar(D):
        lo, hi = rlo(d), rhi(d)
        w = hi - lo
        a, b = max(lo + 0.05 * w, c.q_ref[qadr(d)] - 0.8 * BAND), min(hi - 0.05 * w, c.q_ref[qadr(d)] + 0.8 * BAND)
        if a >= b:
            a, b = lo + 0.05 * w, hi - 0.05 * w
        q[:, qadr(d)] = rng.uniform(a, b, size=B)
    wide = lambda ds: [d for d in scalar(ds) if rhi(d) - rlo(d) >= 0.2]
    fz = frozen_dof(m)
    pulls = []
    made_infeasible = sorted({5 % B, B // 2, B - 1})
    made_outside = sorted({7 % B, B - 2} - set(made_infeasible))
    for i in range(B):
        for d1 in [int(rng.choice(x)) for x in [[d for d in wide(odd) if d != fz]] if x]:
            if d1 in set(wide(even)) and i % 2 == 1:
                continue
            up = rng.uniform() < 0.5
            u = rng.uniform(0.021, 0.04)
            q[i, qadr(d1)] = rhi(d1) - u if up else rlo(d1) + u
            delta[i, d1] = 0.3 if up else -0.3
            pulls.append((i, qadr(d1), 1.0 if up else -1.0))
        both = set(wide(odd)) & set(wide(even)) - {fz}      # (a dof in cfg1 and cfg2: near its range on even instances, the band on odd)
        for d2 in [int(rng.choice(x)) for x in [[d for d in wide(even) if d != fz and (d not in both or i % 2 == 1)]] if x]:
            up = rng.uniform() < 0.5
            if d2 in both:                                   # (the band's end that lies inside the range: the other is cfg1's)
                up = c.q_ref[qadr(d2)] + BAND < rhi(d2)
            edge = min(rhi(d2), c.q_ref[qadr(d2)] + BAND) if up else max(rlo(d2), c.q_ref[qadr(d2)] - BAND)
            u = rng.uniform(0.002, 0.012)
            q[i, qadr(d2)] = edge - u if up else edge + u
            delta[i, d2] = 0.3 if up else -0.3
            pulls.append((i, qadr(d2), 1.0 if up else -1.0))
        # ball joints: an unlimited one anywhere near its reference; a limited one turned about (1, 1, 1) — every other instance to
        # within sqrt(3) x [0.004, 0.018] of BALL_END and pushed on, where cfg1's bound (gain 0.5) on its three dofs is below every
        # velocity bound and cfg0's (0.95) is not the tighter; the others well short of it and pushed at random (a push backwards
        # meets the lower bound, which the reference's arithmetic puts at 0 in every term)
        for j in range(m.njnt):
            if m.jnt_type[j] != 1:
                continue
            a, va = int(m.jnt_qposadr[j]), int(m.jnt_dofadr[j])
            v = np.zeros(m.nv)
            if not m.jnt_limited[j]:
                v[va:va + 3] = rng.normal(scale=0.2, size=3)
            elif i in made_outside and plain_dof(m) is None:     # 1.2 rad: w = cos(0.6) beyond the range's 0.8
                v[va:va + 3] = -0.6 * BALL_AXIS
            elif i % 2 == 1:
                v[va:va + 3] = (BALL_END - 1.8 - np.sqrt(3.0) * rng.uniform(0.004, 0.018)) * BALL_AXIS + rng.normal(scale=3e-4, size=3)
                delta[i, va:va + 3] = 0.3
            else:
                v[va:va + 3] = rng.uniform(-0.2, 0.15) * BALL_AXIS + rng.normal(scale=0.02, size=3)
            q[i, a:a + 4] = oik.Configuration(m, c.q_ref).integrate(v, 1.0)[a:a + 4]
        if i % 2 == 0 and plain_dof(m) is not None:                                   # every other instance: the dof of cfg0 / cfg3 alone, near its range
            d3, up = plain_dof(m), rng.uniform() < 0.5
            u = rng.uniform(2e-5, 8e-5)              # (G1's Levenberg-Marquardt terms leave a posture pull steps of 1e-4)
            q[i, qadr(d3)] = rhi(d3) - u if up else rlo(d3) + u
            delta[i, d3] = 0.3 if up else -0.3
            pulls.append((i, qadr(d3), 1.0 if up else -1.0))
    for i in made_infeasible:
        if fz in odd:
            q[i, qadr(fz)] = rhi(fz) - 0.01            # inside the range, 0.01 inside cfg1's margin: its upper bound is -0.005
        else:                                          # (cfg2 only from the third term on: 0.01 beyond the range, cfg0's bound -0.0095)
            q[i, qadr(fz)] = rhi(fz) + 0.01
    for i in made_outside:                               # (the dof of cfg0 alone: no band to be outside of as well)
        if plain_dof(m) is not None:
            q[i, qadr(plain_dof(m))] = rhi(plain_dof(m)) + 2e-3
    tg = np.empty((B, len(c.frames), 7))
    for i in range(B):
        cfg = oik.Configuration(m, q[i])
        cfg.update(cfg.integrate(delta[i], 1.0))
        for k, (t, n, _, _, _) in enumerate(c.frames):
            tg[i, k] = cfg.get_transform_frame_to_world(m.name2id(t, n), t)
    return q, tg, made_infeasible, made_outside, pulls


# ----------------------------------------------------------------------------------------------------------------- reference
def native_tasks(c):
    fts = [{"frame_type": t, "frame_id": fid, "cost": list(cost), "gain": 1.0, "lm_damping": lm}
           for (t, fid), cost, (_, _, _, _, lm) in zip(c.frame_ids, c.frame_cost, c.frames)]
    return fts, [dict(p) for p in c.post]


def oracle_tasks(c, i):
    tasks = [oik.FrameTaskSpec(fid, t, cost, c.tg[i, k], lm_damping=lm)
             for k, ((t, fid), cost, (_, _, _, _, lm)) in enumerate(zip(c.frame_ids, c.frame_cost, c.frames))]
    tasks += [oik.PostureTaskSpec(p["cost"], c.pt[i, k], p["gain"], p["lm_damping"]) for k, p in enumerate(c.post)]
    return tasks


def terms_of(c, n_cfg, n_vel):
    return c.cfg[:n_cfg] + c.vel[:n_vel]


def box_of_rows(G, h, nv):
    """The stacked rows reduced per dof: min of h over +e_d rows, max of -h over -e_d rows."""
    lo, hi = np.full(nv, -np.inf), np.full(nv, np.inf)
    for r in range(len(h)):
        k = np.flatnonzero(G[r])
        assert len(k) == 1 and abs(G[r, k[0]]) == 1.0
        if G[r, k[0]] > 0:
            hi[k[0]] = min(hi[k[0]], h[r])
        else:
            lo[k[0]] = max(lo[k[0]], -h[r])
    return lo, hi


class Ref:
    """What the numpy oracle says about `rows` of a case under a term list: v (NaN where its QP raises "constraints are
    inconsistent"), status, the box, the bounds active at the solution per term, and the witness figures."""


def solve_one(c, i, terms, extra=()):
    m = c.m
    cfg = oik.Configuration(m, c.q[i])
    st = ST_OUTSIDE if cfg.limit_violations() else 0
    limits = [s for _, s, _ in terms] + list(extra)
    try:
        v, (_, _, G, h) = oik.solve_ik(m, cfg, oracle_tasks(c, i), c.dt, c.damping, limits, return_problem=True)
    except qp_gi.Infeasible as e:
        assert "inconsistent" in str(e), e
        _, _, G, h = oik.build_ik(cfg, oracle_tasks(c, i), c.dt, c.damping, limits)
        return np.full(m.nv, np.nan), st | ST_INFEASIBLE, G, h
    return v, st, G, h


@functools.lru_cache(maxsize=None)
def reference(family, n_cfg, n_vel):
    c = case(family)
    m, terms = c.m, terms_of(case(family), n_cfg, n_vel)
    r = Ref()
    r.rows = list(range(c.B)) if c.sample >= c.B else sorted(set(np.linspace(0, c.B - 1, c.sample).astype(int)) | set(c.made_infeasible) | set(c.made_outside))
    n = len(r.rows)
    r.v, r.st = np.empty((n, m.nv)), np.zeros(n, dtype=np.int32)
    r.lo, r.hi = np.empty((n, m.nv)), np.empty((n, m.nv))
    r.active = {name: np.zeros(n, dtype=int) for name, _, _ in terms}       # bounds of that term the solution sits on
    r.on_bound = np.zeros(n, dtype=int)
    rows_of = []
    for k, i in enumerate(r.rows):
        r.v[k], r.st[k], G, h = solve_one(c, i, terms)
        nbox = sum(2 * len(d["indices"]) for _, _, d in terms)
        r.lo[k], r.hi[k] = box_of_rows(G[:nbox], h[:nbox], m.nv)
        if r.st[k] & ST_INFEASIBLE:
            continue
        dq = r.v[k] * c.dt
        tol = 1e-10 * max(1.0, np.abs(dq).max())
        r.on_bound[k] = int(((np.abs(dq - r.hi[k]) <= tol) | (np.abs(dq - r.lo[k]) <= tol)).sum())
        at = 0
        for name, _, d in terms:
            rows = slice(at, at + 2 * len(d["indices"]))
            at = rows.stop
            r.active[name][k] = int((np.abs(G[rows] @ dq - h[rows]) <= tol).sum())
    # witness: for every term t >= 1, instances where one of its bounds is active — and what dropping it does to v there
    # (cfg3 is cfg0 again, row for row: alone it can move nothing, so the pair is dropped together)
    r.witness = {}
    for t, (name, _, _) in enumerate(terms):
        if name in ("cfg0", "vel0"):
            continue
        twin = "cfg0" if name == "cfg3" else None
        rest = [x for x in terms if x[0] not in (name, twin)]
        hits = [k for k in range(n) if r.active[name][k] > 0 and not (r.st[k] & ST_INFEASIBLE)]
        moved = []
        for k in hits[:16]:              # (a bound another term repeats — a ball joint's lower bound of 0 — is active and moves nothing)
            v2, st2, _, _ = solve_one(c, r.rows[k], rest)
            moved.append(float(np.abs(v2 - r.v[k]).max() / max(1.0, np.abs(r.v[k]).max())) if not (st2 & ST_INFEASIBLE) else np.inf)
            if sum(1 for x in moved if x > 1e-4) >= 4:
                break
        r.witness[name] = (len(hits), moved)
    return r


def check_conditions(family, n_cfg, n_vel, r=None):
    """The conditions on the inputs, from the oracle alone.  Returns the figures it asserted."""
    c = case(family)
    r = r or reference(family, n_cfg, n_vel)
    feasible = (r.st & ST_INFEASIBLE) == 0
    for name, (hits, moved) in r.witness.items():
        assert hits >= 4, (family, n_cfg, n_vel, name, hits)
        assert sum(1 for x in moved if x > 1e-4) >= 4, (family, n_cfg, n_vel, name, moved)
    assert (r.on_bound[feasible] >= 2).sum() * 2 >= len(r.rows), (family, r.on_bound)
    # no dof sits on the device's inconsistency gate lo > hi + 1e-12: |hi - lo| > 1e-9 everywhere but on the frozen dof (exactly 0)
    gap = np.abs(r.hi - r.lo)
    fz = frozen_dof(c.m)
    for k in range(len(r.rows)):
        for d in range(c.m.nv):
            if n_vel >= 2 and d == fz and r.lo[k, d] <= 0.0 <= r.hi[k, d]:
                assert r.lo[k, d] == 0.0 and r.hi[k, d] == 0.0
            else:
                assert gap[k, d] > 1e-9, (family, r.rows[k], d, r.lo[k, d], r.hi[k, d])
    # a frozen dof next to a tightened configuration term is the one way these lists become inconsistent: velocity terms alone
    # contain the zero step, and configuration terms alone would need a band within 5 % of a range end (gain 0.95 against 1.0)
    n_inf = int((~feasible).sum())
    if n_cfg >= 2 and n_vel >= 2 and c.made_infeasible:
        assert n_inf >= 1
        assert all((r.st[r.rows.index(i)] & ST_INFEASIBLE) != 0 for i in c.made_infeasible)
    else:
        assert n_inf == 0
    assert feasible.sum() * 4 >= 3 * len(r.rows)
    return {"infeasible": n_inf, "on_bound_mean": float(r.on_bound[feasible].mean()),
            "active": {k: int(v.sum()) for k, v in r.active.items()}, "witness": {k: (h, min(mv) if mv else None) for k, (h, mv) in r.witness.items()}}
