"""The inputs of the tests of swept clearance and checked ladders on checkers WITH general convex pairs
(tests/test_swept_convex_cpu.py, tests/test_gpu_swept_convex.py), and their references by tests/swept_ref.py and
tests/ladder_free_ref.py — computed once per process and handed out read-only.

The robots' fixtures do not exercise this: on `ur5e_convex` the cylinder-box pair decides one random edge in fifty.  `convex_shapes`
is a model made for it, in the manner of clearance_ref.shapes_mjcf: twelve bodies on one level in a small cube, cylinders, boxes,
ellipsoids and capsules, and a pair list in which the pairs without an analytic routine and the analytic ones interleave."""

import numpy as np

import clearance_ref as cr
import ladder_free_ref as lfref
import swept_ref as sref

_cache = {}

# ---- `convex_shapes`
N_ROWS, BODIES, SPREAD, SEED = 64, 12, 0.4, 11   # (side 0.3 with this pair list: every one of the 32 edges collides)
TYPES = ["cylinder", "box", "ellipsoid", "capsule"]          # of body i % 4
# (body, body) in pair-list order and whether the pair goes through the general convex routine
PAIRS = [(0, 1, True),      # cylinder-box
         (3, 5, False),     # capsule-box
         (0, 4, True),      # cylinder-cylinder
         (1, 5, False),     # box-box
         (2, 9, True),      # ellipsoid-box
         (3, 7, False),     # capsule-capsule
         (6, 8, True),      # ellipsoid-cylinder
         (11, 4, False),    # capsule-cylinder
         (10, 7, True),     # ellipsoid-capsule
         (2, 6, True),      # ellipsoid-ellipsoid
         (8, 9, True),      # cylinder-box
         (5, 9, False),     # box-box
         (10, 0, True),     # ellipsoid-cylinder
         (11, 1, False),    # capsule-box
         (4, 5, True)]      # cylinder-box
N_SAMPLES, N_EDGES = 3, 32                                    # the edges: row i -> row i + 32


def family(k):
    """The two geom types of pair k, sorted: "cylinder-box"."""
    a, b, _ = PAIRS[k]
    order = ["capsule", "ellipsoid", "cylinder", "box"]
    return "-".join(sorted([TYPES[a % 4], TYPES[b % 4]], key=order.index))


def shapes_mjcf(seed=SEED):
    """BODIES bodies, all children of the world, scattered in a cube of side SPREAD, each with one joint (hinge ±1.5 rad or
    slide ±0.15 m about a random axis) and one randomly turned geom of TYPES."""
    rng = np.random.default_rng(seed)
    xml = ['<mujoco><compiler angle="radian"/><worldbody>']
    for i in range(BODIES):
        ax, qt = rng.normal(size=3), rng.normal(size=4)
        ax, qt = ax / np.linalg.norm(ax), qt / np.linalg.norm(qt)
        pos = rng.uniform(-0.5 * SPREAD, 0.5 * SPREAD, size=3) + np.array([0.0, 0.0, 0.5])
        typ = TYPES[i % 4]
        size = {"box": rng.uniform(0.03, 0.08, size=3), "capsule": np.array([rng.uniform(0.02, 0.04), rng.uniform(0.04, 0.1)]),
                "ellipsoid": rng.uniform(0.03, 0.08, size=3), "cylinder": np.array([rng.uniform(0.03, 0.05), rng.uniform(0.03, 0.08)])}[typ]
        joint = ('type="hinge" range="-1.5 1.5"' if i % 2 else 'type="slide" range="-0.15 0.15"')
        xml.append(f'<body name="s{i}" pos="{pos[0]:.4f} {pos[1]:.4f} {pos[2]:.4f}">'
                   f'<joint name="sj{i}" {joint} axis="{ax[0]:.5f} {ax[1]:.5f} {ax[2]:.5f}"/>'
                   f'<geom name="g{i}" type="{typ}" size="{" ".join("%.4f" % x for x in size)}" '
                   f'quat="{qt[0]:.5f} {qt[1]:.5f} {qt[2]:.5f} {qt[3]:.5f}" pos="0.03 0.02 -0.01" mass="0.1"/></body>')
    xml.append("</worldbody></mujoco>")
    return "".join(xml)


def shapes():
    """(model, [CollisionAvoidanceLimit kwargs], q_rows (N_ROWS, nq)) of `convex_shapes`: minimum distance 0, detection 0.25."""
    if "shapes" not in _cache:
        from mink_amd.mjcf import loads_mjcf
        model = loads_mjcf(shapes_mjcf())
        gid = lambda i: model.name2id("geom", "g%d" % i)
        spec = [dict(geom_pairs=[([gid(a)], [gid(b)]) for a, b, _ in PAIRS], minimum_distance_from_collisions=0.0,
                     collision_detection_distance=0.25)]
        q = cr._uniform_in_ranges(model, np.random.default_rng(3), N_ROWS)
        q.setflags(write=False)
        _cache["shapes"] = (model, spec, q)
    return _cache["shapes"]


def limit_objects(model, spec):
    import mink_amd
    return [mink_amd.CollisionAvoidanceLimit(model, **kw) for kw in spec]


def _frozen(ref):
    for a in ref:
        a.setflags(write=False)
    return ref


def shapes_sweep():
    """(q_from, q_to, RefSweep, distances (N_EDGES, N_SAMPLES, n_pairs)) of the N_EDGES edges at N_SAMPLES samples."""
    if "shapes_sweep" not in _cache:
        model, spec, q = shapes()
        limits = cr.limits_of(limit_objects(model, spec))
        a, b = q[:N_EDGES], q[N_EDGES:2 * N_EDGES]
        rows = np.concatenate([sref.sample_rows(model, a[e], b[e], N_SAMPLES) for e in range(N_EDGES)])
        dist = cr.distances(model, limits, rows)
        dist.setflags(write=False)
        per = cr.from_distances(dist, cr.pair_list(limits)[1])
        m, p = per.margin.reshape(N_EDGES, N_SAMPLES), per.pair.reshape(N_EDGES, N_SAMPLES)
        s = m.argmin(axis=1).astype(np.int32)
        e = np.arange(N_EDGES)
        ref = _frozen(sref.RefSweep(m[e, s], s, p[e, s].astype(np.int32), ~(m[e, s] >= 0.0), m))
        _cache["shapes_sweep"] = (a, b, ref, dist.reshape(N_EDGES, N_SAMPLES, -1))
    return _cache["shapes_sweep"]


def separated(ref):
    """Which edges of a reference decide away from a tie (tests/test_gpu_swept.py's rule): the smallest sample's margin more than
    1e-6 from zero and, with more than one sample, more than 1e-6 below the runner-up."""
    ok = np.abs(ref.margin) > 1e-6
    if ref.samples.shape[1] > 1:
        order = np.sort(ref.samples, axis=1)
        ok &= order[:, 1] - order[:, 0] > 1e-6
    return ok


def keep(ref, dropped, at_least):
    """The kept edges of a reference; the number of dropped candidates is pinned, at most a quarter, and enough are left."""
    ok = separated(ref)
    assert int((~ok).sum()) == dropped, (np.nonzero(~ok)[0], dropped)
    assert 4 * dropped <= len(ok) and int(ok.sum()) >= at_least, (dropped, len(ok), at_least)
    return np.nonzero(ok)[0]


def shapes_ref():
    """RefClearance of the fixture's rows."""
    if "shapes_ref" not in _cache:
        model, spec, q = shapes()
        _cache["shapes_ref"] = _frozen(cr.clearance(model, cr.limits_of(limit_objects(model, spec)), q))
    return _cache["shapes_ref"]


# ---- `ur5e_convex`: the real robot's chain depth; pair 1, the wrist cylinder against the box wall, is the general convex one
UR5E_CONVEX_PAIR = 1


def ur5e_convex_edges():
    """(q_from, q_to, RefSweep at ONE sample) between neighbours in the list of the fixture rows whose cylinder-box distance is in
    range (below the detection distance): blends of two random postures move away from the wall, two such rows less so."""
    if "ur5e" not in _cache:
        model, _, q = cr.fixture("ur5e_convex")
        limits = cr.limits_of(cr.fixture_limits("ur5e_convex"))
        near = np.nonzero(cr.fixture_ref("ur5e_convex").distance[:, UR5E_CONVEX_PAIR] < cr.pair_list(limits)[2][UR5E_CONVEX_PAIR])[0]
        a, b = np.ascontiguousarray(q[near[:-1]]), np.ascontiguousarray(q[near[1:]])
        _cache["ur5e"] = (a, b, _frozen(sref.sweep(model, limits, a, b, 1)))
    return _cache["ur5e"]


# ---- a free joint carrying general convex pairs: the floating body of tests/test_gpu_quat_joints.py's fixture
FLOATING_CANS = """<mujoco><compiler angle="radian"/><worldbody>
  <geom name="crate" type="box" size=".1 .2 .2" pos="0.4 0 0" quat="0.98 0.1 0.05 0.1"/>
  <geom name="drum" type="cylinder" size=".1 .2" pos="-0.4 0 0" quat="0.95 0.2 0.1 0"/>
  <geom name="crate2" type="box" size=".2 .2 .1" pos="0 0 0.5" quat="0.97 0.05 0.2 0.1"/>
  <geom name="drum2" type="cylinder" size=".1 .2" pos="0 0.4 0" quat="0.7 0 0.7 0.1"/>
  <body name="base" pos="0 0 0"><freejoint name="root"/>
    <inertial pos="0 0 0" mass="1" diaginertia="1 1 1"/>
    <geom name="l_can" type="cylinder" size=".03 .04" pos="0.08 0 0" quat="1 0 1 0"/>
    <geom name="r_can" type="cylinder" size=".03 .04" pos="-0.08 0 0" quat="1 1 0 0"/>
    <body name="arm" pos="0 0 0.1"><joint name="elbow" type="hinge" axis="0 1 0" range="-1.5 1.5"/>
      <inertial pos="0 0 0.05" mass="0.3" diaginertia="1 1 1"/>
      <geom name="arm_can" type="cylinder" size=".025 .04" pos="0 0 0.08"/>
      <site name="tip" pos="0 0 0.13"/>
    </body>
  </body>
</worldbody></mujoco>"""
CAN_PAIRS = [("l_can", "crate"), ("l_can", "drum"), ("r_can", "crate"), ("r_can", "drum"), ("arm_can", "crate"), ("arm_can", "drum"),
             ("arm_can", "crate2"), ("l_can", "drum2")]
CANS_EDGES, CANS_SAMPLES = 4, 2


def cans():
    """(model, [CollisionAvoidanceLimit kwargs], q_from, q_to, RefSweep): CANS_EDGES edges of the floating body, the base within
    0.2 of the origin, the quaternion of q_to turned by 1.5 to 2.5 rad about a random axis and given as -q on the odd edges."""
    if "cans" not in _cache:
        from mink_amd.mjcf import loads_mjcf
        model = loads_mjcf(FLOATING_CANS)
        spec = [dict(geom_pairs=[([model.name2id("geom", a)], [model.name2id("geom", b)]) for a, b in CAN_PAIRS],
                     minimum_distance_from_collisions=0.15, collision_detection_distance=0.35)]
        rng = np.random.default_rng(4)
        a = np.zeros((CANS_EDGES, model.nq))
        a[:, :3] = rng.uniform(-0.2, 0.2, size=(CANS_EDGES, 3))
        qa = rng.normal(size=(CANS_EDGES, 4))
        a[:, 3:7] = qa / np.linalg.norm(qa, axis=1, keepdims=True)
        a[:, 7] = rng.uniform(-1.5, 1.5, size=CANS_EDGES)
        b = a.copy()
        b[:, :3] = rng.uniform(-0.2, 0.2, size=(CANS_EDGES, 3))
        b[:, 7] = rng.uniform(-1.5, 1.5, size=CANS_EDGES)
        for i in range(CANS_EDGES):
            axis = rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            ang = rng.uniform(1.5, 2.5)
            r = np.concatenate([[np.cos(0.5 * ang)], np.sin(0.5 * ang) * axis])
            w0, v0 = a[i, 3], a[i, 4:7]
            turned = np.concatenate([[w0 * r[0] - v0 @ r[1:]], w0 * r[1:] + r[0] * v0 + np.cross(v0, r[1:])])
            b[i, 3:7] = -turned if i % 2 else turned
        ref = _frozen(sref.sweep(model, cr.limits_of(limit_objects(model, spec)), a, b, CANS_SAMPLES))
        a.setflags(write=False); b.setflags(write=False)
        _cache["cans"] = (model, spec, a, b, ref)
    return _cache["cans"]


# ---- the checked ladder on `convex_shapes`
LADDER_B, LADDER_T, LADDER_S, LADDER_M = 2, 3, 3, 2


def ladder(sparse=False):
    """(q (B, nq), q_nodes (B, T, S, nq), tracked (B, T, S) or None, ladder_free_ref.select's dict): nodes drawn from the fixture's
    rows, three quarters from its free ones; every node tracked or, `sparse`, about half of them."""
    key = ("ladder", sparse)
    if key not in _cache:
        model, spec, rows = shapes()
        limits = cr.limits_of(limit_objects(model, spec))
        B, T, S = LADDER_B, LADDER_T, LADDER_S
        rng = np.random.default_rng(2)
        free = np.nonzero(~shapes_ref().in_collision)[0]
        n = B * T * S
        any_row = np.arange(n) % 4 == 3
        rng.shuffle(any_row)
        pick = np.where(any_row, rng.integers(0, len(rows), size=n), free[rng.integers(0, len(free), size=n)])
        q_nodes = np.ascontiguousarray(rows[pick].reshape(B, T, S, model.nq))
        q = np.tile(np.asarray(model.qpos0, dtype=np.float64), (B, 1))
        trk = (np.random.default_rng(7).random((B, T, S)) < 0.5) if sparse else None
        want = lfref.select(model, limits, q, q_nodes, trk, None, np.inf, LADDER_M)
        for x in [q, q_nodes] + [v for v in want.values() if isinstance(v, np.ndarray)]:
            x.setflags(write=False)
        _cache[key] = (q, q_nodes, trk, want)
    return _cache[key]
