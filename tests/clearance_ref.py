"""numpy restatement of THE RULE OF CLEARANCE (include/minkhip.h) from the oracle's mj_kinematics / mj_geomDistance, and the
fixtures the clearance tests share: the reference of tests/test_gpu_clearance.py and tests/test_gpu_collision_free_ik.py, held
against closed-form numbers by tests/test_clearance_cpu.py.

A fixture is (model, limits, q_rows): `limits` a list of (geom_id_pairs (n, 2), minimum_distance, detection_distance) in pair-list
order.  References are computed once per process and handed out read-only."""

from typing import NamedTuple

import numpy as np

from oracle import mjmath


class RefClearance(NamedTuple):
    margin: np.ndarray        # (N,)
    pair: np.ndarray          # (N,) int32
    n_violated: np.ndarray    # (N,) int32
    in_collision: np.ndarray  # (N,) bool
    distance: np.ndarray      # (N, n_pairs)


def pair_list(limits):
    """(pairs (P, 2), dmin (P,), ddetect (P,)) of a list of (geom_id_pairs, minimum_distance, detection_distance)."""
    pairs = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1, 2) for p, _, _ in limits])
    dmin = np.concatenate([np.full(len(np.asarray(p).reshape(-1, 2)), float(a)) for p, a, _ in limits])
    ddet = np.concatenate([np.full(len(np.asarray(p).reshape(-1, 2)), float(b)) for p, _, b in limits])
    return pairs, dmin, ddet


def distances(model, limits, q_rows):
    """d_k of every row: (N, P)."""
    pairs, _, ddet = pair_list(limits)
    q_rows = np.asarray(q_rows, dtype=np.float64).reshape(-1, model.nq)
    out = np.empty((len(q_rows), len(pairs)))
    d = mjmath.Data(model)
    for i, q in enumerate(q_rows):
        if not np.isfinite(q).all():
            out[i] = np.nan
            continue
        d.qpos[:] = q
        mjmath.mj_kinematics(model, d)
        for k, (g1, g2) in enumerate(pairs):
            out[i, k] = mjmath.mj_geomDistance(model, d, int(g1), int(g2), float(ddet[k]), None)
    return out


def from_distances(dist, dmin):
    """The rule on (N, P) distances: numpy's min / argmin — a NaN term decides, ties go to the lowest pair."""
    terms = (dist - dmin[None, :]) + 0.0
    margin = terms.min(axis=1)
    pair = terms.argmin(axis=1).astype(np.int32)
    n_violated = (~(dist >= dmin[None, :])).sum(axis=1).astype(np.int32)
    return RefClearance(margin, pair, n_violated, ~(margin >= 0.0), dist)


def clearance(model, limits, q_rows):
    return from_distances(distances(model, limits, q_rows), pair_list(limits)[1])


# ---- fixtures
_fixtures, _refs = {}, {}
N_UR5E, N_G1, N_CHAIN = 256, 129, 16
G1_SPREAD, G1_LIFT = 0.5, 0.3  # half width (rad) of the draw around `stand` at every limited hinge, clipped to the joint range; the
                               # base lifted so that the feet at `stand` hang above the detection distance of the floor pairs


def _uniform_in_ranges(model, rng, n):
    lo, hi = np.asarray(model.jnt_range)[:, 0], np.asarray(model.jnt_range)[:, 1]
    q = np.tile(np.asarray(model.qpos0, dtype=np.float64), (n, 1))
    for j in range(model.njnt):
        if int(model.jnt_type[j]) in (2, 3) and model.jnt_limited[j]:
            qa = int(model.jnt_qposadr[j])
            q[:, qa] = rng.uniform(lo[j], hi[j], size=n)
    return q


def ur5e_capsule_pairs(model):
    """All valid capsule geoms of the UR5e's links against floor and wall (parent / child and welded pairs dropped by the limit's
    own constructor): the 14-pair checker."""
    caps = [g for g in range(model.ngeom) if int(model.geom_type[g]) == 3 and model.geom_valid[g]]
    return [(caps, ["floor", "wall"])]


# ---- "shapes": every analytic pair family the robots' fixtures leave out — box–box first —, on a model made for it
N_SHAPES, SHAPES_BODIES, SHAPES_SPREAD = 64, 20, 0.55
SHAPES_TYPES = ["box", "box", "box", "capsule", "capsule", "capsule", "sphere", "sphere", "cylinder", "cylinder"]   # of body i % 10


def shapes_mjcf(seed=11):
    """SHAPES_BODIES bodies, all children of the world (one level of 20 bodies), scattered in a cube of side SHAPES_SPREAD, each
    with one joint (hinge ±1.5 rad or slide ±0.15 m about a random axis) and one randomly turned geom of SHAPES_TYPES."""
    rng = np.random.default_rng(seed)
    xml = ['<mujoco><compiler angle="radian"/><worldbody>']
    for i in range(SHAPES_BODIES):
        ax, qt = rng.normal(size=3), rng.normal(size=4)
        ax, qt = ax / np.linalg.norm(ax), qt / np.linalg.norm(qt)
        pos = rng.uniform(-0.5 * SHAPES_SPREAD, 0.5 * SHAPES_SPREAD, size=3) + np.array([0.0, 0.0, 0.5])
        typ = SHAPES_TYPES[i % 10]
        size = {"box": rng.uniform(0.03, 0.08, size=3), "capsule": np.array([rng.uniform(0.02, 0.04), rng.uniform(0.04, 0.1)]),
                "sphere": rng.uniform(0.03, 0.06, size=1), "cylinder": np.array([rng.uniform(0.03, 0.05), rng.uniform(0.03, 0.08)])}[typ]
        joint = ('type="hinge" range="-1.5 1.5"' if i % 2 else 'type="slide" range="-0.15 0.15"')
        xml.append(f'<body name="s{i}" pos="{pos[0]:.4f} {pos[1]:.4f} {pos[2]:.4f}">'
                   f'<joint name="sj{i}" {joint} axis="{ax[0]:.5f} {ax[1]:.5f} {ax[2]:.5f}"/>'
                   f'<geom name="g{i}" type="{typ}" size="{" ".join("%.4f" % x for x in size)}" '
                   f'quat="{qt[0]:.5f} {qt[1]:.5f} {qt[2]:.5f} {qt[3]:.5f}" pos="0.03 0.02 -0.01" mass="0.1"/></body>')
    xml.append("</worldbody></mujoco>")
    return "".join(xml)


def shapes_pairs():
    """30 pairs of body / geom indices: all 15 box–box pairs, 6 capsule–capsule, 3 sphere–capsule, 3 capsule–cylinder, and one each
    of sphere–sphere, capsule–box, sphere–box."""
    of = lambda t: [i for i in range(SHAPES_BODIES) if SHAPES_TYPES[i % 10] == t]
    box, cap, sph, cyl = of("box"), of("capsule"), of("sphere"), of("cylinder")
    pairs = [(a, b) for k, a in enumerate(box) for b in box[k + 1:]]
    pairs += [(a, b) for k, a in enumerate(cap) for b in cap[k + 1:]][:6]
    pairs += [(sph[k], cap[k]) for k in range(3)] + [(cap[k + 3], cyl[k]) for k in range(3)]
    pairs += [(sph[0], sph[3]), (cap[0], box[0]), (sph[1], box[5])]
    return pairs


def fixture(name):
    """(model, [CollisionAvoidanceLimit kwargs], q_rows) by name: ur5e_wrist, ur5e_convex, ur5e_all, g1, chain, shapes (30 pairs:
    four rows per wavefront, two trips of its 16 lanes over bodies and pairs), shapes_wide (the same pairs twice, with two
    minimum distances: 60 pairs, one row per wavefront), tree_small / tree_wide / tree_convex (tests/tree_cases.py)."""
    if name in _fixtures:
        return _fixtures[name]
    if name.startswith("tree_"):                   # random trees with ball and stacked joints: tests/tree_cases.py
        import tree_cases
        _fixtures[name] = tree_cases.fixture(name)
        return _fixtures[name]
    from mink_amd import workloads
    if name in ("shapes", "shapes_wide"):
        from mink_amd.mjcf import loads_mjcf
        model = fixture("shapes")[0] if name == "shapes_wide" else loads_mjcf(shapes_mjcf())
        gid = lambda i: model.name2id("geom", "g%d" % i)
        pairs = [([gid(a)], [gid(b)]) for a, b in shapes_pairs()]
        spec = [dict(geom_pairs=pairs, minimum_distance_from_collisions=0.0, collision_detection_distance=0.25)]
        if name == "shapes_wide":
            spec.append(dict(geom_pairs=pairs, minimum_distance_from_collisions=-0.01, collision_detection_distance=0.3))
        q = _uniform_in_ranges(model, np.random.default_rng(3), N_SHAPES)
        _fixtures[name] = (model, spec, q)
        return _fixtures[name]
    if name in ("ur5e_wrist", "ur5e_convex", "ur5e_all"):
        model = workloads.load_bench_robot("ur5e_convex" if name == "ur5e_convex" else "ur5e_coll")
        if name == "ur5e_all":
            spec = [dict(geom_pairs=ur5e_capsule_pairs(model), minimum_distance_from_collisions=0.02, collision_detection_distance=0.2)]
        else:
            spec = [dict(geom_pairs=[(["wrist_3_link"], ["floor", "wall"])], minimum_distance_from_collisions=0.05,
                         collision_detection_distance=0.3)]
        q = _uniform_in_ranges(model, np.random.default_rng(0), N_UR5E)
    elif name == "g1":
        model = workloads.load_robot("g1")
        spec = [dict(geom_pairs=[([a], [b]) for a, b in workloads.g1_collision_pairs(model)], minimum_distance_from_collisions=0.06,
                     collision_detection_distance=0.25)]
        rng = np.random.default_rng(0)
        stand = np.asarray(model.key_qpos[model.key_names.index("stand")], dtype=np.float64)
        q = np.tile(stand, (N_G1, 1))
        q[:, 2] += G1_LIFT
        for j in range(model.njnt):
            if int(model.jnt_type[j]) == 3 and model.jnt_limited[j]:
                qa = int(model.jnt_qposadr[j])
                lo, hi = model.jnt_range[j]
                q[:, qa] = np.clip(stand[qa] + rng.uniform(-G1_SPREAD, G1_SPREAD, size=N_G1), lo, hi)
    elif name == "chain":
        import wide_cases as wc
        H80 = wc.collision_case(N_CHAIN)
        model, q = H80["m"], H80["q"]
        spec = [dict(geom_pairs=[([int(a)], [int(b)]) for a, b in wc.HINGE80_PAIRS], minimum_distance_from_collisions=wc.HINGE80_DMIN,
                     collision_detection_distance=wc.HINGE80_DETECT)]
    else:
        raise KeyError(name)
    _fixtures[name] = (model, spec, q)
    return _fixtures[name]


def fixture_limits(name):
    """The fixture's CollisionAvoidanceLimit objects (mink_amd's), fresh."""
    import mink_amd
    model, spec, _ = fixture(name)
    return [mink_amd.CollisionAvoidanceLimit(model, **kw) for kw in spec]


def limits_of(objs):
    """The reference's (pairs, dmin, ddetect) list of CollisionAvoidanceLimit objects."""
    return [(np.asarray(o.geom_id_pairs).reshape(-1, 2), o.minimum_distance_from_collisions, o.collision_detection_distance) for o in objs]


def fixture_ref(name):
    """RefClearance of the fixture's rows, computed once; the arrays are read-only."""
    if name not in _refs:
        model, _, q = fixture(name)
        ref = clearance(model, limits_of(fixture_limits(name)), q)
        for a in ref:
            a.setflags(write=False)
        _refs[name] = ref
    return _refs[name]
