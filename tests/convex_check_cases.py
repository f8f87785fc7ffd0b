"""The inputs of the tests of checked candidate tracking and checked refinement on checkers WITH general convex pairs
(tests/test_convex_checks_cpu.py, tests/test_gpu_convex_checks.py) and the references of the tracking cases by
tests/trajectory_free_ref.py — computed once per process and handed out read-only.  The models are
tests/swept_convex_cases.py's `convex_shapes` and clearance_ref's `ur5e_convex`."""

import numpy as np

import clearance_ref as cr
import swept_convex_cases as sc
import swept_ref as sref
import trajectory_free_ref as tfref

_cache = {}

# ---- candidate tracking on `convex_shapes`: the fixture's first 64 rows as time-major candidates
TRACK = dict(T=4, B=2, S=8, M=3)
WIDE_DMIN = (0.02, 0.0, 0.03)        # the pair list three times: 45 pairs, one row per wavefront
# what the reference alone says about the case (tracking_counts)
TRACK_COUNTS = dict(nodes_in_collision=33, nodes_convex=44, edges_swept=21, edges_in_collision=6, edges_convex=13)

MJ_ELLIPSOID, MJ_CYLINDER, MJ_BOX, MJ_MESH = 4, 5, 6, 7


def convex_mask(model, limits):
    """Per pair of the reference's pair list: whether it goes through the general convex routine — an ellipsoid or a mesh hull
    against anything, cylinder-cylinder, cylinder-box (include/minkhip.h)."""
    pairs = cr.pair_list(limits)[0]
    t = np.asarray(model.geom_type)
    out = []
    for g1, g2 in pairs:
        a, b = sorted((int(t[g1]), int(t[g2])))
        out.append(MJ_ELLIPSOID in (a, b) or MJ_MESH in (a, b) or (a, b) in ((MJ_CYLINDER, MJ_CYLINDER), (MJ_CYLINDER, MJ_BOX)))
    return np.array(out, dtype=bool)


def without_convex(model, limits):
    """The reference's limits with the general convex pairs deleted (a limit left without a pair goes too)."""
    out, k = [], 0
    conv = convex_mask(model, limits)
    for p, dmin, ddet in limits:
        p = np.asarray(p).reshape(-1, 2)
        keep = ~conv[k:k + len(p)]
        k += len(p)
        if keep.any():
            out.append((p[keep], dmin, ddet))
    return out


def shapes_spec(wide=False):
    """(model, [CollisionAvoidanceLimit kwargs]) of `convex_shapes`; wide: its list in three limits with WIDE_DMIN."""
    model, spec, _ = sc.shapes()
    if wide:
        spec = [dict(spec[0], minimum_distance_from_collisions=d) for d in WIDE_DMIN]
    return model, spec


def tracking(wide=False):
    """((model, limits, q (B, nq), q_all (T, B·S, nq)), trajectory_free_ref.rule's dict)."""
    key = ("tracking", wide)
    if key not in _cache:
        model, spec = shapes_spec(wide)
        limits = cr.limits_of(sc.limit_objects(model, spec))
        T, B, S, M = (TRACK[k] for k in "TBSM")
        q_all = np.ascontiguousarray(sc.shapes()[2][:T * B * S].reshape(T, B * S, model.nq))
        q = np.tile(np.asarray(model.qpos0, dtype=np.float64), (B, 1))
        want = tfref.rule(model, limits, q, q_all, None, None, S, M)
        for x in [q, q_all] + [v for v in want.values() if isinstance(v, np.ndarray)]:
            x.setflags(write=False)
        _cache[key] = ((model, limits, q, q_all), want)
    return _cache[key]


def tracking_counts(want=None):
    """The conditions on the (narrow) tracking case, on the reference alone: the counts of TRACK_COUNTS, and no judged margin
    within 1e-6 of zero (the smallest |node margin| is 1.5e-3)."""
    (model, limits, q, q_all), ref = tracking()
    want = ref if want is None else want
    M = TRACK["M"]
    conv = convex_mask(model, limits)
    assert conv.tolist() == [g for _, _, g in sc.PAIRS] and int(conv.sum()) == 9
    nm, em = want["node_margin_all"], want["edge_margin_all"]
    nodes = cr.clearance(model, limits, q_all.reshape(-1, model.nq))
    swept = want["swept"]
    edges = [sref.sweep(model, limits, q_all[t - 1, i][None], q_all[t, i][None], M) for t, i in swept]
    got = dict(nodes_in_collision=int((~(nm >= 0.0)).sum()), nodes_convex=int(conv[nodes.pair].sum()), edges_swept=len(swept),
               edges_in_collision=int(sum(not (em[t, i] >= 0.0) for t, i in swept)),
               edges_convex=int(sum(conv[e.pair[0]] for e in edges)))
    assert got == TRACK_COUNTS, got
    judged = np.concatenate([nm.ravel(), [em[t, i] for t, i in swept]])
    assert np.abs(judged).min() > 1e-6 and 1.4e-3 < np.abs(nm).min() < 1.6e-3
    return got


# ---- the refinement pass: (world, B, T, M, gate, the ladder's iterations, rng_seed, first row of the targets)
# Every counter of the restatement is at least 1 on `ur5e_by_the_wall` alone; `shapes_body8` is the model on which general
# convex pairs decide often (tests/test_gpu_convex_checks.py::test_the_cases_take_every_branch holds the conditions).
REFINE = {"ur5e_by_the_wall": ("ur5e_convex", 5, 6, 2, 16.0, 3, 2, 12),
          "ur5e_three_samples": ("ur5e_convex", 5, 6, 3, np.inf, 4, 1, 0),
          "shapes_body8": ("convex_shapes:8", 5, 4, 3, 4.0, 3, 4, 7),
          # the pair list three times (45 pairs): one instance per wavefront, the 64-lane build of the check
          "shapes_wide": ("convex_shapes_wide:8", 3, 4, 2, 4.0, 3, 4, 7)}
MANY = ("ur5e_convex", 18, 2, 2, np.inf, 3, 4, 0)


def ur5e_rows_by_the_wall(free=False):
    """The rows of the `ur5e_convex` fixture whose cylinder-box distance is in range (below the detection distance); free: those of
    them the reference finds free of collision."""
    _, _, q = cr.fixture("ur5e_convex")
    ref = cr.fixture_ref("ur5e_convex")
    limits = cr.limits_of(cr.fixture_limits("ur5e_convex"))
    near = ref.distance[:, sc.UR5E_CONVEX_PAIR] < cr.pair_list(limits)[2][sc.UR5E_CONVEX_PAIR]
    return np.ascontiguousarray(q[near & ~ref.in_collision] if free else q[near])


def refine_world(world):
    """(model, CollisionAvoidanceLimit objects, rows whose frame poses serve as targets, (frame name, frame type), home (nq,)).
    `ur5e_convex`: the rows of the fixture whose cylinder-box distance is in range — waypoints by the wall.  `convex_shapes:<i>`:
    a frame task on body s<i> of the model on which general convex pairs decide often; `convex_shapes_wide:<i>`: the same under
    the pair list in three limits."""
    if world == "ur5e_convex":
        model = cr.fixture("ur5e_convex")[0]
        return (model, cr.fixture_limits("ur5e_convex"), sc.ur5e_convex_edges()[0], ("attachment_site", "site"),
                np.asarray(model.key_qpos[model.name2id("key", "home")], dtype=np.float64))
    name, body = world.split(":")
    assert name in ("convex_shapes", "convex_shapes_wide")
    model, spec = shapes_spec(wide=name.endswith("_wide"))
    rows = sc.shapes()[2]
    return model, sc.limit_objects(model, spec), rows, ("s" + body, "body"), np.asarray(model.qpos0, dtype=np.float64)
