"""Random kinematic trees WITH geoms for the collision checker's tests (tests/test_tree_checker_cpu.py,
tests/test_gpu_tree_checker.py): what the robots' fixtures and `shapes` leave out — ball joints, bodies with two joints, joint
anchors away from the body origin at every depth, slides behind rotations, chains five bodies deep and deeper.

`tree_mjcf` is the generator (the manner of random_models.random_mjcf, on a stream of its own: that function's draws are other
fixtures' and stay what they are).  Every moving body carries one geom with a random offset and orientation; the world a plane
and a box.  `draw_pairs` draws a pair list from the geom pairs a CollisionAvoidanceLimit keeps (no two geoms of one body, no
parent and child), the required families first.

Three fixtures in the shape clearance_ref.fixture returns — (model, [CollisionAvoidanceLimit kwargs], q_rows) —, which that
function hands out under their names:

* `tree_small`   11 moving bodies under a fixed root, 28 analytic pairs in one limit: four rows per wavefront.
* `tree_wide`    a free root over 16 more bodies, 52 pairs in two limits, the second with minimum_distance < 0: one row per
                 wavefront.
* `tree_convex`  `tree_small`'s tree and pair list with every second sphere an ellipsoid and every second capsule a cylinder:
                 general convex pairs beside analytic ones.

Each asserts its own composition from the model arrays when it is built (`composition`).  q_rows: N_ROWS rows by
random_models.rand_q.  The edges of the tests are rows 0 .. 23 -> 24 .. 47 shortened to b = a (+) 0.3 (b0 (-) a) (`edges`); what
the references alone say about them is pinned in PINNED and computed once per process."""

import numpy as np

import clearance_ref as cr
import keyframe_ref as kf
from oracle import lie as olie
from random_models import rand_q

JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3
GEOM_NAMES = {0: "plane", 2: "sphere", 3: "capsule", 4: "ellipsoid", 5: "cylinder", 6: "box"}
N_ROWS, N_EDGES, EDGE_S, RESOLUTION = 48, 24, 0.3, 0.05
# the analytic families clearance_ref.shapes_pairs() lists (the two type names sorted)
ANALYTIC_FAMILIES = ("box-box", "capsule-capsule", "capsule-sphere", "capsule-cylinder", "sphere-sphere", "box-capsule", "box-sphere")
KINDS = ["hinge", "slide", "ball", "hinge_hinge", "hinge_slide"]
KIND_P = [0.28, 0.1, 0.27, 0.15, 0.2]
CHAIN = 5                                    # bodies 0 .. CHAIN - 1 hang in series: a chain at least this deep

_cache = {}


def _fmt(v):
    return " ".join(f"{x:.6f}" for x in np.atleast_1d(v))


def _size(typ, u):
    """The size of a geom of type `typ` from three uniform draws (every type reads the same three: swapping a type leaves the
    stream alone)."""
    if typ == "sphere":
        return [0.03 + 0.03 * u[0]]
    if typ == "capsule":
        return [0.02 + 0.02 * u[0], 0.04 + 0.06 * u[1]]
    if typ == "cylinder":
        return [0.03 + 0.02 * u[0], 0.03 + 0.05 * u[1]]
    return list(0.03 + 0.05 * u)             # box, ellipsoid


def tree_mjcf(seed, nbody, free_root, spread, swap=None):
    """A random tree of `nbody` moving bodies as MJCF text.  free_root: body 0 carries a free joint and every other body hangs
    below it; else bodies may hang on the world as well.  spread: the scale of the body offsets.  swap(i, type) -> type renames
    the geom type of body i after the draw."""
    rng = np.random.default_rng(seed)
    parent = [-1] + [int(rng.integers(0 if free_root else -1, i)) for i in range(1, nbody)]
    for i in range(1, CHAIN):
        parent[i] = i - 1
    children = {i: [] for i in range(-1, nbody)}
    for i, p in enumerate(parent):
        children[p].append(i)

    def joint(name, typ, pad):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        pos = rng.normal(scale=0.03, size=3)
        lim = ""
        if typ == "slide":                   # every slide limited: an unlimited one makes every edge above it unbounded
            lim = f' range="{-rng.uniform(0.03, 0.12):.4f} {rng.uniform(0.03, 0.12):.4f}"'
        elif rng.uniform() < 0.6:
            lim = f' range="{-rng.uniform(0.3, 1.5):.4f} {rng.uniform(0.3, 1.5):.4f}"'
        return f'{pad}  <joint name="{name}" type="{typ}" axis="{_fmt(ax)}" pos="{_fmt(pos)}"{lim}/>'

    def body(i, depth):
        pad = "  " * (depth + 2)
        pos = rng.normal(scale=spread, size=3)
        if parent[i] < 0:
            pos = pos + np.array([0.0, 0.0, 0.55])
        out = [f'{pad}<body name="b{i}" pos="{_fmt(pos)}" quat="{_fmt(olie.so3_exp(rng.normal(scale=0.6, size=3)))}">']
        kind = str(rng.choice(KINDS, p=KIND_P))
        if i == 0 and free_root:
            out.append(f'{pad}  <freejoint name="root"/>')
        elif kind == "ball":
            out.append(f'{pad}  <joint name="j{i}" type="ball" pos="{_fmt(rng.normal(scale=0.03, size=3))}"/>')
        else:
            for k, typ in enumerate({"hinge": ["hinge"], "slide": ["slide"], "hinge_hinge": ["hinge", "hinge"],
                                     "hinge_slide": ["hinge", "slide"]}[kind]):
                out.append(joint(f"j{i}_{k}", typ, pad))
        typ = str(rng.choice(["sphere", "capsule", "box", "cylinder"], p=[0.25, 0.3, 0.3, 0.15]))
        size = _size(swap(i, typ) if swap else typ, rng.uniform(size=3))
        out.append(f'{pad}  <geom name="g{i}" type="{swap(i, typ) if swap else typ}" size="{_fmt(size)}" '
                   f'pos="{_fmt(rng.normal(scale=0.03, size=3))}" quat="{_fmt(olie.so3_exp(rng.normal(size=3)))}" mass="0.1"/>')
        for c in children[i]:
            out += body(c, depth + 1)
        out.append(f"{pad}</body>")
        return out

    lines = ['<mujoco>', '  <compiler angle="radian" autolimits="true"/>', '  <worldbody>',
             '    <geom name="floor" type="plane" size="2 2 0.1"/>',
             '    <geom name="block" type="box" size="0.12 0.1 0.08" pos="0.22 0.1 0.5" quat="0.96 0.1 0.2 0.15"/>']
    for r in children[-1]:
        lines += body(r, 0)
    lines += ['  </worldbody>', '</mujoco>']
    return "\n".join(lines)


# ---- the pair list
def chain_of(model, b):
    out = []
    while b > 0:
        out.append(b)
        b = int(model.body_parentid[b])
    return out[::-1]


def common_chain(model, g1, g2):
    """The bodies above both geoms, the world left out."""
    a, b = chain_of(model, int(model.geom_bodyid[g1])), chain_of(model, int(model.geom_bodyid[g2]))
    n = 0
    while n < min(len(a), len(b)) and a[n] == b[n]:
        n += 1
    return a[:n]


def family(model, g1, g2):
    return "-".join(sorted(GEOM_NAMES[int(model.geom_type[g])] for g in (g1, g2)))


def _general_convex(fam):
    return "ellipsoid" in fam or fam in ("cylinder-cylinder", "box-cylinder")


def draw_pairs(model, rng, n, required=ANALYTIC_FAMILIES, analytic_only=True):
    """n pairs (g1 < g2) of the geom pairs a CollisionAvoidanceLimit keeps, in a random order: one of every `required` family
    first, a pair with the plane, a pair below a common moving ancestor, a pair with no common chain; the rest as they come."""
    par = np.asarray(model.body_parentid)
    cand = []
    for a in range(model.ngeom):
        for b in range(a + 1, model.ngeom):
            ba, bb = int(model.geom_bodyid[a]), int(model.geom_bodyid[b])
            if ba == bb or par[ba] == bb or par[bb] == ba:
                continue
            if analytic_only and _general_convex(family(model, a, b)):
                continue
            cand.append((a, b))
    cand = [cand[i] for i in rng.permutation(len(cand))]
    want = [lambda p, f=f: family(model, *p) == f for f in required]
    want += [lambda p: "plane" in family(model, *p), lambda p: len(common_chain(model, *p)) > 0,
             lambda p: len(common_chain(model, *p)) == 0 and "plane" not in family(model, *p)]
    out = []
    for ok in want:
        hit = next((p for p in cand if ok(p) and p not in out), None)
        if hit is not None and not any(ok(p) for p in out):
            out.append(hit)
    out += [p for p in cand if p not in out][:n - len(out)]
    return [out[i] for i in rng.permutation(len(out))]


# ---- composition
def composition(model, limits):
    """What the model arrays and the reference's pair list say of a fixture."""
    jt = np.asarray(model.jnt_type)
    jb = np.asarray(model.jnt_bodyid)
    par = np.asarray(model.body_parentid)
    jpos = np.linalg.norm(np.asarray(model.jnt_pos, dtype=np.float64).reshape(-1, 3), axis=1)
    has_child = np.zeros(model.nbody, dtype=bool)
    has_child[par[1:]] = True
    kinds = {b: [int(jt[j]) for j in range(model.njnt) if jb[j] == b] for b in range(1, model.nbody)}
    ball_bodies = [b for b, k in kinds.items() if k == [JNT_BALL]]
    pairs = cr.pair_list(limits)[0]

    def below_a_ball(b):
        return any(kinds[c] == [JNT_BALL] for c in chain_of(model, b)[:-1])

    def behind_rotation(j):
        b = int(jb[j])
        above = [k for c in chain_of(model, b)[:-1] for k in kinds[c]] + [int(jt[i]) for i in range(model.njnt) if jb[i] == b and i < j]
        return any(k in (JNT_HINGE, JNT_BALL, JNT_FREE) for k in above)

    return dict(
        moving_bodies=model.nbody - 1, free_root=int((jt == JNT_FREE).sum()), n_pairs=len(pairs), n_limits=len(limits),
        balls=len(ball_bodies),
        inner_balls_off_origin=sum(1 for b in ball_bodies if has_child[b] and jpos[[j for j in range(model.njnt) if jb[j] == b][0]] > 0.01),
        balls_below_a_ball=sum(1 for b in ball_bodies if below_a_ball(b)),
        hinge_hinge=sum(1 for k in kinds.values() if k == [JNT_HINGE, JNT_HINGE]),
        hinge_slide=sum(1 for k in kinds.values() if k == [JNT_HINGE, JNT_SLIDE]),
        slides=int((jt == JNT_SLIDE).sum()), unlimited_slides=int(((jt == JNT_SLIDE) & (np.asarray(model.jnt_limited) == 0)).sum()),
        slides_behind_a_rotation=sum(1 for j in range(model.njnt) if jt[j] == JNT_SLIDE and behind_rotation(j)),
        hinges=int((jt == JNT_HINGE).sum()), unlimited_hinges=int(((jt == JNT_HINGE) & (np.asarray(model.jnt_limited) == 0)).sum()),
        anchors_off_origin_below_level_one=sum(1 for j in range(model.njnt) if jpos[j] > 0.01 and par[jb[j]] > 0),
        depth=max(len(chain_of(model, b)) for b in range(1, model.nbody)),
        families=sorted({family(model, a, b) for a, b in pairs}),
        pairs_with_common_chain=sum(1 for a, b in pairs if len(common_chain(model, a, b)) > 0),
        pairs_without_common_chain=sum(1 for a, b in pairs if len(common_chain(model, a, b)) == 0),
        pairs_with_the_plane=sum(1 for a, b in pairs if "plane" in family(model, a, b)))


def _assert_mix(c):
    assert c["balls"] >= 2 and c["inner_balls_off_origin"] >= 1, c
    assert c["hinge_hinge"] >= 1 and c["hinge_slide"] >= 1, c
    assert c["slides"] >= 1 and c["unlimited_slides"] == 0 and c["slides_behind_a_rotation"] >= 1, c
    assert 0 < c["unlimited_hinges"] < c["hinges"], c
    assert c["depth"] >= 5 and c["anchors_off_origin_below_level_one"] >= 1, c
    assert c["pairs_with_common_chain"] >= 1 and c["pairs_without_common_chain"] >= 1 and c["pairs_with_the_plane"] >= 1, c


def assert_composition(name, model, limits):
    import convex_check_cases as cc
    c = composition(model, limits)
    conv = cc.convex_mask(model, limits)
    _assert_mix(c)
    if name in ("tree_small", "tree_convex"):
        assert 8 <= c["moving_bodies"] <= 12 and c["free_root"] == 0 and c["n_pairs"] <= 32 and c["n_limits"] == 1, c
    if name == "tree_small":
        assert not conv.any() and set(ANALYTIC_FAMILIES) <= set(c["families"]), c
    if name == "tree_convex":
        assert 6 <= int(conv.sum()) < c["n_pairs"], (c, conv)
        assert not {"mesh"} & set("-".join(c["families"]).split("-"))
    if name == "tree_wide":
        assert 14 <= c["moving_bodies"] <= 20 and c["free_root"] == 1 and 40 <= c["n_pairs"] <= 60 and c["n_limits"] == 2, c
        assert limits[1][1] < 0.0 and c["balls_below_a_ball"] >= 1 and not conv.any(), c
    return c


# ---- the fixtures: name -> (seed of the tree, moving bodies, free root, spread, seed of the pairs, pairs per limit, (dmin, ddetect)
# per limit, seed of the rows)
SPECS = {
    "tree_small": (10, 11, False, 0.15, 1, (28,), ((0.0, 0.25),), 2),
    "tree_wide": (6, 17, True, 0.18, 1, (30, 22), ((0.01, 0.25), (-0.01, 0.3)), 2),
    "tree_convex": (10, 11, False, 0.15, 1, (28,), ((0.0, 0.25),), 2),
}


def _swap_convex(i, typ):
    return {"sphere": "ellipsoid", "capsule": "cylinder"}.get(typ, typ) if i % 2 == 0 else typ


def fixture(name):
    """(model, [CollisionAvoidanceLimit kwargs], q_rows (N_ROWS, nq)), the composition asserted."""
    if name not in _cache:
        import mink_amd
        from mink_amd.mjcf import loads_mjcf
        seed, nbody, free_root, spread, pair_seed, counts, dists, row_seed = SPECS[name]
        model = loads_mjcf(tree_mjcf(seed, nbody, free_root, spread, _swap_convex if name == "tree_convex" else None))
        # (the pair list of `tree_convex` is `tree_small`'s: drawn on the analytic tree, the swapped types make some of it convex)
        plain = loads_mjcf(tree_mjcf(seed, nbody, free_root, spread)) if name == "tree_convex" else model
        rng = np.random.default_rng(pair_seed)
        spec = []
        for k, (n, (dmin, ddet)) in enumerate(zip(counts, dists)):
            pairs = draw_pairs(plain, rng, n)
            spec.append(dict(geom_pairs=[([a], [b]) for a, b in pairs], minimum_distance_from_collisions=dmin,
                             collision_detection_distance=ddet))
        objs = [mink_amd.CollisionAvoidanceLimit(model, **kw) for kw in spec]
        assert [len(o.geom_id_pairs) for o in objs] == list(counts), name           # (the constructor dropped nothing)
        assert_composition(name, model, cr.limits_of(objs))
        rng = np.random.default_rng(row_seed)
        q = np.stack([rand_q(model, rng) for _ in range(N_ROWS)])
        q.setflags(write=False)
        _cache[name] = (model, spec, q)
    return _cache[name]


def limits(name):
    return cr.limits_of(cr.fixture_limits(name))


# ---- what the references alone say (tests/test_tree_checker_cpu.py holds every number; the GPU tests lean on them)
# rows of q_rows in collision; the verdicts (undecided, certified, colliding) of the first CERTIFIED_EDGES edges at resolution 0.05
# with max_samples 64 and 4, and how many are capped (`tree_wide`: 16 edges — its 52 pairs cost the reference a third of a second
# per edge; the 24th edge, which alone is capped at 64, is left to tests/test_tree_checker_cpu.py)
PINNED = {
    "tree_small": dict(rows_in_collision=13, verdicts=(2, 11, 11), capped=0, verdicts_at_4=(12, 1, 11), capped_at_4=24),
    "tree_wide": dict(rows_in_collision=30, verdicts=(1, 4, 11), capped=0, verdicts_at_4=(5, 0, 11), capped_at_4=16),
    "tree_convex": dict(rows_in_collision=14),
}
# candidates whose integers hang on a difference below 1e-6 (test_gpu_certified_sweep.comparable), and how many are compared
CERTIFIED_DROPPED = {"tree_small": 0, "tree_small_capped": 0, "tree_wide": 0, "tree_wide_capped": 0}
CERTIFIED_EDGES = {"tree_small": 24, "tree_wide": 16}
CERTIFIED_COMPARED = {"tree_small": 24, "tree_small_capped": 24, "tree_wide": 16, "tree_wide_capped": 16}
# rows of q_rows whose clearance has a runner-up pair within 1e-6 of the minimum, or a distance within 1e-6 of its dmin
CLEARANCE_DROPPED = {"tree_small": 0, "tree_wide": 0, "tree_convex": 0}
# edges the sweep's filter drops (swept_convex_cases.separated), per (fixture, n_samples)
SWEEP_DROPPED = {("tree_small", 1): 0, ("tree_small", 8): 0, ("tree_wide", 1): 0, ("tree_wide", 8): 0, ("tree_convex", 1): 0,
                 ("tree_convex", 8): 0}
SWEEP_SAMPLES = (1, 8)


def clearance_keep(name):
    """The rows of q_rows whose integers the reference separates: no distance within 1e-6 of its dmin, no other pair's term
    within 1e-6 of the smallest unless equal to it.  The number dropped is pinned and at most a quarter."""
    key = ("clearance_keep", name)
    if key not in _cache:
        ref, dmin = cr.fixture_ref(name), cr.pair_list(limits(name))[1]
        terms = ref.distance - dmin[None, :]
        ok = (np.abs(terms) > 1e-6).all(axis=1)
        for i in range(len(ok)):
            near = terms[i][terms[i] - terms[i].min() <= 1e-6]
            ok[i] &= bool((near == terms[i].min()).all())
        dropped = CLEARANCE_DROPPED[name]
        assert int((~ok).sum()) == dropped and 4 * dropped <= len(ok), (name, np.nonzero(~ok)[0], dropped)
        _cache[key] = np.nonzero(ok)[0]
    return _cache[key]


def sweep_case(name, M):
    """(a, b, RefSweep of all 24 edges at M samples, indices of the kept edges): swept_convex_cases' filter, its drop count
    pinned."""
    key = ("sweep", name, M)
    if key not in _cache:
        import swept_convex_cases as sc
        import swept_ref as sref
        a, b = edges(name)
        ref = sc._frozen(sref.sweep(fixture(name)[0], limits(name), a, b, M))
        _cache[key] = (a, b, ref, sc.keep(ref, SWEEP_DROPPED[(name, M)], 18))
    return _cache[key]


def edges(name):
    """(a, b (N_EDGES, nq)): rows 0 .. 23 -> rows 24 .. 47, shortened to b = a (+) EDGE_S (b0 (-) a)."""
    key = ("edges", name)
    if key not in _cache:
        model, _, q = fixture(name)
        a = q[:N_EDGES].copy()
        b = np.stack([kf.blend_posture(model, x, y, EDGE_S) for x, y in zip(a, q[N_EDGES:2 * N_EDGES])])
        a.setflags(write=False); b.setflags(write=False)
        _cache[key] = (a, b)
    return _cache[key]


# ---- candidate tracking on `tree_convex`: the fixture's first 24 rows as time-major candidates
TRACK = dict(T=3, B=2, S=4, M=3)
# on the reference alone: nodes in collision, edges swept, edges in collision, and the nodes / swept edges whose margin a general
# convex pair attains with a ball joint on one of its two chains
TRACK_COUNTS = dict(nodes_in_collision=7, edges_swept=10, edges_in_collision=6, nodes_convex_below_a_ball=6, edges_convex_below_a_ball=1)


def tracking():
    """((model, limits, q (B, nq), q_all (T, B·S, nq)), trajectory_free_ref.rule's dict, the counts of TRACK_COUNTS)."""
    if "tracking" not in _cache:
        import convex_check_cases as cc
        import swept_ref as sref
        import trajectory_free_ref as tfref
        model, _, rows = fixture("tree_convex")
        lim = limits("tree_convex")
        T, B, S, M = (TRACK[k] for k in "TBSM")
        q_all = np.ascontiguousarray(rows[:T * B * S].reshape(T, B * S, model.nq))
        q = np.tile(np.asarray(model.qpos0, dtype=np.float64), (B, 1))
        want = tfref.rule(model, lim, q, q_all, None, None, S, M)
        for x in [q, q_all] + [v for v in want.values() if isinstance(v, np.ndarray)]:
            x.setflags(write=False)
        # which pairs go through the general convex routine AND hang below a ball joint on either side
        jt, jb = np.asarray(model.jnt_type), np.asarray(model.jnt_bodyid)
        ball_body = {int(jb[j]) for j in range(model.njnt) if jt[j] == JNT_BALL}
        pairs = cr.pair_list(lim)[0]
        deep = cc.convex_mask(model, lim) & np.array([any(c in ball_body for g in p for c in chain_of(model, int(model.geom_bodyid[g])))
                                                      for p in pairs])
        nm, em, swept = want["node_margin_all"], want["edge_margin_all"], want["swept"]
        nodes = cr.clearance(model, lim, q_all.reshape(-1, model.nq))
        swept_refs = [sref.sweep(model, lim, q_all[t - 1, i][None], q_all[t, i][None], M) for t, i in swept]
        counts = dict(nodes_in_collision=int((~(nm >= 0.0)).sum()), edges_swept=len(swept),
                      edges_in_collision=int(sum(not (em[t, i] >= 0.0) for t, i in swept)),
                      nodes_convex_below_a_ball=int(deep[nodes.pair].sum()),
                      edges_convex_below_a_ball=int(sum(deep[e.pair[0]] for e in swept_refs)))
        judged = np.concatenate([nm.ravel(), [em[t, i] for t, i in swept]])
        assert np.abs(judged).min() > 1e-6, np.abs(judged).min()          # (no flag hangs on a difference below 1e-6)
        _cache["tracking"] = ((model, lim, q, q_all), want, counts)
    return _cache["tracking"]


def quaternion_addresses(model):
    """The first qpos address of every ball and free quaternion."""
    return [int(model.jnt_qposadr[j]) + (3 if int(model.jnt_type[j]) == JNT_FREE else 0) for j in range(model.njnt)
            if int(model.jnt_type[j]) in (JNT_FREE, JNT_BALL)]


def negated(model, rows):
    """rows with every ball and free quaternion negated: the same rotations."""
    out = np.array(rows, dtype=np.float64)
    for qa in quaternion_addresses(model):
        out[:, qa:qa + 4] *= -1.0
    return out


def scaled(model, rows, seed):
    """rows with every ball and free quaternion scaled by its own factor in [0.5, 2]: the same rotations."""
    out = np.array(rows, dtype=np.float64)
    rng = np.random.default_rng(seed)
    for qa in quaternion_addresses(model):
        out[:, qa:qa + 4] *= rng.uniform(0.5, 2.0, size=(len(out), 1))
    return out
