"""The shared cases of the certifying ladder's tests (tests/test_ladder_certified_cpu.py, tests/test_gpu_ladder_certified.py):
their construction, the reference stage of tests/ladder_certified_ref.py computed once per process, and the comparability filter.

Construction, the same for every case: rng = default_rng(seed); per instance a base row drawn from the fixture's rows that the
clearance reference finds free; every node (t, s), in order, is keyframe_ref.blend_posture(base, a random fixture row,
rng.uniform(0, smax)); q is qpos0.

Comparability is decided per INSTANCE on the reference alone: an instance is compared when on every swept edge |margin|,
|lower_bound| and the distance of motion / resolution from an integer exceed 1e-6, and |node margin| does at every node (a
node's flag gates which edges are swept at all).  The ladder returns no sample, pair or segment, so no argmin has to be separated."""

import numpy as np

import clearance_ref as cr
import keyframe_ref as kf
import ladder_certified_ref as lcref

# name -> (fixture, (B, T, S), smax, resolution, max_samples, seed, instances dropped by the filter)
CASES = {
    "A": ("ur5e_all", (4, 5, 4), 0.1, 0.04, 16, 0, 0),
    "B": ("ur5e_all", (1, 2, 3), 0.05, 0.02, 32, 0, 0),
    # (S = 2 and the seed whose 16 edges show all three verdicts: the reference of this fixture's 60 pairs costs about a second per edge)
    "C": ("shapes_wide", (2, 3, 2), 0.5, 0.02, 16, 2, 0),
    # two graphs small enough for ladder_free_ref.brute_force: the policies choose different paths on instance 0 of the first;
    # under REQUIRE_CERTIFIED instances 0 and 1 of the second lose waypoints that REJECT_COLLIDING keeps (n_tracked 2, 1 of 3)
    "tiny": ("ur5e_all", (3, 3, 2), 0.15, 0.04, 16, 0, 0),
    "D": ("ur5e_all", (3, 3, 2), 0.3, 0.04, 16, 0, 0),
    # a random tree with ball and stacked joints (tests/tree_cases.py; run by tests/test_gpu_tree_checker.py)
    "tree": ("tree_small", (2, 4, 3), 0.15, 0.05, 32, 1, 0),
}
_cache = {}


def limits_of(fixture):
    return cr.limits_of(cr.fixture_limits(fixture))


def nodes(fixture, shape, smax, seed):
    """(model, q (B, nq), q_nodes (B, T, S, nq))."""
    model, _, rows = cr.fixture(fixture)
    free = rows[~cr.fixture_ref(fixture).in_collision]
    rng = np.random.default_rng(seed)
    B, T, S = shape
    q_nodes = np.empty((B, T, S, model.nq))
    for b in range(B):
        base = free[rng.integers(len(free))]
        for t in range(T):
            for s in range(S):
                other = rows[rng.integers(len(rows))]
                q_nodes[b, t, s] = kf.blend_posture(model, base, other, rng.uniform(0.0, smax))
    q = np.tile(np.asarray(model.qpos0, dtype=np.float64), (B, 1))
    return model, q, q_nodes


def comparable(st, resolution):
    """(B,) bool."""
    sw = st["swept"]
    near = np.zeros(sw.shape, dtype=bool)
    near[sw] |= np.abs(st["edge_margin_all"][sw]) <= 1e-6
    near[sw] |= np.abs(st["edge_lower_bound_all"][sw]) <= 1e-6
    ratio = st["edge_motion_all"][sw] / resolution
    near[sw] |= np.isfinite(ratio) & (np.abs(ratio - np.round(ratio)) <= 1e-6)
    return ~near.any(axis=(1, 2, 3)) & ~(np.abs(st["node_margin"]) <= 1e-6).any(axis=(1, 2))


def case(name):
    """dict(fixture, model, limits, q, q_nodes, resolution, max_samples, stage, keep (the compared instances), select: {policy:
    ladder_certified_ref.select's dict}) — computed once, the arrays read-only."""
    if name not in _cache:
        fixture, shape, smax, resolution, mx, seed, dropped = CASES[name]
        model, q, q_nodes = nodes(fixture, shape, smax, seed)
        limits = limits_of(fixture)
        st = lcref.stage(model, limits, q_nodes, None, resolution, mx)
        ok = comparable(st, resolution)
        assert int((~ok).sum()) == dropped and 4 * dropped <= shape[0], (name, np.nonzero(~ok)[0], dropped)
        sel = {p: lcref.select(model, q, q_nodes, st, p) for p in (lcref.REJECT_COLLIDING, lcref.REQUIRE_CERTIFIED)}
        for x in (q, q_nodes):
            x.setflags(write=False)
        _cache[name] = dict(fixture=fixture, model=model, limits=limits, q=q, q_nodes=q_nodes, resolution=resolution, max_samples=mx,
                            stage=st, keep=np.nonzero(ok)[0], select=sel)
    return _cache[name]
