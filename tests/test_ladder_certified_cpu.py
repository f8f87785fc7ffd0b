"""The numpy reference of the certifying ladder (tests/ladder_certified_ref.py; include/minkhip.h THE RULE "with a certifying
checker") held to its own claims, without a device: it agrees with the enumeration of all paths under both policies; under
REQUIRE_CERTIFIED every counted waypoint is entered by an edge whose lower bound is >= 0; that policy never tracks more waypoints
than REJECT_COLLIDING; and on a dense resampling of every chosen certified edge no margin falls below the edge's lower bound."""

import numpy as np
import pytest

import certified_ref as cf
import clearance_ref as cr
import keyframe_ref as kf
import ladder_certified_cases as lc
import ladder_certified_ref as lcref
import ladder_free_ref as lfref

POLICIES = (lcref.REJECT_COLLIDING, lcref.REQUIRE_CERTIFIED)
SMALL = ("tiny", "D", "B")


@pytest.mark.parametrize("name", ["tiny", "D"])
def test_search_agrees_with_the_enumeration_of_all_paths(name):
    c = lc.case(name)
    for policy in POLICIES:
        want = lcref.select(c["model"], c["q"], c["q_nodes"], c["stage"], policy, search=lfref.brute_force)
        got = c["select"][policy]
        for f in ("node_index", "n_tracked", "n_breaks", "path_length", "edge_break", "edge_collision", "n_edge_collisions",
                  "edge_verdict", "edge_n_samples", "n_certified"):
            np.testing.assert_array_equal(got[f], want[f], err_msg=f"{name}, policy {policy}: {f}")


def test_the_cases_exercise_the_policies():
    """All three verdicts among the swept edges of `tiny`; the policies choose different paths there; in `D` an instance loses a
    waypoint under REQUIRE_CERTIFIED alone."""
    tiny, d = lc.case("tiny"), lc.case("D")
    v = tiny["stage"]["edge_verdict_all"][tiny["stage"]["swept"]]
    assert set(v.tolist()) == {0, 1, 2}
    assert (tiny["select"][0]["node_index"] != tiny["select"][1]["node_index"]).any()
    T = d["q_nodes"].shape[1]
    assert (d["select"][1]["n_tracked"] < T).any() and (d["select"][1]["n_tracked"] < d["select"][0]["n_tracked"]).any()


@pytest.mark.parametrize("name", SMALL)
def test_require_certified_counts_only_proven_motions(name):
    c = lc.case(name)
    out = c["select"][lcref.REQUIRE_CERTIFIED]
    B, T = out["node_index"].shape
    for b in range(B):
        path = out["node_index"][b]
        counted = [t for t in range(T) if c["stage"]["tracked"][b, t, path[t]] and not out["edge_collision"][b, t]]
        assert len(counted) == out["n_tracked"][b]
        for t in counted:
            if t >= 1:
                assert out["edge_verdict"][b, t] == cf.CERTIFIED and out["edge_lower_bound"][b, t] >= 0.0, (name, b, t)
    # an unswept edge is not blocked, a blocked edge is swept, and the mask of the stricter policy contains the other's
    m0, m1 = (lcref.blocked_mask(c["stage"], p) for p in POLICIES)
    assert not (m1 & ~c["stage"]["swept"]).any() and not (m0 & ~m1).any()


@pytest.mark.parametrize("name", SMALL)
def test_require_certified_never_tracks_more(name):
    c = lc.case(name)
    assert (c["select"][lcref.REQUIRE_CERTIFIED]["n_tracked"] <= c["select"][lcref.REJECT_COLLIDING]["n_tracked"]).all()


@pytest.mark.parametrize("name", SMALL)
def test_chosen_certified_edges_hold_on_a_dense_resampling(name):
    """257 points per chosen certified edge: the smallest margin found is at least lower_bound - 1e-9."""
    c = lc.case(name)
    model, limits = c["model"], c["limits"]
    dmin = cr.pair_list(limits)[1]
    edges = set()
    for policy in POLICIES:
        out = c["select"][policy]
        B, T = out["node_index"].shape
        edges |= {(b, t, int(out["node_index"][b, t]), int(out["node_index"][b, t - 1])) for b in range(B) for t in range(1, T)
                  if out["edge_verdict"][b, t] == cf.CERTIFIED}
    assert edges
    worst = np.inf
    for b, t, s1, s in sorted(edges):
        rows = np.stack([kf.blend_posture(model, c["q_nodes"][b, t - 1, s], c["q_nodes"][b, t, s1], i / 256.0) for i in range(257)])
        dense = ((cr.distances(model, limits, rows) - dmin[None, :]) + 0.0).min()
        worst = min(worst, dense - c["stage"]["edge_lower_bound_all"][b, t, s1, s])
    print("%s: %d chosen certified edges x 257 points: smallest dense margin - lower_bound = %.3e" % (name, len(edges), worst))
    assert worst >= -1e-9
