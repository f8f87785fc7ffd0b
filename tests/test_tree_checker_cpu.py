"""The collision checker's rules on random trees with ball and stacked joints, without a device: the fixtures of
tests/tree_cases.py and what the numpy references alone say about them.

* The fixtures' composition, from the model arrays, and every number tests/test_gpu_tree_checker.py leans on: rows in collision,
  verdicts, capped edges, the candidates the filters drop, the counts of the tracking case.
* tests/test_certified_sweep_cpu.py's two properties of THE RULE OF THE CERTIFIED SWEEP — consecutive reference distances of
  every pair differ by at most L_k h + 1e-9; 121 dense reference rows never fall below a certified edge's lower_bound - 1e-9 — on
  `tree_small` and `tree_wide`: D_after(c, j) of stacked joints, the 2 |jnt_pos| shifts, the ball's angular weight and a limited
  slide's range in D of a body above which hinges turn all enter L_k there.  24 edges each, s = 0.3, resolution 0.05.
* A hand-typed reach table: a hinge, below it a ball whose anchor is off the body origin, below that a body with a hinge and then
  a limited slide — against certified_ref.reach_table and, the same arrays typed into tests/host/motion_bound_cases.cpp, against
  motion_bound.h under the host sanitizers.
* The sign and the scale of a quaternion do not enter the reference: b with every ball and free quaternion negated, both ends
  with every such quaternion scaled by 0.5 .. 2, give the plain ends' margins, bounds and counts to 1e-9."""

import numpy as np
import pytest

import certified_ref as cf
import clearance_ref as cr
import test_certified_sweep_cpu as base
import tree_cases as tc
from test_certified_sweep_cpu import host_cases  # noqa: F401  (the sanitized program, built and run once per module)

TOL = 1e-9
TREES = ["tree_small", "tree_wide"]

STACK_MJCF = """<mujoco><compiler angle="radian"/><worldbody>
  <geom name="floor" type="plane" size="1 1 0.1"/>
  <body name="b1" pos="0 0 0.5">
    <joint name="h1" type="hinge" axis="0 1 0" pos="0.1 0 0"/>
    <geom name="ball" type="sphere" size="0.05" pos="0.2 0 0" mass="0.1"/>
    <body name="b2" pos="0.3 0 0">
      <joint name="k2" type="ball" pos="0 0.03 0.04"/>
      <geom name="rod" type="capsule" size="0.03 0.1" pos="0.1 0 0" mass="0.1"/>
      <body name="b3" pos="0 0.4 0">
        <joint name="h3" type="hinge" axis="0 0 1" pos="0.06 0 0.08"/>
        <joint name="s3" type="slide" axis="1 0 0" pos="0.3 0 0" range="-0.1 0.2"/>
        <geom name="brick" type="box" size="0.03 0.04 0.12" pos="0 0 0.05" mass="0.1"/>
      </body>
    </body>
  </body>
</worldbody></mujoco>"""
STACK_PAIRS = [("floor", "brick"), ("ball", "brick"), ("rod", "brick"), ("floor", "rod")]
# Worked out by hand from the header's text.  Joints h1, k2, h3, s3.  r(brick) = |(0.03, 0.04, 0.12)| = 0.13, |geom_pos(brick)| = 0.05;
# r(rod) = 0.03 + 0.1 = 0.13, |geom_pos(rod)| = 0.1.  |jnt_pos|: h1 0.1, k2 |(0, 0.03, 0.04)| = 0.05, h3 |(0.06, 0, 0.08)| = 0.1; the
# slide's anchor enters nowhere.
#   D(b3) = 2·0.1 (h3) + max(|-0.1|, |0.2|) (s3) = 0.4;   D_after(b3, h3) = 0.2 (the slide behind it);   D_after(b3, s3) = 0
#   D(b2) = 2·0.05 (k2) = 0.1;   D_after(b2, k2) = 0;   D_after(b1, h1) = 0
#   floor-brick: the brick hangs on b1 -> b2 -> b3, the floor on the world.
#     h1 on b1:  0.1 + 0 + (|body_pos(b2)| 0.3 + D(b2) 0.1) + (|body_pos(b3)| 0.4 + D(b3) 0.4) + 0.05 + 0.13 = 1.48
#     k2 on b2:  0.05 + 0 + (0.4 + 0.4) + 0.05 + 0.13                                                        = 1.03
#     h3 on b3:  0.1 + D_after(b3, h3) 0.2 + 0.05 + 0.13                                                      = 0.48
#     s3 on b3:  linear 1, angular 0
#   ball-brick: b1 is common (h1: 0, 0); the ball's own remaining chain is empty.  k2, h3, s3 as above.
#   rod-brick:  b1 and b2 are common; h3 and s3 alone.
#   floor-rod:  h1: 0.1 + 0 + (0.3 + 0.1) + 0.1 + 0.13 = 0.73;  k2: 0.05 + 0 + 0.1 + 0.13 = 0.28;  h3 and s3 do not carry the rod.
STACK_COEF = np.array([[[0, 1.48], [0, 1.03], [0, 0.48], [1, 0]],
                       [[0, 0], [0, 1.03], [0, 0.48], [1, 0]],
                       [[0, 0], [0, 0], [0, 0.48], [1, 0]],
                       [[0, 0.73], [0, 0.28], [0, 0], [0, 0]]], dtype=np.float64)


def _stack_model():
    from mink_amd.mjcf import loads_mjcf
    model = loads_mjcf(STACK_MJCF)
    return model, [(model.name2id("geom", a), model.name2id("geom", b)) for a, b in STACK_PAIRS]


# ------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("name", ["tree_small", "tree_wide", "tree_convex"])
def test_fixture_composition(name):
    """The assertions of tree_cases.assert_composition (made when the fixture is built), and the pinned facts beside them."""
    model, spec, q = cr.fixture(name)
    assert cr.fixture(name) is tc.fixture(name)
    c = tc.assert_composition(name, model, tc.limits(name))
    print(name, c)
    assert q.shape == (tc.N_ROWS, model.nq) and not q.flags.writeable
    want = {"tree_small": dict(moving_bodies=11, balls=6, inner_balls_off_origin=4, balls_below_a_ball=5, hinge_hinge=1, hinge_slide=1,
                               slides=2, hinges=5, unlimited_hinges=1, depth=6, n_pairs=28, pairs_with_common_chain=19,
                               pairs_without_common_chain=9, pairs_with_the_plane=5),
            "tree_wide": dict(moving_bodies=17, balls=4, inner_balls_off_origin=1, balls_below_a_ball=2, hinge_hinge=1, hinge_slide=3,
                              slides=7, hinges=9, unlimited_hinges=5, depth=7, n_pairs=52, pairs_with_common_chain=38,
                              pairs_without_common_chain=14, pairs_with_the_plane=8)}
    want["tree_convex"] = want["tree_small"]
    assert {k: c[k] for k in want[name]} == want[name]
    # limited joints inside their range, unit quaternions
    rng = np.asarray(model.jnt_range, dtype=np.float64).reshape(-1, 2)
    for j in range(model.njnt):
        qa, jt = int(model.jnt_qposadr[j]), int(model.jnt_type[j])
        if jt in (tc.JNT_SLIDE, tc.JNT_HINGE) and model.jnt_limited[j]:
            assert (q[:, qa] > rng[j, 0]).all() and (q[:, qa] < rng[j, 1]).all(), j
    for qa in tc.quaternion_addresses(model):
        assert np.abs(np.linalg.norm(q[:, qa:qa + 4], axis=1) - 1.0).max() < 1e-12
    if name == "tree_convex":
        small = cr.fixture("tree_small")[0]
        for f in ("body_parentid", "body_pos", "body_quat", "jnt_type", "jnt_pos", "jnt_axis", "jnt_range", "geom_pos", "geom_quat"):
            np.testing.assert_array_equal(getattr(model, f), getattr(small, f), err_msg=f)
        np.testing.assert_array_equal(cr.pair_list(tc.limits(name))[0], cr.pair_list(tc.limits("tree_small"))[0])
        assert (np.asarray(model.geom_type) != np.asarray(small.geom_type)).sum() >= 2
        np.testing.assert_array_equal(q, cr.fixture("tree_small")[2])


@pytest.mark.parametrize("name", ["tree_small", "tree_wide", "tree_convex"])
def test_pinned_rows_and_sweeps(name):
    """Colliding and free rows, and the candidates the clearance's and the sweep's filters drop (none)."""
    ref = cr.fixture_ref(name)
    assert int(ref.in_collision.sum()) == tc.PINNED[name]["rows_in_collision"] and 0 < ref.in_collision.sum() < tc.N_ROWS
    assert len(tc.clearance_keep(name)) == tc.N_ROWS - tc.CLEARANCE_DROPPED[name]
    for M in tc.SWEEP_SAMPLES:
        _, _, sweep, keep = tc.sweep_case(name, M)
        assert len(keep) == tc.N_EDGES - tc.SWEEP_DROPPED[(name, M)] and 0 < sweep.in_collision.sum() < tc.N_EDGES
    if name == "tree_convex":
        import convex_check_cases as cc
        conv = cc.convex_mask(cr.fixture(name)[0], tc.limits(name))
        assert conv[ref.pair].any() and not conv[ref.pair].all()     # general convex and analytic pairs both decide rows


@pytest.mark.parametrize("name", TREES)
def test_pinned_verdicts(name):
    """All three verdicts at max_samples = 64 among the edges the device is compared on; at 4 every edge is capped and the
    certificates are (almost) gone."""
    import test_gpu_certified_sweep as tg
    for case, key, ckey in ((name, "verdicts", "capped"), (name + "_capped", "verdicts_at_4", "capped_at_4")):
        _, a, b, resolution, mx, ref, keep = tg.case(case)          # (asserts the pinned number of dropped candidates)
        assert tuple(np.bincount(ref.verdict, minlength=3)) == tc.PINNED[name][key], case
        assert int(ref.capped.sum()) == tc.PINNED[name][ckey] and len(keep) == tc.CERTIFIED_COMPARED[case]
        assert (resolution, len(a)) == (tc.RESOLUTION, tc.CERTIFIED_EDGES[name])
    assert all(v > 0 for v in tc.PINNED[name]["verdicts"])
    _, a, b, _, _, ref, _ = tg.case(name)
    n = tc.CERTIFIED_EDGES[name]
    np.testing.assert_array_equal(a, tc.edges(name)[0][:n])
    np.testing.assert_array_equal(b, tc.edges(name)[1][:n])
    whole = base._case(name)[4]                                  # (all 24 edges: what the two properties below run on)
    np.testing.assert_array_equal(ref.verdict, whole.verdict[:n])
    assert tuple(np.bincount(whole.verdict, minlength=3)) == {"tree_small": (2, 11, 11), "tree_wide": (3, 4, 17)}[name]
    assert int(whole.capped.sum()) == {"tree_small": 0, "tree_wide": 1}[name]


def test_pinned_tracking_case():
    (model, limits, q, q_all), want, counts = tc.tracking()
    assert counts == tc.TRACK_COUNTS, counts
    assert counts["nodes_convex_below_a_ball"] > 0 and counts["edges_convex_below_a_ball"] > 0
    assert 0 < counts["edges_in_collision"] < counts["edges_swept"]


def test_pinned_ladder_case():
    """ladder_certified_cases' case "tree": no instance dropped, all three verdicts among the swept edges, and the two policies
    choose different paths on one instance."""
    import ladder_certified_cases as lc
    c = lc.case("tree")
    st = c["stage"]
    assert c["fixture"] == "tree_small" and c["q_nodes"].shape[:3] == (2, 4, 3) and len(c["keep"]) == 2
    assert int(st["swept"].sum()) == 51
    assert np.bincount(st["edge_verdict_all"][st["swept"]], minlength=3).tolist() == [6, 39, 6]
    assert (c["select"][0]["node_index"] != c["select"][1]["node_index"]).any(axis=1).tolist() == [False, True]


# ------------------------------------------------------------------ the rule's own claims
@pytest.mark.parametrize("name", TREES)
def test_reference_distances_are_lipschitz(name):
    base.test_reference_distances_are_lipschitz(name)


@pytest.mark.parametrize("name", TREES)
def test_certificate_is_sound_on_dense_samples(name):
    base.test_certificate_is_sound_on_dense_samples(name)
    assert (base._case(name)[4].verdict == cf.CERTIFIED).sum() >= 1


# ------------------------------------------------------------------ the reach table by hand
def test_reach_table_of_stacked_joints_closed_form():
    model, pairs = _stack_model()
    assert [int(t) for t in model.jnt_type] == [3, 1, 3, 2] and [int(n) for n in model.body_jntnum] == [0, 1, 1, 2]
    coef = cf.reach_table(model, pairs)
    assert coef.shape == (4, 4, 2)
    np.testing.assert_allclose(coef, STACK_COEF, rtol=1e-12, atol=0)
    # an edge that turns the ball by 0.4 rad about z and moves the slide by 0.05: the ball's weight is the arc's angle
    a = np.array([0.1, 1.0, 0.0, 0.0, 0.0, 0.2, 0.0])
    b = np.array([0.1, np.cos(0.2), 0.0, 0.0, np.sin(0.2), 0.2, 0.05])
    lin, rot = cf.edge_weights(model, a, b)
    np.testing.assert_allclose(lin, [0, 0, 0, 0.05], atol=1e-15)
    np.testing.assert_allclose(rot, [0, 0.4, 0, 0], atol=1e-15)
    np.testing.assert_allclose(cf.pair_motion(coef, lin, rot), [1.03 * 0.4 + 0.05, 1.03 * 0.4 + 0.05, 0.05, 0.28 * 0.4], rtol=1e-12)
    lin2, rot2 = cf.edge_weights(model, a, np.concatenate([b[:1], -b[1:5], b[5:]]))         # (-q: the same arc)
    np.testing.assert_allclose(rot2, rot, atol=1e-15)


def test_host_header_on_stacked_joints(host_cases):  # noqa: F811
    got = base._table(host_cases["stack"])
    assert got.shape == (4, 4, 2)
    np.testing.assert_allclose(got, STACK_COEF, rtol=1e-12, atol=0)
    model, pairs = _stack_model()
    np.testing.assert_allclose(got, cf.reach_table(model, pairs), rtol=1e-12, atol=0)


# ------------------------------------------------------------------ quaternion ends
N_QUAT_EDGES = 8


@pytest.mark.parametrize("name", TREES)
def test_sign_and_scale_of_quaternion_ends_do_not_enter_the_reference(name):
    """The first 8 edges: b with every ball and free quaternion negated; both ends with every such quaternion scaled by its own
    factor in [0.5, 2]."""
    model, limits, a, b, full = base._case(name)
    n = N_QUAT_EDGES
    assert len(tc.quaternion_addresses(model)) == {"tree_small": 6, "tree_wide": 5}[name]
    plain = cf.RefCertified(*[x[:n] for x in full])
    for what, (a2, b2) in (("negated", (a[:n], tc.negated(model, b[:n]))), ("scaled", (tc.scaled(model, a[:n], 1), tc.scaled(model, b[:n], 2)))):
        assert not np.array_equal(b2, b[:n])
        got = cf.certified_sweep(model, limits, a2, b2, tc.RESOLUTION, 64)
        for f in ("margin", "lower_bound", "motion"):
            x, y = getattr(got, f), getattr(plain, f)
            np.testing.assert_array_equal(np.isinf(x), np.isinf(y), err_msg=f"{what}: {f}")
            err = np.abs(x[np.isfinite(y)] - y[np.isfinite(y)]).max()
            print("%s, %s: max |%s - plain| %.2e" % (name, what, f, err))
            assert err <= TOL, (what, f, err)
        for f in ("sample", "pair", "segment", "bound_pair", "n_samples", "capped", "verdict"):
            np.testing.assert_array_equal(getattr(got, f), getattr(plain, f), err_msg=f"{what}: {f}")
        assert np.abs(got.L - plain.L).max() <= TOL
