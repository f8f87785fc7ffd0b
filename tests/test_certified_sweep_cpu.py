"""THE RULE OF THE CERTIFIED SWEEP (include/minkhip.h) without a device: the numpy restatement tests/certified_ref.py against
hand-typed numbers and against its own claims, and the host header mink_amd/csrc/motion_bound.h under the host sanitizers.

* The reach table of a hand-typed planar chain — two hinges and a limited slide, a plane, a sphere, a capsule and a box — against
  coefficients worked out by hand below.
* The Lipschitz property the proof rests on: along every edge, consecutive reference distances of every pair differ by at most
  L_k h (+ 1e-9, the project's tolerance for a margin), h the step in u.  Edges: the fixtures' own row pairs, shortened to
  b = a (+) s (b0 (-) a) with s = 0.1 — `ur5e_all` 40, `shapes` 12, `g1` 8 with the base turned by 0.5 .. 2 rad and shifted —,
  walked at the rule's own points for resolution 0.02.  The worst |dd_k| / (L_k h) is printed; it must not exceed 1, and the bound
  must not be vacuous: a worst ratio below 0.1 would mean ten times the samples any edge needs (the rule's own reach terms are
  triangle inequalities along the chain, loose by the chain's folding and no more).
* The soundness of the certificate: on the certified edges, 121 dense reference samples never fall below lower_bound - 1e-9.
* motion_bound.h: tests/host/motion_bound_cases.cpp walks it over the hand-typed chain, an unlimited slide and a plane on a moving
  body (the last two give infinite coefficients) — compiled with the host's address and undefined-behaviour sanitizers, run as a
  child process, nothing loaded into Python; beside the tables, checker_plan.h's two refusals of a certified sweep."""

import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import certified_ref as cf
import clearance_ref as cr
import keyframe_ref as kf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mink_amd", "csrc")
MKH_E_INVALID, MKH_E_LIMIT = -1, -4            # include/minkhip.h
TOL = 1e-9

CHAIN_MJCF = """<mujoco><compiler angle="radian"/><worldbody>
  <geom name="floor" type="plane" size="1 1 0.1"/>
  <body name="b1" pos="0 0 0.5">
    <joint name="h1" type="hinge" axis="0 1 0" pos="0.1 0 0"/>
    <geom name="ball" type="sphere" size="0.05" pos="0.2 0 0" mass="0.1"/>
    <body name="b2" pos="0.3 0 0">
      <joint name="h2" type="hinge" axis="0 1 0" pos="0 0 0.04"/>
      <geom name="rod" type="capsule" size="0.03 0.1" pos="0.1 0 0" mass="0.1"/>
      <body name="b3" pos="0.4 0 0">
        <joint name="s3" type="slide" axis="1 0 0" range="-0.1 0.2"/>
        <geom name="brick" type="box" size="0.03 0.04 0.12" pos="0 0 0.05" mass="0.1"/>
      </body>
    </body>
  </body>
</worldbody></mujoco>"""
CHAIN_PAIRS = [("floor", "brick"), ("ball", "brick"), ("rod", "brick"), ("floor", "ball")]
# Worked out by hand.  r(brick) = |(0.03, 0.04, 0.12)| = 0.13, |geom_pos(brick)| = 0.05; D(b3) = max(|-0.1|, |0.2|) = 0.2 (its slide);
# D(b2) = 2 |jnt_pos(h2)| = 0.08.
#   floor-brick: the brick hangs on b1 -> b2 -> b3, the floor on the world.
#     h1 on b1:  0.1 + 0 + (0.3 + 0.08) + (0.4 + 0.2) + 0.05 + 0.13 = 1.26
#     h2 on b2:  0.04 + 0 + (0.4 + 0.2) + 0.05 + 0.13               = 0.82
#     s3 on b3:  linear 1, angular 0
#   ball-brick: b1 is a common ancestor (h1: 0, 0); the ball's own remaining chain is empty.  h2 and s3 as above.
#   rod-brick:  b1 and b2 are common; s3 alone.
#   floor-ball: h1: 0.1 + 0 + 0.2 + 0.05 = 0.35; h2 and s3 do not carry the ball.
CHAIN_COEF = np.array([[[0, 1.26], [0, 0.82], [1, 0]],
                       [[0, 0], [0, 0.82], [1, 0]],
                       [[0, 0], [0, 0], [1, 0]],
                       [[0, 0.35], [0, 0], [0, 0]]], dtype=np.float64)


def _chain_model():
    from mink_amd.mjcf import loads_mjcf
    model = loads_mjcf(CHAIN_MJCF)
    pairs = [(model.name2id("geom", a), model.name2id("geom", b)) for a, b in CHAIN_PAIRS]
    return model, pairs


def test_reach_table_closed_form():
    model, pairs = _chain_model()
    coef = cf.reach_table(model, pairs)
    assert coef.shape == (4, 3, 2)
    np.testing.assert_allclose(coef, CHAIN_COEF, rtol=1e-12, atol=0)
    assert [cf.geom_radius(model, g) for g, _ in pairs[1:3]] == [0.05, 0.03 + 0.1]
    assert cf.geom_radius(model, pairs[0][0]) == np.inf
    # the weights of an edge and its motion: h1 by 0.5 rad, h2 by -0.25, the slide by 0.1
    a, b = np.array([0.1, 0.2, 0.0]), np.array([0.6, -0.05, 0.1])
    lin, rot = cf.edge_weights(model, a, b)
    np.testing.assert_allclose(lin, [0, 0, 0.1], atol=1e-15)
    np.testing.assert_allclose(rot, [0.5, 0.25, 0], atol=1e-15)
    L = cf.pair_motion(coef, lin, rot)
    np.testing.assert_allclose(L, [1.26 * 0.5 + 0.82 * 0.25 + 0.1, 0.82 * 0.25 + 0.1, 0.1, 0.35 * 0.5], rtol=1e-12)
    assert cf.sample_count(L.max(), False, 0.02, 64) == (46, 0)         # ceil(0.935 / 0.02) - 1
    assert cf.sample_count(L.max(), False, 0.01, 64) == (64, 1)
    assert cf.sample_count(0.0, False, 0.02, 64) == (1, 0)
    assert cf.sample_count(np.inf, True, 0.02, 64) == (64, 1)
    # an infinite coefficient against a weight of 0 contributes 0
    inf = coef.copy()
    inf[0, 1, 1] = np.inf
    assert np.isfinite(cf.pair_motion(inf, lin, np.array([0.5, 0.0, 0.0]))).all()
    assert cf.pair_motion(inf, lin, rot)[0] == np.inf


def _shortened(model, a, b0, s):
    return np.stack([kf.blend_posture(model, x, y, s) for x, y in zip(a, b0)])


def _turned_base(q, rng):
    """q with its base quaternion turned by 0.5 .. 2 rad about a random axis and the base shifted by up to 0.3 m."""
    out = q.copy()
    for i in range(len(q)):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(0.5, 2.0)
        r = np.concatenate([[np.cos(0.5 * ang)], np.sin(0.5 * ang) * axis])
        w0, v0 = q[i, 3], q[i, 4:7]
        out[i, 3:7] = np.concatenate([[w0 * r[0] - v0 @ r[1:]], w0 * r[1:] + r[0] * v0 + np.cross(v0, r[1:])])
        out[i, :3] += rng.uniform(-0.3, 0.3, size=3)
    return out


_cases = {}


def _case(name):
    """(model, limits, a, b, RefCertified at resolution 0.02) of a fixture's shortened edges, computed once.  The random trees
    of tests/tree_cases.py (tests/test_tree_checker_cpu.py runs the two properties on them): their own 24 edges, s = 0.3, at
    resolution 0.05."""
    if name not in _cases and name.startswith("tree_"):
        import tree_cases as tc
        model, limits, (a, b) = cr.fixture(name)[0], tc.limits(name), tc.edges(name)
        _cases[name] = (model, limits, a, b, cf.certified_sweep(model, limits, a, b, tc.RESOLUTION, 64))
    if name not in _cases:
        model, _, q = cr.fixture(name)
        n = {"ur5e_all": 40, "shapes": 12, "g1": 8}[name]
        a, b0 = q[:n].copy(), q[n:2 * n].copy()
        if name == "g1":
            b0 = _turned_base(b0, np.random.default_rng(5))
        b = _shortened(model, a, b0, 0.1)
        limits = cr.limits_of(cr.fixture_limits(name))
        _cases[name] = (model, limits, a, b, cf.certified_sweep(model, limits, a, b, 0.02, 64))
    return _cases[name]


@pytest.mark.parametrize("name", ["ur5e_all", "shapes", "g1"])
def test_reference_distances_are_lipschitz(name):
    model, limits, a, b, ref = _case(name)
    dmin = cr.pair_list(limits)[1]
    worst = 0.0
    for e in range(len(a)):
        assert np.isfinite(ref.L[e]).all() and ref.points[e] is not None
        d = ref.points[e] + dmin[None, :]                       # (M + 2, P)
        h = 1.0 / (int(ref.n_samples[e]) + 1)
        step = np.abs(np.diff(d, axis=0))
        assert (step <= ref.L[e][None, :] * h + TOL).all(), (name, e, (step - ref.L[e][None, :] * h).max())
        moving = ref.L[e] > 0.0
        if moving.any():
            worst = max(worst, float((step[:, moving] / (ref.L[e][moving] * h)[None, :]).max()))
    print("%s: %d edges, worst |dd_k| / (L_k h) = %.3f, n_samples %d .. %d" % (name, len(a), worst, ref.n_samples.min(), ref.n_samples.max()))
    assert 0.1 < worst <= 1.0


@pytest.mark.parametrize("name", ["ur5e_all", "shapes", "g1"])
def test_certificate_is_sound_on_dense_samples(name):
    model, limits, a, b, ref = _case(name)
    dmin = cr.pair_list(limits)[1]
    certified = np.nonzero(ref.verdict == cf.CERTIFIED)[0]
    print("%s: %d certified, %d colliding, %d undecided of %d" % (name, len(certified), (ref.verdict == cf.COLLIDES).sum(),
                                                                  (ref.verdict == cf.UNDECIDED).sum(), len(a)))
    assert (ref.lower_bound[certified] >= 0.0).all() and (ref.margin[certified] >= ref.lower_bound[certified]).all()
    slack = np.inf
    for e in certified:
        rows = np.stack([kf.blend_posture(model, a[e], b[e], float(i) / 120.0) for i in range(121)])
        m = (cr.distances(model, limits, rows) - dmin[None, :]) + 0.0
        slack = min(slack, float(m.min() - ref.lower_bound[e]))
        assert m.min() >= ref.lower_bound[e] - TOL, (name, e, m.min(), ref.lower_bound[e])
    print("%s: smallest dense margin - lower_bound = %.3e" % (name, slack))
    if name != "g1":
        assert len(certified) > 0                               # (the arms' short edges: some are free with room to spare)


def test_verdicts_and_special_edges_of_the_reference():
    model, limits, a, b, ref = _case("ur5e_all")
    # an edge from a row to itself: no motion, one sample, the bound is the margin
    own = cf.certified_sweep(model, limits, a[:3], a[:3], 0.02, 64)
    assert (own.motion == 0.0).all() and (own.n_samples == 1).all() and (own.sample == 0).all() and (own.segment == 0).all()
    np.testing.assert_array_equal(own.lower_bound, own.margin)
    np.testing.assert_array_equal(own.verdict, np.where(own.margin >= 0.0, cf.CERTIFIED, cf.COLLIDES))
    # non-finite ends
    bad_a = a[:2].copy()
    bad_a[0, 1] = np.nan
    bad = cf.certified_sweep(model, limits, bad_a, b[:2], 0.02, 64)
    assert np.isnan(bad.margin[0]) and np.isnan(bad.lower_bound[0]) and np.isnan(bad.motion[0])
    assert (bad.sample[0], bad.pair[0], bad.segment[0], bad.bound_pair[0], bad.capped[0], bad.n_samples[0], bad.verdict[0]) == (0, 0, 0, 0, 0, 1, 2)
    assert bad.verdict[1] == ref.verdict[1] and bad.margin[1] == ref.margin[1]
    # the verdict is a function of margin and lower_bound
    want = np.where(~(ref.margin >= 0.0), cf.COLLIDES, np.where(ref.lower_bound >= 0.0, cf.CERTIFIED, cf.UNDECIDED))
    np.testing.assert_array_equal(ref.verdict, want)


@pytest.fixture(scope="module")
def host_cases(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("motion_bound_cases")
    flags = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
             "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC]
    src, obj, exe = os.path.join(REPO, "tests", "host", "motion_bound_cases.cpp"), str(d / "motion_bound_cases.o"), str(d / "motion_bound_cases")
    r = subprocess.run([hipcc] + flags + ["-c", src, "-o", obj], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    subprocess.run([hipcc, "--offload-host-only", "-Xarch_host", "-fsanitize=address,undefined", obj, "-o", exe], check=True)   # (host code only: the sanitizers never see the device)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]             # the sanitized run: nothing reported
    return {c["case"]: c for c in (json.loads(line) for line in r.stdout.splitlines())}


def _table(c):
    return np.array([float(x) for x in c["coef"]]).reshape(c["n_pairs"], c["njnt"], 2)


def test_host_header_under_sanitizers(host_cases):
    inf = np.inf
    np.testing.assert_allclose(_table(host_cases["chain"]), CHAIN_COEF, rtol=1e-12, atol=0)
    # ... and the numpy restatement on the MJCF the arrays were typed from
    model, pairs = _chain_model()
    np.testing.assert_allclose(_table(host_cases["chain"]), cf.reach_table(model, pairs), rtol=1e-12, atol=0)
    # an unlimited slide: D(b3) = inf reaches every joint above it that carries the brick; the slide itself stays (1, 0)
    np.testing.assert_array_equal(_table(host_cases["unlimited_slide"]),
                                  [[[0, inf], [0, inf], [1, 0]], [[0, 0], [0, inf], [1, 0]], [[0, 0], [0, 0], [1, 0]], [[0, 0.35], [0, 0], [0, 0]]])
    # the plane on b3: r = inf for every rotation that carries it; against the ball b1 is common
    got = _table(host_cases["plane_on_moving_body"])
    np.testing.assert_array_equal(got[0], [[0, 0], [0, 0], [0, 0]])                 # plane and brick on one body: nothing moves them apart
    np.testing.assert_array_equal(got[3], [[0, 0], [0, inf], [1, 0]])
    np.testing.assert_allclose(got[1:3], CHAIN_COEF[1:3], rtol=1e-12, atol=0)


def test_plan_refusals_of_a_certified_sweep(host_cases):
    for name in ("served_quarter", "served_whole", "lds_fits"):
        assert (host_cases[name]["rc"], host_cases[name]["err"]) == (0, ""), name
    assert host_cases["served_quarter"]["lds"] == 4 * (7 * 9 + 3 * 6 + 3 * 14) * 8      # the sweep's slice plus three rows of pairs, four groups
    assert host_cases["served_whole"]["lds"] == (7 * 21 + 3 * 20 + 3 * 60) * 8
    assert host_cases["lds_fits"]["lds"] <= 64 * 1024 < host_cases["lds_over"]["lds"]
    for name in ("convex", "convex_with_sweep_rows"):
        assert host_cases[name]["rc"] == MKH_E_INVALID and "not certified yet" in host_cases[name]["err"], host_cases[name]
        assert host_cases[name]["err"].startswith("mkh_certified_sweep: the checker has general convex pairs")
    assert host_cases["lds_over"]["rc"] == MKH_E_LIMIT and "do not fit 64 KB of LDS" in host_cases["lds_over"]["err"]
    assert host_cases["no_pairs"]["rc"] == MKH_E_INVALID and "has no collision pairs" in host_cases["no_pairs"]["err"]
