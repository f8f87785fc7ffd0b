"""Seed tables without a GPU: the restated metric and K-best rule (tests/seed_table_ref.py) behave on hand-made arrays, SeedTable
and the two seed_table= keywords validate their arguments before they touch a device, the five entry points are declared, bound
and documented, the new kernels are compiled spill-free, and the fixture of the GPU query test is well-posed: no two of the
distances it has to rank are closer than rounding could reorder."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import multistart_ref as mref
import oracle_configs as oc
import seed_table_ref as ref
from oracle import ik as oik

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pose(quat, pos):
    return np.concatenate([np.asarray(quat, dtype=np.float64), np.asarray(pos, dtype=np.float64)])


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def test_metric_and_k_best_on_hand_made_arrays():
    one = np.ones(1)
    keys = np.stack([_pose(_rot([0, 0, 1], 0.3), [0.1, 0.2, 0.3]), _pose(_rot([1, 0, 0], 1.0), [0.4, 0.0, 0.3]),
                     _pose(_rot([0, 1, 0], 2.0), [-0.2, 0.2, 0.1]), _pose(_rot([1, 0, 0], 1.0), [0.4, 0.0, 0.3])])[:, None, :]
    tg = keys[[1, 2]].copy()
    d = ref.distances(tg, keys, one, one)
    assert d.shape == (2, 4)
    # a target equal to an entry: d = 0, exactly; the duplicate pair (1, 3) ties and the lower index comes first
    assert d[0, 1] == 0.0 and d[0, 3] == 0.0 and d[1, 2] == 0.0
    idx, dist = ref.k_best(d, 3)
    assert idx[0].tolist()[:2] == [1, 3] and idx[1, 0] == 2 and idx.dtype == np.int32
    assert (np.diff(dist, axis=1) >= 0.0).all()
    # position and orientation parts: |dp|^2 and 4 sin^2(theta / 2) of the relative rotation
    a, b = _pose(_rot([0, 0, 1], 0.2), [0, 0, 0]), _pose(_rot([0, 0, 1], 0.5), [0.3, 0.0, 0.4])
    dab = ref.distances(a[None, None], b[None, None], one, one)[0, 0]
    assert np.isclose(dab, 0.25 + 4 * np.sin(0.15) ** 2, rtol=1e-14)
    assert np.isclose(ref.distances(a[None, None], b[None, None], one, 0 * one)[0, 0], 0.25, rtol=1e-15)
    assert np.isclose(ref.distances(a[None, None], b[None, None], 0 * one, 3 * one)[0, 0], 12 * np.sin(0.15) ** 2, rtol=1e-14)
    # -q and 2 q targets: the distances of q (the sign exactly; the scale to rounding)
    neg, twice = tg.copy(), tg.copy()
    neg[:, :, :4] *= -1.0; twice[:, :, :4] *= 2.0
    assert np.array_equal(ref.distances(neg, keys, one, one), d)
    assert np.allclose(ref.distances(twice, keys, one, one), d, rtol=0, atol=1e-15)
    assert np.array_equal(ref.k_best(ref.distances(twice, keys, one, one), 4)[0], ref.k_best(d, 4)[0])
    # a NaN target sorts last: every distance DBL_MAX, the first K entries
    bad = tg.copy(); bad[1, 0, 5] = np.nan
    db = ref.distances(bad, keys, one, one)
    assert (db[1] == ref.DBL_MAX).all() and np.array_equal(db[0], d[0])
    assert ref.k_best(db, 3)[0][1].tolist() == [0, 1, 2]
    nanq = tg.copy(); nanq[0, 0, 0] = np.nan
    assert (ref.distances(nanq, keys, one, 0 * one)[0] == ref.DBL_MAX).all()           # (0 · NaN is a NaN: still last)
    zero = tg.copy(); zero[0, 0, :4] = 0.0
    assert (ref.distances(zero, keys, one, one)[0] == ref.DBL_MAX).all()
    # frames are summed; default weights from the descriptors
    two = np.concatenate([keys, keys[::-1]], axis=1)
    d2 = ref.distances(two[[0]], two, np.array([1.0, 2.0]), np.array([0.0, 1.0]))
    want = ref.distances(keys[[0]], keys, one, 0 * one) + ref.distances(keys[::-1][[0]], keys[::-1], 2 * one, one)
    assert np.allclose(d2, want, rtol=1e-15)
    fts = [{"cost": [1, 1, 1, 0, 0, 0]}, {"cost": [0, 0, 0, 0, 2, 0]}, {"cost": [1] * 6, "root_type": "body"}, {"cost": [0] * 6}]
    wp, wo = ref.default_weights(fts)
    assert wp.tolist() == [1, 0, 0, 0] and wo.tolist() == [0, 1, 0, 0]
    assert np.allclose(ref.relative_gaps(np.array([[4.0, 1.0, 2.0]]), 2), [[0.5, 0.5]])


def _ur5e_call_site(B=4):
    import mink_amd
    m = oc.model("ur5e")
    cfg = mink_amd.Configuration(m, np.tile(np.asarray(m.qpos0), (B, 1)))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    task.set_target(mink_amd.SE3(np.array([1.0, 0, 0, 0, 0.3, 0.2, 0.4])))
    return mink_amd, m, cfg, task


def test_argument_validation_needs_no_gpu():
    mink, m, cfg, task = _ur5e_call_site()
    one = mink.Configuration(m, np.asarray(m.qpos0))
    make = lambda *a, **kw: mink.SeedTable(one, [task], *a, **kw)
    with pytest.raises(ValueError, match="single q"):
        mink.SeedTable(cfg, [task], 64)
    with pytest.raises(ValueError, match="n_entries"):
        make(0)
    for bad in (np.zeros(m.nq), np.zeros((4, m.nq + 1)), np.zeros((0, m.nq))):
        with pytest.raises(ValueError, match="entries must have shape"):
            make(entries=bad)
    with pytest.raises(ValueError, match="position_weight must have shape"):
        make(64, position_weight=np.ones(2))
    with pytest.raises(ValueError, match="orientation_weight must be finite"):
        make(64, orientation_weight=np.array([-1.0]))
    with pytest.raises(ValueError, match="position_weight must be finite"):
        make(64, position_weight=np.array([np.nan]))
    with pytest.raises(ValueError, match="all 0"):
        make(64, position_weight=np.zeros(1), orientation_weight=np.zeros(1))
    posture = mink.PostureTask(m, 1.0)
    with pytest.raises(ValueError, match="no plain FrameTask"):
        mink.SeedTable(one, [posture], 64)
    costless = mink.FrameTask("attachment_site", "site", 0.0, 0.0)
    with pytest.raises(ValueError, match="no plain FrameTask"):
        mink.SeedTable(one, [costless], 64)
    tab = make(64)
    assert tab.n_entries == 64 and tab.n_frame == 1 and tab.position_weight.tolist() == [1.0] and tab.orientation_weight.tolist() == [1.0]
    assert make(entries=np.zeros((5, m.nq))).n_entries == 5
    assert mink.SeedTable(mink.Configuration(m, np.asarray(m.qpos0)[None]), [task], 8).q0.shape == (m.nq,)
    pos_only = mink.FrameTask("attachment_site", "site", 1.0, 0.0)
    assert mink.SeedTable(one, [pos_only, posture], 8).orientation_weight.tolist() == [0.0]
    for k, word in ((0, "must be >= 1"), (256, "at most 255"), (65, "exceeds the seed table's 64 entries")):
        with pytest.raises(ValueError, match=word):
            tab.query(np.zeros((3, 7)), k)
    with pytest.raises(ValueError, match="targets must have shape"):
        tab.query(np.zeros((3, 2, 7)), 4)
    # the two keywords
    ms = lambda **kw: mink.solve_ik_multistart(cfg, [task], 1.0, **{**dict(n_seeds=4, max_iters=10, pos_threshold=1e-4,
                                                                          ori_threshold=1e-4), **kw})
    poses = np.tile(np.array([1.0, 0, 0, 0, 0.3, 0.2, 0.4]), (4, 3, 1))
    tms = lambda **kw: mink.solve_ik_trajectory_multistart(cfg, [task], 1.0, {task: poses}, **{**dict(
        n_seeds=4, n_steps=10, pos_threshold=1e-4, ori_threshold=1e-4), **kw})
    mg = oc.model("g1")
    other = mink.SeedTable(mink.Configuration(mg, np.asarray(mg.qpos0)), [mink.FrameTask("left_foot", "site", 1.0, 1.0)], 64)
    for call in (ms, tms):
        with pytest.raises(ValueError, match="seeds and seed_table"):
            call(seed_table=tab, seeds=np.zeros((4, m.nq)))
        with pytest.raises(ValueError, match="must be a SeedTable"):
            call(seed_table=object())
        with pytest.raises(ValueError, match="another model"):
            call(seed_table=other)
        with pytest.raises(ValueError, match="exceeds the seed table's 2 entries"):
            call(seed_table=make(2))
        with pytest.raises(ValueError, match="at most 255"):
            call(seed_table=make(512), n_seeds=257)
    assert "SeedTable" in mink.__all__
    tab.close()
    with pytest.raises(ValueError, match="closed"):
        tab.query(np.zeros((3, 7)), 4)


NEW_FUNCTIONS = ("mkh_seed_table_create", "mkh_seed_table_destroy", "mkh_seed_table_read", "mkh_seed_table_query",
                 "mkh_problem_set_seed_table")


def test_entry_points_are_declared_bound_and_documented():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "minkhip.h")).read()
    for f in NEW_FUNCTIONS:
        assert f in nat.EXPORTED_SYMBOLS, f
        assert getattr(L, f) is not None
        assert re.search(r"^(int32_t|void) " + f + r"\(", hdr, re.M), f
    assert "typedef struct MkhSeedTable MkhSeedTable;" in hdr
    for word in ("max(0, 4 * (1 - c*c))", "sqrt(n_T * n_e)", "DBL_MAX", "ties go to the lower entry index", "K <= 255",
                 "frame_pose tap of mkh_eval", "io->seeds IS NULL"):
        assert word in hdr, word
    # null / bad arguments fail loudly before any device is touched
    h = ctypes.c_void_p()
    assert L.mkh_seed_table_create(None, 4, None, None, 0, None, None, ctypes.byref(h)) == -1
    assert b"null" in L.mkh_last_error()
    assert L.mkh_seed_table_read(None, None, None) == -1
    assert L.mkh_seed_table_query(None, 1, None, 1, None, None, None, 0, None) == -1
    assert b"null seed table" in L.mkh_last_error()
    assert L.mkh_problem_set_seed_table(None, None) == -1
    L.mkh_seed_table_destroy(None)


def test_new_kernels_are_spill_free_without_scratch():
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    for k in ("seed_table_keys_kernel", "seed_table_query_kernel"):
        e = table.get(k)
        assert e is not None, sorted(x for x in table if "seed_table" in x)
        assert e["vgpr_spills_with_callees"] == 0 and e["sgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0, (k, e)
        assert e["callees"] == {}, (k, e["callees"])                  # everything inlined: no call, no stack


def test_gpu_query_fixture_is_well_posed():
    """The fixture of test_gpu_seed_table.py::test_query_is_the_stated_rule by the numpy oracle's kinematics: UR5e tables of 63 …
    4 099 entries drawn around `home` with rng_seed 11, the first 37 far targets, K up to 63.  The GPU test demands indices
    equal to the restatement's; that is safe when the distances it ranks are further apart than the two sides can differ: the
    keys are the device's own on both sides, so only the metric's last-place rounding can differ, ~1e-15 relative — a gap of
    1e-9 relative between ranks 1 … K + 1 leaves six orders of magnitude.  Measured here: the smallest relative gap over ranks
    1 … 64 is 1.9e-6 at N = 63 … 65, 4.2e-6 at N = 1000 and 9.7e-6 at N = 4099."""
    m = oc.model("ur5e")
    sid = m.name2id("site", "attachment_site")
    home = np.array(m.key_qpos[m.name2id("key", "home")], dtype=np.float64)
    fk = lambda qs: np.stack([oik.Configuration(m, q).get_transform_frame_to_world(sid, "site") for q in qs])[:, None, :]
    rng = np.random.default_rng(20261016)                                   # (test_gpu_multistart._far_targets)
    lo, hi = np.maximum(m.jnt_range[:, 0], -np.pi), np.minimum(m.jnt_range[:, 1], np.pi)
    tg = fk(rng.uniform(lo, hi, size=(37, m.nq)))
    entries = mref.draw_seeds(m, np.tile(home, (4099, 1)), 2, rng_seed=11)[:, 1]
    keys = fk(entries)
    one = np.ones(1)
    for N in (63, 64, 65, 1000, 4099):
        K = min(63, N - 1)
        gaps = ref.relative_gaps(ref.distances(tg, keys[:N], one, one), K)
        print(f"N = {N}: smallest relative gap among ranks 1 ... {K + 1} over 37 targets = {gaps.min():.3e}")
        assert gaps.min() > 1e-9, N
