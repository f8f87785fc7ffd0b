"""Multi-start IK without a GPU: the restated random numbers and seeding rule (tests/multistart_ref.py) have the properties the
header promises, the selection rule behaves on hand-made arrays, the public call validates its arguments before it touches a
device, and the three new kernels are compiled spill-free."""

import json
import os

import numpy as np
import pytest

import multistart_ref as ref
import oracle_configs as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _models():
    import mink_amd
    return {"ur5e": oc.model("ur5e"), "g1": oc.model("g1"), "shadow": oc.model("shadow_left"),
            "ballslide": mink_amd.load_mjcf(os.path.join(GOLDEN, "ballslide.xml")),
            "balllimit": mink_amd.load_mjcf(os.path.join(GOLDEN, "balllimit.xml"))}


def _start(m, B, rng):
    q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (B, 1))
    for j in range(m.njnt):
        if m.jnt_type[j] in (ref.JNT_SLIDE, ref.JNT_HINGE):
            q[:, int(m.jnt_qposadr[j])] += rng.normal(scale=0.05, size=B)
    return q


def test_uniform_is_a_pure_function_in_the_unit_interval():
    t, s, k = np.arange(1000)[:, None, None], np.arange(1, 17)[None, :, None], np.arange(8)[None, None, :]
    u = ref.uniform(5, t, s, k)
    assert u.shape == (1000, 16, 8) and (u >= 0.0).all() and (u < 1.0).all()
    assert np.array_equal(u, ref.uniform(5, t, s, k))
    # one value, whatever else is evaluated beside it
    assert ref.uniform(5, 123, 7, 3) == u[123, 6, 3]
    assert not np.array_equal(u, ref.uniform(6, t, s, k))
    # no two of the 128 000 draws coincide, mean and variance of a uniform variable
    assert len(np.unique(u)) == u.size
    assert abs(u.mean() - 0.5) < 5e-3 and abs(u.var() - 1.0 / 12.0) < 2e-3
    # the 64-bit seed is used in full
    assert ref.uniform(2 ** 63 + 1, 0, 1, 0) != ref.uniform(1, 0, 1, 0)


@pytest.mark.parametrize("name", ["ur5e", "g1", "shadow", "ballslide", "balllimit"])
def test_seeds_follow_the_rule(name):
    m = _models()[name]
    rng = np.random.default_rng(3)
    B, S = 64, 16
    q = _start(m, B, rng)
    seeds = ref.draw_seeds(m, q, S, rng_seed=11)
    assert seeds.shape == (B, S, m.nq)
    assert np.array_equal(seeds[:, 0], q)                                  # seed 0: the caller's q, bit for bit
    # shifting target_index0 by k reproduces rows k... of the unshifted draw
    k = 17
    shifted = ref.draw_seeds(m, q[k:], S, rng_seed=11, target_index0=k)
    assert np.array_equal(shifted, seeds[k:])
    # ... and a target's seeds do not depend on the batch around it
    assert np.array_equal(ref.draw_seeds(m, q[5:6], S, rng_seed=11, target_index0=5)[0], seeds[5])
    for j in range(m.njnt):
        jt, a = int(m.jnt_type[j]), int(m.jnt_qposadr[j])
        lo, hi = m.jnt_range[j]
        if jt == ref.JNT_FREE:
            assert np.array_equal(seeds[:, :, a:a + 7], np.repeat(q[:, None, a:a + 7], S, axis=1))
        elif jt == ref.JNT_BALL:
            quat = seeds[:, 1:, a:a + 4]
            assert np.abs(np.linalg.norm(quat, axis=-1) - 1.0).max() < 1e-15
            angle = 2.0 * np.arctan2(np.linalg.norm(quat[..., 1:], axis=-1), quat[..., 0])
            theta_max = hi if m.jnt_limited[j] else np.pi
            assert (angle <= theta_max * (1 + 1e-15)).all() and angle.std() > 0.05 * theta_max
        elif m.jnt_limited[j]:
            x = seeds[:, 1:, a]
            assert (x >= lo).all() and (x < hi).all()
            assert x.min() < lo + 0.02 * (hi - lo) and x.max() > hi - 0.02 * (hi - lo)    # ... and fill it
        elif jt == ref.JNT_HINGE:
            x = seeds[:, 1:, a] - q[:, None, a]
            assert (x >= -np.pi).all() and (x <= np.pi).all()
        else:
            assert np.array_equal(seeds[:, :, a], np.repeat(q[:, None, a], S, axis=1))
    # distinct seeds of one target, distinct targets
    assert len(np.unique(seeds.reshape(B * S, -1)[:, [int(m.jnt_qposadr[m.njnt - 1])]])) > B * (S - 1) // 2


def test_models_cover_every_seeding_kind():
    ms = _models()
    kinds = set()
    for m in ms.values():
        for j in range(m.njnt):
            kinds.add((int(m.jnt_type[j]), bool(m.jnt_limited[j])))
    assert {(ref.JNT_HINGE, True), (ref.JNT_SLIDE, True), (ref.JNT_BALL, False), (ref.JNT_BALL, True), (ref.JNT_FREE, False)} <= kinds


def test_selection_rule_on_hand_made_arrays():
    d = np.array([3.0, 1.0, 1.0, 0.5])
    # ties go to the lowest index
    assert ref.select(d, [1, 1, 1, 0], [0, 0, 0, 0]) == (1, True, 3)
    # the closest eligible seed wins; OUTSIDE_LIMITS alone is no failure
    assert ref.select(d, [1, 1, 1, 1], [0, 0, 0, 1]) == (3, True, 4)
    # a seed with a failure bit is never chosen, converged flag or not
    for bit in (2, 4, 8, 16, 32):
        assert ref.select(d, [1, 1, 1, 1], [0, 0, 0, bit]) == (1, True, 3)
        assert ref.select(d, [1, 0, 0, 1], [0, 0, 0, bit | 1]) == (0, True, 1)
    # no seed converged: seed 0, not converged — also when seed 0 itself failed
    assert ref.select(d, [0, 0, 0, 0], [0, 0, 0, 0]) == (0, False, 0)
    assert ref.select(d, [0, 1, 1, 1], [2, 2, 4, 8]) == (0, False, 0)
    assert ref.select(np.array([7.0]), [1], [0]) == (0, True, 1)


def test_distance_is_the_tangent_space_difference():
    m = _models()["ballslide"]
    rng = np.random.default_rng(0)
    q0 = ref.draw_seeds(m, np.asarray(m.qpos0, dtype=np.float64)[None], 3, rng_seed=1)[0]
    a, b = q0[1], q0[2]
    assert ref.distance(m, a, a) < 1e-30                                  # (conj(a)·a rounds, it is not exactly 1)
    assert ref.distance(m, a, b) > 0.0
    w = rng.uniform(0.5, 2.0, size=m.nv)
    from oracle import mjmath
    dv = np.zeros(m.nv)
    mjmath.mj_differentiatePos(m, dv, 1.0, b, a)
    assert np.isclose(ref.distance(m, a, b, w), float(w @ (dv * dv)), rtol=1e-15)
    # a quaternion and its negative are the same posture
    j = [j for j in range(m.njnt) if m.jnt_type[j] == ref.JNT_BALL][0]
    qa = int(m.jnt_qposadr[j])
    a2 = a.copy(); a2[qa:qa + 4] *= -1.0
    assert abs(ref.distance(m, a2, b) - ref.distance(m, a, b)) < 1e-12


def test_argument_validation_needs_no_gpu():
    import mink_amd

    m = oc.model("ur5e")
    cfg = mink_amd.Configuration(m, np.tile(np.asarray(m.qpos0), (4, 1)))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    task.set_target(mink_amd.SE3(np.array([1.0, 0, 0, 0, 0.3, 0.2, 0.4])))
    call = lambda **kw: mink_amd.solve_ik_multistart(cfg, [task], 1.0, **{**dict(n_seeds=4, max_iters=10, pos_threshold=1e-4,
                                                                                  ori_threshold=1e-4), **kw})
    with pytest.raises(ValueError, match="n_seeds"):
        call(n_seeds=0)
    with pytest.raises(ValueError, match="max_iters"):
        call(max_iters=0)
    with pytest.raises(ValueError, match="max_instances"):
        call(max_instances=0)
    for bad in (np.zeros((3, m.nq)), np.zeros((4, 4, m.nq + 1)), np.zeros((2, 4, m.nq)), np.zeros(m.nq)):
        with pytest.raises(ValueError, match="seeds must have shape"):
            call(seeds=bad)
    with pytest.raises(ValueError, match="reference must have shape"):
        call(reference=np.zeros((3, m.nq)))
    with pytest.raises(ValueError, match="weights must have shape"):
        call(weights=np.ones(m.nv + 1))
    assert "solve_ik_multistart" in mink_amd.__all__ and "MultistartResult" in mink_amd.__all__
    assert mink_amd.MultistartResult._fields[:7] == ("q", "v", "converged", "seed_index", "n_converged", "iters", "status")
    assert mink_amd.MultistartResult._fields[7:] == ("q_all", "converged_all", "iters_all", "status_all", "seeds")


def test_entry_point_is_declared_bound_and_documented():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    assert "mkh_solve_multistart" in nat.EXPORTED_SYMBOLS
    L = nat.lib()
    assert L.mkh_solve_multistart is not None
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    import ctypes
    assert ctypes.sizeof(nat.MkhMultistartIO) == 15 * ctypes.sizeof(ctypes.c_void_p)
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "minkhip.h")).read()
    fields = hdr.split("typedef struct MkhMultistartIO {")[1].split("} MkhMultistartIO;")[0]
    import re
    assert tuple(re.findall(r"\*(\w+);", fields)) == nat.MULTISTART_IO_FIELDS                 # same order as the ctypes mirror
    for word in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15", "target_index0", "mj_differentiatePos"):
        assert word in hdr, word
    # null / bad arguments fail loudly before any device is touched
    io = nat.MkhMultistartIO()
    assert L.mkh_solve_multistart(None, 1, None, None, None, None, 1.0, 1e-3, 10, 1e-4, 1e-4, 4, 0, 0, ctypes.byref(io), 0, None) == -1
    assert b"null problem" in L.mkh_last_error()


def test_new_kernels_are_spill_free_without_scratch():
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    for k in ("multistart_seed_kernel", "multistart_fanout_kernel", "multistart_select_kernel"):
        e = table.get(k)
        assert e is not None, sorted(x for x in table if "multistart" in x)
        assert e["vgpr_spills_with_callees"] == 0 and e["sgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0, (k, e)
        assert e["callees"] == {}, (k, e["callees"])                  # everything inlined: no call, no stack
