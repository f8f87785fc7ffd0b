"""Keyframed trajectory IK without a GPU: the numpy restatement of the interpolation rule (tests/keyframe_ref.py) against first
principles and the oracle's mj_differentiatePos / mj_integratePos, the refusals of the rule raised before any device is
touched (C ABI and public API), the entry point exported, bound and mirrored field for field, and the new kernels compiled
spill-free."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import keyframe_ref as ref
import oracle_configs as oc
from oracle import lie, mjmath

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(name):
    import mink_amd
    if name == "ballslide":
        return mink_amd.load_mjcf(os.path.join(GOLDEN, "ballslide.xml"))
    if name == "h1":
        from mink_amd import workloads
        return workloads.load_robot("h1")
    return oc.model(name)


def _unit(rng, n=None):
    q = rng.normal(size=(4,) if n is None else (n, 4))
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _random_postures(m, n, rng):
    q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (n, 1)) + rng.normal(scale=0.3, size=(n, m.nq))
    for j in range(m.njnt):
        jt, a = int(m.jnt_type[j]), int(m.jnt_qposadr[j])
        if jt in (ref.JNT_FREE, ref.JNT_BALL):
            a += 3 if jt == ref.JNT_FREE else 0
            q[:, a:a + 4] = _unit(rng, n)
    return q


def _quat_mask(m):
    mask = np.zeros(m.nq, dtype=bool)
    for j in range(m.njnt):
        jt, a = int(m.jnt_type[j]), int(m.jnt_qposadr[j])
        if jt in (ref.JNT_FREE, ref.JNT_BALL):
            a += 3 if jt == ref.JNT_FREE else 0
            mask[a:a + 4] = True
    return mask


def test_segment_choice():
    kt = [0.0, 0.5, 2.0, 2.25]
    assert ref.segment(kt, 0.0) == (0, 0.0)
    assert ref.segment(kt, 0.5) == (1, 0.0)                      # on a keyframe: u == 0, the later segment
    assert ref.segment(kt, 2.25) == (3, 0.0)                     # the last keyframe: a copy
    k, u = ref.segment(kt, 1.25)
    assert (k, u) == (1, 0.5)
    k, u = ref.segment(kt, 0.3)
    assert k == 0 and u == (0.3 - 0.0) / (0.5 - 0.0)
    k, u = ref.segment(kt, np.nextafter(2.0, 0.0))
    assert k == 1 and 0.0 < u < 1.0
    assert ref.segment([1.5], 1.5) == (0, 0.0)                   # K = 1
    for bad_k, bad_w in (([0.0, 0.0, 1.0], [0.5]), ([0.0, 1.0, 0.5], [0.5]), ([0.0, 1.0], [0.5, 0.25]), ([0.0, 1.0], [-1e-9]),
                         ([0.0, 1.0], [1.0 + 1e-9]), ([0.0, np.nan], [0.5]), ([0.0, 1.0], [np.nan]), ([], [0.0]), ([0.0], [])):
        with pytest.raises(ValueError):
            ref.check_times(bad_k, bad_w)


def test_pose_blend_from_first_principles():
    rng = np.random.default_rng(3)
    for _ in range(20):
        R = _unit(rng)
        w = rng.normal(size=3)
        w *= rng.uniform(0.0, 2.9) / np.linalg.norm(w)
        a = np.concatenate([R, rng.normal(size=3)])
        b = np.concatenate([lie.so3_multiply(R, lie.so3_exp(w)), rng.normal(size=3)])
        mid = ref.blend_pose(a, b, 0.5)
        want = lie.so3_multiply(R, lie.so3_exp(0.5 * w))
        # the midpoint of R and R exp(w) is R exp(w / 2) — as a rotation: q and -q are the same one
        assert np.abs(lie.so3_as_matrix(mid[:4]) - lie.so3_as_matrix(want)).max() < 1e-13
        assert abs(np.linalg.norm(mid[:4]) - 1.0) < 1e-15
        assert np.array_equal(mid[4:], a[4:] + 0.5 * (b[4:] - a[4:]))
        # +-q_b and +-q_a give the same rotation (the shortest arc whatever the signs)
        u = rng.uniform(0.05, 0.95)
        got = lie.so3_as_matrix(ref.blend_pose(a, b, u)[:4])
        flip = np.array([-1.0] * 4 + [1.0] * 3)
        for a2, b2 in ((a, b * flip), (a * flip, b), (a * flip, b * flip)):
            assert np.abs(lie.so3_as_matrix(ref.blend_pose(a2, b2, u)[:4]) - got).max() < 1e-13
        assert np.array_equal(ref.blend_pose(a, b, 0.0), a)
    # a relative rotation below both small-angle thresholds, and identical keyframes
    R = _unit(rng)
    a = np.concatenate([R, np.zeros(3)])
    b = np.concatenate([lie.so3_multiply(R, lie.so3_exp(np.array([3e-7, -2e-7, 1e-7]))), np.ones(3)])
    mid = ref.blend_pose(a, b, 0.5)
    assert np.abs(mid[:4] - lie.so3_multiply(R, lie.so3_exp(0.5 * np.array([3e-7, -2e-7, 1e-7])))).max() < 1e-15
    same = ref.blend_pose(a, a, 0.3)
    assert np.abs(same - a).max() < 1e-15


@pytest.mark.parametrize("name", ["ballslide", "h1"])
def test_posture_blend_is_integratePos_of_differentiatePos(name):
    m = _model(name)
    rng = np.random.default_rng(8)
    q = _random_postures(m, 12, rng)
    quat = _quat_mask(m)
    assert quat.any() and (~quat).any()
    worst = 0.0
    for i in range(0, 12, 2):
        a, b = q[i], q[i + 1]
        for u in (0.25, 0.5, 0.8125, rng.uniform(0.01, 0.99)):
            v = np.zeros(m.nv)
            mjmath.mj_differentiatePos(m, v, 1.0, a, b)
            want = a.copy()
            mjmath.mj_integratePos(m, want, v, u)
            got = ref.blend_posture(m, a, b, u)
            assert np.array_equal(got[~quat], want[~quat])          # a difference, a product, a sum: exact
            worst = max(worst, float(np.abs(got[quat] - want[quat]).max()))
            assert np.abs(got[quat] - want[quat]).max() < 1e-14     # (the restatement normalises once more)
        assert np.array_equal(ref.blend_posture(m, a, b, 0.0), a)
    print(f"{name}: quaternion entries, max |restatement - oracle| = {worst:.2e}")


def test_waypoints_on_keyframes_are_copies_and_layouts_agree():
    rng = np.random.default_rng(5)
    B, K, n = 3, 4, 2
    kt = np.array([0.0, 0.4, 1.0, 1.7])
    keys = np.concatenate([_unit(rng, B * K * n).reshape(B, K, n, 4), rng.normal(size=(B, K, n, 3))], axis=-1)
    wt = np.array([0.0, 0.4, 0.4, 0.7, 1.7, 1.7])
    out = ref.interpolate(keys, kt, wt, "frame")
    assert out.shape == (B, len(wt), n, 7)
    for t, k in ((0, 0), (1, 1), (2, 1), (4, 3), (5, 3)):
        assert np.array_equal(out[:, t], keys[:, k])
    assert not np.array_equal(out[:, 3], keys[:, 1])
    # waypoint times == key times: the keyframes themselves
    assert np.array_equal(ref.interpolate(keys, kt, kt, "frame"), keys)
    # time-major: the same numbers with the axes swapped; no B axis: (K, n, w) -> (T, n, w)
    tm = ref.interpolate(np.ascontiguousarray(np.swapaxes(keys, 0, 1)), kt, wt, "frame", time_major=True)
    assert tm.shape == (len(wt), B, n, 7) and np.array_equal(np.swapaxes(tm, 0, 1), out)
    com = rng.normal(size=(K, 1, 3))
    oc_ = ref.interpolate(com, kt, wt, "com")
    u = (wt[3] - kt[1]) / (kt[2] - kt[1])
    assert oc_.shape == (len(wt), 1, 3) and np.array_equal(oc_[3], com[1] + u * (com[2] - com[1]))
    # K = 1: every waypoint is the one keyframe
    one = ref.interpolate(keys[:, :1], [2.0], [2.0, 2.0], "frame")
    assert np.array_equal(one[:, 0], keys[:, 0]) and np.array_equal(one[:, 1], keys[:, 0])


def test_public_refusals_need_no_gpu():
    import mink_amd
    from mink_amd import _native as nat

    m = oc.model("ur5e")
    B, K = 4, 3
    cfg = mink_amd.Configuration(m, np.tile(np.asarray(m.qpos0), (B, 1)))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    post = mink_amd.PostureTask(m, cost=1e-2)
    com = mink_amd.ComTask(cost=1.0)
    tasks = [task, post, com]
    poses = np.zeros((B, K, 7)); poses[..., 0] = 1.0
    kt, wt = [0.0, 1.0, 3.0], [0.0, 0.5, 3.0]
    call = lambda targets, **kw: mink_amd.solve_ik_trajectory(cfg, tasks, 1e-2, targets, **kw)
    # the keyframed arguments come together
    with pytest.raises(ValueError, match="need keyframe_times"):
        call({task: poses}, waypoint_times=wt)
    with pytest.raises(ValueError, match="need keyframe_times"):
        call({task: poses}, return_targets=True)
    with pytest.raises(ValueError, match="needs waypoint_times"):
        call({task: poses}, keyframe_times=kt)
    # the times
    for bad in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [3.0, 1.0, 0.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            call({task: poses}, keyframe_times=bad, waypoint_times=[1.0])
    with pytest.raises(ValueError, match="non-decreasing"):
        call({task: poses}, keyframe_times=kt, waypoint_times=[0.5, 0.25])
    for bad in ([-1e-9, 1.0], [0.0, 3.0 + 1e-9]):
        with pytest.raises(ValueError, match="no extrapolation"):
            call({task: poses}, keyframe_times=kt, waypoint_times=bad)
    with pytest.raises(ValueError, match="NaN"):
        call({task: poses}, keyframe_times=[0.0, float("nan"), 3.0], waypoint_times=wt)
    with pytest.raises(ValueError, match="NaN"):
        call({task: poses}, keyframe_times=kt, waypoint_times=[0.0, float("nan")])
    for bad_k, bad_w in (([], wt), (kt, []), (np.zeros((3, 1)), wt), (kt, np.zeros((2, 2)))):
        with pytest.raises(ValueError, match="must have shape"):
            call({task: poses}, keyframe_times=bad_k, waypoint_times=bad_w)
    # K of the sequences: between tasks, and against keyframe_times
    with pytest.raises(ValueError, match="disagree on the number of keyframes K"):
        call({task: poses, post: np.zeros((K + 1, m.nq))}, keyframe_times=kt, waypoint_times=wt)
    with pytest.raises(ValueError, match="keyframe_times has 2"):
        call({task: poses}, keyframe_times=[0.0, 3.0], waypoint_times=wt)
    for bad in (np.zeros((K, 6)), np.zeros((B + 1, K, 7)), np.zeros(7)):
        with pytest.raises(ValueError, match="must have shape"):
            call({task: bad}, keyframe_times=kt, waypoint_times=wt)
    with pytest.raises(ValueError, match="must have shape"):
        call({task: poses, com: np.zeros((B, K, 4))}, keyframe_times=kt, waypoint_times=wt)
    with pytest.raises(ValueError, match="n_steps"):
        call({task: poses}, keyframe_times=kt, waypoint_times=wt, n_steps=0)
    # the same checks behind NativeProblem.solve_keyframes
    k2, w2 = nat.check_keyframe_times([0, 1, 3], [0, 3])
    assert k2.dtype == np.float64 and w2.dtype == np.float64 and k2.tolist() == [0.0, 1.0, 3.0]
    assert nat.KeyframesOut._fields == ("trajectory", "frame_targets", "posture_targets", "com_targets")


def _header_struct():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "minkhip.h")).read()
    return hdr, hdr.split("typedef struct MkhKeyframeIO {")[1].split("} MkhKeyframeIO;")[0]


def test_entry_point_is_declared_bound_and_documented():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    assert "mkh_solve_keyframes" in nat.EXPORTED_SYMBOLS
    L = nat.lib()
    assert L.mkh_solve_keyframes is not None
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr, fields = _header_struct()
    decl = re.findall(r"^\s*(double|int32_t)\s*(\*?)\s*(\w+);", fields, flags=re.M)
    assert tuple(n for _, _, n in decl) == nat.KEYFRAME_IO_FIELDS        # same order as the ctypes mirror
    ctype = {("double", "*"): ctypes.c_void_p, ("int32_t", "*"): ctypes.c_void_p, ("double", ""): ctypes.c_double,
             ("int32_t", ""): ctypes.c_int32}
    mirror = nat.MkhKeyframeIO._fields_
    assert [(n, ctype[(t, p)]) for t, p, n in decl] == list(mirror)

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, ctype[(t, p)]) for t, p, n in decl]

    assert ctypes.sizeof(nat.MkhKeyframeIO) == ctypes.sizeof(FromHeader) == 9 * 8 + 8 + 3 * 4 + 4   # (4 bytes of tail padding)
    for n, _ in mirror:
        assert getattr(nat.MkhKeyframeIO, n).offset == getattr(FromHeader, n).offset, n
    # the outputs it shares with the trajectory call sit where that call has them
    for n in nat.TRAJECTORY_IO_FIELDS[:6]:
        assert getattr(nat.MkhKeyframeIO, n).offset == getattr(nat.MkhTrajectoryIO, n).offset, n
    proto = re.search(r"int32_t mkh_solve_keyframes\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(proto.split(",")) == len(L.mkh_solve_keyframes.argtypes) == 18
    for word in ("THE RULE", "no extrapolation, no silent clamping", "the largest index with key_times[k] <= tau", "SO3.log",
                 "SO3.exp", "never an FMA", "mj_differentiatePos", "mju_quatIntegrate", "posture_keyframed",
                 "frame_targets_out", "bit for bit"):
        assert word in hdr, word


def _call(L, io, p=None, B=2, K=3, T=3, kt=(0.0, 1.0, 3.0), wt=(0.0, 0.5, 3.0), n_steps=5, thr=(1e-3, 1e-3)):
    buf = np.zeros(64)
    kt = None if kt is None else np.asarray(kt, dtype=np.float64)
    wt = None if wt is None else np.asarray(wt, dtype=np.float64)
    return L.mkh_solve_keyframes(p, B, K, T, buf.ctypes.data, buf.ctypes.data, None, None,
                                 None if kt is None else kt.ctypes.data, None if wt is None else wt.ctypes.data, 1e-2, 1e-3,
                                 n_steps, thr[0], thr[1], ctypes.byref(io) if io is not None else None, 0, None)


def test_bad_arguments_fail_before_any_device_is_touched():
    """Everything the rule refuses is judged from the arguments alone, so these need neither a handle nor a GPU: a call
    that passes them all gets as far as "null problem"."""
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    outs = [np.zeros(64) for _ in range(6)]

    def io(**kw):
        x = nat.MkhKeyframeIO()
        x.q_traj, x.v_traj, x.status = (o.ctypes.data for o in outs[:3])
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    err = lambda: L.mkh_last_error()
    assert _call(L, io()) == -1 and b"null problem" in err()                       # MKH_E_INVALID, and nothing else wrong
    assert _call(L, io(), K=1, kt=(0.5,), wt=(0.5, 0.5, 0.5)) == -1 and b"null problem" in err()
    assert _call(L, io(), wt=(1.0, 1.0, 3.0)) == -1 and b"null problem" in err()   # a repeated time, a time on a keyframe
    # the trajectory call's own refusals, in its order
    assert _call(L, io(), B=0) == -1 and b"B must be >= 1" in err()
    assert _call(L, io(), T=0) == -1 and b"T must be >= 1" in err()
    assert _call(L, io(), n_steps=0) == -1 and b"n_steps must be >= 1" in err()
    assert _call(L, None) == -1 and b"required" in err()
    assert _call(L, io(status=None)) == -1 and b"required" in err()
    assert _call(L, io(iters=outs[3].ctypes.data), thr=(-1.0, -1.0)) == -1 and b"must be NULL with a fixed count" in err()
    assert _call(L, io(), thr=(1e-3, -1.0)) == -1 and b"thresholds" in err()
    assert _call(L, io(qvel=outs[4].ctypes.data, waypoint_dt=0.0)) == -1 and b"waypoint_dt > 0" in err()
    # the rule's refusals
    assert _call(L, io(), K=0) == -1 and b"K must be >= 1" in err()
    assert _call(L, io(), kt=None) == -1 and b"key_times and waypoint_times are required" in err()
    assert _call(L, io(), wt=None) == -1 and b"key_times and waypoint_times are required" in err()
    for bad in ((0.0, 0.0, 3.0), (0.0, 3.0, 1.0), (3.0, 1.0, 0.0)):
        assert _call(L, io(), kt=bad) == -1 and b"strictly increasing" in err()
    assert _call(L, io(), kt=(0.0, float("nan"), 3.0)) == -1 and b"key_times[1] is NaN" in err()
    assert _call(L, io(), wt=(0.0, float("nan"), 3.0)) == -1 and b"waypoint_times[1] is NaN" in err()
    assert _call(L, io(), wt=(0.5, 0.25, 3.0)) == -1 and b"non-decreasing" in err()
    assert _call(L, io(), wt=(-1e-9, 0.5, 3.0)) == -1 and b"outside the keyframes' range" in err()
    assert _call(L, io(), wt=(0.0, 0.5, 3.0 + 1e-9)) == -1 and b"no extrapolation" in err()
    assert _call(L, io(), K=1, kt=(0.5,), wt=(0.5, 0.5, 0.6)) == -1 and b"outside the keyframes' range" in err()
    # interpolated targets of a held group cannot be asked for
    assert _call(L, io(posture_targets_out=outs[5].ctypes.data)) == -1 and b"must be NULL for a target that is held" in err()
    assert _call(L, io(com_targets_out=outs[5].ctypes.data)) == -1 and b"must be NULL for a target that is held" in err()
    assert _call(L, io(posture_targets_out=outs[5].ctypes.data, posture_keyframed=1)) == -1 and b"null problem" in err()
    assert _call(L, io(frame_targets_out=outs[5].ctypes.data)) == -1 and b"null problem" in err()


def test_new_kernels_are_spill_free_without_scratch():
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    for k in ("keyframe_frames_kernel", "keyframe_posture_kernel", "keyframe_com_kernel"):
        e = table.get(k)
        assert e is not None, sorted(x for x in table if "keyframe" in x)
        assert e["vgpr_spills_with_callees"] == 0 and e["sgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0, (k, e)
        assert e["callees"] == {}, (k, e["callees"])                  # everything inlined: no call, no stack
    assert sorted(x for x in table if "keyframe" in x) == ["keyframe_com_kernel", "keyframe_frames_kernel", "keyframe_posture_kernel"]


@pytest.mark.parametrize("script", ["examples/batched_keyframes_ur5e.py", "tools/bench_keyframes.py"])
def test_example_and_bench_tool_load_no_undefined_names(script):
    """They only run end-to-end on a GPU (tests/test_entry_scripts.py does the same for the entry scripts)."""
    from test_entry_scripts import REPO, _undefined_globals
    assert _undefined_globals(os.path.join(REPO, script)) == []


def test_bench_tools_host_interpolation_is_the_rule():
    """Leg (c) of tools/bench_keyframes.py times a vectorised numpy slerp: it has to be the same path as the call's."""
    import importlib.util
    from test_entry_scripts import REPO
    spec = importlib.util.spec_from_file_location("bench_keyframes_mod", os.path.join(REPO, "tools", "bench_keyframes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(2)
    B, K, n = 3, 4, 2
    keys = np.concatenate([_unit(rng, B * K * n).reshape(B, K, n, 4), rng.normal(size=(B, K, n, 3))], axis=-1)
    kt, wt = np.linspace(0.0, 1.0, K), np.linspace(0.0, 1.0, 17)[1:]
    got, want = mod.numpy_interpolate(keys, kt, wt), ref.interpolate(keys, kt, wt, "frame")
    same_rotation = np.minimum(np.abs(got[..., :4] - want[..., :4]).max(axis=-1), np.abs(got[..., :4] + want[..., :4]).max(axis=-1))
    assert same_rotation.max() < 1e-12 and np.abs(got[..., 4:] - want[..., 4:]).max() < 1e-14
