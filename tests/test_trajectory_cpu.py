"""Trajectory IK without a GPU: the restated layouts and waypoint velocity (tests/trajectory_ref.py) agree with the oracle's
mj_differentiatePos, the public call validates its arguments before it touches a device, the entry point is exported, bound
and mirrored field for field, and the new kernels are compiled spill-free."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle_configs as oc
import trajectory_ref as ref
from oracle import mjmath

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model(name):
    import mink_amd
    if name == "ballslide":
        return mink_amd.load_mjcf(os.path.join(GOLDEN, "ballslide.xml"))
    if name == "h1":
        from mink_amd import workloads
        return workloads.load_robot("h1")
    return oc.model(name)


def _random_trajectory(m, B, T, rng):
    """Start (B, nq) and configurations (B, T, nq): qpos0 plus noise, quaternions random and normalised."""
    q = np.tile(np.asarray(m.qpos0, dtype=np.float64), (B * (T + 1), 1))
    q += rng.normal(scale=0.3, size=q.shape)
    for j in range(m.njnt):
        jt, a = int(m.jnt_type[j]), int(m.jnt_qposadr[j])
        if jt in (ref.JNT_FREE, ref.JNT_BALL):
            a += 3 if jt == ref.JNT_FREE else 0
            quat = rng.normal(size=(len(q), 4))
            q[:, a:a + 4] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    q = q.reshape(B, T + 1, m.nq)
    return np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1:])


@pytest.mark.parametrize("name", ["ur5e", "h1", "ballslide"])
def test_restated_qvel_is_mj_differentiatePos(name):
    m = _model(name)
    B, T, dt = 5, 4, 0.04
    q0, traj = _random_trajectory(m, B, T, np.random.default_rng(6))
    got = ref.qvel(m, q0, traj, dt)
    assert got.shape == (B, T, m.nv)
    quat = ref.quaternion_dofs(m)
    kinds = {int(t) for t in m.jnt_type}
    assert {"ur5e": {3}, "h1": {0, 3}, "ballslide": {1, 2, 3}}[name] <= kinds
    assert quat.any() == (name != "ur5e")
    worst = 0.0
    for b in range(B):
        for t in range(T):
            want = np.zeros(m.nv)
            mjmath.mj_differentiatePos(m, want, dt, q0[b] if t == 0 else traj[b, t - 1], traj[b, t])
            assert np.array_equal(got[b, t, ~quat], want[~quat]), (b, t)         # a difference, then a quotient: exact
            worst = max(worst, float(np.abs(got[b, t, quat] - want[quat]).max(initial=0.0)))
            assert np.allclose(got[b, t, quat], want[quat], rtol=0, atol=1e-12 / dt)
    print(f"{name}: quaternion dofs, max |restatement - oracle| = {worst:.2e}")
    # the time-major form is the same numbers with the axes swapped
    tm = ref.qvel(m, q0, ref.to_time_major(traj), dt, time_major=True)
    assert tm.shape == (T, B, m.nv) and np.array_equal(ref.to_batch_major(tm), got)
    # a quaternion and its negative are the same rotation; a waypoint that does not move has zero velocity
    still = ref.qvel(m, q0, np.repeat(q0[:, None, :], 2, axis=1), dt)
    assert np.abs(still).max() < 1e-13 / dt


def test_restated_layouts():
    B, T, n, w = 3, 4, 2, 5
    x = np.arange(B * T * n * w, dtype=np.float64).reshape(B, T, n, w)
    tm = ref.to_time_major(x)
    assert tm.shape == (T, B, n, w) and tm.flags.c_contiguous and np.array_equal(tm[2, 1], x[1, 2])
    assert np.array_equal(ref.to_batch_major(tm), x)
    for t in range(T):
        assert np.array_equal(ref.waypoint_target(x, t, n, w, B), x[:, t])
        assert np.array_equal(ref.waypoint_target(tm, t, n, w, B, time_major=True), x[:, t])
        assert np.array_equal(ref.waypoint_target(x[0], t, n, w, B), x[0, t])          # (T, n, w): T leads, both layouts
        assert np.array_equal(ref.waypoint_target(x[:, 0], t, n, w, B), x[:, 0])       # (B, n, w): held
        assert np.array_equal(ref.waypoint_target(x[0, 0], t, n, w, B), x[0, 0])       # (n, w): held
    assert ref.waypoint_target(None, 0, n, w, B) is None


def test_argument_validation_needs_no_gpu():
    import mink_amd

    m = oc.model("ur5e")
    B, T = 4, 3
    cfg = mink_amd.Configuration(m, np.tile(np.asarray(m.qpos0), (B, 1)))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    post = mink_amd.PostureTask(m, cost=1e-2)
    com = mink_amd.ComTask(cost=1.0)
    tasks = [task, post, com]
    poses = np.zeros((B, T, 7)); poses[..., 0] = 1.0
    call = lambda targets, **kw: mink_amd.solve_ik_trajectory(cfg, tasks, 1e-2, targets, **kw)
    for bad in (np.zeros((T, 6)), np.zeros((B + 1, T, 7)), np.zeros((B, T, 8)), np.zeros(7), np.zeros((B, 0, 7)),
                np.zeros((2, B, T, 7))):
        with pytest.raises(ValueError, match="must have shape"):
            call({task: bad})
    with pytest.raises(ValueError, match="must have shape"):
        call({post: np.zeros((T, m.nq + 1))})
    with pytest.raises(ValueError, match="must have shape"):
        call({com: np.zeros((B, T, 4))})
    with pytest.raises(ValueError, match="disagree on the number of waypoints"):
        call({task: poses, post: np.zeros((T + 1, m.nq))})
    with pytest.raises(ValueError, match="disagree on the number of waypoints"):
        call({task: poses[0], com: np.zeros((B, T + 2, 3))})
    for empty in ({}, None, []):
        with pytest.raises(ValueError, match="targets is empty"):
            call(empty)
    with pytest.raises(ValueError, match="not in `tasks`"):
        call({mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0): poses})
    with pytest.raises(ValueError, match="n_steps"):
        call({task: poses}, n_steps=0)
    with pytest.raises(ValueError, match="max_instances"):
        call({task: poses}, max_instances=0)
    for dt in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="waypoint_dt"):
            call({task: poses}, waypoint_dt=dt)
    with pytest.raises(ValueError, match="thresholds"):
        call({task: poses}, pos_threshold=-1e-3)
    assert "solve_ik_trajectory" in mink_amd.__all__ and "TrajectoryResult" in mink_amd.__all__
    assert mink_amd.TrajectoryResult._fields == ("q", "v", "status", "iters", "converged", "qvel")


def _header_struct():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "minkhip.h")).read()
    return hdr, hdr.split("typedef struct MkhTrajectoryIO {")[1].split("} MkhTrajectoryIO;")[0]


def test_entry_point_is_declared_bound_and_documented():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    assert "mkh_solve_trajectory" in nat.EXPORTED_SYMBOLS
    L = nat.lib()
    assert L.mkh_solve_trajectory is not None
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr, fields = _header_struct()
    decl = re.findall(r"^\s*(double|int32_t)\s*(\*?)\s*(\w+);", fields, flags=re.M)
    assert tuple(n for _, _, n in decl) == nat.TRAJECTORY_IO_FIELDS      # same order as the ctypes mirror
    ctype = {("double", "*"): ctypes.c_void_p, ("int32_t", "*"): ctypes.c_void_p, ("double", ""): ctypes.c_double,
             ("int32_t", ""): ctypes.c_int32}
    mirror = nat.MkhTrajectoryIO._fields_
    assert [(n, ctype[(t, p)]) for t, p, n in decl] == list(mirror)

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, ctype[(t, p)]) for t, p, n in decl]

    assert ctypes.sizeof(nat.MkhTrajectoryIO) == ctypes.sizeof(FromHeader) == 6 * 8 + 8 + 3 * 4 + 4   # (4 bytes of tail padding)
    for n, _ in mirror:
        assert getattr(nat.MkhTrajectoryIO, n).offset == getattr(FromHeader, n).offset, n
    for word in ("A FAILING WAYPOINT DOES NOT STOP THE TRAJECTORY", "mj_differentiatePos", "time_major", "posture_per_waypoint",
                 "MKH_FLAG_WARM_START", "max_iters = n_steps"):
        assert word in hdr, word


def _call(L, nat, io, p=None, B=2, T=3, n_steps=5, thr=(1e-3, 1e-3), q=None):
    buf = np.zeros(64)
    return L.mkh_solve_trajectory(p, B, T, buf.ctypes.data if q is None else q, buf.ctypes.data, None, None, 1e-2, 1e-3, n_steps,
                                  thr[0], thr[1], ctypes.byref(io) if io is not None else None, 0, None)


def test_bad_arguments_fail_before_any_device_is_touched():
    """What can be judged from the arguments alone is judged first, so these need neither a handle nor a GPU."""
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    outs = [np.zeros(64) for _ in range(6)]

    def io(**kw):
        x = nat.MkhTrajectoryIO()
        x.q_traj, x.v_traj, x.status = (o.ctypes.data for o in outs[:3])
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    assert _call(L, nat, io()) == -1 and b"null problem" in L.mkh_last_error()      # MKH_E_INVALID
    assert _call(L, nat, io(), T=0) == -1 and b"T must be >= 1" in L.mkh_last_error()
    assert _call(L, nat, io(), B=0) == -1 and b"B must be >= 1" in L.mkh_last_error()
    assert _call(L, nat, io(), n_steps=0) == -1 and b"n_steps must be >= 1" in L.mkh_last_error()
    assert _call(L, nat, None) == -1 and b"required" in L.mkh_last_error()
    for missing in ("q_traj", "v_traj", "status"):
        assert _call(L, nat, io(**{missing: None})) == -1 and b"required" in L.mkh_last_error()
    # iters / converged belong to threshold mode
    for name in ("iters", "converged"):
        assert _call(L, nat, io(**{name: outs[3].ctypes.data}), thr=(-1.0, -1.0)) == -1
        assert b"must be NULL with a fixed count" in L.mkh_last_error()
        assert _call(L, nat, io(**{name: outs[3].ctypes.data})) == -1 and b"null problem" in L.mkh_last_error()
    assert _call(L, nat, io(), thr=(-1.0, -1.0)) == -1 and b"null problem" in L.mkh_last_error()
    assert _call(L, nat, io(), thr=(1e-3, -1.0)) == -1 and b"thresholds" in L.mkh_last_error()
    assert _call(L, nat, io(), thr=(float("nan"), 1e-3)) == -1 and b"thresholds" in L.mkh_last_error()
    # qvel needs its time step
    for wdt in (0.0, -0.1, float("nan")):
        assert _call(L, nat, io(qvel=outs[4].ctypes.data, waypoint_dt=wdt)) == -1 and b"waypoint_dt > 0" in L.mkh_last_error()
    assert _call(L, nat, io(qvel=outs[4].ctypes.data, waypoint_dt=0.02)) == -1 and b"null problem" in L.mkh_last_error()


def test_new_kernels_are_spill_free_without_scratch():
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    for k in ("trajectory_gather_kernel", "trajectory_scatter_kernel", "trajectory_scatter_i32_kernel", "trajectory_qvel_kernel"):
        e = table.get(k)
        assert e is not None, sorted(x for x in table if "trajectory" in x)
        assert e["vgpr_spills_with_callees"] == 0 and e["sgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0, (k, e)
        assert e["callees"] == {}, (k, e["callees"])                  # everything inlined: no call, no stack
