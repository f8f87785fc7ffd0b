"""Multi-start trajectory IK without a GPU: the restated score, selection and layouts (tests/trajectory_multistart_ref.py)
behave on hand-made tables, the public call validates its arguments before it touches a device, the entry point is exported,
bound and mirrored field for field, it refuses what it can judge from its arguments alone, and the new kernels are compiled
spill-free."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle_configs as oc
import trajectory_multistart_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------ the restatement
def test_selection_rule_on_hand_made_tables():
    inf, nan = float("inf"), float("nan")
    # the count beats the length
    assert ref.select([2, 3, 1], [0.1, 9.0, 0.01]) == 1
    # the length beats the index
    assert ref.select([3, 3, 3], [2.0, 1.5, 1.0]) == 2
    assert ref.select([1, 3, 3, 2], [0.0, 2.0, 1.0, 0.5]) == 2
    # exact ties go to the lowest index
    assert ref.select([3, 3, 3], [1.0, 1.0, 1.0]) == 0
    assert ref.select([2, 3, 3, 3], [1.0, 2.0, 1.5, 1.5]) == 2
    # a NaN or infinite length ranks last among its count — and still beats a lower count
    assert ref.select([3, 3, 3], [nan, 5.0, 4.0]) == 2
    assert ref.select([3, 3], [inf, 1e300]) == 1
    assert ref.select([3, 3, 2], [nan, inf, 1.0]) == 0
    assert ref.select([3, 2], [nan, 1.0]) == 0
    # nobody tracked anything: candidate 0, whatever the lengths say
    assert ref.select([0, 0, 0], [5.0, 1.0, 0.5]) == 0
    # one candidate
    assert ref.select([0], [1.0]) == 0 and ref.select([4], [nan]) == 0


def test_score_counts_tracked_waypoints_and_sums_the_path_from_the_callers_q():
    m = oc.model("ur5e")
    rng = np.random.default_rng(0)
    T = 4
    q0 = rng.normal(size=m.nq)
    path = q0 + np.cumsum(rng.normal(scale=0.1, size=(T, m.nq)), axis=0)
    ones = np.ones(T, dtype=np.int32)
    n, length = ref.score(m, q0, path, ones, np.zeros(T, dtype=np.int32))
    steps = np.diff(np.concatenate([q0[None], path]), axis=0)
    assert n == T and np.isclose(length, float((steps ** 2).sum()), rtol=1e-14)
    w = rng.uniform(0.5, 2.0, size=m.nv)
    assert np.isclose(ref.score(m, q0, path, ones, 0 * ones, w)[1], float((w * steps ** 2).sum()), rtol=1e-14)
    # the first term is measured from q0, not from where a seed started: moving q0 changes the length
    assert ref.score(m, q0 + 1.0, path, ones, 0 * ones)[1] > length
    # an OUTSIDE_LIMITS bit is no failure; any other bit is, converged or not; a loop that did not converge is not tracked
    assert ref.score(m, q0, path, ones, np.array([0, 1, 0, 1]))[0] == T
    for bit in (2, 4, 8, 16, 32):
        assert ref.score(m, q0, path, ones, np.array([0, bit, 0, bit | 1]))[0] == T - 2
    assert ref.score(m, q0, path, np.array([1, 0, 1, 0]), 0 * ones)[0] == 2
    assert ref.score(m, q0, path, 0 * ones, 0 * ones) == (0, length)       # the length does not depend on what was tracked


def test_restated_layouts_and_choice():
    m = oc.model("ur5e")
    B, S, T = 3, 4, 5
    rng = np.random.default_rng(1)
    q0 = rng.normal(size=(B, m.nq))
    q_all = rng.normal(size=(T, B * S, m.nq))
    by = ref.by_instance(q_all, B, S)
    assert by.shape == (B, S, T, m.nq) and by.flags.c_contiguous
    assert np.array_equal(by[2, 1, 3], q_all[3, 2 * S + 1])
    cv = (rng.uniform(size=(T, B * S)) < 0.7).astype(np.int32)
    st = rng.choice([0, 0, 0, 1, 2], size=(T, B * S)).astype(np.int32)
    pick, n_tr, n_comp, length, counts, lengths = ref.choose(m, q0, q_all, cv, st, S)
    assert pick.shape == n_tr.shape == n_comp.shape == length.shape == (B,) and counts.shape == lengths.shape == (B, S)
    for b in range(B):
        for s in range(S):
            assert (counts[b, s], lengths[b, s]) == ref.score(m, q0[b], by[b, s], ref.by_instance(cv, B, S)[b, s],
                                                              ref.by_instance(st, B, S)[b, s])
        assert pick[b] == ref.select(counts[b], lengths[b]) and n_tr[b] == counts[b, pick[b]] == counts[b].max()
        assert n_comp[b] == (counts[b] == T).sum() and length[b] == lengths[b, pick[b]]
    bm, tm = ref.chosen(q_all, pick, S), ref.chosen(q_all, pick, S, time_major=True)
    assert bm.shape == (B, T, m.nq) and tm.shape == (T, B, m.nq) and np.array_equal(np.swapaxes(tm, 0, 1), bm)
    assert np.array_equal(bm[1, 2], q_all[2, 1 * S + pick[1]])
    assert np.array_equal(ref.chosen(cv, pick, S)[2], cv[:, 2 * S + pick[2]])


# ------------------------------------------------------------------ the public call
def test_argument_validation_needs_no_gpu():
    import mink_amd

    m = oc.model("ur5e")
    B, T, S = 4, 3, 5
    cfg = mink_amd.Configuration(m, np.tile(np.asarray(m.qpos0), (B, 1)))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    post = mink_amd.PostureTask(m, cost=1e-2)
    tasks = [task, post]
    poses = np.zeros((B, T, 7)); poses[..., 0] = 1.0
    base = dict(n_seeds=S, n_steps=10, pos_threshold=1e-4, ori_threshold=1e-4)
    call = lambda targets={task: poses}, **kw: mink_amd.solve_ik_trajectory_multistart(cfg, tasks, 1.0, targets, **{**base, **kw})
    with pytest.raises(ValueError, match="n_seeds"):
        call(n_seeds=0)
    with pytest.raises(ValueError, match="n_steps"):
        call(n_steps=0)
    with pytest.raises(ValueError, match="max_instances"):
        call(max_instances=0)
    for wdt in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="waypoint_dt"):
            call(waypoint_dt=wdt)
    for thr in (dict(pos_threshold=-1e-3), dict(ori_threshold=-1.0), dict(pos_threshold=-1.0, ori_threshold=-1.0),
                dict(pos_threshold=None), dict(ori_threshold=float("nan"))):
        with pytest.raises(ValueError, match="threshold mode only"):
            call(**thr)
    for bad in (np.zeros((T, 6)), np.zeros((B + 1, T, 7)), np.zeros((B, 0, 7))):
        with pytest.raises(ValueError, match="must have shape"):
            call({task: bad})
    with pytest.raises(ValueError, match="disagree on the number of waypoints"):
        call({task: poses, post: np.zeros((T + 1, m.nq))})
    with pytest.raises(ValueError, match="targets is empty"):
        call({})
    for bad in (np.zeros((3, m.nq)), np.zeros((B, S, m.nq + 1)), np.zeros((2, S, m.nq)), np.zeros(m.nq)):
        with pytest.raises(ValueError, match="seeds must have shape"):
            call(seeds=bad)
    with pytest.raises(ValueError, match="weights must have shape"):
        call(weights=np.ones(m.nv + 1))
    for bad in (-np.ones(m.nv), np.r_[np.ones(m.nv - 1), np.nan]):
        with pytest.raises(ValueError, match="weights must be >= 0"):
            call(weights=bad)
    assert "solve_ik_trajectory_multistart" in mink_amd.__all__ and "TrajectoryMultistartResult" in mink_amd.__all__
    assert mink_amd.TrajectoryMultistartResult._fields == (
        "q", "v", "status", "iters", "converged", "seed_index", "n_tracked", "n_complete", "path_length", "qvel", "q_all", "v_all",
        "status_all", "iters_all", "converged_all", "seeds")
    # the siblings keep their shape: nothing was added to them
    assert mink_amd.TrajectoryResult._fields == ("q", "v", "status", "iters", "converged", "qvel")
    import inspect
    assert "n_seeds" not in inspect.signature(mink_amd.solve_ik_trajectory).parameters


# ------------------------------------------------------------------ the C ABI
def _header_struct():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "minkhip.h")).read()
    return hdr, hdr.split("typedef struct MkhTrajectoryMultistartIO {")[1].split("} MkhTrajectoryMultistartIO;")[0]


def test_entry_point_is_declared_bound_and_documented():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    assert "mkh_solve_trajectory_multistart" in nat.EXPORTED_SYMBOLS
    L = nat.lib()
    assert L.mkh_solve_trajectory_multistart is not None and L.mkh_solve_trajectory_multistart.restype is ctypes.c_int32
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr, fields = _header_struct()
    assert "int32_t mkh_solve_trajectory_multistart(MkhProblem *problem, int32_t B, int32_t T, int32_t n_seeds," in hdr
    decl = re.findall(r"^\s*(?:const\s+)?(double|int32_t)\s*(\*?)\s*(\w+);", fields, flags=re.M)
    assert tuple(n for _, _, n in decl) == nat.TRAJECTORY_MULTISTART_IO_FIELDS      # same order as the ctypes mirror
    ctype = {("double", "*"): ctypes.c_void_p, ("int32_t", "*"): ctypes.c_void_p, ("double", ""): ctypes.c_double,
             ("int32_t", ""): ctypes.c_int32}
    mirror = nat.MkhTrajectoryMultistartIO._fields_
    assert [(n, ctype[(t, p)]) for t, p, n in decl] == list(mirror)

    class FromHeader(ctypes.Structure):
        _fields_ = [(n, ctype[(t, p)]) for t, p, n in decl]

    assert ctypes.sizeof(nat.MkhTrajectoryMultistartIO) == ctypes.sizeof(FromHeader) == 18 * 8 + 8 + 3 * 4 + 4   # (4 bytes of tail padding)
    for n, _ in mirror:
        assert getattr(nat.MkhTrajectoryMultistartIO, n).offset == getattr(FromHeader, n).offset, n
    for word in ("THE RULE", "CANDIDATE 0 OF EVERY INSTANCE STARTS AT THE CALLER'S OWN q[b]", "q_{-1} IS THE CALLER'S q[b] FOR EVERY CANDIDATE",
                 "T·B·S·((nq + nv)·8 + 12)", "n_seeds = 1 IS mkh_solve_trajectory", "ALWAYS time-major", "lowest s",
                 "candidate 0 wins", "~MKH_ST_OUTSIDE_LIMITS"):
        assert word in hdr, word


def test_bad_arguments_fail_before_any_device_is_touched():
    """What can be judged from the arguments alone is judged first, so these need neither a handle nor a GPU."""
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    outs = [np.zeros(64) for _ in range(10)]
    required = ("q_traj", "v_traj", "status", "iters", "converged", "seed_index", "n_tracked", "n_complete", "path_length")

    def io(**kw):
        x = nat.MkhTrajectoryMultistartIO()
        for n, o in zip(required, outs):
            setattr(x, n, o.ctypes.data)
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    def call(io_, B=2, T=3, S=4, n_steps=5, thr=(1e-3, 1e-3), t0=0):
        buf = np.zeros(64)
        return L.mkh_solve_trajectory_multistart(None, B, T, S, buf.ctypes.data, buf.ctypes.data, None, None, 1.0, 1e-3, n_steps,
                                                 thr[0], thr[1], 0, t0, ctypes.byref(io_) if io_ is not None else None, 0, None)

    err = L.mkh_last_error
    assert call(io()) == -1 and b"null problem" in err()                 # MKH_E_INVALID: everything else was in order
    for S in (0, -3):
        assert call(io(), S=S) == -1 and b"n_seeds must be >= 1" in err()
    assert call(io(), B=0) == -1 and b"B must be >= 1" in err()
    assert call(io(), T=0) == -1 and b"T must be >= 1" in err()
    assert call(io(), n_steps=0) == -1 and b"n_steps must be >= 1" in err()
    assert call(io(), t0=-1) == -1 and b"target_index0 must be >= 0" in err()
    # fixed-count mode: nothing to score
    assert call(io(), thr=(-1.0, -1.0)) == -1 and b"threshold mode only" in err() and b"mkh_solve_trajectory_multistart" in err()
    # mixed signs and NaN: the trajectory call's own refusal
    for thr in ((1e-3, -1.0), (-1.0, 1e-3), (float("nan"), 1e-3)):
        assert call(io(), thr=thr) == -1 and b"thresholds must both be" in err()
    # every required output
    assert call(None) == -1 and b"required" in err()
    for missing in required:
        assert call(io(**{missing: None})) == -1 and b"required" in err(), missing
    # qvel needs its time step
    for wdt in (0.0, -0.1, float("nan")):
        assert call(io(qvel=outs[9].ctypes.data, waypoint_dt=wdt)) == -1 and b"waypoint_dt > 0" in err()
    assert call(io(qvel=outs[9].ctypes.data, waypoint_dt=0.02)) == -1 and b"null problem" in err()
    # the siblings still take a fixed count
    tio = nat.MkhTrajectoryIO()
    tio.q_traj, tio.v_traj, tio.status = (o.ctypes.data for o in outs[:3])
    buf = np.zeros(64)
    assert L.mkh_solve_trajectory(None, 2, 3, buf.ctypes.data, buf.ctypes.data, None, None, 1.0, 1e-3, 5, -1.0, -1.0, ctypes.byref(tio),
                                  0, None) == -1 and b"null problem" in err()


def test_new_kernels_are_spill_free_without_scratch():
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    for k in ("tms_score_select_kernel", "tms_gather_kernel", "tms_gather_i32_kernel"):
        e = table.get(k)
        assert e is not None, sorted(x for x in table if "tms" in x)
        assert e["vgpr_spills_with_callees"] == 0 and e["sgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0, (k, e)
        assert e["callees"] == {}, (k, e["callees"])                  # everything inlined: no call, no stack
    with open(os.path.join(GOLDEN, "spill_budget.json")) as fh:
        assert not any("tms_" in k for k in json.load(fh))            # no allowance: tests/test_abi.py holds them to 0 as well


# ------------------------------------------------------------------ the example and the bench tool
@pytest.mark.parametrize("script", ["examples/batched_global_trajectory_ur5e.py", "tools/bench_trajectory_multistart.py"])
def test_example_and_bench_tool_load_no_undefined_names(script):
    """They only run end-to-end on a GPU (tests/test_entry_scripts.py does the same for the entry scripts)."""
    from test_entry_scripts import REPO, _undefined_globals
    assert _undefined_globals(os.path.join(REPO, script)) == []


def test_bench_tools_host_composition_is_the_rule():
    """Leg (c) of tools/bench_trajectory_multistart.py times a numpy score / selection / gather: it has to choose as the call does."""
    import importlib.util
    import mink_amd
    from test_entry_scripts import REPO
    spec = importlib.util.spec_from_file_location("bench_tms_mod", os.path.join(REPO, "tools", "bench_trajectory_multistart.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    m = mink_amd.load_mjcf(os.path.join(GOLDEN, "ballslide.xml"))
    B, S, T = 5, 4, 3
    rng = np.random.default_rng(2)
    q0 = ref.draw_seeds(m, np.tile(np.asarray(m.qpos0, dtype=np.float64), (B, 1)), 2, rng_seed=1)[:, 1]
    q = ref.draw_seeds(m, np.repeat(q0, S * T, axis=0), 2, rng_seed=2)[:, 1].reshape(B * S, T, m.nq)
    cv = rng.uniform(size=(B * S, T)) < 0.7
    st = rng.choice([0, 0, 1, 2], size=(B * S, T)).astype(np.int32)
    cv[:S], cv[S:2 * S] = False, True; st[S:2 * S] = 0                     # nobody tracks anything / the lengths alone decide
    pick, rows = mod.numpy_score_select(m, q0, q, cv, st, S)
    tm = lambda x: np.ascontiguousarray(np.swapaxes(x, 0, 1))
    want = ref.choose(m, q0, tm(q), tm(cv), tm(st), S)
    assert np.array_equal(pick, want[0]) and pick[0] == 0
    assert np.array_equal(rows, ref.chosen(tm(q), pick, S))
    seeds = mod.numpy_seeds(m, q0, S, rng)
    assert seeds.shape == (B, S, m.nq) and np.array_equal(seeds[:, 0], q0)
