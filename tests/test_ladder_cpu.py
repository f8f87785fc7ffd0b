"""Ladder-graph trajectory IK without a GPU: the restated recurrence (tests/ladder_ref.py) against enumeration of every path,
its edge cost against multi-start's distance, the public calls' argument checks before any device is touched, the entry
points exported, bound and mirrored field for field, and the new kernels compiled without spills, scratch or callee frames."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import ladder_ref as ref
import multistart_ref as msref
import oracle_configs as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def _dyadic_rungs(rng, m, T, S, special=True):
    """q0 (nq,), q_nodes (T, S, nq), tracked (T, S) on multiples of 1/8 in [-2, 2]: every difference, square and sum of the
    edge costs is exact in float64.  With `special`: a duplicated node, a NaN node, an inf node, a rung nobody tracked."""
    q0 = rng.integers(-16, 17, size=m.nq) / 8.0
    q = rng.integers(-16, 17, size=(T, S, m.nq)) / 8.0
    trk = rng.uniform(size=(T, S)) < 0.7
    if special:
        if S >= 2:
            q[T // 2, S - 1] = q[T // 2, 0]                     # an exact tie
            trk[T // 2, S - 1] = trk[T // 2, 0]
        if S >= 3 and T >= 2:
            q[1, 1, 0] = np.nan
            q[0, 2, 1] = np.inf
        if T >= 4:
            trk[2] = False
    return q0, q, trk


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 2, 4])
def test_recurrence_is_the_best_of_all_paths(S, T):
    m = oc.model("ur5e")
    rng = np.random.default_rng(100 * S + T)
    seen_break = seen_lost = False
    for trial in range(6):
        q0, q, trk = _dyadic_rungs(rng, m, T, S, special=trial % 2 == 0)
        start, edges = ref.costs(m, q0, q)
        finite = edges[1:][np.isfinite(edges[1:])]
        gates = [np.inf, 0.0] + ([float(np.median(finite))] if finite.size else [])
        for gate in gates:
            path, key, brk = ref.search(start, edges, ~trk, gate)
            path_b, key_b, brk_b = ref.brute_force(start, edges, ~trk, gate)
            np.testing.assert_array_equal(path, path_b, err_msg=f"S={S} T={T} trial {trial} gate {gate}")
            assert key == key_b                                  # exact sums: the same additions in another order agree
            np.testing.assert_array_equal(brk, brk_b)
            assert key == ref.path_key(start, edges, ~trk, path, gate)
            assert brk[0] == 0 and brk.sum() == key[1]
            path_f, key_f, brk_f = ref.search_fast(start, edges, ~trk, gate)
            np.testing.assert_array_equal(path_f, path); np.testing.assert_array_equal(brk_f, brk)
            assert key_f == key
            seen_break, seen_lost = seen_break or key[1] > 0, seen_lost or key[0] > 0
    if T >= 4:                                                   # (the rung nobody tracked: every path loses it)
        assert seen_lost
    if T >= 2:
        assert seen_break


def test_hand_made_ladders():
    inf = float("inf")
    lost = np.zeros((2, 2), dtype=int)
    # length decides; the start edge counts
    start, edges = np.array([1.0, 0.0]), np.zeros((2, 2, 2))
    edges[1] = [[1.0, 4.0], [3.0, 0.5]]                           # edges[t][s'][s]
    path, key, brk = ref.search(start, edges, lost)
    assert path.tolist() == [1, 1] and key == (0, 0, 0.5) and brk.tolist() == [0, 0]
    # a break outranks any length: the gate 0.75 makes every edge but 1 -> 1 a break
    edges[1] = [[1.0, 4.0], [3.0, 0.5]]
    start = np.array([0.0, 100.0])
    assert ref.search(start, edges, lost, 0.75)[1] == (0, 0, 100.5)
    assert ref.search(start, edges, lost)[1] == (0, 0, 1.0)
    # the start edge is never a break, whatever it costs
    assert ref.search(np.array([50.0, 60.0]), edges, lost, 0.75)[1] == (0, 0, 60.5)
    # an untracked node outranks any break
    lost2 = np.array([[0, 0], [1, 0]])
    path, key, brk = ref.search(np.array([0.0, 9.0]), np.array([np.zeros((2, 2)), [[0.0, 0.0], [5.0, 5.0]]]), lost2, 1.0)
    assert path.tolist() == [0, 1] and key == (0, 1, 5.0) and brk.tolist() == [0, 1]
    # exact ties: the lowest end node, then the lowest predecessor
    path, key, _ = ref.search(np.array([1.0, 1.0, 1.0]), np.ones((3, 3, 3)), np.zeros((3, 3), dtype=int))
    assert path.tolist() == [0, 0, 0] and key == (0, 0, 3.0)
    # an infinite edge is taken only when there is nothing else, and the length stays inf (no NaN)
    e = np.zeros((2, 1, 1)); e[1] = inf
    assert ref.search(np.array([2.0]), e, np.zeros((2, 1), dtype=int))[1] == (0, 0, inf)
    assert ref.search(np.array([2.0]), e, np.zeros((2, 1), dtype=int), 10.0)[1] == (0, 1, inf)
    # one waypoint, one node
    path, key, brk = ref.search(np.array([0.25]), np.zeros((1, 1, 1)), np.array([[1]]))
    assert path.tolist() == [0] and key == (1, 0, 0.25) and brk.tolist() == [0]


def test_edge_cost_is_multistarts_distance():
    import mink_amd
    ball = mink_amd.load_mjcf(os.path.join(GOLDEN, "ballslide.xml"))
    for m, tol in ((oc.model("ur5e"), 0.0), (ball, 1e-15), (oc.model("g1"), 1e-15)):
        rng = np.random.default_rng(5)
        base = np.tile(np.asarray(m.qpos0, dtype=np.float64), (7, 1))
        a = msref.draw_seeds(m, base, 2, rng_seed=1)[:, 1]
        b = msref.draw_seeds(m, base, 2, rng_seed=2)[:, 1]
        if m.nq != m.nv and int(m.jnt_type[0]) == ref.JNT_FREE:          # a floating base: move it, turn it
            a[:, :3] += rng.normal(size=(7, 3)); qq = rng.normal(size=(7, 4)); a[:, 3:7] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
        for w in (None, rng.uniform(0.1, 3.0, size=m.nv)):
            c = ref.edge_costs(m, a, b, w)
            want = np.array([[msref.distance(m, a[i], b[j], w) for j in range(7)] for i in range(7)])
            # (the same products; numpy's np.sum adds them pairwise, the rule joint by joint: the last bits may differ)
            np.testing.assert_allclose(c, want, rtol=max(tol, 1e-15) * 8, atol=0)
            # (a node against itself: hinges cancel exactly; conj(q)·q leaves a few ulp of rotation, squared)
            assert (np.diag(ref.edge_costs(m, a, a, w)) <= (0.0 if m.nq == m.nv else 1e-29)).all()
    # hinge values on a dyadic grid: exact, whatever the order
    m = oc.model("ur5e")
    a = np.random.default_rng(6).integers(-16, 17, size=(5, m.nq)) / 8.0
    want = np.array([[msref.distance(m, a[i], a[j]) for j in range(5)] for i in range(5)])
    np.testing.assert_array_equal(ref.edge_costs(m, a, a), want)
    # NaN, inf and overflow: +inf, never NaN; negative weights do not reach the rule (refused by the calls)
    bad = a.copy(); bad[0, 0] = np.nan; bad[1, 1] = np.inf; bad[2, 2] = 1e200
    c = ref.edge_costs(m, bad, a)
    assert np.isinf(c[:3]).all() and np.isfinite(c[3:]).all() and not np.isnan(c).any()


def test_select_layout_and_outputs():
    m = oc.model("ur5e")
    rng = np.random.default_rng(3)
    B, T, S = 2, 3, 4
    q = rng.integers(-8, 9, size=(B, m.nq)) / 4.0
    nodes = rng.integers(-8, 9, size=(B, T, S, m.nq)) / 4.0
    trk = rng.uniform(size=(B, T, S)) < 0.6
    out = ref.select(m, q, nodes, trk, None, 6.0)
    assert out["node_index"].shape == (B, T) and out["q_path"].shape == (B, T, m.nq) and out["edge_break"].shape == (B, T)
    for b in range(B):
        start, edges = ref.costs(m, q[b], nodes[b])
        lost, brk, length = ref.path_key(start, edges, ~trk[b], out["node_index"][b], 6.0)
        assert (out["n_tracked"][b], out["n_breaks"][b], out["path_length"][b]) == (T - lost, brk, length)
        np.testing.assert_array_equal(out["q_path"][b], nodes[b, np.arange(T), out["node_index"][b]])
        assert out["edge_break"][b, 0] == 0 and out["edge_break"][b].sum() == brk
    every = ref.select(m, q, nodes, None, None)
    assert (every["n_tracked"] == T).all() and (every["n_breaks"] == 0).all()


# ------------------------------------------------------------------ the public calls
def test_argument_validation_needs_no_gpu():
    import mink_amd

    m = oc.model("ur5e")
    B, T, S = 4, 3, 5
    cfg = mink_amd.Configuration(m, np.tile(np.asarray(m.qpos0), (B, 1)))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    post = mink_amd.PostureTask(m, cost=1e-2)
    tasks = [task, post]
    poses = np.zeros((B, T, 7)); poses[..., 0] = 1.0
    base = dict(n_seeds=S, max_iters=10, pos_threshold=1e-4, ori_threshold=1e-4)
    call = lambda targets={task: poses}, **kw: mink_amd.solve_ik_trajectory_ladder(cfg, tasks, 1.0, targets, **{**base, **kw})
    for bad in (0, -2):
        with pytest.raises(ValueError, match="n_seeds"):
            call(n_seeds=bad)
    with pytest.raises(ValueError, match="at most 256"):
        call(n_seeds=257)
    with pytest.raises(ValueError, match="at most 65535"):
        call({task: np.broadcast_to(poses[:1, :1], (B, 65536, 7))})
    with pytest.raises(ValueError, match="max_iters"):
        call(max_iters=0)
    with pytest.raises(ValueError, match="max_instances"):
        call(max_instances=0)
    with pytest.raises(ValueError, match="beyond max_instances"):
        call(max_instances=T * S - 1)
    for bad in (-1e-3, float("nan"), -float("inf")):
        with pytest.raises(ValueError, match="max_step must be >= 0"):
            call(max_step=bad)
    for wdt in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="qvel_dt"):
            call(qvel_dt=wdt)
    for thr in (dict(pos_threshold=-1e-3), dict(ori_threshold=-1.0), dict(pos_threshold=None), dict(ori_threshold=float("nan"))):
        with pytest.raises(ValueError, match="threshold mode only"):
            call(**thr)
    for bad in (np.zeros((T, 6)), np.zeros((B + 1, T, 7)), np.zeros((B, 0, 7))):
        with pytest.raises(ValueError, match="must have shape"):
            call({task: bad})
    with pytest.raises(ValueError, match="disagree on the number of waypoints"):
        call({task: poses, post: np.zeros((T + 1, m.nq))})
    with pytest.raises(ValueError, match="targets is empty"):
        call({})
    for bad in (np.zeros((3, m.nq)), np.zeros((B, S, m.nq)), np.zeros((B, T, S, m.nq + 1)), np.zeros((T + 1, S, m.nq)), np.zeros(m.nq)):
        with pytest.raises(ValueError, match="seeds must have shape"):
            call(seeds=bad)
    with pytest.raises(ValueError, match="weights must have shape"):
        call(weights=np.ones(m.nv + 1))
    for bad in (-np.ones(m.nv), np.r_[np.ones(m.nv - 1), np.nan]):
        with pytest.raises(ValueError, match="weights must be >= 0"):
            call(weights=bad)
    # seeds together with a seed table: two sources of the same starts (judged before the table is looked at)
    with pytest.raises(ValueError, match="seeds and seed_table"):
        call(seeds=np.zeros((S, m.nq)), seed_table=object())
    with pytest.raises(ValueError, match="seed_table must be a SeedTable"):
        call(seed_table=object())

    # caller-defined rows are refused, before a handle exists
    class Mine(mink_amd.Task):
        def compute_error(self, configuration):
            return np.zeros((configuration.batch_size, 3))

        def compute_jacobian(self, configuration):
            return np.zeros((configuration.batch_size, 3, configuration.nv))

    with pytest.raises(mink_amd.TaskDefinitionError, match="caller-defined Task / Limit"):
        mink_amd.solve_ik_trajectory_ladder(cfg, [task, Mine(cost=np.ones(3))], 1.0, {task: poses}, **base)

    # the search alone
    nodes = np.zeros((B, T, S, m.nq))
    path = lambda q_nodes=nodes, **kw: mink_amd.ladder_path(cfg, q_nodes, **kw)
    for bad in (np.zeros((T, S)), np.zeros((B + 1, T, S, m.nq)), np.zeros((T, S, m.nq + 1)), None):
        with pytest.raises(ValueError, match="q_nodes must have shape"):
            path(bad)
    with pytest.raises(ValueError, match="at most 256"):
        path(np.zeros((T, 257, m.nq)))
    with pytest.raises(ValueError, match="at most 65535"):
        path(np.broadcast_to(np.zeros((1, 1, m.nq)), (65536, 1, m.nq)))
    with pytest.raises(ValueError, match="at least one"):
        path(np.zeros((T, 0, m.nq)))
    with pytest.raises(ValueError, match="tracked must have shape"):
        path(tracked=np.ones((B, T, S + 1)))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_step must be >= 0"):
            path(max_step=bad)
    with pytest.raises(ValueError, match="weights must be >= 0"):
        path(weights=-np.ones(m.nv))
    with pytest.raises(ValueError, match="weights must have shape"):
        path(weights=np.ones(2))

    for name in ("solve_ik_trajectory_ladder", "LadderResult", "ladder_path", "LadderPath"):
        assert name in mink_amd.__all__ and hasattr(mink_amd, name), name
    assert mink_amd.LadderResult._fields == (
        "q", "v", "status", "iters", "converged", "node_index", "n_tracked", "n_breaks", "path_length", "edge_break", "qvel", "q_all",
        "v_all", "status_all", "iters_all", "converged_all", "seeds")
    assert mink_amd.LadderPath._fields == ("node_index", "q", "n_tracked", "n_breaks", "path_length", "edge_break")
    # the siblings keep their shape
    assert mink_amd.TrajectoryMultistartResult._fields[:9] == ("q", "v", "status", "iters", "converged", "seed_index", "n_tracked",
                                                               "n_complete", "path_length")


# ------------------------------------------------------------------ the C ABI
def _struct(hdr, name):
    fields = hdr.split("typedef struct %s {" % name)[1].split("} %s;" % name)[0]
    return re.findall(r"^\s*(?:const\s+)?(double|int32_t)\s*(\*?)\s*(\w+);", fields, flags=re.M)


def test_entry_points_are_declared_bound_and_documented():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr = open(os.path.join(REPO, "include", "minkhip.h")).read()
    for sym in ("mkh_ladder_select", "mkh_solve_trajectory_ladder"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(L, sym).restype is ctypes.c_int32
        assert f"int32_t {sym}(MkhProblem *problem, int32_t B, int32_t T, int32_t " in hdr
    ctype = {("double", "*"): ctypes.c_void_p, ("int32_t", "*"): ctypes.c_void_p, ("double", ""): ctypes.c_double,
             ("int32_t", ""): ctypes.c_int32}
    for name, mirror, names in (("MkhLadderIO", nat.MkhLadderIO, nat.LADDER_IO_FIELDS),
                                ("MkhTrajectoryLadderIO", nat.MkhTrajectoryLadderIO, nat.TRAJECTORY_LADDER_IO_FIELDS)):
        decl = _struct(hdr, name)
        assert tuple(n for _, _, n in decl) == names
        assert [(n, ctype[(t, p)]) for t, p, n in decl] == list(mirror._fields_)

        class FromHeader(ctypes.Structure):
            _fields_ = [(n, ctype[(t, p)]) for t, p, n in decl]

        assert ctypes.sizeof(mirror) == ctypes.sizeof(FromHeader) == 8 * len(names)
        for n, _ in mirror._fields_:
            assert getattr(mirror, n).offset == getattr(FromHeader, n).offset, n
    # the structs that existed keep their layout
    assert ctypes.sizeof(nat.MkhTrajectoryMultistartIO) == 18 * 8 + 8 + 3 * 4 + 4 and ctypes.sizeof(nat.MkhMultistartIO) == 15 * 8
    for word in ("THE RULE", "1 <= S <= 256", "1 <= T <= 65 535", "The START EDGE", "The start edge is never a break",
                 "the LOWEST s attaining it", "THE RESULT IS DEFINED BY THE RECURRENCE", "never fused", "BITWISE",
                 "(target_index0 + b)·T + t", "every waypoint's OWN", "~MKH_ST_OUTSIDE_LIMITS"):
        assert word in hdr, word


def test_bad_arguments_fail_before_any_device_is_touched():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    err = L.mkh_last_error
    buf = np.zeros(64)
    p = buf.ctypes.data
    io = nat.MkhLadderIO()
    for n in nat.LADDER_IO_FIELDS:
        setattr(io, n, p)
    sel = lambda B=2, T=3, S=4, gate=1.0, io_=io: L.mkh_ladder_select(None, B, T, S, p, p, p, None, gate, ctypes.byref(io_), 0, None)
    assert sel() == -1 and b"null problem" in err()
    tio = nat.MkhTrajectoryLadderIO()
    for n in nat.TRAJECTORY_LADDER_IO_FIELDS:
        if n not in ("max_step_sq", "waypoint_dt", "seeds", "weights", "qvel", "seeds_out", "q_all", "v_all", "status_all",
                     "iters_all", "converged_all"):
            setattr(tio, n, p)
    tio.max_step_sq = float("inf")
    lad = lambda: L.mkh_solve_trajectory_ladder(None, 2, 3, 4, p, p, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, 0, 0, ctypes.byref(tio), 0, None)
    assert lad() == -1 and b"null problem" in err()
    assert L.mkh_solve_trajectory_ladder(None, 2, 3, 4, p, p, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, 0, 0, None, 0, None) == -1
    # the multi-start entry point behind the rungs still refuses what it refused
    mio = nat.MkhMultistartIO()
    assert L.mkh_solve_multistart(None, 2, p, p, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, 4, 0, 0, ctypes.byref(mio), 0, None) == -1
    assert b"null problem" in err()


# ------------------------------------------------------------------ the kernels
NEW_KERNELS = ("ladder_search_kernel", "ladder_gather_kernel", "ladder_gather_i32_kernel", "ladder_tracked_kernel")


def test_new_kernels_have_no_spills_no_scratch_no_callee_frames():
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    for k in NEW_KERNELS:
        e = table.get(k)
        assert e is not None, sorted(x for x in table if "ladder" in x)
        assert e["vgpr_spills_with_callees"] == 0 and e["vgpr_spills"] == 0 and e["scratch_bytes_per_lane"] == 0, (k, e)
        assert e["callees"] == {}, (k, e["callees"])                  # everything inlined: no call, no stack
    with open(os.path.join(GOLDEN, "spill_budget.json")) as fh:
        assert not any("ladder" in k for k in json.load(fh))          # no allowance


# ------------------------------------------------------------------ the example and the bench tool
@pytest.mark.parametrize("script", ["examples/batched_ladder_ur5e.py", "tools/bench_ladder.py"])
def test_example_and_bench_tool_load_no_undefined_names(script):
    from test_entry_scripts import REPO as root, _undefined_globals
    assert _undefined_globals(os.path.join(root, script)) == []
