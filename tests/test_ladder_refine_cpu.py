"""Ladder refinement without a GPU: the restated rule (tests/ladder_refine_ref.py) on hand-made paths against a toy loop — a
table of canned results per (waypoint, start) on dyadic values, so every cost is exact and the expected outputs are typed by
hand —, the public calls' argument checks before any device is touched, the entry points exported, bound and mirrored field
for field, and the new kernels compiled without spills, scratch or callee frames."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import ladder_refine_ref as rref
import oracle_configs as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
INF = float("inf")


# ------------------------------------------------------------------ the restatement against a toy loop
def n(a, nq=6):
    """The UR5e posture with joint 0 at `a`, everything else 0: c(n(a) -> n(b)) = (b - a)^2, exact on dyadic values."""
    x = np.zeros(nq)
    x[0] = a
    return x


class ToyLoop:
    """loop(t, start) from a table {(t, joint 0 of the start): joint 0 of the result}: a listed start converges there in 3
    iterations with status MKH_ST_OUTSIDE_LIMITS (a bit that does not stop a result from tracking) and v = 2 x; a start that is
    not listed stays where it is and does not converge.  Every call is recorded."""

    def __init__(self, table, nv=6):
        self.table, self.nv, self.calls = table, nv, []

    def __call__(self, t, start):
        self.calls.append((t, start[:, 0].tolist()))
        B = len(start)
        x, st, it, cv = start.copy(), np.zeros(B, np.int32), np.full(B, 9, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            hit = self.table.get((t, float(start[b, 0])))
            if hit is not None:
                x[b], st[b], it[b], cv[b] = n(hit), 1, 3, 1
        return x, 2.0 * x, st, it, cv


def run(path, tracked, table, gate, q0=0.0):
    m = oc.model("ur5e")
    loop = ToyLoop(table)
    judged = []
    out = rref.refine(m, loop, n(q0)[None], np.array([[n(a) for a in path]]), None if tracked is None else np.array([tracked]),
                      gate, judged=judged)
    return out, loop, judged


def test_single_far_node_is_pulled_back_by_the_forward_sweep():
    out, loop, _ = run([0.25, 0.5, 4.0, 1.0], None, {(2, 0.5): 0.75}, 1.0)
    assert out["key_in"][0] == (0, 2, 21.375) and out["key_work"][0] == (0, 0, 0.25)
    assert out["q"][0, :, 0].tolist() == [0.25, 0.5, 0.75, 1.0] and not out["q"][0, :, 1:].any()
    assert out["repaired"][0].tolist() == [0, 0, 1, 0] and out["refined"].tolist() == [1]
    assert out["tracked"][0].tolist() == [1, 1, 1, 1] and out["edge_break"][0].tolist() == [0, 0, 0, 0]
    assert (out["n_tracked"][0], out["n_breaks"][0], out["path_length"][0]) == (4, 0, 0.25)
    # the loop's rows at the repaired node only
    assert out["v"][0, 2, 0] == 1.5 and not out["v"][0, [0, 1, 3]].any()
    assert out["status"][0].tolist() == [0, 0, 1, 0] and out["iters"][0].tolist() == [0, 0, 3, 0]
    assert out["converged"][0].tolist() == [0, 0, 1, 0]
    # one launch per waypoint and sweep: 4 forward, 3 backward; the bad waypoint starts at its neighbour, the others at themselves
    assert [t for t, _ in loop.calls] == [0, 1, 2, 3, 2, 1, 0]
    assert [s[0] for _, s in loop.calls] == [0.25, 0.5, 0.5, 1.0, 0.75, 0.5, 0.25]


def test_lost_nodes_are_resolved_from_their_neighbour():
    # T = 2, no gate: only the lost node is bad
    out, loop, judged = run([0.5, 0.75], [1, 0], {(1, 0.5): 1.0}, INF)
    assert out["key_in"][0] == (1, 0, 0.3125) and out["key_work"][0] == (0, 0, 0.5)
    assert out["q"][0, :, 0].tolist() == [0.5, 1.0] and out["repaired"][0].tolist() == [0, 1] and out["refined"].tolist() == [1]
    assert out["tracked"][0].tolist() == [1, 1] and out["n_tracked"].tolist() == [2] and out["path_length"].tolist() == [0.5]
    assert [t for t, _ in loop.calls] == [0, 1, 0]
    # T = 1: the start is the caller's posture, the start edge has no gate, the backward sweep is empty
    out, loop, judged = run([0.5], [0], {(0, 0.0): 8.0}, 1.0)
    assert out["q"][0, 0, 0] == 8.0 and out["repaired"].tolist() == [[1]] and out["refined"].tolist() == [1]
    assert (out["n_tracked"][0], out["n_breaks"][0], out["path_length"][0]) == (1, 0, 64.0) and out["edge_break"].tolist() == [[0]]
    assert loop.calls == [(0, [0.0])] and judged == []
    # ... and a loop that does not converge leaves everything as it came
    out, _, _ = run([0.5], [0], {}, 1.0)
    assert out["refined"].tolist() == [0] and out["repaired"].tolist() == [[0]] and out["q"][0, 0, 0] == 0.5
    assert out["tracked"].tolist() == [[0]] and (out["n_tracked"][0], out["path_length"][0]) == (0, 0.25)
    # a lost node whose repair lands beyond the gate stays lost
    out, _, _ = run([0.5, 0.75], [1, 0], {(1, 0.5): 2.0}, 1.0)
    assert out["refined"].tolist() == [0] and out["tracked"][0].tolist() == [1, 0] and out["q"][0, :, 0].tolist() == [0.5, 0.75]


def test_two_branches_heal_backward_where_forward_cannot():
    # branch A at waypoints 0, 1, branch B at 2, 3; from A the loop of waypoint 2 does not converge, from B everything does
    table = {(1, 4.25): 4.0, (0, 4.0): 3.75}
    out, loop, _ = run([0.25, 0.5, 4.25, 4.5], None, table, 1.0)
    assert out["key_in"][0] == (0, 1, 14.25) and out["key_work"][0] == (0, 0, 14.25)      # the start edge is never a break
    assert out["q"][0, :, 0].tolist() == [3.75, 4.0, 4.25, 4.5] and out["repaired"][0].tolist() == [2, 2, 0, 0]
    assert out["refined"].tolist() == [1] and out["edge_break"][0].tolist() == [0, 0, 0, 0]
    assert (out["n_tracked"][0], out["n_breaks"][0], out["path_length"][0]) == (4, 0, 14.25)
    # forward: waypoint 2 tried from 0.5; backward: 1 from 4.25, then 0 — its edge into 1 became a break — from 4.0
    assert loop.calls == [(0, [0.25]), (1, [0.5]), (2, [0.5]), (3, [4.5]), (2, [4.25]), (1, [4.25]), (0, [4.0])]
    # T = 2, the same shape at its smallest
    out, _, _ = run([0.5, 4.5], None, {(0, 4.5): 4.25}, 1.0)
    assert out["q"][0, :, 0].tolist() == [4.25, 4.5] and out["repaired"][0].tolist() == [2, 0] and out["n_breaks"].tolist() == [0]


def test_guard_restores_a_path_that_the_repairs_made_worse():
    # backward, waypoint 1 moves to branch B (accepted: 0.75^2 from 4.25) but waypoint 0 cannot follow: the break moved one edge
    # down and grew — one break as before, a longer path: the input comes back bit for bit
    path = [0.25, 0.5, 4.25, 4.5]
    out, loop, _ = run(path, None, {(1, 4.25): 5.0}, 1.0)
    assert out["key_in"][0] == (0, 1, 14.25) and out["key_work"][0] == (0, 1, 23.25)
    assert out["refined"].tolist() == [0] and not out["repaired"].any()
    assert out["q"][0, :, 0].tolist() == path and out["edge_break"][0].tolist() == [0, 0, 1, 0]
    assert (out["n_tracked"][0], out["n_breaks"][0], out["path_length"][0]) == (4, 1, 14.25)
    assert not out["v"].any() and not out["status"].any() and not out["iters"].any() and not out["converged"].any()
    # an equal key is not strictly smaller either: the break moves down by one edge, same cost
    out, _, _ = run(path, None, {(1, 4.25): 4.0}, 1.0)
    assert out["key_work"][0] == (0, 1, 14.25) and out["refined"].tolist() == [0] and out["q"][0, :, 0].tolist() == path
    # an untouched good path: every loop starts at its own node, nothing is repaired
    out, loop, _ = run([0.25, 0.5, 0.75, 1.0], None, {}, 1.0)
    assert out["refined"].tolist() == [0] and [s[0] for _, s in loop.calls] == [0.25, 0.5, 0.75, 1.0, 0.75, 0.5, 0.25]


def test_instances_do_not_see_each_other_and_callers_rows_are_kept():
    m = oc.model("ur5e")
    loop = ToyLoop({(2, 0.5): 0.75})
    paths = np.array([[n(a) for a in row] for row in ([0.25, 0.5, 4.0, 1.0], [0.25, 0.5, 0.75, 1.0])])
    mine = dict(v=np.full((2, 4, 6), 7.0), status=np.full((2, 4), 1, np.int32), iters=np.full((2, 4), 5, np.int32),
                converged=np.ones((2, 4), np.int32))
    out = rref.refine(m, loop, np.zeros((2, 6)), paths, None, 1.0, **mine)
    assert out["refined"].tolist() == [1, 0] and out["repaired"].tolist() == [[0, 0, 1, 0], [0, 0, 0, 0]]
    assert out["iters"].tolist() == [[5, 5, 3, 5], [5, 5, 5, 5]] and out["v"][0, 2, 0] == 1.5 and out["v"][1, 2, 0] == 7.0
    assert (mine["iters"] == 5).all()                                                    # (the caller's arrays are not written)


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
    path = np.zeros((B, T, m.nq))
    ladder = lambda targets={task: poses}, tasks_=tasks, **kw: mink_amd.solve_ik_trajectory_ladder(
        cfg, tasks_, 1.0, targets, **{**dict(n_seeds=S, max_iters=10, pos_threshold=1e-4, ori_threshold=1e-4, refine=True), **kw})
    alone = lambda targets={task: poses}, tasks_=tasks, q_path=path, **kw: mink_amd.refine_path(cfg, tasks_, 1.0, targets, q_path, **kw)
    for call in (ladder, alone):
        for thr in (dict(pos_threshold=-1e-3), dict(ori_threshold=-1.0), dict(pos_threshold=None), dict(ori_threshold=float("nan"))):
            with pytest.raises(ValueError, match="threshold mode only"):
                call(**thr)
        for bad in (-1e-3, float("nan"), -float("inf")):
            with pytest.raises(ValueError, match="max_step must be >= 0"):
                call(max_step=bad)
        with pytest.raises(ValueError, match="max_iters"):
            call(max_iters=0)
        with pytest.raises(ValueError, match="max_instances"):
            call(max_instances=0)
        with pytest.raises(ValueError, match="at least one frame task"):
            call({post: np.zeros((T, m.nq))}, [post])
        with pytest.raises(ValueError, match="weights must be >= 0"):
            call(weights=-np.ones(m.nv))
        with pytest.raises(ValueError, match="weights must have shape"):
            call(weights=np.ones(m.nv + 1))
        with pytest.raises(ValueError, match="at most 65535"):
            call({task: np.broadcast_to(poses[:1, :1], (B, 65536, 7))})

        # caller-defined rows are refused, before a handle exists
        class Mine(mink_amd.Task):
            def compute_error(self, configuration):
                return np.zeros((configuration.batch_size, 3))

            def compute_jacobian(self, configuration):
                return np.zeros((configuration.batch_size, 3, configuration.nv))

        with pytest.raises(mink_amd.TaskDefinitionError, match="caller-defined Task / Limit"):
            call(tasks_=[task, Mine(cost=np.ones(3))])
    # the pass alone: its path and flags
    for bad in (np.zeros((T, m.nq + 1)), np.zeros((B + 1, T, m.nq)), np.zeros((B, T + 1, m.nq)), np.zeros(m.nq), None):
        with pytest.raises(ValueError, match="q_path must have shape"):
            alone(q_path=bad)
    for bad in (np.ones((B, T + 1)), np.ones((T + 1,)), np.ones((B, T, 1))):
        with pytest.raises(ValueError, match="tracked must have shape"):
            alone(tracked=bad)
    with pytest.raises(ValueError, match="targets is empty"):
        alone({})

    for name in ("refine_path", "RefinedPath", "RefinedLadderResult"):
        assert name in mink_amd.__all__ and hasattr(mink_amd, name), name
    assert mink_amd.RefinedPath._fields == ("q", "tracked", "repaired", "refined", "edge_break", "n_tracked", "n_breaks",
                                            "path_length", "v", "status", "iters", "converged")
    # the refined ladder's result: LadderResult's fields in its order, the two new ones behind them, None by default
    assert mink_amd.RefinedLadderResult._fields == mink_amd.LadderResult._fields + ("repaired", "refined")
    r = mink_amd.RefinedLadderResult(*range(10))
    assert r.repaired is None and r.refined is None and r.edge_break == 9
    import inspect
    sig = inspect.signature(mink_amd.solve_ik_trajectory_ladder)
    assert sig.parameters["refine"].default is False and list(sig.parameters)[-1] == "refine"


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
    for sym in ("mkh_ladder_refine", "mkh_solve_trajectory_ladder_refined"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(L, sym).restype is ctypes.c_int32
        assert f"int32_t {sym}(MkhProblem *problem, int32_t B, int32_t T, " in hdr
    ctype = {("double", "*"): ctypes.c_void_p, ("int32_t", "*"): ctypes.c_void_p, ("double", ""): ctypes.c_double,
             ("int32_t", ""): ctypes.c_int32}
    decl = _struct(hdr, "MkhLadderRefineIO")
    assert tuple(name for _, _, name in decl) == nat.LADDER_REFINE_IO_FIELDS
    assert [(name, ctype[(t, p)]) for t, p, name in decl] == list(nat.MkhLadderRefineIO._fields_)

    class FromHeader(ctypes.Structure):
        _fields_ = [(name, ctype[(t, p)]) for t, p, name in decl]

    assert ctypes.sizeof(nat.MkhLadderRefineIO) == ctypes.sizeof(FromHeader) == 8 * len(nat.LADDER_REFINE_IO_FIELDS)
    for name, _ in nat.MkhLadderRefineIO._fields_:
        assert getattr(nat.MkhLadderRefineIO, name).offset == getattr(FromHeader, name).offset, name
    # the structs that existed keep their layout
    assert ctypes.sizeof(nat.MkhLadderIO) == 6 * 8 and ctypes.sizeof(nat.MkhTrajectoryLadderIO) == 21 * 8
    assert ctypes.sizeof(nat.MkhTrajectoryMultistartIO) == 18 * 8 + 8 + 3 * 4 + 4 and ctypes.sizeof(nat.MkhMultistartIO) == 15 * 8
    assert ctypes.sizeof(nat.MkhTrajectoryIO) == 6 * 8 + 8 + 3 * 4 + 4
    for word in ("THE RULE OF THE REFINEMENT", "STRICTLY smaller", "bit for bit", "THE RESULT IS NEVER WORSE", "the start edge",
                 "stays exempt", "one rounded addition each", "MKH_FLAG_WARM_START does not enter", "T = 1: the sweep is empty",
                 "+inf legal", "names the node that was replaced", "refine == NULL"):
        assert word in hdr, word


def test_bad_arguments_fail_before_any_device_is_touched():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    err = L.mkh_last_error
    buf = np.zeros(64)
    p = buf.ctypes.data
    rio = nat.MkhLadderRefineIO()
    for name in nat.LADDER_REFINE_IO_FIELDS[2:10]:
        setattr(rio, name, p)
    rio.max_step_sq = 1.0
    ref = lambda io=ctypes.byref(rio): L.mkh_ladder_refine(None, 2, 3, p, p, p, p, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, io, 0, None)
    assert ref() == -1 and b"null problem" in err()
    assert ref(None) == -1
    tio = nat.MkhTrajectoryLadderIO()
    for name in nat.TRAJECTORY_LADDER_IO_FIELDS[3:13]:
        setattr(tio, name, p)
    tio.max_step_sq = float("inf")
    for r in (ctypes.byref(rio), None):
        assert L.mkh_solve_trajectory_ladder_refined(None, 2, 3, 4, p, p, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, 0, 0, ctypes.byref(tio),
                                                     r, 0, None) == -1 and b"null problem" in err()


# ------------------------------------------------------------------ the kernels
NEW_KERNELS = ("ladder_refine_step_kernel", "ladder_refine_guard_kernel")


def test_new_kernels_have_no_spills_no_scratch_no_callee_frames():
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    for k in NEW_KERNELS:
        e = table.get(k)
        assert e is not None, sorted(x for x in table if "ladder" in x)
        assert e["vgpr_spills_with_callees"] == 0 and e["vgpr_spills"] == 0 and e["sgpr_spills"] == 0, (k, e)
        assert e["scratch_bytes_per_lane"] == 0, (k, e)
        assert e["callees"] == {}, (k, e["callees"])                  # everything inlined: no call, no stack
