"""The refinement pass with a checker without a GPU (include/minkhip.h "THE RULE OF THE REFINEMENT, with a checker"): the
restatement (tests/ladder_refine_free_ref.py) on canned loop tables whose nodes and candidates are rows of the UR5e `ur5e_all`
fixture — every branch of the rule is taken at least once —, against the plain restatement under a neutral checker, under a
checker that everything collides with, the guard's promise on every table; the new entry points without a device, the Python
surface, and the kernels' resources."""

import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import clearance_ref as cr
import ladder_refine_free_ref as fref
import ladder_refine_ref as rref
import swept_ref as sref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
M = 3
SHARED = ("q", "tracked", "repaired", "refined", "edge_break", "n_tracked", "n_breaks", "path_length", "v", "status", "iters",
          "converged")
_pool = {}


def pool():
    """The fixture's model and limits, and rows of it by what the reference says of them: A — free rows, the motion between any
    two of them free; Bc — free rows, the motion between any two of them free, every motion between A and Bc blocked (the arm on
    the other side of its base); C — rows in collision.  All margins are more than 1e-3 away from zero."""
    if not _pool:
        model, _, rows = cr.fixture("ur5e_all")
        ref = cr.fixture_ref("ur5e_all")
        limits = cr.limits_of(cr.fixture_limits("ur5e_all"))
        free = np.flatnonzero(ref.margin > 0.01)[:12]
        E = np.full((12, 12), np.nan)
        for i in range(12):
            for j in range(12):
                if i != j:
                    E[i, j] = sref.sweep(model, limits, rows[free[i]][None], rows[free[j]][None], M).margin[0]
        assert (np.abs(E[~np.isnan(E)]) > 1e-3).all()
        A = [0] + [j for j in range(1, 12) if E[0, j] > 0]
        Bc = [j for j in range(1, 12) if E[0, j] < 0]
        ok = lambda I, J, sign: all(sign * E[i, j] > 0 for i in I for j in J if i != j)
        A = [i for i in A if ok([i], A, 1)]                       # (drop a row whose motion to another one of its side is blocked)
        assert len(A) >= 5 and len(Bc) >= 3 and ok(A, A, 1) and ok(Bc, Bc, 1) and ok(A, Bc, -1) and ok(Bc, A, -1), (A, Bc)
        _pool.update(model=model, limits=limits, A=rows[free[A]], Bc=rows[free[Bc]], C=rows[np.flatnonzero(ref.margin < -0.01)[:4]])
    return _pool


class TableLoop:
    """loop(t, start) from a table {(t, start row): result row}: a listed start converges there in 3 iterations with status
    MKH_ST_OUTSIDE_LIMITS (a bit that does not stop a result from tracking) and v = 2 x[:nv]; a start that is not listed stays
    where it is and does not converge.  Every call is recorded."""

    def __init__(self, table):
        self.table = {(t, np.asarray(a).tobytes()): np.asarray(x) for (t, a, x) in table}
        self.calls = []

    def __call__(self, t, start):
        self.calls.append(t)
        B = len(start)
        x, st, it, cv = start.copy(), np.zeros(B, np.int32), np.full(B, 9, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            hit = self.table.get((t, start[b].tobytes()))
            if hit is not None:
                x[b], st[b], it[b], cv[b] = hit, 1, 3, 1
        return x, 2.0 * x, st, it, cv


def tables():
    """name -> (q0, path, tracked, loop table, gate): one instance each."""
    P = pool()
    a, b, c = P["A"], P["Bc"], P["C"]
    cost = lambda u, v: rref.row_costs(P["model"], u[None], v[None])[0]
    far = max(range(1, len(a)), key=lambda i: cost(a[0], a[i]) + cost(a[i], b[1]))      # the longest detour through A
    return {
        "forward":       (a[0], [a[0], c[0], a[2]], None, [(1, a[0], a[1])], INF),
        "backward":      (a[0], [a[0], c[0], a[2]], None, [(1, a[2], a[1])], INF),
        "node":          (a[0], [a[0], c[0], a[2]], None, [(1, a[0], c[1]), (1, a[2], c[2])], INF),
        "edge":          (a[0], [a[0], c[0], a[2]], None, [(1, a[0], b[0]), (1, a[2], b[1])], INF),
        "gate":          (a[0], [a[0], c[0], a[2]], None, [(1, a[0], a[1])], 1e-3),
        "far_collides":  (a[0], [a[0], b[0], b[1]], None, [(1, a[0], a[far])], INF),
        "lost_flag":     (a[0], [a[0], a[1], a[2], a[3]], [1, 0, 1, 0], [(1, a[0], a[4]), (3, a[2], a[1])], INF),
        "T1":            (a[0], [c[0]], None, [(0, a[0], a[1])], INF),
        "T1_kept":       (a[0], [c[0]], None, [(0, a[0], c[1])], INF),
        "T2_forward":    (a[0], [c[0], a[2]], None, [(0, a[0], a[1])], INF),
        "T2_backward":   (a[0], [c[0], a[2]], None, [(0, a[2], a[1])], INF),
    }


def run(name, limits=None, plain=False):
    P = pool()
    q0, path, trk, table, gate = tables()[name]
    loop, judged, margins, counts = TableLoop(table), [], [], {}
    args = (np.asarray(q0)[None], np.array([path]), None if trk is None else np.array([trk]))
    if plain:
        return rref.refine(P["model"], loop, *args, gate), loop
    out = fref.refine(P["model"], P["limits"] if limits is None else limits, loop, *args, M, gate, judged=judged, margins=margins,
                      counts=counts)
    return out, loop, margins, counts


def test_every_branch_of_the_rule_on_designed_tables():
    total = dict.fromkeys(fref.COUNTERS, 0)
    for name in tables():
        out, loop, margins, counts = run(name)
        T = len(tables()[name][1])
        assert loop.calls == list(range(T)) + list(range(T - 2, -1, -1))          # one launch per waypoint and sweep
        assert min(abs(x) for x in margins) > 1e-3
        for k in total:
            total[k] += counts[k]
        # the guard: never worse under the amended key
        key = (T - out["n_tracked"][0], out["n_breaks"][0], out["path_length"][0])
        assert key <= out["key_in"][0] and key == (out["key_work"][0] if out["refined"][0] else out["key_in"][0])
        assert bool(out["refined"][0]) == (out["key_work"][0] < out["key_in"][0])
        # the outputs hang together
        lost = (out["tracked"][0] == 0) | (out["edge_collision"][0] != 0)
        assert out["n_tracked"][0] == T - lost.sum() and out["n_edge_collisions"][0] == out["edge_collision"][0].sum()
        assert np.isposinf(out["edge_margin"][0, 0]) and out["edge_collision"][0, 0] == 0
        assert (np.isnan(out["edge_margin"][0, 1:]) == (out["tracked"][0, 1:] == 0)).all()      # swept iff the destination is tracked
        assert ((out["node_margin"][0] >= 0) | (out["tracked"][0] == 0)).all()
        print(name, counts, "refined", out["refined"].tolist(), "repaired", out["repaired"].tolist(), "key", out["key_in"][0], "->", key)
    print(total)
    assert all(v > 0 for v in total.values()), total


def test_designed_outcomes():
    P = pool()
    a = P["A"]
    # a colliding node is repaired from its predecessor; the far edge is swept for the new node
    out, _, _, counts = run("forward")
    assert out["refined"].tolist() == [1] and out["repaired"][0].tolist() == [0, 1, 0] and out["tracked"][0].tolist() == [1, 1, 1]
    assert counts["accepted_forward"] == 1 and counts["far_edges"] == 1 and out["n_tracked"].tolist() == [3]
    np.testing.assert_array_equal(out["q"][0, 1], a[1])
    assert out["status"][0].tolist() == [0, 1, 0] and out["iters"][0].tolist() == [0, 3, 0] and (out["v"][0, 1] == 2.0 * a[1]).all()
    assert (out["edge_margin"][0, 1:] > 0).all() and not out["edge_collision"].any()
    # ... or from its successor where the forward loop does not converge
    out, _, _, counts = run("backward")
    assert out["repaired"][0].tolist() == [0, 2, 0] and counts["accepted_backward"] == 1 and counts["far_edges"] == 1
    assert out["n_tracked"].tolist() == [3]
    # a candidate in collision, a candidate behind a blocked motion, a candidate beyond the gate: the input comes back bit for bit,
    # the colliding node with flag 0 although it came in as tracked
    for name, why in (("node", "rejected_node"), ("edge", "rejected_edge"), ("gate", "rejected_gate")):
        out, _, _, counts = run(name)
        path = np.array(tables()[name][1])
        assert counts[why] >= 1 and counts["accepted_forward"] == counts["accepted_backward"] == 0
        assert out["refined"].tolist() == [0] and not out["repaired"].any() and out["tracked"][0].tolist() == [1, 0, 1]
        np.testing.assert_array_equal(out["q"][0], path)
        assert not out["v"].any() and not out["status"].any() and not out["iters"].any() and not out["converged"].any()
        assert out["node_margin"][0, 1] < 0 and np.isnan(out["edge_margin"][0, 1])
    # a committed repair whose far edge collides: one waypoint lost as before, a longer path — the guard keeps p
    out, _, _, counts = run("far_collides")
    assert counts["accepted_forward"] == 1 and counts["far_edges"] == 1 and out["work_repaired"][0].tolist() == [0, 1, 0]
    assert out["key_in"][0][:2] == out["key_work"][0][:2] == (1, 0) and out["key_work"][0][2] > out["key_in"][0][2]
    assert out["refined"].tolist() == [0] and not out["repaired"].any() and out["edge_collision"][0].tolist() == [0, 1, 0]
    np.testing.assert_array_equal(out["q"][0], np.array(tables()["far_collides"][1]))
    assert out["tracked"][0].tolist() == [1, 1, 1] and out["n_tracked"].tolist() == [2] and out["edge_margin"][0, 1] < 0
    # T = 1: no edge at all; T = 2: no far edge behind a backward repair at waypoint 0
    out, _, _, counts = run("T1")
    assert out["refined"].tolist() == [1] and out["repaired"].tolist() == [[1]] and counts["far_edges"] == 0
    assert out["edge_margin"].tolist() == [[INF]] and out["n_tracked"].tolist() == [1]
    out, _, _, _ = run("T1_kept")
    assert out["refined"].tolist() == [0] and out["tracked"].tolist() == [[0]] and out["n_tracked"].tolist() == [0]
    out, _, _, counts = run("T2_forward")
    assert out["repaired"].tolist() == [[1, 0]] and counts["far_edges"] == 1 and out["n_tracked"].tolist() == [2]
    out, _, _, counts = run("T2_backward")
    assert out["repaired"].tolist() == [[2, 0]] and counts["far_edges"] == 0 and out["n_tracked"].tolist() == [2]


def _with_dmin(dmin):
    return [(p, dmin, d) for p, _, d in pool()["limits"]]


def test_a_neutral_checker_is_the_plain_pass():
    """minimum_distance_from_collisions = -10: no row is closer than that to anything."""
    for name in tables():
        out, _, margins, _ = run(name, _with_dmin(-10.0))
        want, _ = run(name, plain=True)
        for f in SHARED:
            np.testing.assert_array_equal(out[f], want[f], err_msg=f"{name}: {f}")
        assert out["key_in"] == want["key_in"] and out["key_work"] == want["key_work"]
        assert not out["edge_collision"].any() and not out["n_edge_collisions"].any() and min(margins) > 9.0


def test_a_checker_everything_collides_with():
    """minimum_distance_from_collisions = +10: nothing is accepted, the input comes back bit for bit, nothing counts as tracked."""
    for name in tables():
        out, _, _, counts = run(name, _with_dmin(10.0))
        path = np.array(tables()[name][1])
        assert counts["accepted_forward"] == counts["accepted_backward"] == 0
        assert out["refined"].tolist() == [0] and not out["repaired"].any() and not out["tracked"].any()
        np.testing.assert_array_equal(out["q"][0], path)
        assert out["n_tracked"].tolist() == [0] and not out["edge_collision"].any() and (out["node_margin"] < 0).all()
        assert not out["v"].any() and not out["status"].any() and not out["iters"].any() and not out["converged"].any()


# ------------------------------------------------------------------ the C ABI
def _struct(hdr, name):
    fields = hdr.split("typedef struct %s {" % name)[1].split("} %s;" % name)[0]
    return re.findall(r"^\s*(?:const\s+)?(double|int32_t)\s*(\*?)\s*(\w+);", fields, flags=re.M)


def test_entry_points_are_declared_bound_and_documented():
    from mink_amd import _native as nat
    L = nat.lib()
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr = open(os.path.join(REPO, "include", "minkhip.h")).read()
    for sym in ("mkh_ladder_refine_free", "mkh_solve_trajectory_ladder_free_refined"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(L, sym).restype is ctypes.c_int32
        assert f"int32_t {sym}(MkhProblem *problem, MkhProblem *checker, int32_t B, int32_t T, " in hdr
    assert L.mkh_solve_trajectory_ladder_free_refined.argtypes == L.mkh_solve_trajectory_ladder_free.argtypes
    assert len(L.mkh_ladder_refine_free.argtypes) == len(L.mkh_ladder_refine.argtypes) + 3
    decl = _struct(hdr, "MkhLadderRefineFreeIO")
    assert tuple(name for _, _, name in decl) == nat.LADDER_REFINE_FREE_IO_FIELDS
    assert all((t, p) in (("double", "*"), ("int32_t", "*")) for t, p, _ in decl)
    assert [n for n, _ in nat.MkhLadderRefineFreeIO._fields_] == [name for _, _, name in decl]
    assert ctypes.sizeof(nat.MkhLadderRefineFreeIO) == 4 * ctypes.sizeof(ctypes.c_void_p)
    # the structs that existed keep their layout
    assert ctypes.sizeof(nat.MkhLadderRefineIO) == 8 * len(nat.LADDER_REFINE_IO_FIELDS) and ctypes.sizeof(nat.MkhLadderFreeIO) == 5 * 8
    for word in ("THE RULE OF THE REFINEMENT, with a checker", "whatever its source is", "never accepted", "evaluated anew",
                 "A NaN decides", "a kept node that collides", "node_index keeps the search's choice"):
        assert word in hdr, word


def test_entry_points_refuse_null_arguments():
    from mink_amd import _native as nat
    L = nat.lib()
    rio, fio, tio, lio = nat.MkhLadderRefineIO(), nat.MkhLadderRefineFreeIO(), nat.MkhTrajectoryLadderIO(), nat.MkhLadderFreeIO()
    assert L.mkh_ladder_refine_free(None, None, 2, 3, None, None, None, None, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, 4, ctypes.byref(rio),
                                    ctypes.byref(fio), 0, None) == -1
    assert b"null problem" in L.mkh_last_error()
    for r in (ctypes.byref(rio), None):
        assert L.mkh_solve_trajectory_ladder_free_refined(None, None, 1, 1, 1, 0, 0.1, None, None, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3,
                                                          0, 0, 1, ctypes.byref(tio), None, r, ctypes.byref(lio), 0, None) == -1
        assert b"null problem" in L.mkh_last_error()


def test_python_surface():
    import mink_amd
    from mink_amd import _native as nat
    for name in ("FreeRefinedPath", "FreeRefinedLadderResult", "FreeRefinedLadderNodesResult"):
        assert name in mink_amd.__all__ and hasattr(mink_amd, name), name
    tail = ("edge_collision", "n_edge_collisions", "edge_margin", "node_margin")
    assert mink_amd.FreeRefinedPath._fields == mink_amd.RefinedPath._fields + tail
    assert nat.LadderRefineFreeOut._fields == nat.LadderRefineOut._fields + tail
    assert mink_amd.FreeRefinedLadderResult._fields == mink_amd.FreeLadderResult._fields + ("repaired", "refined")
    assert mink_amd.FreeRefinedLadderNodesResult._fields == mink_amd.FreeLadderNodesResult._fields + ("repaired", "refined")
    p = inspect.signature(mink_amd.refine_path).parameters
    assert p["collision_check"].default is None and p["edge_samples"].default == 8
    assert list(p)[-2:] == ["collision_check", "edge_samples"]           # behind everything that was there
    p = inspect.signature(mink_amd.solve_ik_trajectory_ladder).parameters
    assert list(p)[-1] == "refine" and p["refine"].default is False
    assert inspect.signature(nat.NativeProblem.solve_trajectory_ladder_free).parameters["refine"].default is False
    assert inspect.signature(nat.NativeProblem.ladder_refine_free).parameters["edge_samples"].default == 8


def test_host_side_refusals():
    import mink_amd as mink
    model, _, rows = cr.fixture("ur5e_all")
    cfg = mink.Configuration(model, rows[:1].copy())
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    tg = np.zeros((1, 2, 7)); tg[..., 0] = 1.0
    kw = dict(n_seeds=2, max_iters=3, pos_threshold=1e-4, ori_threshold=1e-4)
    with pytest.raises(ValueError, match='refine="free" is the refinement pass with a checker'):
        mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, refine="free", **kw)
    with pytest.raises(ValueError, match="refine must be False, True or"):
        mink.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: tg}, refine="checked", **kw)
    with pytest.raises(ValueError, match="collision_check must be a CollisionChecker"):
        mink.refine_path(cfg, [task], 1.0, {task: tg}, rows[:2][None], collision_check=object())


def test_kernel_resources():
    """Both builds of the check kernel: no spilled vector register, no scratch, no callee.  The refinement kernels and both builds
    of the sweep keep their names and stay free of spilled vector registers."""
    from mink_amd import _native as nat
    nat.lib()
    with open(os.path.join(REPO, "mink_amd", "kernel_resources.json")) as fh:
        res = json.load(fh)
    assert sorted(k for k in res if k.startswith("lr_check_kernel")) == ["lr_check_kernel<16>", "lr_check_kernel<64>"]
    for name in ("lr_check_kernel<16>", "lr_check_kernel<64>"):
        e = res[name]
        print(name, {k: e[k] for k in ("vgprs", "sgprs", "sgpr_spills", "scratch_bytes_per_lane", "occupancy_waves_per_simd")})
        assert e["vgpr_spills_with_callees"] == 0 and e["vgpr_spills"] == 0 and e["scratch_bytes_per_lane"] == 0 and e["callees"] == {}
    for name in ("ladder_refine_step_kernel", "ladder_refine_guard_kernel", "ladder_refine_step_free_kernel",
                 "ladder_refine_guard_free_kernel", "sweep_kernel<16>", "sweep_kernel<64>"):
        e = res[name]
        assert e["vgpr_spills_with_callees"] == 0 and e["vgpr_spills"] == 0 and e["scratch_bytes_per_lane"] == 0 and e["callees"] == {}, name
    with open(os.path.join(REPO, "tests", "golden", "spill_budget.json")) as fh:
        budget = json.dumps(json.load(fh))
    assert "lr_check" not in budget and "ladder_refine" not in budget


@pytest.mark.parametrize("script", ["examples/batched_collision_free_ladder_ur5e.py", "tools/bench_ladder_refine_free.py"])
def test_example_and_bench_tool_load_no_undefined_names(script):
    from test_entry_scripts import REPO as root, _undefined_globals
    assert _undefined_globals(os.path.join(root, script)) == []
    src = open(os.path.join(root, script)).read()
    assert "refine" in src
