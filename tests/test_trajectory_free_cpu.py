"""CPU-side checks of checked candidate tracking (include/minkhip.h THE RULE "with a checker" of
mkh_solve_trajectory_multistart): the restated rule of tests/trajectory_free_ref.py on hand-made flag tables, the conditions the
GPU tests rely on in the two shared cases of tests/trajectory_free_cases.py, the host-side refusals of the Python layer, the new
entry points without a device, and the kernels' resources."""

import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import clearance_ref as cr
import swept_ref as sref
import trajectory_free_cases as tc
import trajectory_free_ref as tfref
import trajectory_multistart_ref as tmref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = np.inf, np.nan


# ------------------------------------------------------------------ the restated rule on hand-made tables
def _tables(node, edge, converged=None, status=None):
    """flags() on (T, R) tables of margins; the edges asked for are recorded."""
    node, edge = np.array(node, dtype=np.float64), np.array(edge, dtype=np.float64)
    cv = np.ones(node.shape, np.int32) if converged is None else np.array(converged, dtype=np.int32)
    st = np.zeros(node.shape, np.int32) if status is None else np.array(status, dtype=np.int32)
    asked = []

    def edge_margin_of(t, i):
        asked.append((t, i))
        return edge[t, i]

    return tfref.flags(cv, st, node, edge_margin_of) + (asked,)


def test_an_edge_collision_loses_the_waypoint_it_enters():
    """One candidate, T = 4, every node free, the motion 1 -> 2 collides: waypoint 2 is lost, waypoints 1 and 3 count."""
    status, eligible, edge, counted, asked = _tables([[1.0], [1.0], [1.0], [1.0]], [[7.0], [0.5], [-0.1], [0.5]])
    assert not status.any() and eligible.all() and asked == [(1, 0), (2, 0), (3, 0)]
    assert counted[:, 0].tolist() == [True, True, False, True]
    assert edge[:, 0].tolist() == [INF, 0.5, -0.1, 0.5]                  # (the table's entry for t = 0 is never asked for)


def test_a_colliding_node_is_not_swept_into_but_out_of():
    """Node 1 collides (once by a negative margin, once by a NaN): it gets the bit, its edge is not asked for and is NaN, the edge
    out of it into node 2 is asked for; OUTSIDE_LIMITS alone does not make a row ineligible, another status bit does."""
    for m in (-0.2, NAN):
        status, eligible, edge, counted, asked = _tables([[1.0], [m], [1.0]], [[0.0], [9.0], [0.3]], status=[[1], [1], [0]])
        assert status[:, 0].tolist() == [1, 1 | 64, 0] and eligible[:, 0].tolist() == [True, False, True]
        assert asked == [(2, 0)] and np.isposinf(edge[0, 0]) and np.isnan(edge[1, 0]) and edge[2, 0] == 0.3
        assert counted[:, 0].tolist() == [True, False, True]
    status, eligible, edge, counted, asked = _tables([[1.0], [1.0]], [[0.0], [0.3]], converged=[[1], [0]], status=[[2], [0]])
    assert not eligible.any() and asked == [] and np.isnan(edge[1, 0]) and not counted.any() and status[:, 0].tolist() == [2, 0]


def test_the_start_edge_never_counts_and_selection_is_the_plain_rule():
    """Two instances of two candidates.  Waypoint 0 counts whatever the table says about its edge; the count decides before the
    length, the length before the index; nobody tracked anything: candidate 0."""
    node = [[1.0, 1.0, -1.0, -1.0], [1.0, 1.0, -1.0, -1.0]]
    edge = [[-5.0, -5.0, -5.0, -5.0], [-0.1, 0.2, 0.2, 0.2]]
    status, eligible, em, counted, asked = _tables(node, edge)
    assert np.isposinf(em[0]).all() and counted[0].tolist() == [True, True, False, False]
    assert asked == [(1, 0), (1, 1)] and counted[1].tolist() == [False, True, False, False]
    seed, n_tracked, n_complete, counts = tfref.pick(counted, np.array([[1.0, 9.0], [3.0, 2.0]]), 2)
    assert counts.tolist() == [[1, 2], [0, 0]]
    assert seed.tolist() == [1, 0] and n_tracked.tolist() == [2, 0] and n_complete.tolist() == [1, 0]
    # equal counts: the shorter path; equal lengths: the lower index; a NaN length behind every finite one
    both = np.ones((2, 4), dtype=bool)
    assert tfref.pick(both, np.array([[2.0, 1.0], [1.0, 1.0]]), 2)[0].tolist() == [1, 0]
    assert tfref.pick(both, np.array([[NAN, 5.0], [INF, NAN]]), 2)[0].tolist() == [1, 0]


# ------------------------------------------------------------------ the shared cases
def _census(ref):
    nm, em, el = ref["node_margin_all"], ref["edge_margin_all"], ref["eligible"]
    swept = np.isfinite(em[1:])
    return dict(colliding=int((~(nm >= 0.0)).sum()), blocked=int((el[1:] & ~(em[1:] >= 0.0)).sum()), unswept=int((~el[1:]).sum()),
                nearest=float(min(np.abs(nm).min(), np.abs(em[1:][swept]).min())), swept=swept)


def test_shared_case_has_what_the_gpu_tests_rely_on():
    """ur5e_all, B = 3, S = 4, T = 5, M = 5: 8 colliding nodes, 21 blocked edges, 6 edges that are not swept, no reference margin
    within 1.2e-2 of zero (so no flag is excluded at the GPU tests' 1e-9), and both masks change a pick."""
    (model, limits, q, q_all), ref = tc.shared()
    B, S, T, M = (tc.SHARED[k] for k in "BSTM")
    assert q_all.shape == (T, B * S, model.nq) and (q == np.asarray(model.qpos0)).all()
    assert len(cr.pair_list(limits)[1]) <= 32 and model.nbody <= 32            # four rows per wavefront
    c = _census(ref)
    print({k: v for k, v in c.items() if k != "swept"})
    assert (c["colliding"], c["blocked"], c["unswept"]) == (8, 21, 6) and c["nearest"] >= 1.2e-2
    ones, zeros = np.ones((T, B * S), np.int32), np.zeros((T, B * S), np.int32)
    plain = tmref.choose(model, q, q_all, ones, zeros, S)[0]
    nodes_only = tfref.rule(model, limits, q, q_all, None, None, S, M, edges=False)["seed_index"]
    assert plain.tolist() == [1, 3, 3] and nodes_only.tolist() == [0, 3, 3] and ref["seed_index"].tolist() == [0, 3, 1]
    # placement: +inf at waypoint 0 of the _all array, NaN exactly at the rows that are not eligible
    em = ref["edge_margin_all"]
    assert np.isposinf(em[0]).all() and (np.isnan(em[1:]) == ~ref["eligible"][1:]).all() and not np.isinf(em[1:]).any()
    assert sorted(ref["swept"]) == [(t + 1, i) for t, i in zip(*np.nonzero(ref["eligible"][1:]))]
    # the pieces: a node is clearance_ref's row, an edge swept_ref's, the chosen rows plain gathers
    t, i = ref["swept"][3]
    assert em[t, i] == sref.sweep(model, limits, q_all[t - 1, i], q_all[t, i], M).margin[0]
    np.testing.assert_array_equal(ref["node_margin_all"], cr.clearance(model, limits, q_all.reshape(-1, model.nq)).margin.reshape(T, B * S))
    rows = np.arange(B) * S + ref["seed_index"]
    np.testing.assert_array_equal(ref["edge_margin"], em[:, rows].T)
    np.testing.assert_array_equal(ref["q_path"], np.swapaxes(q_all[:, rows], 0, 1))
    np.testing.assert_array_equal(ref["tracked"].sum(axis=1), ref["n_tracked"])
    assert not ref["edge_collision"][:, 0].any() and (ref["edge_collision"].sum(axis=1) == ref["n_edge_collisions"]).all()
    assert (ref["status_all"] == np.where(ref["node_margin_all"] < 0.0, 64, 0)).all()


def test_whole_wavefront_case_has_what_the_gpu_tests_rely_on():
    """g1 (46 pairs, a free joint), B = 2, S = 3, T = 3, M = 3, one node replaced by a row in collision: the drawn rows alone have
    no colliding node and node margins at least 1.8e-2 from zero; with the replacement one colliding node, 2 blocked edges, counts
    that the check changes, and still no margin — node or edge — within 1e-3 of zero."""
    (model, limits, q, q_all), ref = tc.g1()
    B, S, T, M = (tc.G1[k] for k in "BSTM")
    assert len(cr.pair_list(limits)[1]) == 46 and int(model.jnt_type[0]) == 0  # one row per wavefront; quaternion arcs
    drawn = tc.candidates("g1", B, S, T)[3]
    changed = (drawn != q_all).any(axis=2)
    assert changed.sum() == 1 and changed[tc.G1_REPLACED]
    before = cr.clearance(model, limits, drawn.reshape(-1, model.nq))
    assert not before.in_collision.any() and np.abs(before.margin).min() >= 1.8e-2
    c = _census(ref)
    print({k: v for k, v in c.items() if k != "swept"})
    assert (c["colliding"], c["blocked"], c["unswept"]) == (1, 2, 0)
    assert np.abs(ref["node_margin_all"]).min() >= 1.8e-2 and c["nearest"] >= 1e-3          # the margin condition, after the replacement
    assert ref["node_margin_all"][tc.G1_REPLACED] < 0.0 and ref["status_all"][tc.G1_REPLACED] == 64
    # every row tracked, so the plain rule counts T everywhere; the check takes two waypoints from one candidate, one from another
    assert ref["counts"].tolist() == [[3, 1, 3], [2, 3, 3]] and ref["n_complete"].tolist() == [2, 2]
    assert ref["seed_index"].tolist() == [0, 1] and ref["n_tracked"].tolist() == [3, 3]


# ------------------------------------------------------------------ refusals without a device
def test_host_side_refusals():
    import mink_amd
    model, _, rows = cr.fixture("ur5e_all")
    ck = mink_amd.CollisionChecker(model, cr.fixture_limits("ur5e_all"))
    cfg = mink_amd.Configuration(model, rows[:2].copy())
    paths = np.zeros((2, 3, 4, model.nq))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0)
    targets = {task: np.tile(np.array([1.0, 0, 0, 0, 0.3, 0.2, 0.4]), (2, 3, 1))}
    fused = lambda c=cfg, **kw: mink_amd.solve_ik_trajectory_multistart(c, [task], 1.0, targets, 4, 5, 1e-4, 1e-4, **kw)
    other = mink_amd.Configuration(mink_amd.load_robot("g1"))
    for call in (lambda **kw: mink_amd.candidate_path(cfg, paths, **kw), fused):
        with pytest.raises(ValueError, match="collision_check must be a CollisionChecker"):
            call(collision_check=object())
        with pytest.raises(ValueError, match="edge_samples must be >= 1"):
            call(collision_check=ck, edge_samples=0)
    with pytest.raises(ValueError, match="another model"):
        mink_amd.candidate_path(other, np.zeros((3, 4, other.nq)), collision_check=ck)
    with pytest.raises(ValueError, match="another model"):
        fused(other, collision_check=ck)
    with pytest.raises(ValueError, match="q_paths must have shape"):
        mink_amd.candidate_path(cfg, np.zeros((3, 4, model.nq + 1)))
    with pytest.raises(ValueError, match="tracked must have shape"):
        mink_amd.candidate_path(cfg, paths, tracked=np.ones((3, 5)))
    with pytest.raises(ValueError, match="weights must be >= 0"):
        mink_amd.candidate_path(cfg, paths, weights=-np.ones(model.nv))
    # a closed checker, before any handle is asked for
    from mink_amd import _native as nat
    ck.close()

    class Handle:
        nmodel = None
    Handle.nmodel = type("M", (), {"model": model})()
    with pytest.raises(ValueError, match="closed"):
        nat._checker_handle(Handle(), ck, 3)


def test_entry_points_refuse_bad_arguments_before_any_device():
    from mink_amd import _native as nat
    L = nat.lib()
    cio, fio, tio = nat.MkhTrajectoryCandidatesIO(), nat.MkhTrajectoryFreeIO(), nat.MkhTrajectoryMultistartIO()
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.addressof(buf)
    for n in nat.TRAJECTORY_CANDIDATES_IO_FIELDS:
        setattr(cio, n, ptr)
    for n in nat.TRAJECTORY_FREE_IO_FIELDS[:4]:
        setattr(fio, n, ptr)
    for n in ("q_traj", "v_traj", "status", "iters", "converged", "seed_index", "n_tracked", "n_complete", "path_length"):
        setattr(tio, n, ptr)
    fake = ctypes.c_void_p(ptr)            # a handle nobody dereferences: what is refused here is refused from the arguments alone
    sel = lambda p, ck, n, f: L.mkh_select_trajectory_candidates(p, ck, 1, 2, 2, ptr, ptr, None, None, n, ctypes.byref(cio), f, 0, None)
    err = lambda: L.mkh_last_error()
    assert sel(None, None, 1, None) == -1 and b"null problem" in err()
    assert sel(None, None, 1, ctypes.byref(fio)) == -1 and b"free_io is given without a checker" in err()
    assert sel(None, fake, 1, None) == -1 and b"free_io and its outputs" in err()
    assert sel(None, fake, 0, ctypes.byref(fio)) == -1 and b"n_samples = 0 must be >= 1" in err()
    assert sel(None, fake, 1, ctypes.byref(fio)) == -1 and b"null problem" in err()
    hollow = nat.MkhTrajectoryFreeIO()
    assert sel(None, fake, 1, ctypes.byref(hollow)) == -1 and b"free_io and its outputs" in err()
    fused = lambda p, ck, n, f: L.mkh_solve_trajectory_multistart_free(p, ck, 1, 2, 2, ptr, ptr, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, 0, 0,
                                                                       n, ctypes.byref(tio), f, 0, None)
    assert fused(None, fake, 1, None) == -1 and b"free_io and its outputs" in err()
    assert fused(None, fake, 0, ctypes.byref(fio)) == -1 and b"n_samples = 0 must be >= 1" in err()
    assert fused(None, None, 1, ctypes.byref(fio)) == -1 and b"null checker" in err()
    assert fused(None, fake, 1, ctypes.byref(fio)) == -1 and b"null problem" in err()
    # the plain call keeps its own order
    assert L.mkh_solve_trajectory_multistart(None, 1, 2, 2, ptr, ptr, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, 0, 0, ctypes.byref(tio), 0,
                                             None) == -1 and b"null problem" in err()


# ------------------------------------------------------------------ the C ABI and the Python surface
def _struct(hdr, name):
    fields = hdr.split("typedef struct %s {" % name)[1].split("} %s;" % name)[0]
    return re.findall(r"^\s*(?:const\s+)?(double|int32_t)\s*(\*?)\s*(\w+);", fields, flags=re.M)


def test_entry_points_are_declared_bound_and_documented():
    from mink_amd import _native as nat
    L = nat.lib()
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr = open(os.path.join(REPO, "include", "minkhip.h")).read()
    for sym in ("mkh_select_trajectory_candidates", "mkh_solve_trajectory_multistart_free"):
        assert sym in nat.EXPORTED_SYMBOLS and getattr(L, sym).restype is ctypes.c_int32
        assert f"int32_t {sym}(MkhProblem *problem, MkhProblem *checker" in hdr
    assert len(L.mkh_solve_trajectory_multistart_free.argtypes) == len(L.mkh_solve_trajectory_multistart.argtypes) + 3
    for name, fields in (("MkhTrajectoryFreeIO", nat.TRAJECTORY_FREE_IO_FIELDS), ("MkhTrajectoryCandidatesIO", nat.TRAJECTORY_CANDIDATES_IO_FIELDS)):
        decl = _struct(hdr, name)
        assert tuple(n for _, _, n in decl) == fields
        assert all((t, p) in (("double", "*"), ("int32_t", "*")) for t, p, _ in decl)
        assert [n for n, _ in getattr(nat, name)._fields_] == [n for _, _, n in decl]
        assert ctypes.sizeof(getattr(nat, name)) == len(fields) * ctypes.sizeof(ctypes.c_void_p)
    assert nat.TRAJECTORY_FREE_IO_FIELDS == ("node_margin", "edge_margin", "edge_collision", "n_edge_collisions", "node_margin_all",
                                             "edge_margin_all")
    # the struct that existed keeps its layout
    assert ctypes.sizeof(nat.MkhTrajectoryMultistartIO) == 18 * 8 + 8 + 3 * 4 + 4
    for word in ("THE RULE, with a checker (mkh_select_trajectory_candidates", "evaluated AFTER that OR", "IN THE _all ARRAY TOO",
                 "This differs from the ladder's edge_margin_all", "whatever the checker says", "differs by the one bit only",
                 "free_io NULL iff checker NULL", "is still refused"):
        assert word in hdr, word


def test_python_surface():
    import mink_amd
    from mink_amd import _native as nat
    for name in ("FreeTrajectoryMultistartResult", "candidate_path", "CandidatePath", "FreeCandidatePath"):
        assert name in mink_amd.__all__ and hasattr(mink_amd, name), name
    base = mink_amd.TrajectoryMultistartResult._fields
    assert mink_amd.FreeTrajectoryMultistartResult._fields == base + (
        "node_margin", "edge_margin", "edge_collision", "n_edge_collisions", "tracked", "node_margin_all", "edge_margin_all")
    p = inspect.signature(mink_amd.solve_ik_trajectory_multistart).parameters
    assert list(p)[-2:] == ["collision_check", "edge_samples"]           # behind everything that was there
    assert p["collision_check"].default is None and p["edge_samples"].default == 8
    p = inspect.signature(mink_amd.candidate_path).parameters
    assert list(p) == ["configuration", "q_paths", "tracked", "weights", "collision_check", "edge_samples"]
    assert p["tracked"].default is None and p["collision_check"].default is None and p["edge_samples"].default == 8
    assert mink_amd.FreeCandidatePath._fields[:5] == mink_amd.CandidatePath._fields
    p = inspect.signature(nat.NativeProblem.solve_trajectory_multistart_free).parameters
    assert p["edge_samples"].default == 8 and "checker" in p
    assert inspect.signature(nat.NativeProblem.select_trajectory_candidates).parameters["checker"].default is None
    # the counted flags from the (B, T) outputs
    sik = __import__("importlib").import_module("mink_amd.solve_ik")
    el = np.array([[True, True, False, True], [False, True, True, True]])
    em = np.array([[INF, 0.2, NAN, -0.1], [INF, 0.0, NAN, 0.3]])
    assert sik._counted(el, em).tolist() == [[True, True, False, False], [False, True, False, True]]


def test_kernel_resources():
    """Both builds of the check kernel, and the small kernel behind the gathers: no spilled register, vector or scalar, no scratch,
    no callee (tests/test_swept_cpu.py's terms for the sweep).  The score kernel with its optional pointer stays free of spills."""
    from mink_amd import _native as nat
    nat.lib()
    with open(os.path.join(REPO, "mink_amd", "kernel_resources.json")) as fh:
        res = json.load(fh)
    assert sorted(k for k in res if k.startswith("tmf_check_kernel")) == ["tmf_check_kernel<16>", "tmf_check_kernel<64>"]
    for name in ("tmf_check_kernel<16>", "tmf_check_kernel<64>", "tmf_edge_flags_kernel", "tms_score_select_kernel", "sweep_kernel<16>",
                 "sweep_kernel<64>"):
        e = res[name]
        print(name, {k: e[k] for k in ("vgprs", "sgprs", "sgpr_spills", "scratch_bytes_per_lane", "occupancy_waves_per_simd")})
        assert e["vgpr_spills_with_callees"] == 0 and e["vgpr_spills"] == 0 and e["scratch_bytes_per_lane"] == 0 and e["callees"] == {}
        assert e["sgpr_spills"] == 0 and e["sgpr_spills_with_callees"] == 0, (name, e)
    # (the sample loop holds ONE clr_row: three waves per SIMD, as the sweep's)
    assert res["tmf_check_kernel<16>"]["occupancy_waves_per_simd"] >= res["sweep_kernel<16>"]["occupancy_waves_per_simd"]
    assert res["tmf_check_kernel<64>"]["occupancy_waves_per_simd"] >= res["sweep_kernel<64>"]["occupancy_waves_per_simd"]
    with open(os.path.join(REPO, "tests", "golden", "spill_budget.json")) as fh:
        budget = json.dumps(json.load(fh))
    assert "tmf_" not in budget and "tms_score" not in budget


@pytest.mark.parametrize("script", ["examples/batched_collision_free_trajectory_ur5e.py", "tools/bench_trajectory_free.py"])
def test_example_and_bench_tool_load_no_undefined_names(script):
    from test_entry_scripts import REPO as root, _undefined_globals
    assert _undefined_globals(os.path.join(root, script)) == []
    src = open(os.path.join(root, script)).read()
    assert "collision_check" in src or "select_trajectory_candidates" in src
