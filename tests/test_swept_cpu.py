"""CPU-side checks of the swept clearance and the checked ladder (include/minkhip.h "THE RULE OF THE SWEEP", THE RULE "with a
checker"): the references of the GPU tests against enumeration and against the plain ladder's, the condition on the shared
fixture's margins, the host-side refusals of the Python layer, the new entry points without a device, and the kernels' resources."""

import ctypes
import inspect
import json
import os

import numpy as np
import pytest

import clearance_ref as cr
import keyframe_ref as kf
import ladder_free_ref as lfref
import ladder_ref as lref
import swept_cases as sc
import swept_ref as sref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_graph(rng, T=4, S=3):
    """Costs with ties and zeros, a gate that makes breaks, lost nodes and a dense mask."""
    start = rng.integers(0, 4, size=S).astype(np.float64)
    edges = rng.integers(0, 4, size=(T, S, S)).astype(np.float64)
    lost = rng.random((T, S)) < 0.3
    blocked = rng.random((T, S, S)) < 0.5
    return start, edges, lost, blocked


@pytest.mark.parametrize("seed", range(12))
def test_masked_search_is_the_enumeration_of_all_paths(seed):
    """T = 4, S = 3: the recurrence under the amended key against all 81 paths, ties included (integer costs tie often)."""
    start, edges, lost, blocked = _random_graph(np.random.default_rng(seed))
    for gate in (np.inf, 1.5):
        a, b = lfref.search(start, edges, lost, blocked, gate), lfref.brute_force(start, edges, lost, blocked, gate)
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])
        np.testing.assert_array_equal(a[3], b[3])
        # the key's first component counts what the rule says it counts
        path = a[0]
        gone = int(lost[0][path[0]]) + sum(int(lost[t][path[t]]) | int(blocked[t][path[t]][path[t - 1]]) for t in range(1, 4))
        assert a[1][0] == gone


@pytest.mark.parametrize("seed", range(6))
def test_an_all_zero_mask_is_the_plain_search(seed):
    start, edges, lost, _ = _random_graph(np.random.default_rng(100 + seed), T=5, S=4)
    for gate in (np.inf, 1.5):
        a = lfref.search(start, edges, lost, np.zeros((5, 4, 4), dtype=bool), gate)
        b = lref.search(start, edges, lost, gate)
        np.testing.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])
        assert not a[3].any()


def test_the_mask_can_change_the_path_and_lose_a_waypoint():
    """Two nodes per rung, node 0 nearest: the plain search stays on node 0; with the edge 0 -> 0 into waypoint 1 blocked the masked
    one leaves it, and with every edge into waypoint 1 blocked it loses exactly that waypoint."""
    start, edges, lost = np.array([0.0, 1.0]), np.zeros((3, 2, 2)), np.zeros((3, 2), dtype=bool)
    edges[1:] = np.array([[0.0, 1.0], [1.0, 0.0]])
    blocked = np.zeros((3, 2, 2), dtype=bool)
    assert list(lfref.search(start, edges, lost, blocked)[0]) == [0, 0, 0]
    blocked[1, 0, 0] = True
    path, key, _, col = lfref.search(start, edges, lost, blocked)
    assert key[0] == 0 and not col.any() and list(path) != [0, 0, 0]
    blocked[1] = True
    path, key, _, col = lfref.search(start, edges, lost, blocked)
    assert key[0] == 1 and list(col) == [0, 1, 0]


def test_sweep_reference_on_its_pieces():
    """swept_ref.sweep is blend_posture + clearance_ref.clearance + numpy's min / argmin: held here against those pieces on a
    few edges of the UR5e fixture, with a NaN end, an infinite end, and an edge from a row to itself."""
    model, _, rows = cr.fixture("ur5e_all")
    limits = cr.limits_of(cr.fixture_limits("ur5e_all"))
    a, b = rows[:5].copy(), rows[5:10].copy()
    a[1, 2] = np.nan
    b[2, 0] = np.inf
    b[3] = a[3]
    M = 3
    out = sref.sweep(model, limits, a, b, M)
    assert out.samples.shape == (5, M)
    for e in (0, 4):
        q_mid = kf.blend_posture(model, a[e], b[e], 2.0 / 4.0)
        np.testing.assert_array_equal(q_mid, a[e] + 0.5 * (b[e] - a[e]))                  # (hinges only: a + u (b - a))
        assert out.samples[e, 1] == cr.clearance(model, limits, q_mid[None]).margin[0]
        assert out.margin[e] == out.samples[e].min() and out.sample[e] == out.samples[e].argmin()
    for e in (1, 2):
        assert np.isnan(out.margin[e]) and out.sample[e] == 0 and out.pair[e] == 0 and out.in_collision[e]
    own = cr.clearance(model, limits, a[3][None])
    assert out.margin[3] == own.margin[0] and out.sample[3] == 0 and out.pair[3] == own.pair[0]


def test_fixture_condition_on_the_ladder_case():
    """Collision flags are thresholds on margins: the shared ladder case keeps every reference margin more than 1e-6 away from
    zero, so no case is ever excluded — and it exercises what the GPU test is about: colliding nodes, blocked edges, edges that
    are not swept, a path the mask changes, an instance that must lose a waypoint.  The figures are pinned: 9 colliding nodes of
    80, 232 of the 256 edges swept and 141 of them blocked, the path changed in instances 0 and 2, n_tracked (5, 4, 5, 5), min |edge
    margin| 4.6e-4, min |node margin| 2.3e-2.  (The issue's probe quotes 6 nodes, 149 edges, all four paths changed and 1.15e-3:
    it drew its nodes in another order from the same rows — its code is not part of the repository —; the set-up — three quarters from the free rows, one quarter from all, default_rng(0) — is the same.)"""
    (model, limits, q, q_nodes), (node_margin, eff, em), sel = sc.ladder_ref()
    B, T, S = eff.shape
    assert (B, T, S) == (4, 5, 4)
    swept = np.isfinite(em)
    print("ladder case: %d colliding nodes of %d, %d blocked edges of %d swept (%d edges), min |edge margin| %.3e, min |node margin| %.3e"
          % (int((~eff).sum()), eff.size, int(sel["blocked"].sum()), int(swept.sum()), em[:, 1:].size,
             np.abs(em[swept]).min(), np.abs(node_margin).min()))
    assert np.isfinite(node_margin).all() and np.abs(node_margin).min() > 1e-6
    assert np.abs(em[swept]).min() > 1e-6
    assert not swept[:, 0].any() and (swept[:, 1:] == np.broadcast_to(eff[:, 1:, :, None], (B, T - 1, S, S))).all()
    assert 0 < (~eff).sum() < eff.size // 2 and 0 < sel["blocked"].sum() < swept.sum()
    plain = lref.select(model, q, q_nodes)
    changed = (plain["node_index"] != sel["node_index"]).any(axis=1)
    print("the mask changes the path of instances", np.nonzero(changed)[0], "; n_tracked", sel["n_tracked"])
    assert changed.any() and (sel["n_tracked"] < T).any() and (sel["n_tracked"] == T).any()
    assert (int((~eff).sum()), int(swept.sum()), int(sel["blocked"].sum())) == (9, 232, 141)
    assert changed.tolist() == [True, False, True, False] and sel["n_tracked"].tolist() == [5, 4, 5, 5]
    assert 4.5e-4 < np.abs(em[swept]).min() < 4.7e-4 and 2.2e-2 < np.abs(node_margin).min() < 2.4e-2
    # every returned edge of a complete path is free, by the sweep on the path itself
    for b in np.nonzero(sel["n_tracked"] == T)[0]:
        path = q_nodes[b, np.arange(T), sel["node_index"][b]]
        assert not sref.sweep(model, limits, path[:-1], path[1:], 7).in_collision.any()
        assert not cr.clearance(model, limits, path).in_collision.any()


def test_host_side_refusals():
    import mink_amd
    model, _, rows = cr.fixture("ur5e_all")
    ck = mink_amd.CollisionChecker(model, cr.fixture_limits("ur5e_all"))
    cfg = mink_amd.Configuration(model, rows[:2].copy())
    nodes = np.zeros((2, 3, 4, model.nq))
    with pytest.raises(ValueError, match="edge_samples"):
        mink_amd.ladder_path(cfg, nodes, collision_check=ck, edge_samples=0)
    with pytest.raises(ValueError, match="CollisionChecker"):
        mink_amd.ladder_path(cfg, nodes, collision_check=object())
    other = mink_amd.Configuration(mink_amd.load_robot("g1"))
    with pytest.raises(ValueError, match="another model"):
        mink_amd.ladder_path(other, np.zeros((3, 4, other.nq)), collision_check=ck)
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0)
    targets = {task: np.tile(np.array([1.0, 0, 0, 0, 0.3, 0.2, 0.4]), (2, 3, 1))}
    call = lambda **kw: mink_amd.solve_ik_trajectory_ladder(cfg, [task], 1.0, targets, 4, 5, 1e-4, 1e-4, collision_check=ck, **kw)
    with pytest.raises(ValueError, match="refine"):
        call(refine=True)
    with pytest.raises(ValueError, match="edge_samples"):
        call(edge_samples=0)
    with pytest.raises(ValueError, match="another model"):
        mink_amd.solve_ik_trajectory_ladder(other, [task], 1.0, targets, 4, 5, 1e-4, 1e-4, collision_check=ck)
    with pytest.raises(ValueError, match="n_samples"):
        ck.swept_clearance(rows[:2], rows[2:4], n_samples=0)
    with pytest.raises(ValueError, match="one shape"):
        ck.swept_clearance(rows[:2], rows[2:5])
    with pytest.raises(ValueError, match="one shape"):
        ck.swept_clearance(rows[:2, :5], rows[2:4, :5])
    ck.close()
    with pytest.raises(ValueError, match="closed"):
        ck.swept_clearance(rows[:2], rows[2:4])


def test_python_surface():
    import mink_amd
    for name in ("SweptClearance", "FreeLadderPath", "FreeLadderResult", "FreeLadderNodesResult"):
        assert name in mink_amd.__all__ and hasattr(mink_amd, name), name
    assert mink_amd.SweptClearance._fields == ("margin", "sample", "pair", "in_collision")
    for cls, base in ((mink_amd.FreeLadderPath, mink_amd.LadderPath), (mink_amd.FreeLadderResult, mink_amd.LadderResult),
                      (mink_amd.FreeLadderNodesResult, mink_amd.LadderNodesResult)):
        n = len(base._fields)
        assert cls._fields[:n] == base._fields and cls._fields[n:n + 3] == ("edge_collision", "n_edge_collisions", "edge_margin")
    for fn in (mink_amd.ladder_path, mink_amd.solve_ik_trajectory_ladder):
        p = inspect.signature(fn).parameters
        assert p["collision_check"].default is None and p["edge_samples"].default == 8
    assert inspect.signature(mink_amd.CollisionChecker.swept_clearance).parameters["n_samples"].default == 8


def test_entry_points_refuse_null_arguments():
    from mink_amd import _native as nat
    lib = nat.lib()
    sio, lio, fio, tio = nat.MkhSweptClearanceIO(), nat.MkhLadderIO(), nat.MkhLadderFreeIO(), nat.MkhTrajectoryLadderIO()
    assert lib.mkh_swept_clearance(None, 1, None, None, 1, ctypes.byref(sio), 0, None) == -1
    assert b"null problem" in lib.mkh_last_error()
    assert lib.mkh_ladder_select_free(None, None, 1, 1, 1, None, None, None, None, 1.0, 1, ctypes.byref(lio), ctypes.byref(fio), 0, None) == -1
    assert b"null problem" in lib.mkh_last_error()
    assert lib.mkh_solve_trajectory_ladder_free(None, None, 1, 1, 1, 0, 0.1, None, None, None, None, 1.0, 1e-3, 5, 1e-3, 1e-3, 0, 0, 1,
                                                ctypes.byref(tio), None, None, ctypes.byref(fio), 0, None) == -1
    assert b"null problem" in lib.mkh_last_error()
    assert ctypes.sizeof(nat.MkhSweptClearanceIO) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(nat.MkhLadderFreeIO) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_kernel_resources():
    """Both builds of the sweep, and the two clearance builds behind the move of their row body into the shared header: no
    spilled register, vector or scalar, no scratch, no callee (tests/test_clearance_cpu.py's terms).  The masked search beside
    the plain one: no spilled VGPR and no scratch (the plain search's scalar spills are its own: tests/test_ladder_cpu.py)."""
    from mink_amd import _native as nat
    nat.lib()
    with open(os.path.join(REPO, "mink_amd", "kernel_resources.json")) as fh:
        res = json.load(fh)
    assert sorted(k for k in res if k.startswith("sweep_kernel")) == ["sweep_kernel<16>", "sweep_kernel<64>"]
    for name in ("sweep_kernel<16>", "sweep_kernel<64>", "clearance_kernel<16>", "clearance_kernel<64>", "ladder_search_kernel",
                 "ladder_search_free_kernel", "ladder_free_tracked_kernel"):
        e = res[name]
        print(name, {k: e[k] for k in ("vgprs", "sgprs", "sgpr_spills", "scratch_bytes_per_lane", "occupancy_waves_per_simd")})
        assert e["vgpr_spills_with_callees"] == 0 and e["vgpr_spills"] == 0 and e["scratch_bytes_per_lane"] == 0 and e["callees"] == {}
        if name.startswith(("sweep_kernel", "clearance_kernel")):
            assert e["sgpr_spills"] == 0 and e["sgpr_spills_with_callees"] == 0, (name, e)
    with open(os.path.join(REPO, "tests", "golden", "spill_budget.json")) as fh:
        budget = json.dumps(json.load(fh))
    assert "sweep_kernel" not in budget and "ladder_search_free" not in budget


@pytest.mark.parametrize("script", ["examples/batched_collision_free_ladder_ur5e.py", "tools/bench_swept.py"])
def test_example_and_bench_tool_load_no_undefined_names(script):
    from test_entry_scripts import REPO as root, _undefined_globals
    assert _undefined_globals(os.path.join(root, script)) == []
