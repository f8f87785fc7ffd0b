"""The ladder on deduplicated nodes and the turn unwinding without a GPU: the unwinding rule (tests/unwind_ref.py) on designed
values, the properties the header claims for the composed rule (tests/ladder_nodes_ref.py) on synthetic rungs, argument
validation before any device is touched, and the new symbols declared, bound and documented."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import ladder_nodes_ref as lnref
import ladder_ref
import oracle_configs as oc
import unwind_cases as uc
import unwind_ref as uw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T2 = uw.TWO_PI
PI = np.float64(np.pi)


# ------------------------------------------------------------------ 1. the unwinding rule on designed values
def test_eligibility():
    m = uc.turns_model()
    assert [e[0] for e in uw.eligible(m)] == [uc.UNLIMITED, uc.WIDE]          # not the short hinge, the slide, the ball, the free joint
    u = oc.model("ur5e")
    assert [e[0] for e in uw.eligible(u)] == [0, 1, 3, 4, 5]                  # the elbow's range, 6.283, is less than TWO_PI
    assert float(u.jnt_range[2][1] - u.jnt_range[2][0]) < float(T2) <= float(u.jnt_range[0][1] - u.jnt_range[0][0])
    assert T2 == 2.0 * PI and repr(float(T2)) == "6.283185307179586"


def test_half_turns_round_to_even_and_the_map_is_idempotent():
    one = lambda x, r, lim=False, lo=0.0, hi=0.0: uw.unwind_value(np.float64(x), np.float64(r), lim, np.float64(lo), np.float64(hi))
    # r - x exactly +pi and -pi: quotient +0.5 / -0.5, the even neighbour is 0 — the value stays, bit for bit
    for x, r in ((0.0, PI), (0.0, -PI), (0.25 - PI, 0.25), (0.25 + PI, 0.25)):
        assert (np.float64(r) - np.float64(x)) / T2 in (0.5, -0.5)
        assert uw.same_bits(one(x, r), x)
    # 1.5 -> 2 and 2.5 -> 2 (half to even), and the results are fixed points
    for x, r, k in ((0.0, 3.0 * PI, 2.0), (1.0 + 5.0 * PI, 1.0, -2.0), (0.0, -3.0 * PI, -2.0)):
        assert abs((np.float64(r) - np.float64(x)) / T2) in (1.5, 2.5)
        y = one(x, r)
        assert y == np.float64(x) + np.float64(k) * T2
        assert uw.same_bits(one(y, r), y)
    assert np.signbit(one(-0.0, 0.1)) and one(-0.0, 0.1) == 0.0                # k = 0 returns x itself: -0.0 stays -0.0
    # ordinary values: the nearest turn, then nothing
    rng = np.random.default_rng(0)
    for x, r in zip(rng.uniform(-40, 40, 200), rng.uniform(-7, 7, 200)):
        y = one(x, r)
        assert abs(r - y) <= float(PI) * (1 + 1e-15) and uw.same_bits(one(y, r), y)
        assert abs(np.rint((y - x) / T2) * T2 - (y - x)) < 1e-13


def test_limits_cut_the_shift_back():
    lo, hi = np.float64(-9.5), np.float64(9.5)
    one = lambda x, r: uw.unwind_value(np.float64(x), np.float64(r), True, lo, hi)
    # at the limits and one ulp inside, pulled outward by the reference: stays (inside stays inside)
    for x, r in ((hi, hi + 5.0), (lo, lo - 5.0), (np.nextafter(hi, -np.inf), hi + 5.0), (np.nextafter(lo, np.inf), lo - 5.0)):
        assert uw.same_bits(one(x, r), x)
    # ... and inward: moves by whole turns, stays inside
    assert one(hi, hi - 7.0) == hi - T2 and one(lo, lo + 13.0) == lo + 2.0 * T2
    # cut back by one turn: the quotient says 1, x + TWO_PI is beyond range_hi
    x = np.float64(9.4 - float(T2) + 3.0)
    assert np.rint((np.float64(9.4) - x) / T2) == 1.0 and x + T2 > hi and uw.same_bits(one(x, 9.4), x)
    # cut back by two: the quotient says 3, one turn fits
    x, r = np.float64(2.7), np.float64(22.4)
    assert np.rint((r - x) / T2) == 3.0 and x + 2.0 * T2 > hi >= x + T2 and one(x, r) == x + T2
    # the mirror image at range_lo
    assert np.rint((-r + x) / T2) == -3.0 and one(-x, -r) == -x - T2
    # a value outside its range is not pulled in, and does not move further out
    assert uw.same_bits(one(hi + 1.0, hi + 8.0), hi + 1.0)
    # every result of a value inside the range is inside
    rng = np.random.default_rng(1)
    for x, r in zip(rng.uniform(lo, hi, 300), rng.uniform(-30, 30, 300)):
        assert lo <= one(x, r) <= hi


def test_nan_inf_and_huge_quotients_leave_the_value():
    for lim in (False, True):
        one = lambda x, r: uw.unwind_value(np.float64(x), np.float64(r), lim, np.float64(-9.5), np.float64(9.5))
        for x, r in ((np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (-np.inf, 0.0), (0.0, np.inf), (np.inf, np.inf), (0.0, 1e7), (1e300, -1e300)):
            assert uw.same_bits(one(x, r), x), (x, r)
    assert uw.unwind_value(np.float64(0.0), np.float64(6.2e6), False, 0.0, 0.0) != 0.0      # (|quotient| just below 1e6 still moves)


@pytest.mark.parametrize("name", ["turns", "ur5e"])
def test_rows_other_entries_are_bit_copies(name):
    m = uc.turns_model() if name == "turns" else oc.model("ur5e")
    rows, q_ref = uc.designed_rows(m)
    out = uw.unwind(m, rows, q_ref, 64)
    moved = [e[0] for e in uw.eligible(m)]
    rest = [k for k in range(m.nq) if k not in moved]
    assert uw.same_bits(out[:, rest], rows[:, rest])                           # slide, ball, free, the short hinge / the elbow: bits (NaN rows too)
    assert len(rest) == (13 if name == "turns" else 1)
    assert uw.same_bits(uw.unwind(m, out, q_ref, 64), out)                     # idempotent on every designed row
    changed = ~(out.view(np.int64) == rows.view(np.int64))
    assert changed[:, moved].any() and not changed[:, rest].any()
    for qa, limited, lo, hi in uw.eligible(m):
        inside = (rows[:, qa] >= lo) & (rows[:, qa] <= hi) if limited else np.isfinite(rows[:, qa])
        if limited:
            assert ((out[inside, qa] >= lo) & (out[inside, qa] <= hi)).all()
        k = (out[inside, qa] - rows[inside, qa]) / float(T2)
        assert np.abs(k - np.rint(k)).max() < 1e-9                             # whole turns: the pose moves by rounding only


# ------------------------------------------------------------------ 2. the composed rule, on synthetic rungs
def _synthetic_rungs(m, B, T, S, seed, turns=False):
    """Loop results as a ladder sees them: per rung a few branches (random configurations) with small scatter, some untracked,
    one rung nobody tracked; with `turns` every candidate additionally on a random turn of the UR5e's long-range joints."""
    rng = np.random.default_rng(seed)
    lo, hi = np.maximum(m.jnt_range[:, 0], -np.pi), np.minimum(m.jnt_range[:, 1], np.pi)
    q = rng.uniform(lo, hi, size=(B, m.nq)) * 0.3
    branches = rng.uniform(lo, hi, size=(B, T, 3, m.nq))
    pick = rng.integers(0, 3, size=(B, T, S))
    q_all = np.take_along_axis(branches, pick[..., None], axis=2) + 1e-3 * rng.normal(size=(B, T, S, m.nq))
    if turns:
        for qa, _, jlo, jhi in uw.eligible(m):
            shift = rng.integers(-1, 2, size=(B, T, S)) * float(T2)
            moved = q_all[..., qa] + shift
            q_all[..., qa] = np.where((moved >= jlo) & (moved <= jhi), moved, q_all[..., qa])
    trk = rng.uniform(size=(B, T, S)) < 0.8
    if T > 1:
        trk[0, 1] = False
    return q, q_all, trk


def test_nodes_are_a_subset_and_the_key_is_never_smaller():
    m = oc.model("ur5e")
    B, T, S, K = 3, 4, 8, 2
    q, q_all, trk = _synthetic_rungs(m, B, T, S, seed=5)
    gate = 4.0
    plain = ladder_ref.select(m, q, q_all, trk, None, gate)
    nodes, path, chosen = lnref.solve(m, q, q_all, trk, K, 0.1, None, gate)
    np.testing.assert_array_equal(path["n_tracked"], plain["n_tracked"])        # a rung holds a tracked node iff a tracked candidate
    assert plain["n_tracked"][0] == T - 1
    for b in range(B):
        key_n = (T - path["n_tracked"][b], path["n_breaks"][b], path["path_length"][b])
        key_p = (T - plain["n_tracked"][b], plain["n_breaks"][b], plain["path_length"][b])
        assert key_n >= key_p, (b, key_n, key_p)
    # the set rule's bookkeeping: covered + uncovered = eligible, nodes are candidates, empty slots repeat candidate 0
    np.testing.assert_array_equal(nodes.multiplicity.sum(axis=2) + nodes.n_uncovered, nodes.n_converged)
    np.testing.assert_array_equal(nodes.n_converged, trk.sum(axis=2))
    np.testing.assert_array_equal(nodes.tracked.sum(axis=2), nodes.n_distinct)
    assert (nodes.n_uncovered > 0).any() and (nodes.n_distinct[0, 1] == 0)
    for b in range(B):
        for t in range(T):
            for j in range(K):
                s = nodes.seed_index[b, t, j]
                assert (s >= 0) == bool(nodes.tracked[b, t, j]) == (j < nodes.n_distinct[b, t])
                assert uw.same_bits(nodes.q[b, t, j], q_all[b, t, max(s, 0)]) and (s < 0 or trk[b, t, s])
    np.testing.assert_array_equal(chosen >= 0, np.take_along_axis(nodes.tracked, path["node_index"][..., None], axis=2)[..., 0])


def test_enough_nodes_and_no_radius_is_the_plain_ladder():
    m = oc.model("ur5e")
    B, T, S = 3, 4, 6
    q, q_all, trk = _synthetic_rungs(m, B, T, S, seed=6)
    for gate in (np.inf, 4.0):
        plain = ladder_ref.select(m, q, q_all, trk, None, gate)
        nodes, path, chosen = lnref.solve(m, q, q_all, trk, S + 2, 0.0, None, gate)
        np.testing.assert_array_equal(nodes.n_distinct, trk.sum(axis=2))        # every tracked candidate is a node
        assert (nodes.n_uncovered == 0).all()
        np.testing.assert_array_equal(path["n_tracked"], plain["n_tracked"])
        # where every rung holds a tracked candidate the paths are the same; on the rung nobody tracked (instance 0) the plain
        # ladder chooses among S untracked rows, the nodes hold candidate 0's only: the key may be larger there, never smaller
        full = plain["n_tracked"] == T
        assert full.tolist() == [False, True, True]
        for f in ("n_breaks", "path_length", "q_path"):
            np.testing.assert_array_equal(path[f][full], plain[f][full], err_msg=f)
        np.testing.assert_array_equal(chosen[full], plain["node_index"][full])
        assert (path["n_breaks"][0], path["path_length"][0]) >= (plain["n_breaks"][0], plain["path_length"][0])
        assert (chosen[0] < 0).tolist() == [False, True, False, False]


def test_unwinding_frees_slots():
    """Candidates of three branches spread over turns: raw, a rung holds up to 3 · (turns) distinct nodes; unwound toward q, 3."""
    m = oc.model("ur5e")
    B, T, S, K = 2, 3, 16, 4
    q, q_all, trk = _synthetic_rungs(m, B, T, S, seed=7, turns=True)
    trk[:] = True
    raw = lnref.nodes(m, q, q_all, trk, K, 0.1)
    unw = lnref.nodes(m, q, q_all, trk, K, 0.1, unwind=True)
    # (a branch that lies half a turn from the reference in some joint may come out on both sides of it: 3 or 4 nodes here)
    assert unw.n_uncovered.sum() < raw.n_uncovered.sum() and (unw.n_uncovered == 0).all() and (unw.n_distinct >= 3).all()
    assert (raw.n_distinct == K).all() and (raw.n_uncovered > 0).all()
    assert uw.same_bits(unw.candidates, uw.unwind(m, q_all.reshape(-1, m.nq), q, T * S).reshape(q_all.shape))
    np.testing.assert_array_equal(unw.n_converged, raw.n_converged)             # the flags are carried over


# ------------------------------------------------------------------ 3. argument validation without a device
def test_argument_validation_needs_no_gpu():
    import mink_amd
    from mink_amd import _native as nat

    m = oc.model("ur5e")
    B, T, S = 4, 3, 5
    cfg = mink_amd.Configuration(m, np.tile(np.asarray(m.qpos0), (B, 1)))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    poses = np.zeros((B, T, 7)); poses[..., 0] = 1.0
    ladder = lambda **kw: mink_amd.solve_ik_trajectory_ladder(
        cfg, [task], 1.0, {task: poses}, **{**dict(n_seeds=S, max_iters=10, pos_threshold=1e-4, ori_threshold=1e-4, n_nodes=2), **kw})
    with pytest.raises(ValueError, match="pass n_nodes"):
        ladder(n_nodes=None, unwind_turns=True)
    for K in (0, 65, -1):
        with pytest.raises(ValueError, match="n_solutions"):
            ladder(n_nodes=K)
    with pytest.raises(ValueError, match="must be an integer"):
        ladder(n_nodes="many")
    for r in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_distance"):
            ladder(min_distance=r)
    with pytest.raises(ValueError, match="candidates per target"):
        ladder(n_seeds=4097, max_instances=1 << 30)
    with pytest.raises(ValueError, match="at most 256"):                        # without n_nodes the search's limit stands
        ladder(n_seeds=320, n_nodes=None)
    with pytest.raises(ValueError, match="at least one"):
        ladder(n_seeds=0)
    with pytest.raises(ValueError, match="max_step must be >= 0"):
        ladder(max_step=-1.0)
    with pytest.raises(ValueError, match="at most 65535"):
        mink_amd.solve_ik_trajectory_ladder(cfg, [task], 1.0, {task: np.broadcast_to(poses[:1, :1], (B, 65536, 7))}, n_seeds=1,
                                            n_nodes=1, max_iters=10, pos_threshold=1e-4, ori_threshold=1e-4)
    # the limits on the host, by themselves: 320 candidates into 4 nodes pass, the set's limits hold
    nat.check_ladder_nodes_shape(320, 4, 3, float("inf"), 0.1)
    nat.check_ladder_nodes_shape(4096, 64, 65535, 0.0, 0.0)
    for bad in ((4097, 4, 3, 1.0, 0.1), (8, 65, 3, 1.0, 0.1), (8, 0, 3, 1.0, 0.1), (0, 1, 3, 1.0, 0.1), (8, 4, 0, 1.0, 0.1),
                (8, 4, 65536, 1.0, 0.1), (8, 4, 3, -1.0, 0.1), (8, 4, 3, 1.0, -0.1), (8, 4, 3, 1.0, float("inf"))):
        with pytest.raises(ValueError):
            nat.check_ladder_nodes_shape(*bad)

    for bad in (np.zeros(m.nq), np.zeros((5, m.nq + 1)), np.zeros((3, 5, m.nq)), np.zeros((4, 0, m.nq)), None):
        with pytest.raises(ValueError, match="q_rows must have shape"):
            mink_amd.unwind_turns(cfg, bad)
    with pytest.raises(ValueError, match="reference must have shape"):
        mink_amd.unwind_turns(cfg, np.zeros((5, m.nq)), reference=np.zeros((3, m.nq)))

    import inspect
    for f in (mink_amd.solve_ik_solutions, mink_amd.distinct_solutions, mink_amd.solve_ik_trajectory_ladder):
        assert inspect.signature(f).parameters["unwind_turns"].default is False, f
    sig = inspect.signature(mink_amd.solve_ik_trajectory_ladder).parameters
    assert sig["n_nodes"].default is None and sig["min_distance"].default == 0.1
    for name in ("unwind_turns", "LadderNodesResult", "RefinedLadderNodesResult"):
        assert name in mink_amd.__all__ and hasattr(mink_amd, name), name
    own = ("node_seed_index", "node_multiplicity", "node_distance", "n_distinct", "n_converged", "n_uncovered", "seed_index")
    assert mink_amd.LadderNodesResult._fields == mink_amd.LadderResult._fields + own
    assert mink_amd.RefinedLadderNodesResult._fields == mink_amd.RefinedLadderResult._fields + own
    assert nat.TrajectoryLadderNodesOut._fields == nat.TrajectoryLadderOut._fields + own
    assert mink_amd.LadderResult._fields[-1] == "seeds" and mink_amd.RefinedLadderResult._fields[-1] == "refined"   # they did not grow


# ------------------------------------------------------------------ 4. the ABI
NEW_FUNCTIONS = ("mkh_unwind_turns", "mkh_solve_trajectory_ladder_nodes")
NEW_KERNELS = ("unwind_turns_kernel", "ladder_nodes_flags_kernel")


def test_entry_points_are_declared_bound_and_documented():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "minkhip.h")).read()
    for f in NEW_FUNCTIONS:
        assert f in nat.EXPORTED_SYMBOLS, f
        assert getattr(L, f).restype is ctypes.c_int32
        assert re.search(r"^int32_t " + f + r"\(", hdr, re.M), f
    assert re.search(r"^#define MKH_FLAG_UNWIND_TURNS 1024\b", hdr, re.M) and nat.FLAG_UNWIND_TURNS == 1024
    flags = [int(v) for v in re.findall(r"^#define MKH_FLAG_\w+ (\d+)", hdr, re.M)]
    assert sorted(flags) == [1 << k for k in range(11)]                  # the next free bit, no bit twice
    assert ctypes.sizeof(nat.MkhLadderNodesIO) == 7 * ctypes.sizeof(ctypes.c_void_p)
    fields = hdr.split("typedef struct MkhLadderNodesIO {")[1].split("} MkhLadderNodesIO;")[0]
    assert tuple(re.findall(r"\*(\w+);", fields)) == nat.LADDER_NODES_IO_FIELDS              # same order as the ctypes mirror
    for word in ("THE RULE OF THE UNWINDING", "TWO_PI = 6.283185307179586", "rounding half to even", "idempotent, bitwise",
                 "stays inside", "CARRIED OVER", "MODULO THE UNWINDING", "1 <= n_nodes <= 64", "tracked iff j < n_distinct",
                 "Nothing the call allocates is\n * sized B·T·S"):
        assert word in hdr, word
    # null / bad arguments fail loudly before any device is touched
    assert L.mkh_unwind_turns(None, 1, 1, None, None, None, 0, None) == -1
    assert b"null problem" in L.mkh_last_error()
    io, nio = nat.MkhTrajectoryLadderIO(), nat.MkhLadderNodesIO()
    assert L.mkh_solve_trajectory_ladder_nodes(None, 1, 1, 4, 2, 0.1, None, None, None, None, 1.0, 1e-3, 10, 1e-4, 1e-4, 0, 0,
                                               ctypes.byref(io), ctypes.byref(nio), None, 0, None) == -1
    assert b"null problem" in L.mkh_last_error()


def test_new_kernels_keep_their_vector_registers():
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    with open(os.path.join(GOLDEN, "spill_budget.json")) as fh:
        budget = json.load(fh)
    for k in NEW_KERNELS:
        e = table.get(k)
        assert e is not None, (k, sorted(x for x in table if "unwind" in x or "nodes" in x))
        assert e["vgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0 and e["callees"] == {}, (k, e)
        assert k not in budget
