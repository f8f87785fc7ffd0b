"""The plain solve's four routes (mink_amd/csrc/solve_plan.h solve_route) hold the same rows: device pointers, the pinned scratch of
a small host call, staged copies — with the taps and the warm-start state that travel with them — and the refusals of its entry
points through the ABI, each message typed from the source as it stood before the host path was split into solve_host.hip.

Sizes, G1 config 3 (nq 44, nv 43, four frame tasks, 67 task rows, 45 bodies): a row of inputs and outputs is 924 bytes, a row of all
fourteen taps 42 852 more.  So 96 rows are staged with or without taps; one row with every tap (44 KB) and sixteen rows with the
light taps (2 336 bytes each) are below the scratch's 64 KB and go through it; 48 rows with every tap are staged again."""

import ctypes as C

import numpy as np
import pytest

import native_configs as nc

pytestmark = pytest.mark.gpu

ALL_TAPS = ["xpos", "xquat", "frame_pose", "subtree_com", "task_e", "task_J", "H", "c", "box_lo", "box_hi", "coll_G", "coll_h", "qp_iters",
            "cycles"]
LIGHT_TAPS = ["frame_pose", "subtree_com", "c", "box_lo", "box_hi", "qp_iters", "cycles"]


@pytest.fixture(scope="module")
def g1_rows():
    from mink_amd import _native as nat, workloads
    import mink_amd as mink
    g1 = mink.load_robot("g1")
    nm = nat.NativeModel(g1)
    B = 96
    prob, dt, damping = nc.build("g1_c3", nm, B)
    base = g1.key_qpos[g1.name2id("key", "stand")]
    q, tg = workloads.make_batch(g1, nm, prob, np.random.default_rng(12), B, base_q=base)
    return g1, nm, prob, dt, damping, q, tg, base[None, :]


def _same(got, want, rows, names, what):
    for n in names:
        np.testing.assert_array_equal(got[n], want[n][rows], err_msg=f"{what}: {n}")


@pytest.mark.parametrize("solve_qp", [False, True])
def test_taps_equal_across_the_routes(g1_rows, solve_qp):
    """Every tap, v and status, bitwise and row for row: 96 rows staged; rows [0, 48) with every tap (staged as well: 2 MB); row 7
    with every tap and rows [40, 56) with the light ones through the pinned scratch, where the layout's tap blocks lie behind the
    inputs, v and the int32 block (no v block when solve_qp is off); the 96 rows on device tensors.
    Two taps are not compared everywhere, for what they hold: `cycles` is shader-clock stamps, different at every run (it is asked for
    so that its block is part of the layout); `qp_iters` is written by the QP alone, so an evaluation leaves it as it came — zeroed by
    the host routes, the caller's own uninitialised tensor on the device route."""
    torch = pytest.importorskip("torch")
    g1, nm, prob, dt, damping, q, tg, pt = g1_rows
    compared = [n for n in ALL_TAPS if n != "cycles"]

    def call(rows, taps, to=lambda x: x):
        out = prob.solve(to(q[rows]), to(tg[rows]), to(pt), None, dt, damping, taps=taps, solve_qp=solve_qp)
        get = lambda x: None if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy())
        d = {n: get(out[2][n]) for n in taps}
        d["v"], d["status"] = get(out[0]), get(out[1])
        return d

    full = slice(0, 96)
    big = call(full, ALL_TAPS)
    assert big["cycles"].shape == (96, 16) and big["H"].shape == (96, g1.nv, g1.nv)
    if solve_qp:
        assert (big["status"] == 0).all() and np.abs(big["v"]).max() > 0 and (big["qp_iters"] >= 0).all()
    else:
        assert big["v"] is None and big["status"] is None and (big["qp_iters"] == 0).all()
    assert np.abs(big["H"]).max() > 0 and np.abs(big["task_J"]).max() > 0
    outs = ["v", "status"] if solve_qp else []
    for rows, taps in ((slice(0, 48), ALL_TAPS), (slice(7, 8), ALL_TAPS), (slice(40, 56), LIGHT_TAPS)):
        small = call(rows, taps)
        _same(small, big, rows, [n for n in taps if n != "cycles"] + outs, f"host rows {rows}")
    dev = torch.device("cuda", 0)
    on_dev = call(full, ALL_TAPS, to=lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev))
    torch.cuda.synchronize()
    _same(on_dev, big, full, [n for n in compared if solve_qp or n != "qp_iters"] + outs, "device rows")


def test_warm_start_equal_across_the_routes(g1_rows):
    """Consecutive warm-started solves on one handle per route — 96 rows staged, rows 0–7 through the pinned scratch, 96 rows on
    device tensors: v, status and the pivot counts of every call are the same rows, bitwise.  Three calls: the state a call leaves is
    read from the third on (mkh_types.h SolveArgs::warm)."""
    torch = pytest.importorskip("torch")
    g1, nm, _, dt, damping, q, tg, pt = g1_rows
    dev = torch.device("cuda", 0)
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    np_ = lambda x: x if isinstance(x, np.ndarray) else x.cpu().numpy()

    def three(B, conv):
        prob = nc.build("g1_c3", nm, 96)[0]
        res = []
        for k in range(3):
            v, st, taps = prob.solve(conv(q[:B]), conv(tg[:B]), conv(pt), None, dt, damping, taps=["qp_iters"], warm_start=True)
            res.append((np_(v), np_(st), np_(taps["qp_iters"])))
        return res

    staged, pinned, device = three(96, lambda x: x), three(8, lambda x: x), three(96, to)
    torch.cuda.synchronize()
    for k in range(3):
        for a, b, c in zip(staged[k], pinned[k], device[k]):
            np.testing.assert_array_equal(b, a[:8])
            np.testing.assert_array_equal(c, a)
    assert (staged[2][1] == 0).all()


# ------------------------------------------------------------------ refusals through the ABI
def _refused(call, text):
    from mink_amd import _native as nat
    rc = call()
    assert rc == -1, rc                                                                    # MKH_E_INVALID
    assert nat.lib().mkh_last_error().decode() == text


def test_refusals_of_the_plain_solve_entry_points(g1_rows):
    """Every message of solve_refusal with its code, on live handles, in front of any work: typed from run() of minkhip.hip as the
    parent commit had it."""
    from mink_amd import _native as nat, workloads
    import mink_amd as mink
    g1, nm, prob, dt, damping, q, tg, pt = g1_rows
    L = nat.lib()
    P = lambda x: None if x is None else x.ctypes.data
    B = 4
    q4, tg4, pt4 = np.ascontiguousarray(q[:B]), np.ascontiguousarray(tg[:B]), np.ascontiguousarray(pt)
    v, st = np.zeros((B, g1.nv)), np.zeros(B, dtype=np.int32)
    qo, it, cv = np.zeros((B, g1.nq)), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    h = prob.handle

    def solve(B=B, q=q4, ft=tg4, pt=pt4, ct=None, dt=dt, flags=0, handle=h):
        return lambda: L.mkh_solve(handle, B, P(q), P(ft), P(pt), P(ct), dt, damping, P(v), P(st), flags, None)

    _refused(solve(B=0), "B must be >= 1")
    _refused(solve(flags=nat.FLAG_UNWIND_TURNS),
             "a solve: MKH_FLAG_UNWIND_TURNS is honoured by mkh_solve_multistart_set and mkh_solve_trajectory_ladder_nodes only")
    _refused(solve(q=None), "q is null")
    _refused(solve(ft=None), "frame_targets is null (TargetNotSet)")
    _refused(solve(pt=None), "posture_target is null (TargetNotSet)")
    _refused(solve(dt=0.0), "dt must be > 0")
    _refused(solve(dt=float("nan")), "dt must be > 0")
    _refused(lambda: L.mkh_solve_steps(h, B, P(q4), P(tg4), P(pt4), None, dt, damping, 0, P(qo), P(v), P(st), 0, None), "n_steps must be >= 1")
    _refused(solve(B=97, q=np.zeros((97, g1.nq)), ft=np.zeros((97, 4, 7))), "B=97 exceeds max_batch=96 of this problem")
    # the order: B before the unwind flag before q before the targets before dt before n_steps before max_batch
    _refused(solve(B=0, q=None, dt=0.0, flags=nat.FLAG_UNWIND_TURNS), "B must be >= 1")
    _refused(solve(q=None, ft=None, dt=0.0), "q is null")
    _refused(lambda: L.mkh_solve_steps(h, 97, P(q4), P(tg4), P(pt4), None, 0.0, damping, 0, P(qo), P(v), P(st), 0, None), "dt must be > 0")
    _refused(lambda: L.mkh_solve_steps(h, 97, P(q4), P(tg4), P(pt4), None, dt, damping, 0, P(qo), P(v), P(st), 0, None), "n_steps must be >= 1")
    # a COM task's target
    full = nc.build("g1_full", nm, B)[0]
    tg5 = np.zeros((B, 5, 7)); tg5[:, :, 0] = 1.0
    _refused(solve(ft=tg5, ct=None, handle=full.handle), "com_target is null (TargetNotSet)")
    # dense (plugin) rows: a UR5e problem with three task rows, two limit rows and box rows, and one with none of them
    ur = mink.load_robot("ur5e")
    um = nat.NativeModel(ur)
    plain = nc.build("ur5e_c2", um, B)[0]
    ft_of = plain.n_frame
    dense_p = nat.NativeProblem(um, frame_tasks=[nc._ft(ur, "attachment_site", "site", 1.0, 1.0, 1.0)], configuration_limits=[nc._cfg_limit(ur)],
                                max_batch=B, dense_tasks=[{"cost": [1.0, 1.0, 1.0], "gain": 1.0}], dense_limit_rows=2, dense_limit_box=True)
    uq = np.tile(ur.key_qpos[0], (B, 1))
    uft = np.zeros((B, 1, 7)); uft[:, :, 0] = 1.0
    upt = np.ascontiguousarray(ur.key_qpos[0][None, :])
    uv = np.zeros((B, ur.nv))
    e, J, G, hh, lo = np.zeros((B, 3)), np.zeros((B, 3, ur.nv)), np.zeros((B, 2, ur.nv)), np.ones((B, 2)), -np.ones((B, ur.nv))

    def dense_call(handle, rows, ft=uft, pt=None):
        dr = nat.MkhDenseRows()
        for name, x in rows.items():
            setattr(dr, name, x.ctypes.data)
        return lambda: L.mkh_solve_dense(handle, B, P(uq), P(ft), P(pt), None, C.byref(dr), dt, damping, P(uv), P(st), None, 0, None)

    uft_plain = np.zeros((B, ft_of, 7)); uft_plain[:, :, 0] = 1.0
    _refused(dense_call(plain.handle, {"limit_lo": lo}, ft=uft_plain, pt=upt if plain.n_posture else None),
             "limit_lo / limit_hi need a problem created with dense_limit_box = 1")
    dh = dense_p.handle
    _refused(lambda: L.mkh_solve(dh, B, P(uq), P(uft), None, None, dt, damping, P(uv), P(st), 0, None),
             "this problem has dense (plugin) rows: call mkh_solve_dense")
    _refused(dense_call(dh, {"task_e": e, "limit_G": G, "limit_h": hh}), "dense task_e / task_J is null")
    _refused(dense_call(dh, {"task_e": e, "task_J": J, "limit_G": G}), "dense limit_G / limit_h is null")
    # ("... no fused steps" needs dense rows AND steps: no entry point passes both — mkh_solve_steps is refused one test earlier)
    uqo = uq.copy()
    _refused(lambda: L.mkh_solve_steps(dh, B, P(uq), P(uft), None, None, dt, damping, 2, P(uqo), P(uv), P(st), 0, None),
             "this problem has dense (plugin) rows: call mkh_solve_dense")
    # ... and the entry points' own: outputs and thresholds
    _refused(lambda: L.mkh_solve(h, B, P(q4), P(tg4), P(pt4), None, dt, damping, None, P(st), 0, None), "v_out is null")
    _refused(lambda: L.mkh_solve_steps(h, B, P(q4), P(tg4), P(pt4), None, dt, damping, 2, None, P(v), P(st), 0, None), "v_out / q_out is null")
    _refused(lambda: L.mkh_solve_until(h, B, P(q4), P(tg4), P(pt4), None, dt, damping, 4, -1.0, 1e-2, P(qo), P(v), P(st), P(it), P(cv), 0, None),
             "thresholds must be >= 0")
    _refused(lambda: L.mkh_solve(None, B, P(q4), P(tg4), P(pt4), None, dt, damping, P(v), P(st), 0, None), "null problem")
    # a served call after all of them: the handle is as it was
    assert solve()() == 0 and (st == 0).all()
    np.testing.assert_array_equal(v, prob.solve(q4, tg4, pt4, None, dt, damping)[0])


def test_refused_threshold_loop_leaves_the_warm_start_state_alone(g1_rows):
    """mkh_solve_until on a handle without frame tasks is refused before the warm-start state is touched: warm-started solves around
    the refused call (of another batch size, which would reset the state of a served call) give what a fresh handle's give."""
    from mink_amd import _native as nat
    g1, nm, _, dt, damping, q, _, pt = g1_rows

    def handle():
        return nat.NativeProblem(nm, posture_tasks=[{"cost": 1.0}], configuration_limits=[nc._cfg_limit(g1)],
                                 velocity_limits=[nc._vel_limit(g1)], max_batch=8)

    def solves(prob, ks):
        out = []
        for k in ks:
            v, st, taps = prob.solve(q[:8] + 0.05 * k, None, pt + 0.3, None, dt, damping, taps=["qp_iters"], warm_start=True)
            out.append((v, st, taps["qp_iters"]))
        return out

    fresh = solves(handle(), range(4))
    prob = handle()
    got = solves(prob, range(3))
    with pytest.raises(nat.MinkHipError, match="^libminkhip error -1: mkh_solve_until needs at least one frame task to test the thresholds on$"):
        prob.solve(q[:4], None, pt, None, dt, damping, n_steps=4, until=(1e-3, 1e-2), warm_start=True)
    got += solves(prob, [3])
    for a, b in zip(got, fresh):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
