"""Lists of limits and two posture tasks on every kernel family, against the numpy oracle with the stacked list.

The reference stacks whatever `limits=[...]` holds (mink/solve_ik.py:25-40); the device folds up to four ConfigurationLimits and four
VelocityLimits per dof in a loop over its own copy of the tables — lane tables (wavefront kernels), LaneProblem / LaneProblem2 (lane
and row kernels), plain arrays (workgroup-per-problem kernel).  tests/limit_lists.py defines one list of eight terms and the inputs
per model, and checks from the oracle alone that every term after the first binds somewhere and matters there (the witness
condition), so that a kernel which ignores a term, reads it at a wrong stride or starts it from a wrong default cannot pass.

Per family and (cfg, vel) count: v against the oracle at the project's 1e-8·max(1, |v_ref|inf); status equal to the oracle's outcome
per instance (MKH_ST_INFEASIBLE with v = NaN exactly where its QP raises "constraints are inconsistent", MKH_ST_OUTSIDE_LIMITS by the
model's range, not by the tightened terms); the box taps of the wavefront / wide kernels exact on hinge and slide dofs (both sides
compute gain·(bound − q) and dt·v in float64 without a fused step) and to 1e-13 on ball dofs (tests/test_gpu_golden.py's bound
for balllimit's rows); and order invariance — the list reversed, rotated by one and by two, and its velocity terms folded on the host
into one term of per-dof minima all give bitwise the same v on the same kernel (fmin / fmax commute): the check that bites on the row and lane
builds, which have no taps.

What the inputs can and cannot be made to do (tests/limit_lists.py has the reasoning): velocity terms alone always admit the zero
step and configuration terms alone would need a band within 5 % of a range end to contradict each other, so the (3, 0) and (0, 3)
lists have no infeasible instance — there the test asserts that the oracle solves every one; cfg3 is cfg0 row for row, so its
witness drops the pair; one limited dof is kept out of cfg1 and cfg2 so that cfg0 and cfg3 bind at all; and `balllimit` is the
fixture's model with 32 instances sampled like every other family's (the fixture's own 16 meet none of the conditions), its
limited ball joint in cfg0 and cfg1 with the joint's range in its slots, where the lower gain makes cfg1 the tighter term.

Measured on an MI355X, worst relative error against the oracle over the four counts (every figure far below the 1e-8 bound):

  UR5e      ik_quad_kernel 1.1e-14, ik_lane_kernel_6 9.6e-15, ik_solve_kernel_8_0 8.3e-15; three fused steps on
            ik_quad_kernel_loop and ik_solve_kernel_8_16 2.2e-14
  LEAP      ik_quad_kernel_16 5.0e-14; ik_quad_kernel_16_loop 1.8e-13
  H1        ik_quad_kernel_32 2.6e-14; ik_quad_kernel_32_loop 9.4e-13, ik_solve_kernel_32_48_r32_w3 (loop) 2.7e-13
  G1        ik_solve_kernel_44_32_r44_w3o (dispatch's pick at B = 70) and ik_solve_kernel_44_32_r44 (two waves) 2.0e-14,
            ik_solve_kernel_44_0_w3 (direct start) 9.1e-15; _w3o from 10 752 and _w4o from 32 805 instances 1.9e-14
  balllimit ik_solve_kernel_8_0 6.0e-14          chain70  ik_wide_kernel 6.2e-14
  plugin    ik_solve_kernel_8_256 2.4e-15        two collision limits  ik_solve_kernel_16_8+wide 8.4e-14
  six VelocityLimits through solve_ik 8.5e-15

The box taps were exact on every hinge and slide dof and every order of the list gave bitwise the same v on every kernel.  One
defect came out while the ball joint's terms were designed: the kernels rebuild a ball joint's bound as (u, u, u, u) from the one
value its dofs' table entries hold, so a descriptor with a quaternion of its own in the joint's four slots of lower / upper was
evaluated as something else (every instance infeasible where the oracle solved all); problem creation now refuses it.  The (4, 4) list, from the oracle — infeasible instances, then bounds active at the solution per term
(cfg0 … cfg3, vel0 … vel3): UR5e 3 of 67, 34 / 59 / 42 / 34, 88 / 128 / 32 / 60; LEAP 3 of 35, 30 / 26 / 13 / 30, 171 / 64 / 167 / 31;
H1 3 of 35, 17 / 21 / 18 / 17, 208 / 64 / 208 / 31; G1 3 of the 20 sampled, 9 / 13 / 8 / 9, 202 / 34 / 74 / 13; chain70 3 of 12,
29 / 7 / 5 / 29, 274 / 18 / 272 / 9; balllimit 3 of 32, 38 / 51 / 14 / 38, 84 / 58 / 18 / 20.
"""

import os

import numpy as np
import pytest

import limit_lists as ll
import native_configs as nc
import oracle_configs as oc
from oracle import ik as oik
from oracle import qp_gi

pytestmark = pytest.mark.gpu

TWIN, W4 = "ik_solve_kernel_44_32_r44_w3o", "ik_solve_kernel_44_32_r44_w4o"
B_TWIN, B_W4 = 10752, 32768 + 37        # tests/test_gpu_headline_paths.py, tests/test_gpu_w4_headline.py: the smallest batches that select them


_models = {}


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    yield _native
    for nm in _models.values():
        nm.close()
    _models.clear()


def _nmodel(nat, family):
    if family not in _models:
        _models[family] = nat.NativeModel(ll.model_of(family))
    return _models[family]


def _problem(nat, family, cfg, vel, max_batch, **extra):
    c = ll.case(family)
    fts, posts = ll.native_tasks(c)
    return nat.NativeProblem(_nmodel(nat, family), frame_tasks=fts, posture_tasks=posts, configuration_limits=[d for _, _, d in cfg],
                             velocity_limits=[d for _, _, d in vel], max_batch=max_batch, **extra)


def _solve(prob, c, rows=slice(None), **kw):
    return prob.solve(c.q[rows], c.tg[rows], c.pt[rows], None, c.dt, c.damping, **kw)


def _rel(v, ref):
    return np.abs(v - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))


def _against_oracle(c, r, v, st, label):
    """v and status of one launch against the reference of its sampled rows; statuses of the other rows at least consistent."""
    inf = (r.st & ll.ST_INFEASIBLE) != 0
    assert np.array_equal(st[r.rows], r.st), (label, st[r.rows].tolist(), r.st.tolist())
    assert np.isnan(v[r.rows][inf]).all() and not np.isnan(v[r.rows][~inf]).any(), label
    assert ((st & ~3) == 0).all() and np.array_equal(np.isnan(v).any(axis=1), (st & ll.ST_INFEASIBLE) != 0), (label, np.unique(st))
    err = _rel(v[r.rows][~inf], r.v[~inf])
    print("%s: max rel err vs oracle %.2e on %d instances, %d infeasible" % (label, err.max(), int((~inf).sum()), int(inf.sum())))
    assert err.max() <= 1e-8, (label, err.max(), int(np.asarray(r.rows)[~inf][err.argmax()]))
    return float(err.max())


def _same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


@pytest.fixture
def handles(nat):
    """problem(family, cfg terms, vel terms, max_batch, ...) -> NativeProblem, closed when the test ends."""
    made = []

    def problem(family, cfg, vel, max_batch, **extra):
        made.append(_problem(nat, family, cfg, vel, max_batch, **extra))
        return made[-1]

    yield problem
    for prob in made:
        prob.close()


def _orders(problem, family, n_cfg, n_vel, B):
    """The list as given, reversed, rotated by one and by two (with four terms every slot, the last one too, then holds in some
    order a term that is no copy of another), and with the velocity terms folded into one: [(label, problem)]."""
    c = ll.case(family)
    cfg, vel = c.cfg[:n_cfg], c.vel[:n_vel]
    out = [("as given", problem(family, cfg, vel, B)), ("reversed", problem(family, cfg[::-1], vel[::-1], B)),
           ("rotated", problem(family, cfg[1:] + cfg[:1], vel[1:] + vel[:1], B))]
    if max(n_cfg, n_vel) > 2:
        out.append(("rotated by two", problem(family, cfg[2:] + cfg[:2], vel[2:] + vel[:2], B)))
    if n_vel > 1:
        out.append(("velocity terms folded", problem(family, cfg, [("fold", None, ll.folded_velocity(c.m, vel))], B)))
    return out


def _box_taps(c, r, prob, label, kernels, **kw):
    """box_lo / box_hi against the oracle's rows reduced per dof: exact on hinge / slide dofs, 1e-13 on ball dofs; a dof in no term
    (a free joint's among them) is unbounded."""
    _, _, taps = _solve(prob, c, taps=["box_lo", "box_hi"], **kw)
    assert prob.last_kernel().startswith(kernels), (label, prob.last_kernel())
    _, D, jid = ll.dof_sets(c.m)
    scalar = np.array([c.m.jnt_type[jid[d]] in (2, 3) for d in range(c.m.nv)])
    for name, got, want in (("box_lo", taps["box_lo"][r.rows], r.lo), ("box_hi", taps["box_hi"][r.rows], r.hi)):
        bad = np.argwhere(got[:, scalar] != want[:, scalar])
        assert len(bad) == 0, (label, name, bad[:4].tolist(), got[:, scalar][tuple(bad[0])], want[:, scalar][tuple(bad[0])])
        if (~scalar).any():
            fin = np.isfinite(want[:, ~scalar])
            assert np.array_equal(np.isfinite(got[:, ~scalar]), fin), (label, name)
            assert np.array_equal(got[:, ~scalar][~fin], want[:, ~scalar][~fin])
            assert np.abs(got[:, ~scalar][fin] - want[:, ~scalar][fin]).max(initial=0.0) <= 1e-13, (label, name)
    free = [d for d in range(c.m.nv) if d not in D]
    assert np.isneginf(taps["box_lo"][:, free]).all() and np.isposinf(taps["box_hi"][:, free]).all()


def _figures(family, n_cfg, n_vel):
    fig = ll.check_conditions(family, n_cfg, n_vel)
    print("%s (%d, %d): oracle: %d infeasible, %.1f dofs on a bound per instance, active bounds per term %s" % (
        family, n_cfg, n_vel, fig["infeasible"], fig["on_bound_mean"], fig["active"]))
    return fig


def _oracle_loop(c, i, terms, n_steps):
    """tests/test_gpu_wide.py's loop on the numpy oracle; None where a step is infeasible."""
    from test_gpu_wide import _oracle_loop as loop
    try:
        return loop(c.m, ll.oracle_tasks(c, i), [s for _, s, _ in terms], c.q[i], c.tg[i], c.dt, c.damping, n_steps)[:2]
    except qp_gi.Infeasible:
        return None


def _loop_check(c, prob, terms, kernel, label, **kw):
    """n_steps = 3 in one launch against the callers' loop on the oracle: every fourth instance and the ones built to be infeasible."""
    qK, vK, st = _solve(prob, c, n_steps=3, **kw)
    assert prob.last_kernel() == kernel or (kernel == "ik_solve_kernel" and prob.last_kernel().startswith(kernel)), (label, prob.last_kernel())
    worst, n_inf = 0.0, 0
    for i in sorted(set(range(0, c.B, 4)) | set(c.made_infeasible)):
        ref = _oracle_loop(c, i, terms, 3)
        if ref is None:
            n_inf += 1
            assert st[i] & ll.ST_INFEASIBLE, (label, i, st[i])
            continue
        assert (st[i] & ~1) == 0, (label, i, st[i])
        worst = max(worst, float(np.abs(vK[i] - ref[1]).max() / max(1.0, np.abs(ref[1]).max())))
        np.testing.assert_allclose(qK[i], ref[0], rtol=0, atol=1e-9)
    print("%s on %s: 3 fused steps, max rel err of the last v vs the oracle's loop %.2e (%d infeasible)" % (label, prob.last_kernel(), worst, n_inf))
    assert worst <= 1e-8


# ------------------------------------------------------------------------------------------------------------------ families
@pytest.mark.parametrize("n_cfg,n_vel", ll.COUNTS)
def test_ur5e_row_lane_and_wavefront_kernels(handles, n_cfg, n_vel):
    """UR5e, B = 67 (a ragged last row and wavefront): `ik_quad_kernel` by default, the lane kernel, the wavefront kernel, and
    the fused loops of the row and the wavefront kernel."""
    c, r = ll.case("ur5e"), ll.reference("ur5e", n_cfg, n_vel)
    _figures("ur5e", n_cfg, n_vel)
    terms = ll.terms_of(c, n_cfg, n_vel)
    probs = _orders(handles, "ur5e", n_cfg, n_vel, c.B)
    for flags, kernel in (({}, "ik_quad_kernel"), ({"lane_kernel": True}, "ik_lane_kernel_6"), ({"wave_kernel": True}, "ik_solve_kernel")):
        base = None
        for label, prob in probs:
            out = _solve(prob, c, **flags)
            assert prob.last_kernel() == kernel or (kernel == "ik_solve_kernel" and prob.last_kernel().startswith(kernel)), prob.last_kernel()
            if base is None:
                base = out
                _against_oracle(c, r, out[0], out[1], "ur5e (%d, %d) %s" % (n_cfg, n_vel, prob.last_kernel()))
            else:
                assert _same(out, base), ("ur5e", kernel, label, int(np.flatnonzero((out[0] != base[0]).any(axis=1))[0]))
    _box_taps(c, r, probs[0][1], "ur5e taps", "ik_solve_kernel")
    _loop_check(c, probs[0][1], terms, "ik_quad_kernel_loop", "ur5e (%d, %d)" % (n_cfg, n_vel))
    _loop_check(c, probs[0][1], terms, "ik_solve_kernel", "ur5e (%d, %d) wavefront" % (n_cfg, n_vel), wave_kernel=True)


@pytest.mark.parametrize("n_cfg,n_vel", ll.COUNTS)
def test_leap_hand_sixteen_register_build(handles, n_cfg, n_vel):
    """LEAP hand (16 dofs, four fingertip tasks), B = 35: `ik_quad_kernel_16`."""
    c, r = ll.case("leap"), ll.reference("leap", n_cfg, n_vel)
    _figures("leap", n_cfg, n_vel)
    base = None
    for label, prob in _orders(handles, "leap", n_cfg, n_vel, c.B):
        out = _solve(prob, c)
        assert prob.last_kernel() == "ik_quad_kernel_16", prob.last_kernel()
        if base is None:
            base = out
            _against_oracle(c, r, out[0], out[1], "leap (%d, %d) %s" % (n_cfg, n_vel, prob.last_kernel()))
            _box_taps(c, r, prob, "leap taps", "ik_solve_kernel")
            _loop_check(c, prob, ll.terms_of(c, n_cfg, n_vel), "ik_quad_kernel_16_loop", "leap (%d, %d)" % (n_cfg, n_vel))
        else:
            assert _same(out, base), ("leap", label)


@pytest.mark.parametrize("n_cfg,n_vel", ll.COUNTS)
def test_h1_two_row_build_and_its_loop(handles, n_cfg, n_vel):
    """H1 under its bench task set (feet and wrists), B = 35: `ik_quad_kernel_32` and `ik_quad_kernel_32_loop`; the free
    joint's dofs are in no term and stay unbounded."""
    c, r = ll.case("h1"), ll.reference("h1", n_cfg, n_vel)
    _figures("h1", n_cfg, n_vel)
    probs = _orders(handles, "h1", n_cfg, n_vel, c.B)
    base = None
    for label, prob in probs:
        out = _solve(prob, c)
        assert prob.last_kernel() == "ik_quad_kernel_32", prob.last_kernel()
        if base is None:
            base = out
            _against_oracle(c, r, out[0], out[1], "h1 (%d, %d) %s" % (n_cfg, n_vel, prob.last_kernel()))
        else:
            assert _same(out, base), ("h1", label)
    assert np.isinf(r.lo[:, :6]).all() and np.isinf(r.hi[:, :6]).all()
    _box_taps(c, r, probs[0][1], "h1 taps", "ik_solve_kernel")
    # (a floating base under frame and posture tasks alone loops on the wavefront kernel by default: MKH_FLAG_QUAD_KERNEL, as
    #  tests/test_gpu_two_row_loop.py selects the two-row loop)
    _loop_check(c, probs[0][1], ll.terms_of(c, n_cfg, n_vel), "ik_quad_kernel_32_loop", "h1 (%d, %d)" % (n_cfg, n_vel), quad_kernel=True)
    _loop_check(c, probs[0][1], ll.terms_of(c, n_cfg, n_vel), "ik_solve_kernel", "h1 (%d, %d) wavefront" % (n_cfg, n_vel))


@pytest.mark.parametrize("n_cfg,n_vel", ll.COUNTS)
def test_g1_wavefront_builds(handles, n_cfg, n_vel):
    """G1 under `g1_c3`'s frame tasks, B = 70: the build dispatch picks, the direct QP start and the two-waves map on the same
    instances — each against the oracle on a 16-instance sample (plus the instances built to be infeasible or out of range),
    against each other on the full batch, and each order-invariant."""
    c, r = ll.case("g1"), ll.reference("g1", n_cfg, n_vel)
    _figures("g1", n_cfg, n_vel)
    probs = _orders(handles, "g1", n_cfg, n_vel, c.B)
    seen, outs = [], []
    for flags in ({}, {"direct_qp": True}, {"two_waves": True}):
        base = None
        for label, prob in probs:
            out = _solve(prob, c, **flags)
            assert prob.last_kernel().startswith("ik_solve_kernel_4"), prob.last_kernel()
            if base is None:
                base = out
                seen.append(prob.last_kernel())
                _against_oracle(c, r, out[0], out[1], "g1 (%d, %d) %s" % (n_cfg, n_vel, prob.last_kernel()))
            else:
                assert _same(out, base), ("g1", flags, label)
        outs.append(base)
    print("g1 (%d, %d): builds %s" % (n_cfg, n_vel, seen))
    assert "_r44" in seen[0] and "_r44" not in seen[1], seen             # the low-rank start by default, the direct start on request
    feasible = (outs[0][1] & ll.ST_INFEASIBLE) == 0
    for o in outs[1:]:
        assert np.array_equal(o[1], outs[0][1])
        assert _rel(o[0][feasible], outs[0][0][feasible]).max() <= 1e-8
    _box_taps(c, r, probs[0][1], "g1 taps", "ik_solve_kernel")


def test_g1_headline_builds_from_their_batch_sizes(handles):
    """The one-problem-per-workgroup twin and the four-waves build are only taken from 10 752 and 32 768 instances: the 70
    instances of the (4, 4) list repeated to those sizes (device pointers: a host-pointer call of that size is cut into chunks),
    every copy bitwise what the build gives the first one, and the first 70 against the oracle's sample and the small batch."""
    torch = pytest.importorskip("torch")
    c, r = ll.case("g1"), ll.reference("g1", 4, 4)
    small = handles("g1", c.cfg, c.vel, c.B)
    v0, st0 = _solve(small, c)
    dev = torch.device("cuda", 0)
    for B, kernel in ((B_TWIN, TWIN), (B_W4, W4)):
        prob = handles("g1", c.cfg, c.vel, B)
        rep = -(-B // c.B)
        to = lambda x: torch.from_numpy(np.ascontiguousarray(np.tile(x, (rep,) + (1,) * (x.ndim - 1))[:B])).to(dev)
        v, st = prob.solve(to(c.q), to(c.tg), to(c.pt), None, c.dt, c.damping)
        torch.cuda.synchronize()
        v, st = v.cpu().numpy(), st.cpu().numpy()
        assert prob.last_kernel() == kernel, (B, prob.last_kernel())
        _against_oracle(c, r, v[:c.B], st[:c.B], "g1 (4, 4) %s from B = %d" % (kernel, B))
        full = (B // c.B) * c.B
        assert np.array_equal(v[:full].reshape(-1, c.B, c.m.nv), np.broadcast_to(v[:c.B], (B // c.B, c.B, c.m.nv)), equal_nan=True)
        assert np.array_equal(st[:full].reshape(-1, c.B), np.broadcast_to(st[:c.B], (B // c.B, c.B)))
        assert np.array_equal(v[full:], v[:B - full], equal_nan=True)
        feasible = (st0 & ll.ST_INFEASIBLE) == 0
        assert np.array_equal(st[:c.B], st0) and _rel(v[:c.B][feasible], v0[feasible]).max() <= 1e-8


@pytest.mark.parametrize("n_cfg,n_vel", ll.COUNTS)
def test_limited_ball_joint_in_two_terms(handles, n_cfg, n_vel):
    """`balllimit` (the model of tests/golden/ik_balllimit.npz, inputs sampled like the other families'), B = 32: the limited ball
    joint sits in cfg0 (gain 0.95) and cfg1 (gain 0.5, the tighter of the two; asserted from the oracle in
    tests/test_limit_lists_cpu.py with what dropping it does), its dofs in vel0 and vel2."""
    c, r = ll.case("balllimit"), ll.reference("balllimit", n_cfg, n_vel)
    _figures("balllimit", n_cfg, n_vel)
    base = None
    for label, prob in _orders(handles, "balllimit", n_cfg, n_vel, c.B):
        out = _solve(prob, c)
        assert prob.last_kernel().startswith("ik_solve_kernel"), prob.last_kernel()
        if base is None:
            base = out
            _against_oracle(c, r, out[0], out[1], "balllimit (%d, %d) %s" % (n_cfg, n_vel, prob.last_kernel()))
            _box_taps(c, r, prob, "balllimit taps", "ik_solve_kernel")
        else:
            assert _same(out, base), ("balllimit", label)


@pytest.mark.parametrize("n_cfg,n_vel", ll.COUNTS)
def test_chain_beyond_one_wavefront(handles, n_cfg, n_vel):
    """The 70-dof chain of tests/test_gpu_wide.py, B = 12: `ik_wide_kernel`, plain arrays at stride nv."""
    c, r = ll.case("chain70"), ll.reference("chain70", n_cfg, n_vel)
    _figures("chain70", n_cfg, n_vel)
    base = None
    for label, prob in _orders(handles, "chain70", n_cfg, n_vel, c.B):
        out = _solve(prob, c)
        assert prob.last_kernel() == "ik_wide_kernel", prob.last_kernel()
        if base is None:
            base = out
            _against_oracle(c, r, out[0], out[1], "chain70 (%d, %d) %s" % (n_cfg, n_vel, prob.last_kernel()))
            _box_taps(c, r, prob, "chain70 taps", "ik_wide_kernel")
        else:
            assert _same(out, base), ("chain70", label)


def test_plugin_route_intersects_the_merged_box(handles):
    """The plugin route (mkh_solve_dense), B = 16: the (4, 4) list of the UR5e plus a user box limit on three dofs, one of them
    one-sided, one tighter than every built-in term, so that dense_lo / dense_hi intersect the merged box."""
    c, B = ll.case("ur5e"), 16
    rows = sorted(set(range(13)) | set(c.made_infeasible) | set(c.made_outside))[:B]
    assert len(rows) == B
    terms = ll.terms_of(c, 4, 4)
    lo, hi = np.full((B, c.m.nv), -np.inf), np.full((B, c.m.nv), np.inf)
    lo[:, 0], hi[:, 0] = -0.004, 0.004
    hi[:, 5] = 0.002 + 1e-4 * np.arange(B)                    # per instance
    lo[:, 2] = -0.02                                          # looser than the list: changes nothing
    prob = handles("ur5e", c.cfg, c.vel, B, dense_limit_box=True)
    v, st = prob.solve(c.q[rows], c.tg[rows], c.pt[rows], None, c.dt, c.damping, dense={"limit_lo": lo, "limit_hi": hi})
    assert prob.last_kernel().startswith("ik_solve_kernel"), prob.last_kernel()
    worst, n_inf, on_user = 0.0, 0, 0
    for k, i in enumerate(rows):
        G = np.zeros((4, c.m.nv)); G[0, 0] = 1; G[1, 0] = -1; G[2, 5] = 1; G[3, 2] = -1
        user = oik.DenseLimitSpec(G, np.array([hi[k, 0], -lo[k, 0], hi[k, 5], -lo[k, 2]]))
        v_ref, st_ref, _, _ = ll.solve_one(c, i, terms, extra=[user])
        assert st[k] == st_ref, (i, st[k], st_ref)
        if st_ref & ll.ST_INFEASIBLE:
            n_inf += 1
            assert np.isnan(v[k]).all()
            continue
        worst = max(worst, float(np.abs(v[k] - v_ref).max() / max(1.0, np.abs(v_ref).max())))
        on_user += int(abs(abs(v_ref[0] * c.dt) - 0.004) < 1e-12) + int(abs(v_ref[5] * c.dt - hi[k, 5]) < 1e-12)
    print("plugin route on %s: max rel err vs oracle %.2e, %d infeasible, %d user bounds active" % (prob.last_kernel(), worst, n_inf, on_user))
    assert worst <= 1e-8 and n_inf >= 1 and on_user >= 8


def test_two_collision_limits_with_their_own_parameters(nat):
    """`ur5e_coll`: two CollisionAvoidanceLimits over different pair subsets with their own gain, minimum distance, detection
    distance and bound relaxation (one of them 1e-3), one geom pair in both: the coll_G / coll_h taps in list order against the
    oracle's rows (tests/test_gpu_golden.py's bounds for this fixture), v against the oracle."""
    d = np.load(os.path.join(oc.GOLDEN, "ik_ur5e_coll.npz"))
    m = oc.model("ur5e")
    nm = _nmodel(nat, "ur5e")
    pairs = [tuple(int(x) for x in p) for p in d["geom_id_pairs"]]
    assert len(pairs) == 2
    colA = oik.CollisionAvoidanceLimitSpec(pairs, 0.85, 0.005, 0.3, 0.0)
    colB = oik.CollisionAvoidanceLimitSpec(pairs[1:], 0.5, 0.02, 0.2, 1e-3)
    as_native = lambda s: {"geom_id_pairs": np.array(s.geom_id_pairs), "gain": s.gain, "minimum_distance_from_collisions": s.minimum_distance_from_collisions,
                           "collision_detection_distance": s.collision_detection_distance, "bound_relaxation": s.bound_relaxation}
    B = len(d["q"])
    g = {"frame_type": "geom", "frame_id": m.name2id("geom", "wrist_2_link"), "cost": [0.5, 0.5, 0.5, 0.1, 0.2, 0.3], "gain": 0.7, "lm_damping": 0.0}
    prob = nat.NativeProblem(nm, frame_tasks=[nc._ft(m, "attachment_site", "site", 1.0, 1.0, 1.0), g], configuration_limits=[nc._cfg_limit(m)],
                             collision_limits=[as_native(colA), as_native(colB)], velocity_limits=[nc._vel_limit(m)], max_batch=B)
    assert prob.n_pairs == 3
    dt, damping = 5e-2, 1e-3
    v, st, taps = prob.solve(d["q"], d["frame_targets"], None, None, dt, damping, taps=["coll_G", "coll_h"])
    v2, st2 = prob.solve(d["q"], d["frame_targets"], None, None, dt, damping)
    print("two collision limits:", prob.last_kernel())
    worst, differ, active = 0.0, 0, 0
    for i in range(B):
        _, tasks, limits, _, _ = oc.ur5e_coll(d, i)
        limits = [limits[0], colA, colB, limits[2]]
        v_ref, (_, _, G, h) = oik.solve_ik(m, d["q"][i], tasks, dt, damping, limits, return_problem=True)
        Gc, hc = G[12:15], h[12:15]
        fin = np.isfinite(hc)
        assert np.array_equal(np.isfinite(taps["coll_h"][i]), fin), i
        np.testing.assert_allclose(taps["coll_h"][i][fin], hc[fin], rtol=0, atol=1e-9)
        np.testing.assert_allclose(taps["coll_G"][i], Gc, rtol=0, atol=1e-10)
        differ += int(fin[1] and fin[2] and abs(hc[1] - hc[2]) > 1e-6)
        active += int((np.abs(Gc[fin] @ (v_ref * dt) - hc[fin]) < 1e-10).sum())
        for out in (v, v2):
            worst = max(worst, float(np.abs(out[i] - v_ref).max() / max(1.0, np.abs(v_ref).max())))
    print("two collision limits: max rel err vs oracle %.2e; the shared pair's two rows differ on %d of %d instances; %d rows active" % (worst, differ, B, active))
    prob.close()
    assert ((st & ~1) == 0).all() and np.array_equal(st, st2)
    assert worst <= 1e-8 and differ >= 4 and active >= 4


def test_more_than_four_velocity_limits_fold_on_the_host():
    """solve_ik(..., limits=[...]) with six VelocityLimits on the UR5e: the surplus folds into the fourth term as per-dof minima.
    Against the oracle with all six stacked, and bitwise against the call that hands over the four folded terms itself."""
    import mink_amd as mink
    c = ll.case("ur5e")
    m = mink.load_robot("ur5e")
    names = list(m.jnt_names)
    rows = [i for i in range(c.B) if i not in c.made_infeasible][:32]
    cfg = mink.Configuration(m, c.q[rows])
    ft = mink.FrameTask("attachment_site", "site", position_cost=1.0, orientation_cost=1.0, lm_damping=1.0)
    ft.set_target(mink.SE3(c.tg[rows][:, 0]))
    post = mink.PostureTask(m, cost=1e-2)
    post.set_target(c.q_ref)
    vmaps = [{n: 0.3 for n in names}, {names[0]: 0.5, names[1]: 0.25}, {names[3]: 0.2, names[4]: 0.2}, {names[4]: 0.05},
             {names[1]: 0.1, names[5]: 0.15}, {names[4]: 0.5, names[2]: 0.12}]
    six = [mink.VelocityLimit(m, v) for v in vmaps]
    merged = dict(vmaps[3])
    for v in vmaps[4:]:
        for n, x in v.items():
            merged[n] = min(merged.get(n, np.inf), x)
    four = [mink.VelocityLimit(m, v) for v in vmaps[:3] + [merged]]
    lim0 = [mink.ConfigurationLimit(m)]
    v6 = mink.solve_ik(cfg, [ft, post], c.dt, "mi355x", c.damping, limits=lim0 + six)
    v4 = mink.solve_ik(cfg, [ft, post], c.dt, "mi355x", c.damping, limits=lim0 + four)
    assert np.array_equal(v6, v4)
    om = oc.model("ur5e")
    worst, bound = 0.0, 0
    for k, i in enumerate(rows):
        tasks = [oik.FrameTaskSpec(om.name2id("site", "attachment_site"), "site", np.ones(6), c.tg[i, 0], lm_damping=1.0),
                 oik.PostureTaskSpec(np.full(om.nv, 1e-2), c.q_ref)]
        limits = [oik.ConfigurationLimitSpec()] + [oik.VelocityLimitSpec(np.array(l.indices), np.array(l.limit)) for l in six]
        v_ref = oik.solve_ik(om, c.q[i], tasks, c.dt, c.damping, limits)
        worst = max(worst, float(np.abs(v6[k] - v_ref).max() / max(1.0, np.abs(v_ref).max())))
        bound += int(abs(abs(v_ref[1]) - 0.1) < 1e-12) + int(abs(abs(v_ref[2]) - 0.12) < 1e-12)
    print("six velocity limits: max rel err vs oracle %.2e; bounds of the fifth and sixth term active %d times" % (worst, bound))
    assert worst <= 1e-8 and bound >= 8
