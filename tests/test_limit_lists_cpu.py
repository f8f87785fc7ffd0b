"""The inputs of tests/test_gpu_limit_lists.py, checked from the numpy oracle alone before a kernel sees them (tests/limit_lists.py
check_conditions): every term after the first of its kind binds on at least four instances and moves the solution there by more
than 1e-4 relative when it is dropped; at least half of the instances have two or more dofs on a bound; no dof sits on the device's
inconsistency gate except the frozen one, which sits on it exactly; the instances built to be infeasible are, and three quarters
are not."""

import numpy as np
import pytest

import limit_lists as ll


@pytest.mark.parametrize("family", ["ur5e", "leap", "h1", "g1", "balllimit", "chain70"])
def test_conditions_on_the_inputs(family):
    for n_cfg, n_vel in ll.COUNTS:
        fig = ll.check_conditions(family, n_cfg, n_vel)
        print(family, (n_cfg, n_vel), fig)
        assert set(fig["witness"]) == {name for name, _, _ in ll.terms_of(ll.case(family), n_cfg, n_vel)} - {"cfg0", "vel0"}


@pytest.mark.parametrize("n_cfg,n_vel", [(2, 2), (4, 4), (3, 0)])
def test_the_ball_joints_second_term_binds(n_cfg, n_vel):
    """The limited ball joint of `balllimit` sits in cfg0 (gain 0.95) and cfg1 (gain 0.5).  On at least four feasible instances
    cfg1's upper bound on one of its three dofs is the tighter of the two and the solution sits on it, and there a solve without
    cfg1 moves v_ref by more than 1e-4 relative: a ball branch that stopped after its first term, or took every term at cfg0's
    gain, would miss the 1e-8 bound there."""
    from oracle import ik as oik
    c = ll.case("balllimit")
    r = ll.reference("balllimit", n_cfg, n_vel)
    terms = ll.terms_of(c, n_cfg, n_vel)
    ball = [5, 6, 7]
    hits, moved = [], []
    for k, i in enumerate(r.rows):
        if r.st[k] & ll.ST_INFEASIBLE:
            continue
        cfg = oik.Configuration(c.m, c.q[i])
        hi = {}
        for name in ("cfg0", "cfg1"):
            spec = next(s for n, s, _ in terms if n == name)
            G, h = oik.limit_inequalities(cfg, spec, c.dt)
            hi[name] = ll.box_of_rows(G, h, c.m.nv)[1][ball]
        dq = r.v[k][ball] * c.dt
        if ((hi["cfg1"] < hi["cfg0"] - 1e-6) & (np.abs(dq - hi["cfg1"]) <= 1e-10)).any():
            hits.append(k)
    assert len(hits) >= 4, len(hits)
    for k in hits[:6]:
        v2, st2, _, _ = ll.solve_one(c, r.rows[k], [t for t in terms if t[0] != "cfg1"])
        assert not st2 & ll.ST_INFEASIBLE
        moved.append(float(np.abs(v2 - r.v[k]).max() / max(1.0, np.abs(r.v[k]).max())))
    print("balllimit (%d, %d): cfg1 the tighter term and active on a ball dof in %d instances; without it v moves by %s" % (
        n_cfg, n_vel, len(hits), ["%.1e" % x for x in moved]))
    assert sum(1 for x in moved if x > 1e-4) >= 4, moved


def test_the_list_is_what_it_says():
    """Subsets disjoint, the copy a copy, the frozen dof frozen, vel3 the tightest, a free joint's dofs in no term."""
    for family in ("ur5e", "h1", "balllimit"):
        c = ll.case(family)
        m = c.m
        L, D, jid = ll.dof_sets(m)
        odd, even = ll.subsets(m)
        assert odd and even and not set(odd) & set(even) and set(odd) | set(even) <= set(L)
        (_, s0, d0), (_, s1, d1), (_, s2, d2), (_, s3, d3) = c.cfg
        assert (s0.gain, s1.gain, s2.gain, s3.gain) == (0.95, 0.5, 1.0, 0.95) and s1.min_distance_from_limits == 0.02
        assert all(np.array_equal(d0[k], d3[k]) for k in ("lower", "upper", "indices")) and d0["indices"].tolist() == L
        assert d1["indices"].tolist() == odd and d2["indices"].tolist() == even
        v0, v1, v2, v3 = (d for _, _, d in c.vel)
        assert v0["indices"].tolist() == D and v1["indices"].tolist() + v2["indices"].tolist() == D
        assert (v1["limit"] == 0.0).sum() == 1 and v1["indices"][v1["limit"] == 0.0][0] == ll.frozen_dof(m)
        assert len(v3["indices"]) == 1 and v3["limit"][0] < min(v0["limit"].min(), v2["limit"].min(), v1["limit"][v1["limit"] > 0].min())
        free = [d for d in range(m.nv) if d not in D]
        assert not set(free) & (set(L) | set(D)) and (family != "h1" or free == list(range(6)))
    # the limited ball joint: in cfg0 and cfg1 (two gains, the same range in its four slots), its dofs in vel0 and vel2
    c = ll.case("balllimit")
    ball = [5, 6, 7]
    assert set(ball) <= set(c.cfg[0][2]["indices"]) and c.cfg[1][2]["indices"].tolist() == ball and not set(ball) & set(c.cfg[2][2]["indices"])
    assert np.array_equal(c.cfg[0][2]["upper"][6:10], c.cfg[1][2]["upper"][6:10]) and np.array_equal(c.cfg[0][2]["lower"][6:10], c.cfg[1][2]["lower"][6:10])
    assert set(ball) <= set(c.vel[0][2]["indices"]) & set(c.vel[2][2]["indices"])
