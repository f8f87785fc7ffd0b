"""The reference side of tests/test_gpu_wood_lists.py, on the CPU: every fixture of tests/wood_list_cases.py is well posed —
the C oracle solves each of its instances, and the numpy oracle, which shares no code with it, agrees on every eighth to
1e-10·max(1, ‖v‖∞).  A fixture that fails here is changed, never the device test's tolerance."""

import numpy as np
import pytest

import wood_list_cases as wl
from oracle import ik as oik


@pytest.mark.parametrize("name", list(wl.BUILDERS))
def test_both_oracles_solve_the_fixture_and_agree(name):
    c = wl.case(name)
    v_ref, st_ref = wl.reference(name)
    assert c.q.shape == (wl.B, c.model.nq) and np.isfinite(c.frame_targets).all()
    assert (st_ref == 0).all(), (name, np.unique(st_ref, return_counts=True))         # no Infeasible, no NotPositiveDefinite
    worst = 0.0
    for i in range(0, wl.B, 8):
        tasks, limits = wl.oracle_tasks(c, i)
        v = oik.solve_ik(c.oracle_model, c.q[i], tasks, c.dt, c.damping, limits)     # (raises where the problem is infeasible)
        worst = max(worst, np.abs(v - v_ref[i]).max() / max(1.0, np.abs(v_ref[i]).max()))
    print("%s: numpy oracle vs C oracle on %d instances: %.2e" % (name, len(range(0, wl.B, 8)), worst))
    assert worst < 1e-10, (name, worst)


def test_the_anchor_models_differ_in_one_joint_position_only():
    z, m = wl.case("anchors_zero").model, wl.case("anchors_moved").model
    assert not np.asarray(z.jnt_pos).any()
    moved = np.flatnonzero(np.abs(np.asarray(m.jnt_pos)).reshape(m.njnt, 3).max(axis=1) > 0)
    assert len(moved) == 1 and int(m.jnt_type[moved[0]]) == 3                        # one hinge
    assert max(np.bincount(np.asarray(z.jnt_bodyid))) == 2                           # a body with two joints
    np.testing.assert_array_equal(wl.case("anchors_zero").q, wl.case("anchors_moved").q)


def test_the_chains_sit_around_the_list_capacity():
    for n in (16, 17, 40, 63):
        assert wl.case("chain%d" % n).model.nv == n
    # G1's bench task set: chains of different lengths in one problem
    m = wl.case("g1_bench").model
    assert m.nv == 43 and not np.asarray(m.jnt_pos).any()                            # the joint-anchor flag is on for the headline
