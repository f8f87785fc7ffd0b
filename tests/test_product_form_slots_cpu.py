"""History slots of ONE double for the product form (tools/proto_product_form.py, `one_double`): a slot keeps own_q per lane, the
pivot's two wave-uniform scalars σ_k² and 1/d stay apart, and the multiplier g_q[j] = ((σ_k²)·own_q[j])·(1/d) is formed again
whenever a row is asked for.  That is what a register map with more, narrower slots would hold.  Three checks:

  * the re-formed multiplier is the stored one, float64 ==, on every entry of every row formed — so the solve is the two-double
    solve bit for bit, at any P;
  * at P = 13 — the slots of the four-waves map, as many as the two-double maps hold — no more than 1 % of 2 048 benchmark-like
    solves refactorise (the project's threshold for keeping the history in registers; ten slots would be 0.68 %);
  * the 24 golden instances, which flip-flop in block steps, all end (no status 8: the block-step carry stays).

The 512-problem sample is the one tests/test_product_form_cpu.py's sibling tools print (seed 0); measure and bound against the
golden velocities as there: |v − v_ref|∞ / max(1, |v_ref|∞) < 1e-8."""

import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

P_SLOTS = 13
N_SHARE, N_EQUAL, SEED = 2048, 512, 0


@pytest.fixture(scope="module")
def sample():
    import proto_product_form as pf
    return pf, pf.g1_problems(*pf.g1_batch(N_SHARE, SEED))


@pytest.mark.parametrize("cold", (True, False), ids=("refined", "unrefined"))
def test_reformed_multiplier_is_the_stored_one(sample, cold):
    pf, problems = sample
    problems = problems[:N_EQUAL]
    v2, st2, piv2, ref2 = pf.replay(problems, P=P_SLOTS, cold_refine=cold)
    uneq = []
    v1, st1, piv1, ref1 = pf.replay(problems, P=P_SLOTS, cold_refine=cold, one_double=True, unequal=uneq)
    print("P = %d, refinement %s: %d pivots, %d solves refactorise, unequal entries %d" % (P_SLOTS, cold, int(piv1.sum()), int((ref1 > 0).sum()), sum(uneq)))
    assert piv1.sum() > N_EQUAL                       # (rows with a history were formed at all)
    assert sum(uneq) == 0
    assert np.array_equal(st1, st2) and np.array_equal(piv1, piv2) and np.array_equal(ref1, ref2)
    assert np.array_equal(v1, v2)                     # bitwise (no NaN: every status is 0)
    assert (st1 == 0).all()


def test_share_that_refactorises_at_13_slots(sample):
    pf, problems = sample
    v, st, piv, ref = pf.replay(problems, P=P_SLOTS, one_double=True)
    share = (ref > 0).mean()
    print("P = %d: %d of %d solves refactorise (%.2f %%); histogram of pivots per solve %s" % (
        P_SLOTS, int((ref > 0).sum()), len(ref), 100.0 * share, np.bincount(piv).tolist()))
    assert (st == 0).all()
    assert share <= 0.01


def test_golden_instances_end_at_13_slots():
    import proto_product_form as pf
    d = np.load(os.path.join(REPO, "tests", "golden", "ik_g1_c3.npz"))
    problems = pf.g1_problems(d["q"], d["frame_targets"], d["posture_target"])
    for cold in (True, False):
        v, st, piv, ref = pf.replay(problems, P=P_SLOTS, cold_refine=cold, one_double=True)
        err = np.abs(v - d["v"]).max(axis=1) / np.maximum(1.0, np.abs(d["v"]).max(axis=1))
        print("golden, refinement %s: pivots max %d, refactorisations max %d, max rel err %.2e" % (cold, piv.max(), ref.max(), err.max()))
        assert (st == 0).all(), st                    # (8 = iteration cap: a refactorisation counts as P iterations)
        assert ref.max() > 0
        assert err.max() < 1e-8
