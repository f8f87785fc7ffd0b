"""The numpy statement of the product-form active set (tools/proto_product_form.py: the kernel's rules — cold-start refinement,
block steps, hand-over, Goldfarb–Idnani — on the factors of the low-rank start, a history of P pivots, refactorisation from the
active set when it is full) against the plain-C oracle, on the 256 seeded G1 config-3 problems that tests/test_gpu_product_form.py
solves on the device.  Measure and bound of tests/test_gpu_headline_paths.py: |v − v_ref|∞ / max(1, |v_ref|∞) < 1e-8 on EVERY
instance; statuses agree.  P = 13 is the kernel's history; P = 2 refactorises every solve that needs a third pivot.

The same fixture without the cold-start refinement is what exercises refactorisation on the device (MKH_DIAG_NO_COLD_REFINE): the
replay must report more than 13 pivots on at least a quarter of its instances (13.4 pivots per solve on average
without the refinement)."""

import os
import sys

import numpy as np
import pytest

import oracle_configs as oc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

B_SMALL, SEED_SMALL = 256, 1601          # (as in tests/test_gpu_product_form.py)


@pytest.fixture(scope="module")
def fixture():
    import proto_product_form as pf
    from oracle import cport
    q, tg, stand = pf.g1_batch(B_SMALL, SEED_SMALL)
    pt = np.asarray(stand)[None, :].copy()
    m, tasks, limits, dt, damping = oc.g1_c3(tg[0], pt[0])
    v_ref, st_ref = cport.CProblem(m, tasks, limits).solve_batch(q, tg, pt, dt, damping, nthreads=min(16, os.cpu_count() or 1))
    return pf, pf.g1_problems(q, tg, stand), v_ref, st_ref


def _check(v, st, v_ref, st_ref, label):
    assert (st_ref == 0).all(), (label, np.unique(st_ref, return_counts=True))       # the oracle solves every instance
    assert np.array_equal(st, st_ref), (label, np.unique(st, return_counts=True))    # statuses agree
    err = np.abs(v - v_ref).max(axis=1) / np.maximum(1.0, np.abs(v_ref).max(axis=1))
    print("%s: max rel err vs C oracle %.2e" % (label, err.max()))
    assert err.max() < 1e-8, (label, err.max(), int(err.argmax()))                   # EVERY instance


def test_history_of_13(fixture):
    pf, problems, v_ref, st_ref = fixture
    v, st, piv, ref = pf.replay(problems, P=13)
    print("P = 13: pivots per solve mean %.2f max %d, %d of %d solves refactorise" % (piv.mean(), piv.max(), int((ref > 0).sum()), len(ref)))
    _check(v, st, v_ref, st_ref, "P = 13")


def test_history_of_2(fixture):
    pf, problems, v_ref, st_ref = fixture
    v, st, piv, ref = pf.replay(problems, P=2)
    print("P = 2: %d of %d solves refactorise, up to %d times" % (int((ref > 0).sum()), len(ref), ref.max()))
    assert (ref[piv > 2] > 0).all() and (piv > 2).mean() > 0.25   # every solve with more than two pivots — 4 in 10 on this distribution
    _check(v, st, v_ref, st_ref, "P = 2")


def test_without_the_refinement_the_history_fills(fixture):
    pf, problems, v_ref, st_ref = fixture
    v, st, piv, ref = pf.replay(problems, P=13, cold_refine=False)
    print("no refinement: pivots per solve mean %.2f, more than 13 on %d of %d, %d refactorise" % (
        piv.mean(), int((piv > 13).sum()), len(piv), int((ref > 0).sum())))
    assert (piv > 13).mean() >= 0.25
    assert (ref[piv > 13] > 0).all()
    _check(v, st, v_ref, st_ref, "P = 13 without the refinement")


def test_block_steps_go_on_across_refactorisations():
    """The 24 golden G1 instances include ill-conditioned, heavily saturated ones (cond(H) ≈ 2e5, 25 of 37 bounds active) on which
    block steps flip-flop.  Started afresh after every refactorisation they never hand over to Goldfarb–Idnani: two instances ran
    350 pivots into the iteration cap (status 8), on the device too.  The count of block steps and the best infeasibility count
    are carried across refactorisations instead; every instance ends, with and without the cold-start refinement."""
    import proto_product_form as pf
    d = np.load(os.path.join(REPO, "tests", "golden", "ik_g1_c3.npz"))
    problems = pf.g1_problems(d["q"], d["frame_targets"], d["posture_target"])
    for cold in (True, False):
        v, st, piv, ref = pf.replay(problems, P=13, cold_refine=cold)
        err = np.abs(v - d["v"]).max(axis=1) / np.maximum(1.0, np.abs(d["v"]).max(axis=1))
        print("golden, refinement %s: pivots max %d, refactorisations max %d, max rel err %.2e" % (cold, piv.max(), ref.max(), err.max()))
        assert (st == 0).all(), st
        assert ref.max() > 0 and piv.max() < 100
        assert err.max() < 1e-8
