"""Distinct solution sets without a GPU: the two restatements of the rule (tests/solution_set_ref.py) agree, slot 0 is
multi-start's choice, the counts add up, both public functions validate their arguments before they touch a device, the two entry
points are declared, bound and documented, and the new kernel is compiled without spilled vector registers."""

import ctypes
import json
import os
import re

import numpy as np
import pytest

import multistart_ref as ms
import oracle_configs as oc
import solution_set_cases as cases
import solution_set_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _models():
    import mink_amd
    return {"ur5e": oc.model("ur5e"), "ballslide": mink_amd.load_mjcf(os.path.join(GOLDEN, "ballslide.xml"))}


def _same(a: ref.Selection, b: ref.Selection):
    np.testing.assert_array_equal(a.seed_index, b.seed_index)
    np.testing.assert_array_equal(a.multiplicity, b.multiplicity)
    np.testing.assert_array_equal(a.distance, b.distance)
    assert (a.n_distinct, a.n_eligible, a.n_uncovered) == (b.n_distinct, b.n_eligible, b.n_uncovered)


def _check_target(m, q, ok, q_ref, K, r, w=None):
    a = ref.select_cover(m, q, ok, q_ref, K, r, w)
    b = ref.select_walk(m, q, ok, q_ref, K, r, w)
    _same(a, b)
    # slot 0 is multi-start's choice
    dr = ref.d_ref(m, q, q_ref, w)
    best, conv, n = ms.select(dr, ok.astype(np.int32), np.zeros(len(q), dtype=np.int32))
    assert a.n_eligible == n
    if conv:
        assert a.seed_index[0] == best and a.distance[0] == dr[best]
    else:
        assert a.n_distinct == 0 and (a.seed_index == -1).all()
    # the counts add up; empty slots are flagged
    assert a.multiplicity.sum() == a.n_eligible - a.n_uncovered
    filled = np.arange(K) < a.n_distinct
    assert (a.seed_index[filled] >= 0).all() and (a.multiplicity[filled] >= 1).all() and np.isfinite(a.distance[filled]).all()
    assert (a.seed_index[~filled] == -1).all() and (a.multiplicity[~filled] == 0).all() and np.isinf(a.distance[~filled]).all()
    assert (np.diff(a.distance[filled]) >= 0).all()                       # ascending distance from the reference
    assert a.n_uncovered == 0 or a.n_distinct == K
    return a


@pytest.mark.parametrize("name", ["ur5e", "ballslide"])
def test_two_formulations_agree_on_random_candidates(name):
    """Unstructured candidates (no margins): both restatements make the same comparisons on the same numbers, so they agree
    whatever the geometry — r from "nothing merges" to "everything merges", K from 1 to more than there are candidates."""
    m = _models()[name]
    rng = np.random.default_rng(5)
    n = 0
    for S, K, r in ((1, 1, 0.1), (9, 3, 0.0), (17, 4, 0.3), (17, 64, 1.0), (40, 2, 0.5), (40, 8, 10.0)):
        for _ in range(3):
            q_ref = ms.draw_seeds(m, np.asarray(m.qpos0, dtype=np.float64)[None], 2, rng_seed=int(rng.integers(1 << 30)))[0, 1]
            q = np.array([cases._moved(m, q_ref, rng.normal(scale=rng.choice([0.05, 0.5]), size=m.nv)) for _ in range(S)])
            ok = rng.uniform(size=S) < 0.8
            w = None if n % 2 else rng.uniform(0.1, 10.0, size=m.nv)
            a = _check_target(m, q, ok, q_ref, K, r, w)
            n += a.n_distinct
    assert n > 20


def test_ties_exact_duplicates_and_nothing_eligible():
    m = _models()["ur5e"]
    rng = np.random.default_rng(1)
    q_ref = np.asarray(m.qpos0, dtype=np.float64)
    a, b, c = (cases._moved(m, q_ref, u) for u in (np.eye(m.nv)[0] * 0.5, np.eye(m.nv)[1] * 0.5, np.eye(m.nv)[2] * 0.7))
    # a and b are equally far from the reference: the tie goes to the lower index, whichever of them that is
    for q, want in ((np.array([c, b, a, b, a]), [1, 2, 0]), (np.array([c, a, b, a, b]), [1, 2, 0])):
        s = _check_target(m, q, np.ones(5, dtype=bool), q_ref, 4, 0.0)
        assert s.seed_index.tolist() == want + [-1] and s.multiplicity.tolist() == [2, 2, 1, 0] and s.n_uncovered == 0
    # r = 0 merges bitwise duplicates only: a row that differs in its last bit is a solution of its own
    a2 = a.copy(); a2[0] = np.nextafter(a2[0], 1.0)
    s = _check_target(m, np.array([a, a, a2]), np.ones(3, dtype=bool), q_ref, 4, 0.0)
    assert s.n_distinct == 2 and sorted(s.multiplicity[:2].tolist()) == [1, 2]
    # truncation: K smaller than the number of solutions leaves the farthest uncovered
    s = _check_target(m, np.array([c, b, a, b, a]), np.ones(5, dtype=bool), q_ref, 2, 0.1)
    assert s.seed_index.tolist() == [1, 2] and s.n_uncovered == 1
    # ineligible candidates are never chosen and never counted
    s = _check_target(m, np.array([c, b, a, b, a]), np.array([1, 0, 1, 0, 0], dtype=bool), q_ref, 3, 0.1)
    assert s.seed_index.tolist() == [2, 0, -1] and s.multiplicity.tolist() == [1, 1, 0] and s.n_eligible == 2
    s = _check_target(m, np.array([c, b]), np.zeros(2, dtype=bool), q_ref, 3, 0.1)
    assert s.n_distinct == 0 and s.n_eligible == 0 and s.n_uncovered == 0
    # a NaN row is last among the eligible, covers only itself and is covered by nothing
    bad = a.copy(); bad[3] = np.nan
    s = _check_target(m, np.array([bad, a, a]), np.ones(3, dtype=bool), q_ref, 3, 0.1)
    assert s.seed_index.tolist() == [1, 0, -1] and s.multiplicity.tolist() == [2, 1, 0] and s.distance[1] == ref.DBL_MAX
    del rng


@pytest.mark.parametrize("name", ["ur5e", "ballslide"])
def test_cluster_fixture_meets_its_conditions_and_is_recovered(name):
    """The synthetic cases of the GPU test: their margins hold by the numpy distance, and the rule finds the clusters."""
    m = _models()[name]
    rng = np.random.default_rng(3)
    w = rng.uniform(0.1, 10.0, size=m.nv)
    for weights, dup, r in ((None, False, 0.1), (w, False, 0.1), (None, True, 0.0)):
        q, valid, q_ref, centres = cases.make_case(m, rng, 2, 30, 3, weights=weights, duplicates=dup)
        cases.check_case(m, centres, q_ref, 0.1, weights)
        for b in range(2):
            s = _check_target(m, q[b], valid[b] != 0, q_ref[b], 5, r, weights)
            assert s.n_distinct == 3 and s.n_uncovered == 0
            assert dup or s.margin > 1e-9                                 # (bitwise copies tie exactly: the index decides)
            np.testing.assert_allclose(s.distance[:3], [0.25, 0.4225, 0.64], rtol=1e-4)


def test_argument_validation_needs_no_gpu():
    import mink_amd

    m = oc.model("ur5e")
    cfg = mink_amd.Configuration(m, np.tile(np.asarray(m.qpos0), (4, 1)))
    task = mink_amd.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    task.set_target(mink_amd.SE3(np.array([1.0, 0, 0, 0, 0.3, 0.2, 0.4])))
    call = lambda **kw: mink_amd.solve_ik_solutions(cfg, [task], 1.0, **{**dict(n_seeds=4, n_solutions=2, max_iters=10,
                                                                                 pos_threshold=1e-4, ori_threshold=1e-4), **kw})
    with pytest.raises(ValueError, match="n_seeds"):
        call(n_seeds=0)
    for K in (0, -1, 65):
        with pytest.raises(ValueError, match="n_solutions"):
            call(n_solutions=K)
    for r in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_distance"):
            call(min_distance=r)
    with pytest.raises(ValueError, match="candidates per target"):
        call(n_seeds=4097)
    with pytest.raises(ValueError, match="max_iters"):
        call(max_iters=0)
    with pytest.raises(ValueError, match="max_instances"):
        call(max_instances=0)
    for bad in (np.zeros((3, m.nq)), np.zeros((4, 4, m.nq + 1)), np.zeros((2, 4, m.nq)), np.zeros(m.nq)):
        with pytest.raises(ValueError, match="seeds must have shape"):
            call(seeds=bad)
    with pytest.raises(ValueError, match="reference must have shape"):
        call(reference=np.zeros((3, m.nq)))
    with pytest.raises(ValueError, match="weights must have shape"):
        call(weights=np.ones(m.nv + 1))
    with pytest.raises(ValueError, match="seeds and seed_table"):
        call(seeds=np.zeros((4, m.nq)), seed_table=object())
    with pytest.raises(ValueError, match="seed_table must be a SeedTable"):
        call(seed_table=object())
    with pytest.raises(TypeError):
        call(update=False)                                                # a set does not update the configuration: no keyword

    cand = np.zeros((4, 5, m.nq))
    sel = lambda q_candidates=cand, **kw: mink_amd.distinct_solutions(cfg, q_candidates, **{**dict(n_solutions=2), **kw})
    for bad in (np.zeros((5, m.nq + 1)), np.zeros((3, 5, m.nq)), np.zeros(m.nq), np.zeros((4, 0, m.nq)), None):
        with pytest.raises(ValueError, match="q_candidates must have shape"):
            sel(bad)
    for K in (0, 65):
        with pytest.raises(ValueError, match="n_solutions"):
            sel(n_solutions=K)
    for r in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_distance"):
            sel(min_distance=r)
    with pytest.raises(ValueError, match="candidates per target"):
        sel(np.zeros((4097, m.nq)))
    with pytest.raises(ValueError, match="valid must have shape"):
        sel(valid=np.ones((4, 6)))
    with pytest.raises(ValueError, match="reference must have shape"):
        sel(reference=np.zeros((3, m.nq)))
    with pytest.raises(ValueError, match="weights must have shape"):
        sel(weights=np.ones(m.nv + 1))

    for name in ("solve_ik_solutions", "SolutionSet", "distinct_solutions", "DistinctSet"):
        assert name in mink_amd.__all__ and hasattr(mink_amd, name), name
    assert mink_amd.SolutionSet._fields == ("q", "v", "valid", "seed_index", "distance", "multiplicity", "iters", "status",
                                            "n_distinct", "n_converged", "n_uncovered", "q_all", "converged_all", "iters_all",
                                            "status_all", "seeds")
    assert mink_amd.DistinctSet._fields == ("q", "valid", "seed_index", "distance", "multiplicity", "n_distinct", "n_valid",
                                            "n_uncovered")


NEW_FUNCTIONS = ("mkh_solve_multistart_set", "mkh_select_distinct")


def test_entry_points_are_declared_bound_and_documented():
    from mink_amd import _native as nat
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    L = nat.lib()
    assert L.mkh_version() == 108                                        # additive: the ABI number stays
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "minkhip.h")).read()
    for f in NEW_FUNCTIONS:
        assert f in nat.EXPORTED_SYMBOLS, f
        assert getattr(L, f) is not None
        assert re.search(r"^int32_t " + f + r"\(", hdr, re.M), f
    assert ctypes.sizeof(nat.MkhSolutionSetIO) == 18 * ctypes.sizeof(ctypes.c_void_p)
    fields = hdr.split("typedef struct MkhSolutionSetIO {")[1].split("} MkhSolutionSetIO;")[0]
    assert tuple(re.findall(r"\*(\w+);", fields)) == nat.SOLUTION_SET_IO_FIELDS              # same order as the ctypes mirror
    for word in ("THE RULE OF THE SET", "ties to the lowest index", "stays uncovered", "DIFFERENT", "bitwise what mkh_solve_multistart returns",
                 "1 <= n_solutions <= 64", "4 096 candidates"):
        assert word in hdr, word
    # null / bad arguments fail loudly before any device is touched
    io = nat.MkhSolutionSetIO()
    args = (None, 1, None, None, None, None, 1.0, 1e-3, 10, 1e-4, 1e-4, 4)
    assert L.mkh_solve_multistart_set(*args, 2, 0.1, 0, 0, ctypes.byref(io), 0, None) == -1
    assert b"null problem" in L.mkh_last_error()
    assert L.mkh_select_distinct(None, 1, 4, None, None, None, None, 2, 0.1, ctypes.byref(io), 0, None) == -1
    assert b"null problem" in L.mkh_last_error()


def test_new_kernel_keeps_its_vector_registers():
    """No spilled VGPR, no scratch, no call (tests/test_abi.py holds every kernel outside the spill budget to zero).  Scalar
    registers that do not fit are parked in lanes of a vector register, not in memory: scratch stays 0."""
    from mink_amd.csrc import build as hipbuild

    hipbuild.build(verbose=False)
    with open(hipbuild.RESOURCES) as fh:
        table = json.load(fh)
    e = table.get("solution_set_select_kernel")
    assert e is not None, sorted(x for x in table if "solution" in x)
    assert e["vgpr_spills_with_callees"] == 0 and e["scratch_bytes_per_lane"] == 0, e
    assert e["callees"] == {}, e["callees"]                               # everything inlined: no call, no stack
    with open(os.path.join(GOLDEN, "spill_budget.json")) as fh:
        assert "solution_set_select_kernel" not in json.load(fh)
