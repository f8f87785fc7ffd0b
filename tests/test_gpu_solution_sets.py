"""Distinct solution sets on the device (mkh_select_distinct / mkh_solve_multistart_set and the public calls on them): the
selection is the stated rule — exactly, on candidates whose every decision has a margin, and on the loops' own results —, slot 0
is multi-start's choice bit for bit, the loops know nothing of the selection, the result depends on neither chunks nor the kind
of array passed in, and the sets compose with the ladder search."""

import numpy as np
import pytest

import multistart_ref as ms
import solution_set_cases as cases
import solution_set_ref as ref
import test_gpu_multistart as tm
import test_gpu_trajectory_multistart as tms
from mink_amd import workloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _np(x):
    return None if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy())


# ------------------------------------------------------------------ 1. the rule, exact, on synthetic candidates
_models = {}


def _model(nat, name):
    """(model, a problem handle on it): the selection only reads the model's joint table through the handle."""
    if name not in _models:
        m = tm._mjcf(name) if name == "ballslide" else workloads.load_robot(name)
        nm = nat.NativeModel(m, 0)
        prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "body", "frame_id": m.nbody - 1, "cost": [1.0] * 6}], max_batch=1)
        _models[name] = (m, nm, prob)
    return _models[name][0], _models[name][2]


def _reference_sets(m, q, valid, q_ref, K, r, w):
    return [ref.select_cover(m, q[b], np.ones(q.shape[1], bool) if valid is None else valid[b] != 0, q_ref[b], K, r, w)
            for b in range(len(q))]


def _assert_is_the_rule(m, out, want, q, K, what):
    """Every output of a selection against the numpy rule: the integers and the gathered rows exactly; `distance`, the one
    computed double, to 1e-12 relative — the device's sum may fuse a product into an addition and its atan2 is another
    library's: a few units of 2^-53 per term of a sum of nv <= 64 terms, and for a rotation an absolute 1e-16 in the angle,
    which at the d_ref >= 0.25 of these cases is below 1e-15 relative."""
    B = len(want)
    out = type(out)(*[_np(x) for x in out])
    worst = 0.0
    for b, s in enumerate(want):
        for f in ("seed_index", "multiplicity"):
            np.testing.assert_array_equal(getattr(out, f)[b], getattr(s, f), err_msg=f"{what}: target {b}: {f}")
        assert (int(out.n_distinct[b]), int(out.n_uncovered[b])) == (s.n_distinct, s.n_uncovered), (what, b)
        assert int(out.n_valid[b]) == s.n_eligible, (what, b)
        for j in range(K):
            row = q[b, s.seed_index[j]] if j < s.n_distinct else q[b, 0]      # (an empty slot repeats candidate 0)
            np.testing.assert_array_equal(out.q[b, j], row, err_msg=f"{what}: target {b} slot {j}")
        filled = np.arange(K) < s.n_distinct
        assert np.isposinf(out.distance[b][~filled]).all()
        if filled.any():
            worst = max(worst, float(np.abs(out.distance[b][filled] / s.distance[filled] - 1.0).max()))
    print(f"{what}: {B} targets, n_distinct {[s.n_distinct for s in want]}, n_uncovered {[s.n_uncovered for s in want]}, "
          f"largest relative deviation of a distance {worst:.2e}")
    assert worst <= 1e-12


#         B,  S,  K, clusters, what it reaches
_CASES = {"lane_tail": (7, 130, 5, 4),         # two full lane rounds plus a tail; K beyond the clusters: an empty slot
          "single": (3, 1, 1, 1),              # one candidate, one slot
          "truncated": (3, 70, 2, 4),          # K below the clusters: n_uncovered > 0
          "none_valid": (2, 70, 3, 3),         # nothing eligible: every slot empty
          "duplicates": (3, 70, 5, 3),         # r = 0 on bitwise copies
          "weights": (3, 130, 5, 4)}           # non-unit weights


@pytest.mark.parametrize("case", list(_CASES))
@pytest.mark.parametrize("name", ["ur5e", "g1", "ballslide"])
def test_selection_is_the_rule_exactly(nat, name, case):
    """select_distinct alone (no loops) on clusters of candidates: centres >= 3 r apart, their d_ref >= 1e-3 apart, members
    within 1e-6 of their centre (tests/solution_set_cases.py asserts these by the numpy distance) — every decision has a
    margin, so every output is numpy's and no target is excluded."""
    m, prob = _model(nat, name)
    B, S, K, C = _CASES[case]
    rng = np.random.default_rng(sum(map(ord, name + case)))
    w = rng.uniform(0.1, 10.0, size=m.nv) if case == "weights" else None
    r = 0.0 if case == "duplicates" else 0.1
    q, valid, q_ref, centres = cases.make_case(m, rng, B, S, C, weights=w, duplicates=case == "duplicates",
                                               valid_fraction=1.0 if case == "single" else 0.9)
    cases.check_case(m, centres, q_ref, 0.1, w)
    if case == "none_valid":
        valid[:] = 0
    want = _reference_sets(m, q, valid, q_ref, K, r, w)
    out = prob.select_distinct(q, valid, q_ref, w, n_solutions=K, min_distance=r)
    _assert_is_the_rule(m, out, want, q, K, f"{name} {case}")
    # the fixture reaches what its name says
    nd, nu = np.array([s.n_distinct for s in want]), np.array([s.n_uncovered for s in want])
    if case in ("lane_tail", "weights"):
        assert (nd == C).all() and (nu == 0).all() and K > C
    elif case == "truncated":
        assert (nd == K).all() and (nu > 0).all()
    elif case == "none_valid":
        assert (nd == 0).all() and (_np(out.seed_index) == -1).all() and (_np(out.multiplicity) == 0).all()
    elif case == "duplicates":
        assert (nd == C).all() and all(s.multiplicity.sum() == s.n_eligible for s in want)
    if case == "lane_tail":
        # valid=None: every candidate counts; device tensors in, device tensors out, the same numbers
        import torch
        want_all = _reference_sets(m, q, None, q_ref, K, r, w)
        out_all = prob.select_distinct(q, None, q_ref, w, n_solutions=K, min_distance=r)
        _assert_is_the_rule(m, out_all, want_all, q, K, f"{name} {case}, valid=None")
        dev = torch.device("cuda:0")
        out_t = prob.select_distinct(torch.as_tensor(q, device=dev), torch.as_tensor(valid, device=dev),
                                     torch.as_tensor(q_ref, device=dev), None, n_solutions=K, min_distance=r)
        assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in out_t)
        for f in out._fields:
            np.testing.assert_array_equal(_np(getattr(out_t, f)), getattr(out, f), err_msg=f"torch: {f}")


# ------------------------------------------------------------------ 2. slot 0 is multi-start's, bitwise
_K, _R = 4, 0.1
_solved = {}


def _setup(nat, name):
    """The three set-ups of test_gpu_multistart.py::test_selection_is_the_stated_rule, at their shapes there."""
    if name == "ur5e_far":
        from mink_amd.api_specs import configuration_limit_desc
        m = workloads.load_robot("ur5e")
        nm = nat.NativeModel(m, 0)
        B, S, iters, pth, oth, dt, damping = 96, 16, 40, 1e-4, 1e-4, 1.0, 1e-3
        prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "attachment_site"),
                                                   "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 1.0}],
                                 configuration_limits=[configuration_limit_desc(m)], max_batch=B * S)
        q = np.tile(m.key_qpos[0], (B, 1))
        tg = tm._far_targets(m, B)[:, None, :]
        pt = ct = None
    elif name == "ballslide":
        import mink_amd as mink
        from mink_amd.api_specs import configuration_limit_desc
        m = tm._mjcf("ballslide")
        nm = nat.NativeModel(m, 0)
        B, S, iters, pth, oth, dt, damping = 32, 16, 40, 1e-3, 1e-2, 1.0, 1e-3
        prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": m.name2id("site", "tip"),
                                                   "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 0.1}],
                                 configuration_limits=[configuration_limit_desc(m)], max_batch=B * S)
        q = tm._start(m, B, np.random.default_rng(4))
        goal = ms.draw_seeds(m, q, 2, rng_seed=77)[:, 1]
        tg = mink.Configuration(m, goal).get_transform_frame_to_world("tip", "site").wxyz_xyz[:, None, :]
        pt = ct = None
    else:
        m, nm, prob, (q, tg, pt, ct), dt, damping, (B, S, pth, oth, iters) = tm._workload(nat, name)
    kw = dict(n_seeds=S, max_iters=iters, pos_threshold=pth, ori_threshold=oth, rng_seed=8, return_all=True)
    return m, nm, prob, (q, tg, pt, ct, dt, damping), kw


def _solve_both(nat, name):
    """(model, q, plain multi-start, the set, the same two with reference= and weights=) of one set-up, solved once."""
    if name not in _solved:
        m, nm, prob, args, kw = _setup(nat, name)
        plain = prob.solve_multistart(*args, **kw)
        sets = prob.solve_multistart_set(*args, n_solutions=_K, min_distance=_R, **kw)
        rng = np.random.default_rng(1)
        B, S = plain.q_all.shape[:2]
        q_ref = plain.q_all[np.arange(B), rng.integers(0, S, size=B)].copy()
        w = rng.uniform(0.1, 10.0, size=m.nv)
        plain_r = prob.solve_multistart(*args, reference=q_ref, weights=w, **kw)
        sets_r = prob.solve_multistart_set(*args, n_solutions=_K, min_distance=_R, reference=q_ref, weights=w, **kw)
        prob.close(); nm.close()
        _solved[name] = (m, args[0], plain, sets, (q_ref, w, plain_r, sets_r))
        for res in (plain, sets, plain_r, sets_r):
            for x in res:
                x.setflags(write=False)
    return _solved[name]


def _assert_slot0(plain, sets, what):
    B, S = plain.q_all.shape[:2]
    for f in ("q_all", "converged_all", "iters_all", "status_all", "seeds"):       # the loops know nothing of the selection
        np.testing.assert_array_equal(getattr(sets, f), getattr(plain, f), err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(sets.n_converged, plain.n_converged, err_msg=what)
    some = plain.n_converged > 0
    for f in ("q", "v", "iters", "status", "seed_index"):
        np.testing.assert_array_equal(getattr(sets, f)[some, 0], getattr(plain, f)[some], err_msg=f"{what}: slot 0: {f}")
    # nothing converged: every slot is empty and repeats what multi-start returns, seed 0's result
    assert (sets.n_distinct[~some] == 0).all() and (sets.seed_index[~some] == -1).all() and (sets.multiplicity[~some] == 0).all()
    assert np.isposinf(sets.distance[~some]).all() and (plain.seed_index[~some] == 0).all()
    for f in ("q", "v", "iters", "status"):
        got, one = getattr(sets, f)[~some], getattr(plain, f)[~some]
        np.testing.assert_array_equal(got, np.repeat(one[:, None], _K, axis=1), err_msg=f"{what}: empty targets: {f}")
    # empty slots of the other targets repeat seed 0's row too; filled ones are rows of the loops
    for b in np.flatnonzero(some):
        for j in range(_K):
            s = sets.seed_index[b, j] if j < sets.n_distinct[b] else 0
            assert (sets.seed_index[b, j] >= 0) == (j < sets.n_distinct[b])
            np.testing.assert_array_equal(sets.q[b, j], plain.q_all[b, s])
            assert sets.iters[b, j] == plain.iters_all[b, s] and sets.status[b, j] == plain.status_all[b, s]
    return int(some.sum())


@pytest.mark.parametrize("name", ["ur5e_far", "shadow_c4", "ballslide"])
def test_slot_zero_is_multistarts_choice_bitwise(nat, name):
    m, q, plain, sets, (q_ref, w, plain_r, sets_r) = _solve_both(nat, name)
    B = len(q)
    n = _assert_slot0(plain, sets, name)
    n_r = _assert_slot0(plain_r, sets_r, name + ", reference= and weights=")
    print(f"{name}: {n} of {B} targets with a converged seed ({n_r} with reference=), n_distinct histogram "
          f"{np.bincount(sets.n_distinct, minlength=_K + 1).tolist()}, with reference= {np.bincount(sets_r.n_distinct, minlength=_K + 1).tolist()}")
    if name == "ur5e_far":
        assert 0 < n < B                                                     # both branches of the invariant
        assert (sets_r.seed_index[:, 0] != sets.seed_index[:, 0]).sum() > 0  # the reference changes the order


# ------------------------------------------------------------------ 3. the rule on solved candidates
def _assert_rule_on_loops(m, sets, q_ref, w, what):
    B, S = sets.q_all.shape[:2]
    excluded = []
    for b in range(B):
        ok = ms.eligible(sets.converged_all[b], sets.status_all[b])
        s = ref.select_cover(m, sets.q_all[b], ok, q_ref[b], _K, _R, w)
        assert int(sets.n_converged[b]) == s.n_eligible
        if ref.near_tie(s, 1e-9):
            excluded.append(b)
            continue
        for f in ("seed_index", "multiplicity"):
            np.testing.assert_array_equal(getattr(sets, f)[b], getattr(s, f), err_msg=f"{what}: target {b}: {f}")
        assert (int(sets.n_distinct[b]), int(sets.n_uncovered[b])) == (s.n_distinct, s.n_uncovered), (what, b)
        filled = np.arange(_K) < s.n_distinct
        np.testing.assert_allclose(sets.distance[b][filled], s.distance[filled], rtol=1e-9)
    print(f"{what}: {len(excluded)} of {B} targets within 1e-9 of a tie: {excluded}")
    assert len(excluded) <= 0.02 * B
    return excluded


def test_selection_on_solved_candidates_is_the_rule(nat):
    """The numpy rule on the device's own q_all / converged_all / status_all of the `ur5e_far` call (B = 96, S = 16, K = 4,
    r = 0.1, rng_seed 8) gives the device's seed_index, multiplicity, n_distinct, n_uncovered for every target none of whose
    decisions lies within a relative 1e-9 of a tie; at most 2 % of the targets may be excluded that way.

    CPU check of this fixture (the C oracle's solve + the numpy oracle's integration and error test, the loop of
    test_gpu_wide.py::_oracle_loop on the seeds of multistart_ref.draw_seeds, rng_seed 8): 628 of
    1 536 loops converge, none fails; 94 targets have a converged seed, 90 more than one; n_distinct is 0 / 1 / 2 / 3 / 4 on
    2 / 4 / 6 / 5 / 79 targets — 90 of 96 hold at least two distinct solutions, against the 24 the test needs —; 7 targets have
    a slot that merges two or more seeds; NO decision of the reference lies within 1e-9 of a tie (the closest: a relative
    6.4e-6), so the 2 % are head-room for the device's own rounding of its own loops, not for this fixture."""
    m, q, plain, sets, (q_ref, w, plain_r, sets_r) = _solve_both(nat, "ur5e_far")
    B = len(q)
    _assert_rule_on_loops(m, sets, q, None, "ur5e_far")
    _assert_rule_on_loops(m, sets_r, q_ref, w, "ur5e_far, reference= and weights=")
    # the fixture exercises the rule: a quarter of the targets hold two distinct branches, and some slot merges seeds
    print(f"n_distinct >= 2 on {int((sets.n_distinct >= 2).sum())} of {B} targets, largest multiplicity {int(sets.multiplicity.max())}, "
          f"n_uncovered > 0 on {int((sets.n_uncovered > 0).sum())}")
    assert (sets.n_distinct >= 2).sum() > B // 4
    assert (sets.multiplicity >= 2).any()
    np.testing.assert_array_equal(sets.multiplicity.sum(axis=1), sets.n_converged - sets.n_uncovered)


# ------------------------------------------------------------------ 4. independence
_KW = dict(damping=1e-3, rng_seed=5, return_all=True)


def _same(other, whole, what):
    for f in whole._fields:
        np.testing.assert_array_equal(_np(getattr(other, f)), getattr(whole, f), err_msg=f"{what}: {f}")


def test_result_does_not_depend_on_chunks_array_kind_or_where_the_seeds_come_from(nat):
    import mink_amd as mink
    import torch
    B, S, K = 40, 8, 3
    m, cfg, tasks, lims, tg = tm._far_ur5e(B)
    whole = mink.solve_ik_solutions(cfg, tasks, 1.0, S, K, 40, 1e-4, 1e-4, limits=lims, **_KW)
    assert list(cfg._problems.values())[-1].max_batch == B * S                  # one chunk
    assert (whole.n_distinct >= 2).sum() > 0 and (whole.multiplicity >= 2).sum() > 0
    for chunks, rows in ((2, 20), (5, 8)):
        _, cfg_c, tasks_c, lims_c, _ = tm._far_ur5e(B)
        part = mink.solve_ik_solutions(cfg_c, tasks_c, 1.0, S, K, 40, 1e-4, 1e-4, limits=lims_c, max_instances=rows * S + 3, **_KW)
        assert list(cfg_c._problems.values())[-1].max_batch == rows * S and -(-B // rows) == chunks
        _same(part, whole, f"{chunks} chunks")
    # the seeds a first call returned, passed back in: the generator is not consulted
    again = mink.solve_ik_solutions(cfg, tasks, 1.0, S, K, 40, 1e-4, 1e-4, limits=lims, seeds=whole.seeds, **{**_KW, "rng_seed": 99})
    _same(again, whole, "seeds=")
    # numpy against torch inputs, one level down (a Configuration holds its q on the host)
    prob = list(cfg._problems.values())[-1]
    q = cfg.q_batch
    args = dict(n_seeds=S, n_solutions=K, min_distance=0.1, max_iters=40, pos_threshold=1e-4, ori_threshold=1e-4, rng_seed=5,
                return_all=True)
    o_np = prob.solve_multistart_set(q, tg[:, None, :], None, None, 1.0, 1e-3, **args)
    dev = torch.device("cuda:0")
    o_t = prob.solve_multistart_set(torch.as_tensor(q, device=dev), torch.as_tensor(np.ascontiguousarray(tg[:, None, :]), device=dev),
                                    None, None, 1.0, 1e-3, **args)
    assert all(isinstance(x, torch.Tensor) and x.device.type == "cuda" for x in o_t)
    _same(o_t, o_np, "torch")
    for f in ("q", "v", "seed_index", "distance", "multiplicity", "n_distinct", "n_converged", "n_uncovered", "q_all"):
        np.testing.assert_array_equal(getattr(o_np, f), getattr(whole, f), err_msg=f)
    # a seed table: slot 0 is what solve_ik_multistart returns with the same table
    table = mink.SeedTable(mink.Configuration(m, cfg.q_batch[0]), tasks, 512, limits=lims)
    try:
        kw = {k: v for k, v in _KW.items() if k != "rng_seed"}
        sets = mink.solve_ik_solutions(cfg, tasks, 1.0, S, K, 40, 1e-4, 1e-4, limits=lims, seed_table=table, rng_seed=1, **kw)
        one = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, limits=lims, seed_table=table, rng_seed=2, update=False, **kw)
        np.testing.assert_array_equal(sets.seeds, one.seeds)
        np.testing.assert_array_equal(sets.q_all, one.q_all)
        some = one.converged
        assert some.any()
        np.testing.assert_array_equal(sets.q[some, 0], one.q[some])
        np.testing.assert_array_equal(sets.seed_index[some, 0], one.seed_index[some])
        np.testing.assert_array_equal(sets.q[~some, 0], one.q[~some])
        np.testing.assert_array_equal(sets.valid[:, 0], some)
    finally:
        table.close()


# ------------------------------------------------------------------ 5. ladder composition
def test_sets_compose_with_the_ladder_search(nat):
    """UR5e, 8 lines of 5 waypoints (the far paths of the ladder tests), 16 seeds, 4 slots: the ladder search over the K
    deduplicated nodes per waypoint tracks as many waypoints as the search over all S loop results — a waypoint with an
    eligible seed keeps at least slot 0."""
    import mink_amd as mink
    B, T, S, K = 8, tms._T5, 16, 4
    m, cfg, task, lims, tg = tms._far_setup(B=B)
    flat = mink.Configuration(m, np.repeat(cfg.q_batch, T, axis=0))
    task.set_target(mink.SE3(tg.reshape(B * T, 7)))
    sets = mink.solve_ik_solutions(flat, [task], 1.0, S, K, 40, 1e-4, 1e-4, limits=lims, damping=1e-3, rng_seed=5, return_all=True)
    eligible = ms.eligible(sets.converged_all, sets.status_all)
    few = mink.ladder_path(cfg, sets.q.reshape(B, T, K, m.nq), sets.valid.reshape(B, T, K))
    full = mink.ladder_path(cfg, sets.q_all.reshape(B, T, S, m.nq), eligible.reshape(B, T, S))
    print(f"far UR5e paths: tracked waypoints {few.n_tracked.tolist()} on {K} nodes, {full.n_tracked.tolist()} on {S}; "
          f"path length {np.round(few.path_length, 3).tolist()} against {np.round(full.path_length, 3).tolist()}")
    np.testing.assert_array_equal(few.n_tracked, full.n_tracked)
    np.testing.assert_array_equal(few.n_tracked, eligible.reshape(B, T, S).any(axis=2).sum(axis=1))
    assert 0 < few.n_tracked.sum() and (sets.n_distinct >= 2).any()


# ------------------------------------------------------------------ 6. public API
def test_public_api(nat):
    import mink_amd as mink
    B, S, K = 32, 6, 3
    m, cfg, tasks, lims, tg = tm._far_ur5e(B)
    home = cfg.q_batch.copy()
    res = mink.solve_ik_solutions(cfg, tasks, 1.0, S, K, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, return_all=True)
    assert isinstance(res, mink.SolutionSet)
    np.testing.assert_array_equal(cfg.q_batch, home)                      # a set never updates the configuration
    assert res.q.shape == (B, K, m.nq) and res.v.shape == (B, K, m.nv) and res.q.dtype == np.float64
    for f, dt in (("valid", bool), ("seed_index", np.int32), ("distance", np.float64), ("multiplicity", np.int32), ("iters", np.int32),
                  ("status", np.int32)):
        assert getattr(res, f).shape == (B, K) and getattr(res, f).dtype == dt, f
    for f in ("n_distinct", "n_converged", "n_uncovered"):
        assert getattr(res, f).shape == (B,) and getattr(res, f).dtype == np.int32, f
    assert res.q_all.shape == (B, S, m.nq) and res.seeds.shape == (B, S, m.nq) and res.converged_all.shape == (B, S)
    assert res.converged_all.dtype == bool and res.iters_all.shape == (B, S) and res.status_all.shape == (B, S)
    np.testing.assert_array_equal(res.valid, res.seed_index >= 0)
    np.testing.assert_array_equal(res.valid.sum(axis=1), res.n_distinct)
    plain = mink.solve_ik_solutions(cfg, tasks, 1.0, S, K, 40, 1e-4, 1e-4, damping=1e-3, limits=lims)
    assert plain.q_all is None and plain.seeds is None and plain.converged_all is None
    np.testing.assert_array_equal(plain.q, res.q)
    # slot 0 is solve_ik_multistart's result
    one = mink.solve_ik_multistart(cfg, tasks, 1.0, S, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, update=False)
    np.testing.assert_array_equal(res.q[:, 0], one.q); np.testing.assert_array_equal(res.valid[:, 0], one.converged)
    # the selection alone over these loops' results is the same set; a larger r merges, r = 0 does not
    alone = mink.distinct_solutions(cfg, res.q_all, ms.eligible(res.converged_all, res.status_all), n_solutions=K, min_distance=0.1)
    assert isinstance(alone, mink.DistinctSet)
    for f in ("q", "valid", "seed_index", "distance", "multiplicity", "n_distinct", "n_uncovered"):
        np.testing.assert_array_equal(getattr(alone, f), getattr(res, f), err_msg=f)
    np.testing.assert_array_equal(alone.n_valid, res.n_converged)
    assert alone.q.shape == (B, K, m.nq) and alone.valid.dtype == bool and alone.n_valid.shape == (B,)
    merged = mink.distinct_solutions(cfg, res.q_all, ms.eligible(res.converged_all, res.status_all), n_solutions=K, min_distance=100.0)
    assert (merged.n_distinct <= 1).all() and (merged.n_uncovered == 0).all()
    np.testing.assert_array_equal(merged.multiplicity[:, 0], res.n_converged)
    np.testing.assert_array_equal(cfg.q_batch, home)
    # an unbatched configuration: unbatched fields
    c1 = mink.Configuration(m, home[0])
    t1 = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0); t1.set_target(mink.SE3(tg[3]))
    r1 = mink.solve_ik_solutions(c1, [t1], 1.0, S, K, 40, 1e-4, 1e-4, damping=1e-3, limits=lims, return_all=True)
    assert r1.q.shape == (K, m.nq) and r1.v.shape == (K, m.nv) and r1.valid.shape == (K,) and r1.q_all.shape == (S, m.nq)
    assert np.ndim(r1.n_distinct) == 0 and r1.converged_all.shape == (S,)
    d1 = mink.distinct_solutions(c1, r1.q_all, n_solutions=2)
    assert d1.q.shape == (2, m.nq) and d1.seed_index.shape == (2,) and np.ndim(d1.n_uncovered) == 0
    np.testing.assert_array_equal(c1.q_batch[0], home[0])
