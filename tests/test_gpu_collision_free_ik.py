"""collision_check= of solve_ik_multistart / solve_ik_solutions / solve_ik_goalset (include/minkhip.h "THE RULE OF CLEARANCE",
"Attached"): the stage behind the loops marks exactly the candidates the numpy reference finds in collision, the selections
then are the existing rules on the marked rows, and what comes out converged is free.

UR5e, a FrameTask on attachment_site, ConfigurationLimit; B = 32 targets, S = 16 seeds, 20 iterations, every loop started at
`home`.  The targets are the end-effector poses of joint rows the reference finds collision-free; the checker is the 14-pair one
(every link capsule against floor and wall, dmin 0.02, detect 0.2)."""

import numpy as np
import pytest

import clearance_ref as cr
import goalset_ref as gsr
import multistart_ref as ms
import solution_set_ref as ssr

pytestmark = pytest.mark.gpu
B, S, ITERS = 32, 16, 20
THR = (1e-4, 1e-4)
KW = dict(damping=1e-3, rng_seed=5, update=False, return_all=True)


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    if _native.lib().mkh_device_count() < 1:
        pytest.skip("no GPU")
    return _native


_state = {}


def _limits():
    return cr.limits_of(cr.fixture_limits("ur5e_all"))


def _free_rows(n, colliding=False):
    model, _, q = cr.fixture("ur5e_all")
    ref = cr.fixture_ref("ur5e_all")
    return q[ref.in_collision == colliding][:n]


def _poses(model, q):
    import mink_amd as mink
    return mink.Configuration(model, q).get_transform_frame_to_world("attachment_site", "site").wxyz_xyz


def _setup(n=B, start=None, targets=None):
    """(model, configuration at `home` (or `start`), task with its targets set, limits, targets (n, 7))."""
    import mink_amd as mink
    model, _, _ = cr.fixture("ur5e_all")
    tg = _poses(model, _free_rows(n)) if targets is None else targets
    home = np.tile(model.key_qpos[model.name2id("key", "home")], (n, 1)) if start is None else start
    cfg = mink.Configuration(model, home)
    task = mink.FrameTask("attachment_site", "site", 1.0, 1.0, lm_damping=1.0)
    task.set_target(mink.SE3(tg))
    return model, cfg, task, [mink.ConfigurationLimit(model)], tg


def _checker(neutral=False):
    import mink_amd as mink
    model, spec, _ = cr.fixture("ur5e_all")
    if neutral:                            # no configuration is closer than −10 m to anything
        spec = [dict(kw, minimum_distance_from_collisions=-10.0) for kw in spec]
    return mink.CollisionChecker(model, [mink.CollisionAvoidanceLimit(model, **kw) for kw in spec], max_rows=4096)


def _multistart(ck=None, **more):
    import mink_amd as mink
    model, cfg, task, lims, _ = _setup()
    return model, cfg, mink.solve_ik_multistart(cfg, [task], 1.0, S, ITERS, *THR, limits=lims, collision_check=ck, **{**KW, **more})


def _plain_and_checked():
    """The plain and the checked multi-start call of this file's set-up, and the reference's verdict on every candidate."""
    if not _state:
        model, cfg, plain = _multistart()
        ck = _checker()
        _, _, checked = _multistart(ck)
        ck.close()
        mask = cr.clearance(model, _limits(), plain.q_all.reshape(B * S, -1)).in_collision.reshape(B, S)
        _state.update(model=model, q_ref=cfg.q_batch.copy(), plain=plain, checked=checked, mask=mask)
    return _state


def _same(a, b, what, skip=()):
    for f in a._fields:
        if f not in skip:
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f"{what}: {f}")


def test_neutral_checker_changes_nothing(nat):
    import mink_amd as mink
    ck = _checker(neutral=True)
    _, _, plain = _multistart()
    _, _, checked = _multistart(ck)
    _same(checked, plain, "multistart")
    model, cfg, task, lims, _ = _setup()
    sets = lambda c: mink.solve_ik_solutions(cfg, [task], 1.0, S, 4, ITERS, *THR, min_distance=0.3, limits=lims, damping=1e-3, rng_seed=5,
                                             return_all=True, collision_check=c)
    _same(sets(ck), sets(None), "solutions")
    G = 2
    goals = np.stack([_poses(model, _free_rows(2 * B)[g::2]) for g in range(G)], axis=1)
    gs = lambda c: mink.solve_ik_goalset(cfg, [task], 1.0, {task: goals}, S // 2, ITERS, *THR, limits=lims, collision_check=c, **KW)
    _same(gs(ck), gs(None), "goalset")
    ck.close()


def test_the_stage_marks_what_the_reference_marks_and_the_selection_is_the_rule(nat):
    st = _plain_and_checked()
    model, plain, checked, mask, q_ref = st["model"], st["plain"], st["checked"], st["mask"], st["q_ref"]
    for f in ("q_all", "iters_all", "converged_all", "seeds"):
        np.testing.assert_array_equal(getattr(checked, f), getattr(plain, f), err_msg=f)
    assert (plain.status_all & 64 == 0).all()
    np.testing.assert_array_equal(checked.status_all, plain.status_all | np.where(mask, 64, 0).astype(plain.status_all.dtype))
    print("multistart: %d of %d candidates marked, %d of them converged" % (mask.sum(), mask.size, (mask & plain.converged_all).sum()))
    assert 0.1 * mask.size <= mask.sum() <= 0.9 * mask.size and (mask & plain.converged_all).sum() >= B // 4
    # the selection: tests/multistart_ref.py on the marked rows
    n_checked_choice = 0
    for b in range(B):
        d = np.array([ms.distance(model, checked.q_all[b, s], q_ref[b]) for s in range(S)])
        s_ref, conv, n_ok = ms.select(d, checked.converged_all[b], checked.status_all[b])
        ok = ms.eligible(checked.converged_all[b], checked.status_all[b])
        assert int(checked.n_converged[b]) == n_ok and bool(checked.converged[b]) == conv
        s = int(checked.seed_index[b])
        np.testing.assert_array_equal(checked.q[b], checked.q_all[b, s])
        assert checked.status[b] == checked.status_all[b, s] and checked.iters[b] == checked.iters_all[b, s]
        if not conv:
            assert s == 0
            continue
        assert ok[s]
        if (np.sort(d[ok])[1:2] > d[ok].min() * (1 + 1e-9) + 1e-12).all():      # (no near-tie: exactly numpy's choice)
            assert s == s_ref
            n_checked_choice += 1
    assert n_checked_choice >= B // 2


def test_solutions_and_goal_sets_compose_the_same_way(nat):
    import mink_amd as mink
    st = _plain_and_checked()
    model, mask, q_ref = st["model"], st["mask"], st["q_ref"]
    ck = _checker()
    # ---- distinct sets: the same loops as multi-start's, so the same marks
    K, r = 4, 0.3
    _, cfg, task, lims, _ = _setup()
    sets = lambda c: mink.solve_ik_solutions(cfg, [task], 1.0, S, K, ITERS, *THR, min_distance=r, limits=lims, damping=1e-3, rng_seed=5,
                                             return_all=True, collision_check=c)
    plain, checked = sets(None), sets(ck)
    for f in ("q_all", "iters_all", "converged_all"):
        np.testing.assert_array_equal(getattr(checked, f), getattr(plain, f), err_msg=f)
    np.testing.assert_array_equal(plain.q_all, st["plain"].q_all)
    np.testing.assert_array_equal(checked.status_all, plain.status_all | np.where(mask, 64, 0).astype(plain.status_all.dtype))
    near = 0
    for b in range(B):
        ok = ms.eligible(checked.converged_all[b], checked.status_all[b])
        sel = ssr.select_cover(model, checked.q_all[b], ok, q_ref[b], K, r)
        assert int(checked.n_converged[b]) == sel.n_eligible
        if ssr.near_tie(sel, 1e-9):
            near += 1
            continue
        np.testing.assert_array_equal(checked.seed_index[b], sel.seed_index)
        np.testing.assert_array_equal(checked.multiplicity[b], sel.multiplicity)
        assert (int(checked.n_distinct[b]), int(checked.n_uncovered[b])) == (sel.n_distinct, sel.n_uncovered)
        for k in range(sel.n_distinct):
            np.testing.assert_array_equal(checked.q[b, k], checked.q_all[b, sel.seed_index[k]])
            assert not mask[b, sel.seed_index[k]]
    assert near <= 2
    # ---- goal sets: two goals per target, eight seeds each
    G, Sg = 2, S // 2
    goals = np.stack([_poses(model, _free_rows(2 * B)[g::2]) for g in range(G)], axis=1)
    gs = lambda c: mink.solve_ik_goalset(cfg, [task], 1.0, {task: goals}, Sg, ITERS, *THR, limits=lims, collision_check=c, **KW)
    plain, checked = gs(None), gs(ck)
    ck.close()
    gmask = cr.clearance(model, _limits(), plain.q_all.reshape(B * G * Sg, -1)).in_collision.reshape(B, G, Sg)
    for f in ("q_all", "iters_all", "converged_all"):
        np.testing.assert_array_equal(getattr(checked, f), getattr(plain, f), err_msg=f)
    np.testing.assert_array_equal(checked.status_all, plain.status_all | np.where(gmask, 64, 0).astype(plain.status_all.dtype))
    assert (gmask & plain.converged_all).sum() >= B // 4
    lost = 0
    for b in range(B):
        d = gsr.d_ref(model, checked.q_all[b], q_ref[b])
        ok = ms.eligible(checked.converged_all[b], checked.status_all[b])
        c = gsr.select(d, ok)
        np.testing.assert_array_equal(checked.n_converged_goal[b], ok.sum(axis=1))
        np.testing.assert_array_equal(checked.reached[b], c.reached)
        assert int(checked.n_reached[b]) == c.n_reached and bool(checked.converged[b]) == c.converged
        lost += int((plain.reached[b] & ~checked.reached[b]).sum())
        g, s = int(checked.goal_index[b]), int(checked.seed_index[b])
        np.testing.assert_array_equal(checked.q[b], checked.q_all[b, max(g, 0), s])
        every = np.sort(np.where(ok, d, np.inf).reshape(-1))
        if c.converged and (every[1:2] > every[0] * (1 + 1e-9) + 1e-12).all():
            assert (g, s) == (c.goal_index, c.seed_index)
    print("goal set: %d of %d candidates marked, %d goals reached only without the checker" % (gmask.sum(), gmask.size, lost))


def test_checked_picks_are_free_where_plain_picks_collide(nat):
    """Seen on the device: 29 of the 32 plain picks converged and the reference finds 5 of them in collision; the checked call
    converges the same 29 targets, none in collision (smallest margin 6.6 mm)."""
    st = _plain_and_checked()
    model, plain, checked = st["model"], st["plain"], st["checked"]
    ref_plain = cr.clearance(model, _limits(), plain.q)
    ref_checked = cr.clearance(model, _limits(), checked.q)
    n_plain = int((ref_plain.in_collision & plain.converged).sum())
    print("plain picks: %d of %d converged, %d of them in collision; checked picks: %d converged, %d in collision, min margin %.3e"
          % (plain.converged.sum(), B, n_plain, checked.converged.sum(), (ref_checked.in_collision & checked.converged).sum(),
             ref_checked.margin[checked.converged].min()))
    assert n_plain >= 3
    assert not (ref_checked.margin[checked.converged] < -1e-9).any()
    differs = plain.converged != checked.converged
    assert (checked.n_converged[differs] == 0).all() and not checked.converged[differs].any()
    assert (checked.n_converged <= plain.n_converged).all()


def test_seed_zero_in_collision_with_one_seed(nat):
    """One seed, started AT a colliding configuration whose own pose is the target: the loop converges at once, into a collision —
    converged = False, the bit in the status, no exception."""
    import mink_amd as mink
    n = 8
    q_c = _free_rows(n, colliding=True)
    model, cfg, task, lims, _ = _setup(n, start=q_c, targets=_poses(cr.fixture("ur5e_all")[0], q_c))
    plain = mink.solve_ik_multistart(cfg, [task], 1.0, 1, ITERS, *THR, limits=lims, **KW)
    assert plain.converged.all() and (plain.status & ~1 == 0).all()
    ck = _checker()
    res = mink.solve_ik_multistart(cfg, [task], 1.0, 1, ITERS, *THR, limits=lims, collision_check=ck, **KW)
    ck.close()
    assert not res.converged.any() and (res.status & 64 != 0).all() and (res.n_converged == 0).all() and (res.seed_index == 0).all()
    np.testing.assert_array_equal(res.q, plain.q)


def test_chunks_do_not_change_the_checked_result(nat):
    st = _plain_and_checked()
    ck = _checker()
    _, _, chunked = _multistart(ck, max_instances=S)           # one target per native call
    ck.close()
    _same(chunked, st["checked"], "max_instances = S")


def test_a_goal_whose_seeds_all_collide_is_not_reached(nat):
    import mink_amd as mink
    n, G = 8, 2
    model = cr.fixture("ur5e_all")[0]
    q_c, q_f = _free_rows(n, colliding=True), _free_rows(n)
    # goal 0: the colliding start's own pose (its one seed converges at once, into the collision); goal 1: a free row's pose
    goals = np.stack([_poses(model, q_c), _poses(model, q_f)], axis=1)
    _, cfg, task, lims, _ = _setup(n, start=q_c, targets=goals[:, 0])
    ck = _checker()
    call = lambda c: mink.solve_ik_goalset(cfg, [task], 1.0, {task: goals}, 1, ITERS, *THR, limits=lims, collision_check=c, **KW)
    plain, res = call(None), call(ck)
    ck.close()
    assert plain.reached[:, 0].all() and (plain.goal_index[plain.converged] == 0).all()
    assert not res.reached[:, 0].any() and (res.n_converged_goal[:, 0] == 0).all() and (res.status_goal[:, 0] & 64 != 0).all()
    np.testing.assert_array_equal(res.n_reached, res.reached.sum(axis=1))
    assert (res.goal_index[res.converged] == 1).all()
    assert not (res.converged & ~res.reached[:, 1]).any()


def test_other_fan_out_calls_refuse_an_attached_checker(nat):
    from mink_amd.api_specs import configuration_limit_desc
    model = cr.fixture("ur5e_all")[0]
    nm = nat.NativeModel(model, 0)
    prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": model.name2id("site", "attachment_site"),
                                               "cost": [1.0] * 6, "gain": 1.0, "lm_damping": 1.0}],
                             configuration_limits=[configuration_limit_desc(model)], max_batch=64)
    ck = _checker()
    handle = ck._handle(nm)
    q = np.tile(model.key_qpos[0], (2, 1))
    tg = np.tile(_poses(model, _free_rows(2))[:, None, None, :], (1, 3, 1, 1))
    kw = dict(n_seeds=4, max_iters=5, pos_threshold=1e-4, ori_threshold=1e-4)
    assert nat.lib().mkh_problem_set_collision_check(prob.handle, handle.handle) == 0
    try:
        with pytest.raises(nat.MinkHipError, match="mkh_solve_trajectory_ladder: a collision checker is attached"):
            prob.solve_trajectory_ladder(q, tg, None, None, 1.0, 1e-3, **kw)
    finally:
        assert nat.lib().mkh_problem_set_collision_check(prob.handle, None) == 0
    out = prob.solve_trajectory_ladder(q, tg, None, None, 1.0, 1e-3, **kw)      # detached: the call as it was
    assert out.q.shape == (2, 3, model.nq)
    # a checker of another model handle is refused
    nm2 = nat.NativeModel(model, 0)
    assert nat.lib().mkh_problem_set_collision_check(prob.handle, ck._handle(nm2).handle) == -1
    assert b"another MkhModel" in nat.lib().mkh_last_error()
    ck.close(); prob.close(); nm.close(); nm2.close()
