"""The fan-out calls across the native rung loop (ms_loops / ms_rungs in minkhip.hip): a handle whose max_batch holds one rung
per chunk, and one that holds two with a tail, give bit for bit what a handle that holds every loop gives — for the fused refined
ladder, for a seed table in front of the ladder and the goal set, and the candidates of the ladder on nodes stay multi-start's
across a chunk boundary.  The far UR5e fixture of tests/test_gpu_ladder_nodes.py at B, T, S = 3, 5, 16."""

import numpy as np
import pytest

import test_gpu_ladder as tl
import test_gpu_ladder_nodes as tn
from test_gpu_ladder_nodes import _same

pytestmark = pytest.mark.gpu
B, T, S = 3, 5, 16
CHUNKED = (S, 2 * S + 5)                      # one rung per chunk; two rungs per chunk and a tail (15 rungs)


@pytest.fixture(scope="module")
def nat():
    from mink_amd import _native
    assert _native.lib().mkh_device_count() >= 1
    return _native


def _same_fields(got, want, what):
    for f in want._fields:
        if getattr(want, f) is not None:
            _same(getattr(got, f), getattr(want, f), f"{what}: {f}")
        else:
            assert getattr(got, f) is None, (what, f)


def test_refined_ladder_across_chunking_and_pointers(nat):
    import torch
    w = tn._far_world(nat, B, T, B * T * S)
    wts = np.random.default_rng(2).uniform(0.5, 2.0, size=w.m.nv)
    kw = tl._kw(w, S, rng_seed=8, weights=wts, max_step_sq=1.0, qvel_dt=0.05, refine=True, return_all=True)
    args = (w.q, w.tg, w.pt, w.ct, w.dt, w.damping)
    dev = torch.device("cuda:0")
    on = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)
    t_args = [on(x) if isinstance(x, np.ndarray) else x for x in args]
    whole = w.prob.solve_trajectory_ladder(*args, **kw)
    kernel = w.prob.last_kernel()
    assert whole.tracked is not None and whole.repaired is not None and whole.refined is not None and whole.qvel is not None
    assert whole.q_all.shape == (B, T, S, w.m.nq) and whole.seeds.shape == (B, T, S, w.m.nq)
    for mb in (B * T * S,) + CHUNKED:
        h = tn._far_world(nat, B, T, mb)
        if mb in CHUNKED:
            _same_fields(h.prob.solve_trajectory_ladder(*args, **kw), whole, f"max_batch = {mb}")
            assert h.prob.last_kernel() == kernel, (mb, h.prob.last_kernel(), kernel)
        tens = h.prob.solve_trajectory_ladder(*t_args, **{**kw, "weights": on(wts)})
        assert all(x is None or (isinstance(x, torch.Tensor) and x.device.type == "cuda") for x in tens)
        _same_fields(tens, whole, f"torch, max_batch = {mb}")
        assert h.prob.last_kernel() == kernel, (mb, h.prob.last_kernel(), kernel)


def test_seed_table_across_chunking(nat):
    w = tn._far_world(nat, B, T, B * T * S)
    table = nat.NativeSeedTable(w.prob, 32, w.q[0], rng_seed=3)
    try:
        kw = tl._kw(w, S, rng_seed=8, return_all=True, seed_table=table)
        args = (w.q, w.tg, w.pt, w.ct, w.dt, w.damping)           # (w.tg as goals: G = T = 5 goals of one frame per target)
        ladder = w.prob.solve_trajectory_ladder(*args, max_step_sq=1.0, **kw)
        goals = w.prob.solve_goalset(*args, **kw)
        assert ladder.seeds.shape == (B, T, S, w.m.nq) and goals.seeds.shape == (B, T, S, w.m.nq)
        _same(goals.seeds, ladder.seeds, "the goal set's starts are the ladder's: one table, the same (B·5) targets")
        drawn = w.prob.solve_trajectory_ladder(*args, max_step_sq=1.0, **{**kw, "seed_table": None})
        assert (ladder.seeds.view(np.int64) != drawn.seeds.view(np.int64)).any()      # the table was used
        for mb in CHUNKED:
            h = tn._far_world(nat, B, T, mb)
            _same_fields(h.prob.solve_trajectory_ladder(*args, max_step_sq=1.0, **kw), ladder, f"ladder, max_batch = {mb}")
            _same_fields(h.prob.solve_goalset(*args, **kw), goals, f"goal set, max_batch = {mb}")
    finally:
        table.close()


def test_candidates_of_the_nodes_are_multistarts_across_a_chunk_boundary(nat):
    K = 4
    w = tn._far_world(nat, B, T, B * T * S)
    h = tn._far_world(nat, B, T, 2 * S + 5)
    args = (w.q, w.tg, w.pt, w.ct, w.dt, w.damping)
    t0 = 2                                                        # (rows of a sharded caller: the draws sit at t0 * T + rung)
    got = h.prob.solve_trajectory_ladder_nodes(*args, n_nodes=K, return_all=True, unwind_turns=False, rng_seed=8, target_index0=t0,
                                               **tl._kw(w, S))
    ms = w.prob.solve_multistart(np.repeat(w.q, T, axis=0), w.tg.reshape(B * T, *w.tg.shape[2:]), w.pt, w.ct, w.dt, w.damping,
                                 rng_seed=8, target_index0=t0 * T, return_all=True, **tl._kw(w, S))
    _same(got.seeds.reshape(B * T, S, w.m.nq), ms.seeds, "seeds")
    some = ms.n_converged > 0
    assert some.any(), ms.n_converged
    slot0 = got.node_seed_index[:, :, 0].ravel()
    np.testing.assert_array_equal(slot0[some], ms.seed_index[some])
    assert (slot0[~some] == -1).all()
    np.testing.assert_array_equal(got.n_converged.ravel(), ms.n_converged)
