"""Problem handles give their device memory back.

mkh_problem_create uploads a plan into memory the handle owns (minkhip.hip upload_problem: the descriptors' arrays in one owned
list, the buffers calls read by name); mkh_problem_destroy must release all of it.  One problem per kernel family: create, solve
64 instances, destroy — the device's free memory around the first handle is its footprint as the runtime sees it, and 32 more
cycles may not lose 8 of those (a handle that leaks its descriptors loses 32; the margin is for other tenants of a shared card and
the allocator's granularity)."""

import ctypes

import numpy as np
import pytest

import native_configs as nc
import random_models as rm
from mink_amd import _native as nat
from mink_amd import mjcf, workloads

pytestmark = pytest.mark.gpu
B = 64


def _free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return int(free.value)


def _ur5e_c2():
    model = workloads.load_robot("ur5e")
    nm = nat.NativeModel(model)
    make = lambda: nc.build("ur5e_c2", nm, B)[0]
    prob = make()
    q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(3), B, base_q=model.key_qpos[model.name2id("key", "home")])
    prob.close()
    return nm, make, (q, tg, np.array(model.qpos0)[None, :], None, 2e-3, 1e-3), "ik_quad_kernel"     # (the row kernel reads the lane / row descriptor)


def _ur5e_capsules():
    model = workloads.load_robot("ur5e")
    nm = nat.NativeModel(model)
    caps = [g for g in range(model.ngeom) if int(model.geom_type[g]) == 3]
    by_body = {int(model.geom_bodyid[g]): g for g in caps}
    bodies = sorted(by_body)
    pairs = [[by_body[bodies[0]], by_body[bodies[-1]]], [by_body[bodies[1]], by_body[bodies[-1]]]]     # upper arm / forearm against the wrist
    col = {"geom_id_pairs": pairs, "gain": 0.85, "minimum_distance_from_collisions": 0.005,
           "collision_detection_distance": 0.3, "bound_relaxation": 0.0}
    make = lambda: nat.NativeProblem(nm, frame_tasks=[nc._ft(model, "attachment_site", "site", 1.0, 1.0, 1.0)],
                                     posture_tasks=[{"cost": 1e-2}], configuration_limits=[nc._cfg_limit(model)],
                                     velocity_limits=[nc._vel_limit(model)], collision_limits=[col], max_batch=B)
    prob = make()
    q, tg = workloads.make_batch(model, nm, prob, np.random.default_rng(4), B, base_q=model.key_qpos[model.name2id("key", "home")])
    prob.close()
    return nm, make, (q, tg, np.array(model.qpos0)[None, :], None, 2e-3, 1e-3), "+wide"


def _ur5e_convex():
    name = "ur5e_convex"
    model = workloads.load_bench_robot(name)
    nm = nat.NativeModel(model)
    prob, dt, damping = workloads.bench_config(name, model, nm, B)
    q, tg, pt, _ = workloads.bench_batch(name, model, nm, prob, np.random.default_rng(5), B)
    prob.close()
    return nm, (lambda: workloads.bench_config(name, model, nm, B)[0]), (q, tg, pt, None, dt, damping), "136+wide"     # (below 32 768 pair evaluations the in-kernel routine runs; the split's buffers exist all the same)


def _ball_chain():
    xml, sites = rm.ball_chain_mjcf()
    model = mjcf.loads_mjcf(xml)
    assert model.nv == 68
    nm = nat.NativeModel(model)
    cost = [1.0, 1.0, 1.0, 0.3, 0.3, 0.3]
    fts = [{"frame_type": "site", "frame_id": model.name2id("site", s), "cost": cost, "gain": 1.0, "lm_damping": 0.5} for s in sites]
    make = lambda: nat.NativeProblem(nm, frame_tasks=fts, posture_tasks=[{"cost": 0.05}],
                                     velocity_limits=[{"indices": np.arange(model.nv), "limit": np.full(model.nv, 1.0)}], max_batch=B)
    rng = np.random.default_rng(6)
    q = np.array([rm.rand_q(model, rng) for _ in range(B)])
    prob = make()
    _, tg = workloads.make_batch(model, nm, prob, rng, B, base_q=np.array(model.qpos0))
    prob.close()
    return nm, make, (q, tg, np.array(model.qpos0)[None, :], None, 1e-2, 1e-3), "ik_wide_kernel"


@pytest.mark.parametrize("setup", [_ur5e_c2, _ur5e_capsules, _ur5e_convex, _ball_chain], ids=lambda f: f.__name__.lstrip("_"))
def test_create_solve_destroy_gives_the_memory_back(setup):
    nm, make, (q, tg, pt, ct, dt, damping), kernel = setup()
    free0 = _free_bytes()
    prob = make()
    v, st = prob.solve(q, tg, pt, ct, dt, damping)
    assert kernel in prob.last_kernel(), prob.last_kernel()
    footprint = free0 - _free_bytes()
    prob.close()
    free1 = _free_bytes()
    # the same descriptor on a second handle: the same plan, the same upload, the same bits
    other = make()
    v2, st2 = other.solve(q, tg, pt, ct, dt, damping)
    other.close()
    assert np.array_equal(v, v2) and np.array_equal(st, st2)
    for _ in range(31):
        p = make()
        p.solve(q, tg, pt, ct, dt, damping)
        p.close()
    lost = free1 - _free_bytes()
    print("%s: footprint %d B, free memory after the first destroy %+d B, lost over 32 more cycles %d B"
          % (kernel, footprint, free1 - free0, lost))
    if footprint <= 0:
        print("no comparison: the first handle's footprint read as %d B (another tenant freed memory meanwhile)" % footprint)
        return
    assert lost < 8 * footprint, (lost, footprint)
