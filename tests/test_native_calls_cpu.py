"""What every fan-out method of NativeProblem hands to libminkhip, pinned without a device.

`nat.lib` is replaced by a recorder whose every mkh_* returns 0 (the two create calls write a non-null handle), and each method
is called once per mode on the UR5e (nq = nv = 6, one frame task, one posture task) with numpy inputs of pairwise distinct
sizes — B = 2, T = 3, 4 nodes / solutions, G = 5, 8 keyframes, 9 seeds — so that a swapped axis or a swapped pair of output
arrays shows.  Per call the record holds the native function's name, every scalar argument, the flags, every number field of
every IO struct and every pointer as `null`, `in:<argument>` (the caller's own array), `out:<result field>` (an array that
comes back) or `copy` (an array the binding made: converted flags, a default), and per result field None or (shape, dtype).

The expectations, tests/golden/native_calls.json, were written by this file's recorder on the commit BEFORE the Python side of
these calls was refactored (`python tests/test_native_calls_cpu.py <that checkout> <json>`); they are never regenerated from
the code under test.  The device-pointer kind (torch tensors) cannot run without a GPU: this file covers host arrays only.
"""

import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "native_calls.json")
B, T, N, G, KF, S = 2, 3, 4, 5, 8, 9
POINTER_FLOOR = 1 << 22          # every scalar of the scenarios lies far below, every address of the process above


class _Recorder:
    """Stands in for the CDLL: every function records (name, raw arguments) and returns 0."""

    def __init__(self):
        self.calls, self.n_handles = [], 0

    def __getattr__(self, name):
        if not name.startswith("mkh_"):
            raise AttributeError(name)

        def call(*args):
            if name.endswith("_create") or name.endswith("_create_diag"):
                self.n_handles += 1
                args[-1]._obj.value = self.n_handles          # C.byref(handle)
                return 0
            if name.endswith("_destroy"):
                return None
            self.calls.append((name, [self._raw(a) for a in args]))
            return 0

        return call

    @staticmethod
    def _raw(a):
        """An argument as it is at call time: structs by value, the rest as they are."""
        obj = getattr(a, "_obj", None)
        if isinstance(obj, C.Structure):
            return {"struct": type(obj).__name__,
                    "fields": [(n, t is C.c_void_p, getattr(obj, n)) for n, t in obj._fields_]}
        if isinstance(a, C.c_void_p):
            return {"handle": a.value}
        return a


def _flatten(res, prefix=""):
    """{dotted field name: array or None} of a result: NamedTuples by field, plain tuples by position."""
    out = {}
    names = getattr(res, "_fields", None) or [str(i) for i in range(len(res))]
    for n, x in zip(names, res):
        if isinstance(x, tuple):
            out.update(_flatten(x, prefix + n + "."))
        else:
            out[prefix + n] = x
    return out


def _base_address(x):
    return x.__array_interface__["data"][0]


def _describe(calls, inputs, result):
    fields = _flatten(result)
    where = {}
    for n, x in inputs.items():
        where.setdefault(_base_address(x), "in:" + n)
    for n, x in fields.items():
        if x is not None:
            where[_base_address(x)] = "out:" + n

    def pointer(v):
        return "null" if v is None else where.get(v, "copy")

    def arg(a):
        if isinstance(a, dict) and "struct" in a:
            return {a["struct"]: {n: pointer(v) if is_ptr else v for n, is_ptr, v in a["fields"]}}
        if isinstance(a, dict):
            return "handle:%s" % a["handle"]
        if a is None:
            return "null"
        if isinstance(a, int) and not isinstance(a, bool) and a >= POINTER_FLOOR:
            return pointer(a)
        return a

    return {"calls": [[name, [arg(a) for a in args]] for name, args in calls],
            "result": {n: None if x is None else [list(x.shape), str(x.dtype)] for n, x in fields.items()}}


def _scenarios():
    """[(label, method name, keyword arguments)]; `checker` stands for the checker handle."""
    rng = np.random.default_rng(5)
    f = lambda *shape: np.ascontiguousarray(rng.normal(size=shape))
    flags = lambda *shape: rng.integers(0, 2, size=shape).astype(bool)
    nq = nv = 6
    loop = dict(max_iters=7, pos_threshold=1e-3, ori_threshold=2e-3)
    drawn = dict(n_seeds=S, rng_seed=11, target_index0=13, dt=0.02, damping=1e-6)
    one = dict(q=f(B, nq), frame_targets=f(B, 1, 7))
    many = lambda L: dict(q=f(B, nq), frame_targets=f(B, L, 1, 7))
    out = []
    add = lambda label, method, **kw: out.append((label, method, kw))

    add("multistart", "solve_multistart", **one, posture_target=f(1, nq), **drawn, **loop)
    add("multistart/all", "solve_multistart", **one, posture_target=f(B, 1, nq), **drawn, **loop, return_all=True,
        seeds=f(B, S, nq), reference=f(B, nq), weights=f(nv) ** 2, wave_kernel=True)
    add("set", "solve_multistart_set", **one, posture_target=f(1, nq), **drawn, **loop, n_solutions=N, min_distance=0.25)
    add("set/unwind", "solve_multistart_set", **one, posture_target=f(1, nq), **drawn, **loop, n_solutions=N, return_all=True,
        unwind_turns=True, lane_kernel=True, reference=f(B, nq))
    add("select_distinct", "select_distinct", q_candidates=f(B, S, nq), valid=flags(B, S), reference=f(B, nq), weights=f(nv) ** 2,
        n_solutions=N, min_distance=0.25)
    add("goalset", "solve_goalset", **many(G), posture_target=f(1, nq), **drawn, **loop, goal_cost=f(B, G) ** 2,
        goal_valid=flags(B, G))
    add("goalset/all", "solve_goalset", **many(G), posture_target=f(B, G, 1, nq), **drawn, **loop, return_all=True,
        seeds=f(B, G, S, nq), reference=f(B, nq), weights=f(nv) ** 2, quad_kernel=True)
    add("select_goalset", "select_goalset", q_candidates=f(B, G, S, nq), valid=flags(B, G, S), reference=f(B, nq),
        weights=f(nv) ** 2, goal_cost=f(B, G) ** 2, goal_valid=flags(B, G))
    step = dict(dt=0.02, damping=1e-6, n_steps=7)
    add("trajectory/fixed", "solve_trajectory", **many(T), posture_target=f(1, nq), **step)
    add("trajectory/fixed/time_major", "solve_trajectory", q=f(B, nq), frame_targets=f(T, B, 1, 7), posture_target=f(T, 1, nq),
        **step, time_major=True, qvel_dt=0.5, wave_kernel=True)
    add("trajectory/until", "solve_trajectory", **many(T), posture_target=f(B, T, 1, nq), **step, until=(1e-3, 2e-3), qvel_dt=0.5,
        warm_start=True)
    add("trajectory/until/time_major", "solve_trajectory", q=f(B, nq), frame_targets=f(T, B, 1, 7),
        posture_target=f(T, B, 1, nq), **step, until=(1e-3, 2e-3), time_major=True)
    times = dict(keyframe_times=np.linspace(0.0, 7.0, KF), waypoint_times=np.array([0.5, 1.0, 6.25]))
    add("keyframes", "solve_keyframes", q=f(B, nq), frame_keys=f(B, KF, 1, 7), posture_keys=f(B, KF, 1, nq), **times, **step,
        until=(1e-3, 2e-3), return_targets=True, qvel_dt=0.5)
    add("keyframes/time_major", "solve_keyframes", q=f(B, nq), frame_keys=f(KF, B, 1, 7), posture_keys=f(KF, 1, nq), **times,
        **step, time_major=True, return_targets=True)
    add("keyframes/held", "solve_keyframes", q=f(B, nq), frame_keys=f(B, KF, 1, 7), posture_keys=f(1, nq), **times, **step)
    cands = dict(n_seeds=S, rng_seed=11, target_index0=13, dt=0.02, damping=1e-6, n_steps=7, pos_threshold=1e-3,
                 ori_threshold=2e-3)
    add("trajectory_multistart", "solve_trajectory_multistart", **many(T), posture_target=f(1, nq), **cands)
    add("trajectory_multistart/all", "solve_trajectory_multistart", **many(T), posture_target=f(B, T, 1, nq), **cands,
        return_all=True, seeds=f(B, S, nq), weights=f(nv) ** 2, qvel_dt=0.5, quad_kernel=True)
    add("trajectory_multistart_free", "solve_trajectory_multistart_free", **many(T), posture_target=f(1, nq), **cands,
        checker="checker", edge_samples=10)
    add("trajectory_multistart_free/all", "solve_trajectory_multistart_free", q=f(B, nq), frame_targets=f(T, B, 1, 7),
        posture_target=f(1, nq), **cands, checker="checker", edge_samples=10, return_all=True, time_major=True)
    add("select_trajectory_candidates", "select_trajectory_candidates", q=f(B, nq), q_paths=f(T, B * S, nq),
        tracked=flags(T, B * S), weights=f(nv) ** 2)
    add("select_trajectory_candidates/every", "select_trajectory_candidates", q=f(B, nq), q_paths=f(T, B * S, nq))
    add("select_trajectory_candidates/checker", "select_trajectory_candidates", q=f(B, nq), q_paths=f(T, B * S, nq),
        tracked=flags(T, B * S), checker="checker", edge_samples=10)
    add("select_trajectory_candidates/checker/margins", "select_trajectory_candidates", q=f(B, nq), q_paths=f(T, B * S, nq),
        checker="checker", edge_samples=10, return_margins=True)
    add("ladder_select", "ladder_select", q=f(B, nq), q_nodes=f(B, T, S, nq), tracked=flags(B, T, S), max_step_sq=2.25,
        weights=f(nv) ** 2)
    add("ladder_select/every", "ladder_select", q=f(B, nq), q_nodes=f(B, T, S, nq))
    add("ladder_select_free", "ladder_select_free", q=f(B, nq), q_nodes=f(B, T, S, nq), checker="checker", edge_samples=10)
    add("ladder_select_free/margins", "ladder_select_free", q=f(B, nq), q_nodes=f(B, T, S, nq), checker="checker",
        tracked=flags(B, T, S), max_step_sq=2.25, edge_samples=10, return_margins=True)
    ladder = dict(**drawn, **loop, max_step_sq=2.25)
    add("ladder", "solve_trajectory_ladder", **many(T), posture_target=f(1, nq), **ladder)
    add("ladder/all", "solve_trajectory_ladder", **many(T), posture_target=f(B, T, 1, nq), **ladder, return_all=True,
        seeds=f(B, T, S, nq), weights=f(nv) ** 2, qvel_dt=0.5, wave_kernel=True)
    add("ladder/refine", "solve_trajectory_ladder", **many(T), posture_target=f(1, nq), **ladder, refine=True, qvel_dt=0.5)
    add("ladder_nodes", "solve_trajectory_ladder_nodes", **many(T), posture_target=f(1, nq), **ladder, n_nodes=N,
        min_distance=0.25, return_all=True)
    add("ladder_nodes/refine/unwind", "solve_trajectory_ladder_nodes", **many(T), posture_target=f(1, nq), **ladder, n_nodes=N,
        min_distance=0.25, unwind_turns=True, refine=True, lane_kernel=True)
    for nodes in (False, True):
        for refine in (False, True):
            kw = dict(n_nodes=N, min_distance=0.25, unwind_turns=refine) if nodes else {}
            add("ladder_free" + ("/nodes" if nodes else "") + ("/refine" if refine else ""), "solve_trajectory_ladder_free",
                **many(T), posture_target=f(1, nq), **ladder, checker="checker", edge_samples=10, refine=refine,
                return_all=nodes != refine, **kw)
    path = lambda: dict(q=f(B, nq), q_path=f(B, T, nq), frame_targets=f(B, T, 1, 7), dt=0.02, damping=1e-6, **loop)
    known = lambda: dict(v=f(B, T, nv), status=rng.integers(0, 3, size=(B, T)), iters=rng.integers(0, 7, size=(B, T)),
                         converged=flags(B, T))
    add("ladder_refine", "ladder_refine", **path(), posture_target=f(1, nq), tracked=flags(B, T), max_step_sq=2.25,
        weights=f(nv) ** 2, **known(), quad_kernel=True)
    add("ladder_refine/every", "ladder_refine", **path(), posture_target=f(B, T, 1, nq))
    add("ladder_refine_free", "ladder_refine_free", **path(), posture_target=f(1, nq), checker="checker", edge_samples=10)
    add("ladder_refine_free/known", "ladder_refine_free", **path(), posture_target=f(B, T, 1, nq), checker="checker",
        tracked=flags(B, T), edge_samples=10, max_step_sq=2.25, **known())
    return out


@contextlib.contextmanager
def _recorded(nat):
    """(recorder, problem, checker) with `nat.lib` replaced; the handles are closed before the real one comes back."""
    from mink_amd import workloads

    rec, real = _Recorder(), nat.lib
    nat.lib = lambda: rec
    made = []
    try:
        model = workloads.load_robot("ur5e")
        assert (model.nq, model.nv) == (6, 6)
        nm = nat.NativeModel(model, device=0)
        made.append(nm)
        site = model.name2id("site", "attachment_site")
        prob = nat.NativeProblem(nm, frame_tasks=[{"frame_type": "site", "frame_id": site, "cost": [1.0] * 6, "gain": 1.0,
                                                   "lm_damping": 1.0}], posture_tasks=[{"cost": 1e-2}], max_batch=64)
        made.append(prob)
        pairs = np.array([[0, 1]], dtype=np.int32)
        checker = nat.NativeProblem(nm, collision_limits=[{"geom_id_pairs": pairs, "gain": 0.85, "bound_relaxation": 0.0,
                                                           "minimum_distance_from_collisions": 0.005,
                                                           "collision_detection_distance": 0.3}], max_batch=64)
        made.append(checker)
        yield rec, prob, checker
    finally:
        for x in reversed(made):
            x.close()
        nat.lib = real


def record_all():
    """{label: record} of every scenario, on whichever mink_amd is importable."""
    from mink_amd import _native as nat

    records = {}
    with _recorded(nat) as (rec, prob, checker):
        for label, method, kw in _scenarios():
            inputs = {n: x for n, x in kw.items() if isinstance(x, np.ndarray)}
            kw = {n: checker if isinstance(x, str) and x == "checker" else x for n, x in kw.items()}
            rec.calls = []
            result = getattr(prob, method)(**kw)
            assert label not in records
            records[label] = _describe(rec.calls, inputs, result if isinstance(result, tuple) else (result,))
    return json.loads(json.dumps(records))


def test_every_native_call_is_the_recorded_one():
    got = record_all()
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert sorted(got) == sorted(want)
    for label in want:
        assert got[label]["result"] == want[label]["result"], label
        assert got[label]["calls"] == want[label]["calls"], label
    assert len(want) >= 40


def test_output_tables_name_fields_of_their_structs():
    from mink_amd import _native as nat
    tables = {n: t for n, t in vars(nat).items() if isinstance(t, nat._out)}
    assert len(tables) >= 16, sorted(tables)
    for name, table in tables.items():
        pointers = {n for n, t in table.struct._fields_ if t is C.c_void_p}
        assert set(table) <= pointers, (name, set(table) - pointers)
        assert all(dtype in (np.float64, np.int32) for _, dtype, _ in table.values()), name


if __name__ == "__main__":            # python tests/test_native_calls_cpu.py <checkout whose mink_amd is recorded> <json to write>
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    records = record_all()
    with open(sys.argv[2], "w") as fh:                  # one line per native call and one per result, so that a diff reads
        fh.write("{\n" + ",\n".join(
            '%s: {"calls": [\n  %s],\n "result": %s}' % (json.dumps(label), ",\n  ".join(json.dumps(c, sort_keys=True) for c in r["calls"]),
                                                        json.dumps(r["result"], sort_keys=True))
            for label, r in sorted(records.items())) + "\n}\n")
