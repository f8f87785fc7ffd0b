"""ctypes binding of libminkhip.so (include/minkhip.h).

This is the whole Python↔device boundary: plain pointers and sizes, no torch types.
numpy arrays are passed as host pointers (the library stages them); torch CUDA
tensors are passed as device pointers with MKH_FLAG_DEVICE_PTRS (asynchronous on the
current torch stream).  There is no CPU fallback: if the library or a GPU is missing
every call raises.
"""

from __future__ import annotations

import collections
import itertools
import ctypes as C
import os
import threading
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np

from .flatmodel import FlatModel

# (MKH_LIB_TAG: an experiment build made with MKH_BUILD_TAG, mink_amd/csrc/build.py — same-box A/B runs only)
_LIB_TAG = os.environ.get("MKH_LIB_TAG", "")
_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         f"libminkhip_{_LIB_TAG}.so" if _LIB_TAG else "libminkhip.so")

MKH_OK = 0
FLAG_DEVICE_PTRS, FLAG_POSTURE_BATCHED, FLAG_COM_BATCHED, FLAG_DIRECT_QP, FLAG_WAVE_KERNEL, FLAG_LANE_KERNEL = 1, 2, 4, 8, 16, 32
FLAG_TWO_WAVES = 64
FLAG_WARM_START = 128
FLAG_QUAD_KERNEL = 256
FLAG_FULL_ROWS = 512
FLAG_UNWIND_TURNS = 1024         # solve_multistart_set / solve_trajectory_ladder_nodes only: include/minkhip.h "THE RULE OF THE UNWINDING"
# per-handle diagnostic switches of mkh_problem_create_diag (include/minkhip.h MKH_DIAG_*): parity tests and measurements only
DIAG_NO_WIDE_REDO, DIAG_NO_TIGHT_REDO, DIAG_NO_COLD_REFINE, DIAG_NO_PAIR_CULL = 1, 2, 4, 8
_diag_default = threading.local()


class diag_options:
    """`with diag_options(DIAG_NO_WIDE_REDO): prob = NativeProblem(...)` — every handle created by THIS thread inside the block
    gets these MKH_DIAG_* bits (tests and bench.py build their problems through helper functions; the switch travels in the
    call, not in the process environment).  A `diag=` argument of NativeProblem wins."""

    def __init__(self, bits: int):
        self.bits = int(bits)

    def __enter__(self):
        self.prev = getattr(_diag_default, "bits", 0)
        _diag_default.bits = self.bits
        return self

    def __exit__(self, *exc):
        _diag_default.bits = self.prev
        return False
ST_OUTSIDE_LIMITS, ST_INFEASIBLE, ST_NOT_PD, ST_ITER_LIMIT, ST_ROW_OVERFLOW = 1, 2, 4, 8, 16
ST_IN_COLLISION = 64             # set on a candidate of a fan-out call with a collision checker: include/minkhip.h "THE RULE OF CLEARANCE"
FRAME_TYPE_ID = {"body": 0, "geom": 1, "site": 2}

_pd = C.POINTER(C.c_double)
_pi = C.POINTER(C.c_int32)
_F8, _I4 = np.float64, np.int32
_EVERY_NAMES = {"seeds_out": "seeds"}
_LEADS = ("L", "P", "C")       # axes that stand for several: the (B, T) / (T, B) lead of a trajectory, a keyframed group's
_NONE, _ALL, _MARGINS, _ALONE = frozenset(), frozenset({"all"}), frozenset({"margins"}), frozenset({"alone"})


def _on(names: tuple, *flags) -> frozenset:
    """The switches among `names` whose flag is set: the key of a table's generated function."""
    return frozenset(itertools.compress(names, flags))


class _out(dict):
    """The outputs of one IO struct: field → (axes, dtype, condition), and `names` where the result calls a field otherwise
    than the struct does.  An axis ("B T q") names an entry of the call's sizes, a number stands for itself; a field belongs to
    a call when its condition is None or among the call's switches ("all": return_all, "qvel", "until", ...).

    Allocation, the struct and the result all derive from the table BY NAME, once, when the module is imported: for every set
    of its conditions `make[frozenset of switches]` is a generated straight-line function
        make(empty, ptr, sizes, **struct fields) → (the struct, {result field: array})
    that allocates the fields of that set, points a new struct at them — and at the inputs and numbers passed by keyword — and
    names them as the result does.  A call costs what the same statements written out by hand cost."""

    def __init__(self, struct, fields, names=None):
        super().__init__(fields)
        self.struct, self.names = struct, dict(names or {})
        conditions = sorted({c for _, _, c in fields.values() if c is not None})
        self.make = {}
        for k in range(2 ** len(conditions)):
            on = frozenset(c for i, c in enumerate(conditions) if k >> i & 1)
            self.make[on] = self._generate(on)

    def _generate(self, on):
        def shape(axes):
            lead, rest = (f"sizes[{axes[0]!r}] + ", axes[1:]) if axes[0] in _LEADS else ("", axes)
            return lead + "(" + "".join((a if a.isdigit() else f"sizes[{a!r}]") + ", " for a in rest) + ")"

        fields = [(n, axes.split(), "_F8" if dtype is _F8 else "_I4") for n, (axes, dtype, c) in self.items() if c is None or c in on]
        source = ["def make(empty, ptr, sizes, **fields):"]
        source += [f"    {n} = empty({shape(axes)}, {dtype})" for n, axes, dtype in fields]
        source += ["    return struct(" + "".join(f"{n}=ptr({n}), " for n, _, _ in fields) + "**fields), {" +
                   "".join(f"{self.names.get(n, n)!r}: {n}, " for n, _, _ in fields) + "}"]
        scope = {"struct": self.struct, "_F8": _F8, "_I4": _I4}
        exec("\n".join(source), scope)
        return scope["make"]


def _extended(name, base, own, doc, optional=True, module=__name__):
    """The result type `name`: `base`'s fields in its order and with its defaults, behind them `own` — None by default, or,
    not `optional`, required (`base` then has no defaults either)."""
    defaults = [base._field_defaults[f] for f in base._fields if f in base._field_defaults] + [None] * len(own) if optional else None
    cls = collections.namedtuple(name, base._fields + tuple(own), defaults=defaults, module=module)
    cls.__doc__ = doc
    return cls


class MkhFlatModel(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in ("nq", "nv", "nbody", "njnt", "ngeom", "nsite")]
        + [(n, _pi) for n in ("body_parentid", "body_rootid", "body_jntnum", "body_jntadr",
                              "body_dofnum", "body_dofadr")]
        + [(n, _pd) for n in ("body_pos", "body_quat", "body_ipos", "body_mass", "body_subtreemass")]
        + [(n, _pi) for n in ("jnt_type", "jnt_qposadr", "jnt_dofadr", "jnt_bodyid", "jnt_limited")]
        + [(n, _pd) for n in ("jnt_pos", "jnt_axis", "jnt_range", "qpos0")]
        + [(n, _pi) for n in ("dof_bodyid", "dof_jntid", "dof_parentid", "site_bodyid")]
        + [(n, _pd) for n in ("site_pos", "site_quat")]
        + [(n, _pi) for n in ("geom_bodyid", "geom_type")]
        + [(n, _pd) for n in ("geom_size", "geom_pos", "geom_quat")]
        + [("nmesh", C.c_int32), ("nmeshvert", C.c_int32)]
        + [(n, _pi) for n in ("geom_dataid", "mesh_vertadr", "mesh_vertnum")]
        + [("mesh_vert", _pd)]
    )


class MkhFrameTaskDesc(C.Structure):
    _fields_ = [("frame_type", C.c_int32), ("frame_id", C.c_int32), ("cost", C.c_double * 6),
                ("gain", C.c_double), ("lm_damping", C.c_double), ("root_type", C.c_int32), ("root_id", C.c_int32)]


class MkhPostureTaskDesc(C.Structure):
    _fields_ = [("cost", _pd), ("gain", C.c_double), ("lm_damping", C.c_double)]


class MkhComTaskDesc(C.Structure):
    _fields_ = [("cost", C.c_double * 3), ("gain", C.c_double), ("lm_damping", C.c_double)]


class MkhConfigurationLimitDesc(C.Structure):
    _fields_ = [("gain", C.c_double), ("lower", _pd), ("upper", _pd), ("n_indices", C.c_int32),
                ("indices", _pi)]


class MkhVelocityLimitDesc(C.Structure):
    _fields_ = [("n_indices", C.c_int32), ("indices", _pi), ("limit", _pd)]


class MkhCollisionLimitDesc(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("geom_id_pairs", _pi), ("gain", C.c_double),
                ("minimum_distance_from_collisions", C.c_double),
                ("collision_detection_distance", C.c_double), ("bound_relaxation", C.c_double)]


class MkhDenseTaskDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("cost", _pd), ("gain", C.c_double), ("lm_damping", C.c_double)]


class MkhDenseRows(C.Structure):
    _fields_ = [("task_e", C.c_void_p), ("task_J", C.c_void_p), ("limit_G", C.c_void_p), ("limit_h", C.c_void_p),
                ("limit_lo", C.c_void_p), ("limit_hi", C.c_void_p)]


class MkhProblemDesc(C.Structure):
    _fields_ = [
        ("n_frame_tasks", C.c_int32), ("frame_tasks", C.POINTER(MkhFrameTaskDesc)),
        ("n_posture_tasks", C.c_int32), ("posture_tasks", C.POINTER(MkhPostureTaskDesc)),
        ("n_com_tasks", C.c_int32), ("com_tasks", C.POINTER(MkhComTaskDesc)),
        ("n_configuration_limits", C.c_int32), ("configuration_limits", C.POINTER(MkhConfigurationLimitDesc)),
        ("n_velocity_limits", C.c_int32), ("velocity_limits", C.POINTER(MkhVelocityLimitDesc)),
        ("n_collision_limits", C.c_int32), ("collision_limits", C.POINTER(MkhCollisionLimitDesc)),
        ("n_dense_tasks", C.c_int32), ("dense_tasks", C.POINTER(MkhDenseTaskDesc)),
        ("n_dense_limit_rows", C.c_int32), ("dense_limit_box", C.c_int32),
    ]


MULTISTART_IO_FIELDS = ("seeds", "q_ref", "weights", "q_best", "v_best", "iters", "status", "converged", "seed_index",
                        "n_converged", "q_all", "converged_all", "iters_all", "status_all", "seeds_out")


class MkhMultistartIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MULTISTART_IO_FIELDS]


class MultistartOut(NamedTuple):
    """What NativeProblem.solve_multistart returns (arrays of the caller's kind: numpy or torch).  The *_all fields and
    `seeds` are None unless asked for with return_all."""
    q: object
    v: object
    converged: object
    seed_index: object
    n_converged: object
    iters: object
    status: object
    q_all: object = None
    converged_all: object = None
    iters_all: object = None
    status_all: object = None
    seeds: object = None


_EVERY_SEED = {"q_all": ("B S q", _F8, "all"), "converged_all": ("B S", _I4, "all"), "iters_all": ("B S", _I4, "all"),
               "status_all": ("B S", _I4, "all"), "seeds_out": ("B S q", _F8, "all")}
MULTISTART_OUT = _out(MkhMultistartIO, {
    "q_best": ("B q", _F8, None), "v_best": ("B v", _F8, None), "iters": ("B", _I4, None), "status": ("B", _I4, None),
    "converged": ("B", _I4, None), "seed_index": ("B", _I4, None), "n_converged": ("B", _I4, None), **_EVERY_SEED},
    {"q_best": "q", "v_best": "v", **_EVERY_NAMES})

SOLUTION_SET_MAX_K = 64          # slots per target and candidates per target of a distinct set (include/minkhip.h
SOLUTION_SET_MAX_S = 4096        # "THE RULE OF THE SET")
SOLUTION_SET_IO_FIELDS = ("seeds", "q_ref", "weights", "q_set", "v_set", "iters", "status", "seed_index", "multiplicity",
                          "distance", "n_distinct", "n_converged", "n_uncovered", "q_all", "converged_all", "iters_all",
                          "status_all", "seeds_out")


class MkhSolutionSetIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SOLUTION_SET_IO_FIELDS]


class SolutionSetOut(NamedTuple):
    """What NativeProblem.solve_multistart_set returns (arrays of the caller's kind): per slot `q` (B, K, nq), `v` (B, K, nv),
    `seed_index` (−1: empty slot), `distance`, `multiplicity`, `iters`, `status` (B, K); per target `n_distinct`, `n_converged`,
    `n_uncovered` (B,).  The *_all fields and `seeds` are None unless asked for with return_all."""
    q: object
    v: object
    seed_index: object
    distance: object
    multiplicity: object
    iters: object
    status: object
    n_distinct: object
    n_converged: object
    n_uncovered: object
    q_all: object = None
    converged_all: object = None
    iters_all: object = None
    status_all: object = None
    seeds: object = None


class DistinctOut(NamedTuple):
    """What NativeProblem.select_distinct returns: `q` (B, K, nq), `seed_index`, `distance`, `multiplicity` (B, K), `n_distinct`,
    `n_valid`, `n_uncovered` (B,)."""
    q: object
    seed_index: object
    distance: object
    multiplicity: object
    n_distinct: object
    n_valid: object
    n_uncovered: object


# (mkh_select_distinct fills a part of these fields, and calls n_converged its n_valid: DISTINCT_OUT)
SOLUTION_SET_OUT = _out(MkhSolutionSetIO, {
    "q_set": ("B K q", _F8, None), "v_set": ("B K v", _F8, None), "seed_index": ("B K", _I4, None),
    "distance": ("B K", _F8, None), "multiplicity": ("B K", _I4, None), "iters": ("B K", _I4, None),
    "status": ("B K", _I4, None), "n_distinct": ("B", _I4, None), "n_converged": ("B", _I4, None),
    "n_uncovered": ("B", _I4, None), **_EVERY_SEED}, {"q_set": "q", "v_set": "v", **_EVERY_NAMES})
DISTINCT_OUT = _out(MkhSolutionSetIO, {n: SOLUTION_SET_OUT[n] for n in ("q_set", "seed_index", "distance", "multiplicity", "n_distinct",
                                                                        "n_converged", "n_uncovered")},
                    {"q_set": "q", "n_converged": "n_valid"})


def check_solution_set(K: int, min_distance: float, S: Optional[int] = None) -> None:
    """What mkh_solve_multistart_set / mkh_select_distinct refuse about K, r and S, judged on the host."""
    if not 1 <= K <= SOLUTION_SET_MAX_K:
        raise ValueError(f"n_solutions = {K} must be in 1 ... {SOLUTION_SET_MAX_K}")
    if not (min_distance >= 0.0 and min_distance < float("inf")):
        raise ValueError(f"min_distance = {min_distance} must be >= 0 and finite (0: exact duplicates only)")
    if S is not None and S > SOLUTION_SET_MAX_S:
        raise ValueError(f"{S} candidates per target: a distinct set is selected among at most {SOLUTION_SET_MAX_S}")


GOAL_SET_MAX_ROWS = 2 ** 31 - 1  # B·G·S of one native call (include/minkhip.h "THE RULE OF THE GOAL SET")
GOAL_SET_IO_FIELDS = ("seeds", "q_ref", "weights", "goal_cost", "goal_valid", "q_best", "v_best", "iters", "status", "converged",
                      "goal_index", "seed_index", "n_reached", "score", "q_goal", "v_goal", "iters_goal", "status_goal",
                      "seed_index_goal", "reached", "n_converged_goal", "distance_goal", "q_all", "converged_all", "iters_all",
                      "status_all", "seeds_out")


class MkhGoalSetIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in GOAL_SET_IO_FIELDS]


class GoalSetOut(NamedTuple):
    """What NativeProblem.solve_goalset returns (arrays of the caller's kind): per target `q` (B, nq), `v` (B, nv), `converged`,
    `goal_index` (−1: no valid goal), `seed_index`, `n_reached`, `score` (+inf: nothing reached), `iters`, `status` (B,); per
    goal `q_goal` (B, G, nq), `v_goal` (B, G, nv), `reached`, `seed_index_goal`, `n_converged_goal`, `distance_goal` (+inf: not
    reached), `iters_goal`, `status_goal` (B, G).  The *_all fields, (B, G, S, ·), and `seeds` are None unless asked for with
    return_all."""
    q: object
    v: object
    converged: object
    goal_index: object
    seed_index: object
    n_reached: object
    score: object
    iters: object
    status: object
    q_goal: object
    v_goal: object
    reached: object
    seed_index_goal: object
    n_converged_goal: object
    distance_goal: object
    iters_goal: object
    status_goal: object
    q_all: object = None
    converged_all: object = None
    iters_all: object = None
    status_all: object = None
    seeds: object = None


class GoalSelectOut(NamedTuple):
    """What NativeProblem.select_goalset returns: `q` (B, nq), `converged`, `goal_index`, `seed_index`, `n_reached`, `score`
    (B,), `q_goal` (B, G, nq), `reached`, `seed_index_goal`, `n_valid_goal` (the valid candidates of a goal), `distance_goal`
    (B, G)."""
    q: object
    converged: object
    goal_index: object
    seed_index: object
    n_reached: object
    score: object
    q_goal: object
    reached: object
    seed_index_goal: object
    n_valid_goal: object
    distance_goal: object


# (mkh_select_goalset fills a part of these fields, and calls n_converged_goal its n_valid_goal: GOAL_SELECT_OUT)
GOAL_SET_OUT = _out(MkhGoalSetIO, {
    "q_best": ("B q", _F8, None), "v_best": ("B v", _F8, None), "converged": ("B", _I4, None),
    "goal_index": ("B", _I4, None), "seed_index": ("B", _I4, None), "n_reached": ("B", _I4, None),
    "score": ("B", _F8, None), "iters": ("B", _I4, None), "status": ("B", _I4, None),
    "q_goal": ("B G q", _F8, None), "v_goal": ("B G v", _F8, None), "reached": ("B G", _I4, None),
    "seed_index_goal": ("B G", _I4, None), "n_converged_goal": ("B G", _I4, None), "distance_goal": ("B G", _F8, None),
    "iters_goal": ("B G", _I4, None), "status_goal": ("B G", _I4, None),
    "q_all": ("B G S q", _F8, "all"), "converged_all": ("B G S", _I4, "all"), "iters_all": ("B G S", _I4, "all"),
    "status_all": ("B G S", _I4, "all"), "seeds_out": ("B G S q", _F8, "all")}, {"q_best": "q", "v_best": "v", **_EVERY_NAMES})
GOAL_SELECT_OUT = _out(MkhGoalSetIO, {n: GOAL_SET_OUT[n] for n in ("q_best", "converged", "goal_index", "seed_index", "n_reached", "score",
                                                                   "q_goal", "reached", "seed_index_goal", "n_converged_goal",
                                                                   "distance_goal")},
                       {"q_best": "q", "n_converged_goal": "n_valid_goal"})


def check_goalset_shape(B: int, G: int, S: int) -> None:
    """What mkh_solve_goalset / mkh_select_goalset refuse about the shape of a goal set, judged on the host: the selection keeps
    no per-candidate state, so the only cap is the row count of one call."""
    if G < 1:
        raise ValueError(f"a goal set needs at least one goal: G (n_goals) = {G} must be >= 1")
    if S < 1:
        raise ValueError(f"a goal needs at least one start: S (n_seeds) = {S} must be >= 1")
    if B < 1:
        raise ValueError(f"B = {B} must be >= 1")
    if B * G * S > GOAL_SET_MAX_ROWS:
        raise ValueError(f"B*G*S = {B * G * S} rows in one call: at most {GOAL_SET_MAX_ROWS}")


def _goal_inputs(kit, goal_cost, goal_valid, B: int, G: int):
    """goal_cost (B, G) float64 and goal_valid (B, G) int32 of a native goal-set call in the call's kind, shapes checked; a
    host array's costs are judged here (finite, >= 0), a device tensor's by the rule's NaN clause."""
    goal_cost = kit.prep(kit.want(goal_cost, (B, G), "goal_cost"))
    if goal_cost is not None and not _is_torch(goal_cost) and not (np.isfinite(goal_cost) & (goal_cost >= 0.0)).all():
        raise ValueError("goal_cost must be finite and >= 0")
    return goal_cost, kit.flags01(goal_valid, (B, G), "goal_valid")


TRAJECTORY_IO_FIELDS = ("q_traj", "v_traj", "status", "iters", "converged", "qvel", "waypoint_dt", "posture_per_waypoint",
                        "com_per_waypoint", "time_major")


class MkhTrajectoryIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TRAJECTORY_IO_FIELDS[:6]] + [("waypoint_dt", C.c_double)] + \
        [(n, C.c_int32) for n in TRAJECTORY_IO_FIELDS[7:]]


class TrajectoryOut(NamedTuple):
    """What NativeProblem.solve_trajectory returns (arrays of the caller's kind: numpy or torch), (B, T, ·) — (T, B, ·) with
    time_major.  `iters` / `converged` are None in fixed-count mode, `qvel` unless qvel_dt was given."""
    q: object
    v: object
    status: object
    iters: object = None
    converged: object = None
    qvel: object = None


# (L: the lead of the call, (B, T) or — time_major — (T, B); the three trajectory structs share these fields)
TRAJECTORY_NAMES = {"q_traj": "q", "v_traj": "v", **_EVERY_NAMES}
TRAJECTORY_OUT = _out(MkhTrajectoryIO, {
    "q_traj": ("L q", _F8, None), "v_traj": ("L v", _F8, None), "status": ("L", _I4, None), "iters": ("L", _I4, "until"),
    "converged": ("L", _I4, "until"), "qvel": ("L v", _F8, "qvel")}, TRAJECTORY_NAMES)

KEYFRAME_IO_FIELDS = ("q_traj", "v_traj", "status", "iters", "converged", "qvel", "frame_targets_out", "posture_targets_out",
                      "com_targets_out", "waypoint_dt", "posture_keyframed", "com_keyframed", "time_major")


class MkhKeyframeIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in KEYFRAME_IO_FIELDS[:9]] + [("waypoint_dt", C.c_double)] + \
        [(n, C.c_int32) for n in KEYFRAME_IO_FIELDS[10:]]


class KeyframesOut(NamedTuple):
    """What NativeProblem.solve_keyframes returns: the TrajectoryOut of the T waypoints and, with return_targets, the
    interpolated targets in the layout solve_trajectory takes them in (None for a group that is held or absent)."""
    trajectory: TrajectoryOut
    frame_targets: object = None
    posture_targets: object = None
    com_targets: object = None


# MkhKeyframeIO: TRAJECTORY_OUT and, with return_targets, the interpolated targets of the groups that have keyframes (P, C: the
# lead of a batched group, (T,) of one shared by the batch)
KEYFRAME_OUT = _out(MkhKeyframeIO, {
    **TRAJECTORY_OUT, "frame_targets_out": ("L nf 7", _F8, "frames"), "posture_targets_out": ("P np q", _F8, "postures"),
    "com_targets_out": ("C nc 3", _F8, "coms")},
    {**TRAJECTORY_NAMES, "frame_targets_out": "frame_targets", "posture_targets_out": "posture_targets",
    "com_targets_out": "com_targets"})


TRAJECTORY_MULTISTART_IO_FIELDS = ("seeds", "weights", "q_traj", "v_traj", "status", "iters", "converged", "seed_index", "n_tracked",
                                   "n_complete", "path_length", "qvel", "seeds_out", "q_all", "v_all", "status_all", "iters_all",
                                   "converged_all", "waypoint_dt", "posture_per_waypoint", "com_per_waypoint", "time_major")


class MkhTrajectoryMultistartIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TRAJECTORY_MULTISTART_IO_FIELDS[:18]] + [("waypoint_dt", C.c_double)] + \
        [(n, C.c_int32) for n in TRAJECTORY_MULTISTART_IO_FIELDS[19:]]


class TrajectoryMultistartOut(NamedTuple):
    """What NativeProblem.solve_trajectory_multistart returns (arrays of the caller's kind: numpy or torch).  The chosen
    candidate's trajectory `q`, `v`, `status`, `iters`, `converged` (B, T, ·) — (T, B, ·) with time_major; per instance (B,) the
    chosen `seed_index`, its `n_tracked` waypoints, `n_complete` of the S candidates, its `path_length`; `qvel` unless qvel_dt
    was not given.  With return_all every candidate's results, time-major whatever time_major says — `q_all` (T, B·S, nq),
    `v_all` (T, B·S, nv), `status_all`, `iters_all`, `converged_all` (T, B·S) — and the `seeds` (B·S, nq); None otherwise."""
    q: object
    v: object
    status: object
    iters: object
    converged: object
    seed_index: object
    n_tracked: object
    n_complete: object
    path_length: object
    qvel: object = None
    q_all: object = None
    v_all: object = None
    status_all: object = None
    iters_all: object = None
    converged_all: object = None
    seeds: object = None


# (R = B·S candidate rows; every candidate's arrays are time-major whatever the lead is)
TRAJECTORY_MULTISTART_OUT = _out(MkhTrajectoryMultistartIO, {
    **TRAJECTORY_OUT, "seed_index": ("B", _I4, None), "n_tracked": ("B", _I4, None),
    "n_complete": ("B", _I4, None), "path_length": ("B", _F8, None), "seeds_out": ("R q", _F8, "all"),
    "q_all": ("T R q", _F8, "all"), "v_all": ("T R v", _F8, "all"), "status_all": ("T R", _I4, "all"),
    "iters_all": ("T R", _I4, "all"), "converged_all": ("T R", _I4, "all")}, TRAJECTORY_NAMES)

TRAJECTORY_FREE_IO_FIELDS = ("node_margin", "edge_margin", "edge_collision", "n_edge_collisions", "node_margin_all", "edge_margin_all")
TRAJECTORY_CANDIDATES_IO_FIELDS = ("seed_index", "n_tracked", "n_complete", "path_length", "q_path")


class MkhTrajectoryFreeIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TRAJECTORY_FREE_IO_FIELDS]


class MkhTrajectoryCandidatesIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TRAJECTORY_CANDIDATES_IO_FIELDS]


class TrajectoryFreeOut(NamedTuple):
    """What the checked candidate-tracking calls add (include/minkhip.h "THE RULE, with a checker" of
    mkh_solve_trajectory_multistart), of the chosen candidate: node_margin and edge_margin (B, T) — (T, B) with time_major; entry
    0 of edge_margin +inf, NaN where the edge was not swept —, edge_collision (B, T) int32, n_edge_collisions (B,) int32, and,
    where asked for, every row's node_margin_all and edge_margin_all (T, B·S), always time-major."""
    node_margin: object
    edge_margin: object
    edge_collision: object
    n_edge_collisions: object
    node_margin_all: object = None
    edge_margin_all: object = None


class TrajectoryCandidatesOut(NamedTuple):
    """What NativeProblem.select_trajectory_candidates returns: per instance (B,) the chosen `seed_index`, its `n_tracked`
    waypoints, `n_complete` of the S candidates and its `path_length`; `q` (B, T, nq), the chosen candidate's rows."""
    seed_index: object
    n_tracked: object
    n_complete: object
    path_length: object
    q: object


TRAJECTORY_FREE_OUT = _out(MkhTrajectoryFreeIO, {
    "node_margin": ("L", _F8, None), "edge_margin": ("L", _F8, None), "edge_collision": ("L", _I4, None),
    "n_edge_collisions": ("B", _I4, None), "node_margin_all": ("T R", _F8, "all"),
    "edge_margin_all": ("T R", _F8, "all")})
TRAJECTORY_CANDIDATES_OUT = _out(MkhTrajectoryCandidatesIO, {
    "seed_index": ("B", _I4, None), "n_tracked": ("B", _I4, None), "n_complete": ("B", _I4, None),
    "path_length": ("B", _F8, None), "q_path": ("B T q", _F8, None)}, {"q_path": "q"})

LADDER_MAX_S = 256         # nodes per rung (back-pointers are bytes) and waypoints per path (include/minkhip.h "THE RULE")
LADDER_MAX_T = 65535
LADDER_IO_FIELDS = ("node_index", "n_tracked", "n_breaks", "path_length", "edge_break", "q_path")


class MkhLadderIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LADDER_IO_FIELDS]


class LadderPathOut(NamedTuple):
    """What NativeProblem.ladder_select returns (arrays of the caller's kind): the chosen `node_index` (B, T), per instance
    `n_tracked`, `n_breaks` and `path_length` (B,), `edge_break` (B, T) and the nodes gathered through the path, `q` (B, T, nq)."""
    node_index: object
    n_tracked: object
    n_breaks: object
    path_length: object
    edge_break: object
    q: object


LADDER_OUT = _out(MkhLadderIO, {
    "node_index": ("B T", _I4, None), "n_tracked": ("B", _I4, None), "n_breaks": ("B", _I4, None),
    "path_length": ("B", _F8, None), "edge_break": ("B T", _I4, None), "q_path": ("B T q", _F8, None)}, {"q_path": "q"})


TRAJECTORY_LADDER_IO_FIELDS = ("seeds", "weights", "max_step_sq", "q_traj", "v_traj", "status", "iters", "converged", "node_index",
                               "n_tracked", "n_breaks", "path_length", "edge_break", "qvel", "seeds_out", "q_all", "v_all",
                               "status_all", "iters_all", "converged_all", "waypoint_dt")


class MkhTrajectoryLadderIO(C.Structure):
    _fields_ = [(n, C.c_double if n in ("max_step_sq", "waypoint_dt") else C.c_void_p) for n in TRAJECTORY_LADDER_IO_FIELDS]


class TrajectoryLadderOut(NamedTuple):
    """What NativeProblem.solve_trajectory_ladder returns (arrays of the caller's kind).  The chosen nodes' rows `q`, `v`, `status`,
    `iters`, `converged` (B, T, ·); the search's `node_index`, `edge_break` (B, T), `n_tracked`, `n_breaks`, `path_length` (B,);
    `qvel` unless qvel_dt was not given.  With return_all every node's `q_all` (B, T, S, nq), `v_all` (B, T, S, nv),
    `status_all`, `iters_all`, `converged_all` (B, T, S) and the `seeds` (B, T, S, nq); None otherwise.  With refine the path is
    the refinement's (LadderRefineOut) and `tracked`, `repaired` (B, T), `refined` (B,) are its; None otherwise."""
    q: object
    v: object
    status: object
    iters: object
    converged: object
    node_index: object
    n_tracked: object
    n_breaks: object
    path_length: object
    edge_break: object
    qvel: object = None
    q_all: object = None
    v_all: object = None
    status_all: object = None
    iters_all: object = None
    converged_all: object = None
    seeds: object = None
    tracked: object = None
    repaired: object = None
    refined: object = None


# (W: the nodes of a rung — S, or n_nodes of the ladder on distinct nodes)
TRAJECTORY_LADDER_OUT = _out(MkhTrajectoryLadderIO, {
    "q_traj": ("B T q", _F8, None), "v_traj": ("B T v", _F8, None), "status": ("B T", _I4, None),
    "iters": ("B T", _I4, None), "converged": ("B T", _I4, None), "node_index": ("B T", _I4, None),
    "n_tracked": ("B", _I4, None), "n_breaks": ("B", _I4, None), "path_length": ("B", _F8, None),
    "edge_break": ("B T", _I4, None), "qvel": ("B T v", _F8, "qvel"), "q_all": ("B T W q", _F8, "all"),
    "v_all": ("B T W v", _F8, "all"), "status_all": ("B T W", _I4, "all"), "iters_all": ("B T W", _I4, "all"),
    "converged_all": ("B T W", _I4, "all"), "seeds_out": ("B T S q", _F8, "all")}, TRAJECTORY_NAMES)

LADDER_REFINE_IO_FIELDS = ("weights", "max_step_sq", "q_path_out", "tracked_out", "repaired", "refined", "edge_break", "n_tracked",
                           "n_breaks", "path_length", "v", "status", "iters", "converged")


class MkhLadderRefineIO(C.Structure):
    _fields_ = [(n, C.c_double if n == "max_step_sq" else C.c_void_p) for n in LADDER_REFINE_IO_FIELDS]


class LadderRefineOut(NamedTuple):
    """What NativeProblem.ladder_refine returns (arrays of the caller's kind): the returned path `q` (B, T, nq) with its
    `tracked` flags (B, T); `repaired` (B, T): 0 kept, 1 / 2 replaced by the forward / backward sweep; `refined` (B,): 1 where
    the re-tracked path was returned; `edge_break` (B, T), `n_tracked`, `n_breaks`, `path_length` (B,) of the returned path; the
    caller's `v`, `status`, `iters`, `converged` with the rows of repaired nodes replaced by their loops' (None where not passed)."""
    q: object
    tracked: object
    repaired: object
    refined: object
    edge_break: object
    n_tracked: object
    n_breaks: object
    path_length: object
    v: object = None
    status: object = None
    iters: object = None
    converged: object = None


# ("alone": what mkh_ladder_refine itself writes; behind a fused ladder the path's outputs are the ladder struct's.  v, status,
# iters and converged are the caller's in-out arrays: copies of them are put into the struct, nothing is allocated)
LADDER_REFINE_OUT = _out(MkhLadderRefineIO, {
    "q_path_out": ("B T q", _F8, "alone"), "tracked_out": ("B T", _I4, None), "repaired": ("B T", _I4, None),
    "refined": ("B", _I4, None), "edge_break": ("B T", _I4, "alone"), "n_tracked": ("B", _I4, "alone"),
    "n_breaks": ("B", _I4, "alone"), "path_length": ("B", _F8, "alone")}, {"q_path_out": "q", "tracked_out": "tracked"})


def check_ladder_shape(S: int, T: int, max_step_sq: float) -> None:
    """The limits of include/minkhip.h "THE RULE" on a ladder's shape and gate, with no device in sight."""
    if S < 1:
        raise ValueError("a rung needs at least one node: S (n_seeds) must be >= 1")
    if T < 1:
        raise ValueError("a ladder needs at least one waypoint: T must be >= 1")
    if S > LADDER_MAX_S:
        raise ValueError(f"S = {S} nodes per rung: at most {LADDER_MAX_S} (back-pointers are bytes)")
    if T > LADDER_MAX_T:
        raise ValueError(f"T = {T} waypoints: at most {LADDER_MAX_T}")
    if not max_step_sq >= 0.0:
        raise ValueError(f"max_step must be >= 0 (None: no gate), got a squared gate of {max_step_sq}")


LADDER_NODES_IO_FIELDS = ("node_seed_index", "node_multiplicity", "node_distance", "n_distinct", "n_converged", "n_uncovered",
                          "seed_index")


class MkhLadderNodesIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LADDER_NODES_IO_FIELDS]


LADDER_NODES_OUT = _out(MkhLadderNodesIO, {
    "node_seed_index": ("B T K", _I4, None), "node_multiplicity": ("B T K", _I4, None),
    "node_distance": ("B T K", _F8, None), "n_distinct": ("B T", _I4, None), "n_converged": ("B T", _I4, None),
    "n_uncovered": ("B T", _I4, None), "seed_index": ("B T", _I4, None)})
TrajectoryLadderNodesOut = _extended(
    "TrajectoryLadderNodesOut", TrajectoryLadderOut, LADDER_NODES_IO_FIELDS,
    """What NativeProblem.solve_trajectory_ladder_nodes returns (arrays of the caller's kind): TrajectoryLadderOut's fields, in
    its order — with return_all the *_all fields are the NODES' rows, (B, T, K, ·), and `seeds` the (B, T, S, nq) starts — and
    behind them the set's: `node_seed_index`, `node_multiplicity`, `node_distance` (B, T, K), `n_distinct`, `n_converged`,
    `n_uncovered` (B, T), and `seed_index` (B, T), the chosen node's candidate index.""")


def check_ladder_nodes_shape(S: int, K: int, T: int, max_step_sq: float, min_distance: float) -> None:
    """The limits of include/minkhip.h on mkh_solve_trajectory_ladder_nodes' shape, gate and radius, with no device in sight:
    the search's on the K nodes and T, the set's on K, the radius and the S candidates of a rung."""
    if S < 1:
        raise ValueError("a rung needs at least one candidate: n_seeds must be >= 1")
    check_solution_set(K, min_distance, S)
    check_ladder_shape(K, T, max_step_sq)


def check_keyframe_times(key_times, waypoint_times):
    """The checks of include/minkhip.h "THE RULE" on the two time arrays, with no device in sight: float64 (K,) and (T,) arrays, or
    ValueError — key times strictly increasing, waypoint times non-decreasing and inside the keyframes' range, no NaN."""
    try:
        kt = np.ascontiguousarray(key_times, dtype=np.float64)
        wt = np.ascontiguousarray(waypoint_times, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError("keyframe_times and waypoint_times must be arrays of numbers") from e
    if kt.ndim != 1 or kt.size < 1:
        raise ValueError(f"keyframe_times must have shape (K,) with K >= 1, got {kt.shape}")
    if wt.ndim != 1 or wt.size < 1:
        raise ValueError(f"waypoint_times must have shape (T,) with T >= 1, got {wt.shape}")
    if np.isnan(kt).any() or np.isnan(wt).any():
        raise ValueError("keyframe_times / waypoint_times contain NaN")
    if (np.diff(kt) <= 0.0).any():
        raise ValueError("keyframe_times must be strictly increasing")
    if (np.diff(wt) < 0.0).any():
        raise ValueError("waypoint_times must be non-decreasing")
    if wt[0] < kt[0] or wt[-1] > kt[-1]:
        raise ValueError(f"waypoint_times must lie inside the keyframes' range [{kt[0]}, {kt[-1]}]: there is no extrapolation")
    return kt, wt


TAP_NAMES = ("xpos", "xquat", "frame_pose", "subtree_com", "task_e", "task_J", "H", "c", "box_lo",
             "box_hi", "coll_G", "coll_h", "qp_iters", "cycles")


class MkhClearanceIO(C.Structure):
    _fields_ = [("margin", C.c_void_p), ("pair", C.c_void_p), ("n_violated", C.c_void_p), ("distance", C.c_void_p)]


class ClearanceOut(NamedTuple):
    """mkh_clearance of N rows (include/minkhip.h "THE RULE OF CLEARANCE"): margin (N,), pair (N,) int32, n_violated (N,) int32,
    distance (N, n_pairs) or None."""
    margin: object
    pair: object
    n_violated: object
    distance: object = None


class MkhSweptClearanceIO(C.Structure):
    _fields_ = [("margin", C.c_void_p), ("sample", C.c_void_p), ("pair", C.c_void_p)]


class SweptClearanceOut(NamedTuple):
    """mkh_swept_clearance of N edges (include/minkhip.h "THE RULE OF THE SWEEP"): margin (N,), sample (N,) int32, pair (N,) int32."""
    margin: object
    sample: object
    pair: object


CERTIFIED_SWEEP_FIELDS = ("margin", "sample", "pair", "lower_bound", "segment", "bound_pair", "n_samples", "motion", "capped", "verdict")
SWEEP_UNDECIDED, SWEEP_CERTIFIED, SWEEP_COLLIDES = 0, 1, 2     # MKH_SWEEP_*


class MkhCertifiedSweepIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in CERTIFIED_SWEEP_FIELDS]


class CertifiedSweepOut(NamedTuple):
    """mkh_certified_sweep of N edges (include/minkhip.h "THE RULE OF THE CERTIFIED SWEEP"), (N,) each: margin, lower_bound and
    motion float64, the rest int32."""
    margin: object
    sample: object
    pair: object
    lower_bound: object
    segment: object
    bound_pair: object
    n_samples: object
    motion: object
    capped: object
    verdict: object


LADDER_FREE_IO_FIELDS = ("edge_collision", "n_edge_collisions", "edge_margin", "node_margin", "edge_margin_all")


class MkhLadderFreeIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LADDER_FREE_IO_FIELDS]


class LadderFreeOut(NamedTuple):
    """What the checked ladder calls add (include/minkhip.h THE RULE "with a checker"): edge_collision (B, T) int32,
    n_edge_collisions (B,) int32, edge_margin (B, T), and, where asked for, node_margin (B, T, S) and edge_margin_all (B, T, S, S)."""
    edge_collision: object
    n_edge_collisions: object
    edge_margin: object
    node_margin: object = None
    edge_margin_all: object = None


LADDER_FREE_OUT = _out(MkhLadderFreeIO, {
    "edge_collision": ("B T", _I4, None), "n_edge_collisions": ("B", _I4, None), "edge_margin": ("B T", _F8, None),
    "node_margin": ("B T S", _F8, "margins"), "edge_margin_all": ("B T S S", _F8, "margins")})

LADDER_CERTIFIED_IO_FIELDS = ("edge_verdict", "edge_lower_bound", "edge_n_samples", "n_certified", "edge_verdict_all")
EDGE_REJECT_COLLIDING, EDGE_REQUIRE_CERTIFIED = 0, 1     # MKH_EDGE_*


class MkhLadderCertifiedIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LADDER_CERTIFIED_IO_FIELDS]


LadderCertifiedOut = _extended(
    "LadderCertifiedOut", LadderFreeOut, LADDER_CERTIFIED_IO_FIELDS,
    """What the certifying ladder calls add (include/minkhip.h THE RULE "with a certifying checker"): LadderFreeOut's fields in its
    order — edge_collision and n_edge_collisions count what the search blocked, undecided edges included under
    EDGE_REQUIRE_CERTIFIED; edge_margin is the certified sweep's, both ends included —, then of the chosen path edge_verdict (B, T)
    int32 (SWEEP_*, -1: not swept), edge_lower_bound (B, T), edge_n_samples (B, T) int32, n_certified (B,) int32, and, where asked
    for, edge_verdict_all (B, T, S, S) int8.""")
LADDER_CERTIFIED_OUT = _out(MkhLadderCertifiedIO, {
    "edge_verdict": ("B T", _I4, None), "edge_lower_bound": ("B T", _F8, None), "edge_n_samples": ("B T", _I4, None),
    "n_certified": ("B", _I4, None)})       # (edge_verdict_all, bytes, is no entry of a table of doubles and int32: _verdict_bytes)


def _verdict_bytes(kit, cio, proof, B, T, S):
    """edge_verdict_all (B, T, S, S) int8 of the call's kind, into the struct and the result."""
    proof["edge_verdict_all"] = kit.empty((B, T, S, S), np.int8)
    cio.edge_verdict_all = kit.ptr(proof["edge_verdict_all"])


def check_edge_rule(resolution, max_samples) -> None:
    """The certified rule's arguments, with no device in sight (mkh_certified_sweep's checks)."""
    if not (np.isfinite(float(resolution)) and float(resolution) > 0.0):
        raise ValueError(f"edge_resolution must be finite and > 0, got {resolution}")
    if not 1 <= int(max_samples) <= 4096:
        raise ValueError(f"max_edge_samples must be in [1, 4096], got {max_samples}")


LADDER_REFINE_FREE_IO_FIELDS = ("edge_collision", "n_edge_collisions", "edge_margin", "node_margin")


class MkhLadderRefineFreeIO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LADDER_REFINE_FREE_IO_FIELDS]


LADDER_REFINE_FREE_OUT = _out(MkhLadderRefineFreeIO, {
    "edge_collision": ("B T", _I4, None), "n_edge_collisions": ("B", _I4, None),
    "edge_margin": ("B T", _F8, None), "node_margin": ("B T", _F8, None)})
LadderRefineFreeOut = _extended(
    "LadderRefineFreeOut", LadderRefineOut, LADDER_REFINE_FREE_IO_FIELDS,
    """What NativeProblem.ladder_refine_free returns (include/minkhip.h "THE RULE OF THE REFINEMENT, with a checker"):
    LadderRefineOut's fields in its order — `tracked` the EFFECTIVE flags of the returned path —, then of the returned path
    edge_collision (B, T) int32, n_edge_collisions (B,) int32, edge_margin (B, T) (entry 0 +inf, NaN where not swept) and
    node_margin (B, T).""")


class MkhTaps(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TAP_NAMES]


class MinkHipError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load libminkhip.so (built by mink_amd/csrc/build.py).  Fails loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise MinkHipError(
            f"{_LIB_PATH} not found: build it with `python -m mink_amd.csrc.build` "
            "(there is no CPU fallback for the solve path)")
    try:
        # PyTorch-ROCm ships its own libamdhip64; load it first so that the process has ONE HIP
        # runtime (loading /opt/rocm's copy first makes a later torch.cuda init fail with
        # "No HIP GPUs are available").  torch is only plumbing here: memory, streams, RCCL.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_LIB_PATH)
    L.mkh_version.restype = C.c_int32
    L.mkh_last_error.restype = C.c_char_p
    L.mkh_device_count.restype = C.c_int32
    L.mkh_model_create.argtypes = [C.POINTER(MkhFlatModel), C.c_int32, C.POINTER(C.c_void_p)]
    L.mkh_model_destroy.argtypes = [C.c_void_p]
    L.mkh_model_destroy.restype = None
    L.mkh_problem_create.argtypes = [C.c_void_p, C.POINTER(MkhProblemDesc), C.c_int32, C.POINTER(C.c_void_p)]
    L.mkh_problem_create_diag.argtypes = [C.c_void_p, C.POINTER(MkhProblemDesc), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.mkh_problem_create_diag.restype = C.c_int32
    L.mkh_problem_destroy.argtypes = [C.c_void_p]
    L.mkh_problem_destroy.restype = None
    L.mkh_problem_num_task_rows.argtypes = [C.c_void_p]
    L.mkh_problem_num_collision_pairs.argtypes = [C.c_void_p]
    L.mkh_problem_last_kernel.argtypes = [C.c_void_p]
    L.mkh_problem_last_kernel.restype = C.c_char_p
    common = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
              C.c_void_p, C.c_void_p]
    L.mkh_solve.argtypes = common + [C.c_int32, C.c_void_p]
    L.mkh_eval.argtypes = common + [C.POINTER(MkhTaps), C.c_int32, C.c_void_p]
    L.mkh_solve_until.argtypes = common[:8] + [C.c_int32, C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p]
    L.mkh_solve_until.restype = C.c_int32
    L.mkh_solve_multistart.argtypes = common[:8] + [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_uint64, C.c_int64,
                                                    C.POINTER(MkhMultistartIO), C.c_int32, C.c_void_p]
    L.mkh_solve_multistart.restype = C.c_int32
    L.mkh_solve_multistart_set.argtypes = common[:8] + [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double,
                                                        C.c_uint64, C.c_int64, C.POINTER(MkhSolutionSetIO), C.c_int32, C.c_void_p]
    L.mkh_solve_multistart_set.restype = C.c_int32
    L.mkh_select_distinct.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_double, C.POINTER(MkhSolutionSetIO), C.c_int32, C.c_void_p]
    L.mkh_select_distinct.restype = C.c_int32
    L.mkh_solve_goalset.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + common[2:8] + \
        [C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_uint64, C.c_int64, C.POINTER(MkhGoalSetIO), C.c_int32, C.c_void_p]
    L.mkh_solve_goalset.restype = C.c_int32
    L.mkh_select_goalset.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(MkhGoalSetIO), C.c_int32, C.c_void_p]
    L.mkh_select_goalset.restype = C.c_int32
    L.mkh_solve_trajectory.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + common[2:8] + \
        [C.c_int32, C.c_double, C.c_double, C.POINTER(MkhTrajectoryIO), C.c_int32, C.c_void_p]
    L.mkh_solve_trajectory.restype = C.c_int32
    L.mkh_solve_keyframes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + common[2:6] + [C.c_void_p, C.c_void_p] + \
        common[6:8] + [C.c_int32, C.c_double, C.c_double, C.POINTER(MkhKeyframeIO), C.c_int32, C.c_void_p]
    L.mkh_solve_keyframes.restype = C.c_int32
    L.mkh_solve_trajectory_multistart.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + common[2:8] + \
        [C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.POINTER(MkhTrajectoryMultistartIO), C.c_int32, C.c_void_p]
    L.mkh_solve_trajectory_multistart.restype = C.c_int32
    L.mkh_solve_trajectory_multistart_free.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + common[2:8] + \
        [C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(MkhTrajectoryMultistartIO),
         C.POINTER(MkhTrajectoryFreeIO), C.c_int32, C.c_void_p]
    L.mkh_solve_trajectory_multistart_free.restype = C.c_int32
    L.mkh_select_trajectory_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MkhTrajectoryCandidatesIO),
                                                   C.POINTER(MkhTrajectoryFreeIO), C.c_int32, C.c_void_p]
    L.mkh_select_trajectory_candidates.restype = C.c_int32
    L.mkh_ladder_select.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_double, C.POINTER(MkhLadderIO), C.c_int32, C.c_void_p]
    L.mkh_ladder_select.restype = C.c_int32
    L.mkh_solve_trajectory_ladder.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + common[2:8] + \
        [C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.POINTER(MkhTrajectoryLadderIO), C.c_int32, C.c_void_p]
    L.mkh_solve_trajectory_ladder.restype = C.c_int32
    L.mkh_solve_trajectory_ladder_refined.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + common[2:8] + \
        [C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.POINTER(MkhTrajectoryLadderIO), C.POINTER(MkhLadderRefineIO),
         C.c_int32, C.c_void_p]
    L.mkh_solve_trajectory_ladder_refined.restype = C.c_int32
    L.mkh_solve_trajectory_ladder_nodes.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double] + \
        common[2:8] + [C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.POINTER(MkhTrajectoryLadderIO),
                       C.POINTER(MkhLadderNodesIO), C.POINTER(MkhLadderRefineIO), C.c_int32, C.c_void_p]
    L.mkh_solve_trajectory_ladder_nodes.restype = C.c_int32
    L.mkh_unwind_turns.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.mkh_unwind_turns.restype = C.c_int32
    L.mkh_ladder_refine.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p] + common[3:8] + \
        [C.c_int32, C.c_double, C.c_double, C.POINTER(MkhLadderRefineIO), C.c_int32, C.c_void_p]
    L.mkh_ladder_refine.restype = C.c_int32
    L.mkh_solve_dense.argtypes = common[:6] + [C.POINTER(MkhDenseRows), C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                               C.POINTER(MkhTaps), C.c_int32, C.c_void_p]
    L.mkh_solve_dense.restype = C.c_int32
    L.mkh_solve_steps.argtypes = common[:8] + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.mkh_integrate.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                C.c_int32, C.c_void_p]
    L.mkh_lie_eval.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.mkh_lie_eval.restype = C.c_int32
    L.mkh_geom_distance_eval.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mkh_geom_distance_eval.restype = C.c_int32
    L.mkh_problem_launch_info.argtypes = [C.c_void_p, C.c_int32] + [C.POINTER(C.c_int32)] * 4
    L.mkh_seed_table_create.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_void_p)]
    L.mkh_seed_table_destroy.argtypes = [C.c_void_p]
    L.mkh_seed_table_destroy.restype = None
    L.mkh_seed_table_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mkh_seed_table_query.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_int32, C.c_void_p]
    L.mkh_problem_set_seed_table.argtypes = [C.c_void_p, C.c_void_p]
    L.mkh_clearance.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(MkhClearanceIO), C.c_int32, C.c_void_p]
    L.mkh_clearance.restype = C.c_int32
    L.mkh_problem_set_collision_check.argtypes = [C.c_void_p, C.c_void_p]
    L.mkh_problem_set_collision_check.restype = C.c_int32
    L.mkh_swept_clearance.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(MkhSweptClearanceIO),
                                      C.c_int32, C.c_void_p]
    L.mkh_swept_clearance.restype = C.c_int32
    L.mkh_certified_sweep.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32,
                                      C.POINTER(MkhCertifiedSweepIO), C.c_int32, C.c_void_p]
    L.mkh_certified_sweep.restype = C.c_int32
    L.mkh_checker_motion_reach.argtypes = [C.c_void_p, C.c_void_p]
    L.mkh_checker_motion_reach.restype = C.c_int32
    L.mkh_problem_set_sweep_rows.argtypes = [C.c_void_p, C.c_int64]
    L.mkh_problem_set_sweep_rows.restype = C.c_int32
    L.mkh_problem_set_check_rows.argtypes = [C.c_void_p, C.c_int64]
    L.mkh_problem_set_check_rows.restype = C.c_int32
    L.mkh_ladder_select_free.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_double, C.c_int32, C.POINTER(MkhLadderIO), C.POINTER(MkhLadderFreeIO),
                                         C.c_int32, C.c_void_p]
    L.mkh_ladder_select_free.restype = C.c_int32
    L.mkh_solve_trajectory_ladder_free.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double] + \
        common[2:8] + [C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(MkhTrajectoryLadderIO),
                       C.POINTER(MkhLadderNodesIO), C.POINTER(MkhLadderRefineIO), C.POINTER(MkhLadderFreeIO), C.c_int32, C.c_void_p]
    L.mkh_solve_trajectory_ladder_free.restype = C.c_int32
    L.mkh_solve_trajectory_ladder_free_refined.argtypes = L.mkh_solve_trajectory_ladder_free.argtypes
    L.mkh_ladder_select_certified.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                              C.POINTER(MkhLadderIO), C.POINTER(MkhLadderFreeIO), C.POINTER(MkhLadderCertifiedIO),
                                              C.c_int32, C.c_void_p]
    L.mkh_ladder_select_certified.restype = C.c_int32
    L.mkh_solve_trajectory_ladder_certified.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double] + \
        common[2:8] + [C.c_int32, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.c_double, C.c_int32, C.c_int32,
                       C.POINTER(MkhTrajectoryLadderIO), C.POINTER(MkhLadderNodesIO), C.POINTER(MkhLadderRefineIO),
                       C.POINTER(MkhLadderFreeIO), C.POINTER(MkhLadderCertifiedIO), C.c_int32, C.c_void_p]
    L.mkh_solve_trajectory_ladder_certified.restype = C.c_int32
    L.mkh_solve_trajectory_ladder_free_refined.restype = C.c_int32
    L.mkh_ladder_refine_free.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p] + \
        common[3:8] + [C.c_int32, C.c_double, C.c_double, C.c_int32, C.POINTER(MkhLadderRefineIO),
                       C.POINTER(MkhLadderRefineFreeIO), C.c_int32, C.c_void_p]
    L.mkh_ladder_refine_free.restype = C.c_int32
    for f in ("mkh_seed_table_create", "mkh_seed_table_read", "mkh_seed_table_query", "mkh_problem_set_seed_table"):
        getattr(L, f).restype = C.c_int32
    for f in ("mkh_model_create", "mkh_problem_create", "mkh_problem_num_task_rows",
              "mkh_problem_num_collision_pairs", "mkh_solve", "mkh_eval", "mkh_integrate",
              "mkh_problem_launch_info", "mkh_solve_steps"):
        getattr(L, f).restype = C.c_int32
    _lib = L
    return L


EXPORTED_SYMBOLS = (
    "mkh_version", "mkh_last_error", "mkh_device_count", "mkh_model_create", "mkh_model_destroy",
    "mkh_problem_create", "mkh_problem_destroy", "mkh_problem_num_task_rows",
    "mkh_problem_num_collision_pairs", "mkh_solve", "mkh_eval", "mkh_integrate", "mkh_problem_launch_info",
    "mkh_solve_steps", "mkh_problem_last_kernel", "mkh_lie_eval", "mkh_solve_dense", "mkh_solve_until",
    "mkh_geom_distance_eval", "mkh_problem_create_diag", "mkh_solve_multistart",
    "mkh_solve_trajectory", "mkh_solve_keyframes", "mkh_solve_trajectory_multistart",
    "mkh_seed_table_create", "mkh_seed_table_destroy", "mkh_seed_table_read", "mkh_seed_table_query",
    "mkh_problem_set_seed_table", "mkh_ladder_select", "mkh_solve_trajectory_ladder",
    "mkh_ladder_refine", "mkh_solve_trajectory_ladder_refined", "mkh_solve_multistart_set", "mkh_select_distinct",
    "mkh_solve_goalset", "mkh_select_goalset", "mkh_unwind_turns", "mkh_solve_trajectory_ladder_nodes",
    "mkh_clearance", "mkh_problem_set_collision_check",
    "mkh_swept_clearance", "mkh_problem_set_sweep_rows", "mkh_problem_set_check_rows", "mkh_ladder_select_free", "mkh_solve_trajectory_ladder_free",
    "mkh_ladder_refine_free", "mkh_solve_trajectory_ladder_free_refined",
    "mkh_select_trajectory_candidates", "mkh_solve_trajectory_multistart_free",
    "mkh_certified_sweep", "mkh_checker_motion_reach",
    "mkh_ladder_select_certified", "mkh_solve_trajectory_ladder_certified",
)

LIE_OPS = {"se3_log": (0, 7, 0, (6,)), "se3_jlog": (1, 7, 0, (6, 6)), "se3_ljacinv": (2, 6, 0, (6, 6)),
           "se3_multiply": (3, 7, 7, (7,)), "se3_inverse": (4, 7, 0, (7,)), "se3_rminus": (5, 7, 7, (6,)),
           "so3_log": (6, 4, 0, (3,)), "so3_matrix": (7, 4, 0, (3, 3)), "se3_apply": (8, 7, 3, (3,))}


def lie_eval(op: str, a, b=None, device: int = 0) -> np.ndarray:
    """The device SO3/SE3 functions of the hot path over a batch of inputs (mkh_lie_eval; host arrays)."""
    code, na, nb, oshape = LIE_OPS[op]
    a = _f64(a).reshape(-1, na)
    n = len(a)
    if nb:
        b = _f64(b).reshape(-1, nb)
        if len(b) != n:
            raise ValueError("a and b must have the same leading dimension")
    out = np.empty((n,) + oshape)
    _check(lib().mkh_lie_eval(int(device), code, n, a.ctypes.data, b.ctypes.data if nb else None, out.ctypes.data, 0, None))
    return out


def geom_distance_eval(type1, size1, pos1, quat1, type2, size2, pos2, quat2, distmax: float, device: int = 0):
    """mj_geomDistance of n primitive geom pairs on the device routines of the collision phase (mkh_geom_distance_eval):
    types (n,), sizes (n, 3), world positions (n, 3), world quaternions wxyz (n, 4) → dist (n,), fromto (n, 6)."""
    t1 = _f64(type1).reshape(-1, 1)
    n = len(t1)
    rec = np.concatenate([t1, _f64(size1).reshape(n, 3), _f64(pos1).reshape(n, 3), _f64(quat1).reshape(n, 4),
                          _f64(type2).reshape(n, 1), _f64(size2).reshape(n, 3), _f64(pos2).reshape(n, 3),
                          _f64(quat2).reshape(n, 4)], axis=1)
    rec = np.ascontiguousarray(rec)
    dist, fromto = np.empty(n), np.empty((n, 6))
    _check(lib().mkh_geom_distance_eval(int(device), n, rec.ctypes.data, float(distmax), dist.ctypes.data, fromto.ctypes.data, None))
    return dist, fromto


def _check(rc: int) -> None:
    if rc != MKH_OK:
        raise MinkHipError(f"libminkhip error {rc}: {lib().mkh_last_error().decode()}")


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _shape_text(shape) -> str:
    """A shape as a tuple prints, symbolic axes ("B", "T") by their names."""
    return "(" + ", ".join(str(a) for a in shape) + ("," if len(shape) == 1 else "") + ")"


def _host_address(x):
    return None if x is None else x.ctypes.data


def _device_address(x):
    return None if x is None else x.data_ptr()


class _Kit:
    """The argument kit of an outer-loop call, from the kind of its q.  numpy: float64 host arrays, the default stream, no flag;
    torch: float64 tensors on q's device, the current stream's handle, FLAG_DEVICE_PTRS in `devp`.  It unpacks into (prep, empty,
    ptr, stream, devp) for the calls that need no more."""

    def __init__(self, q):
        self.torch, self.dev, self.stream, self.devp = None, None, None, 0
        # ptr(x): the address of an array of the call's kind, None for None; empty(shape, np.float64 | np.int32): an output array
        self.ptr, self.empty = _host_address, np.empty
        if _is_torch(q):
            import torch
            self.torch, self.dev, self.ptr, self.empty = torch, q.device, _device_address, self._device_empty
            self.stream, self.devp = _raw_stream(torch, q.device), FLAG_DEVICE_PTRS

    def __iter__(self):
        return iter((self.prep, self.empty, self.ptr, self.stream, self.devp))

    def prep(self, x):
        """An optional input as a contiguous float64 array of the call's kind."""
        if self.torch is None:
            return None if x is None else _f64(x)
        if x is None or (x.dtype is self.torch.float64 and x.device == self.dev and x.is_contiguous()):
            return x
        return self.torch.as_tensor(x).to(device=self.dev, dtype=self.torch.float64).contiguous()

    def _device_empty(self, shape, dtype):
        t = self.torch
        return t.empty(shape, dtype=t.float64 if dtype is np.float64 else (t.int8 if dtype is np.int8 else t.int32), device=self.dev)

    def ones(self, shape):
        """int32 flags that are all set: "None means every row"."""
        x = self.empty(shape, np.int32)
        x[...] = 1
        return x

    @staticmethod
    def want(x, shape, name, required=False):
        """x, its shape checked: an int axis must match, a named one ("T") takes any size.  None passes unless `required`."""
        if x is None and not required:
            return None
        got = None if x is None else tuple(x.shape)
        if got != shape and (x is None or len(got) != len(shape) or
                             any(a != b for a, b in zip(shape, got) if not isinstance(a, str))):
            raise ValueError(f"{name} must have shape {_shape_text(shape)}, got {got}")
        return x

    def flags01(self, x, shape, name):
        """The caller's flags as a fresh contiguous int32 0 / 1 array of the call's kind (None stays None)."""
        if self.want(x, shape, name) is None:
            return None
        if self.torch is None:
            return _i32(np.asarray(x) != 0)
        return (self.torch.as_tensor(x) != 0).to(device=self.dev, dtype=self.torch.int32).contiguous()

    def i32_copy(self, x, shape, name):
        """A caller's in-out integers as a fresh contiguous int32 array of the call's kind (None stays None)."""
        if self.want(x, shape, name) is None:
            return None
        if self.torch is None:
            return np.array(x, dtype=np.int32, order="C")
        return self.torch.as_tensor(x).to(device=self.dev, dtype=self.torch.int32).contiguous().clone()

    def f64_copy(self, x, shape, name):
        """A caller's in-out reals as a fresh contiguous float64 array of the call's kind (None stays None)."""
        if self.want(x, shape, name) is None:
            return None
        return np.array(x, dtype=np.float64, order="C") if self.torch is None else self.prep(x).clone()


def _call_kit(q) -> _Kit:
    """The kit of a call whose arrays are of q's kind."""
    return _Kit(q)


def _held_or_rows(x, lead: tuple, n: int, w: int, name: str, flag: int, strict: bool = True):
    """The flag bit of a posture / CoM target from its shape: 0 for one target held for the whole call, (n, w); `flag` for one per
    row of the call's lead — (B,), (B, G) or (B, T) —, lead + (n, w).  Any other shape raises — or, not `strict`, returns None for
    the caller to read further."""
    if x is None:
        raise ValueError(f"{name} is required")
    shp = tuple(x.shape)
    if shp == (n, w):
        return 0
    if shp == lead + (n, w):
        return flag
    if strict:
        raise ValueError(f"{name} must have shape {(n, w)} or {lead + (n, w)}, got {shp}")
    return None


def _raw_stream(torch, dev) -> int:
    """hipStream_t of torch's current stream on `dev` (the private accessor costs a tenth of building a Stream object)."""
    try:
        return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())
    except AttributeError:
        return torch.cuda.current_stream(dev).cuda_stream


class NativeModel:
    """Device copy of a FlatModel (mkh_model_create)."""

    def __init__(self, model: FlatModel, device: int = 0):
        self.model = model
        self.device = int(device)
        m = model
        self._keep = {}
        fm = MkhFlatModel()
        for n in ("nq", "nv", "nbody", "njnt", "ngeom", "nsite"):
            setattr(fm, n, int(getattr(m, n)))
        fm.nmesh = int(len(m.mesh_vertnum))
        fm.nmeshvert = int(len(m.mesh_vert))
        for n, ctype in MkhFlatModel._fields_[6:]:
            if n in ("nmesh", "nmeshvert"):
                continue
            arr = getattr(m, n)
            arr = _i32(arr) if ctype is _pi else _f64(arr)
            if arr.size == 0:
                arr = np.zeros(1, dtype=arr.dtype)
            self._keep[n] = arr
            setattr(fm, n, arr.ctypes.data_as(ctype))
        h = C.c_void_p()
        _check(lib().mkh_model_create(C.byref(fm), self.device, C.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            lib().mkh_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def integrate(self, q, v, dt: float, out=None):
        """Configuration.integrate for a batch (mkh_integrate)."""
        if _is_torch(q):
            import torch
            q = q.contiguous(); v = v.contiguous()
            out = torch.empty_like(q) if out is None else out
            stream = torch.cuda.current_stream(q.device).cuda_stream
            _check(lib().mkh_integrate(self.handle, q.shape[0], q.data_ptr(), v.data_ptr(), float(dt),
                                       out.data_ptr(), FLAG_DEVICE_PTRS, stream))
            return out
        q = _f64(q); v = _f64(v)
        out = np.empty_like(q)
        _check(lib().mkh_integrate(self.handle, q.shape[0], q.ctypes.data, v.ctypes.data, float(dt),
                                   out.ctypes.data, 0, None))
        return out


class NativeSeedTable:
    """A seed table on one device (mkh_seed_table_create): `n_entries` postures drawn around `q0` by multi-start's seeding rule
    at (rng_seed, t = j, s = 1) — or the caller's `entries` (N, nq) —, keyed on the world poses of `problem`'s frame-task
    frames.  The table owns its device memory: `problem` may be closed afterwards."""

    def __init__(self, problem: "NativeProblem", n_entries: int, q0=None, *, entries=None, rng_seed: int = 0,
                 position_weight=None, orientation_weight=None):
        m = problem.nmodel.model
        self.device = problem.nmodel.device
        self.nq, self.n_frame = int(m.nq), int(problem.n_frame)
        if entries is not None:
            entries = _f64(entries)
            if entries.ndim != 2 or entries.shape[1] != m.nq or len(entries) < 1:
                raise ValueError(f"entries must have shape (N, {m.nq}) with N >= 1, got {entries.shape}")
            n_entries = len(entries)
        if q0 is not None:
            q0 = _f64(q0)
            if q0.shape != (m.nq,):
                raise ValueError(f"q0 must have shape ({m.nq},), got {q0.shape}")
        elif entries is None:
            raise ValueError("q0 is required when the entries are drawn")
        n_entries = int(n_entries)
        if n_entries < 1:
            raise ValueError("n_entries must be >= 1")
        w = []
        for x, name in ((position_weight, "position_weight"), (orientation_weight, "orientation_weight")):
            if x is not None:
                x = _f64(x)
                if x.shape != (self.n_frame,):
                    raise ValueError(f"{name} must have shape ({self.n_frame},), got {x.shape}")
            w.append(x)
        ptr = lambda x: None if x is None else x.ctypes.data
        h = C.c_void_p()
        with problem._lock:
            _check(lib().mkh_seed_table_create(problem.handle, n_entries, ptr(q0), ptr(entries), int(rng_seed) & (2 ** 64 - 1),
                                               ptr(w[0]), ptr(w[1]), C.byref(h)))
        self.handle = h
        self.n_entries = n_entries

    def close(self):
        if getattr(self, "handle", None):
            lib().mkh_seed_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _native_for(self, problem: "NativeProblem") -> "NativeSeedTable":
        return self

    def read(self):
        """(q (N, nq), poses (N, n_frame, 7)) on the host (mkh_seed_table_read)."""
        q, poses = np.empty((self.n_entries, self.nq)), np.empty((self.n_entries, self.n_frame, 7))
        _check(lib().mkh_seed_table_read(self.handle, q.ctypes.data, poses.ctypes.data))
        return q, poses

    def query(self, frame_targets, k: int):
        """(index (B, k) int32, distance (B, k), q (B, k, nq)) of the k entries nearest to each row of frame_targets
        (B, n_frame, 7), ascending (mkh_seed_table_query).  numpy in → numpy out (synchronous); torch tensors on the table's
        device in → torch tensors out, asynchronous on the current stream."""
        k = int(k)
        prep, empty, ptr, stream, devp = _call_kit(frame_targets)
        ft = prep(frame_targets)
        if ft.ndim != 3 or tuple(ft.shape[1:]) != (self.n_frame, 7) or ft.shape[0] < 1:
            raise ValueError(f"frame_targets must have shape (B, {self.n_frame}, 7) with B >= 1, got {tuple(ft.shape)}")
        if devp and (ft.device.index if ft.device.index is not None else 0) != self.device:
            raise ValueError(f"frame_targets live on {ft.device}, the seed table on device {self.device}")
        B = int(ft.shape[0])
        rows = max(k, 0)
        idx, dist = empty((B, rows), np.int32), empty((B, rows), np.float64)
        slab = empty((B, rows + 1, self.nq), np.float64)
        _check(lib().mkh_seed_table_query(self.handle, B, ptr(ft), k, ptr(idx), ptr(dist), ptr(slab), devp, stream))
        return idx, dist, slab[:, 1:]


class _attached:
    """A seed table attached to a handle for one call (mkh_problem_set_seed_table), detached on the way out."""

    def __init__(self, problem: "NativeProblem", table):
        self.problem = problem
        self.table = None if table is None else table._native_for(problem)

    def __enter__(self):
        if self.table is not None:
            if not self.table.handle:
                raise ValueError("the seed table is closed")
            _check(lib().mkh_problem_set_seed_table(self.problem.handle, self.table.handle))

    def __exit__(self, *exc):
        if self.table is not None:
            lib().mkh_problem_set_seed_table(self.problem.handle, None)


class _with_checker:
    """The locks of a call that takes its checker as an argument (mkh_ladder_select_free, mkh_solve_trajectory_ladder_free,
    mkh_ladder_refine_free, mkh_solve_trajectory_ladder_free_refined, mkh_select_trajectory_candidates,
    mkh_solve_trajectory_multistart_free): the
    problem's first, the checker's second; a problem that checks itself has one."""

    def __init__(self, problem: "NativeProblem", checker: "NativeProblem"):
        self.locks = [problem._lock] + ([checker._lock] if checker is not problem else [])
        self.checker = checker

    def __enter__(self):
        for k in self.locks:
            k.acquire()
        if not self.checker.handle:
            self.__exit__()
            raise ValueError("the collision checker is closed")

    def __exit__(self, *exc):
        for k in reversed(self.locks):
            k.release()


def _checker_handle(problem: "NativeProblem", checker, edge_samples) -> "NativeProblem":
    """The native checker of a checked ladder call on `problem`, judged on the host."""
    if int(edge_samples) < 1:
        raise ValueError(f"edge_samples must be >= 1, got {edge_samples}")
    checker = checker._native_for(problem)
    if checker.nmodel is not problem.nmodel:
        raise ValueError("the checker belongs to another NativeModel than the problem")
    return checker


class _checked:
    """A collision checker attached to a handle for one call (mkh_problem_set_collision_check), detached on the way out.
    `checker`: None, a NativeProblem with collision pairs on the handle's device and model, or an object with
    `_native_for(problem)` that returns one (mink_amd.CollisionChecker).  The checker handle's lock is held for the call: host-pointer
    calls that share a checker from several threads are serialised on it; device-pointer calls are asynchronous, and those that
    share a checker must be ordered by the caller (one stream, or events), as for any handle."""

    def __init__(self, problem: "NativeProblem", checker):
        self.problem = problem
        self.checker = None if checker is None else checker._native_for(problem)

    def __enter__(self):
        if self.checker is not None:
            # the call runs on the checker handle's buffers (its pre-evaluated convex pairs): one call per handle holds for it too.
            # Always the problem's lock first, the checker's second; a problem that checks itself holds its one lock already.
            self.locked = self.checker is not self.problem
            if self.locked:
                self.checker._lock.acquire()
            try:
                if not self.checker.handle:
                    raise ValueError("the collision checker is closed")
                _check(lib().mkh_problem_set_collision_check(self.problem.handle, self.checker.handle))
            except BaseException:
                if self.locked:
                    self.checker._lock.release()
                raise

    def __exit__(self, *exc):
        if self.checker is not None:
            lib().mkh_problem_set_collision_check(self.problem.handle, None)
            if self.locked:
                self.checker._lock.release()


class NativeProblem:
    """Device descriptor of one solve_ik call site (mkh_problem_create)."""

    def __init__(self, nmodel: NativeModel, frame_tasks: Sequence[dict] = (), posture_tasks: Sequence[dict] = (),
                 com_tasks: Sequence[dict] = (), configuration_limits: Sequence[dict] = (),
                 velocity_limits: Sequence[dict] = (), collision_limits: Sequence[dict] = (),
                 max_batch: int = 1, dense_tasks: Sequence[dict] = (), dense_limit_rows: int = 0,
                 dense_limit_box: bool = False, diag: Optional[int] = None):
        self.nmodel = nmodel
        m = nmodel.model
        keep = []
        d = MkhProblemDesc()

        def arr(ctype_struct, items):
            a = (ctype_struct * max(1, len(items)))()
            keep.append(a)
            return a

        ft = arr(MkhFrameTaskDesc, frame_tasks)
        for i, t in enumerate(frame_tasks):
            ft[i].frame_type = FRAME_TYPE_ID[t["frame_type"]]
            ft[i].frame_id = int(t["frame_id"])
            ft[i].cost = (C.c_double * 6)(*[float(x) for x in t["cost"]])
            ft[i].gain = float(t.get("gain", 1.0)); ft[i].lm_damping = float(t.get("lm_damping", 0.0))
            ft[i].root_type = FRAME_TYPE_ID[t["root_type"]] if t.get("root_type") is not None else -1
            ft[i].root_id = int(t.get("root_id", 0))
        pt = arr(MkhPostureTaskDesc, posture_tasks)
        for i, t in enumerate(posture_tasks):
            c = _f64(np.broadcast_to(t["cost"], (m.nv,))); keep.append(c)
            pt[i].cost = c.ctypes.data_as(_pd)
            pt[i].gain = float(t.get("gain", 1.0)); pt[i].lm_damping = float(t.get("lm_damping", 0.0))
        ct = arr(MkhComTaskDesc, com_tasks)
        for i, t in enumerate(com_tasks):
            ct[i].cost = (C.c_double * 3)(*[float(x) for x in np.broadcast_to(t["cost"], (3,))])
            ct[i].gain = float(t.get("gain", 1.0)); ct[i].lm_damping = float(t.get("lm_damping", 0.0))
        cl = arr(MkhConfigurationLimitDesc, configuration_limits)
        for i, t in enumerate(configuration_limits):
            lo, up, idx = _f64(t["lower"]), _f64(t["upper"]), _i32(t["indices"])
            keep += [lo, up, idx]
            cl[i].gain = float(t["gain"]); cl[i].lower = lo.ctypes.data_as(_pd); cl[i].upper = up.ctypes.data_as(_pd)
            cl[i].n_indices = len(idx); cl[i].indices = idx.ctypes.data_as(_pi)
        vl = arr(MkhVelocityLimitDesc, velocity_limits)
        for i, t in enumerate(velocity_limits):
            idx, lim = _i32(t["indices"]), _f64(t["limit"])
            keep += [idx, lim]
            vl[i].n_indices = len(idx); vl[i].indices = idx.ctypes.data_as(_pi); vl[i].limit = lim.ctypes.data_as(_pd)
        co = arr(MkhCollisionLimitDesc, collision_limits)
        for i, t in enumerate(collision_limits):
            pairs = _i32(np.asarray(t["geom_id_pairs"]).reshape(-1, 2)); keep.append(pairs)
            co[i].n_pairs = len(pairs); co[i].geom_id_pairs = pairs.ctypes.data_as(_pi)
            co[i].gain = float(t["gain"])
            co[i].minimum_distance_from_collisions = float(t["minimum_distance_from_collisions"])
            co[i].collision_detection_distance = float(t["collision_detection_distance"])
            co[i].bound_relaxation = float(t["bound_relaxation"])
        d.n_frame_tasks, d.frame_tasks = len(frame_tasks), ft
        d.n_posture_tasks, d.posture_tasks = len(posture_tasks), pt
        d.n_com_tasks, d.com_tasks = len(com_tasks), ct
        d.n_configuration_limits, d.configuration_limits = len(configuration_limits), cl
        d.n_velocity_limits, d.velocity_limits = len(velocity_limits), vl
        d.n_collision_limits, d.collision_limits = len(collision_limits), co
        dn = arr(MkhDenseTaskDesc, dense_tasks)
        for i, t in enumerate(dense_tasks):
            c = _f64(np.atleast_1d(t["cost"])); keep.append(c)
            dn[i].k = len(c); dn[i].cost = c.ctypes.data_as(_pd)
            dn[i].gain = float(t.get("gain", 1.0)); dn[i].lm_damping = float(t.get("lm_damping", 0.0))
        d.n_dense_tasks, d.dense_tasks = len(dense_tasks), dn
        d.n_dense_limit_rows = int(dense_limit_rows)
        d.dense_limit_box = 1 if dense_limit_box else 0
        self.dense_limit_box = bool(dense_limit_box)
        self.n_dense_rows = int(sum(len(np.atleast_1d(t["cost"])) for t in dense_tasks))
        self.n_dense_limit_rows = int(dense_limit_rows)
        h = C.c_void_p()
        # (diag: DIAG_* bits — which launches stand behind this handle; 0 = the product's own choice, mkh_problem_create)
        if diag is None:
            diag = getattr(_diag_default, "bits", 0)
        self.diag = int(diag)
        if diag:
            _check(lib().mkh_problem_create_diag(nmodel.handle, C.byref(d), int(max_batch), int(diag), C.byref(h)))
        else:
            _check(lib().mkh_problem_create(nmodel.handle, C.byref(d), int(max_batch), C.byref(h)))
        self.handle = h
        # one in-flight call per handle (it owns the staging buffers and the ticket counter): host-pointer calls are
        # synchronous, so a lock makes them safe from several threads; device-pointer calls are asynchronous and must
        # be ordered by the caller (same stream or events) — include/minkhip.h
        self._lock = threading.Lock()
        self.max_batch = int(max_batch)
        self.n_frame, self.n_posture, self.n_com = len(frame_tasks), len(posture_tasks), len(com_tasks)
        self.n_rows = lib().mkh_problem_num_task_rows(h)
        self.n_pairs = lib().mkh_problem_num_collision_pairs(h)

    def close(self):
        if getattr(self, "handle", None):
            lib().mkh_problem_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _native_for(self, problem: "NativeProblem") -> "NativeProblem":
        return self

    def clearance(self, q_rows, return_distances: bool = False) -> ClearanceOut:
        """mkh_clearance with this handle as the checker: q_rows (N, nq) → margin (N,), pair (N,), n_violated (N,) and, asked
        for, distance (N, n_pairs) — include/minkhip.h "THE RULE OF CLEARANCE".  Any N: the rows are walked in chunks of
        max_batch.  numpy in → numpy out (synchronous); a torch CUDA tensor in → torch tensors out, asynchronous on the
        current stream, no host copy."""
        m = self.nmodel.model
        prep, empty, ptr, stream, devp = _call_kit(q_rows)
        q_rows = prep(q_rows)
        if len(q_rows.shape) != 2 or int(q_rows.shape[1]) != m.nq or int(q_rows.shape[0]) < 1:
            raise ValueError(f"q_rows must have shape (N, {m.nq}) with N >= 1, got {tuple(q_rows.shape)}")
        if devp and (q_rows.device.index if q_rows.device.index is not None else 0) != self.nmodel.device:
            raise ValueError(f"q_rows live on {q_rows.device}, the checker on device {self.nmodel.device}")
        N = int(q_rows.shape[0])
        out = ClearanceOut(empty((N,), np.float64), empty((N,), np.int32), empty((N,), np.int32),
                           empty((N, self.n_pairs), np.float64) if return_distances else None)
        io = MkhClearanceIO(ptr(out.margin), ptr(out.pair), ptr(out.n_violated), ptr(out.distance))
        with self._lock:
            _check(lib().mkh_clearance(self.handle, N, ptr(q_rows), C.byref(io), devp, stream))
        return out

    def swept_clearance(self, q_from, q_to, n_samples: int = 8) -> SweptClearanceOut:
        """mkh_swept_clearance with this handle as the checker: the edges from q_from (N, nq) to q_to (N, nq), `n_samples`
        interior samples each → margin (N,), sample (N,), pair (N,) — include/minkhip.h "THE RULE OF THE SWEEP".  numpy in →
        numpy out (synchronous); torch CUDA tensors in → torch tensors out, asynchronous on the current stream."""
        m = self.nmodel.model
        if int(n_samples) < 1:
            raise ValueError(f"n_samples must be >= 1, got {n_samples}")
        prep, empty, ptr, stream, devp = _call_kit(q_from)
        q_from, q_to = prep(q_from), prep(q_to)
        if len(q_from.shape) != 2 or int(q_from.shape[1]) != m.nq or int(q_from.shape[0]) < 1:
            raise ValueError(f"q_from must have shape (N, {m.nq}) with N >= 1, got {tuple(q_from.shape)}")
        if tuple(q_to.shape) != tuple(q_from.shape):
            raise ValueError(f"q_to must have q_from's shape {tuple(q_from.shape)}, got {tuple(q_to.shape)}")
        N = int(q_from.shape[0])
        out = SweptClearanceOut(empty((N,), np.float64), empty((N,), np.int32), empty((N,), np.int32))
        io = MkhSweptClearanceIO(ptr(out.margin), ptr(out.sample), ptr(out.pair))
        with self._lock:
            _check(lib().mkh_swept_clearance(self.handle, N, ptr(q_from), ptr(q_to), int(n_samples), C.byref(io), devp, stream))
        return out

    def certified_sweep(self, q_from, q_to, resolution: float, max_samples: int = 64) -> CertifiedSweepOut:
        """mkh_certified_sweep with this handle as the checker: the edges from q_from (N, nq) to q_to (N, nq), each at the sample
        count its motion bound asks for at `resolution`, at most `max_samples` → the ten (N,) outputs of include/minkhip.h "THE
        RULE OF THE CERTIFIED SWEEP".  numpy in → numpy out (synchronous); torch CUDA tensors in → torch tensors out, asynchronous
        on the current stream."""
        m = self.nmodel.model
        prep, empty, ptr, stream, devp = _call_kit(q_from)
        q_from, q_to = prep(q_from), prep(q_to)
        if len(q_from.shape) != 2 or int(q_from.shape[1]) != m.nq or int(q_from.shape[0]) < 1:
            raise ValueError(f"q_from must have shape (N, {m.nq}) with N >= 1, got {tuple(q_from.shape)}")
        if tuple(q_to.shape) != tuple(q_from.shape):
            raise ValueError(f"q_to must have q_from's shape {tuple(q_from.shape)}, got {tuple(q_to.shape)}")
        N = int(q_from.shape[0])
        out = CertifiedSweepOut(*[empty((N,), np.float64 if f in ("margin", "lower_bound", "motion") else np.int32)
                                  for f in CERTIFIED_SWEEP_FIELDS])
        io = MkhCertifiedSweepIO(*[ptr(x) for x in out])
        with self._lock:
            _check(lib().mkh_certified_sweep(self.handle, N, ptr(q_from), ptr(q_to), float(resolution), int(max_samples), C.byref(io),
                                             devp, stream))
        return out

    def motion_reach(self) -> np.ndarray:
        """mkh_checker_motion_reach: the (n_pairs, njnt, 2) reach table of this handle's pair list."""
        out = np.empty((self.n_pairs, self.nmodel.model.njnt, 2))
        with self._lock:
            _check(lib().mkh_checker_motion_reach(self.handle, out.ctypes.data))
        return out

    def set_sweep_rows(self, rows: int) -> None:
        """mkh_problem_set_sweep_rows with this handle as the checker: room for the general convex pairs' distances of `rows`
        swept samples (8 bytes per such pair and row) — what lets swept_clearance and the checked ladder calls take a checker
        with cylinder-box, ellipsoid or mesh-hull pairs, in chunks of rows // n_samples edges.  0 frees it.  Synchronizes the
        device."""
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or int(rows) < 0:
            raise ValueError(f"rows must be an int >= 0, got {rows!r}")
        with self._lock:
            _check(lib().mkh_problem_set_sweep_rows(self.handle, int(rows)))

    def set_check_rows(self, rows: int) -> None:
        """mkh_problem_set_check_rows with this handle as the checker: room for the general convex pairs' distances of `rows`
        rows judged inside a call (8 bytes per such pair and row) — what lets checked candidate tracking (>= 1 + n_samples) and,
        together with set_sweep_rows, the checked refinement pass (>= 1 + 2 n_samples) take a checker with cylinder-box,
        ellipsoid or mesh-hull pairs.  0 frees it.  Synchronizes the device."""
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or int(rows) < 0:
            raise ValueError(f"rows must be an int >= 0, got {rows!r}")
        with self._lock:
            _check(lib().mkh_problem_set_check_rows(self.handle, int(rows)))

    def last_kernel(self) -> str:
        """Kernel variant launched by the last solve on this handle (diagnostic)."""
        return lib().mkh_problem_last_kernel(self.handle).decode()

    def launch_info(self, B: int) -> Dict[str, int]:
        g, b, l, t = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().mkh_problem_launch_info(self.handle, int(B), C.byref(g), C.byref(b), C.byref(l), C.byref(t)))
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value, "tableau_rows": t.value}

    # ------------------------------------------------------------------ solve
    def _tap_shapes(self, B: int) -> Dict[str, tuple]:
        m = self.nmodel.model
        return {
            "xpos": (B, m.nbody, 3), "xquat": (B, m.nbody, 4), "frame_pose": (B, self.n_frame, 7),
            "subtree_com": (B, 3), "task_e": (B, self.n_rows), "task_J": (B, self.n_rows, m.nv),
            "H": (B, m.nv, m.nv), "c": (B, m.nv), "box_lo": (B, m.nv), "box_hi": (B, m.nv),
            "coll_G": (B, self.n_pairs, m.nv), "coll_h": (B, self.n_pairs), "qp_iters": (B,),
            "cycles": (B, 16),
        }

    def solve(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
              damping: float = 1e-12, taps: Sequence[str] = (), solve_qp: bool = True,
              out=None, status_out=None, n_steps: Optional[int] = None, q_out=None, direct_qp: bool = False,
              dense: Optional[dict] = None, until: Optional[tuple] = None, wave_kernel: bool = False, lane_kernel: bool = False,
              two_waves: bool = False, warm_start: bool = False, quad_kernel: bool = False, full_rows: bool = False):
        """Returns (v, status[, taps dict]).  numpy in → numpy out (synchronous);
        torch CUDA tensors in → torch tensors out (asynchronous on the current stream).
        `until` = (pos_threshold, ori_threshold) with n_steps = max_iters: the threshold-terminated loop
        (mkh_solve_until), returns (q_final, v_last, status, iters, converged).
        `dense`: the plugin rows of a problem created with dense_tasks / dense_limit_rows —
        {"task_e": (B, K), "task_J": (B, K, nv), "limit_G": (B, M, nv), "limit_h": (B, M)} (mkh_solve_dense)."""
        with self._lock:
            return self._solve(q, frame_targets, posture_target, com_target, dt, damping, taps, solve_qp, out,
                               status_out, n_steps, q_out, direct_qp, dense, until, wave_kernel, lane_kernel, two_waves, warm_start, quad_kernel, full_rows)

    def _solve(self, q, frame_targets, posture_target, com_target, dt, damping, taps, solve_qp, out, status_out,
               n_steps, q_out, direct_qp, dense=None, until=None, wave_kernel=False, lane_kernel=False, two_waves=False,
               warm_start=False, quad_kernel=False, full_rows=False):
        m = self.nmodel.model
        use_torch = _is_torch(q)
        B = int(q.shape[0])
        if B > self.max_batch:      # the handle's per-instance state (staging, warm-start sets) is sized by max_batch
            raise MinkHipError(f"B={B} exceeds max_batch={self.max_batch} of this problem")
        flags = (FLAG_DIRECT_QP if direct_qp else 0) | (FLAG_WAVE_KERNEL if wave_kernel else 0) | \
            (FLAG_LANE_KERNEL if lane_kernel else 0) | (FLAG_TWO_WAVES if two_waves else 0) | \
            (FLAG_WARM_START if warm_start else 0) | (FLAG_QUAD_KERNEL if quad_kernel else 0) | \
            (FLAG_FULL_ROWS if full_rows else 0)

        if use_torch:
            import torch
            dev = q.device

            f64 = torch.float64

            def prep(x):     # (the common case — already float64, on the device, contiguous — must cost nothing: a UR5e
                #              solve of 4 096 instances is a 19 µs kernel, the host side of this call has to stay below it)
                if x is None or (x.dtype is f64 and x.device == dev and x.is_contiguous()):
                    return x
                return x.to(device=dev, dtype=f64).contiguous()

            q = prep(q); frame_targets = prep(frame_targets); posture_target = prep(posture_target)
            com_target = prep(com_target)
            ptr = lambda x: 0 if x is None else x.data_ptr()
            flags |= FLAG_DEVICE_PTRS
            v = (torch.empty((B, m.nv), dtype=torch.float64, device=dev) if out is None else out) if solve_qp else None
            st = (torch.empty((B,), dtype=torch.int32, device=dev) if status_out is None else status_out) if solve_qp else None
            stream = _raw_stream(torch, dev)
            tapbufs = {}
            shapes = self._tap_shapes(B) if taps else None
            for n in taps:
                dt_ = torch.int32 if n == "qp_iters" else (torch.int64 if n == "cycles" else torch.float64)
                tapbufs[n] = torch.empty(shapes[n], dtype=dt_, device=dev)
                if n in ("task_e", "task_J", "subtree_com"):
                    tapbufs[n].zero_()
        else:
            q = _f64(q)
            frame_targets = None if frame_targets is None else _f64(frame_targets)
            posture_target = None if posture_target is None else _f64(posture_target)
            com_target = None if com_target is None else _f64(com_target)
            ptr = lambda x: None if x is None else x.ctypes.data
            v = (np.empty((B, m.nv)) if out is None else out) if solve_qp else None
            st = (np.zeros((B,), dtype=np.int32) if status_out is None else status_out) if solve_qp else None
            stream = None
            shapes = self._tap_shapes(B)
            tapbufs = {n: np.zeros(shapes[n], dtype=np.int32 if n == "qp_iters" else (np.int64 if n == "cycles" else np.float64)) for n in taps}
        if q.shape != (B, m.nq):
            raise ValueError(f"q must have shape (B, {m.nq}), got {tuple(q.shape)}")
        if self.n_frame and (frame_targets is None or tuple(frame_targets.shape) != (B, self.n_frame, 7)):
            raise ValueError(f"frame_targets must have shape ({B}, {self.n_frame}, 7)")
        if self.n_posture:
            if posture_target is None:
                raise ValueError("posture_target is required")
            if tuple(posture_target.shape) == (B, self.n_posture, m.nq):
                flags |= FLAG_POSTURE_BATCHED
            elif tuple(posture_target.shape) != (self.n_posture, m.nq):
                raise ValueError(f"posture_target must have shape ({self.n_posture}, {m.nq}) or (B, ...)")
        if self.n_com:
            if com_target is None:
                raise ValueError("com_target is required")
            if tuple(com_target.shape) == (B, self.n_com, 3):
                flags |= FLAG_COM_BATCHED
            elif tuple(com_target.shape) != (self.n_com, 3):
                raise ValueError(f"com_target must have shape ({self.n_com}, 3) or (B, ...)")
        args = [self.handle, B, ptr(q), ptr(frame_targets), ptr(posture_target), ptr(com_target), float(dt),
                float(damping), ptr(v), ptr(st)]
        if self.n_dense_rows or self.n_dense_limit_rows or self.dense_limit_box:
            if n_steps is not None:
                raise ValueError("dense (plugin) rows are evaluated by the caller at q: no fused steps")
            dense = dense or {}
            shapes_d = {"task_e": (B, self.n_dense_rows), "task_J": (B, self.n_dense_rows, m.nv),
                        "limit_G": (B, self.n_dense_limit_rows, m.nv), "limit_h": (B, self.n_dense_limit_rows)}
            if self.dense_limit_box:
                shapes_d.update({"limit_lo": (B, m.nv), "limit_hi": (B, m.nv)})
            dr, keep_d = MkhDenseRows(), []
            for name, shp in shapes_d.items():
                if 0 in shp:
                    continue
                x = dense.get(name)
                if x is None and name in ("limit_lo", "limit_hi"):
                    continue                                   # one-sided box rows
                if x is None or tuple(x.shape) != shp:
                    raise ValueError(f"dense['{name}'] must have shape {shp}")
                x = prep(x) if use_torch else _f64(x)
                keep_d.append(x)
                setattr(dr, name, x.data_ptr() if use_torch else x.ctypes.data)
            tp = None
            if taps or not solve_qp:
                tp = MkhTaps()
                for n in taps:
                    setattr(tp, n, tapbufs[n].data_ptr() if use_torch else tapbufs[n].ctypes.data)
            _check(lib().mkh_solve_dense(*args[:6], C.byref(dr), float(dt), float(damping), ptr(v), ptr(st),
                                         C.byref(tp) if tp is not None else None, flags, stream))
            return (v, st, tapbufs) if tp is not None else (v, st)
        if n_steps is not None:
            # fused (solve, integrate) x n_steps on the device: returns (q_final, v_last, status)
            if use_torch:
                import torch
                qo = torch.empty_like(q) if q_out is None else q_out
            else:
                qo = np.empty_like(q) if q_out is None else q_out
            if until is not None:
                if use_torch:
                    it = torch.empty((B,), dtype=torch.int32, device=dev); cv = torch.empty_like(it)
                else:
                    it = np.zeros((B,), dtype=np.int32); cv = np.zeros((B,), dtype=np.int32)
                _check(lib().mkh_solve_until(*args[:8], int(n_steps), float(until[0]), float(until[1]), ptr(qo), ptr(v),
                                             ptr(st), ptr(it), ptr(cv), flags, stream))
                return qo, v, st, it, cv
            _check(lib().mkh_solve_steps(*args[:8], int(n_steps), ptr(qo), ptr(v), ptr(st), flags, stream))
            return qo, v, st
        if taps or not solve_qp:
            tp = MkhTaps()
            for n in taps:
                setattr(tp, n, tapbufs[n].data_ptr() if use_torch else tapbufs[n].ctypes.data)
            _check(lib().mkh_eval(*args, C.byref(tp), flags, stream))
            if "qp_iters" in tapbufs:
                # packed by the kernel: active-set selections | loop iterations << 10 | rank-1 pivots << 20
                raw = tapbufs["qp_iters"]
                tapbufs["qp_loops"] = (raw >> 10) & 1023
                tapbufs["qp_pivots"] = (raw >> 20) & 1023
                tapbufs["qp_iters"] = raw & 1023
            return v, st, tapbufs
        _check(lib().mkh_solve(*args, flags, stream))
        return v, st

    # ---------------------------------------------- what every fan-out call asks
    @staticmethod
    def _kernel_flags(wave: bool, lane: bool, quad: bool, extra: int = 0) -> int:
        return (FLAG_WAVE_KERNEL if wave else 0) | (FLAG_LANE_KERNEL if lane else 0) | (FLAG_QUAD_KERNEL if quad else 0) | int(extra)

    def _refuse_dense(self, what: str) -> None:
        if self.n_dense_rows or self.n_dense_limit_rows or self.dense_limit_box:
            raise ValueError(f"dense (plugin) rows are evaluated by the caller at q: no fused loop, no {what}")

    def _need_frame(self, what: str) -> None:
        if not self.n_frame:
            raise ValueError(f"{what} needs at least one frame task to test the thresholds on")

    def _held_flags(self, posture_target, com_target, lead: tuple) -> int:
        """FLAG_POSTURE_BATCHED / FLAG_COM_BATCHED from the shapes of the two targets, each held or one per row of `lead`."""
        m, flags = self.nmodel.model, 0
        if self.n_posture:
            flags |= _held_or_rows(posture_target, lead, self.n_posture, m.nq, "posture_target", FLAG_POSTURE_BATCHED)
        if self.n_com:
            flags |= _held_or_rows(com_target, lead, self.n_com, 3, "com_target", FLAG_COM_BATCHED)
        return flags

    # ------------------------------------------------------------ multi-start
    def solve_multistart(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                         damping: float = 1e-12, *, n_seeds: int, max_iters: int, pos_threshold: float, ori_threshold: float,
                         rng_seed: int = 0, target_index0: int = 0, seeds=None, reference=None, weights=None,
                         return_all: bool = False, wave_kernel: bool = False, lane_kernel: bool = False,
                         quad_kernel: bool = False, seed_table=None, collision_check=None) -> MultistartOut:
        """mkh_solve_multistart: the threshold-terminated loop from `n_seeds` starts per row of q (seed 0 = the row itself, the
        others drawn on the device or taken from `seeds` (B, S, nq)), the converged result closest to `reference` (default q)
        picked on the device.  numpy in → numpy out (synchronous); torch CUDA tensors in → torch tensors out, asynchronous on
        the current stream, no host copy.  The handle needs max_batch >= B·n_seeds.  `seed_table` (a SeedTable or
        NativeSeedTable, not together with `seeds`): seeds 1 … n_seeds − 1 are the table's entries nearest to each target,
        looked up on the device in front of the seed kernel; the table is attached for this call only.  `collision_check` (a
        CollisionChecker, or a NativeProblem with collision pairs on this handle's model — this handle itself included): every
        candidate whose final q is in collision gets ST_IN_COLLISION in its status row directly behind the loops and is not
        eligible (include/minkhip.h "THE RULE OF CLEARANCE"); attached for this call only."""
        if seeds is not None and seed_table is not None:
            raise ValueError("seeds and seed_table are two sources of the same starts: pass one of them")
        with self._lock, _attached(self, seed_table), _checked(self, collision_check):
            return self._solve_multistart(q, frame_targets, posture_target, com_target, dt, damping, int(n_seeds), int(max_iters),
                                          float(pos_threshold), float(ori_threshold), int(rng_seed), int(target_index0), seeds,
                                          reference, weights, return_all, wave_kernel, lane_kernel, quad_kernel)

    def solve_multistart_set(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                             damping: float = 1e-12, *, n_seeds: int, n_solutions: int, max_iters: int, pos_threshold: float,
                             ori_threshold: float, min_distance: float = 0.1, rng_seed: int = 0, target_index0: int = 0,
                             seeds=None, reference=None, weights=None, return_all: bool = False, wave_kernel: bool = False,
                             lane_kernel: bool = False, quad_kernel: bool = False, seed_table=None,
                             unwind_turns: bool = False, collision_check=None) -> SolutionSetOut:
        """mkh_solve_multistart_set: solve_multistart's seeds and loops, then up to `n_solutions` converged results per row of q
        no two of which lie within `min_distance` of each other (Σ_k weights_k·(a ⊖ b)_k² <= min_distance²), in ascending
        distance from `reference` (default q) — slot 0 is solve_multistart's choice (the rule: include/minkhip.h "THE RULE OF THE
        SET").  numpy in → numpy out (synchronous); torch CUDA tensors in → torch tensors out, asynchronous on the current
        stream, no host copy.  Everything else as in solve_multistart.  `unwind_turns` (MKH_FLAG_UNWIND_TURNS): the loops'
        results are moved to the turn nearest the reference before they are compared; q_all then holds the unwound rows.
        `collision_check`: as in solve_multistart (the check runs in front of the unwinding)."""
        if seeds is not None and seed_table is not None:
            raise ValueError("seeds and seed_table are two sources of the same starts: pass one of them")
        check_solution_set(int(n_solutions), float(min_distance), int(n_seeds))
        with self._lock, _attached(self, seed_table), _checked(self, collision_check):
            return self._solve_multistart(q, frame_targets, posture_target, com_target, dt, damping, int(n_seeds), int(max_iters),
                                          float(pos_threshold), float(ori_threshold), int(rng_seed), int(target_index0), seeds,
                                          reference, weights, return_all, wave_kernel, lane_kernel, quad_kernel,
                                          solution_set=(int(n_solutions), float(min_distance)),
                                          extra_flags=FLAG_UNWIND_TURNS if unwind_turns else 0)

    def unwind_turns(self, q_rows, reference, out=None):
        """mkh_unwind_turns: include/minkhip.h "THE RULE OF THE UNWINDING" alone — q_rows (n, nq) or (B, S, nq), every row moved
        to the full turn of its eligible hinges nearest its reference: reference (B, nq), row i of the flattened rows using
        reference[i // S] (a 2-D q_rows: S = n / B, which must divide).  `out` may be q_rows itself.  numpy in → numpy out
        (synchronous); torch CUDA tensors in → torch tensors out on the current stream, no host copy."""
        m = self.nmodel.model
        shp = tuple(q_rows.shape)
        if len(shp) not in (2, 3) or shp[-1] != m.nq or min(shp) < 1:
            raise ValueError(f"q_rows must have shape (n, {m.nq}) or (B, S, {m.nq}), got {shp}")
        prep, empty, ptr, stream, devp = _call_kit(q_rows)
        q_rows, reference = prep(q_rows), prep(reference)
        n = shp[0] if len(shp) == 2 else shp[0] * shp[1]
        if reference is None or len(reference.shape) != 2 or int(reference.shape[1]) != m.nq or int(reference.shape[0]) < 1:
            raise ValueError(f"reference must have shape (B, {m.nq})")
        Bref = int(reference.shape[0])
        if n % Bref or (len(shp) == 3 and shp[0] != Bref):
            raise ValueError(f"{n} rows do not split evenly among {Bref} reference rows")
        if out is None:
            out = empty(shp, np.float64)
        elif tuple(out.shape) != shp or prep(out) is not out:
            raise ValueError(f"out must be a contiguous float64 array of shape {shp}, of q_rows' kind")
        with self._lock:
            _check(lib().mkh_unwind_turns(self.handle, n, n // Bref, ptr(q_rows), ptr(reference), ptr(out), devp, stream))
        return out

    def select_distinct(self, q_candidates, valid=None, reference=None, weights=None, *, n_solutions: int,
                        min_distance: float = 0.1) -> DistinctOut:
        """mkh_select_distinct: the rule of solve_multistart_set alone over the caller's own candidates — q_candidates
        (B, S, nq), valid (B, S) (None: every candidate), reference (B, nq) (required), weights (nv,).  numpy in → numpy out
        (synchronous); torch CUDA tensors in → torch tensors out on the current stream, no host copy."""
        m, kit = self.nmodel.model, _call_kit(q_candidates)
        K = int(n_solutions)
        kit.want(q_candidates, ("B", "S", m.nq), "q_candidates")
        B, S = int(q_candidates.shape[0]), int(q_candidates.shape[1])
        check_solution_set(K, float(min_distance), S)
        if B < 1 or S < 1:
            raise ValueError(f"q_candidates must hold at least one target and one candidate, got {tuple(q_candidates.shape)}")
        q_candidates = kit.prep(q_candidates)
        reference = kit.want(kit.prep(reference), (B, m.nq), "reference", required=True)
        weights = kit.want(kit.prep(weights), (m.nv,), "weights")
        valid = kit.flags01(valid, (B, S), "valid")
        io, out = DISTINCT_OUT.make[_NONE](kit.empty, kit.ptr, dict(B=B, K=K, q=m.nq))
        with self._lock:
            _check(lib().mkh_select_distinct(self.handle, B, S, kit.ptr(q_candidates), kit.ptr(valid), kit.ptr(reference),
                                             kit.ptr(weights), K, float(min_distance), C.byref(io), kit.devp, kit.stream))
        return DistinctOut(**out)

    def solve_goalset(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                      damping: float = 1e-12, *, n_seeds: int, max_iters: int, pos_threshold: float, ori_threshold: float,
                      goal_cost=None, goal_valid=None, rng_seed: int = 0, target_index0: int = 0, seeds=None, reference=None,
                      weights=None, return_all: bool = False, wave_kernel: bool = False, lane_kernel: bool = False,
                      quad_kernel: bool = False, seed_table=None, collision_check=None) -> GoalSetOut:
        """mkh_solve_goalset: multi-start to the best of G goals per row of q — solve_multistart's seeds and loops on the (B·G)
        flattened (target, goal) pairs (seed 0 of every goal the row of q itself, the others drawn at target index
        (target_index0 + b)·G + g, taken from `seeds` (B, G, S, nq) or from `seed_table`, queried with every goal's own
        targets), per goal the converged seed closest to `reference` (default q), per target the reached goal with the smallest
        goal_cost + distance (the rule: include/minkhip.h "THE RULE OF THE GOAL SET").  frame_targets (B, G, n_frame, 7);
        posture / CoM targets held for the whole call, (n, w), or (B, G, n, w); goal_cost, goal_valid (B, G).  The handle needs
        max_batch >= n_seeds; B·G·n_seeds loops beyond max_batch run in chunks of whole goals.  numpy in → numpy out
        (synchronous); torch CUDA tensors in → torch tensors out on the current stream, no host copy.  `collision_check`: as in
        solve_multistart — a goal whose candidates all collide is not reached."""
        if seeds is not None and seed_table is not None:
            raise ValueError("seeds and seed_table are two sources of the same starts: pass one of them")
        m, kit = self.nmodel.model, _call_kit(q)
        B, S, max_iters = int(q.shape[0]), int(n_seeds), int(max_iters)
        if max_iters < 1:
            raise ValueError("max_iters must be >= 1")
        self._refuse_dense("goal set")
        self._need_frame("a goal set")
        kit.want(frame_targets, (B, "G", self.n_frame, 7), "frame_targets", required=True)
        G = int(frame_targets.shape[1])
        check_goalset_shape(B, G, S)
        if S > self.max_batch:
            raise MinkHipError(f"n_seeds={S} exceeds max_batch={self.max_batch} of this problem")
        q = kit.want(kit.prep(q), ("B", m.nq), "q")
        frame_targets, posture_target, com_target = kit.prep(frame_targets), kit.prep(posture_target), kit.prep(com_target)
        flags = self._kernel_flags(wave_kernel, lane_kernel, quad_kernel, kit.devp) | \
            self._held_flags(posture_target, com_target, (B, G))
        seeds = kit.want(kit.prep(seeds), (B, G, S, m.nq), "seeds")
        reference = kit.want(kit.prep(reference), (B, m.nq), "reference")
        weights = kit.want(kit.prep(weights), (m.nv,), "weights")
        goal_cost, goal_valid = _goal_inputs(kit, goal_cost, goal_valid, B, G)
        ptr = kit.ptr
        io, out = GOAL_SET_OUT.make[_ALL if return_all else _NONE](
            kit.empty, ptr, dict(B=B, G=G, S=S, q=m.nq, v=m.nv), seeds=ptr(seeds), q_ref=ptr(reference), weights=ptr(weights),
            goal_cost=ptr(goal_cost), goal_valid=ptr(goal_valid))
        with self._lock, _attached(self, seed_table), _checked(self, collision_check):
            _check(lib().mkh_solve_goalset(self.handle, B, G, kit.ptr(q), kit.ptr(frame_targets), kit.ptr(posture_target),
                                           kit.ptr(com_target), float(dt), float(damping), max_iters, float(pos_threshold),
                                           float(ori_threshold), S, int(rng_seed) & (2 ** 64 - 1), int(target_index0), C.byref(io),
                                           flags, kit.stream))
        return GoalSetOut(**out)

    def select_goalset(self, q_candidates, valid=None, reference=None, weights=None, *, goal_cost=None,
                       goal_valid=None) -> GoalSelectOut:
        """mkh_select_goalset: the two levels of solve_goalset alone over the caller's own candidates — q_candidates
        (B, G, S, nq), valid (B, G, S) (None: every candidate), reference (B, nq) (required), weights (nv,), goal_cost and
        goal_valid (B, G).  numpy in → numpy out (synchronous); torch CUDA tensors in → torch tensors out on the current
        stream, no host copy."""
        m, kit = self.nmodel.model, _call_kit(q_candidates)
        kit.want(q_candidates, ("B", "G", "S", m.nq), "q_candidates")
        B, G, S = (int(x) for x in q_candidates.shape[:3])
        check_goalset_shape(B, G, S)
        q_candidates = kit.prep(q_candidates)
        reference = kit.want(kit.prep(reference), (B, m.nq), "reference", required=True)
        weights = kit.want(kit.prep(weights), (m.nv,), "weights")
        valid = kit.flags01(valid, (B, G, S), "valid")
        goal_cost, goal_valid = _goal_inputs(kit, goal_cost, goal_valid, B, G)
        io, out = GOAL_SELECT_OUT.make[_NONE](kit.empty, kit.ptr, dict(B=B, G=G, q=m.nq), goal_cost=kit.ptr(goal_cost),
                                              goal_valid=kit.ptr(goal_valid))
        with self._lock:
            _check(lib().mkh_select_goalset(self.handle, B, G, S, kit.ptr(q_candidates), kit.ptr(valid), kit.ptr(reference),
                                            kit.ptr(weights), C.byref(io), kit.devp, kit.stream))
        return GoalSelectOut(**out)

    def _solve_multistart(self, q, frame_targets, posture_target, com_target, dt, damping, S, max_iters, pos_thr, ori_thr,
                          rng_seed, target_index0, seeds, reference, weights, return_all, wave_kernel, lane_kernel, quad_kernel,
                          solution_set=None, extra_flags: int = 0):
        m, kit = self.nmodel.model, _call_kit(q)
        B = int(q.shape[0])
        if S < 1:
            raise ValueError("n_seeds must be >= 1")
        if max_iters < 1:
            raise ValueError("max_iters must be >= 1")
        if B * S > self.max_batch:
            raise MinkHipError(f"B*n_seeds={B * S} exceeds max_batch={self.max_batch} of this problem")
        self._refuse_dense("multi-start")
        q = kit.want(kit.prep(q), ("B", m.nq), "q")
        self._need_frame("multi-start")
        frame_targets = kit.want(kit.prep(frame_targets), (B, self.n_frame, 7), "frame_targets", required=True)
        posture_target, com_target = kit.prep(posture_target), kit.prep(com_target)
        flags = self._kernel_flags(wave_kernel, lane_kernel, quad_kernel, int(extra_flags) | kit.devp) | \
            self._held_flags(posture_target, com_target, (B,))
        seeds = kit.want(kit.prep(seeds), (B, S, m.nq), "seeds")
        reference = kit.want(kit.prep(reference), (B, m.nq), "reference")
        weights = kit.want(kit.prep(weights), (m.nv,), "weights")
        ptr = kit.ptr
        if solution_set is None:
            table, cls, call = MULTISTART_OUT, MultistartOut, lib().mkh_solve_multistart
        else:
            table, cls, call = SOLUTION_SET_OUT, SolutionSetOut, lib().mkh_solve_multistart_set
        io, out = table.make[_ALL if return_all else _NONE](
            kit.empty, ptr, dict(B=B, S=S, K=solution_set[0] if solution_set else 0, q=m.nq, v=m.nv), seeds=ptr(seeds),
            q_ref=ptr(reference), weights=ptr(weights))
        _check(call(self.handle, B, kit.ptr(q), kit.ptr(frame_targets), kit.ptr(posture_target), kit.ptr(com_target), float(dt),
                    float(damping), max_iters, pos_thr, ori_thr, S, *(solution_set or ()), rng_seed & (2 ** 64 - 1), target_index0,
                    C.byref(io), flags, kit.stream))
        return cls(**out)

    # ------------------------------------------------------------- trajectory
    def solve_trajectory(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                         damping: float = 1e-12, n_steps: int = 1, until: Optional[tuple] = None,
                         qvel_dt: Optional[float] = None, time_major: bool = False, warm_start: bool = False,
                         wave_kernel: bool = False, lane_kernel: bool = False, quad_kernel: bool = False) -> TrajectoryOut:
        """mkh_solve_trajectory: every row of q follows its own T waypoints, waypoint t solved by the fused loop from where
        waypoint t − 1 ended — `until` = (pos_threshold, ori_threshold): the threshold-terminated loop with max_iters = n_steps;
        None: n_steps fixed steps.  frame_targets (B, T, n_frame, 7); posture / CoM targets as in solve(), or with a T axis
        after B (leading when the target has no B axis; a 3-d target whose first axis equals B is read as (B, ...)).  time_major: T leads every array that has one, outputs included.
        numpy in → numpy out (synchronous); torch CUDA tensors in → torch tensors out, asynchronous on the current stream, no
        host copy.  A failing waypoint does not stop its trajectory (include/minkhip.h)."""
        with self._lock:
            return self._solve_trajectory(q, frame_targets, posture_target, com_target, dt, damping, int(n_steps), until, qvel_dt,
                                          bool(time_major), warm_start, wave_kernel, lane_kernel, quad_kernel)

    def solve_keyframes(self, q, keyframe_times, waypoint_times, frame_keys=None, posture_keys=None, com_keys=None,
                        dt: float = 1e-2, damping: float = 1e-12, n_steps: int = 1, until: Optional[tuple] = None,
                        qvel_dt: Optional[float] = None, time_major: bool = False, return_targets: bool = False,
                        warm_start: bool = False, wave_kernel: bool = False, lane_kernel: bool = False,
                        quad_kernel: bool = False) -> KeyframesOut:
        """mkh_solve_keyframes: solve_trajectory whose T = len(waypoint_times) waypoint targets are interpolated on the device
        from K = len(keyframe_times) keyframes (the rule: include/minkhip.h).  The target arrays are solve_trajectory's with a
        K axis where that call has its T axis — frame_keys (B, K, n_frame, 7); posture / CoM keys held as in solve(), or with
        a K axis; time_major: K leads the inputs, T the outputs.  The two time arrays are host sequences shared by the batch.
        return_targets: also the interpolated targets, in the layout solve_trajectory takes them in.  numpy in → numpy out;
        torch CUDA tensors in → torch tensors out on the current stream, no host copy."""
        kt, wt = check_keyframe_times(keyframe_times, waypoint_times)
        with self._lock:
            return self._solve_trajectory(q, frame_keys, posture_keys, com_keys, dt, damping, int(n_steps), until, qvel_dt,
                                          bool(time_major), warm_start, wave_kernel, lane_kernel, quad_kernel,
                                          keys=(kt, wt, bool(return_targets)))

    def solve_trajectory_multistart(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                                    damping: float = 1e-12, *, n_seeds: int, n_steps: int, pos_threshold: float,
                                    ori_threshold: float, rng_seed: int = 0, target_index0: int = 0, seeds=None, weights=None,
                                    qvel_dt: Optional[float] = None, time_major: bool = False, warm_start: bool = False,
                                    return_all: bool = False, wave_kernel: bool = False, lane_kernel: bool = False,
                                    quad_kernel: bool = False, seed_table=None) -> TrajectoryMultistartOut:
        """mkh_solve_trajectory_multistart: solve_trajectory's threshold-terminated loops from `n_seeds` candidate starts per row
        of q (candidate 0 = the row itself, the others drawn on the device as in solve_multistart or taken from `seeds`
        (B, S, nq)); per row the candidate that tracked the most waypoints, then the one with the shortest path from q
        (Σ_t Σ_k weights_k·(q_t ⊖ q_{t−1})_k²), is picked and gathered on the device (the rule: include/minkhip.h).  Targets
        and time_major as in solve_trajectory.  numpy in → numpy out (synchronous); torch CUDA tensors in → torch tensors out,
        asynchronous on the current stream, no host copy.  The handle needs max_batch >= B·n_seeds.  `seed_table` (not
        together with `seeds`): candidates 1 … n_seeds − 1 start at the table's entries nearest to waypoint 0's targets."""
        if seeds is not None and seed_table is not None:
            raise ValueError("seeds and seed_table are two sources of the same starts: pass one of them")
        with self._lock, _attached(self, seed_table):
            return self._solve_trajectory(q, frame_targets, posture_target, com_target, dt, damping, int(n_steps),
                                          (float(pos_threshold), float(ori_threshold)), qvel_dt, bool(time_major), warm_start,
                                          wave_kernel, lane_kernel, quad_kernel,
                                          cands=(int(n_seeds), int(rng_seed), int(target_index0), seeds, weights, bool(return_all)))

    def solve_trajectory_multistart_free(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                                         damping: float = 1e-12, *, checker: "NativeProblem", edge_samples: int = 8, n_seeds: int,
                                         n_steps: int, pos_threshold: float, ori_threshold: float, rng_seed: int = 0,
                                         target_index0: int = 0, seeds=None, weights=None, qvel_dt: Optional[float] = None,
                                         time_major: bool = False, warm_start: bool = False, return_all: bool = False,
                                         wave_kernel: bool = False, lane_kernel: bool = False, quad_kernel: bool = False,
                                         seed_table=None):
        """mkh_solve_trajectory_multistart_free: solve_trajectory_multistart under THE RULE "with a checker" (include/minkhip.h) —
        `checker` a handle with collision limits on the same NativeModel, `edge_samples` interior samples per motion.  Every row of
        every candidate is checked as a node, the motion into every eligible row is swept, and a waypoint counts only when it is
        free and entered by a free motion.  Returns (TrajectoryMultistartOut, TrajectoryFreeOut); with `return_all` the latter
        carries node_margin_all and edge_margin_all (T, B·S)."""
        if seeds is not None and seed_table is not None:
            raise ValueError("seeds and seed_table are two sources of the same starts: pass one of them")
        checker = _checker_handle(self, checker, edge_samples)
        with _with_checker(self, checker), _attached(self, seed_table):
            return self._solve_trajectory(q, frame_targets, posture_target, com_target, dt, damping, int(n_steps),
                                          (float(pos_threshold), float(ori_threshold)), qvel_dt, bool(time_major), warm_start,
                                          wave_kernel, lane_kernel, quad_kernel,
                                          cands=(int(n_seeds), int(rng_seed), int(target_index0), seeds, weights, bool(return_all)),
                                          free=(checker, int(edge_samples)))

    def select_trajectory_candidates(self, q, q_paths, tracked=None, weights=None, checker: Optional["NativeProblem"] = None,
                                     edge_samples: int = 8, return_margins: bool = False):
        """mkh_select_trajectory_candidates: the selection of solve_trajectory_multistart alone, over the caller's own candidates —
        q (B, nq) the current postures, q_paths (T, B·S, nq) time-major, tracked (T, B·S) (None: every row), weights (nv,) >= 0.
        Without `checker` THE RULE on the caller's flags: returns (TrajectoryCandidatesOut, None).  With one THE RULE "with a
        checker", `tracked` playing converged_all: returns (TrajectoryCandidatesOut, TrajectoryFreeOut), the latter (B, T) and, with
        `return_margins`, with node_margin_all and edge_margin_all (T, B·S).  numpy in → numpy out (synchronous); torch CUDA
        tensors in → torch tensors out on the current stream, no host copy."""
        m, kit = self.nmodel.model, _call_kit(q)
        if checker is not None:
            checker = _checker_handle(self, checker, edge_samples)
        B = int(q.shape[0])
        if len(q_paths.shape) != 3 or int(q_paths.shape[0]) < 1 or int(q_paths.shape[1]) < B or int(q_paths.shape[1]) % B:
            raise ValueError(f"q_paths must have shape (T, B*S, {m.nq}) with B = {B}, got {tuple(q_paths.shape)}")
        T, R = int(q_paths.shape[0]), int(q_paths.shape[1])
        q = kit.want(kit.prep(q), ("B", m.nq), "q")
        q_paths = kit.want(kit.prep(q_paths), (T, R, m.nq), "q_paths")
        weights = kit.want(kit.prep(weights), (m.nv,), "weights")
        tracked = kit.flags01(tracked, (T, R), "tracked")
        sizes = dict(L=(B, T), B=B, T=T, R=R, q=m.nq)
        io, out = TRAJECTORY_CANDIDATES_OUT.make[_NONE](kit.empty, kit.ptr, sizes)
        rows = (B, T, R // B, kit.ptr(q), kit.ptr(q_paths), kit.ptr(tracked), kit.ptr(weights))
        if checker is None:
            with self._lock:
                _check(lib().mkh_select_trajectory_candidates(self.handle, None, *rows, 0, C.byref(io), None, kit.devp, kit.stream))
            return TrajectoryCandidatesOut(**out), None
        fio, more = TRAJECTORY_FREE_OUT.make[_ALL if return_margins else _NONE](kit.empty, kit.ptr, sizes)
        with _with_checker(self, checker):
            _check(lib().mkh_select_trajectory_candidates(self.handle, checker.handle, *rows, int(edge_samples), C.byref(io),
                                                          C.byref(fio), kit.devp, kit.stream))
        return TrajectoryCandidatesOut(**out), TrajectoryFreeOut(**more)

    # ----------------------------------------------------------------- ladder
    def ladder_select(self, q, q_nodes, tracked=None, max_step_sq: float = float("inf"), weights=None) -> LadderPathOut:
        """mkh_ladder_select: the dynamic program of include/minkhip.h "THE RULE" over the caller's rungs — q (B, nq) the current
        postures, q_nodes (B, T, S, nq), tracked (B, T, S) (None: every node), the squared break gate, weights (nv,) >= 0.
        numpy in → numpy out (synchronous); torch CUDA tensors in → torch tensors out on the current stream, no host copy."""
        return self._ladder_select(q, q_nodes, tracked, max_step_sq, weights, None, 0, False)[0]

    def ladder_select_free(self, q, q_nodes, checker: "NativeProblem", tracked=None, max_step_sq: float = float("inf"), weights=None,
                           edge_samples: int = 8, return_margins: bool = False):
        """mkh_ladder_select_free: ladder_select under THE RULE "with a checker" — `checker` a handle with collision limits on
        the same NativeModel, `edge_samples` interior samples per edge.  Returns (LadderPathOut, LadderFreeOut); with
        `return_margins` the latter carries node_margin (B, T, S) and edge_margin_all (B, T, S, S)."""
        checker = _checker_handle(self, checker, edge_samples)
        return self._ladder_select(q, q_nodes, tracked, max_step_sq, weights, checker, int(edge_samples), bool(return_margins))

    def ladder_select_certified(self, q, q_nodes, checker: "NativeProblem", tracked=None, max_step_sq: float = float("inf"),
                                weights=None, resolution: float = 0.02, max_samples: int = 64, require_certified: bool = False,
                                return_margins: bool = False):
        """mkh_ladder_select_certified: ladder_select under THE RULE "with a certifying checker" — every edge into an effectively
        tracked node judged by certified_sweep's rule at `resolution` and `max_samples`, blocked where it collides or, with
        `require_certified`, wherever it is not proven free.  Returns (LadderPathOut, LadderCertifiedOut); with `return_margins`
        the latter carries node_margin (B, T, S), edge_margin_all (B, T, S, S) and edge_verdict_all (B, T, S, S) int8."""
        check_edge_rule(resolution, max_samples)
        checker = _checker_handle(self, checker, 1)
        rule = (float(resolution), int(max_samples), EDGE_REQUIRE_CERTIFIED if require_certified else EDGE_REJECT_COLLIDING)
        return self._ladder_select(q, q_nodes, tracked, max_step_sq, weights, checker, 0, bool(return_margins), rule)

    def _ladder_select(self, q, q_nodes, tracked, max_step_sq, weights, checker, edge_samples, return_margins, certified=None):
        m, kit = self.nmodel.model, _call_kit(q)
        B = int(q.shape[0])
        kit.want(q_nodes, (B, "T", "S", m.nq), "q_nodes")
        T, S = int(q_nodes.shape[1]), int(q_nodes.shape[2])
        check_ladder_shape(S, T, float(max_step_sq))
        q, q_nodes = kit.want(kit.prep(q), ("B", m.nq), "q"), kit.prep(q_nodes)
        weights = kit.want(kit.prep(weights), (m.nv,), "weights")
        tracked = kit.ones((B, T, S)) if tracked is None else kit.flags01(tracked, (B, T, S), "tracked")
        sizes = dict(B=B, T=T, S=S, q=m.nq)
        io, out = LADDER_OUT.make[_NONE](kit.empty, kit.ptr, sizes)
        rungs = (B, T, S, kit.ptr(q), kit.ptr(q_nodes), kit.ptr(tracked), kit.ptr(weights), float(max_step_sq))
        if checker is None:
            with self._lock:
                _check(lib().mkh_ladder_select(self.handle, *rungs, C.byref(io), kit.devp, kit.stream))
            return LadderPathOut(**out), None
        fio, more = LADDER_FREE_OUT.make[_MARGINS if return_margins else _NONE](kit.empty, kit.ptr, sizes)
        if certified is not None:
            cio, proof = LADDER_CERTIFIED_OUT.make[_NONE](kit.empty, kit.ptr, sizes)
            if return_margins:
                _verdict_bytes(kit, cio, proof, B, T, S)
            with _with_checker(self, checker):
                _check(lib().mkh_ladder_select_certified(self.handle, checker.handle, *rungs, *certified, C.byref(io), C.byref(fio),
                                                         C.byref(cio), kit.devp, kit.stream))
            return LadderPathOut(**out), LadderCertifiedOut(**more, **proof)
        with _with_checker(self, checker):
            _check(lib().mkh_ladder_select_free(self.handle, checker.handle, *rungs, edge_samples, C.byref(io), C.byref(fio),
                                                kit.devp, kit.stream))
        return LadderPathOut(**out), LadderFreeOut(**more)

    def solve_trajectory_ladder(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                                damping: float = 1e-12, *, n_seeds: int, max_iters: int, pos_threshold: float,
                                ori_threshold: float, max_step_sq: float = float("inf"), rng_seed: int = 0, target_index0: int = 0,
                                seeds=None, weights=None, qvel_dt: Optional[float] = None, return_all: bool = False,
                                wave_kernel: bool = False, lane_kernel: bool = False, quad_kernel: bool = False,
                                seed_table=None, refine: bool = False) -> TrajectoryLadderOut:
        """mkh_solve_trajectory_ladder: `n_seeds` IK solutions per waypoint — multi-start's loops on the (B·T) flattened targets,
        seed 0 of every rung the row of q itself, the others drawn, taken from `seeds` (B, T, S, nq) or from `seed_table`
        (queried with every waypoint's own targets) — then ladder_select's search and the gather of the chosen nodes, in one
        call.  frame_targets (B, T, n_frame, 7); posture / CoM targets held for the whole call, (n, w), or (B, T, n, w).  The
        handle needs max_batch >= n_seeds; B·T·n_seeds loops beyond max_batch run in chunks of whole rungs.  numpy in → numpy
        out (synchronous); torch CUDA tensors in → torch tensors out on the current stream, no host copy.  With `refine` the
        path is re-tracked across its breaks and lost nodes behind the search (mkh_solve_trajectory_ladder_refined; the handle
        then needs max_batch >= B as well) and `tracked`, `repaired`, `refined` are returned with it."""
        return self._solve_trajectory_ladder(q, frame_targets, posture_target, com_target, dt, damping, n_seeds, max_iters,
                                             pos_threshold, ori_threshold, max_step_sq, rng_seed, target_index0, seeds, weights,
                                             qvel_dt, return_all, wave_kernel, lane_kernel, quad_kernel, seed_table, refine, None)

    def solve_trajectory_ladder_nodes(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                                      damping: float = 1e-12, *, n_seeds: int, n_nodes: int, max_iters: int, pos_threshold: float,
                                      ori_threshold: float, min_distance: float = 0.1, unwind_turns: bool = False,
                                      max_step_sq: float = float("inf"), rng_seed: int = 0, target_index0: int = 0, seeds=None,
                                      weights=None, qvel_dt: Optional[float] = None, return_all: bool = False,
                                      wave_kernel: bool = False, lane_kernel: bool = False, quad_kernel: bool = False,
                                      seed_table=None, refine: bool = False) -> TrajectoryLadderNodesOut:
        """mkh_solve_trajectory_ladder_nodes: solve_trajectory_ladder with every rung's `n_seeds` loop results reduced on the
        device to at most `n_nodes` distinct ones (select_distinct's rule with `min_distance`, the reference q, the ladder's
        weights; with `unwind_turns` moved to the turn nearest q first) before the search — n_seeds up to 4 096, the search and
        the node workspace on n_nodes <= 64 per rung.  Everything else as in solve_trajectory_ladder; with return_all the *_all
        fields are the nodes' rows (B, T, K, ·)."""
        return self._solve_trajectory_ladder(q, frame_targets, posture_target, com_target, dt, damping, n_seeds, max_iters,
                                             pos_threshold, ori_threshold, max_step_sq, rng_seed, target_index0, seeds, weights,
                                             qvel_dt, return_all, wave_kernel, lane_kernel, quad_kernel, seed_table, refine,
                                             (int(n_nodes), float(min_distance), bool(unwind_turns)))

    def solve_trajectory_ladder_free(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                                     damping: float = 1e-12, *, checker: "NativeProblem", edge_samples: int = 8, n_seeds: int,
                                     max_iters: int, pos_threshold: float, ori_threshold: float, n_nodes: Optional[int] = None,
                                     min_distance: float = 0.1, unwind_turns: bool = False, max_step_sq: float = float("inf"),
                                     rng_seed: int = 0, target_index0: int = 0, seeds=None, weights=None,
                                     qvel_dt: Optional[float] = None, return_all: bool = False, wave_kernel: bool = False,
                                     lane_kernel: bool = False, quad_kernel: bool = False, seed_table=None,
                                     refine: bool = False):
        """mkh_solve_trajectory_ladder_free: solve_trajectory_ladder (n_nodes None) or solve_trajectory_ladder_nodes under THE
        RULE "with a checker": colliding candidates get ST_IN_COLLISION behind the loops, every edge into a tracked node is swept
        with `edge_samples` interior samples, and the search runs on the mask.  Returns (the plain call's result, LadderFreeOut).
        With `refine` the checked refinement pass runs on the chosen path behind the search
        (mkh_solve_trajectory_ladder_free_refined; the handle then needs max_batch >= B as well): the plain result carries
        `tracked`, `repaired`, `refined`, and LadderFreeOut follows the returned path."""
        checker = _checker_handle(self, checker, edge_samples)
        nodes = None if n_nodes is None else (int(n_nodes), float(min_distance), bool(unwind_turns))
        return self._solve_trajectory_ladder(q, frame_targets, posture_target, com_target, dt, damping, n_seeds, max_iters,
                                             pos_threshold, ori_threshold, max_step_sq, rng_seed, target_index0, seeds, weights,
                                             qvel_dt, return_all, wave_kernel, lane_kernel, quad_kernel, seed_table, bool(refine),
                                             nodes, (checker, int(edge_samples)))

    def solve_trajectory_ladder_certified(self, q, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                                          damping: float = 1e-12, *, checker: "NativeProblem", resolution: float,
                                          max_samples: int = 64, require_certified: bool = False, n_seeds: int, max_iters: int,
                                          pos_threshold: float, ori_threshold: float, n_nodes: Optional[int] = None,
                                          min_distance: float = 0.1, unwind_turns: bool = False,
                                          max_step_sq: float = float("inf"), rng_seed: int = 0, target_index0: int = 0, seeds=None,
                                          weights=None, qvel_dt: Optional[float] = None, return_all: bool = False,
                                          wave_kernel: bool = False, lane_kernel: bool = False, quad_kernel: bool = False,
                                          seed_table=None):
        """mkh_solve_trajectory_ladder_certified: solve_trajectory_ladder_free with the edges judged by certified_sweep's rule at
        `resolution` and `max_samples` instead of a fixed sample count (ladder_select_certified states the policy).  Returns (the
        plain call's result, LadderCertifiedOut).  There is no refinement here: the pass still samples."""
        check_edge_rule(resolution, max_samples)
        checker = _checker_handle(self, checker, 1)
        nodes = None if n_nodes is None else (int(n_nodes), float(min_distance), bool(unwind_turns))
        rule = (float(resolution), int(max_samples), EDGE_REQUIRE_CERTIFIED if require_certified else EDGE_REJECT_COLLIDING)
        return self._solve_trajectory_ladder(q, frame_targets, posture_target, com_target, dt, damping, n_seeds, max_iters,
                                             pos_threshold, ori_threshold, max_step_sq, rng_seed, target_index0, seeds, weights,
                                             qvel_dt, return_all, wave_kernel, lane_kernel, quad_kernel, seed_table, False,
                                             nodes, (checker, 0, rule))

    def _solve_trajectory_ladder(self, q, frame_targets, posture_target, com_target, dt, damping, n_seeds, max_iters,
                                 pos_threshold, ori_threshold, max_step_sq, rng_seed, target_index0, seeds, weights, qvel_dt,
                                 return_all, wave_kernel, lane_kernel, quad_kernel, seed_table, refine, nodes, free=None):
        """The body of the ladder calls; `nodes`: None, or (n_nodes, min_distance, unwind_turns); `free`: None, or (checker,
        edge_samples) — the result is then (the plain result, LadderFreeOut) — or (checker, 0, (resolution, max_samples, policy)),
        the certified rule — (the plain result, LadderCertifiedOut)."""
        if seeds is not None and seed_table is not None:
            raise ValueError("seeds and seed_table are two sources of the same starts: pass one of them")
        m, kit = self.nmodel.model, _call_kit(q)
        B, S, max_iters = int(q.shape[0]), int(n_seeds), int(max_iters)
        if max_iters < 1:
            raise ValueError("max_iters must be >= 1")
        if qvel_dt is not None and not float(qvel_dt) > 0.0:
            raise ValueError("qvel_dt must be > 0")
        if not (float(pos_threshold) >= 0.0 and float(ori_threshold) >= 0.0):
            raise ValueError("thresholds must be >= 0: a ladder's rungs run in threshold mode only")
        self._refuse_dense("ladder")
        self._need_frame("a ladder")
        kit.want(frame_targets, (B, "T", self.n_frame, 7), "frame_targets", required=True)
        T = int(frame_targets.shape[1])
        K, r, unwind = nodes or (0, 0.0, False)
        if nodes is None:
            check_ladder_shape(S, T, float(max_step_sq))
        else:
            check_ladder_nodes_shape(S, K, T, float(max_step_sq), r)
        if S > self.max_batch:
            raise MinkHipError(f"n_seeds={S} exceeds max_batch={self.max_batch} of this problem")
        if refine and B > self.max_batch:
            raise MinkHipError(f"B={B} exceeds max_batch={self.max_batch} of this problem (a sweep of the refinement is one launch)")
        q = kit.want(kit.prep(q), ("B", m.nq), "q")
        frame_targets, posture_target, com_target = kit.prep(frame_targets), kit.prep(posture_target), kit.prep(com_target)
        flags = self._kernel_flags(wave_kernel, lane_kernel, quad_kernel, kit.devp | (FLAG_UNWIND_TURNS if unwind else 0)) | \
            self._held_flags(posture_target, com_target, (B, T))
        seeds = kit.want(kit.prep(seeds), (B, T, S, m.nq), "seeds")
        weights = kit.want(kit.prep(weights), (m.nv,), "weights")
        # (W, the nodes of a rung: what the *_all arrays hold)
        sizes = dict(B=B, T=T, S=S, K=K, W=S if nodes is None else K, q=m.nq, v=m.nv)
        empty, ptr = kit.empty, kit.ptr
        io, out = TRAJECTORY_LADDER_OUT.make[_on(("qvel", "all"), qvel_dt is not None, return_all)](
            empty, ptr, sizes, seeds=ptr(seeds), weights=ptr(weights), max_step_sq=float(max_step_sq),
            waypoint_dt=float(qvel_dt) if qvel_dt is not None else 0.0)
        rio = nio = None
        if refine:                                  # (tracked, repaired, refined: the pass's own; the path's outputs are `out`'s)
            rio, fixed = LADDER_REFINE_OUT.make[_NONE](empty, ptr, sizes)
            out.update(fixed)
            rio = C.byref(rio)
        if nodes is not None:
            nio, sets = LADDER_NODES_OUT.make[_NONE](empty, ptr, sizes)
            out.update(sets)
            nio = C.byref(nio)
        loops = (ptr(q), ptr(frame_targets), ptr(posture_target), ptr(com_target), float(dt), float(damping),
                 max_iters, float(pos_threshold), float(ori_threshold), int(rng_seed) & (2 ** 64 - 1), int(target_index0))
        result = TrajectoryLadderOut if nodes is None else TrajectoryLadderNodesOut
        if free is None:
            with self._lock, _attached(self, seed_table):
                if nodes is None:
                    _check(lib().mkh_solve_trajectory_ladder_refined(self.handle, B, T, S, *loops, C.byref(io), rio, flags, kit.stream))
                else:
                    _check(lib().mkh_solve_trajectory_ladder_nodes(self.handle, B, T, S, K, r, *loops, C.byref(io), nio, rio, flags,
                                                                   kit.stream))
            return result(**out)
        fio, more = LADDER_FREE_OUT.make[_NONE](empty, ptr, sizes)
        if len(free) == 3:
            cio, proof = LADDER_CERTIFIED_OUT.make[_NONE](empty, ptr, sizes)
            with _with_checker(self, free[0]), _attached(self, seed_table):
                _check(lib().mkh_solve_trajectory_ladder_certified(self.handle, free[0].handle, B, T, S, K, r, *loops, *free[2],
                                                                   C.byref(io), nio, rio, C.byref(fio), C.byref(cio), flags,
                                                                   kit.stream))
            return result(**out), LadderCertifiedOut(**more, **proof)
        call = lib().mkh_solve_trajectory_ladder_free_refined if refine else lib().mkh_solve_trajectory_ladder_free
        with _with_checker(self, free[0]), _attached(self, seed_table):
            _check(call(self.handle, free[0].handle, B, T, S, K, r, *loops, free[1], C.byref(io), nio, rio, C.byref(fio), flags,
                        kit.stream))
        return result(**out), LadderFreeOut(**more)

    def ladder_refine(self, q, q_path, tracked=None, frame_targets=None, posture_target=None, com_target=None, dt: float = 1e-2,
                      damping: float = 1e-12, *, max_iters: int, pos_threshold: float, ori_threshold: float,
                      max_step_sq: float = float("inf"), weights=None, v=None, status=None, iters=None, converged=None,
                      wave_kernel: bool = False, lane_kernel: bool = False, quad_kernel: bool = False) -> LadderRefineOut:
        return self._ladder_refine(q, q_path, tracked, frame_targets, posture_target, com_target, dt, damping, max_iters,
                                   pos_threshold, ori_threshold, max_step_sq, weights, v, status, iters, converged, wave_kernel,
                                   lane_kernel, quad_kernel, None)

    def ladder_refine_free(self, q, q_path, checker: "NativeProblem", tracked=None, frame_targets=None, posture_target=None,
                           com_target=None, dt: float = 1e-2, damping: float = 1e-12, *, max_iters: int, pos_threshold: float,
                           ori_threshold: float, edge_samples: int = 8, max_step_sq: float = float("inf"), weights=None, v=None,
                           status=None, iters=None, converged=None, wave_kernel: bool = False, lane_kernel: bool = False,
                           quad_kernel: bool = False) -> LadderRefineFreeOut:
        """mkh_ladder_refine_free: ladder_refine under "THE RULE OF THE REFINEMENT, with a checker" — `checker` a handle with
        collision limits on the same model and device; every repair candidate is checked as a node and the motions on both
        sides of it are swept with `edge_samples` interior samples, on the device between the loops."""
        checker = _checker_handle(self, checker, edge_samples)
        return self._ladder_refine(q, q_path, tracked, frame_targets, posture_target, com_target, dt, damping, max_iters,
                                   pos_threshold, ori_threshold, max_step_sq, weights, v, status, iters, converged, wave_kernel,
                                   lane_kernel, quad_kernel, (checker, int(edge_samples)))

    def _ladder_refine(self, q, q_path, tracked, frame_targets, posture_target, com_target, dt, damping, max_iters, pos_threshold,
                       ori_threshold, max_step_sq, weights, v, status, iters, converged, wave_kernel, lane_kernel, quad_kernel,
                       free):
        """The body of ladder_refine and ladder_refine_free (`free`: None, or (checker, edge_samples)).
        mkh_ladder_refine: the refinement pass of include/minkhip.h "THE RULE OF THE REFINEMENT" over the caller's path —
        q (B, nq) the current postures, q_path (B, T, nq), tracked (B, T) (None: every node), the targets in
        solve_trajectory_ladder's shapes, the loop parameters of the re-tracking sweeps, the squared break gate, weights (nv,)
        >= 0.  `v` (B, T, nv), `status`, `iters`, `converged` (B, T): what the caller knows of its path's nodes; copies come
        back with the rows of repaired nodes replaced.  numpy in → numpy out (synchronous); torch CUDA tensors in → torch
        tensors out on the current stream, no host copy."""
        m, kit = self.nmodel.model, _call_kit(q)
        B, max_iters = int(q.shape[0]), int(max_iters)
        if max_iters < 1:
            raise ValueError("max_iters must be >= 1")
        if not (float(pos_threshold) >= 0.0 and float(ori_threshold) >= 0.0):
            raise ValueError("thresholds must be >= 0: the refinement's loops run in threshold mode only")
        self._refuse_dense("ladder refinement")
        self._need_frame("a ladder refinement")
        kit.want(q_path, (B, "T", m.nq), "q_path", required=True)
        T = int(q_path.shape[1])
        check_ladder_shape(1, T, float(max_step_sq))
        if B > self.max_batch:
            raise MinkHipError(f"B={B} exceeds max_batch={self.max_batch} of this problem")
        q, q_path = kit.want(kit.prep(q), ("B", m.nq), "q"), kit.prep(q_path)
        frame_targets = kit.want(kit.prep(frame_targets), (B, T, self.n_frame, 7), "frame_targets", required=True)
        posture_target, com_target = kit.prep(posture_target), kit.prep(com_target)
        flags = self._kernel_flags(wave_kernel, lane_kernel, quad_kernel, kit.devp) | \
            self._held_flags(posture_target, com_target, (B, T))
        weights = kit.want(kit.prep(weights), (m.nv,), "weights")
        tracked = kit.ones((B, T)) if tracked is None else kit.flags01(tracked, (B, T), "tracked")
        sizes = dict(B=B, T=T, q=m.nq)
        known = dict(v=kit.f64_copy(v, (B, T, m.nv), "v"), status=kit.i32_copy(status, (B, T), "status"),
                     iters=kit.i32_copy(iters, (B, T), "iters"), converged=kit.i32_copy(converged, (B, T), "converged"))
        ptr = kit.ptr
        io, out = LADDER_REFINE_OUT.make[_ALONE](kit.empty, ptr, sizes, weights=ptr(weights), max_step_sq=float(max_step_sq),
                                                 **{n: ptr(x) for n, x in known.items()})
        out.update(known)                           # (the caller's in-out arrays come back as they are: the copies made above)
        loops = (B, T, kit.ptr(q), kit.ptr(q_path), kit.ptr(tracked), kit.ptr(frame_targets), kit.ptr(posture_target),
                 kit.ptr(com_target), float(dt), float(damping), max_iters, float(pos_threshold), float(ori_threshold))
        if free is None:
            with self._lock:
                _check(lib().mkh_ladder_refine(self.handle, *loops, C.byref(io), flags, kit.stream))
            return LadderRefineOut(**out)
        fio, more = LADDER_REFINE_FREE_OUT.make[_NONE](kit.empty, ptr, sizes)
        with _with_checker(self, free[0]):
            _check(lib().mkh_ladder_refine_free(self.handle, free[0].handle, *loops, free[1], C.byref(io), C.byref(fio), flags,
                                                kit.stream))
        return LadderRefineFreeOut(**out, **more)

    def _solve_trajectory(self, q, frame_targets, posture_target, com_target, dt, damping, n_steps, until, qvel_dt, tm,
                          warm_start, wave_kernel, lane_kernel, quad_kernel, keys=None, cands=None, free=None):
        m, kit = self.nmodel.model, _call_kit(q)
        B = int(q.shape[0])
        if n_steps < 1:
            raise ValueError("n_steps must be >= 1")
        if qvel_dt is not None and not float(qvel_dt) > 0.0:
            raise ValueError("qvel_dt must be > 0")
        if cands is not None:
            if cands[0] < 1:
                raise ValueError("n_seeds must be >= 1")
            if not (until[0] >= 0.0 and until[1] >= 0.0):
                raise ValueError("thresholds must be >= 0: multi-start trajectories run in threshold mode only")
            if B * cands[0] > self.max_batch:
                raise MinkHipError(f"B*n_seeds={B * cands[0]} exceeds max_batch={self.max_batch} of this problem")
        if B > self.max_batch:
            raise MinkHipError(f"B={B} exceeds max_batch={self.max_batch} of this problem")
        self._refuse_dense("trajectory")
        if until is not None:
            self._need_frame("threshold mode")
        flags = self._kernel_flags(wave_kernel, lane_kernel, quad_kernel, (FLAG_WARM_START if warm_start else 0) | kit.devp)
        q = kit.want(kit.prep(q), ("B", m.nq), "q")
        frame_targets, posture_target, com_target = kit.prep(frame_targets), kit.prep(posture_target), kit.prep(com_target)
        T = None
        if self.n_frame:
            shape = ("T", B, self.n_frame, 7) if tm else (B, "T", self.n_frame, 7)
            kit.want(frame_targets, shape, "frame_targets", required=True)
            T = int(frame_targets.shape[0 if tm else 1])
            if T < 1:
                raise ValueError(f"frame_targets must have shape {_shape_text(shape)} with T >= 1, got {tuple(frame_targets.shape)}")

        def held_or_timed(x, n, w, name, flag):
            """(per_waypoint, flags bit) of a posture / CoM target from its shape."""
            nonlocal T
            held = _held_or_rows(x, (B,), n, w, name, flag, strict=False)      # (n, w) / (B, n, w) as in solve(): no T axis
            if held is not None:
                return 0, held
            shp = tuple(x.shape)
            if len(shp) == 4:                                  # (B, T, n, w) / (T, B, n, w)
                Tx = shp[0 if tm else 1]
                T = Tx if T is None else T
                if shp == ((T, B, n, w) if tm else (B, T, n, w)):
                    return 1, flag
            elif len(shp) == 3 and shp[1:] == (n, w):          # (T, n, w); T == B was read as (B, ...) above
                T = shp[0] if T is None else T
                if shp[0] == T:
                    return 1, 0
            raise ValueError(f"{name} must have shape ({n}, {w}), (B, {n}, {w}), (T, {n}, {w}) or "
                             f"{'(T, B' if tm else '(B, T'}, {n}, {w}), got {shp}")

        p_time = c_time = 0
        if self.n_posture:
            p_time, f = held_or_timed(posture_target, self.n_posture, m.nq, "posture_target", FLAG_POSTURE_BATCHED)
            flags |= f
        if self.n_com:
            c_time, f = held_or_timed(com_target, self.n_com, 3, "com_target", FLAG_COM_BATCHED)
            flags |= f
        if T is None:
            raise ValueError("no target has a T axis: nothing says how many waypoints there are")
        if keys is not None:                                   # (the axis read off the shapes is the keyframes'; T is the waypoints')
            K, T = T, len(keys[1])
            if K != len(keys[0]):
                raise ValueError(f"the targets have {K} keyframes, keyframe_times has {len(keys[0])}")
        lead = (T, B) if tm else (B, T)
        sizes = dict(L=lead, B=B, T=T, q=m.nq, v=m.nv)
        until_on, qvel_on = until is not None, qvel_dt is not None
        empty, ptr = kit.empty, kit.ptr
        numbers = dict(waypoint_dt=float(qvel_dt) if qvel_on else 0.0, time_major=int(tm))
        thr = (float(until[0]), float(until[1])) if until_on else (-1.0, -1.0)
        loops = (ptr(q), ptr(frame_targets), ptr(posture_target), ptr(com_target))
        if cands is not None:
            S, rng_seed, target_index0, seeds, weights, want_all = cands
            seeds = kit.want(kit.prep(seeds), (B, S, m.nq), "seeds")
            weights = kit.want(kit.prep(weights), (m.nv,), "weights")
            sizes.update(R=B * S)
            cio, out = TRAJECTORY_MULTISTART_OUT.make[_on(("until", "qvel", "all"), until_on, qvel_on, want_all)](
                empty, ptr, sizes, seeds=ptr(seeds), weights=ptr(weights), posture_per_waypoint=p_time, com_per_waypoint=c_time, **numbers)
            args = (B, T, S, *loops, float(dt), float(damping), n_steps, thr[0], thr[1], rng_seed & (2 ** 64 - 1), target_index0)
            if free is None:
                _check(lib().mkh_solve_trajectory_multistart(self.handle, *args, C.byref(cio), flags, kit.stream))
                return TrajectoryMultistartOut(**out)
            fio, more = TRAJECTORY_FREE_OUT.make[_ALL if want_all else _NONE](empty, ptr, sizes)   # (the caller holds both locks)
            _check(lib().mkh_solve_trajectory_multistart_free(self.handle, free[0].handle, *args, free[1], C.byref(cio),
                                                              C.byref(fio), flags, kit.stream))
            return TrajectoryMultistartOut(**out), TrajectoryFreeOut(**more)
        if keys is not None:
            kt, wt, want_targets = keys
            group = lambda batched: lead if batched else (T,)
            sizes.update(P=group(flags & FLAG_POSTURE_BATCHED), C=group(flags & FLAG_COM_BATCHED), nf=self.n_frame, np=self.n_posture,
                         nc=self.n_com)
            kio, out = KEYFRAME_OUT.make[_on(("until", "qvel", "frames", "postures", "coms"), until_on, qvel_on,
                                             want_targets and self.n_frame, want_targets and p_time, want_targets and c_time)](
                empty, ptr, sizes, posture_keyframed=p_time, com_keyframed=c_time, **numbers)
            _check(lib().mkh_solve_keyframes(self.handle, B, K, T, *loops, kt.ctypes.data, wt.ctypes.data, float(dt), float(damping),
                                             n_steps, thr[0], thr[1], C.byref(kio), flags, kit.stream))
            paths = {n: out.pop(n) for n in KeyframesOut._fields[1:] if n in out}
            return KeyframesOut(TrajectoryOut(**out), **paths)
        io, out = TRAJECTORY_OUT.make[_on(("until", "qvel"), until_on, qvel_on)](empty, ptr, sizes, posture_per_waypoint=p_time,
                                                                        com_per_waypoint=c_time, **numbers)
        _check(lib().mkh_solve_trajectory(self.handle, B, T, *loops, float(dt), float(damping), n_steps, thr[0], thr[1], C.byref(io),
                                          flags, kit.stream))
        return TrajectoryOut(**out)
