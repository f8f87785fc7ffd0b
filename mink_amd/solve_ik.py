"""Batched `solve_ik` / `build_ik` with mink's signature (mink/solve_ik.py:43-105).

The Task/Limit objects are snapshotted into one device descriptor per call site
(cached on the Configuration by their constructor state); targets travel per call.
"""

from __future__ import annotations

import logging
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _native as nat
from . import exceptions
from .configuration import Configuration
from .distributed import shard_bounds
from .flatmodel import JNT_FREE

DEVICE_SOLVERS = ("mi355x", "hip", "quadprog")
PROBLEM_CACHE_SIZE = 16       # compiled descriptors kept per Configuration (least recently used are destroyed)
MAX_BOX_TERMS = 4             # ConfigurationLimits / VelocityLimits of one device descriptor (mkh_types.h kMaxBoxTerms)


class Problem(NamedTuple):
    """The (P, q, G, h) of qpsolvers.Problem, possibly with a leading batch dimension."""
    P: np.ndarray
    q: np.ndarray
    G: Optional[np.ndarray]
    h: Optional[np.ndarray]


def _key(x):
    if isinstance(x, dict):
        return tuple((k, _key(v)) for k, v in sorted(x.items()))
    if isinstance(x, np.ndarray):
        return (x.shape, x.tobytes())
    if isinstance(x, (list, tuple)):
        return tuple(_key(v) for v in x)
    return x


def _limit_rows(configuration: Configuration, lim, dt: float):
    """(G, h) of a caller-defined limit for every instance: (B, m, nv), (B, m); m = 0 when inactive."""
    B, nv = configuration.batch_size, configuration.nv
    c = lim.compute_qp_inequalities(configuration, dt)
    if c.inactive:
        return np.zeros((B, 0, nv)), np.zeros((B, 0))
    G, h = np.asarray(c.G, dtype=np.float64), np.asarray(c.h, dtype=np.float64)
    m = h.shape[-1]
    if G.shape not in ((m, nv), (B, m, nv)) or h.shape not in ((m,), (B, m)):
        raise exceptions.LimitDefinitionError(
            f"{type(lim).__name__}.compute_qp_inequalities must return G ({m}, {nv}) or ({B}, {m}, {nv}) and h ({m},) "
            f"or ({B}, {m}); got {G.shape}, {h.shape}")
    return np.broadcast_to(G, (B, m, nv)), np.broadcast_to(h, (B, m))


def _fold_box_rows(G: np.ndarray, h: np.ndarray):
    """Split the rows G·Δq ≤ h of a caller-defined limit into per-dof BOX bounds and general half-spaces.

    A row whose only nonzero entry (over the whole batch) sits in one column k is g·Δq_k ≤ h: an upper bound h / g for
    g > 0, a lower bound for g < 0.  The reference stacks such rows into its dense G like any other
    (mink/solve_ik.py:25-40) and quadprog treats them as general constraints; on the device they join lo ≤ Δq ≤ hi and
    cost no tableau row — an acceleration-style limit [I; −I] (2·nv rows) would otherwise never fit next to
    64 − nv half-space rows.  Returns (lo, hi, G_rest, h_rest, any_single): (B, nv), (B, nv), (B, m', nv), (B, m'), and whether
    the limit HAS single-entry rows at all — the structural fact the handle's layout is keyed on (their current values may
    all be inactive, h = +inf: the same handle must serve the next call where they are not)."""
    B, m, nv = G.shape
    lo, hi = np.full((B, nv), -np.inf), np.full((B, nv), np.inf)
    if m == 0:
        return lo, hi, G, h, False
    pattern = (G != 0.0).any(axis=0)                                # (m, nv): columns a row ever touches
    single = pattern.sum(axis=1) == 1
    for r in np.flatnonzero(single):
        k = int(np.flatnonzero(pattern[r])[0])
        g, hr = G[:, r, k], h[:, r]
        with np.errstate(divide="ignore", invalid="ignore"):
            b = hr / g
        pos, neg, zero = g > 0.0, g < 0.0, g == 0.0
        hi[pos, k] = np.minimum(hi[pos, k], b[pos])
        lo[neg, k] = np.maximum(lo[neg, k], b[neg])
        bad = zero & (hr < 0.0)                                     # 0·Δq ≤ h < 0: infeasible, as the reference would find
        hi[bad, k], lo[bad, k] = -np.inf, np.inf
    keep = ~single
    return lo, hi, G[:, keep], h[:, keep], bool(single.any())


def _fold_velocity_terms(terms):
    """At most MAX_BOX_TERMS VelocityLimit descriptors: the reference stacks any number (mink/solve_ik.py:25-40); the surplus is
    folded into the last term as elementwise minima.  Exact, not approximately so: the rows are ±Δq_k ≤ dt·v with dt > 0, and
    min over terms of dt·v equals dt·(min over terms of v) bitwise (rounding is monotone)."""
    if len(terms) <= MAX_BOX_TERMS:
        return terms
    vmin = {}
    for t in terms[MAX_BOX_TERMS - 1:]:
        for k, v in zip(np.asarray(t["indices"]).tolist(), np.asarray(t["limit"], dtype=np.float64).tolist()):
            vmin[k] = min(vmin.get(k, np.inf), v)
    idx = sorted(vmin)
    folded = {"indices": np.array(idx, dtype=np.int64), "limit": np.array([vmin[k] for k in idx], dtype=np.float64)}
    return list(terms[:MAX_BOX_TERMS - 1]) + [folded]


def _dense_inputs(configuration: Configuration, layout, dt: float):
    """Per-call arrays of the plugin route (mkh_solve_dense), None when the call site has no caller-defined rows."""
    if not layout["dense"] and not layout["dense_limits"]:
        return None
    if layout.get("dense_box") is not None:
        out_box = {"limit_lo": np.ascontiguousarray(layout["dense_box"][0]), "limit_hi": np.ascontiguousarray(layout["dense_box"][1])}
    else:
        out_box = {}
    out = {}
    if layout["dense"]:
        rows = [t._dense_rows(configuration) for t in layout["dense"]]
        out["task_e"] = np.ascontiguousarray(np.concatenate([e for e, _ in rows], axis=1))
        out["task_J"] = np.ascontiguousarray(np.concatenate([J for _, J in rows], axis=1))
    if layout["dense_limit_rows"]:
        rows = layout["dense_limit_data"]                             # evaluated by _compile at this call's dt
        out["limit_G"] = np.ascontiguousarray(np.concatenate([G for G, _ in rows], axis=1))
        out["limit_h"] = np.ascontiguousarray(np.concatenate([h for _, h in rows], axis=1))
    out.update(out_box)
    return out


def _compile(configuration: Configuration, tasks: Sequence, limits: Optional[Sequence], batch: int,
             dense_dt: float = 1.0, devices: Optional[Sequence[int]] = None):
    """The cached handle of a call site for `batch` instances, and its layout.  `devices`: the devices to compile for (default:
    the configuration's list) — more than one gives a ShardedProblem, `batch` split among them."""
    from .limits import ConfigurationLimit
    from .tasks import Task

    if limits is None:
        limits = configuration._default_limits                       # mink/solve_ik.py:28-29
        if limits is None:
            limits = configuration._default_limits = [ConfigurationLimit(configuration.model)]
    # Memo for control loops: the same task / limit objects with the same costs → the same handle and layout, without
    # rebuilding and hashing every descriptor (78 µs of a 185 µs G1 iteration; tools/bench_control_loop.py).
    fps = [x._fingerprint() for x in tasks] + [x._fingerprint() for x in limits]
    # (a device list of its own — an outer loop that uses fewer devices than the configuration lists — is a handle of its own)
    devices = list(configuration.devices if devices is None else devices)
    on = () if devices == configuration.devices else (tuple(devices),)
    memo_key = None if any(f is None for f in fps) else (tuple(fps), len(tasks), batch) + on
    if memo_key is not None:
        hit = configuration._compile_memo.get(memo_key)
        if hit is not None and hit[0] in configuration._problems:
            prob = configuration._problems.pop(hit[0])
            configuration._problems[hit[0]] = prob                   # most recently used
            return prob, hit[1]
    groups = {"frame": [], "posture": [], "com": [], "cfg": [], "vel": [], "col": [], "dense": []}
    layout = {"frame": [], "posture": [], "com": [], "dense": [], "dense_limits": [], "dense_limit_rows": 0}
    for t in tasks:
        if t._is_dense():                                           # caller-defined Task subclass: dense rows
            kind, desc = Task._native_desc(t, configuration)
        else:
            kind, desc = t._native_desc(configuration)
        groups[kind].append(desc)
        layout[kind].append(t)
    for lim in limits:
        if lim._is_dense():                                         # caller-defined Limit subclass: dense rows
            layout["dense_limits"].append(lim)
            continue
        kind, desc = lim._native_desc()
        if kind in ("cfg", "vel") and len(desc["indices"]) == 0:
            continue                                                # inactive Constraint() (solve_ik.py:34)
        groups[kind].append(desc)
    if len(groups["cfg"]) > MAX_BOX_TERMS:
        # (no exact fold: the gains differ, and a ball joint's distance to its limit is not monotone in the bound)
        raise exceptions.LimitDefinitionError(
            f"{len(groups['cfg'])} ConfigurationLimits in one call; the device evaluates at most {MAX_BOX_TERMS} "
            f"(merge limits that share a gain into one, with the tighter lower / upper per joint)")
    groups["vel"] = _fold_velocity_terms(groups["vel"])
    if layout["dense_limits"]:
        # the row count of a plugin limit is only known from what it returns: evaluate once here (dt does not change
        # the shape), keep the rows for this call
        raw = [_limit_rows(configuration, lim, dense_dt) for lim in layout["dense_limits"]]
        folded = [_fold_box_rows(np.asarray(G), np.asarray(h)) for G, h in raw]
        layout["dense_limit_data"] = [(G, h) for _, _, G, h, _ in folded]
        layout["dense_limit_rows"] = sum(h.shape[-1] for _, h in layout["dense_limit_data"])
        lo = np.maximum.reduce([f[0] for f in folded]); hi = np.minimum.reduce([f[1] for f in folded])
        if any(f[4] for f in folded):          # (structural: a box limit whose rows are all inactive now keeps its handle)
            layout["dense_box"] = (lo, hi)
        # (more general rows than the 64 − nv a wavefront holds: the instances in which that many are active are solved again by
        #  the workgroup-per-problem kernel with every row, as the reference's np.vstack would — mink/solve_ik.py:25-40; its
        #  workspace holds 448 rows per instance)
        cap = 448
        if layout["dense_limit_rows"] > cap:
            names = ", ".join(type(lim).__name__ for lim in layout["dense_limits"])
            raise exceptions.LimitDefinitionError(
                f"caller-defined limits ({names}) contribute {layout['dense_limit_rows']} general rows G·Δq ≤ h (rows with a "
                f"single nonzero entry are folded into the per-dof box and do not count); at most {cap} half-space rows per "
                f"instance, shared with collision contacts")
    key = (_key(groups), batch, layout["dense_limit_rows"], layout.get("dense_box") is not None) + on
    cache = configuration._problems
    prob = cache.pop(key, None)
    if prob is None:
        kwargs = dict(frame_tasks=groups["frame"], posture_tasks=groups["posture"],
                      com_tasks=groups["com"], configuration_limits=groups["cfg"], velocity_limits=groups["vel"],
                      collision_limits=groups["col"], max_batch=batch, dense_tasks=groups["dense"],
                      dense_limit_rows=layout["dense_limit_rows"], dense_limit_box=layout.get("dense_box") is not None)
        if len(devices) > 1 and batch >= len(devices):
            from .distributed import ShardedProblem                  # one handle per listed device, rows split among them
            prob = ShardedProblem(configuration.model, devices, **kwargs)
        else:
            prob = nat.NativeProblem(configuration.native, **kwargs)
    cache[key] = prob                                               # (re)insert as most recently used
    # Costs, gains and lm_damping are part of the device descriptor, so a caller that retunes a cost every control
    # step compiles a new descriptor every step: bound the cache (LRU) and free the evicted device buffers.  A handle
    # that a caller up the stack is about to solve on is pinned: caller-defined tasks evaluate built-in ones
    # (Task._eval → _compile) between the outer _compile and its solve, and must not evict the outer handle.
    pinned = configuration._pinned_problems
    for old in [k for k in cache if k not in pinned][:max(0, len(cache) - PROBLEM_CACHE_SIZE)]:
        cache.pop(old).close()
    layout["cache_key"] = key
    if memo_key is not None:
        if len(configuration._compile_memo) >= 4 * PROBLEM_CACHE_SIZE:
            configuration._compile_memo.clear()
        configuration._compile_memo[memo_key] = (key, layout)
    return prob, layout


class _pin:
    """Keep a compiled handle out of LRU eviction while its caller still has to solve on it."""

    def __init__(self, configuration: Configuration, layout):
        self.pins, self.key = configuration._pinned_problems, layout["cache_key"]

    def __enter__(self):
        self.pins[self.key] = self.pins.get(self.key, 0) + 1

    def __exit__(self, *exc):
        n = self.pins[self.key] - 1
        if n:
            self.pins[self.key] = n
        else:
            del self.pins[self.key]


def _gather_targets(configuration: Configuration, layout):
    B = configuration.batch_size
    ft = pt = ct = None
    if layout["frame"]:
        ft = np.stack([t._native_target(configuration) for t in layout["frame"]], axis=1)
    if layout["posture"]:
        rows = [t._native_target(configuration) for t in layout["posture"]]
        if any(r.ndim == 2 for r in rows):
            pt = np.stack([np.broadcast_to(r, (B, r.shape[-1])) for r in rows], axis=1)
        else:
            pt = np.stack(rows, axis=0)
    if layout["com"]:
        rows = [t._native_target(configuration) for t in layout["com"]]
        if any(r.ndim == 2 for r in rows):
            ct = np.stack([np.broadcast_to(r, (B, 3)) for r in rows], axis=1)
        else:
            ct = np.stack(rows, axis=0)
    return ft, pt, ct


def build_ik(configuration: Configuration, tasks: Sequence, dt: float, damping: float = 1e-12,
             limits: Optional[Sequence] = None) -> Problem:
    """mink/solve_ik.py:43-65: the dense QP (P, q, G, h) — evaluated on the device, returned for
    inspection.  G/h stack the limits in list order exactly like the reference."""
    from .limits import ConfigurationLimit

    prob, layout = _compile(configuration, tasks, limits, configuration.batch_size, dt)
    ft, pt, ct = _gather_targets(configuration, layout)
    with _pin(configuration, layout):
        _, _, out = prob.solve(configuration.q_batch, ft, pt, ct, dt, damping, taps=["H", "c"], solve_qp=False,
                               dense=_dense_inputs(configuration, layout, dt))
    lims = [ConfigurationLimit(configuration.model)] if limits is None else limits
    G_list, h_list = [], []
    for lim in lims:
        c = lim.compute_qp_inequalities(configuration, dt)
        if not c.inactive:
            G_list.append(np.asarray(c.G)); h_list.append(np.asarray(c.h))
    un = configuration._unbatch
    if not G_list:
        return Problem(un(out["H"]), un(out["c"]), None, None)
    B = configuration.batch_size

    def bcast(a, nd):
        return a if (not configuration.batched or a.ndim == nd + 1) else np.broadcast_to(a, (B,) + a.shape)

    G = np.concatenate([bcast(g, 2) for g in G_list], axis=-2)
    h = np.concatenate([bcast(x, 1) for x in h_list], axis=-1)
    return Problem(un(out["H"]), un(out["c"]), G, h)


def solve_ik(configuration: Configuration, tasks: Sequence, dt: float, solver: str = "mi355x",
             damping: float = 1e-12, safety_break: bool = False, limits: Optional[Sequence] = None,
             return_status: bool = False, **kwargs) -> np.ndarray:
    """Velocity tangent to the batch of configurations (mink/solve_ik.py:68-105).

    `solver` is kept for signature compatibility; every value selects the device active-set
    solver (the reference forwards the string to qpsolvers).  Returns v of shape (nv,) or (B, nv).

    The reference forwards `**kwargs` to the QP solver; the one understood here is `warm_start=True` for closed loops
    (solve, integrate, solve again on the same batch): the active-set phase starts from where the previous solve of the
    same tasks / limits on this configuration ended (MKH_FLAG_WARM_START) — same optimum, fewer pivots once the loop has
    run for a few steps.  Other solver keywords are accepted and ignored.
    """
    warm_start = bool(kwargs.pop("warm_start", False))
    del kwargs
    prob, layout = _compile(configuration, tasks, limits, configuration.batch_size, dt)
    ft, pt, ct = _gather_targets(configuration, layout)
    with _pin(configuration, layout):
        v, status = prob.solve(configuration.q_batch, ft, pt, ct, dt, damping,
                               dense=_dense_inputs(configuration, layout, dt), warm_start=warm_start)
    if (status & nat.ST_OUTSIDE_LIMITS).any():
        configuration.check_limits(safety_break=safety_break)      # raises / warns like the reference
    bad = np.nonzero(status & ~nat.ST_OUTSIDE_LIMITS)[0]
    if len(bad):
        s = int(status[bad[0]])
        why = ("constraints are inconsistent, no solution" if s & nat.ST_INFEASIBLE else
               "matrix P is not positive definite" if s & nat.ST_NOT_PD else
               "active-set iteration limit reached" if s & nat.ST_ITER_LIMIT else
               "more simultaneous contacts than tableau rows")
        raise exceptions.SolverError(f"QP failed for {len(bad)} of {len(status)} instances "
                                     f"(first: index {int(bad[0])}, status {s}): {why}")
    v = configuration._unbatch(v)
    if return_status:
        return v, configuration._unbatch(status)
    return v


def solve_ik_steps(configuration: Configuration, tasks: Sequence, dt: float, n_steps: int,
                   solver: str = "mi355x", damping: float = 1e-12, safety_break: bool = False,
                   limits: Optional[Sequence] = None, update: bool = True,
                   pos_threshold: Optional[float] = None, ori_threshold: Optional[float] = None):
    """`n_steps` iterations of  v = solve_ik(...); configuration.integrate_inplace(v, dt)  fused in one
    kernel launch (the loop mink's callers write themselves, e.g. examples/arm_ur5e_actuators.py:88-97).

    Returns (q_final, v_last); with `update` the configuration is advanced in place.

    With `pos_threshold` / `ori_threshold` the loop is the callers' real one — it breaks, per instance, as soon as
    every frame task's error is within the thresholds after the integration (arm_ur5e_actuators.py:93-97), `n_steps`
    is max_iters — and the return value is (q_final, v_last, iters, converged).

    Robots of 17 … 32 dofs or links loop on the row kernel's two-row build, floating base included, where that measured faster
    than the wavefront kernel's loop (a ComTask or RelativeFrameTask, or no floating base), and where every free
    joint is on a task chain."""
    until = _thresholds(pos_threshold, ori_threshold)
    prob, layout = _compile(configuration, tasks, limits, configuration.batch_size, dt)
    _refuse_plugin_rows(layout, "solve_ik_steps")
    ft, pt, ct = _gather_targets(configuration, layout)
    res = prob.solve(configuration.q_batch, ft, pt, ct, dt, damping, n_steps=int(n_steps), until=until)
    q, v, status = res[:3]
    if (status & nat.ST_OUTSIDE_LIMITS).any():
        # The bit is the OR over the fused steps (the reference loop checks every iteration, solve_ik.py:97): the
        # start configuration first, then — a violation that appeared at step k > 0 — the last one.  An instance
        # that left and re-entered its limits in between only warns.
        # With safety_break the two check_limits calls raise NotWithinConfigurationLimits like the reference; without
        # it ONE warning is logged (a control loop calls this every tick: no fresh Configuration, no warning per joint).
        if safety_break:
            configuration.check_limits(safety_break=True)
            Configuration(configuration.model, q, device=configuration.device).check_limits(safety_break=True)
        logging.warning("solve_ik_steps: %d instance(s) were outside their configuration limits at some fused step",
                        int(((status & nat.ST_OUTSIDE_LIMITS) != 0).sum()))
    bad = np.nonzero(status & ~nat.ST_OUTSIDE_LIMITS)[0]
    if len(bad):
        raise exceptions.SolverError(f"QP failed for {len(bad)} of {len(status)} instances "
                                     f"(first: index {int(bad[0])}, status {int(status[bad[0]])})")
    if update:
        configuration.update(q if configuration.batched else q[0])
    if until is not None:
        return (configuration._unbatch(q), configuration._unbatch(v), configuration._unbatch(res[3]),
                configuration._unbatch(res[4].astype(bool)))
    return configuration._unbatch(q), configuration._unbatch(v)


def _thresholds(pos_threshold, ori_threshold):
    """The (pos, ori) pair of a threshold-terminated loop, None when neither is given (one alone: the other never decides)."""
    if pos_threshold is None and ori_threshold is None:
        return None
    return (float(pos_threshold if pos_threshold is not None else np.inf),
            float(ori_threshold if ori_threshold is not None else np.inf))


def _refuse_plugin_rows(layout, who: str) -> None:
    if layout["dense"] or layout["dense_limits"]:
        raise exceptions.TaskDefinitionError(
            f"{who} fuses the outer loop on the device; caller-defined Task / Limit subclasses are evaluated on "
            "the host at every step: call solve_ik + integrate_inplace in a loop instead")


class MultistartResult(NamedTuple):
    """Result of solve_ik_multistart: per target the chosen seed's final configuration `q`, its last velocity `v`, whether any
    seed `converged`, the chosen `seed_index` (0 when none did), `n_converged` of the S seeds, and the chosen seed's `iters`
    and `status`.  With return_all also every instance's `q_all` (B, S, nq), `converged_all`, `iters_all`, `status_all`
    (B, S) and the `seeds` (B, S, nq) the loops started from; None otherwise."""
    q: np.ndarray
    v: np.ndarray
    converged: np.ndarray
    seed_index: np.ndarray
    n_converged: np.ndarray
    iters: np.ndarray
    status: np.ndarray
    q_all: Optional[np.ndarray] = None
    converged_all: Optional[np.ndarray] = None
    iters_all: Optional[np.ndarray] = None
    status_all: Optional[np.ndarray] = None
    seeds: Optional[np.ndarray] = None


def _host_array(x, name: str):
    """An optional array argument as float64 numpy (a torch tensor, wherever it lives, is brought to the host: the
    Configuration holds its q there)."""
    if x is None:
        return None
    if nat._is_torch(x):
        x = x.detach().cpu().numpy()
    try:
        return np.ascontiguousarray(x, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{name} must be an array of numbers") from e


def _optional_array(x, name: str, row: tuple, B: Optional[int] = None):
    """An optional argument (seeds, reference, weights) on the host with its shape checked: `row`, or — given `B` — one row for
    the whole batch or one per instance, returned as (B,) + row."""
    x = _host_array(x, name)
    if x is None:
        return None
    if B is None:
        if x.shape != row:
            raise ValueError(f"{name} must have shape {row}, got {x.shape}")
    elif x.shape == row:
        x = np.ascontiguousarray(np.broadcast_to(x, (B,) + row))
    elif x.shape != (B,) + row:
        raise ValueError(f"{name} must have shape {row} or {(B,) + row}, got {x.shape}")
    return x


def _compile_outer(configuration: Configuration, tasks, limits, dt: float, who: str, S: int, max_instances: int):
    """The handle(s) of an outer-loop call with S loop rows per instance, and its plan: (handles, layout, chunk, n_dev).  The
    instances are walked in chunks of `chunk` — as many as fit `max_instances` loop rows — and the configuration's first
    `n_dev` devices share a chunk by instance: one NativeProblem, or the shards of a ShardedProblem, each sized for its share."""
    B, devices = configuration.batch_size, configuration.devices
    chunk = min(B, max(1, int(max_instances) // S))
    n_dev = len(devices) if (len(devices) > 1 and chunk >= len(devices)) else 1
    shard = -(-chunk // n_dev)
    prob, layout = _compile(configuration, tasks, limits, n_dev * shard * S, dt, devices=devices[:n_dev])
    _refuse_plugin_rows(layout, who)
    return ([prob] if n_dev == 1 else prob.shards), layout, chunk, n_dev


def _rows(x, held_ndim: int, lo: int, hi: int):
    """Rows [lo, hi) of an optional per-instance array; one that is held for the batch (`held_ndim` axes) as it is."""
    return None if x is None else (x if x.ndim == held_ndim else np.ascontiguousarray(x[lo:hi]))


def _join(cls, parts):
    """The jobs' results, concatenated by instance into one `cls` (a NamedTuple whose absent fields are None in every part).
    Where a job returns a pair (out, more), `cls` is the pair of their types and the pair of the joined results comes back."""
    if type(parts[0]) is tuple:
        return tuple(_join(c, [p[k] for p in parts]) for k, c in enumerate(cls))
    return cls(*[None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=0) for k in range(len(cls._fields))])


def _present(configuration: Configuration, cls, sources, flags=(), **computed):
    """The caller's result `cls` from joined native results, BY FIELD NAME: every field of `cls` is `computed`'s where one is
    passed, else that of the first of `sources` (one result, or a tuple of them) that has it; None stays None, the fields named
    in `flags` become bool, and every array loses its leading axis for an unbatched configuration."""
    sources = sources if type(sources) is tuple else (sources,)
    un, fields, n_flags = configuration._unbatch, [], 0
    for f in cls._fields:
        n_flags += f in flags
        if f in computed:
            x = computed[f]
        else:
            x = None
            for s in sources:
                x = getattr(s, f, None)
                if x is not None:
                    break
        if x is None:
            if f not in cls._field_defaults:
                raise TypeError(f"{cls.__name__}.{f} is required and no native result carries it")
            fields.append(None)
        else:
            fields.append(un(x.astype(bool) if f in flags else x))
    if n_flags != len(flags):
        raise TypeError(f"{cls.__name__} has no field for one of the flags {flags}")
    return cls._make(fields)


def _loop_scalars(max_instances, n_seeds=None, loop: str = "max_iters", length=None, step_name: str = "waypoint_dt", step=None,
                  thresholds=None, whose: str = ""):
    """The scalar arguments of a fan-out call, judged on the host in one order: `n_seeds` (where the call has it), the loop
    `length` — of the keyword `loop`, max_iters or n_steps —, `max_instances`, the uniform `step` of the keyword `step_name`
    (None: not given) and, where `thresholds` = (pos, ori) is passed, both of them: `whose` loops run in threshold mode only.
    Returns (S, length) as ints, S None without n_seeds."""
    S = None if n_seeds is None else int(n_seeds)
    if S is not None and S < 1:
        raise ValueError("n_seeds must be >= 1")
    length = int(length)
    if length < 1:
        raise ValueError(f"{loop} must be >= 1")
    if int(max_instances) < 1:
        raise ValueError("max_instances must be >= 1")
    if step is not None and not float(step) > 0.0:
        raise ValueError(f"{step_name} must be > 0")
    if thresholds is not None:
        pos, ori = thresholds
        if pos is None or ori is None or not (float(pos) >= 0.0 and float(ori) >= 0.0):
            raise ValueError(f"thresholds must be >= 0: {whose} run in threshold mode only")
    return S, length


def _host_flags(x, name: str, row: tuple, B: int):
    """Optional flags (valid, tracked) on the host as a bool array (B,) + row: given as `row` for the whole batch, or one per
    instance; a torch tensor, wherever it lives, is brought to the host."""
    if x is None:
        return None
    x = np.asarray(x.detach().cpu().numpy() if nat._is_torch(x) else x)
    if x.shape not in (row, (B,) + row):
        raise ValueError(f"{name} must have shape {row} or {(B,) + row}, got {x.shape}")
    return np.ascontiguousarray(np.broadcast_to(x != 0, (B,) + row))


def _held_over(targets, B: int, L: int):
    """Posture / CoM targets of a call whose rows are (instance, goal) or (instance, waypoint): a batched target that is held
    over that second axis gets it — the native calls take (n, w) or (B, L, n, w)."""
    return [x if x is None or x.ndim != 3 else np.ascontiguousarray(np.broadcast_to(x[:, None], (B, L) + x.shape[1:]))
            for x in targets]


def _status_epilogue(status: np.ndarray, who: str, outside: str, failed: str, safety_break=None) -> None:
    """What an outer-loop call reports from its (B,) or (B, T) status bits, as solve_ik_steps does: ONE warning for instances
    that were outside their configuration limits at some step (`outside` names them), SolverError for a QP failure (`failed`:
    the message, with {n} failures of {of}, the {first} index and its {status}).  `safety_break`: a function that names the
    row at an index — the first row outside its limits then raises NotWithinConfigurationLimits instead of the warning."""
    out = (status & nat.ST_OUTSIDE_LIMITS) != 0
    if safety_break is not None and out.any():
        raise _outside_limits(f"{who}: {safety_break(*(int(x) for x in np.argwhere(out)[0]))} left its configuration limits at "
                              "some fused step")
    if status.ndim == 2:
        out = out.any(axis=1)
    if out.any():
        logging.warning(who + ": %d " + outside + " were outside their configuration limits at some fused step", int(out.sum()))
    # (ST_IN_COLLISION is no QP failure: a collision checker's verdict on the chosen row, which its status and converged = False state)
    bad = np.argwhere((status & ~(nat.ST_OUTSIDE_LIMITS | nat.ST_IN_COLLISION)) != 0)
    if len(bad):
        first = tuple(int(x) for x in bad[0])
        raise exceptions.SolverError(failed.format(n=len(bad), of=status.size, first=first[0] if status.ndim == 1 else first,
                                                   status=int(status[first])))


SEED_TABLE_MAX_K = 255         # entries per target of one query (include/minkhip.h "Seed tables")
SEED_TABLE_BUILD_BATCH = 4096  # instances per evaluation of the keys


class SeedTable:
    """Stored postures keyed on the end-effector poses they reach, for multi-start seeded from the nearest ones
    (include/minkhip.h "Seed tables"): pass it as `seed_table=` to solve_ik_multistart / solve_ik_trajectory_multistart and
    seeds 1 … n_seeds − 1 of every target are the table's entries nearest to that target instead of blind draws.

    `configuration` holds the single q the `n_entries` entries are drawn around, by multi-start's seeding rule at
    (rng_seed, t = j, s = 1) — free joints and unlimited slides keep its value, so the table of a floating-base robot belongs
    to that base pose.  `entries` (N, nq) are the table as given instead (earlier solutions, a teach-in set).  The keys are
    the world poses of the frames of the FrameTasks in `tasks`, in task order; the metric is
    Σ_f position_weight_f·|Δp|² + orientation_weight_f·4 sin²(θ/2), weights 1 where the task has a cost of that kind
    (RelativeFrameTasks: 0), or the (n_frame,) arrays given.  One device table per device is built on first use — its content
    is a function of (model, q, rng_seed) or of `entries` alone, so the shards of a multi-device call agree — through the
    configuration's compile cache; the table does not need that handle afterwards."""

    def __init__(self, configuration: Configuration, tasks: Sequence, n_entries: int = 16384, *, limits: Optional[Sequence] = None,
                 rng_seed: int = 0, entries=None, position_weight=None, orientation_weight=None):
        import threading

        if configuration.batch_size != 1:
            raise ValueError(f"configuration must hold a single q (the one the entries are drawn around), got a batch of "
                             f"{configuration.batch_size}")
        self.model, self.nq = configuration.model, configuration.nq
        self.q0 = np.array(configuration.q_batch[0], dtype=np.float64)
        entries = _host_array(entries, "entries")
        if entries is not None:
            if entries.ndim != 2 or entries.shape[1] != self.nq or len(entries) < 1:
                raise ValueError(f"entries must have shape (N, {self.nq}) with N >= 1, got {entries.shape}")
            n_entries = len(entries)
        self.n_entries = int(n_entries)
        if self.n_entries < 1:
            raise ValueError("n_entries must be >= 1")
        self.entries, self.rng_seed = entries, int(rng_seed)
        descs = [t._native_desc(configuration) for t in tasks if not t._is_dense()]
        frames = [d for kind, d in descs if kind == "frame"]
        self.n_frame = len(frames)
        plain = lambda d, part: d.get("root_type") is None and any(float(c) > 0.0 for c in d["cost"][part])
        default = [np.array([1.0 if plain(d, part) else 0.0 for d in frames]) for part in (slice(0, 3), slice(3, 6))]
        if not (default[0].any() or default[1].any()):
            raise ValueError(f"the tasks hold no plain FrameTask with a non-zero cost ({self.n_frame} frame tasks): nothing to key "
                             "the entries on")
        w = []
        for x, name, dflt in ((position_weight, "position_weight", default[0]), (orientation_weight, "orientation_weight", default[1])):
            x = _optional_array(x, name, (self.n_frame,))
            if x is not None and not (np.isfinite(x).all() and (x >= 0.0).all()):
                raise ValueError(f"{name} must be finite and >= 0")
            w.append(dflt if x is None else x)
        if not (w[0].any() or w[1].any()):
            raise ValueError("position_weight and orientation_weight are all 0: every entry would be at distance 0")
        self.position_weight, self.orientation_weight = w
        self._configuration, self._tasks = configuration, list(tasks)
        self._limits = None if limits is None else list(limits)
        self._tables, self._cfgs, self._host = {}, {configuration.device: configuration}, None
        self._lock = threading.Lock()
        self._closed = False

    # -- device tables
    def _table(self, device: int) -> "nat.NativeSeedTable":
        with self._lock:
            if self._closed:
                raise ValueError("the seed table is closed")
            tab = self._tables.get(device)
            if tab is None:
                cfg = self._cfgs.get(device)
                if cfg is None:
                    cfg = self._cfgs[device] = Configuration(self.model, self.q0, device=device)
                prob, layout = _compile(cfg, self._tasks, self._limits, min(self.n_entries, SEED_TABLE_BUILD_BATCH), devices=[device])
                _refuse_plugin_rows(layout, "SeedTable")
                with _pin(cfg, layout):
                    tab = nat.NativeSeedTable(prob, self.n_entries, self.q0, entries=self.entries, rng_seed=self.rng_seed,
                                              position_weight=self.position_weight, orientation_weight=self.orientation_weight)
                self._tables[device] = tab
            return tab

    def _native_for(self, problem) -> "nat.NativeSeedTable":
        return self._table(problem.nmodel.device)

    def _read(self):
        if self._host is None:
            self._host = self._table(self._configuration.device).read()
        return self._host

    @property
    def q(self) -> np.ndarray:
        """(N, nq): the entries."""
        return self._read()[0]

    @property
    def poses(self) -> np.ndarray:
        """(N, n_frame, 7): the world pose (wxyz, xyz) of every frame-task frame at every entry."""
        return self._read()[1]

    def _check_k(self, k: int, what: str = "k") -> int:
        k = int(k)
        if k < 1:
            raise ValueError(f"{what} = {k} must be >= 1")
        if k > SEED_TABLE_MAX_K:
            raise ValueError(f"{what} = {k}: a seed table returns at most {SEED_TABLE_MAX_K} entries per target")
        if k > self.n_entries:
            raise ValueError(f"{what} = {k} exceeds the seed table's {self.n_entries} entries")
        return k

    def query(self, targets, k: int):
        """The k entries nearest to each target: (index (B, k), distance (B, k), q (B, k, nq)), ascending, ties to the lower
        index.  `targets` (B, n_frame, 7) — or (B, 7) / (7,) with one frame task — as numpy (→ numpy) or as a torch tensor on
        a device (→ torch tensors there, on the current stream)."""
        k = self._check_k(k)
        is_torch = nat._is_torch(targets)
        t = targets if is_torch else _host_array(targets, "targets")
        if t.ndim == 1:
            t = t.reshape(1, -1)
        if t.ndim == 2 and self.n_frame == 1:
            t = t.reshape(t.shape[0], 1, t.shape[1])
        if t.ndim != 3 or tuple(t.shape[1:]) != (self.n_frame, 7) or t.shape[0] < 1:
            raise ValueError(f"targets must have shape (B, {self.n_frame}, 7), got {tuple(targets.shape)}")
        if is_torch:
            device = t.device.index if t.device.index is not None else 0
        else:
            device = self._configuration.device
        return self._table(device).query(t, k)

    def close(self) -> None:
        with self._lock:
            self._closed = True
            for tab in self._tables.values():
                tab.close()
            self._tables = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Clearance(NamedTuple):
    """Result of CollisionChecker.clearance, each with the leading shape of the rows: `margin` = min_k (d_k − dmin_k), the `pair`
    (index into the checker's pair list) that attains it — the lowest on a tie —, `n_violated` pairs closer than their minimum
    distance, `in_collision` = not (margin >= 0) — a NaN row is in collision —, and, asked for, every `distance` d_k
    (..., n_pairs), capped at the pair's detection distance."""
    margin: object
    pair: object
    n_violated: object
    in_collision: object
    distance: object = None


class SweptClearance(NamedTuple):
    """Result of CollisionChecker.swept_clearance, each with the leading shape of the edges: `margin` = the smallest clearance
    margin over the interior samples of the straight joint-space move, `sample` the (lowest) sample index that attains it,
    `pair` the pair of that sample's clearance, `in_collision` = not (margin >= 0) — a NaN or infinite end collides."""
    margin: object
    sample: object
    pair: object
    in_collision: object


class CertifiedSweep(NamedTuple):
    """Result of CollisionChecker.certified_sweep, each with the leading shape of the edges (include/minkhip.h "THE RULE OF THE
    CERTIFIED SWEEP").  `n_samples` interior samples were chosen from `motion`, the bound on how far the edge moves any pair of
    geoms against each other (`capped`: the resolution asked for more than max_samples).  `margin`, `sample`, `pair`: the
    smallest clearance margin over the n_samples + 2 points, ends included, the (lowest) point 0 .. n_samples + 1 that attains
    it and that point's pair.  `lower_bound`: what the margin of any pair can fall to BETWEEN the points at the worst, attained
    on `segment` 0 .. n_samples by `bound_pair`; -inf where the motion has no bound.  `verdict`: 2 collides — not (margin >= 0) —,
    1 certified free — margin >= 0 and lower_bound >= 0: every pair keeps its minimum distance along the whole edge —, 0
    undecided.  `certified` = verdict == 1, `in_collision` = verdict == 2."""
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
    certified: object
    in_collision: object


class CollisionChecker:
    """Clearance of configurations on the device, and the `collision_check=` of solve_ik_multistart / solve_ik_solutions /
    solve_ik_goalset (include/minkhip.h "THE RULE OF CLEARANCE").

    `limits`: built-in CollisionAvoidanceLimit objects of `model`; their geom pairs, in order, are the pair list — pair k with
    its limit's minimum_distance_from_collisions and collision_detection_distance (gain and bound_relaxation do not enter).
    A row is in collision when some pair is closer than its minimum distance.  One native handle per device model is built on
    first use, for `max_rows` rows per launch (more rows are walked in chunks).

    `sweep_rows`: what the calls that judge the MOTION between configurations — swept_clearance, ladder_path and
    solve_ik_trajectory_ladder with `collision_check=` — need of a checker with general convex pairs (cylinder-box,
    cylinder-cylinder, ellipsoids, mesh hulls): a device buffer for the distances of those pairs at `sweep_rows` swept samples,
    8 bytes per such pair and sample.  Such a call walks its edges in chunks of sweep_rows // n_samples edges; the results do
    not depend on the value, which must be at least the call's samples per edge.  0, the default: those calls refuse such a
    checker.  A checker of analytic pairs alone never needs it.

    `check_rows`: what the calls that judge rows they produce themselves — candidate_path and
    solve_ik_trajectory_multistart with `collision_check=`, refine_path with `collision_check=` and
    solve_ik_trajectory_ladder(refine="free") — need of such a checker: a second device buffer, for the distances of those pairs
    on `check_rows` judged rows (a node, or a sample of an edge into it), 8 bytes per such pair and row.  Candidate tracking needs
    check_rows >= 1 + edge_samples and judges its candidate rows in chunks of check_rows // (1 + edge_samples); the two
    refinement calls need check_rows >= 1 + 2 edge_samples AND sweep_rows >= edge_samples and judge the loop results of a
    waypoint step in chunks of check_rows // (1 + 2 edge_samples).  The results do not depend on the value.  0, the default:
    those calls refuse such a checker.  A checker of analytic pairs alone never needs it."""

    def __init__(self, model, limits: Sequence, max_rows: int = 65536, sweep_rows: int = 0, check_rows: int = 0):
        import threading
        from .configuration import as_flat_model
        from .limits import CollisionAvoidanceLimit

        self.model = as_flat_model(model)
        limits = list(limits)
        for lim in limits:
            if not isinstance(lim, CollisionAvoidanceLimit) or lim._is_dense():
                raise exceptions.LimitDefinitionError(
                    f"a CollisionChecker takes built-in CollisionAvoidanceLimit objects, got {type(lim).__name__}"
                    + (" (a subclass that overrides compute_qp_inequalities has no pair list the device evaluates)"
                       if isinstance(lim, CollisionAvoidanceLimit) else ""))
        self._descs = [lim._native_desc()[1] for lim in limits]
        pairs = [d["geom_id_pairs"].reshape(-1, 2) for d in self._descs]
        self.geom_id_pairs = np.concatenate(pairs, axis=0).astype(np.int32) if pairs else np.zeros((0, 2), np.int32)
        self.n_pairs = int(len(self.geom_id_pairs))
        if self.n_pairs < 1:
            raise exceptions.LimitDefinitionError("a CollisionChecker needs at least one geom pair")
        self.minimum_distance = np.concatenate([np.full(len(p), float(d["minimum_distance_from_collisions"]))
                                                for p, d in zip(pairs, self._descs)])
        self.detection_distance = np.concatenate([np.full(len(p), float(d["collision_detection_distance"]))
                                                  for p, d in zip(pairs, self._descs)])
        self.max_rows = int(max_rows)
        if self.max_rows < 1:
            raise ValueError("max_rows must be >= 1")
        if isinstance(sweep_rows, bool) or not isinstance(sweep_rows, (int, np.integer)) or int(sweep_rows) < 0:
            raise ValueError(f"sweep_rows must be an int >= 0, got {sweep_rows!r}")
        self.sweep_rows = int(sweep_rows)
        if isinstance(check_rows, bool) or not isinstance(check_rows, (int, np.integer)) or int(check_rows) < 0:
            raise ValueError(f"check_rows must be an int >= 0, got {check_rows!r}")
        self.check_rows = int(check_rows)
        self._handles = {}                 # id(NativeModel) → (NativeModel, NativeProblem)
        self._lock = threading.Lock()
        self._closed = False

    def _handle(self, nmodel) -> "nat.NativeProblem":
        with self._lock:
            if self._closed:
                raise ValueError("the collision checker is closed")
            hit = self._handles.get(id(nmodel))
            if hit is None:
                prob = nat.NativeProblem(nmodel, collision_limits=self._descs, max_batch=self.max_rows)
                try:
                    if self.sweep_rows:
                        prob.set_sweep_rows(self.sweep_rows)
                    if self.check_rows:
                        prob.set_check_rows(self.check_rows)
                except Exception:
                    prob.close()
                    raise
                hit = self._handles[id(nmodel)] = (nmodel, prob)
            return hit[1]

    def _native_for(self, problem) -> "nat.NativeProblem":
        if problem.nmodel.model is not self.model:
            raise ValueError("collision_check belongs to another model than the configuration")
        return self._handle(problem.nmodel)

    def clearance(self, q_rows, return_distances: bool = False) -> Clearance:
        """The clearance of `q_rows` — (nq,), (N, nq) or (..., nq); the outputs take the leading shape.  numpy (or anything
        array-like) in → numpy out; a torch tensor on a device in → torch tensors there, on the current stream."""
        from .configuration import native_model

        if self._closed:
            raise ValueError("the collision checker is closed")
        nq = self.model.nq
        is_torch = nat._is_torch(q_rows)
        q = q_rows if is_torch else _host_array(q_rows, "q_rows")
        if q.ndim < 1 or int(q.shape[-1]) != nq:
            raise ValueError(f"q_rows must have shape (..., {nq}), got {tuple(q.shape)}")
        lead = tuple(int(x) for x in q.shape[:-1])
        if 0 in lead:
            raise ValueError(f"q_rows holds no row: shape {tuple(q.shape)}")
        if is_torch and q.device.type != "cuda":
            is_torch, q = False, _host_array(q, "q_rows")
        device = (q.device.index if q.device.index is not None else 0) if is_torch else 0
        o = self._handle(native_model(self.model, device)).clearance(q.reshape(-1, nq), bool(return_distances))
        return Clearance(o.margin.reshape(lead), o.pair.reshape(lead), o.n_violated.reshape(lead),
                         ~(o.margin >= 0.0).reshape(lead),
                         None if o.distance is None else o.distance.reshape(lead + (self.n_pairs,)))

    def swept_clearance(self, q_from, q_to, n_samples: int = 8) -> SweptClearance:
        """The swept clearance of the straight joint-space moves from `q_from` to `q_to` — (nq,), (N, nq) or (..., nq), the
        same shape —: `n_samples` interior samples per edge at u = i / (n_samples + 1), each judged as `clearance` judges a row
        (include/minkhip.h "THE RULE OF THE SWEEP"); the ends themselves are not sampled.  The samples are built and evaluated
        on the device.  A checker with general convex pairs (cylinder-box, ellipsoids, mesh hulls) needs `sweep_rows` >=
        n_samples (the constructor's keyword): MinkHipError without.
        numpy in → numpy out; torch tensors on a device in → torch tensors there, on the current stream."""
        from .configuration import native_model

        if self._closed:
            raise ValueError("the collision checker is closed")
        if int(n_samples) < 1:
            raise ValueError(f"n_samples must be >= 1, got {n_samples}")
        nq = self.model.nq
        is_torch = nat._is_torch(q_from) and nat._is_torch(q_to) and q_from.device.type == "cuda" and q_to.device == q_from.device
        a, b = (q_from, q_to) if is_torch else (_host_array(q_from, "q_from"), _host_array(q_to, "q_to"))
        if a.ndim < 1 or int(a.shape[-1]) != nq or tuple(b.shape) != tuple(a.shape):
            raise ValueError(f"q_from and q_to must have one shape (..., {nq}), got {tuple(a.shape)} and {tuple(b.shape)}")
        lead = tuple(int(x) for x in a.shape[:-1])
        if 0 in lead:
            raise ValueError(f"q_from holds no row: shape {tuple(a.shape)}")
        device = (a.device.index if a.device.index is not None else 0) if is_torch else 0
        o = self._handle(native_model(self.model, device)).swept_clearance(a.reshape(-1, nq), b.reshape(-1, nq), int(n_samples))
        return SweptClearance(o.margin.reshape(lead), o.sample.reshape(lead), o.pair.reshape(lead), ~(o.margin >= 0.0).reshape(lead))

    def certified_sweep(self, q_from, q_to, resolution: float, max_samples: int = 64) -> CertifiedSweep:
        """The straight joint-space moves from `q_from` to `q_to` — (nq,), (N, nq) or (..., nq), the same shape — swept at a
        sample count of their own and judged BETWEEN the samples as well (include/minkhip.h "THE RULE OF THE CERTIFIED SWEEP").
        `resolution` (metres, > 0): how far a pair of geoms may move against each other between two neighbouring points; an
        edge whose motion bound is `motion` gets ceil(motion / resolution) - 1 interior samples, at least 1 and at most
        `max_samples` (1 .. 4096), and both ends are judged too.  Certifying an edge takes margins of about resolution / 2 at
        the points, so a resolution at or above twice (detection distance - minimum distance) certifies nothing.  A checker
        with general convex pairs (cylinder-box, ellipsoids, mesh hulls) is refused: MinkHipError.
        numpy in → numpy out; torch tensors on a device in → torch tensors there, on the current stream."""
        from .configuration import native_model

        if self._closed:
            raise ValueError("the collision checker is closed")
        nq = self.model.nq
        is_torch = nat._is_torch(q_from) and nat._is_torch(q_to) and q_from.device.type == "cuda" and q_to.device == q_from.device
        a, b = (q_from, q_to) if is_torch else (_host_array(q_from, "q_from"), _host_array(q_to, "q_to"))
        if a.ndim < 1 or int(a.shape[-1]) != nq or tuple(b.shape) != tuple(a.shape):
            raise ValueError(f"q_from and q_to must have one shape (..., {nq}), got {tuple(a.shape)} and {tuple(b.shape)}")
        lead = tuple(int(x) for x in a.shape[:-1])
        if 0 in lead:
            raise ValueError(f"q_from holds no row: shape {tuple(a.shape)}")
        device = (a.device.index if a.device.index is not None else 0) if is_torch else 0
        o = self._handle(native_model(self.model, device)).certified_sweep(a.reshape(-1, nq), b.reshape(-1, nq), float(resolution),
                                                                           int(max_samples))
        return CertifiedSweep(*[x.reshape(lead) for x in o], (o.verdict == nat.SWEEP_CERTIFIED).reshape(lead),
                              (o.verdict == nat.SWEEP_COLLIDES).reshape(lead))

    def motion_reach(self, device: int = 0) -> np.ndarray:
        """The reach table of the pair list, (n_pairs, njnt, 2): per pair and joint, what multiplies the joint's linear and its
        angular travel along an edge in the motion bound of that pair (include/minkhip.h "THE RULE OF THE CERTIFIED SWEEP")."""
        from .configuration import native_model

        if self._closed:
            raise ValueError("the collision checker is closed")
        return self._handle(native_model(self.model, int(device))).motion_reach()

    def close(self) -> None:
        with self._lock:
            self._closed = True
            for _, prob in self._handles.values():
                prob.close()
            self._handles = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_collision_check(collision_check, configuration: Configuration, edge_samples=None, refine: bool = False):
    """The `collision_check=` keyword of the fan-out calls, judged on the host (`edge_samples`, `refine`: the ladder calls')."""
    if collision_check is None:
        return
    if refine:
        raise ValueError("refine=True together with collision_check: the refinement pass knows nothing of collisions")
    if edge_samples is not None and int(edge_samples) < 1:
        raise ValueError(f"edge_samples must be >= 1, got {edge_samples}")
    if not isinstance(collision_check, CollisionChecker):
        raise ValueError(f"collision_check must be a CollisionChecker, got {type(collision_check).__name__}")
    if collision_check.model is not configuration.model:
        raise ValueError("collision_check belongs to another model than the configuration")


def _check_seed_table(seed_table, seeds, configuration: Configuration, S: int):
    """The `seed_table=` keyword of the two multi-start calls, judged on the host."""
    if seed_table is None:
        return
    if seeds is not None:
        raise ValueError("seeds and seed_table are two sources of the same starts: pass one of them")
    if not isinstance(seed_table, SeedTable):
        raise ValueError(f"seed_table must be a SeedTable, got {type(seed_table).__name__}")
    if seed_table.nq != configuration.nq or seed_table.model.njnt != configuration.model.njnt:
        raise ValueError(f"seed_table belongs to another model (nq = {seed_table.nq}, this configuration: nq = {configuration.nq})")
    if S > 1:
        seed_table._check_k(S - 1, "n_seeds - 1")


def solve_ik_multistart(configuration: Configuration, tasks: Sequence, dt: float, n_seeds: int, max_iters: int,
                        pos_threshold: float, ori_threshold: float, solver: str = "mi355x", damping: float = 1e-12,
                        limits: Optional[Sequence] = None, rng_seed: int = 0, seeds=None, reference=None, weights=None,
                        update: bool = True, return_all: bool = False, max_instances: int = 1 << 20,
                        seed_table: Optional["SeedTable"] = None,
                        collision_check: Optional["CollisionChecker"] = None) -> MultistartResult:
    """Global IK by multi-start: the threshold-terminated loop of solve_ik_steps from `n_seeds` starts per target, the best
    solution picked on the device — seeding, target fan-out and selection happen there, in one call.

    Seed 0 of every target is the configuration's own q, so the result is never worse than solve_ik_steps from it.  The other
    starts are drawn per joint (limited hinge / slide: uniform in its range; unlimited hinge: within ±π of q; ball: a random
    rotation of at most its range; free joints and unlimited slides keep the caller's value) by a stateless generator — a pure
    function of (rng_seed, target index, seed index, joint): the result does not depend on `max_instances`, the device list or
    the batch around a target — or taken from `seeds`, (S, nq) or (B, S, nq) (row 0 is still replaced by q).

    Among the seeds that converged without a QP failure the one closest to `reference` (default: q) wins: smallest
    Σ_k weights_k·(q_s ⊖ reference)_k² in the tangent space, ties to the lowest index.  A target none of whose seeds converged
    returns seed 0's result with converged = False — exactly what solve_ik_steps returns from q.  Failures are reported for
    the CHOSEN seeds only, like solve_ik_steps reports them: a warning for configuration limits, SolverError for a QP failure
    (which can only be seed 0's, of a target where nothing converged); a failed random seed is just discarded.

    `seed_table` (a SeedTable; not together with `seeds`): seeds 1 … n_seeds − 1 of every target are the table's entries
    nearest to the target's frame poses, looked up on the device in front of the seed kernel — they depend on the target
    alone, not on rng_seed, chunks or shards.  The table is attached to the handle for this call only.

    `collision_check` (a CollisionChecker): directly behind the loops every seed's final q is checked on the device and a seed
    that is in collision gets ST_IN_COLLISION in its status and is not eligible — `n_converged` counts the seeds that converged
    AND are free, and `status_all` carries the bit.  With a checker the call is no longer "never worse than solve_ik_steps from
    q": where nothing is eligible the result is still seed 0's with converged = False — also when seed 0 converged into a
    collision, which its status then says (no SolverError for that bit).  Attached to the handle for this call only.

    When B·n_seeds exceeds `max_instances` the targets are walked in chunks; a multi-device configuration shards by target."""
    del solver
    S, max_iters = _loop_scalars(max_instances, n_seeds, length=max_iters)
    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    seeds = _optional_array(seeds, "seeds", (S, nq), B)
    reference = _optional_array(reference, "reference", (nq,), B)
    weights = _optional_array(weights, "weights", (nv,))
    _check_seed_table(seed_table, seeds, configuration, S)
    _check_collision_check(collision_check, configuration)
    handles, layout, chunk, n_dev = _compile_outer(configuration, tasks, limits, dt, "solve_ik_multistart", S, max_instances)
    ft, pt, ct = _gather_targets(configuration, layout)
    q = configuration.q_batch
    kw = dict(n_seeds=S, max_iters=max_iters, pos_threshold=float(pos_threshold), ori_threshold=float(ori_threshold),
              rng_seed=int(rng_seed), return_all=bool(return_all))

    def job(handle, lo, hi):
        return handle.solve_multistart(q[lo:hi], _rows(ft, 2, lo, hi), _rows(pt, 2, lo, hi), _rows(ct, 2, lo, hi), dt, damping,
                                       target_index0=lo, seeds=_rows(seeds, 2, lo, hi), reference=_rows(reference, 1, lo, hi),
                                       weights=weights, seed_table=seed_table, collision_check=collision_check, **kw)

    res = _join(nat.MultistartOut, _chunks_and_shards(configuration, layout, handles, B, chunk, n_dev, job))
    _status_epilogue(res.status, "solve_ik_multistart", "chosen instance(s)",
                     "QP failed for the chosen seed of {n} of {of} targets (first: index {first}, status {status}); "
                     "none of their seeds converged")
    if update:
        configuration.update(res.q if configuration.batched else res.q[0])
    return _present(configuration, MultistartResult, res, flags=("converged", "converged_all"))


class SolutionSet(NamedTuple):
    """Result of solve_ik_solutions: per target up to K distinct solutions in ascending distance from the reference — `q`
    (B, K, nq), `v` (B, K, nv), `valid` (B, K) (False: an empty slot, which repeats seed 0's result), `seed_index` (−1 in an
    empty slot), `distance` (+inf), `multiplicity` (the converged seeds the slot stands for; 0), `iters`, `status` (B, K) — and
    `n_distinct`, `n_converged`, `n_uncovered` (B,): slots filled, seeds that converged, converged seeds that no slot covers
    (0: the set is complete for these seeds).  With return_all also `q_all`, `converged_all`, `iters_all`, `status_all`, `seeds`
    as in MultistartResult.  Without the leading axis for an unbatched configuration."""
    q: np.ndarray
    v: np.ndarray
    valid: np.ndarray
    seed_index: np.ndarray
    distance: np.ndarray
    multiplicity: np.ndarray
    iters: np.ndarray
    status: np.ndarray
    n_distinct: np.ndarray
    n_converged: np.ndarray
    n_uncovered: np.ndarray
    q_all: Optional[np.ndarray] = None
    converged_all: Optional[np.ndarray] = None
    iters_all: Optional[np.ndarray] = None
    status_all: Optional[np.ndarray] = None
    seeds: Optional[np.ndarray] = None


class DistinctSet(NamedTuple):
    """Result of distinct_solutions: `q` (B, K, nq), `valid`, `seed_index` (the candidate's index; −1 in an empty slot),
    `distance`, `multiplicity` (B, K), and `n_distinct`, `n_valid`, `n_uncovered` (B,) — without the leading axis for an
    unbatched configuration."""
    q: np.ndarray
    valid: np.ndarray
    seed_index: np.ndarray
    distance: np.ndarray
    multiplicity: np.ndarray
    n_distinct: np.ndarray
    n_valid: np.ndarray
    n_uncovered: np.ndarray


def _set_args(n_solutions, min_distance, S=None):
    """(K, r) of a distinct set, judged on the host."""
    try:
        K, r = int(n_solutions), float(min_distance)
    except (TypeError, ValueError) as e:
        raise ValueError("n_solutions must be an integer and min_distance a number") from e
    nat.check_solution_set(K, r, S)
    return K, r


def solve_ik_solutions(configuration: Configuration, tasks: Sequence, dt: float, n_seeds: int, n_solutions: int, max_iters: int,
                       pos_threshold: float, ori_threshold: float, min_distance: float = 0.1, solver: str = "mi355x",
                       damping: float = 1e-12, limits: Optional[Sequence] = None, rng_seed: int = 0, seeds=None, reference=None,
                       weights=None, return_all: bool = False, max_instances: int = 1 << 20,
                       seed_table: Optional["SeedTable"] = None, unwind_turns: bool = False,
                       collision_check: Optional["CollisionChecker"] = None) -> SolutionSet:
    """The distinct IK solutions of every target that multi-start finds: solve_ik_multistart's seeds and loops — `n_seeds`
    starts per target, the same generator, `seeds`, `seed_table`, chunks and shards — and, instead of its one result, up to
    `n_solutions` converged results per target no two of which lie within `min_distance` of each other, picked and
    deduplicated on the device.

    Distances are multi-start's: d(a, b) = Σ_k weights_k·(a ⊖ b)_k² in the tangent space; two results are the same solution
    when d <= min_distance² (0: exact duplicates only).  The slots are filled in ascending distance from `reference`
    (default: q): slot 0 is what solve_ik_multistart returns, slot j the closest converged result that none of the slots
    before it covers; `multiplicity` counts the seeds a slot stands for.  Slots beyond `n_distinct` are empty — valid = False,
    seed 0's result in q.  `n_uncovered` > 0 says that more distinct solutions were found than `n_solutions` holds.  Two
    solutions a full turn of an unlimited hinge apart count as different — unless `unwind_turns` is set: every loop result is
    then moved to the turn nearest the reference first (the function unwind_turns; `q_all` returns the moved rows), so the
    slots go to IK branches and not to turns of one branch.  Slot 0 is then the closest MOVED result.

    `collision_check` (a CollisionChecker): as in solve_ik_multistart — colliding results get ST_IN_COLLISION behind the loops
    (in front of the unwinding) and fill no slot; `n_converged` counts the converged and free ones.  With a checker slot 0 is
    no longer "never worse than solve_ik_steps from q": an empty set repeats seed 0's result, whose status says so when it
    collides.

    The configuration is not changed: a set does not update it.  Failures are reported for slot 0 only, as
    solve_ik_multistart reports them for its choice."""
    del solver
    S, max_iters = _loop_scalars(max_instances, n_seeds, length=max_iters)
    K, r = _set_args(n_solutions, min_distance, S)
    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    seeds = _optional_array(seeds, "seeds", (S, nq), B)
    reference = _optional_array(reference, "reference", (nq,), B)
    weights = _optional_array(weights, "weights", (nv,))
    _check_seed_table(seed_table, seeds, configuration, S)
    _check_collision_check(collision_check, configuration)
    handles, layout, chunk, n_dev = _compile_outer(configuration, tasks, limits, dt, "solve_ik_solutions", S, max_instances)
    ft, pt, ct = _gather_targets(configuration, layout)
    q = configuration.q_batch
    kw = dict(n_seeds=S, n_solutions=K, min_distance=r, max_iters=max_iters, pos_threshold=float(pos_threshold),
              ori_threshold=float(ori_threshold), rng_seed=int(rng_seed), return_all=bool(return_all),
              unwind_turns=bool(unwind_turns))

    def job(handle, lo, hi):
        return handle.solve_multistart_set(q[lo:hi], _rows(ft, 2, lo, hi), _rows(pt, 2, lo, hi), _rows(ct, 2, lo, hi), dt, damping,
                                           target_index0=lo, seeds=_rows(seeds, 2, lo, hi), reference=_rows(reference, 1, lo, hi),
                                           weights=weights, seed_table=seed_table, collision_check=collision_check, **kw)

    res = _join(nat.SolutionSetOut, _chunks_and_shards(configuration, layout, handles, B, chunk, n_dev, job))
    _status_epilogue(res.status[:, 0], "solve_ik_solutions", "chosen instance(s)",
                     "QP failed for the chosen seed of {n} of {of} targets (first: index {first}, status {status}); "
                     "none of their seeds converged")
    return _present(configuration, SolutionSet, res, flags=("converged_all",), valid=res.seed_index >= 0)


def unwind_turns(configuration: Configuration, q_rows, reference=None) -> np.ndarray:
    """Move configurations to the full turn nearest a reference posture: q_rows (S, nq) or (B, S, nq); `reference` (nq,) or
    (B, nq) (default: the configuration's q).  Every hinge that is unlimited, or whose range spans at least 2π, is
    shifted by the whole number of turns that brings it nearest its reference value without leaving its range; every other
    entry — slides, short-range hinges, the quaternions of ball and free joints — is copied bit for bit.  The pose of the robot
    does not change (a hinge at x + 2πk is the hinge at x).  The rule in full, which the device and numpy restate bit for bit:
    include/minkhip.h "THE RULE OF THE UNWINDING".  Returns (B, S, nq) — (S, nq) for an unbatched configuration; the
    configuration is not changed."""
    from .tasks import PostureTask

    B, nq = configuration.batch_size, configuration.nq
    q_rows = _host_array(q_rows, "q_rows")
    if q_rows is None or q_rows.ndim not in (2, 3) or q_rows.shape[-1] != nq or q_rows.shape[-2] < 1 \
            or (q_rows.ndim == 3 and q_rows.shape[0] != B):
        raise ValueError(f"q_rows must have shape (S, {nq}) or ({B}, S, {nq}), got {None if q_rows is None else q_rows.shape}")
    rows = np.ascontiguousarray(np.broadcast_to(q_rows, (B, q_rows.shape[-2], nq)))
    reference = _optional_array(reference, "reference", (nq,), B)
    # (the kernel reads the model's joint table through a problem handle: the smallest one, a posture task, serves)
    prob, layout = _compile(configuration, [PostureTask(configuration.model, cost=1.0)], None, 1, devices=configuration.devices[:1])
    with _pin(configuration, layout):
        out = prob.unwind_turns(rows, configuration.q_batch if reference is None else reference)
    return configuration._unbatch(out)


def distinct_solutions(configuration: Configuration, q_candidates, valid=None, n_solutions: int = 8, min_distance: float = 0.1,
                       reference=None, weights=None, unwind_turns: bool = False) -> DistinctSet:
    """The selection of solve_ik_solutions alone, over the caller's own candidates (closed-form IK branches, the q_all of an
    earlier call filtered again with another min_distance, the rungs of a ladder): q_candidates (S, nq) or (B, S, nq), `valid`
    (same leading shape; default: every candidate), `reference` (nq,) or (B, nq) (default: the configuration's q).  Up to
    `n_solutions` valid candidates no two of which lie within `min_distance` of each other, in ascending distance from the
    reference, ties to the lowest index — the rule of solve_ik_solutions.  With `unwind_turns` the candidates are moved to the
    turn nearest the reference first (the function unwind_turns) and `q` holds the moved rows.  The configuration is not
    changed."""
    from .tasks import PostureTask

    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    q_candidates = _host_array(q_candidates, "q_candidates")
    if q_candidates is None or q_candidates.ndim not in (2, 3) or q_candidates.shape[-1] != nq or q_candidates.shape[-2] < 1 \
            or (q_candidates.ndim == 3 and q_candidates.shape[0] != B):
        raise ValueError(f"q_candidates must have shape (S, {nq}) or ({B}, S, {nq}), got "
                         f"{None if q_candidates is None else q_candidates.shape}")
    S = q_candidates.shape[-2]
    K, r = _set_args(n_solutions, min_distance, S)
    q_candidates = np.ascontiguousarray(np.broadcast_to(q_candidates, (B, S, nq)))
    valid = _host_flags(valid, "valid", (S,), B)
    reference = _optional_array(reference, "reference", (nq,), B)
    weights = _optional_array(weights, "weights", (nv,))
    # (the selection reads the model's joint table through a problem handle: the smallest one, a posture task, serves)
    prob, layout = _compile(configuration, [PostureTask(configuration.model, cost=1.0)], None, 1, devices=configuration.devices[:1])
    ref = configuration.q_batch if reference is None else reference
    with _pin(configuration, layout):
        if unwind_turns:                 # (the two device calls composed: the candidates moved to the turn nearest `ref` first)
            q_candidates = prob.unwind_turns(q_candidates, ref)
        out = prob.select_distinct(q_candidates, valid, ref, weights, n_solutions=K, min_distance=r)
    return _present(configuration, DistinctSet, out, valid=out.seed_index >= 0)


class GoalSetResult(NamedTuple):
    """Result of solve_ik_goalset.  Per target: the chosen (goal, seed)'s final configuration `q`, its last velocity `v`,
    whether any goal was reached (`converged`), the chosen `goal_index` (nothing reached: the lowest valid goal, −1 when no goal
    is valid) and `seed_index` (0), `n_reached` goals, the chosen goal's `score` = goal_cost + distance (+inf), and the chosen
    loop's `iters` and `status`.  Per goal, (B, G, ·): `q_goal`, `v_goal` of the goal's closest converged seed (seed 0's when
    the goal is not reached), `reached`, `seed_index_goal`, `n_converged_goal` of its S seeds, `distance_goal` (+inf),
    `iters_goal`, `status_goal`.  With return_all also every loop's `q_all` (B, G, S, nq), `converged_all`, `iters_all`,
    `status_all` (B, G, S) and the `seeds` (B, G, S, nq) the loops started from; None otherwise.  Without the leading axis for an
    unbatched configuration."""
    q: np.ndarray
    v: np.ndarray
    converged: np.ndarray
    goal_index: np.ndarray
    seed_index: np.ndarray
    n_reached: np.ndarray
    score: np.ndarray
    iters: np.ndarray
    status: np.ndarray
    q_goal: np.ndarray
    v_goal: np.ndarray
    reached: np.ndarray
    seed_index_goal: np.ndarray
    n_converged_goal: np.ndarray
    distance_goal: np.ndarray
    iters_goal: np.ndarray
    status_goal: np.ndarray
    q_all: Optional[np.ndarray] = None
    converged_all: Optional[np.ndarray] = None
    iters_all: Optional[np.ndarray] = None
    status_all: Optional[np.ndarray] = None
    seeds: Optional[np.ndarray] = None


class GoalChoice(NamedTuple):
    """Result of best_goal: `q` (B, nq), `converged`, `goal_index`, `seed_index`, `n_reached`, `score` (B,), and per goal `q_goal`
    (B, G, nq), `reached`, `seed_index_goal`, `n_valid_goal`, `distance_goal` (B, G) — without the leading axis for an unbatched
    configuration."""
    q: np.ndarray
    converged: np.ndarray
    goal_index: np.ndarray
    seed_index: np.ndarray
    n_reached: np.ndarray
    score: np.ndarray
    q_goal: np.ndarray
    reached: np.ndarray
    seed_index_goal: np.ndarray
    n_valid_goal: np.ndarray
    distance_goal: np.ndarray


def _goal_arrays(goal_cost, goal_valid, B: int, G: int):
    """goal_cost as float64 (B, G) and goal_valid as bool (B, G) on the host — each given as (G,) or (B, G) — or None."""
    goal_cost = _host_array(goal_cost, "goal_cost")
    if goal_cost is not None:
        if goal_cost.shape not in ((G,), (B, G)):
            raise ValueError(f"goal_cost must have shape {(G,)} or {(B, G)}, got {goal_cost.shape}")
        if not (np.isfinite(goal_cost) & (goal_cost >= 0.0)).all():
            raise ValueError("goal_cost must be finite and >= 0")
        goal_cost = np.ascontiguousarray(np.broadcast_to(goal_cost, (B, G)))
    return goal_cost, _host_flags(goal_valid, "goal_valid", (G,), B)


def solve_ik_goalset(configuration: Configuration, tasks: Sequence, dt: float, goals, n_seeds: int, max_iters: int,
                     pos_threshold: float, ori_threshold: float, goal_cost=None, goal_valid=None, reference=None, weights=None,
                     seeds=None, seed_table: Optional["SeedTable"] = None, rng_seed: int = 0, return_all: bool = False,
                     update: bool = True, max_instances: int = 1 << 20, damping: float = 1e-12,
                     limits: Optional[Sequence] = None, safety_break: bool = False, solver: str = "mi355x",
                     collision_check: Optional["CollisionChecker"] = None) -> GoalSetResult:
    """Global IK to the best of G candidate poses per target — the grasp poses of an object, the poses a placement accepts,
    the yaws of a symmetric tool: which of them the robot reaches, and the configuration of the one closest to the current
    posture, in one call, picked on the device.

    `goals` is the trajectory calls' mapping {task: (G, w) or (B, G, w)} with the goals where those have their waypoints; at
    least one FrameTask is needed.  Every goal of instance b is solved by solve_ik_multistart's loops from the configuration's
    own q[b]: `n_seeds` starts, seed 0 q[b] itself, the others drawn by the stateless generator at target index b·G + g, taken
    from `seeds` — (S, nq), (G, S, nq) or (B, G, S, nq) — or from `seed_table`, queried with every goal's own frame targets.

    Per goal, the converged seed closest to `reference` (default: q) wins, as in solve_ik_multistart (`weights`, ties to the
    lowest seed); a goal with such a seed, and not masked out by `goal_valid` — (G,) or (B, G) — is reached.  Per target, the
    reached goal with the smallest `goal_cost` + distance wins (`goal_cost` (G,) or (B, G), finite and >= 0; ties to the lowest
    goal).  Where nothing is reached the row is seed 0's of the lowest valid goal — what solve_ik_steps returns from q towards
    it — with converged = False.  Masked goals still run their loops: pad a ragged set by repeating a valid goal (the rule in
    full: include/minkhip.h "THE RULE OF THE GOAL SET").

    `collision_check` (a CollisionChecker): as in solve_ik_multistart — a seed whose final q is in collision gets
    ST_IN_COLLISION and is not eligible, so a goal whose seeds all collide is not reached; `n_converged_goal` and `n_reached`
    count the free ones.  With a checker the call is no longer "never worse than solve_ik_steps from q" towards a goal.

    Limits warnings and SolverError follow solve_ik_trajectory_ladder's rules on the CHOSEN rows only (`safety_break` as there).
    With `update` the configuration is left at the chosen q.  The instances are walked in chunks of as many as keep
    chunk·G·n_seeds within `max_instances`; a multi-device configuration shards by instance; the result depends on neither."""
    del solver
    S, max_iters = _loop_scalars(max_instances, n_seeds, length=max_iters, thresholds=(pos_threshold, ori_threshold),
                                 whose="a goal set's loops")
    _refuse_plugin_rows({"dense": [t for t in tasks if t._is_dense()], "dense_limits": [x for x in (limits or ()) if x._is_dense()]},
                        "solve_ik_goalset")
    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    seqs, G = _trajectory_targets(configuration, tasks, goals, axis="goals G")
    _need_frame_task(tasks, "a goal set")
    nat.check_goalset_shape(1, G, S)
    if G * S > int(max_instances):
        raise ValueError(f"one instance's goal set has G*n_seeds = {G * S} loops, beyond max_instances = {int(max_instances)}")
    goal_cost, goal_valid = _goal_arrays(goal_cost, goal_valid, B, G)
    seeds = _host_array(seeds, "seeds")
    if seeds is not None:
        if seeds.shape not in ((S, nq), (G, S, nq), (B, G, S, nq)):
            raise ValueError(f"seeds must have shape {(S, nq)}, {(G, S, nq)} or {(B, G, S, nq)}, got {seeds.shape}")
        seeds = np.ascontiguousarray(np.broadcast_to(seeds, (B, G, S, nq)))
    reference = _optional_array(reference, "reference", (nq,), B)
    weights = _optional_array(weights, "weights", (nv,))
    _check_seed_table(seed_table, seeds, configuration, S)
    _check_collision_check(collision_check, configuration)
    handles, layout, chunk, n_dev = _compile_outer(configuration, tasks, limits, dt, "solve_ik_goalset", G * S, max_instances)
    ft, pt, ct = _stacked_targets(configuration, layout, seqs, G)
    pt, ct = _held_over((pt, ct), B, G)
    q = configuration.q_batch
    kw = dict(n_seeds=S, max_iters=max_iters, pos_threshold=float(pos_threshold), ori_threshold=float(ori_threshold),
              rng_seed=int(rng_seed), weights=weights, return_all=bool(return_all))

    def job(handle, lo, hi):
        return handle.solve_goalset(q[lo:hi], _rows(ft, 0, lo, hi), _rows(pt, 2, lo, hi), _rows(ct, 2, lo, hi), dt, damping,
                                    target_index0=lo, seeds=_rows(seeds, 0, lo, hi), reference=_rows(reference, 0, lo, hi),
                                    goal_cost=_rows(goal_cost, 0, lo, hi), goal_valid=_rows(goal_valid, 0, lo, hi),
                                    seed_table=seed_table, collision_check=collision_check, **kw)

    res = _join(nat.GoalSetOut, _chunks_and_shards(configuration, layout, handles, B, chunk, n_dev, job))
    chosen = lambda b: f"the chosen loop of instance {b} (goal {int(res.goal_index[b])}, seed {int(res.seed_index[b])})"
    _status_epilogue(res.status, "solve_ik_goalset", "chosen instance(s)",
                     "QP failed for the chosen loop of {n} of {of} targets (first: index {first}, status {status}); "
                     "none of their goals was reached", safety_break=chosen if safety_break else None)
    if update:
        configuration.update(res.q if configuration.batched else res.q[0])
    return _present(configuration, GoalSetResult, res, flags=("converged", "reached", "converged_all"))


def best_goal(configuration: Configuration, q_candidates, valid=None, goal_cost=None, goal_valid=None, reference=None,
              weights=None) -> GoalChoice:
    """The selection of solve_ik_goalset alone, over the caller's own candidates — the closed-form IK branches of every grasp
    pose: q_candidates (G, S, nq) or (B, G, S, nq), `valid` (same leading shape; default: every candidate), `goal_cost` and
    `goal_valid` (G,) or (B, G), `reference` (nq,) or (B, nq) (default: the configuration's q).  Per goal the valid candidate
    closest to the reference, per target the reached goal with the smallest goal_cost + distance, ties to the lowest index —
    the rule of solve_ik_goalset.  The configuration is not changed."""
    from .tasks import PostureTask

    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    q_candidates = _host_array(q_candidates, "q_candidates")
    if q_candidates is None or q_candidates.ndim not in (3, 4) or q_candidates.shape[-1] != nq or q_candidates.shape[-2] < 1 \
            or q_candidates.shape[-3] < 1 or (q_candidates.ndim == 4 and q_candidates.shape[0] != B):
        raise ValueError(f"q_candidates must have shape (G, S, {nq}) or ({B}, G, S, {nq}), got "
                         f"{None if q_candidates is None else q_candidates.shape}")
    G, S = q_candidates.shape[-3], q_candidates.shape[-2]
    nat.check_goalset_shape(B, G, S)
    q_candidates = np.ascontiguousarray(np.broadcast_to(q_candidates, (B, G, S, nq)))
    valid = _host_flags(valid, "valid", (G, S), B)
    goal_cost, goal_valid = _goal_arrays(goal_cost, goal_valid, B, G)
    reference = _optional_array(reference, "reference", (nq,), B)
    weights = _optional_array(weights, "weights", (nv,))
    # (the selection reads the model's joint table through a problem handle: the smallest one, a posture task, serves)
    prob, layout = _compile(configuration, [PostureTask(configuration.model, cost=1.0)], None, 1, devices=configuration.devices[:1])
    with _pin(configuration, layout):
        out = prob.select_goalset(q_candidates, valid, configuration.q_batch if reference is None else reference, weights,
                                  goal_cost=goal_cost, goal_valid=goal_valid)
    return _present(configuration, GoalChoice, out, flags=("converged", "reached"))


class TrajectoryResult(NamedTuple):
    """Result of solve_ik_trajectory, (B, T, ·) — (T, ·) for an unbatched configuration: the configuration `q` at the end of
    every waypoint's loop, the loop's last velocity `v`, its `status` bits, and in threshold mode its `iters` and `converged`
    (None with a fixed step count); `qvel` = (q_t ⊖ q_{t−1}) / waypoint_dt when waypoint_dt was given, else None."""
    q: np.ndarray
    v: np.ndarray
    status: np.ndarray
    iters: Optional[np.ndarray] = None
    converged: Optional[np.ndarray] = None
    qvel: Optional[np.ndarray] = None


def _trajectory_targets(configuration: Configuration, tasks: Sequence, targets, axis: str = "waypoints T"):
    """{id(task): (B, T, w) array} and T from the caller's mapping — shapes checked, nothing touched on a device.  (`axis`
    names the sequences' axis in messages: the keyframed call's sequences have K keyframes there.)"""
    from .tasks import ComTask, FrameTask, PostureTask

    items = list(targets.items()) if hasattr(targets, "items") else list(targets or ())
    if not items:
        raise ValueError("targets is empty: at least one task needs a (T, ...) sequence of targets")
    B, T, out = configuration.batch_size, None, {}
    for task, arr in items:
        if not any(task is t for t in tasks):
            raise ValueError(f"targets names a {type(task).__name__} that is not in `tasks`")
        if isinstance(task, FrameTask):                      # (RelativeFrameTask included)
            w, what = 7, "wxyz_xyz poses"
        elif isinstance(task, PostureTask):
            w, what = configuration.nq, "postures"
        elif isinstance(task, ComTask):
            w, what = 3, "CoM positions"
        else:
            raise ValueError(f"targets: a {type(task).__name__} takes no target sequence (FrameTask, RelativeFrameTask, "
                             "PostureTask and ComTask do)")
        arr = _host_array(getattr(arr, "wxyz_xyz", arr), f"targets[{type(task).__name__}]")
        if arr.ndim == 2 and arr.shape[1] == w and arr.shape[0] >= 1:
            arr = np.broadcast_to(arr, (B,) + arr.shape)
        elif not (arr.ndim == 3 and arr.shape[0] == B and arr.shape[2] == w and arr.shape[1] >= 1):
            raise ValueError(f"targets[{type(task).__name__}] must have shape (T, {w}) or ({B}, T, {w}) ({what}), got {arr.shape}")
        if T is not None and arr.shape[1] != T:
            raise ValueError(f"targets disagree on the number of {axis}: {T} and {arr.shape[1]}")
        T = arr.shape[1]
        out[id(task)] = arr
    return out, T


def _stacked_targets(configuration: Configuration, layout, seqs, L: int):
    """(frame, posture, CoM) target arrays of a trajectory call from the sequences of _trajectory_targets: a group is per
    waypoint — (B, L, n, w) — when any of its tasks has a sequence (frame targets: always), else as solve_ik_steps passes it."""
    B = configuration.batch_size

    def stack(group, w, timed=False):
        if not group:
            return None
        held = [np.asarray(t._native_target(configuration)) if id(t) not in seqs else None for t in group]
        if not timed and not any(id(t) in seqs for t in group):
            if all(h.ndim == 1 for h in held):
                return np.stack(held, axis=0)
            return np.stack([np.broadcast_to(h, (B, w)) for h in held], axis=1)
        rows = [seqs[id(t)] if h is None else np.broadcast_to(np.broadcast_to(h, (B, w))[:, None, :], (B, L, w))
                for t, h in zip(group, held)]
        return np.ascontiguousarray(np.stack(rows, axis=2))

    return stack(layout["frame"], 7, timed=True), stack(layout["posture"], configuration.nq), stack(layout["com"], 3)


def solve_ik_trajectory(configuration: Configuration, tasks: Sequence, dt: float, targets, n_steps: int = 1,
                        solver: str = "mi355x", damping: float = 1e-12, limits: Optional[Sequence] = None,
                        pos_threshold: Optional[float] = None, ori_threshold: Optional[float] = None,
                        waypoint_dt: Optional[float] = None, warm_start: bool = False, update: bool = True,
                        max_instances: int = 1 << 20, keyframe_times=None, waypoint_times=None,
                        return_targets: bool = False):
    """Follow a time sequence of targets: every instance has T waypoints, waypoint t is solved by the fused loop of
    solve_ik_steps from where waypoint t − 1 ended — in one call, nothing crossing the bus between waypoints.

    `targets` maps task objects of `tasks` to their sequences: FrameTask / RelativeFrameTask (T, 7) or (B, T, 7) wxyz_xyz,
    PostureTask (T, nq) or (B, T, nq), ComTask (T, 3) or (B, T, 3).  A task absent from the mapping keeps its set_target value
    for the whole trajectory.  `n_steps` is the loop length per waypoint (1: tracking mode, one differential step per frame);
    with `pos_threshold` / `ori_threshold` it is max_iters of the threshold-terminated loop and the result carries `iters` and
    `converged` per waypoint.  `waypoint_dt`: also return the joint velocity between consecutive waypoints.

    Keyframes.  With `keyframe_times` (K strictly increasing times) the sequences of `targets` are K sparse KEYFRAMES, and
    the T = len(waypoint_times) waypoint targets are interpolated from them on the device: only the keyframes cross the bus.
    `waypoint_times` (required then) are non-decreasing and lie inside [keyframe_times[0], keyframe_times[-1]] — there is no
    extrapolation and no clamping.  A waypoint at a keyframe's time IS that keyframe, bit for bit; in between, with
    u = (τ − t_k) / (t_{k+1} − t_k): frame targets blend rotation and translation apart — the shortest arc
    q_a·exp(u·log(q_a⁻¹·q_b)) and p_a + u·(p_b − p_a), not the SE3 screw; postures q_a ⊕ u·(q_b ⊖ q_a) per joint type
    (mj_differentiatePos / mj_integratePos); CoM targets a + u·(b − a) (the rule in full: include/minkhip.h).  Both time
    arrays are shared by the batch; `waypoint_dt` stays one uniform step.  `return_targets=True` returns
    (TrajectoryResult, {task: (B, T, w) array}) — the interpolated path of every task of `targets`, as the loops read it.
    Without `keyframe_times`, `waypoint_times` or `return_targets` raise ValueError.

    A waypoint that does not converge does NOT stop its trajectory: the next one starts from where the loop ended, and
    `converged[b, t]` says what happened.  Limits warnings and SolverError follow solve_ik_steps' rules on the OR of the
    statuses over the trajectory (the error names the first (instance, waypoint)).  With `update` the configuration is left
    at q[:, -1].  When B exceeds `max_instances` the trajectories are walked in chunks of instances; a multi-device
    configuration shards by trajectory."""
    del solver
    _, n_steps = _loop_scalars(max_instances, loop="n_steps", length=n_steps, step=waypoint_dt)
    kt = wt = None
    if keyframe_times is None:
        if waypoint_times is not None or return_targets:
            raise ValueError("waypoint_times and return_targets belong to the keyframed call: they need keyframe_times")
        seqs, L = _trajectory_targets(configuration, tasks, targets)      # L: the length of the sequences' axis
    else:
        if waypoint_times is None:
            raise ValueError("keyframe_times needs waypoint_times: the times at which the keyframes are sampled")
        kt, wt = nat.check_keyframe_times(_host_array(keyframe_times, "keyframe_times"), _host_array(waypoint_times, "waypoint_times"))
        seqs, L = _trajectory_targets(configuration, tasks, targets, axis="keyframes K")
        if L != len(kt):
            raise ValueError(f"targets have {L} keyframes, keyframe_times has {len(kt)}")
    until = _thresholds(pos_threshold, ori_threshold)
    if until is not None and (until[0] < 0.0 or until[1] < 0.0):
        raise ValueError("thresholds must be >= 0")
    B = configuration.batch_size
    handles, layout, chunk, n_dev = _compile_outer(configuration, tasks, limits, dt, "solve_ik_trajectory", 1, max_instances)
    ft, pt, ct = _stacked_targets(configuration, layout, seqs, L)
    q = configuration.q_batch

    def job(handle, lo, hi):
        args = (_rows(ft, 0, lo, hi), _rows(pt, 2, lo, hi), _rows(ct, 2, lo, hi), dt, damping)
        kw = dict(n_steps=n_steps, until=until, qvel_dt=waypoint_dt, warm_start=bool(warm_start))
        if kt is None:
            return handle.solve_trajectory(q[lo:hi], *args, **kw)
        return handle.solve_keyframes(q[lo:hi], kt, wt, *args, return_targets=bool(return_targets), **kw)

    parts = _chunks_and_shards(configuration, layout, handles, B, chunk, n_dev, job)
    paths = None
    if kt is not None:                                         # (parts: KeyframesOut — the trajectory and the interpolated targets)
        if return_targets:
            paths = [None if parts[0][k] is None else np.concatenate([p[k] for p in parts], axis=0) for k in (1, 2, 3)]
        parts = [p.trajectory for p in parts]
    res = _join(TrajectoryResult, parts)
    _status_epilogue(res.status, "solve_ik_trajectory", "instance(s)",
                     "QP failed at {n} of {of} waypoints (first: (instance, waypoint) = {first}, status {status})")
    if update:
        configuration.update(res.q[:, -1] if configuration.batched else res.q[0, -1])
    un = configuration._unbatch
    res = _present(configuration, TrajectoryResult, res, flags=("converged",))
    if paths is None:
        return res
    # the interpolated path of every task of `targets`: its column of its group's (B, T, n, w) array
    by_task = {}
    for group, arr in zip((layout["frame"], layout["posture"], layout["com"]), paths):
        for n, t in enumerate(group):
            if id(t) in seqs:
                by_task[t] = un(np.ascontiguousarray(arr[:, :, n]))
    return res, by_task


class TrajectoryMultistartResult(NamedTuple):
    """Result of solve_ik_trajectory_multistart.  The chosen candidate's trajectory, (B, T, ·) — (T, ·) for an unbatched
    configuration —: `q`, `v`, `status`, `iters`, `converged` as in TrajectoryResult; per instance the chosen `seed_index`, the
    number `n_tracked` of waypoints it tracked, `n_complete` of the S candidates that tracked all T, and its `path_length`;
    `qvel` when waypoint_dt was given.  With return_all every candidate's `q_all` (B, S, T, nq), `v_all` (B, S, T, nv),
    `status_all`, `iters_all`, `converged_all` (B, S, T) and the `seeds` (B, S, nq) they started from; None otherwise."""
    q: np.ndarray
    v: np.ndarray
    status: np.ndarray
    iters: np.ndarray
    converged: np.ndarray
    seed_index: np.ndarray
    n_tracked: np.ndarray
    n_complete: np.ndarray
    path_length: np.ndarray
    qvel: Optional[np.ndarray] = None
    q_all: Optional[np.ndarray] = None
    v_all: Optional[np.ndarray] = None
    status_all: Optional[np.ndarray] = None
    iters_all: Optional[np.ndarray] = None
    converged_all: Optional[np.ndarray] = None
    seeds: Optional[np.ndarray] = None


_FREE_PATH_FIELDS = ("node_margin", "edge_margin", "edge_collision", "n_edge_collisions", "tracked", "node_margin_all",
                     "edge_margin_all")
FreeTrajectoryMultistartResult = nat._extended(
    "FreeTrajectoryMultistartResult", TrajectoryMultistartResult, _FREE_PATH_FIELDS,
    """Result of solve_ik_trajectory_multistart(collision_check=...): TrajectoryMultistartResult's fields in its order — `n_tracked`
    and `n_complete` count the waypoints that are tracked, free of collision and entered by a free motion; `status` and
    `status_all` carry ST_IN_COLLISION where a row collides —, then of the chosen candidate `node_margin` and `edge_margin` (B, T)
    (entry 0 of edge_margin +inf, NaN where the motion was not swept), `edge_collision` (B, T) bool, `n_edge_collisions` (B,)
    and `tracked` (B, T) bool, the waypoints that counted: what refine_path(tracked=...) takes.  With return_all every
    candidate's `node_margin_all` and `edge_margin_all` (B, S, T); None otherwise.""", module=__name__)


def _counted(eligible: np.ndarray, edge_margin: np.ndarray) -> np.ndarray:
    """The waypoints of a chosen candidate that counted (include/minkhip.h "THE RULE, with a checker", Score), from its (B, T)
    outputs: eligible, and — behind waypoint 0 — entered by a motion whose swept margin is >= 0."""
    free_edge = np.zeros(edge_margin.shape, dtype=bool)
    np.greater_equal(edge_margin, 0.0, out=free_edge, where=~np.isnan(edge_margin))
    free_edge[:, 0] = True
    return eligible & free_edge


def solve_ik_trajectory_multistart(configuration: Configuration, tasks: Sequence, dt: float, targets, n_seeds: int, n_steps: int,
                                   pos_threshold: float, ori_threshold: float, solver: str = "mi355x", damping: float = 1e-12,
                                   limits: Optional[Sequence] = None, rng_seed: int = 0, seeds=None, weights=None,
                                   waypoint_dt: Optional[float] = None, warm_start: bool = False, update: bool = True,
                                   return_all: bool = False, max_instances: int = 1 << 20,
                                   seed_table: Optional["SeedTable"] = None,
                                   collision_check: Optional["CollisionChecker"] = None,
                                   edge_samples: int = 8) -> TrajectoryMultistartResult:
    """Track a time sequence of targets globally: `n_seeds` candidate trajectories per instance, seeded like
    solve_ik_multistart and each tracked like solve_ik_trajectory (waypoint t from the same candidate's waypoint t − 1, so a
    candidate is continuous by construction), scored over the whole path, one chosen and gathered on the device — in one call.

    `targets` as in solve_ik_trajectory (no keyframes here).  `n_steps` is max_iters of the threshold-terminated loop of every
    waypoint; both thresholds are required (there is nothing to score after a fixed count).  Candidate 0 starts at the
    configuration's own q: it is solve_ik_trajectory's trajectory; the others start as solve_ik_multistart's seeds do (same
    stateless generator, same `seeds` argument).

    A waypoint is tracked when its loop converged without a QP failure.  Per instance the candidate that tracked the most
    waypoints wins; among those the shortest path Σ_t Σ_k weights_k·(q_t ⊖ q_{t−1})_k², q_{−1} = the configuration's q for every
    candidate (the jump to a far seed counts); ties go to the lowest index; when nobody tracked anything, candidate 0.  Limits
    warnings and SolverError follow solve_ik_trajectory's rules on the CHOSEN candidate only.  With `update` the configuration
    is left at the chosen q[:, -1].  When B·n_seeds exceeds `max_instances` the instances are walked in chunks; a multi-device
    configuration shards by instance; the result depends on neither.

    `seed_table` (a SeedTable; not together with `seeds`): candidates 1 … n_seeds − 1 start at the table's entries nearest to
    waypoint 0's frame targets, as in solve_ik_multistart.

    `collision_check` (a CollisionChecker of the same model): the candidate whose waypoints and motions are free of collision.
    The loops are the same, bit for bit; behind them every row of every candidate is checked on the device (a row in collision
    gets ST_IN_COLLISION and does not count), the motion into every row that still counts is swept from the same candidate's
    previous row with `edge_samples` interior samples (CollisionChecker.swept_clearance's rule; the first motion, from the
    configuration's q, is never swept), and a waypoint entered by a colliding motion does not count either.  Count, length and
    ties then decide as above.  The result is a FreeTrajectoryMultistartResult.  A checker with general convex pairs
    (cylinder-box, ellipsoids, mesh hulls) needs its `check_rows` >= 1 + edge_samples: the rows are then judged in chunks of
    check_rows // (1 + edge_samples), and the result does not depend on the value.  Without collision_check the call is the
    one above, unchanged."""
    del solver
    _check_collision_check(collision_check, configuration, edge_samples)
    S, n_steps = _loop_scalars(max_instances, n_seeds, loop="n_steps", length=n_steps, step=waypoint_dt,
                               thresholds=(pos_threshold, ori_threshold), whose="multi-start trajectories")
    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    seqs, T = _trajectory_targets(configuration, tasks, targets)
    seeds = _optional_array(seeds, "seeds", (S, nq), B)
    weights = _optional_array(weights, "weights", (nv,))
    if weights is not None and not (weights >= 0.0).all():
        raise ValueError("weights must be >= 0 (no NaN): the path length is a sum of non-negative terms")
    _check_seed_table(seed_table, seeds, configuration, S)
    handles, layout, chunk, n_dev = _compile_outer(configuration, tasks, limits, dt, "solve_ik_trajectory_multistart", S,
                                                   max_instances)
    ft, pt, ct = _stacked_targets(configuration, layout, seqs, T)
    q = configuration.q_batch
    kw = dict(n_seeds=S, n_steps=n_steps, pos_threshold=float(pos_threshold), ori_threshold=float(ori_threshold),
              rng_seed=int(rng_seed), weights=weights, qvel_dt=waypoint_dt, warm_start=bool(warm_start), return_all=bool(return_all))

    def job(handle, lo, hi):
        args = (q[lo:hi], _rows(ft, 0, lo, hi), _rows(pt, 2, lo, hi), _rows(ct, 2, lo, hi), dt, damping)
        more = None
        if collision_check is None:
            out = handle.solve_trajectory_multistart(*args, target_index0=lo, seeds=_rows(seeds, 0, lo, hi), seed_table=seed_table,
                                                     **kw)
        else:
            out, more = handle.solve_trajectory_multistart_free(*args, checker=collision_check, edge_samples=int(edge_samples),
                                                                target_index0=lo, seeds=_rows(seeds, 0, lo, hi),
                                                                seed_table=seed_table, **kw)
        # every candidate's results, time-major (T, n·S, ·) → (n, S, T, ·), so that chunks and shards concatenate by instance
        n = hi - lo
        by_inst = lambda x: np.ascontiguousarray(np.moveaxis(x.reshape((T, n, S) + x.shape[2:]), 0, 2))
        if return_all:
            out = out._replace(q_all=by_inst(out.q_all), v_all=by_inst(out.v_all), status_all=by_inst(out.status_all),
                               iters_all=by_inst(out.iters_all), converged_all=by_inst(out.converged_all),
                               seeds=out.seeds.reshape(n, S, nq))
        if more is None:
            return out
        if return_all:
            more = more._replace(node_margin_all=by_inst(more.node_margin_all), edge_margin_all=by_inst(more.edge_margin_all))
        return out, more

    parts = _chunks_and_shards(configuration, layout, handles, B, chunk, n_dev, job)
    flags = ("converged", "converged_all")
    if collision_check is None:
        res = _join(nat.TrajectoryMultistartOut, parts)
    else:
        res, more = _join((nat.TrajectoryMultistartOut, nat.TrajectoryFreeOut), parts)
    _status_epilogue(res.status, "solve_ik_trajectory_multistart", "chosen trajectorie(s)",
                     "QP failed at {n} of {of} waypoints of the chosen candidates (first: (instance, waypoint) = {first}, "
                     "status {status})")
    if update:
        configuration.update(res.q[:, -1] if configuration.batched else res.q[0, -1])
    if collision_check is None:
        return _present(configuration, TrajectoryMultistartResult, res, flags)
    counted = _counted((res.converged != 0) & ((res.status & ~nat.ST_OUTSIDE_LIMITS) == 0), more.edge_margin)
    return _present(configuration, FreeTrajectoryMultistartResult, (res, more), flags + ("edge_collision",), tracked=counted)


class CandidatePath(NamedTuple):
    """Result of candidate_path: per instance the chosen `seed_index`, its path `q` (B, T, nq) — (T, nq) for an unbatched
    configuration —, the `n_tracked` waypoints it tracked, `n_complete` of the S candidates and its `path_length`."""
    seed_index: np.ndarray
    q: np.ndarray
    n_tracked: np.ndarray
    n_complete: np.ndarray
    path_length: np.ndarray


FreeCandidatePath = nat._extended(
    "FreeCandidatePath", CandidatePath, _FREE_PATH_FIELDS,
    """Result of candidate_path(collision_check=...): CandidatePath's fields, then of the chosen candidate `node_margin` and
    `edge_margin` (B, T), `edge_collision` (B, T) bool, `n_edge_collisions` (B,), `tracked` (B, T) bool — the waypoints that
    counted — and every candidate's `node_margin_all` and `edge_margin_all` (B, S, T).""", optional=False, module=__name__)


def candidate_path(configuration: Configuration, q_paths, tracked=None, weights=None,
                   collision_check: Optional["CollisionChecker"] = None, edge_samples: int = 8) -> CandidatePath:
    """The selection of solve_ik_trajectory_multistart alone, over the caller's own candidate paths: q_paths (S, T, nq) or
    (B, S, T, nq), `tracked` (same leading shape, default: every waypoint counts as tracked), the first motion from the
    configuration's q.  The rule — most tracked waypoints, then the shortest path Σ_t Σ_k weights_k·(q_t ⊖ q_{t−1})_k², then the
    lowest index; nobody tracked anything: candidate 0 — is that call's; the configuration is not changed.

    `collision_check` (a CollisionChecker of the same model): every row is checked on the device and a row in collision does
    not count; the motion into every row that still counts is swept from the same candidate's previous row with `edge_samples`
    interior samples, and a waypoint entered by a colliding motion does not count.  The result is then a FreeCandidatePath.
    A checker with general convex pairs (cylinder-box, ellipsoids, mesh hulls) needs its `check_rows` >= 1 + edge_samples; the
    rows are then judged in chunks of check_rows // (1 + edge_samples), and the result does not depend on the value."""
    from .tasks import PostureTask

    _check_collision_check(collision_check, configuration, edge_samples)
    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    q_paths = _host_array(q_paths, "q_paths")
    if q_paths is None or q_paths.ndim not in (3, 4) or q_paths.shape[-1] != nq or (q_paths.ndim == 4 and q_paths.shape[0] != B):
        raise ValueError(f"q_paths must have shape (S, T, {nq}) or ({B}, S, T, {nq}), got {None if q_paths is None else q_paths.shape}")
    S, T = q_paths.shape[-3], q_paths.shape[-2]
    if S < 1 or T < 1:
        raise ValueError(f"q_paths needs at least one candidate and one waypoint, got S = {S}, T = {T}")
    # (B, S, T, ·) → the loops' time-major (T, B·S, ·)
    q_tm = np.ascontiguousarray(np.moveaxis(np.broadcast_to(q_paths, (B, S, T, nq)), 2, 0)).reshape(T, B * S, nq)
    tracked = _host_flags(tracked, "tracked", (S, T), B)
    trk_tm = None if tracked is None else np.ascontiguousarray(np.moveaxis(tracked, 2, 0)).reshape(T, B * S)
    weights = _optional_array(weights, "weights", (nv,))
    if weights is not None and not (weights >= 0.0).all():
        raise ValueError("weights must be >= 0 (no NaN): the path length is a sum of non-negative terms")
    # (the selection reads the model's joint table through a problem handle: the smallest one, a posture task, serves)
    prob, layout = _compile(configuration, [PostureTask(configuration.model, cost=1.0)], None, 1, devices=configuration.devices[:1])
    with _pin(configuration, layout):
        out, more = prob.select_trajectory_candidates(configuration.q_batch, q_tm, trk_tm, weights, collision_check,
                                                      int(edge_samples), collision_check is not None)
    if collision_check is None:
        return _present(configuration, CandidatePath, out)
    by_inst = lambda x: np.ascontiguousarray(np.moveaxis(x.reshape(T, B, S), 0, 2))
    given = np.ones((B, S, T), dtype=bool) if tracked is None else tracked
    chosen = given[np.arange(B), out.seed_index]                         # (B, T): the caller's flags of the chosen candidate
    counted = _counted(chosen & (more.node_margin >= 0.0), more.edge_margin)
    return _present(configuration, FreeCandidatePath, (out, more), flags=("edge_collision",), tracked=counted,
                    node_margin_all=by_inst(more.node_margin_all), edge_margin_all=by_inst(more.edge_margin_all))


class LadderResult(NamedTuple):
    """Result of solve_ik_trajectory_ladder.  The chosen path, (B, T, ·) — (T, ·) for an unbatched configuration —: `q`, `v`,
    `status`, `iters`, `converged` of the chosen node of every waypoint; `node_index` (B, T) its index in the rung and
    `edge_break` (B, T) whether the step into the waypoint exceeds max_step (entry 0: never); per instance `n_tracked` (waypoints
    whose chosen node converged without a QP failure), `n_breaks` and `path_length`; `qvel` when waypoint_dt was given.  With
    return_all every node's `q_all` (B, T, S, nq), `v_all` (B, T, S, nv), `status_all`, `iters_all`, `converged_all` (B, T, S)
    and the `seeds` (B, T, S, nq) the loops started from; None otherwise."""
    q: np.ndarray
    v: np.ndarray
    status: np.ndarray
    iters: np.ndarray
    converged: np.ndarray
    node_index: np.ndarray
    n_tracked: np.ndarray
    n_breaks: np.ndarray
    path_length: np.ndarray
    edge_break: np.ndarray
    qvel: Optional[np.ndarray] = None
    q_all: Optional[np.ndarray] = None
    v_all: Optional[np.ndarray] = None
    status_all: Optional[np.ndarray] = None
    iters_all: Optional[np.ndarray] = None
    converged_all: Optional[np.ndarray] = None
    seeds: Optional[np.ndarray] = None


_REFINED_FIELDS = ("repaired", "refined")
_CHECKED_FIELDS = ("edge_collision", "n_edge_collisions", "edge_margin")
RefinedLadderResult = nat._extended(
    "RefinedLadderResult", LadderResult, _REFINED_FIELDS,
    """Result of solve_ik_trajectory_ladder(refine=True): LadderResult's fields, in its order, for the path the refinement pass
    returned, and behind them `repaired` (B, T) — 0 kept, 1 / 2 replaced by the forward / backward sweep — and `refined` (B,):
    where the path differs from the search's.  `node_index` names the replaced node at a repaired waypoint.""", module=__name__)
LadderNodesResult = nat._extended(
    "LadderNodesResult", LadderResult, nat.LADDER_NODES_IO_FIELDS,
    """Result of solve_ik_trajectory_ladder(n_nodes=K): LadderResult's fields, in its order, for the ladder searched on the K
    deduplicated nodes of every rung — `node_index` is a slot in 0 … K − 1, and with return_all the *_all fields are the NODES'
    rows, (B, T, K, ·), `seeds` the (B, T, S, nq) starts — and behind them what the selection says of every rung:
    `node_seed_index` (B, T, K) the candidate each node is (−1: an empty slot, which repeats candidate 0 and is not tracked),
    `node_multiplicity` the candidates it stands for, `node_distance` its distance from q; `n_distinct`, `n_converged`,
    `n_uncovered` (B, T) nodes filled, candidates tracked, tracked candidates that no node covers; `seed_index` (B, T) the
    chosen node's candidate index.""", module=__name__)
RefinedLadderNodesResult = nat._extended(
    "RefinedLadderNodesResult", RefinedLadderResult, nat.LADDER_NODES_IO_FIELDS,
    """Result of solve_ik_trajectory_ladder(n_nodes=K, refine=True): RefinedLadderResult's fields, in its order, and behind them
    LadderNodesResult's own.""", module=__name__)


class LadderPath(NamedTuple):
    """Result of ladder_path: the chosen `node_index` (B, T), the nodes along it `q` (B, T, nq), `edge_break` (B, T), and per
    instance `n_tracked`, `n_breaks`, `path_length` — without the leading axis for an unbatched configuration."""
    node_index: np.ndarray
    q: np.ndarray
    n_tracked: np.ndarray
    n_breaks: np.ndarray
    path_length: np.ndarray
    edge_break: np.ndarray


FreeLadderPath = nat._extended(
    "FreeLadderPath", LadderPath, nat.LADDER_FREE_IO_FIELDS,
    """Result of ladder_path(collision_check=...): LadderPath's fields, in its order, then `edge_collision` (B, T) — the motion
    into waypoint t passes through collision, entry 0 never —, `n_edge_collisions` (B,), `edge_margin` (B, T) — the swept margin
    of the chosen edges, +inf at waypoint 0, NaN where the edge was not swept —, `node_margin` (B, T, S) and `edge_margin_all`
    (B, T, S, S), entry [b, t, s', s].  `n_tracked` counts the waypoints that are tracked, free of collision and entered by a
    free motion.""", optional=False, module=__name__)
FreeLadderResult = nat._extended(
    "FreeLadderResult", LadderResult, _CHECKED_FIELDS,
    """Result of solve_ik_trajectory_ladder(collision_check=...): LadderResult's fields, in its order, and behind them
    `edge_collision` (B, T), `n_edge_collisions` (B,) and `edge_margin` (B, T) of the chosen path, as in FreeLadderPath.""",
    module=__name__)
FreeLadderNodesResult = nat._extended(
    "FreeLadderNodesResult", LadderNodesResult, _CHECKED_FIELDS,
    """Result of solve_ik_trajectory_ladder(collision_check=..., n_nodes=K): LadderNodesResult's fields, in its order, and behind
    them `edge_collision`, `n_edge_collisions`, `edge_margin`, as in FreeLadderPath.""", module=__name__)
FreeRefinedLadderResult = nat._extended(
    "FreeRefinedLadderResult", FreeLadderResult, _REFINED_FIELDS,
    """Result of solve_ik_trajectory_ladder(collision_check=..., refine="free"): FreeLadderResult's fields, in its order — all of
    the RETURNED path, `edge_collision`, `n_edge_collisions` and `edge_margin` included —, and behind them `repaired` (B, T) and
    `refined` (B,) of the checked refinement pass.""", module=__name__)
FreeRefinedLadderNodesResult = nat._extended(
    "FreeRefinedLadderNodesResult", FreeLadderNodesResult, _REFINED_FIELDS,
    """Result of solve_ik_trajectory_ladder(collision_check=..., n_nodes=K, refine="free"): FreeLadderNodesResult's fields, in its
    order, and behind them `repaired` and `refined`, as in FreeRefinedLadderResult.""", module=__name__)


_CERTIFIED_FIELDS = ("edge_verdict", "edge_lower_bound", "edge_n_samples", "n_certified")
CertifiedLadderPath = nat._extended(
    "CertifiedLadderPath", FreeLadderPath, nat.LADDER_CERTIFIED_IO_FIELDS,
    """Result of ladder_path(collision_check=..., edge_resolution=...): FreeLadderPath's fields, in its order — `edge_margin` and
    `edge_margin_all` are the certified sweep's margins, both ends of an edge included; `edge_collision` and `n_edge_collisions`
    say what the search counted as blocked, which with require_certified includes the undecided edges —, then of the chosen path
    `edge_verdict` (B, T) — 2 collides, 1 proven free along the whole motion, 0 undecided, −1 not swept (waypoint 0 included) —,
    `edge_lower_bound` (B, T) — +inf at waypoint 0, NaN where not swept —, `edge_n_samples` (B, T) — 0 where not swept —,
    `n_certified` (B,) and `edge_verdict_all` (B, T, S, S) int8, entry [b, t, s', s].""", optional=False, module=__name__)
CertifiedLadderResult = nat._extended(
    "CertifiedLadderResult", FreeLadderResult, _CERTIFIED_FIELDS,
    """Result of solve_ik_trajectory_ladder(collision_check=..., edge_resolution=...): FreeLadderResult's fields, in its order, and
    behind them `edge_verdict`, `edge_lower_bound`, `edge_n_samples` (B, T) and `n_certified` (B,) of the chosen path, as in
    CertifiedLadderPath.""", module=__name__)
CertifiedLadderNodesResult = nat._extended(
    "CertifiedLadderNodesResult", FreeLadderNodesResult, _CERTIFIED_FIELDS,
    """Result of solve_ik_trajectory_ladder(collision_check=..., n_nodes=K, edge_resolution=...): FreeLadderNodesResult's fields, in
    its order, and behind them `edge_verdict`, `edge_lower_bound`, `edge_n_samples`, `n_certified`, as in CertifiedLadderPath.""",
    module=__name__)


def _edge_rule(edge_resolution, max_edge_samples, require_certified, edge_samples, collision_check, refine):
    """The certified edge rule of the ladder calls, judged on the host: None without `edge_resolution`, else (resolution,
    max_samples, require_certified)."""
    if edge_resolution is None:
        if require_certified:
            raise ValueError("require_certified belongs to the certified edge rule: pass edge_resolution")
        return None
    if collision_check is None:
        raise ValueError("edge_resolution is the certified edge rule of a checked call: pass collision_check")
    if int(edge_samples) != 8:
        raise ValueError("edge_resolution and edge_samples are two rules for the same edges: the certified rule takes its sample "
                         "counts from the motion bound (max_edge_samples caps them)")
    if refine:
        raise ValueError("edge_resolution together with refine: the refinement pass still samples its edges — certifying it (and "
                         "candidate tracking) is the follow-up; refine the returned path with refine_path")
    nat.check_edge_rule(edge_resolution, max_edge_samples)
    return float(edge_resolution), int(max_edge_samples), bool(require_certified)


def _max_step_sq(max_step) -> float:
    """The squared gate of the ladder's break rule from the caller's joint-space step (None: no gate)."""
    if max_step is None:
        return float("inf")
    max_step = float(max_step)
    if not max_step >= 0.0:
        raise ValueError(f"max_step must be >= 0 (None: no gate), got {max_step}")
    return max_step * max_step


def _outside_limits(message: str) -> exceptions.NotWithinConfigurationLimits:
    """NotWithinConfigurationLimits for a status bit of a fused loop: the bit names no joint and no value (the exception's own
    constructor formats both), so the message is the caller's."""
    e = exceptions.NotWithinConfigurationLimits.__new__(exceptions.NotWithinConfigurationLimits)
    exceptions.MinkError.__init__(e, message)
    return e


def _need_frame_task(tasks, what: str) -> None:
    """The threshold-terminated loops test their thresholds on frame tasks: judged on the objects, before a handle exists."""
    from .tasks import FrameTask

    if not any(isinstance(t, FrameTask) for t in tasks):
        raise ValueError(f"{what} needs at least one frame task to test the thresholds on")


def _ladder_weights(weights, nv: int):
    weights = _optional_array(weights, "weights", (nv,))
    if weights is not None and not (weights >= 0.0).all():
        raise ValueError("weights must be >= 0 (no NaN): an edge cost is a sum of non-negative terms")
    return weights


def solve_ik_trajectory_ladder(configuration: Configuration, tasks: Sequence, dt: float, targets, n_seeds: int, max_iters: int,
                               pos_threshold: float, ori_threshold: float, max_step: Optional[float] = None, weights=None,
                               seeds=None, seed_table: Optional["SeedTable"] = None, rng_seed: int = 0,
                               qvel_dt: Optional[float] = None, return_all: bool = False, update: bool = True,
                               max_instances: int = 1 << 20, damping: float = 1e-12, limits: Optional[Sequence] = None,
                               safety_break: bool = False, solver: str = "mi355x", n_nodes: Optional[int] = None,
                               min_distance: float = 0.1, unwind_turns: bool = False,
                               collision_check: Optional["CollisionChecker"] = None, edge_samples: int = 8,
                               edge_resolution: Optional[float] = None, max_edge_samples: int = 64,
                               require_certified: bool = False, refine: bool = False):
    """Track a time sequence of targets through a ladder graph: `n_seeds` IK solutions per waypoint, solved independently of
    each other, and a dynamic program on the device that picks one per waypoint — the path that is complete first, free of
    joint-space jumps second and shortest third (the rule in full: include/minkhip.h).  Where solve_ik_trajectory_multistart
    keeps one whole candidate, the ladder may change IK branch at every waypoint.

    `targets` as in solve_ik_trajectory (no keyframes).  Rung t of instance b is solve_ik_multistart's set of solutions for
    waypoint t's targets from the configuration's own q[b]: seed 0 is q[b], the others are drawn by the stateless generator at
    target index b·T + t, taken from `seeds` — (S, nq), (T, S, nq) or (B, T, S, nq) — or from `seed_table`, queried with every
    waypoint's own frame targets.  A node is tracked when its loop converged without a QP failure.

    An edge costs Σ_k weights_k·(q_t ⊖ q_{t−1})_k² (the first one from the configuration's q); it is a break when that exceeds
    max_step² (`max_step` None: never).  A path's key is (untracked nodes, breaks, length), compared in that order; ties go to
    the lowest node index.  Limits warnings and SolverError follow solve_ik_trajectory's rules on the CHOSEN nodes only
    (`safety_break`, as in mink: False keeps going — the warning — where True raises NotWithinConfigurationLimits).  With
    `update` the configuration is left at the chosen q[:, -1].  The instances are walked in chunks of as many as keep
    chunk·T·n_seeds within `max_instances`; a multi-device configuration shards by instance; the result depends on neither.

    `refine=True` runs refine_path's pass behind the search, in the same call on the device: the chosen path is re-tracked
    across its breaks and lost nodes with the same loop parameters, gate and weights, and comes back only where that makes its
    key strictly smaller — the result is never worse than the search's.  Everything above then speaks of the returned path,
    and the result is a RefinedLadderResult: LadderResult's fields and, behind them, `repaired` and `refined`.

    `n_nodes=K` searches on at most K DISTINCT nodes per rung instead of on all n_seeds results: between the loops and the
    search every rung is reduced on the device by distinct_solutions' rule — radius `min_distance`, reference the
    configuration's q, the ladder's `weights` — so that the search costs T·K² and the device holds B·T·K node rows, whatever
    n_seeds is: n_seeds may then reach 4 096 (1 <= K <= 64).  The nodes are a subset of the results, so the path's key is never
    smaller than without n_nodes and the number of tracked waypoints is the same.  `unwind_turns` (with n_nodes only; alone
    it raises) moves every result to the turn nearest q first, see the function unwind_turns.  The result is then a
    LadderNodesResult — a RefinedLadderNodesResult with refine —: the fields above and, behind them, the selection's.  With
    n_nodes None the call is the one described above, unchanged.

    `collision_check` (a CollisionChecker of the same model; not together with refine=True — the pass that knows of collisions is
    refine="free", below): a joint path whose waypoints and motions
    are free of collision.  Behind the loops every result is checked on the device and a result in collision gets
    ST_IN_COLLISION (in `status_all`; with n_nodes it takes no slot), so it is not tracked; every edge into a tracked node is
    swept with `edge_samples` interior samples and the search counts a waypoint entered by a colliding motion as lost (ladder_path
    states the rule).  The result is a FreeLadderResult / FreeLadderNodesResult: the fields above and `edge_collision`,
    `n_edge_collisions`, `edge_margin`.  A checker with general convex pairs (cylinder-box, ellipsoids, mesh hulls) needs its
    `sweep_rows` >= edge_samples, with and without n_nodes — and together with refine="free" its `check_rows` >=
    1 + 2 edge_samples as well (refine_path's condition).  Without collision_check the call takes exactly the path described
    above.

    `refine="free"` (with collision_check only) runs refine_path(collision_check=...)'s pass behind the checked search, in the
    same call on the device: lost waypoints, breaks and waypoints entered by a colliding motion are re-solved from their
    neighbour on the path, a repair is taken only when it and the motion into it are free, and the path comes back only where
    its key — the checked ladder's — is strictly smaller.  The result is a FreeRefinedLadderResult /
    FreeRefinedLadderNodesResult: the checked call's fields, all of the returned path, then `repaired` and `refined`.

    `edge_resolution` (metres; with collision_check, not together with a non-default edge_samples or any refine) replaces the
    fixed sample count by CollisionChecker.certified_sweep's rule: every edge into a tracked node gets the sample count its own
    motion bound asks for at that resolution, at most `max_edge_samples`, both of its ends are judged, and it comes out
    colliding, proven free for the WHOLE motion, or undecided.  The search blocks the colliding edges — with
    `require_certified` every edge that is not proven free, so that every waypoint `n_tracked` counts is entered by a proven
    motion.  The result is a CertifiedLadderResult / CertifiedLadderNodesResult: the checked call's fields, then `edge_verdict`,
    `edge_lower_bound`, `edge_n_samples` and `n_certified`.  A checker with general convex pairs is refused."""
    del solver
    rule = _edge_rule(edge_resolution, max_edge_samples, require_certified, edge_samples, collision_check, refine)
    free_refine = isinstance(refine, str)
    if free_refine:
        if refine != "free":
            raise ValueError(f'refine must be False, True or "free", got {refine!r}')
        if collision_check is None:
            raise ValueError('refine="free" is the refinement pass with a checker: pass collision_check')
    _check_collision_check(collision_check, configuration, edge_samples, bool(refine) and not free_refine)
    S = int(n_seeds)                                    # (what S may be is the ladder's to say: nat.check_ladder_shape, below)
    if n_nodes is None and unwind_turns:
        raise ValueError("unwind_turns works in front of the selection of n_nodes distinct nodes per rung: pass n_nodes")
    K = r = None
    if n_nodes is not None:
        K, r = _set_args(n_nodes, min_distance, S)
    _, max_iters = _loop_scalars(max_instances, length=max_iters, step_name="qvel_dt", step=qvel_dt,
                                 thresholds=(pos_threshold, ori_threshold), whose="a ladder's rungs")
    step_sq = _max_step_sq(max_step)
    # (judged on the objects themselves: the handle's layout says the same, but only once a handle exists)
    _refuse_plugin_rows({"dense": [t for t in tasks if t._is_dense()], "dense_limits": [x for x in (limits or ()) if x._is_dense()]},
                        "solve_ik_trajectory_ladder")
    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    seqs, T = _trajectory_targets(configuration, tasks, targets)
    if K is None:
        nat.check_ladder_shape(S, T, step_sq)
    else:
        nat.check_ladder_nodes_shape(S, K, T, step_sq, r)
    _need_frame_task(tasks, "a ladder")
    if S * T > int(max_instances):
        raise ValueError(f"one instance's ladder has T*n_seeds = {T * S} loops, beyond max_instances = {int(max_instances)}")
    seeds = _host_array(seeds, "seeds")
    if seeds is not None:
        if seeds.shape not in ((S, nq), (T, S, nq), (B, T, S, nq)):
            raise ValueError(f"seeds must have shape {(S, nq)}, {(T, S, nq)} or {(B, T, S, nq)}, got {seeds.shape}")
        seeds = np.ascontiguousarray(np.broadcast_to(seeds, (B, T, S, nq)))
    weights = _ladder_weights(weights, nv)
    _check_seed_table(seed_table, seeds, configuration, S)
    handles, layout, chunk, n_dev = _compile_outer(configuration, tasks, limits, dt, "solve_ik_trajectory_ladder", S * T,
                                                   max_instances)
    ft, pt, ct = _stacked_targets(configuration, layout, seqs, T)
    pt, ct = _held_over((pt, ct), B, T)
    q = configuration.q_batch
    kw = dict(n_seeds=S, max_iters=max_iters, pos_threshold=float(pos_threshold), ori_threshold=float(ori_threshold),
              max_step_sq=step_sq, rng_seed=int(rng_seed), weights=weights, qvel_dt=qvel_dt, return_all=bool(return_all))
    if K is not None:
        kw.update(n_nodes=K, min_distance=r, unwind_turns=bool(unwind_turns))

    def job(handle, lo, hi):
        args = (q[lo:hi], _rows(ft, 0, lo, hi), _rows(pt, 2, lo, hi), _rows(ct, 2, lo, hi), dt, damping)
        rows = dict(target_index0=lo, seeds=_rows(seeds, 0, lo, hi), seed_table=seed_table)
        if rule is not None:
            return handle.solve_trajectory_ladder_certified(*args, checker=collision_check, resolution=rule[0], max_samples=rule[1],
                                                            require_certified=rule[2], **rows, **kw)
        if collision_check is not None:
            return handle.solve_trajectory_ladder_free(*args, checker=collision_check, edge_samples=int(edge_samples),
                                                       refine=free_refine, **rows, **kw)
        call = handle.solve_trajectory_ladder if K is None else handle.solve_trajectory_ladder_nodes
        return call(*args, refine=bool(refine), **rows, **kw)

    # (the native result, and behind a checker the pair of it and the checker's outputs: the result types by (nodes, checker, refined))
    native = nat.TrajectoryLadderOut if K is None else nat.TrajectoryLadderNodesOut
    res = _join(native if collision_check is None else (native, nat.LadderFreeOut if rule is None else nat.LadderCertifiedOut),
                _chunks_and_shards(configuration, layout, handles, B, chunk, n_dev, job))
    path = res if collision_check is None else res[0]
    _status_epilogue(path.status, "solve_ik_trajectory_ladder", "chosen path(s)",
                     "QP failed at {n} of {of} chosen nodes (first: (instance, waypoint) = {first}, status {status})",
                     safety_break=(lambda b, t: f"the chosen node of (instance, waypoint) = ({b}, {t})") if safety_break else None)
    if update:
        configuration.update(path.q[:, -1] if configuration.batched else path.q[0, -1])
    cls = {(False, False): (LadderResult, RefinedLadderResult), (True, False): (LadderNodesResult, RefinedLadderNodesResult),
           (False, True): (FreeLadderResult, FreeRefinedLadderResult),
           (True, True): (FreeLadderNodesResult, FreeRefinedLadderNodesResult)}[K is not None, collision_check is not None][bool(refine)]
    if rule is not None:
        cls = CertifiedLadderResult if K is None else CertifiedLadderNodesResult
    flags = ("converged", "edge_break", "converged_all") + (("refined",) if refine else ()) + \
        (("edge_collision",) if collision_check is not None else ())
    return _present(configuration, cls, res, flags)


class RefinedPath(NamedTuple):
    """Result of refine_path, (B, T, ·) / (B,) — without the leading axis for an unbatched configuration: the returned path `q`
    with its `tracked` flags; `repaired`: 0 kept, 1 / 2 replaced by the forward / backward sweep; `refined`: whether the
    re-tracked path was returned (else everything is the input path's); `edge_break`, `n_tracked`, `n_breaks`, `path_length` of
    the returned path; `v`, `status`, `iters`, `converged` of the loops of the repaired nodes (zeros at kept nodes)."""
    q: np.ndarray
    tracked: np.ndarray
    repaired: np.ndarray
    refined: np.ndarray
    edge_break: np.ndarray
    n_tracked: np.ndarray
    n_breaks: np.ndarray
    path_length: np.ndarray
    v: np.ndarray
    status: np.ndarray
    iters: np.ndarray
    converged: np.ndarray


FreeRefinedPath = nat._extended(
    "FreeRefinedPath", RefinedPath, nat.LADDER_REFINE_FREE_IO_FIELDS,
    """Result of refine_path(collision_check=...): RefinedPath's fields, in its order — `tracked` the EFFECTIVE flags of the
    returned path: tracked and free of collision —, then of the returned path `edge_collision` (B, T) — the motion into waypoint t
    passes through collision, entry 0 never —, `n_edge_collisions` (B,), `edge_margin` (B, T) — +inf at waypoint 0, NaN where the
    edge was not swept — and `node_margin` (B, T).  `n_tracked` counts the waypoints that are tracked, free of collision and
    entered by a free motion.""", optional=False, module=__name__)


def refine_path(configuration: Configuration, tasks: Sequence, dt: float, targets, q_path, tracked=None, max_iters: int = 32,
                pos_threshold: float = 1e-4, ori_threshold: float = 1e-4, max_step: Optional[float] = None, weights=None,
                update: bool = True, max_instances: int = 1 << 20, damping: float = 1e-12, limits: Optional[Sequence] = None,
                safety_break: bool = False, solver: str = "mi355x", collision_check: Optional["CollisionChecker"] = None,
                edge_samples: int = 8) -> RefinedPath:
    """The ladder's refinement pass alone, over the caller's own path: q_path (T, nq) or (B, T, nq) — a ladder's chosen path,
    a planner's, an earlier call's — with `tracked` (same leading shape, default: every node counts as tracked) and the
    `targets` of solve_ik_trajectory (no keyframes) the path is meant to follow.

    A working copy of the path is swept forward, then backward.  A waypoint is bad when its node is not tracked or the step
    from the neighbour the sweep comes from costs more than max_step² (the ladder's edge cost, with `weights`; `max_step` None:
    only lost nodes are bad; the step from the configuration's q into waypoint 0 is never a break).  A bad waypoint is
    re-solved by the threshold-terminated loop from that neighbour and the result is taken when it converged without a QP
    failure and stays within max_step of the neighbour.  The working copy is returned only where its key (untracked nodes,
    breaks, length) is strictly smaller than the input path's: the result is never worse than what came in (the rule in
    full: include/minkhip.h).  Each sweep costs T loop launches on the B instances.

    Limits warnings and SolverError follow solve_ik_trajectory's rules on the RETURNED repaired nodes only (`safety_break` as
    in solve_ik_trajectory_ladder).  With `update` the configuration is left at the returned q[:, -1].  When B exceeds
    `max_instances` the paths are walked in chunks of instances; a multi-device configuration shards by instance; the result
    depends on neither.

    `collision_check` (a CollisionChecker of the same model): the pass whose repairs are free of collision.  A node in collision
    counts as not tracked and a waypoint entered by a colliding motion as lost (ladder_path's rule, `edge_samples` interior
    samples per motion) — both are bad and get re-solved; a result is taken only when it is itself free of collision and the
    motion from the neighbour is; the motion on its other side is swept anew, and the key that decides which path comes back
    counts all of it.  Everything is checked on the device between the loops.  The result is then a FreeRefinedPath.  A
    checker with general convex pairs (cylinder-box, ellipsoids, mesh hulls) needs its `check_rows` >= 1 + 2 edge_samples AND its
    `sweep_rows` >= edge_samples (the pass sweeps the incoming path); the loop results of a waypoint step are then judged in
    chunks of check_rows // (1 + 2 edge_samples) instances, and the result does not depend on either value.  Without
    collision_check the call is the one above, unchanged."""
    del solver
    _check_collision_check(collision_check, configuration, edge_samples)
    _, max_iters = _loop_scalars(max_instances, length=max_iters, thresholds=(pos_threshold, ori_threshold),
                                 whose="the refinement's loops")
    step_sq = _max_step_sq(max_step)
    _refuse_plugin_rows({"dense": [t for t in tasks if t._is_dense()], "dense_limits": [x for x in (limits or ()) if x._is_dense()]},
                        "refine_path")
    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    seqs, T = _trajectory_targets(configuration, tasks, targets)
    nat.check_ladder_shape(1, T, step_sq)
    q_path = _host_array(q_path, "q_path")
    if q_path is None or q_path.shape not in ((T, nq), (B, T, nq)):
        raise ValueError(f"q_path must have shape {(T, nq)} or {(B, T, nq)}, got {None if q_path is None else q_path.shape}")
    q_path = np.ascontiguousarray(np.broadcast_to(q_path, (B, T, nq)))
    tracked = _host_flags(tracked, "tracked", (T,), B)
    weights = _ladder_weights(weights, nv)
    _need_frame_task(tasks, "a ladder refinement")
    handles, layout, chunk, n_dev = _compile_outer(configuration, tasks, limits, dt, "refine_path", 1, max_instances)
    ft, pt, ct = _stacked_targets(configuration, layout, seqs, T)
    pt, ct = _held_over((pt, ct), B, T)
    q = configuration.q_batch

    def job(handle, lo, hi):
        n = hi - lo
        kw = dict(max_iters=max_iters, pos_threshold=float(pos_threshold), ori_threshold=float(ori_threshold), max_step_sq=step_sq,
                  weights=weights, v=np.zeros((n, T, nv)), status=np.zeros((n, T), np.int32), iters=np.zeros((n, T), np.int32),
                  converged=np.zeros((n, T), np.int32))
        args = (None if tracked is None else tracked[lo:hi], _rows(ft, 0, lo, hi), _rows(pt, 2, lo, hi), _rows(ct, 2, lo, hi), dt,
                damping)
        if collision_check is not None:
            return handle.ladder_refine_free(q[lo:hi], q_path[lo:hi], collision_check, *args, edge_samples=int(edge_samples), **kw)
        return handle.ladder_refine(q[lo:hi], q_path[lo:hi], *args, **kw)

    res = _join(nat.LadderRefineOut if collision_check is None else nat.LadderRefineFreeOut,
                _chunks_and_shards(configuration, layout, handles, B, chunk, n_dev, job))
    _status_epilogue(res.status, "refine_path", "returned path(s)",
                     "QP failed at {n} of {of} returned nodes (first: (instance, waypoint) = {first}, status {status})",
                     safety_break=(lambda b, t: f"the repaired node of (instance, waypoint) = ({b}, {t})") if safety_break else None)
    if update:
        configuration.update(res.q[:, -1] if configuration.batched else res.q[0, -1])
    flags = ("tracked", "refined", "edge_break", "converged")
    if collision_check is None:
        return _present(configuration, RefinedPath, res, flags)
    return _present(configuration, FreeRefinedPath, res, flags + ("edge_collision",))


def ladder_path(configuration: Configuration, q_nodes, tracked=None, max_step: Optional[float] = None, weights=None,
                collision_check: Optional["CollisionChecker"] = None, edge_samples: int = 8,
                edge_resolution: Optional[float] = None, max_edge_samples: int = 64, require_certified: bool = False) -> LadderPath:
    """The ladder's search alone, over the caller's own rungs (closed-form IK branches, solutions of earlier calls): q_nodes
    (T, S, nq) or (B, T, S, nq), `tracked` (same leading shape, default: every node counts as tracked), the start edge from the
    configuration's q.  The rule — key (untracked, breaks, length), ties to the lowest index — is solve_ik_trajectory_ladder's;
    the configuration is not changed.

    `collision_check` (a CollisionChecker of the same model): the path whose waypoints and motions are free of collision.  Every
    node is checked on the device and a node in collision counts as not tracked; every edge into a tracked node is swept with
    `edge_samples` interior samples (CollisionChecker.swept_clearance's rule) and a waypoint entered by a colliding motion counts
    as lost, so the key's first component counts the waypoints that are untracked, in collision or entered through collision.
    The result is then a FreeLadderPath.  A checker with general convex pairs (cylinder-box, ellipsoids, mesh hulls) needs its
    `sweep_rows` >= edge_samples; the edges are then swept in chunks of sweep_rows // edge_samples, and the result does not
    depend on the value.  Without collision_check the call is the one above, unchanged.

    `edge_resolution` (metres; with collision_check, not together with a non-default edge_samples) judges the edges by
    CollisionChecker.certified_sweep's rule instead: the sample count of an edge follows from its own motion bound at that
    resolution (at most `max_edge_samples`), both of its ends are judged — so an edge that LEAVES a colliding node collides —,
    and its verdict is colliding, proven free along the whole motion, or undecided.  The search blocks the colliding edges, with
    `require_certified` every edge that is not proven free.  The result is then a CertifiedLadderPath.  A checker with general
    convex pairs is refused.  Without edge_resolution the call is the one above, unchanged."""
    from .tasks import PostureTask

    rule = _edge_rule(edge_resolution, max_edge_samples, require_certified, edge_samples, collision_check, False)
    _check_collision_check(collision_check, configuration, edge_samples)
    step_sq = _max_step_sq(max_step)
    B, nq, nv = configuration.batch_size, configuration.nq, configuration.nv
    q_nodes = _host_array(q_nodes, "q_nodes")
    if q_nodes is None or q_nodes.ndim not in (3, 4) or q_nodes.shape[-1] != nq or (q_nodes.ndim == 4 and q_nodes.shape[0] != B):
        raise ValueError(f"q_nodes must have shape (T, S, {nq}) or ({B}, T, S, {nq}), got {None if q_nodes is None else q_nodes.shape}")
    T, S = q_nodes.shape[-3], q_nodes.shape[-2]
    nat.check_ladder_shape(S, T, step_sq)
    q_nodes = np.ascontiguousarray(np.broadcast_to(q_nodes, (B, T, S, nq)))
    tracked = _host_flags(tracked, "tracked", (T, S), B)
    weights = _ladder_weights(weights, nv)
    # (the search reads the model's joint table through a problem handle: the smallest one, a posture task, serves)
    prob, layout = _compile(configuration, [PostureTask(configuration.model, cost=1.0)], None, 1, devices=configuration.devices[:1])
    with _pin(configuration, layout):
        if collision_check is None:
            return _present(configuration, LadderPath, prob.ladder_select(configuration.q_batch, q_nodes, tracked, step_sq, weights),
                            flags=("edge_break",))
        if rule is not None:
            out = prob.ladder_select_certified(configuration.q_batch, q_nodes, collision_check, tracked, step_sq, weights, *rule, True)
        else:
            out = prob.ladder_select_free(configuration.q_batch, q_nodes, collision_check, tracked, step_sq, weights, int(edge_samples),
                                          True)
    return _present(configuration, FreeLadderPath if rule is None else CertifiedLadderPath, out, flags=("edge_break", "edge_collision"))


def _chunks_and_shards(configuration: Configuration, layout, handles, B: int, chunk: int, n_dev: int, job):
    """[job(handle, lo, hi), ...] over the rows [0, B): chunks of `chunk` rows, each split among the `n_dev` handles of
    _compile_outer, which run side by side.  The one driver of solve_ik_multistart, solve_ik_trajectory and
    solve_ik_trajectory_multistart: a job is told its global row offset `lo`, so results do not depend on chunks or shards
    (ShardedProblem.solve splits rows without telling a shard its offset: its shards are driven from here instead)."""
    parts = []
    with _pin(configuration, layout):
        for c0 in range(0, B, chunk):
            c1 = min(B, c0 + chunk)
            bounds = [(c0 + lo, c0 + hi) for lo, hi in (shard_bounds(c1 - c0, n_dev, r) for r in range(n_dev))]
            bounds = [(lo, hi) for lo, hi in bounds if hi > lo]
            if len(bounds) == 1:
                parts.append(job(handles[0], *bounds[0]))
            else:
                from concurrent.futures import ThreadPoolExecutor
                with ThreadPoolExecutor(max_workers=len(bounds)) as pool:      # (a libminkhip call releases the GIL)
                    parts += [f.result() for f in [pool.submit(job, h, lo, hi) for h, (lo, hi) in zip(handles, bounds)]]
    return parts
