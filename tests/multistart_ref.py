"""numpy restatement of multi-start IK's device-side rules (include/minkhip.h, mkh_solve_multistart): the counter-based
random numbers, the per-joint seeding rule and the selection rule.  Written from the header's text, not from the kernels."""

import numpy as np

from oracle import mjmath

JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_G = np.uint64(0x9E3779B97F4A7C15)
ST_OUTSIDE_LIMITS = 1


def _mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform(rng_seed, t, s, k):
    """u(rng_seed, t, s, k) in [0, 1): broadcasts over t (global target index), s (seed index), k (draw index)."""
    t, s, k = (np.asarray(x, dtype=np.uint64) for x in (t, s, k))
    with np.errstate(over="ignore"):
        h = _mix(np.uint64(int(rng_seed) & 0xFFFFFFFFFFFFFFFF) + _G)
        h = _mix((h ^ t) + _G)
        h = _mix((h ^ ((s << np.uint64(32)) | k)) + _G)
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def draw_seeds(model, q, n_seeds, rng_seed=0, target_index0=0):
    """(B, S, nq): row 0 of every target is q[b]; rows s >= 1 by the seeding rule."""
    q = np.asarray(q, dtype=np.float64)
    B, S = q.shape[0], int(n_seeds)
    out = np.repeat(q[:, None, :], S, axis=1)
    if S == 1:
        return out
    t = (np.arange(B, dtype=np.uint64) + np.uint64(target_index0))[:, None]
    s = np.arange(1, S, dtype=np.uint64)[None, :]
    u = lambda k: uniform(rng_seed, t, s, k)
    for j in range(model.njnt):
        jt, qa = int(model.jnt_type[j]), int(model.jnt_qposadr[j])
        limited = bool(model.jnt_limited[j])
        lo, hi = (float(x) for x in model.jnt_range[j])
        if jt in (JNT_SLIDE, JNT_HINGE):
            if limited:
                out[:, 1:, qa] = lo + (hi - lo) * u(qa)
            elif jt == JNT_HINGE:
                out[:, 1:, qa] = (q[:, None, qa] - np.pi) + (2.0 * np.pi) * u(qa)
        elif jt == JNT_BALL:
            theta_max = hi if limited else np.pi
            z = 2.0 * u(qa) - 1.0
            r = np.sqrt(1.0 - z * z)
            phi = (2.0 * np.pi) * u(qa + 1)
            half = 0.5 * (theta_max * u(qa + 2))
            sh = np.sin(half)
            out[:, 1:, qa] = np.cos(half)
            out[:, 1:, qa + 1] = (r * np.cos(phi)) * sh
            out[:, 1:, qa + 2] = (r * np.sin(phi)) * sh
            out[:, 1:, qa + 3] = z * sh
    return out


def distance(model, q, q_ref, weights=None):
    """d = sum_k w_k ((q (-) q_ref)_k)^2 with mj_differentiatePos at dt = 1."""
    dv = np.zeros(model.nv)
    mjmath.mj_differentiatePos(model, dv, 1.0, np.asarray(q_ref, dtype=np.float64), np.asarray(q, dtype=np.float64))
    w = np.ones(model.nv) if weights is None else np.asarray(weights, dtype=np.float64)
    return float(np.sum(w * dv * dv))


def eligible(converged, status):
    return (np.asarray(converged) != 0) & ((np.asarray(status) & ~ST_OUTSIDE_LIMITS) == 0)


def select(d, converged, status):
    """(seed_index, converged, n_converged) of one target from its seeds' distances d (S,), loop flags and status bits:
    the eligible seed with the smallest d, ties to the lowest index; no eligible seed → seed 0, not converged."""
    ok = eligible(converged, status)
    if not ok.any():
        return 0, False, 0
    dd = np.where(ok, np.asarray(d, dtype=np.float64), np.inf)
    best = int(np.flatnonzero(ok & (dd == dd[ok].min()))[0])
    return best, True, int(ok.sum())
