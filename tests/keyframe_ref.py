"""numpy restatement of keyframed trajectory IK's interpolation (include/minkhip.h, mkh_solve_keyframes, "THE RULE").
Written from the header's text, not from the kernels, on the oracle's own Lie and MuJoCo math (oracle/lie.py,
oracle/mjmath.py): which segment a waypoint time falls in, the three blends, and where the K and T axes sit."""

import numpy as np

from oracle import lie, mjmath

JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3


def check_times(key_times, waypoint_times):
    """The refusals of the rule, as ValueError."""
    kt, wt = np.asarray(key_times, dtype=np.float64), np.asarray(waypoint_times, dtype=np.float64)
    if kt.ndim != 1 or wt.ndim != 1 or kt.size < 1 or wt.size < 1:
        raise ValueError("K >= 1 key times and T >= 1 waypoint times")
    if np.isnan(kt).any() or np.isnan(wt).any():
        raise ValueError("NaN")
    if (np.diff(kt) <= 0).any():
        raise ValueError("key times must increase")
    if (np.diff(wt) < 0).any():
        raise ValueError("waypoint times must not decrease")
    if wt.min() < kt[0] or wt.max() > kt[-1]:
        raise ValueError("waypoint time outside the keyframes' range")
    return kt, wt


def segment(key_times, tau):
    """(k, u): k the largest index with key_times[k] <= tau; u = 0 at the last keyframe, else one rounded subtraction over
    one rounded subtraction."""
    kt = np.asarray(key_times, dtype=np.float64)
    k = int(np.nonzero(kt <= tau)[0][-1])
    if k == len(kt) - 1:
        return k, 0.0
    num = np.float64(tau) - kt[k]
    den = kt[k + 1] - kt[k]
    return k, float(num / den)


def _lerp(a, b, u):
    d = b - a                      # a rounded difference,
    p = u * d                      # a rounded product,
    return a + p                   # a rounded sum


def blend_pose(a, b, u):
    """wxyz_xyz between poses a and b: rotation normalize(q_a exp(u log(q_a^-1 q_b))), translation p_a + u (p_b - p_a)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if u == 0.0:
        return a.copy()
    w = lie.so3_log(lie.so3_multiply(lie.so3_inverse(a[:4]), b[:4]))
    q = lie.so3_multiply(a[:4], lie.so3_exp(u * w))
    return np.concatenate([q / np.linalg.norm(q), _lerp(a[4:], b[4:], u)])


def blend_posture(m, a, b, u):
    """q_a (+) u (q_b (-) q_a) joint by joint."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = a.copy()
    if u == 0.0:
        return out
    for j in range(m.njnt):
        jt, qa = int(m.jnt_type[j]), int(m.jnt_qposadr[j])
        if jt in (JNT_SLIDE, JNT_HINGE):
            out[qa] = _lerp(a[qa], b[qa], u)
            continue
        if jt == JNT_FREE:
            out[qa:qa + 3] = _lerp(a[qa:qa + 3], b[qa:qa + 3], u)
            qa += 3
        neg, dif = np.empty(4), np.empty(4)
        mjmath.mju_negQuat(neg, a[qa:qa + 4])
        mjmath.mju_mulQuat(dif, neg, b[qa:qa + 4])
        quat = a[qa:qa + 4].copy()
        mjmath.mju_quatIntegrate(quat, mjmath.mju_quat2Vel(dif, 1.0), u)
        out[qa:qa + 4] = quat / np.linalg.norm(quat)
    return out


def blend_com(a, b, u):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.copy() if u == 0.0 else _lerp(a, b, u)


def _keys_bk(x, rows, time_major):
    """A keyframe array with its rows axis first and its K axis second, whatever the layout: (B, K, n, w) / (K, B, n, w)
    time-major / (K, n, w) without a B axis (rows = 1)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 3:
        return x[None]
    assert x.ndim == 4 and (x.shape[1] if time_major else x.shape[0]) == rows
    return np.swapaxes(x, 0, 1) if time_major else x


def interpolate(keys, key_times, waypoint_times, kind, model=None, time_major=False):
    """The interpolated targets of one group in the layout the trajectory call takes them in: keys (B, K, n, w) ->
    (B, T, n, w); (K, B, n, w) time-major -> (T, B, n, w); (K, n, w) -> (T, n, w).  kind: "frame", "posture" or "com"."""
    kt, wt = check_times(key_times, waypoint_times)
    x = np.asarray(keys, dtype=np.float64)
    xb = _keys_bk(x, x.shape[1] if (time_major and x.ndim == 4) else x.shape[0], time_major)
    R, K, n, w = xb.shape
    assert K == len(kt)
    out = np.empty((R, len(wt), n, w))
    for t, tau in enumerate(wt):
        k, u = segment(kt, tau)
        for r in range(R):
            for i in range(n):
                a = xb[r, k, i]
                c = xb[r, min(k + 1, K - 1), i]
                if kind == "frame":
                    out[r, t, i] = blend_pose(a, c, u)
                elif kind == "posture":
                    out[r, t, i] = blend_posture(model, a, c, u)
                else:
                    out[r, t, i] = blend_com(a, c, u)
    if x.ndim == 3:
        return out[0]
    return np.ascontiguousarray(np.swapaxes(out, 0, 1)) if time_major else out
