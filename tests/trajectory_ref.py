"""numpy restatement of trajectory IK's layouts and of its waypoint velocity (include/minkhip.h, mkh_solve_trajectory).
Written from the header's text, not from the kernels: where the T axis of every array sits, which slab of a target a
waypoint reads, and qvel[b, t] = mj_differentiatePos(q_{t-1}[b], q_t[b]) at waypoint_dt with q_{-1} = q."""

import numpy as np

JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3


def to_time_major(x):
    """(B, T, ...) -> (T, B, ...), contiguous."""
    return None if x is None else np.ascontiguousarray(np.swapaxes(np.asarray(x), 0, 1))


def to_batch_major(x):
    """(T, B, ...) -> (B, T, ...), contiguous."""
    return to_time_major(x)


def waypoint_target(x, t, n, w, B, time_major=False):
    """What waypoint t's loop gets of a posture / CoM target x of n tasks of width w, as a held target of solve():
    (n, w) and (B, n, w) are held over the trajectory; (T, n, w) has a leading T axis; four axes: (B, T, n, w), or
    (T, B, n, w) time-major.  A 3-d array whose first axis equals B is the batched held target."""
    if x is None:
        return None
    x = np.asarray(x)
    if x.ndim == 2:
        return x
    if x.ndim == 3:
        return x if x.shape[0] == B else np.ascontiguousarray(x[t])
    return np.ascontiguousarray(x[t] if time_major else x[:, t])


def _qmul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def _rotation_vector_over_dt(prev, cur, dt):
    """conj(prev) * cur as a rotation vector (angle in (-pi, pi]) divided by dt."""
    conj = prev * np.array([1.0, -1.0, -1.0, -1.0])
    d = _qmul(conj, cur)
    axis = d[..., 1:]
    s = np.linalg.norm(axis, axis=-1)
    small = s < 1e-15
    unit = np.where(small[..., None], np.array([1.0, 0.0, 0.0]), axis / np.where(small, 1.0, s)[..., None])
    angle = 2.0 * np.arctan2(s, d[..., 0])
    angle = np.where(angle > np.pi, angle - 2.0 * np.pi, angle)
    return unit * (angle / dt)[..., None]


def qvel(model, q, q_traj, waypoint_dt, time_major=False):
    """(B, T, nv) — (T, B, nv) time-major — from the start q (B, nq) and the trajectory's configurations."""
    q = np.asarray(q, dtype=np.float64)
    qt = np.asarray(q_traj, dtype=np.float64)
    if time_major:
        qt = np.swapaxes(qt, 0, 1)
    prev = np.concatenate([q[:, None, :], qt[:, :-1, :]], axis=1)          # q_{t-1}, q_{-1} = q
    out = np.zeros(qt.shape[:2] + (model.nv,))
    dt = float(waypoint_dt)
    for j in range(model.njnt):
        jt, qa, va = int(model.jnt_type[j]), int(model.jnt_qposadr[j]), int(model.jnt_dofadr[j])
        if jt in (JNT_SLIDE, JNT_HINGE):
            out[..., va] = (qt[..., qa] - prev[..., qa]) / dt
            continue
        if jt == JNT_FREE:
            out[..., va:va + 3] = (qt[..., qa:qa + 3] - prev[..., qa:qa + 3]) / dt
            qa += 3; va += 3
        out[..., va:va + 3] = _rotation_vector_over_dt(prev[..., qa:qa + 4], qt[..., qa:qa + 4], dt)
    return np.ascontiguousarray(np.swapaxes(out, 0, 1)) if time_major else out


def quaternion_dofs(model):
    """Boolean mask over nv: the dofs that come from a quaternion (ball joints, the rotation of free joints)."""
    mask = np.zeros(model.nv, dtype=bool)
    for j in range(model.njnt):
        jt, va = int(model.jnt_type[j]), int(model.jnt_dofadr[j])
        if jt == JNT_BALL:
            mask[va:va + 3] = True
        elif jt == JNT_FREE:
            mask[va + 3:va + 6] = True
    return mask
