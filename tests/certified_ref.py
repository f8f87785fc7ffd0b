"""numpy restatement of THE RULE OF THE CERTIFIED SWEEP (include/minkhip.h): the reach table from the flat model, the edge weights
from the sweep's own difference, the sample count, the points by keyframe_ref.blend_posture, each judged by
clearance_ref.distances, and numpy's min / argmin over margins and cone crossings.  Written from the header's text, not from the
kernel or the host header.  The reference of tests/test_gpu_certified_sweep.py; tests/test_certified_sweep_cpu.py holds it
against closed-form numbers and against its own claim (the Lipschitz property, the soundness of the certificate)."""

from typing import NamedTuple

import numpy as np

import clearance_ref as cr
import keyframe_ref as kf
from oracle import mjmath

JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3
PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = 0, 2, 3, 4, 5, 6, 7
UNDECIDED, CERTIFIED, COLLIDES = 0, 1, 2


class RefCertified(NamedTuple):
    margin: np.ndarray        # (N,)
    sample: np.ndarray        # (N,) int32
    pair: np.ndarray          # (N,) int32
    lower_bound: np.ndarray   # (N,)
    segment: np.ndarray       # (N,) int32
    bound_pair: np.ndarray    # (N,) int32
    n_samples: np.ndarray     # (N,) int32
    motion: np.ndarray        # (N,)
    capped: np.ndarray        # (N,) int32
    verdict: np.ndarray       # (N,) int32
    L: np.ndarray             # (N, P): the motion bound of every pair
    points: list              # per edge (M + 2, P): m_{k,i}; None for an edge with a non-finite end
    cones: list               # per edge (M + 1, P): the crossing points; None for a non-finite or an unbounded edge


def geom_radius(model, g):
    t, s = int(model.geom_type[g]), np.asarray(model.geom_size[g], dtype=np.float64)
    if t == SPHERE:
        return float(s[0])
    if t == CAPSULE:
        return float(s[0] + s[1])
    if t == ELLIPSOID:
        return float(s.max())
    if t == CYLINDER:
        return float(np.hypot(s[0], s[1]))
    if t == BOX:
        return float(np.linalg.norm(s))
    if t == MESH:
        k = int(model.geom_dataid[g])
        v = np.asarray(model.mesh_vert, dtype=np.float64).reshape(-1, 3)[int(model.mesh_vertadr[k]):int(model.mesh_vertadr[k]) + int(model.mesh_vertnum[k])]
        return float(np.linalg.norm(v, axis=1).max())
    return np.inf                                               # a plane


def _joints(model, c):
    return range(int(model.body_jntadr[c]), int(model.body_jntadr[c]) + int(model.body_jntnum[c])) if int(model.body_jntnum[c]) > 0 else range(0)


def _shift(model, j):
    """What joint j adds to D of its body."""
    jt = int(model.jnt_type[j])
    if jt == JNT_SLIDE:
        if not model.jnt_limited[j]:
            return np.inf
        q0 = float(model.qpos0[int(model.jnt_qposadr[j])])
        lo, hi = (float(x) for x in np.asarray(model.jnt_range).reshape(-1, 2)[j])
        return max(abs(lo - q0), abs(hi - q0))
    if jt in (JNT_HINGE, JNT_BALL):
        return 2.0 * float(np.linalg.norm(np.asarray(model.jnt_pos).reshape(-1, 3)[j]))
    return np.inf                                               # a free joint


def _D(model, c, after=None):
    """D(c), or D_after(c, j) with after = j."""
    return sum((_shift(model, j) for j in _joints(model, c) if after is None or j > after), 0.0)


def _chain(model, b):
    out = []
    while b > 0:
        out.append(b)
        b = int(model.body_parentid[b])
    return out[::-1]


def reach_table(model, pairs):
    """(P, njnt, 2): coef[k][j][0] for the linear weight of joint j, [1] for the angular one."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    coef = np.zeros((len(pairs), model.njnt, 2))
    body_pos, jnt_pos, geom_pos = (np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (model.body_pos, model.jnt_pos, model.geom_pos))
    for k, gs in enumerate(pairs):
        chains = [_chain(model, int(model.geom_bodyid[int(g)])) for g in gs]
        n = 0
        while n < min(len(chains[0]), len(chains[1])) and chains[0][n] == chains[1][n]:
            n += 1
        for g, chain in zip(gs, chains):
            g, rest = int(g), chain[n:]
            for t, c in enumerate(rest):
                for j in _joints(model, c):
                    jt = int(model.jnt_type[j])
                    coef[k, j, 0] = 1.0 if jt in (JNT_SLIDE, JNT_FREE) else 0.0
                    if jt != JNT_SLIDE:
                        rho = np.linalg.norm(jnt_pos[j]) + _D(model, c, after=j)
                        rho += sum(np.linalg.norm(body_pos[ci]) + _D(model, ci) for ci in rest[t + 1:])
                        coef[k, j, 1] = rho + np.linalg.norm(geom_pos[g]) + geom_radius(model, g)
    return coef


def edge_weights(model, a, b):
    """(lin (njnt,), rot (njnt,)) of b (-) a: the sweep's own difference."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    lin, rot = np.zeros(model.njnt), np.zeros(model.njnt)
    for j in range(model.njnt):
        jt, qa = int(model.jnt_type[j]), int(model.jnt_qposadr[j])
        if jt == JNT_HINGE:
            rot[j] = abs(b[qa] - a[qa])
            continue
        if jt == JNT_SLIDE:
            lin[j] = abs(b[qa] - a[qa])
            continue
        if jt == JNT_FREE:
            lin[j] = np.linalg.norm(b[qa:qa + 3] - a[qa:qa + 3])
            qa += 3
        neg, dif = np.empty(4), np.empty(4)
        mjmath.mju_negQuat(neg, a[qa:qa + 4])
        mjmath.mju_mulQuat(dif, neg, b[qa:qa + 4])
        rot[j] = np.linalg.norm(mjmath.mju_quat2Vel(dif, 1.0))
    return lin, rot


def pair_motion(coef, lin, rot):
    """L_k (P,): a weight of 0 contributes 0 whatever its coefficient."""
    L = np.zeros(len(coef))
    for j in range(coef.shape[1]):
        if lin[j] > 0.0:
            L = L + coef[:, j, 0] * lin[j]
        if rot[j] > 0.0:
            L = L + coef[:, j, 1] * rot[j]
    return L


def slide_outside(model, q):
    rng = np.asarray(model.jnt_range, dtype=np.float64).reshape(-1, 2)
    for j in range(model.njnt):
        if int(model.jnt_type[j]) == JNT_SLIDE and model.jnt_limited[j]:
            x = q[int(model.jnt_qposadr[j])]
            if x < rng[j, 0] or x > rng[j, 1]:
                return True
    return False


def sample_count(motion, unbounded, resolution, max_samples):
    """(M, capped)."""
    want = np.ceil(motion / resolution) - 1.0
    capped = int(want > max_samples)
    if unbounded or capped:
        return int(max_samples), capped
    return int(max(want, 1.0)), capped


def point_rows(model, a, b, M):
    """q(u_i), i = 0 .. M + 1: (M + 2, nq)."""
    return np.stack([kf.blend_posture(model, a, b, float(i) / float(M + 1)) for i in range(M + 2)])


def certified_sweep(model, limits, q_from, q_to, resolution, max_samples=64, coef=None):
    """The rule on N edges: q_from, q_to (N, nq); `limits` as clearance_ref.clearance takes them."""
    pairs, dmin, _ = cr.pair_list(limits)
    coef = reach_table(model, pairs) if coef is None else coef
    q_from = np.asarray(q_from, dtype=np.float64).reshape(-1, model.nq)
    q_to = np.asarray(q_to, dtype=np.float64).reshape(-1, model.nq)
    N, P = len(q_from), len(pairs)
    f8, i4 = (lambda v: np.full(N, v, dtype=np.float64)), (lambda v: np.full(N, v, dtype=np.int32))
    out = RefCertified(f8(np.nan), i4(0), i4(0), f8(np.nan), i4(0), i4(0), i4(1), f8(np.nan), i4(0), i4(COLLIDES), np.full((N, P), np.nan),
                       [None] * N, [None] * N)
    for e in range(N):
        a, b = q_from[e], q_to[e]
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        L = pair_motion(coef, *edge_weights(model, a, b))
        motion = float(L.max())
        unbounded = not np.isfinite(motion) or slide_outside(model, a) or slide_outside(model, b)
        M, capped = sample_count(motion, unbounded, resolution, max_samples)
        m = (cr.distances(model, limits, point_rows(model, a, b, M)) - dmin[None, :]) + 0.0            # (M + 2, P)
        i, k = np.unravel_index(np.argmin(m), m.shape)          # (row-major: the lowest point, then its lowest pair; the first NaN)
        out.margin[e], out.sample[e], out.pair[e] = m[i, k], i, k
        out.n_samples[e], out.motion[e], out.capped[e], out.L[e] = M, motion, capped, L
        out.points[e] = m
        if unbounded:
            out.lower_bound[e] = -np.inf
        else:
            cones = 0.5 * ((m[:-1] + m[1:]) - (L / float(M + 1))[None, :])                              # (M + 1, P)
            s, kb = np.unravel_index(np.argmin(cones), cones.shape)
            out.lower_bound[e], out.segment[e], out.bound_pair[e] = cones[s, kb], s, kb
            out.cones[e] = cones
        out.verdict[e] = COLLIDES if not (out.margin[e] >= 0.0) else (CERTIFIED if out.lower_bound[e] >= 0.0 else UNDECIDED)
    return out
