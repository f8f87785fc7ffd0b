"""Synthetic candidate sets for the distinct-set selection (tests/test_solution_set_cpu.py, tests/test_gpu_solution_sets.py):
clusters of candidates around centres placed on the model's configuration manifold so that every decision of the rule has a
margin — centres at least 3·r apart in the weighted metric, their distances from the reference at least 1e-3 apart, the
candidates of a cluster within 1e-6 of its centre."""

import numpy as np

import multistart_ref as ms
from oracle import mjmath


def rotational_dofs(m):
    """The tangent coordinates that belong to a quaternion (free joint: its last three, ball joint: all three)."""
    out = []
    for j in range(m.njnt):
        jt, va = int(m.jnt_type[j]), int(m.jnt_dofadr[j])
        if jt == ms.JNT_FREE:
            out += [va + 3, va + 4, va + 5]
        elif jt == ms.JNT_BALL:
            out += [va, va + 1, va + 2]
    return out


def _moved(m, q, v):
    q = np.array(q, dtype=np.float64)
    mjmath.mj_integratePos(m, q, np.asarray(v, dtype=np.float64), 1.0)
    return q


def make_case(m, rng, B, S, n_clusters, weights=None, noise=1e-6, valid_fraction=0.9, duplicates=False):
    """(q_cand (B, S, nq), valid (B, S) int32, q_ref (B, nq), centres (B, n_clusters, nq)).  Centre c of a target lies
    a_c = 0.5 + 0.15·c (weighted norm) from the reference along a tangent coordinate of its own — one of them a quaternion's
    when the model has one —, so d_ref(c) = a_c² (0.25, 0.4225, 0.64, ...: gaps >= 0.17) and two centres are about
    sqrt(a_c² + a_c'²) >= 0.8 apart: 8·r for r = 0.1.  Candidates are centres moved by `noise`·N(0, 1) per tangent coordinate —
    or, with `duplicates`, bitwise copies of the centres.  check_case() asserts the conditions."""
    assert n_clusters <= m.nv
    w = np.ones(m.nv) if weights is None else np.asarray(weights, dtype=np.float64)
    rot = rotational_dofs(m)
    q_cand, valid = np.empty((B, S, m.nq)), np.zeros((B, S), dtype=np.int32)
    q_ref, centres = np.empty((B, m.nq)), np.empty((B, n_clusters, m.nq))
    for b in range(B):
        q_ref[b] = _moved(m, m.qpos0, rng.normal(scale=0.3, size=m.nv))
        axes = list(rng.permutation(m.nv)[:n_clusters])
        if rot and not set(axes) & set(rot):
            axes[0] = int(rng.choice(rot))
        for c, k in enumerate(axes):
            u = np.zeros(m.nv)
            u[k] = (0.5 + 0.15 * c) / np.sqrt(w[k]) * rng.choice([-1.0, 1.0])
            centres[b, c] = _moved(m, q_ref[b], u)
        member = rng.integers(0, n_clusters, size=S)
        member[:min(S, n_clusters)] = rng.permutation(n_clusters)[:min(S, n_clusters)]      # every cluster is populated (S allowing)
        member = rng.permutation(member)
        for s in range(S):
            q_cand[b, s] = centres[b, member[s]] if duplicates else _moved(m, centres[b, member[s]], noise * rng.normal(size=m.nv))
        valid[b] = rng.uniform(size=S) < valid_fraction
    return q_cand, valid, q_ref, centres


def check_case(m, centres, q_ref, r, weights=None):
    """The fixture's conditions, by the numpy distance: centres >= 3·r apart, their d_ref >= 1e-3 apart."""
    for b in range(len(centres)):
        n = len(centres[b])
        dr = sorted(ms.distance(m, c, q_ref[b], weights) for c in centres[b])
        assert all(y - x >= 1e-3 for x, y in zip(dr, dr[1:])), (b, dr)
        for i in range(n):
            for j in range(n):
                if i != j:
                    assert ms.distance(m, centres[b, i], centres[b, j], weights) >= 9.0 * r * r, (b, i, j)
