"""numpy restatement of THE RULE "with a certifying checker" (include/minkhip.h, mkh_ladder_select_certified), by composition
only: the gating of ladder_free_ref.margins (node margins, effective flags, which edges are swept at all),
certified_ref.certified_sweep on the gated edge list, and ladder_free_ref.search on the mask the policy makes of the verdicts.
Nothing here restates a rule of its own."""

import numpy as np

import certified_ref as cf
import ladder_free_ref as lfref
import ladder_ref as lref

REJECT_COLLIDING, REQUIRE_CERTIFIED = 0, 1


def stage(model, limits, q_nodes, tracked_nodes, resolution, max_samples=64):
    """The stage in front of the search on (B, T, S, nq) nodes, the same for both policies: a dict of node_margin and the effective
    flags `tracked` (B, T, S), and per edge [b, t, s', s] (B, T, S, S): `swept`, edge_margin_all and edge_lower_bound_all (NaN
    where not swept), edge_n_samples_all (0), edge_verdict_all (int8, -1), edge_motion_all (NaN)."""
    q_nodes = np.asarray(q_nodes, dtype=np.float64)
    B, T, S, nq = q_nodes.shape
    # (the gating is ladder_free_ref.margins': one interior sample per edge is the cheapest way to ask it)
    node_margin, eff, _ = lfref.margins(model, limits, q_nodes, tracked_nodes, 1)
    swept = np.zeros((B, T, S, S), dtype=bool)
    swept[:, 1:] = eff[:, 1:, :, None]
    out = dict(node_margin=node_margin, tracked=eff, swept=swept,
               edge_margin_all=np.full((B, T, S, S), np.nan), edge_lower_bound_all=np.full((B, T, S, S), np.nan),
               edge_motion_all=np.full((B, T, S, S), np.nan), edge_n_samples_all=np.zeros((B, T, S, S), np.int32),
               edge_verdict_all=np.full((B, T, S, S), -1, np.int8))
    idx = np.argwhere(swept)                                    # (row-major: b, t, s', s)
    if len(idx):
        a = np.stack([q_nodes[b, t - 1, s] for b, t, s1, s in idx])
        c = np.stack([q_nodes[b, t, s1] for b, t, s1, s in idx])
        cs = cf.certified_sweep(model, limits, a, c, resolution, max_samples)
        at = tuple(idx.T)
        out["edge_margin_all"][at], out["edge_lower_bound_all"][at], out["edge_motion_all"][at] = cs.margin, cs.lower_bound, cs.motion
        out["edge_n_samples_all"][at], out["edge_verdict_all"][at] = cs.n_samples, cs.verdict
    return out


def blocked_mask(st, policy):
    v = st["edge_verdict_all"]
    if policy == REJECT_COLLIDING:
        return st["swept"] & (v == cf.COLLIDES)
    if policy == REQUIRE_CERTIFIED:
        return st["swept"] & (v != cf.CERTIFIED)
    raise ValueError(f"edge_policy = {policy}")


def select(model, q, q_nodes, st, policy, weights=None, max_step_sq=np.inf, search=lfref.search):
    """mkh_ladder_select_certified on host arrays behind stage(): ladder_ref.select's dict, MkhLadderFreeIO's and
    MkhLadderCertifiedIO's outputs, the mask as `blocked`.  `search`: ladder_free_ref.search, or its brute_force."""
    q_nodes = np.asarray(q_nodes, dtype=np.float64)
    B, T, S, nq = q_nodes.shape
    eff, blocked = st["tracked"], blocked_mask(st, policy)
    out = dict(st, blocked=blocked, node_index=np.zeros((B, T), np.int32), n_tracked=np.zeros(B, np.int32), n_breaks=np.zeros(B, np.int32),
               path_length=np.zeros(B), edge_break=np.zeros((B, T), np.int32), q_path=np.zeros((B, T, nq)),
               edge_collision=np.zeros((B, T), np.int32), n_edge_collisions=np.zeros(B, np.int32),
               edge_margin=np.full((B, T), np.nan), edge_lower_bound=np.full((B, T), np.nan),
               edge_n_samples=np.zeros((B, T), np.int32), edge_verdict=np.full((B, T), -1, np.int32), n_certified=np.zeros(B, np.int32))
    for b in range(B):
        start, edges = lref.costs(model, q[b], q_nodes[b], weights)
        path, key, brk, col = search(start, edges, ~eff[b], blocked[b], max_step_sq)
        out["node_index"][b], out["edge_break"][b], out["edge_collision"][b] = path, brk, col
        out["n_tracked"][b], out["n_breaks"][b], out["path_length"][b] = T - key[0], key[1], key[2]
        out["n_edge_collisions"][b] = col.sum()
        out["q_path"][b] = q_nodes[b, np.arange(T), path]
        out["edge_margin"][b, 0] = out["edge_lower_bound"][b, 0] = np.inf
        for t in range(1, T):
            e = (b, t, path[t], path[t - 1])
            out["edge_margin"][b, t], out["edge_lower_bound"][b, t] = st["edge_margin_all"][e], st["edge_lower_bound_all"][e]
            out["edge_n_samples"][b, t], out["edge_verdict"][b, t] = st["edge_n_samples_all"][e], st["edge_verdict_all"][e]
        out["n_certified"][b] = (out["edge_verdict"][b, 1:] == cf.CERTIFIED).sum()
    return out
