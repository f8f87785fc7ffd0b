"""Designed inputs for the in-wave QP: half-space rows that are duplicate, dependent, almost dependent,
contradictory or of zero norm.  Random Gaussian rows (tests/test_gpu_plugin.py) are in general position with probability
1, so they never reach the dependent-row test in front of a pivot, the t2 = ∞ branch, the arg-max tie or MKH_ST_DEGENERATE.

Every family is a function `family(nv, B, budget=None, scale=1.0)` → `(e, J, cost, G, h)`: a dense task of K rows
(`oracle/ik.py::DenseTaskSpec`: H = Σ cost²·JᵀJ + damping·I, c = Jᵀ(cost²·e): the task asks for J·Δq = −e) and a dense limit of M rows G·Δq ≤ h, for a
batch of B instances.  cond(H) is kept moderate — K = max(2, nv // 2) Gaussian rows, cost 1, DAMPING = 1e-2 — the
degeneracy sits in the constraints only.  With x0 = −H⁻¹c, `a` three Gaussian rows and b = a·x0 − U(0.1, 1) (x0 violates
them), the rows of each family are stated at its function.  Seeds and row counts are fixed here; `budget` is the number
of half-space rows the launch path under test can hold (a family that draws more is cut by its generator); `scale`
multiplies e and every offset — the QP is equivariant under it (x scales alike), it only places x against the robot's
joint-limit box, which is not part of these inputs."""

import numpy as np

from oracle import ik as oik

DAMPING = 1e-2
# How the families are placed against a robot's box (the built-in ConfigurationLimit and a loose VelocityLimit, as rows ±e_i
# in the reference): every model at the middle of its joint ranges, x of order SCALE, velocity box ±DT·VMAX = ±0.2.  The
# narrowest joint of the G1 leaves ±0.249, so the box binds in the tail of a family only, and never at the `vertex` point.
DT, VMAX, SCALE = 1e-2, 20.0, 0.05

SEEDS = {"duplicate": 101, "scaled": 102, "near_parallel_1e-4": 103, "near_parallel_1e-7": 104, "equality_pairs": 105,
         "vertex": 106, "zero_and_inf": 107, "combination": 108, "touching": 109, "infeasible": 110,
         "barely_feasible": 111, "single_entry": 112, "single_entry_contradict": 113}
# the pull of near_parallel (b = a·x0 − pull·U(0.1, 1)), see _near_parallel: tests/test_qp_cases_cpu.py records how many
# instances end with both rows of a pair active
NEAR_PARALLEL_PULL = 1.0


def objective(e, J, cost, damping=DAMPING):
    """(H, c) of one dense task for the whole batch, as oracle/ik.py::task_qp_objective states it (gain 1, no lm_damping)."""
    Jw = J * cost[None, :, None]
    H = np.einsum("bki,bkj->bij", Jw, Jw) + damping * np.eye(J.shape[-1])
    c = np.einsum("bki,bk->bi", Jw, cost[None, :] * e)               # (the task asks for J·Δq = −e: c = +Jᵀ(cost²·e))
    return H, c


class _Base:
    """The part every family shares: the task rows, x0 and the three violated Gaussian rows a·x ≤ b."""

    def __init__(self, name, nv, B, scale):
        self.rng = rng = np.random.default_rng(SEEDS[name])
        self.nv, self.B, self.scale = nv, B, scale
        K = max(2, nv // 2)
        self.J = rng.normal(size=(B, K, nv))
        self.e = scale * rng.normal(size=(B, K))
        self.cost = np.ones(K)
        self.H, self.c = objective(self.e, self.J, self.cost)
        self.x0 = np.linalg.solve(self.H, -self.c[..., None])[..., 0]
        self.a = rng.normal(size=(B, 3, nv))
        self.gap = scale * rng.uniform(0.1, 1.0, size=(B, 3))
        self.ax0 = np.einsum("bmi,bi->bm", self.a, self.x0)
        self.b = self.ax0 - self.gap

    def out(self, G, h):
        return self.e, self.J, self.cost, np.ascontiguousarray(G), np.ascontiguousarray(h)


def duplicate(nv, B, budget=None, scale=1.0):
    """[a; a; a[0]] ≤ [b; b; b[0]]: exactly equal rows — the second copy has a zero projected normal."""
    s = _Base("duplicate", nv, B, scale)
    return s.out(np.concatenate([s.a, s.a, s.a[:, :1]], axis=1), np.concatenate([s.b, s.b, s.b[:, :1]], axis=1))


def scaled(nv, B, budget=None, scale=1.0):
    """[a; 1e3·a; 1e-3·a], h scaled alike: the same half-spaces at norms six decades apart."""
    s = _Base("scaled", nv, B, scale)
    return s.out(np.concatenate([s.a, 1e3 * s.a, 1e-3 * s.a], axis=1), np.concatenate([s.b, 1e3 * s.b, 1e-3 * s.b], axis=1))


def _near_parallel(name, theta, nv, B, scale, on_intersection):
    """Rows [a; a + θ·p] ≤ [b; h₂].  Odd instances take h₂ as drawn: (a + θp)·x0 − (a·x0 − b) + 0.1·θ·N(0, 1).  There the
    two rows of a pair are never both active, whatever the pull: with s = a·H⁻¹·a, u = a·H⁻¹·p, w = p·H⁻¹·p both multipliers
    are positive only for an offset inside a window θ²·(a·x0 − b)·(w − u²/s)/s wide, and the noise is 0.1·θ wide (measured on
    the reference: 0 of 16 at θ = 1e-4).  So EVEN instances get the h₂ that puts the minimiser on the intersection.  Let A
    be the rows of a·x ≤ b that are active at the minimiser of that 3-row problem (found by trying the 7 subsets).  Each
    k ∈ A shares its multiplier with its twin — λ_k for a_k, ρ_k·λ_k for a_k + θ·p_k, ρ ~ U(0.2, 5) — with λ from
    a_k·x* = b_k at x* = x0 − H⁻¹·Σ_A (a_k + ρ_k·(a_k + θ·p_k))·λ_k, and h₂ = (a + θp)·x* on A.  `NEAR_PARALLEL_PULL`
    scales a·x0 − b in both kinds.
    Only at θ = 1e-4 (`on_intersection`): a minimiser on the intersection of two planes at angle θ moves by ε/θ when an
    offset moves by ε, so at θ = 1e-7 the rounding of h₂ alone (1e-17) is worth 1e-10 in x = 1e-8 in v, the whole tolerance
    the device is held to — the problem would be ill-posed by construction (tests/test_qp_cases_cpu.py holds every family to
    a sensitivity of 1 % of that tolerance).  At θ = 1e-7 every instance takes h₂ as drawn; the twins are then within 1e-9 of
    each other in normalised slack, which is what `active` means everywhere in this suite."""
    s = _Base(name, nv, B, scale)
    p = s.rng.normal(size=(B, 3, nv))
    gap = NEAR_PARALLEL_PULL * s.gap
    a2 = s.a + theta * p
    h2 = np.einsum("bmi,bi->bm", a2, s.x0) - gap + 0.1 * theta * scale * s.rng.normal(size=(B, 3))
    rho = s.rng.uniform(0.2, 5.0, size=(B, 3))
    for i in range(0, B, 2) if on_intersection else ():
        Hia = np.linalg.solve(s.H[i], s.a[i].T)                     # (nv, 3)
        for A in ([0], [1], [2], [0, 1], [0, 2], [1, 2], [0, 1, 2]):
            mu = np.linalg.solve(s.a[i][A] @ Hia[:, A], gap[i][A])
            rest = [k for k in range(3) if k not in A]
            if (mu > 0.0).all() and (s.a[i][rest] @ (Hia[:, A] @ mu) > gap[i][rest]).all():
                break                                               # the KKT set of the 3-row problem (it is unique)
        D = s.a[i][A] + rho[i][A][:, None] * a2[i][A]               # Σ_A D_k·λ_k: the pull of the pairs in A
        HiD = np.linalg.solve(s.H[i], D.T)
        lam = np.linalg.solve(s.a[i][A] @ HiD, gap[i][A])
        if (lam > 0.0).all():
            h2[i][A] = a2[i][A] @ (s.x0[i] - HiD @ lam)
    return s.out(np.concatenate([s.a, a2], axis=1), np.concatenate([s.ax0 - gap, h2], axis=1))


def near_parallel_1e4(nv, B, budget=None, scale=1.0):
    """[a; a + θ·p], θ = 1e-4, h₂ = (a + θp)·x0 − (a·x0 − b) + 0.1·θ·N(0, 1): almost dependent active rows (§4.4)."""
    return _near_parallel("near_parallel_1e-4", 1e-4, nv, B, scale, True)


def near_parallel_1e7(nv, B, budget=None, scale=1.0):
    """The same at θ = 1e-7, every h₂ as drawn (see _near_parallel)."""
    return _near_parallel("near_parallel_1e-7", 1e-7, nv, B, scale, False)


def equality_pairs(nv, B, budget=None, scale=1.0):
    """[a[:2]; −a[:2]; a[2]] ≤ [b[:2]; −b[:2]; b[2]]: slabs of zero width, two opposing rows active at once."""
    s = _Base("equality_pairs", nv, B, scale)
    return s.out(np.concatenate([s.a[:, :2], -s.a[:, :2], s.a[:, 2:]], axis=1),
                 np.concatenate([s.b[:, :2], -s.b[:, :2], s.b[:, 2:]], axis=1))


def vertex(nv, B, budget=None, scale=1.0):
    """nv + 4 Gaussian rows through one point x_s = x0 + 0.5·N(0, I), h = G·x_s, each row signed so that x_s is the
    minimiser: more rows active at the optimum than there are dofs.  Cut to `budget` rows when the path holds fewer (then
    M ≤ nv, the rows are signed by the multipliers of the equality-constrained problem, and every row is active)."""
    s = _Base("vertex", nv, B, scale)
    M = nv + 4 if budget is None else min(nv + 4, budget)
    xs = s.x0 + 0.5 * scale * s.rng.normal(size=(B, nv))
    G = s.rng.normal(size=(B, M, nv))
    for i in range(B):
        g = s.H[i] @ xs[i] + s.c[i]                                  # gradient at x_s: −g = Gᵀλ with λ > 0 is wanted
        if M > nv:
            mu = np.linalg.lstsq(G[i].T, -g, rcond=None)[0]          # (minimum norm: every entry nonzero almost surely)
        else:
            HiGt = np.linalg.solve(s.H[i], G[i].T)
            mu = np.linalg.solve(G[i] @ HiGt, -(G[i] @ np.linalg.solve(s.H[i], g)))
        G[i] *= np.where(mu < 0.0, -1.0, 1.0)[:, None]
    return s.out(G, np.einsum("bmi,bi->bm", G, xs))


def zero_and_inf(nv, B, budget=None, scale=1.0):
    """[a; 0ᵀ; two Gaussian rows] ≤ [b; 0; +inf; +inf]: a row of zeros with h = 0, inactive rows between live ones."""
    s = _Base("zero_and_inf", nv, B, scale)
    g2 = s.rng.normal(size=(B, 2, nv))
    G = np.concatenate([s.a[:, :1], np.zeros((B, 1, nv)), g2[:, :1], s.a[:, 1:2], g2[:, 1:], s.a[:, 2:]], axis=1)
    inf = np.full((B, 1), np.inf)
    h = np.concatenate([s.b[:, :1], np.zeros((B, 1)), inf, s.b[:, 1:2], inf, s.b[:, 2:]], axis=1)
    return s.out(G, h)


def combination(nv, B, budget=None, scale=1.0):
    """[a[0]; a[1]; a[0] + a[1]] ≤ [b₀; b₁; b₀ + b₁]: a row that is exactly the sum of two active ones."""
    s = _Base("combination", nv, B, scale)
    return s.out(np.concatenate([s.a[:, :2], s.a[:, :1] + s.a[:, 1:2]], axis=1),
                 np.concatenate([s.b[:, :2], s.b[:, :1] + s.b[:, 1:2]], axis=1))


def touching(nv, B, budget=None, scale=1.0):
    """a ≤ a·x0 exactly: zero violation at the unconstrained minimiser (a tie at the first arg-max)."""
    s = _Base("touching", nv, B, scale)
    return s.out(s.a, s.ax0.copy())


def _slab(name, w, nv, B, scale):
    s = _Base(name, nv, B, scale)
    return s.out(np.concatenate([s.a[:, :1], -s.a[:, :1]], axis=1), np.concatenate([s.b[:, :1], -s.b[:, :1] - w * scale], axis=1))


def infeasible(nv, B, budget=None, scale=1.0):
    """[a[0]; −a[0]] ≤ [b₀; −b₀ − 1e-3]: a slab of negative width, to be reported."""
    return _slab("infeasible", 1e-3, nv, B, scale)


def barely_feasible(nv, B, budget=None, scale=1.0):
    """[a[0]; −a[0]] ≤ [b₀; −b₀ + 1e-6]: a slab 1e-6 wide, to be solved."""
    return _slab("barely_feasible", -1e-6, nv, B, scale)


def single_entry_dofs(nv):
    """(limited dofs, pinned dof, contradicted dof) of the single_entry families — the same columns in every instance,
    which is what makes a row single-entry for the host (mink_amd/solve_ik.py::_fold_box_rows looks at the whole batch)."""
    return [0, nv // 3, (2 * nv) // 3], nv - 1, 1


def _single_entry(name, contradict, nv, B, scale):
    s = _Base(name, nv, B, scale)
    lim, pin, bad = single_entry_dofs(nv)
    I = np.eye(nv)
    u = s.x0 - scale * s.rng.uniform(0.1, 1.0, size=(B, nv))         # below x0: every bound binds unless the box is tighter
    rows, hs = [], []
    for d in lim:                                                   # the same bound twice, at different scale
        rows += [2.0 * I[d], I[d]]; hs += [2.0 * u[:, d], u[:, d]]
    rows += [I[pin], -I[pin]]; hs += [u[:, pin], -u[:, pin]]         # Δq_pin = u
    rows += [np.zeros(nv)]; hs += [np.zeros(B)]                     # 0ᵀ·Δq ≤ 0
    if contradict:
        w = scale * s.rng.uniform(0.1, 1.0, size=B)
        rows += [I[bad], -I[bad]]; hs += [-w, -w]                    # Δq_bad ≤ −w and Δq_bad ≥ w
    G = np.broadcast_to(np.array(rows), (B, len(rows), nv))
    return s.out(G, np.stack(hs, axis=1))


def single_entry(nv, B, budget=None, scale=1.0):
    """Rows ±e_i: three dofs bounded twice at different scale (2·e_i ≤ 2·u, e_i ≤ u), one dof pinned (e_i ≤ u, −e_i ≤ −u),
    one row of zeros — what the host folds into MkhDenseRows.limit_lo / limit_hi.  Public-API route only."""
    return _single_entry("single_entry", False, nv, B, scale)


def single_entry_contradict(nv, B, budget=None, scale=1.0):
    """single_entry plus e_j ≤ −w, −e_j ≤ −w on one dof: folded rows that contradict each other, to be reported."""
    return _single_entry("single_entry_contradict", True, nv, B, scale)


FAMILIES = {"duplicate": duplicate, "scaled": scaled, "near_parallel_1e-4": near_parallel_1e4,
            "near_parallel_1e-7": near_parallel_1e7, "equality_pairs": equality_pairs, "vertex": vertex,
            "zero_and_inf": zero_and_inf, "combination": combination, "touching": touching, "infeasible": infeasible,
            "barely_feasible": barely_feasible, "single_entry": single_entry,
            "single_entry_contradict": single_entry_contradict}
INFEASIBLE = ("infeasible", "single_entry_contradict")
SINGLE_ENTRY = ("single_entry", "single_entry_contradict")
GENERAL = tuple(n for n in FAMILIES if n not in SINGLE_ENTRY)


def pad_rows(name, G, h, e, J, cost, M, scale=1.0):
    """Pad a family with Gaussian rows that are slack at x0 (h = g·x0 + scale·U(0, 1)) up to M rows: on a path that
    keeps only the tightest rows of an instance, the ones the solution then violates send it to the all-rows redo."""
    B, m, nv = G.shape
    rng = np.random.default_rng(SEEDS[name] + 1000)
    H, c = objective(e, J, cost)
    x0 = np.linalg.solve(H, -c[..., None])[..., 0]
    g = rng.normal(size=(B, M - m, nv))
    hg = np.einsum("bmi,bi->bm", g, x0) + scale * rng.uniform(0.0, 1.0, size=(B, M - m))
    return np.concatenate([G, g], axis=1), np.concatenate([h, hg], axis=1)


def mid_range_q(model):
    """qpos0 with every limited hinge / slide joint at the middle of its range (a free joint stays at the origin)."""
    q = np.array(model.qpos0, dtype=np.float64)
    for j in range(model.njnt):
        if model.jnt_type[j] in (2, 3) and model.jnt_limited[j]:
            q[int(model.jnt_qposadr[j])] = 0.5 * (model.jnt_range[j][0] + model.jnt_range[j][1])
    return q


def box_limit_specs(model, vmax=VMAX):
    """The built-in part of every problem: ConfigurationLimit plus a loose VelocityLimit on every hinge / slide dof."""
    idx = np.array([int(model.jnt_dofadr[j]) for j in range(model.njnt) if model.jnt_type[j] != 0])
    return [oik.ConfigurationLimitSpec(), oik.VelocityLimitSpec(idx, np.full(len(idx), vmax))]


def stacked_qp(cfg, case, i, dt=DT, vmax=VMAX, damping=DAMPING):
    """(P, c, G, h) of instance i as the reference stacks it (oracle/ik.py::build_ik): the box as rows ±e_i, then the family."""
    e, J, cost, G, h = case
    return oik.build_ik(cfg, [oik.DenseTaskSpec(e[i], J[i], cost)], dt, damping,
                        box_limit_specs(cfg.model, vmax) + [oik.DenseLimitSpec(G[i], h[i])])
