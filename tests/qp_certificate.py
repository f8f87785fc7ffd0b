"""An optimality certificate for min ½xᵀPx + cᵀx s.t. Gx ≤ h that shares no code with either oracle.

`oracle/qp_gi.py::kkt_residual` takes its multipliers from `lstsq` on the active rows.  On a linearly dependent active set
the minimum-norm solution can be negative where a non-negative one exists (two copies of one row: lstsq splits the
multiplier evenly, but with a third dependent row it may put a negative share on one of them), so it cannot judge the
problems of tests/qp_cases.py.  Here the multipliers come from non-negative least squares: a residual of zero means a
λ ≥ 0 with Px + c + G_Aᵀλ = 0 exists, whatever the rank of G_A."""

import numpy as np
from scipy.optimize import nnls

ACTIVE_TOL = 1e-9        # normalised slack below which a row counts as active (the threshold kkt_residual uses)


def certificate(P, c, G, h, x):
    """→ (primal, active, stationarity).

    primal: max_i (G_i·x − h_i)/‖G_i‖ over finite rows of non-zero norm; a row of zeros counts as violated (by −h_i) iff h_i < 0.
    active: indices of the rows with (h_i − G_i·x)/‖G_i‖ ≤ 1e-9.
    stationarity: ‖P⁻¹(Px + c + G_Aᵀλ)‖∞ with λ = nnls(G_Aᵀ, −(Px + c)) — the displacement in x the residual stands for.
    (NNLS runs on rows of unit norm: the cone {G_Aᵀλ, λ ≥ 0} does not depend on the scale of a row, the conditioning does.)"""
    P, c, G, h, x = (np.asarray(a, dtype=np.float64) for a in (P, c, G, h, x))
    nrm = np.sqrt((G * G).sum(axis=1))
    fin = np.isfinite(h)
    live = fin & (nrm > 0.0)
    slack = np.full(len(h), np.inf)
    slack[live] = (h[live] - G[live] @ x) / nrm[live]
    primal = float(-slack[live].min()) if live.any() else -np.inf
    dead = fin & (nrm == 0.0) & (h < 0.0)
    if dead.any():
        primal = max(primal, float(-h[dead].min()))
    active = np.flatnonzero(slack <= ACTIVE_TOL)
    g = P @ x + c
    r = g
    if len(active):
        N = G[active] / nrm[active, None]
        lam, _ = nnls(N.T, -g, maxiter=50 * (len(active) + len(x)))
        r = g + N.T @ lam
    return primal, active, float(np.abs(np.linalg.solve(P, r)).max())
