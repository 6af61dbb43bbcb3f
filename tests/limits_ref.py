"""Float64 restatement of the soft-limits penalty a plant with limits adds to the generalised running cost (include/mpcg.h, LIMITS; mpcg_plant_clone_limits,
mpcg_generate_kkt_xuref / mpcg_compute_merit_xuref given such a plant) — TEST INFRASTRUCTURE, written from the formulas, on top of tests/xuref_ref.py:

    viol(x; lo, hi) = x > hi ? x - hi : (x < lo ? x - lo : 0)                          strict comparisons: a value on a bound and a NaN violate nothing
    J_k += 1/2 q_weight sum_i viol(q_i)^2 + 1/2 qd_weight sum_i viol(qd_i)^2 + [k < N-1] 1/2 u_weight sum_i viol(u_i)^2

The KKT blocks gain the Gauss-Newton terms: w [viol != 0] on the diagonals of Q_k and R_k, w viol in q_k and r_k, the last block at x_{N-1}.  C and c
do not change.  The merit gains the sum above, every knot at its own state."""
from dataclasses import dataclass, field

import numpy as np

import merit_ref
import merit_ref_f64
import xuref_ref as X

NJ, n, m, ROW = X.NJ, X.n, X.m, X.ROW


def _seven(v, default):
    a = np.full(NJ, default, np.float64) if v is None else np.broadcast_to(np.asarray(v, np.float64), (NJ,)).copy()
    a.setflags(write=False)
    return a


@dataclass(frozen=True)
class Limits:
    """Bounds per joint ([7] each; None: no bound on that side) and one weight per kind."""
    q_lo: np.ndarray = None
    q_hi: np.ndarray = None
    qd_lo: np.ndarray = None
    qd_hi: np.ndarray = None
    u_lo: np.ndarray = None
    u_hi: np.ndarray = None
    q_weight: float = 0.0
    qd_weight: float = 0.0
    u_weight: float = 0.0

    def __post_init__(self):
        for name in ("q", "qd", "u"):
            object.__setattr__(self, name + "_lo", _seven(getattr(self, name + "_lo"), -np.inf))
            object.__setattr__(self, name + "_hi", _seven(getattr(self, name + "_hi"), np.inf))

    @property
    def x_lo(self):
        return np.concatenate([self.q_lo, self.qd_lo])

    @property
    def x_hi(self):
        return np.concatenate([self.q_hi, self.qd_hi])

    @property
    def x_weight(self):
        return np.concatenate([np.full(NJ, self.q_weight), np.full(NJ, self.qd_weight)])

    def rounded_to_float(self):
        """The limits the float builds ("kkt_f32", "merit_f32") use: bounds and weights rounded to float."""
        f = lambda a: np.asarray(a, np.float32).astype(np.float64)
        return Limits(f(self.q_lo), f(self.q_hi), f(self.qd_lo), f(self.qd_hi), f(self.u_lo), f(self.u_hi), float(np.float32(self.q_weight)),
                      float(np.float32(self.qd_weight)), float(np.float32(self.u_weight)))


def viol(x, lo, hi):
    """viol(x; lo, hi), elementwise; strict comparisons (NaN -> 0)."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x > hi, x - hi, np.where(x < lo, x - lo, 0.0))


def side(x, lo, hi):
    """-1 below, 0 inside (or on a bound), +1 above."""
    x = np.asarray(x, np.float64)
    return np.where(x > hi, 1, np.where(x < lo, -1, 0))


def penalty(z, N, lim):
    """sum_k of the limits terms of J_k at the iterate z of one trajectory."""
    x, u = X.split(z, N)
    vx = viol(x, lim.x_lo, lim.x_hi)
    total = 0.5 * (lim.x_weight * vx * vx).sum()
    if N > 1:
        vu = viol(u, lim.u_lo, lim.u_hi)
        total += 0.5 * lim.u_weight * (vu * vu).sum()
    return total


def generate_kkt(model, xu, goals, xs, N, rows, cost, lim, dt=X.iiwa_ref.TIMESTEP, integrator=0, base=None):
    """xuref_ref.generate_kkt's (G, C, g, c) of ONE trajectory plus the limits terms."""
    G, C, g, c = X.generate_kkt(model, xu, goals, xs, N, rows, cost, dt, integrator, base)
    G, g = G.copy(), g.copy()
    x, u = X.split(xu, N)
    gq, gr = n * n + m * m, np.arange(n) * (n + 1)
    for k in range(N):
        vx = viol(x[k], lim.x_lo, lim.x_hi)
        G[gq * k + gr] += lim.x_weight * (vx != 0)
        g[ROW * k:ROW * k + n] += lim.x_weight * vx
        if k < N - 1:
            vu = viol(u[k], lim.u_lo, lim.u_hi)
            G[gq * k + n * n + np.arange(m) * (m + 1)] += lim.u_weight * (vu != 0)
            g[ROW * k + n:ROW * (k + 1)] += lim.u_weight * vu
    return G, C, g, c


def merit_at(model, z, goals, xs, N, mu, rows, cost, lim, dt=X.iiwa_ref.TIMESTEP, integrator=0):
    return X.merit_at(model, z, goals, xs, N, mu, rows, cost, dt, integrator) + penalty(z, N, lim)


def merits(model, xu, dz, step_sizes, goals, xs, N, mu, rows_of, cost, lim, dt=X.iiwa_ref.TIMESTEP, integrator=0, double=False, base=None):
    """[B, A] float64 merits.  base: xuref_ref.merits of the same arguments, if the caller has it (the penalty is added to it)."""
    trial = merit_ref_f64.trial if double else merit_ref.trial
    out = np.array(base, np.float64) if base is not None else X.merits(model, xu, dz, step_sizes, goals, xs, N, mu, rows_of, cost, dt, integrator, double)
    for b in range(len(xu)):
        for a, alpha in enumerate(step_sizes):
            out[b, a] += penalty(trial(xu[b], None if dz is None else dz[b], alpha), N, lim)
    return out
