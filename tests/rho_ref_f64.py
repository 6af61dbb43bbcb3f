"""numpy-float64 restatement of the rho adaptation behind the SQP line search: the rule of tests/rho_ref.py (reference include/pcg/sqp.cuh:304-320)
with every operation one np.float64 operation — one rounding each, no contraction, correctly rounded divisions — TEST INFRASTRUCTURE, the checker of
mpcg_line_search_step_rho_f64 (mpcgpu_amd/csrc/merit_plant.hip.h).  The update of the iterate is the correctly rounded fused multiply-add, restated in
exact rational arithmetic rounded once (fma), so the step sizes need not be powers of two.

    p < 0  (no step):  drho = max(drho * f, f);      rho = max(rho * drho, rho_min);   rho > rho_max: rho = rho_reset, done = 1
    p >= 0 (a step):   drho = min(drho / f, 1 / f);  rho = max(rho * drho, rho_min)"""
from fractions import Fraction

import numpy as np

from rho_ref import FACTOR, RHO_MAX, RHO_MIN, STEP_FROZEN

f64 = np.float64


def fma(a, d, x):
    """fma(a, d, x) in double, elementwise over d and x: Fraction arithmetic is exact and float() of a Fraction rounds once, to nearest even.
    Non-finite operands go through numpy (a NaN or an infinity has no Fraction; nothing is left to round)."""
    d, x = np.asarray(d, f64), np.asarray(x, f64)
    out = np.empty(x.shape, f64)
    fa = Fraction(float(a))
    for i in np.ndindex(x.shape):
        if np.isfinite(d[i]) and np.isfinite(x[i]):
            out[i] = float(fa * Fraction(float(d[i])) + Fraction(float(x[i])))
        else:
            out[i] = f64(a) * d[i] + x[i]
    return out


def update(rho, drho, p, factor=FACTOR, rho_min=RHO_MIN, rho_max=RHO_MAX, rho_reset=RHO_MIN):
    """One trajectory, one line search with outcome p (< 0: failed): (rho, drho, done) as np.float64, np.float64, bool."""
    rho, drho, f, lo, hi = f64(rho), f64(drho), f64(factor), f64(rho_min), f64(rho_max)
    if p < 0:
        drho = max(f64(drho * f), f)
        rho = max(f64(rho * drho), lo)
        if rho > hi:
            return f64(rho_reset), drho, True
        return rho, drho, False
    drho = min(f64(drho / f), f64(f64(1.0) / f))
    rho = max(f64(rho * drho), lo)
    return rho, drho, False


def step(merit, step_sizes, merit_ref, dz, xu, rho=None, drho=None, done=None, factor=FACTOR, rho_min=RHO_MIN, rho_max=RHO_MAX, rho_reset=RHO_MIN):
    """mpcg_line_search_step_rho_f64 on host arrays, in place (rho = drho = done = None: mpcg_line_search_step_f64): merit [B, A], merit_ref, rho, drho
    float64 [B], done uint8 [B], dz, xu float64 [B, L].  Returns the step codes (int32 [B])."""
    B = len(merit_ref)
    out = np.empty(B, np.int32)
    for b in range(B):
        if done is not None and done[b] != 0:
            out[b] = STEP_FROZEN
            continue
        best, p = merit_ref[b], -1
        for i, v in enumerate(merit[b]):
            if v < best:
                best, p = v, i
        out[b] = p
        if p >= 0:
            merit_ref[b] = best
            xu[b] = fma(step_sizes[p], dz[b], xu[b])
        if rho is not None:
            rho[b], drho[b], gave_up = update(rho[b], drho[b], p, factor, rho_min, rho_max, rho_reset)
            if gave_up:
                done[b] = 1
    return out
