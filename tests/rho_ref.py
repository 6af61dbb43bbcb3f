"""numpy restatement of the rho adaptation behind the SQP line search (reference include/pcg/sqp.cuh:304-320; the host twin is
mpcgpu_compat::use_mpcg_line_search, include/mpcgpu_compat/sqp_stages.cuh:127-134) — TEST INFRASTRUCTURE, the checker of
mpcg_line_search_step_rho and mpcg_line_search_step_rho_f64 (mpcgpu_amd/csrc/merit_plant.hip.h).  Every operation is one operation of dtype
(np.float32 or np.float64): one rounding each, no contraction, correctly rounded divisions.

    p < 0  (no step):  drho = max(drho * f, f);      rho = max(rho * drho, rho_min);   rho > rho_max: rho = rho_reset, done = 1
    p >= 0 (a step):   drho = min(drho / f, 1 / f);  rho = max(rho * drho, rho_min)

The reference's constants: f = 1.2, rho_min = 1e-3, rho_max = 10.  The update of the iterate is xu + alpha dz rounded once: in float32 the plain
numpy expression, for step sizes that are powers of two (the product alpha * dz is then exact, as in the fused update); in float64 the correctly
rounded fused multiply-add, restated in exact rational arithmetic (fma), so the step sizes need not be powers of two."""
from fractions import Fraction

import numpy as np

FACTOR, RHO_MIN, RHO_MAX = 1.2, 1e-3, 10.0
STEP_FROZEN = -2                       # MPCG_STEP_FROZEN


def fma(a, d, x):
    """fma(a, d, x) in double, elementwise over d and x: Fraction arithmetic is exact and float() of a Fraction rounds once, to nearest even.
    Non-finite operands go through numpy (a NaN or an infinity has no Fraction; nothing is left to round)."""
    f64 = np.float64
    d, x = np.asarray(d, f64), np.asarray(x, f64)
    out = np.empty(x.shape, f64)
    fa = Fraction(float(a))
    for i in np.ndindex(x.shape):
        if np.isfinite(d[i]) and np.isfinite(x[i]):
            out[i] = float(fa * Fraction(float(d[i])) + Fraction(float(x[i])))
        else:
            out[i] = f64(a) * d[i] + x[i]
    return out


def update(rho, drho, p, factor=FACTOR, rho_min=RHO_MIN, rho_max=RHO_MAX, rho_reset=RHO_MIN, dtype=np.float32):
    """One trajectory, one line search with outcome p (< 0: failed): (rho, drho, done) as dtype, dtype, bool."""
    t = np.dtype(dtype).type
    rho, drho, f, lo, hi = t(rho), t(drho), t(factor), t(rho_min), t(rho_max)
    if p < 0:
        drho = max(t(drho * f), f)
        rho = max(t(rho * drho), lo)
        if rho > hi:
            return t(rho_reset), drho, True
        return rho, drho, False
    drho = min(t(drho / f), t(t(1.0) / f))
    rho = max(t(rho * drho), lo)
    return rho, drho, False


def step(merit, step_sizes, merit_ref, dz, xu, rho=None, drho=None, done=None, factor=FACTOR, rho_min=RHO_MIN, rho_max=RHO_MAX, rho_reset=RHO_MIN,
         dtype=np.float32):
    """mpcg_line_search_step_rho(_f64) on host arrays, in place (rho = drho = done = None: the plain mpcg_line_search_step(_f64)): merit [B, A],
    merit_ref, rho, drho dtype [B], done uint8 [B], dz, xu dtype [B, L].  Returns the step codes (int32 [B])."""
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
            if np.dtype(dtype) == np.float32:
                xu[b] = (xu[b] + np.float32(step_sizes[p]) * dz[b]).astype(np.float32)
            else:
                xu[b] = fma(step_sizes[p], dz[b], xu[b])
        if rho is not None:
            rho[b], drho[b], gave_up = update(rho[b], drho[b], p, factor, rho_min, rho_max, rho_reset, dtype)
            if gave_up:
                done[b] = 1
    return out
