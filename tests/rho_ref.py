"""numpy-float32 restatement of the rho adaptation behind the SQP line search (reference include/pcg/sqp.cuh:304-320; the host twin is
mpcgpu_compat::use_mpcg_line_search, include/mpcgpu_compat/sqp_stages.cuh:127-134) — TEST INFRASTRUCTURE, the checker of
mpcg_line_search_step_rho (mpcgpu_amd/csrc/merit_plant.hip.h).  Every operation is one np.float32 operation: one rounding each, no
contraction, correctly rounded divisions.

    p < 0  (no step):  drho = max(drho * f, f);      rho = max(rho * drho, rho_min);   rho > rho_max: rho = rho_reset, done = 1
    p >= 0 (a step):   drho = min(drho / f, 1 / f);  rho = max(rho * drho, rho_min)

The reference's constants: f = 1.2, rho_min = 1e-3, rho_max = 10."""
import numpy as np

FACTOR, RHO_MIN, RHO_MAX = 1.2, 1e-3, 10.0
STEP_FROZEN = -2                       # MPCG_STEP_FROZEN


def update(rho, drho, p, factor=FACTOR, rho_min=RHO_MIN, rho_max=RHO_MAX, rho_reset=RHO_MIN):
    """One trajectory, one line search with outcome p (< 0: failed): (rho, drho, done) as np.float32, np.float32, bool."""
    f32 = np.float32
    rho, drho, f, lo, hi = f32(rho), f32(drho), f32(factor), f32(rho_min), f32(rho_max)
    if p < 0:
        drho = max(f32(drho * f), f)
        rho = max(f32(rho * drho), lo)
        if rho > hi:
            return f32(rho_reset), drho, True
        return rho, drho, False
    drho = min(f32(drho / f), f32(f32(1.0) / f))
    rho = max(f32(rho * drho), lo)
    return rho, drho, False


def step(merit, step_sizes, merit_ref, dz, xu, rho, drho, done, factor=FACTOR, rho_min=RHO_MIN, rho_max=RHO_MAX, rho_reset=RHO_MIN):
    """mpcg_line_search_step_rho on host arrays, in place: merit [B, A], merit_ref, rho, drho float32 [B], done uint8 [B], dz, xu float32 [B, L].
    Returns the step codes (int32 [B]).  The step sizes must be powers of two (the product alpha * dz is then exact, as in the fused update)."""
    B = len(merit_ref)
    out = np.empty(B, np.int32)
    for b in range(B):
        if done[b] != 0:
            out[b] = STEP_FROZEN
            continue
        best, p = merit_ref[b], -1
        for i, v in enumerate(merit[b]):
            if v < best:
                best, p = v, i
        out[b] = p
        if p >= 0:
            merit_ref[b] = best
            xu[b] = (xu[b] + np.float32(step_sizes[p]) * dz[b]).astype(np.float32)
        rho[b], drho[b], gave_up = update(rho[b], drho[b], p, factor, rho_min, rho_max, rho_reset)
        if gave_up:
            done[b] = 1
    return out
