"""The double trial iterate in front of tests/merit_ref.py::merit_at — TEST INFRASTRUCTURE, the checker of mpcg_compute_merit_f64
(mpcgpu_amd/csrc/merit_plant.hip.h).  merit_at takes the trial iterate itself; here it is the correctly rounded double fma(alpha, dz, xu), restated
per element in exact rational arithmetic rounded once (tests/rho_ref_f64.py::fma).  Goals and xs are used as the doubles they are: merit_at rounds
them to float32 first, so a caller of `merits` passes float32-representable goals and xs (the iterate and the step are genuinely double)."""
import numpy as np

import iiwa_ref
import merit_ref
from rho_ref_f64 import fma


def trial(xu, dz, alpha):
    """fma(alpha, dz, xu) in double with one rounding; alpha == 0 reads no dz."""
    xu = np.ascontiguousarray(xu, np.float64)
    if alpha == 0.0 or dz is None:
        return xu.copy()
    return fma(alpha, dz, xu)


def merits(model, xu, dz, step_sizes, goals, xs, N, mu, qd_cost, r_cost, dt=iiwa_ref.TIMESTEP):
    """[B, A] float64 merits of a batch at the double trial iterates: xu, dz [B, (n+m)N - m] float64, goals [B, N, 6], xs [B, n] or None."""
    B = len(xu)
    out = np.zeros((B, len(step_sizes)))
    for b in range(B):
        for a, alpha in enumerate(step_sizes):
            out[b, a] = merit_ref.merit_at(model, trial(xu[b], None if dz is None else dz[b], alpha), goals[b], None if xs is None else xs[b],
                                           N, mu, qd_cost, r_cost, dt)
    return out
