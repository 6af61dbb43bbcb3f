"""GPU: mpcg_riccati_gains(_f64) with G past 2^32 bytes — tests/large_extents.py: D distinct trajectories tiled over the batch on the device,
every tile of K bit for bit the call on the distinct ones, no element of K left at the prefill, G, C and rho intact; and the call on the
distinct ones against the restatement tests/riccati_ref.py at the bound of tests/test_gpu_riccati.py.

Sizes: 14 x 7 at three knots, 686 elements of G per trajectory; float B = 1,565,222, double B = 782,611, G, C, K and rho
together 9.2 GB.  rho is the device vector, D distinct values: rho_v[b] is indexed with the batch as well."""
import numpy as np
import pytest
import torch

import large_extents as le
import riccati_ref as rr
from test_gpu_riccati import check_against_reference, reference

pytestmark = pytest.mark.gpu
RHOS = [1e-3, 0.5, 10.0, 3e-2, 1.7]                     # (tests/test_gpu_rho.py's: one rho per trajectory)
TORCH = {"f32": torch.float32, "f64": torch.float64}
SPECS = le.riccati_specs()


@pytest.mark.parametrize("spec", SPECS, ids=[s.label for s in SPECS])
def test_riccati_gains_past_2_32(spec):
    from mpcgpu_amd import PcgSolver
    prec = spec.label.split()[1]
    n, m, N, D, dt = le.n14, le.m7, le.RICCATI_N, spec.D, le.A.DT[prec]
    G, Cd = rr.make_case(n, m, N, D, dt)
    rho = np.array(RHOS[:D], dt)
    assert le.nbytes(spec.arrays[0], spec.B) > 2 ** 32 >= le.nbytes(spec.arrays[0], spec.B - 8)
    sol = PcgSolver(N, max_batch=spec.B)
    out = le.run(spec, {"G": G, "C": Cd, "rho": rho.reshape(D, 1)},
                 lambda a, Bt: sol.riccati_gains(a["G"], a["C"], a["rho"].view(-1), K=a["K"]))
    sol.close()
    e_ref, K64 = reference(("large", prec), G, Cd, n, m, N, rho.astype(np.float64))
    check_against_reference(out["K"], e_ref, K64, TORCH[prec], spec.label)
