"""CPU: the double-precision block-tridiagonal direct solve — the library exports mpcg_block_solve_f64, and its yardstick (the oracle's
block LU sweep, which dispatches on the dtype of S) is as accurate as the GPU tests assume: in float64 it is at rounding level of the
float64 direct solve, and with float data widened, swept in double and rounded once it is at the rounding of the float output."""
import numpy as np
import pytest

from mpcgpu_amd import _lib, synth
from test_generic_producers_cpu import make_kkt_nm
from util import relinf

RHO = 1e-3
# relative to max |x|.  Double: measured <= 8.9e-15 at the generic shapes and 3.1e-11 at n = 14, N = 33 and 128 (cond ~1e5 x the 1.1e-16 of a
# double, times what a pivot-free sweep loses); the limit is a decade of a double's 16 digits above cond x epsilon.  Float in, double inside,
# float out: measured 3.5e-8 ... 4.1e-8 — half an ulp of float is 6e-8: the rounding of the output.
LIMIT_F64 = 1e-10
LIMIT_F32_IO = 1e-6


def test_the_library_declares_and_exports_the_entry(hiplib):
    assert "mpcg_block_solve_f64" in _lib.SYMBOLS
    assert hasattr(hiplib, "mpcg_block_solve_f64")
    assert _lib.SYMBOLS["mpcg_block_solve_f64"] == _lib.SYMBOLS["mpcg_block_solve"]      # the same argument list, pointers to double


@pytest.mark.parametrize("N", [2, 33, 128])
def test_oracle_double_sweep_vs_direct_solve_n14(orc, N):
    k = synth.make_kkt(N, 1, 6228)
    S, _, g = synth.form_schur(k, rho=RHO, dtype=np.float64)
    err = relinf(orc.block_solve(S[0], g[0], N), orc.direct_solve(S[0], g[0], N))
    print(N, err)
    assert err <= LIMIT_F64


@pytest.mark.parametrize("N", [2, 9])
@pytest.mark.parametrize("n", [1, 4, 13, 17, 40, 64])
def test_oracle_double_sweep_vs_direct_solve_at_any_state_size(orc, n, N):
    m = max(1, n // 3)
    k = make_kkt_nm(N, 1, 40 + N, n, m)
    G, C, g, c = synth.pack_kkt_dense(k, np.float64)
    S, _, gam, _ = orc.form_schur(G[0], C[0], g[0], c[0], N, np.float64(RHO), ss=False, n=n, m=m)
    assert S.dtype == np.float64
    err = relinf(orc.block_solve(S, gam, N, n=n), orc.direct_solve(S, gam, N, n=n))
    print(n, N, err)
    assert err <= LIMIT_F64


@pytest.mark.parametrize("N", [2, 33, 128])
def test_oracle_float_data_swept_in_double_and_rounded_vs_direct_solve(orc, N):
    """What "block_solve_f64" = 1 computes: float S / gamma widened (exact), the sweep in double, lambda rounded to float once."""
    k = synth.make_kkt(N, 1, 6228)
    S, _, g = synth.form_schur(k, rho=RHO)
    assert S.dtype == np.float32
    lam = orc.block_solve(S[0].astype(np.float64), g[0].astype(np.float64), N).astype(np.float32)
    x = orc.direct_solve(S[0], g[0], N)
    err, err_f32 = relinf(lam, x), relinf(orc.block_solve(S[0], g[0], N), x)
    print(N, err, "float sweep:", err_f32)
    assert err <= LIMIT_F32_IO
