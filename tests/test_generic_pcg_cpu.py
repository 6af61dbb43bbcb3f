"""CPU: the fixtures of the generic-state-size PCG tests (tests/generic_pcg_cases.py, tests/test_gpu_generic_pcg.py) pinned to what the reference
arithmetic can do before a GPU is involved — as tests/test_generic_producers_cpu.py does for the producers.  These are conditions on the INPUTS:
if a seed misses one, the seed or the draw weights change, never the condition; the GPU tests skip nothing."""
import numpy as np
import pytest

import generic_pcg_cases as gc
from util import relinf


@pytest.mark.parametrize("rho", gc.RHOS)
@pytest.mark.parametrize("pc", gc.PCS)
@pytest.mark.parametrize("n,m,N", [s[:3] for s in gc.SHAPES])
def test_float32_oracle_is_finite_and_near_the_float64_iterate_at_every_fixed_count(orc, n, m, N, pc, rho):
    """Every K of k_for: the float32 oracle is finite and within 1e-5 of the float64 iterate (measured: <= 4.6e-6, at (64, 20, 39) "ss"; it64
    between 11 and 76 for every shape with N > 5) — these systems are well conditioned, fixed-count runs stop short of exact convergence."""
    S, P, g = gc.system(n, m, N, 2, gc.SEED, np.float32, rho, pc)
    lam0 = gc.start(n, N, 2, gc.SEED, np.float32)
    it64, Ks = gc.k_for(S, P, g, lam0, n, N, pc)
    assert Ks and all(1 <= K <= max(1, it64 - 3) and K <= 25 for K in Ks)
    if N > 5:
        assert 11 <= it64 <= 76 and Ks[:2] == [1, 3] and Ks[-1] == min(25, it64 - 3)
    blocks = np.isnan(P.reshape(2, N, 3, n * n)).all(axis=3)            # the slots a kernel must not read are NaN in what the GPU gets
    assert blocks[:, 0, 0].all() and blocks[:, N - 1, 2].all() and blocks.sum() == 2 * (2 if pc == "ss" else 2 * N)
    for K in Ks:
        for b in range(2):
            r64 = gc.ref64(S[b], P[b], g[b], lam0[b], n, N, K, pc)["lam"]
            r32 = orc.pcg(gc.z(S[b]), gc.z(P[b]), g[b], lam0[b], N, K, 0.0, pc, n=n)["lam"]
            assert np.isfinite(r32).all() and np.isfinite(r64).all()
            d = relinf(r32, r64)
            print(n, m, N, pc, rho, "it64", it64, "K", K, "trajectory", b, d)
            assert d <= 1e-5


def test_past_exact_convergence_the_float32_oracle_breaks_down(orc):
    """Why k_for exists: (1, 1, N = 2) under "ss" has converged after one iteration, and K = 3 is 0 / 0 in float32."""
    S, P, g = gc.system(1, 1, 2, 2, gc.SEED, np.float32, 1e-3, "ss")
    it64, Ks = gc.k_for(S, P, g, np.zeros((2, 2), np.float32), 1, 2, "ss")
    assert it64 == 1 and Ks == [1]
    assert not np.isfinite(orc.pcg(gc.z(S[0]), gc.z(P[0]), g[0], np.zeros(2, np.float32), 2, 3, 0.0, "ss", n=1)["lam"]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,m,N", gc.ASYM_SHAPES)
def test_asymmetric_variants_are_told_apart(orc, n, m, N, dtype):
    """The float64 oracle iterate on the asymmetric matrices is more than 100 x the GPU test's tolerance away from the iterate on the
    symmetrised ones (right := left^T): a kernel that took the right block from the next row's left block would fail.  K = 1 and 3: with an
    asymmetric S the iteration is no longer CG, and by K = 25 its float32 band reaches 0.14 at (13, 5, 9) — no yardstick."""
    S, P, g = gc.system(n, m, N, 2, gc.SEED, dtype, 1e-3, "ss")
    lam0 = gc.start(n, N, 2, gc.SEED, dtype)
    for b in range(2):
        for name, (Sa, Pa) in gc.asymmetric(S[b], P[b], n, N, gc.SEED).items():
            left = lambda M: M.reshape(N, 3, n * n)[:, :2]
            assert np.array_equal(left(Sa), left(S[b]), equal_nan=True) and np.array_equal(left(Pa), left(P[b]), equal_nan=True)
            for K in gc.ASYM_KS:
                ra = gc.ref64(Sa, Pa, g[b], lam0[b], n, N, K, "ss")["lam"]
                rs = gc.ref64(gc.symmetrised(Sa, n, N), gc.symmetrised(Pa, n, N), g[b], lam0[b], n, N, K, "ss")["lam"]
                tol = (gc.tol32 if dtype == np.float32 else gc.tol64)(Sa, Pa, g[b], lam0[b], n, N, K, "ss", ra)
                print(n, N, np.dtype(dtype).name, name, "K", K, "distance", relinf(rs, ra), "tolerance", tol)
                assert np.isfinite(ra).all() and relinf(rs, ra) > 100 * tol


def test_fuzz_seed_covers_both_widths_warm_starts_and_double(orc):
    r = gc.fuzz(cases=80, seed=gc.FUZZ_SEED)
    print(r)
    gc.check_fuzz_inputs(r)
