"""GPU: the generic-state-size PCG kernel (pcg_generic_kernel<T, 0, NTHR>, mpcgpu_amd/csrc/pcg_f64.hip.h — the only PCG a handle with
state_size != 14 has) at its branch points, against the float64 oracle.  Cases and tolerances: tests/generic_pcg_cases.py, pinned on the CPU by
tests/test_generic_pcg_cpu.py.  Both workgroup widths with a run-time n, several trips of the row loop, dynamic LDS above 48 and 64 KiB, the
shape limits and the double refusal, the neighbours of the tuned size, block-asymmetric matrices, warm starts, the 0-iteration exits, the
12-argument entries' r / p, bit equality run to run, across batch compositions and beyond the resident workgroups, a seeded fuzz.

Measured worst error / tolerance on an MI355X: see DESIGN.md §5 (generic state sizes)."""
import numpy as np
import pytest
import torch

import generic_pcg_cases as gc
from util import fp32_iters_band, relinf

pytestmark = pytest.mark.gpu

RHO = 1e-3
SHAPES3 = [s[:3] for s in gc.SHAPES]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()              # (a copy: the shared systems are read-only)


def solver(n, N, B=2):
    from mpcgpu_amd import PcgSolver
    return PcgSolver(N, max_batch=B, state_size=n)


def run(sol, dtype, dS, dP, dg, lam0, K, pc, tol=0.0):
    """One solve from lam0 (host); returns (lambda, iters, exits) on the host."""
    from mpcgpu_amd import pcg_config
    lam = dev(lam0.copy())
    it, ex = (sol.solve if dtype == np.float32 else sol.solve_f64)(dS, dP, dg, lam, pcg_config(pcg_exit_tol=tol, pcg_max_iter=K), pc)
    torch.cuda.synchronize()
    return lam.cpu().numpy(), it.cpu().numpy(), ex.cpu().numpy()


def check_launch(sol, n, N, dtype):
    esz = np.dtype(dtype).itemsize
    assert sol.get_option("last_kernel_family") == 3
    assert sol.get_option("last_kernel_waves") == gc.waves(n, N)
    assert sol.get_option("last_kernel_lds_bytes") == gc.lds_bytes(n, N, esz)
    if esz == 4:
        assert sol.lib.mpcg_pcg_lds_bytes(n, N) == gc.lds_bytes(n, N) == 4 * (2 * (N + 2) * n + 2 * N * n + 16)


def fixed_k_vs_oracle(n, m, N, pc, dtype):
    """B = 2 (trajectory 0 cold, trajectory 1 from 0.1 * randn), every K of k_for: counts, flags, the launch, lambda inside the band."""
    S, P, g = gc.system(n, m, N, 2, gc.SEED, dtype, RHO, pc)
    lam0 = gc.start(n, N, 2, gc.SEED, dtype)
    it64, Ks = gc.k_for(S, P, g, lam0, n, N, pc)
    sol = solver(n, N)
    dS, dP, dg = dev(S), dev(P), dev(g)
    worst = 0.0
    for K in Ks:
        lam, it, ex = run(sol, dtype, dS, dP, dg, lam0, K, pc)
        assert (it == K).all() and (ex == 1).all(), (K, it, ex)
        check_launch(sol, n, N, dtype)
        for b in range(2):
            ref = gc.ref64(S[b], P[b], g[b], lam0[b], n, N, K, pc)["lam"]
            tol = (gc.tol32 if dtype == np.float32 else gc.tol64)(S[b], P[b], g[b], lam0[b], n, N, K, pc, ref)
            assert np.isfinite(lam[b]).all(), (K, b)
            e = relinf(lam[b], ref)
            worst = max(worst, e / tol)
            print(f"n={n} m={m} N={N} {pc} {np.dtype(dtype).name} it64={it64} K={K} trajectory {b}: error {e:.2e} tolerance {tol:.2e}")
            assert e <= tol, (K, b, e, tol)
    print(f"worst error / tolerance n={n} m={m} N={N} {pc} {np.dtype(dtype).name}: {worst:.3f}")


@pytest.mark.parametrize("pc", gc.PCS)
@pytest.mark.parametrize("n,m,N", SHAPES3)
def test_fixed_count_float_vs_float64_oracle(orc, n, m, N, pc):
    """Tolerance: the suite's tight tier, max(2e-5, 4 x fp32_band).  Measured worst error / tolerance on an MI355X: 0.188 (at (64, 20, 39),
    block-Jacobi; per shape in DESIGN.md §5)."""
    fixed_k_vs_oracle(n, m, N, pc, np.float32)


@pytest.mark.parametrize("pc", gc.PCS)
@pytest.mark.parametrize("n,m,N", [s for s in SHAPES3 if gc.fits_double(s[0], s[2])])
def test_fixed_count_double_vs_float64_oracle(orc, n, m, N, pc):
    """Every shape whose double iterates fit 160 KiB.  Tolerance: max(1e-10, 20 x the band of a one-ulp change of gamma)."""
    fixed_k_vs_oracle(n, m, N, pc, np.float64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,m,N", gc.ASYM_SHAPES)
def test_block_asymmetric_matrices_are_solved_as_given(orc, n, m, N, dtype):
    """A generic handle reads all three block columns (PcgArgsG::lower stays 0): an S or Pinv whose right blocks are NOT the next row's left
    blocks transposed is solved as given — twice per case on one handle, so a symmetry latch would have had time to resolve.  Only the answers
    are asserted (the CPU module shows the symmetrised system's iterate is > 100 tolerances away)."""
    S, P, g = gc.system(n, m, N, 2, gc.SEED, dtype, RHO, "ss")
    lam0 = gc.start(n, N, 2, gc.SEED, dtype)
    variants = [gc.asymmetric(S[b], P[b], n, N, gc.SEED) for b in range(2)]
    sol = solver(n, N)
    dg = dev(g)
    for name in ("pinv", "s"):
        Sa, Pa = (np.stack([variants[b][name][i] for b in range(2)]) for i in range(2))
        dS, dP = dev(Sa), dev(Pa)
        for K in gc.ASYM_KS:
            for call in range(2):
                lam, it, ex = run(sol, dtype, dS, dP, dg, lam0, K, "ss")
                assert (it == K).all() and (ex == 1).all()
                check_launch(sol, n, N, dtype)
                for b in range(2):
                    ref = gc.ref64(Sa[b], Pa[b], g[b], lam0[b], n, N, K, "ss")["lam"]
                    tol = (gc.tol32 if dtype == np.float32 else gc.tol64)(Sa[b], Pa[b], g[b], lam0[b], n, N, K, "ss", ref)
                    e = relinf(lam[b], ref)
                    print(f"asymmetric {name} n={n} N={N} {np.dtype(dtype).name} K={K} call {call} trajectory {b}: error {e:.2e} tolerance {tol:.2e}")
                    assert np.isfinite(lam[b]).all() and e <= tol, (name, K, call, b, e, tol)


@pytest.mark.parametrize("pc", gc.PCS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tolerance_exit_then_zero_iterations_leave_lambda_bit_for_bit(orc, dtype, pc):
    n, m, N = 33, 11, 40
    tol = 1e-6 if dtype == np.float32 else 1e-10
    S, P, g = gc.system(n, m, N, 2, gc.SEED, dtype, RHO, pc)
    lam0 = gc.start(n, N, 2, gc.SEED, dtype)
    sol = solver(n, N)
    dS, dP = dev(S), dev(P)
    lam, it, ex = run(sol, dtype, dS, dP, dev(g), lam0, 500, pc, tol=tol)
    assert (ex == 0).all(), ex
    for b in range(2):
        if dtype == np.float32:
            lo, hi = fp32_iters_band(orc, S[b], P[b], g[b], lam0[b], N, 500, tol, pc, n=n)
        else:
            ref = orc.pcg(gc.z(S[b]), gc.z(P[b]), g[b], lam0[b], N, 500, tol, pc, n=n)["iters"]
            lo, hi = ref - max(2, 0.03 * ref), ref + max(2, 0.03 * ref)
        print(f"tolerance exit {np.dtype(dtype).name} {pc} trajectory {b}: {int(it[b])} iterations, band {lo}..{hi}")
        assert lo <= int(it[b]) <= hi, (b, int(it[b]), lo, hi)
    # a second call from the converged lambda with a -0.0 planted in it: the right-hand side that lambda solves (S lambda in float64, rounded)
    # leaves a residual of rounding size, so the oracle in the same precision takes no iteration — and neither may the kernel, which has to
    # hand lambda back bit for bit
    lam[:, 7] = -0.0
    lam[1, n * N - 1] = -0.0
    g2 = np.stack([orc.bt_spmv(gc.z(S[b], np.float64), lam[b].astype(np.float64), N, n=n) for b in range(2)]).astype(dtype)
    for b in range(2):
        r = orc.pcg(gc.z(S[b]), gc.z(P[b]), g2[b], lam[b], N, 500, tol, pc, n=n, hist=True)
        assert r["iters"] == 0 and not r["max_iter_exit"] and r["eta_hist"][0] < tol / 10, r["eta_hist"]
    lam2, it2, ex2 = run(sol, dtype, dS, dP, dev(g2), lam, 500, pc, tol=tol)
    assert (it2 == 0).all() and (ex2 == 0).all(), (it2, ex2)
    assert lam2.tobytes() == lam.tobytes() and np.signbit(lam2[0, 7]) and np.signbit(lam2[1, n * N - 1])
    # max_iter = 0: no iteration, the flag says "ran out of iterations", lambda bit for bit
    lam3, it3, ex3 = run(sol, dtype, dS, dP, dev(g), lam, 0, pc, tol=0.0)
    assert (it3 == 0).all() and (ex3 == 1).all(), (it3, ex3)
    assert lam3.tobytes() == lam.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,m,N", [(15, 7, 9), (64, 20, 39)])
def test_twelve_argument_entries_return_lambda_r_and_p(orc, n, m, N, dtype):
    """mpcg_pcg_solve_ref / _ref_f64 (one trajectory, symmetric stair): lambda, r and p after K iterations against the oracle's, each vector
    inside its own band."""
    S, P, g = gc.system(n, m, N, 2, gc.SEED, dtype, RHO, "ss")
    lam0 = gc.start(n, N, 2, gc.SEED, dtype)
    b = 1                                               # the warm-started trajectory
    it64, Ks = gc.k_for(S[b], P[b], g[b], lam0[b], n, N, "ss")
    sol = solver(n, N, 1)
    dS, dP, dg = dev(S[b]), dev(P[b]), dev(g[b])
    for K in Ks:
        lam = dev(lam0[b].copy())
        r, p = (torch.full((n * N,), float("nan"), dtype=TORCH[dtype], device="cuda") for _ in range(2))
        it, ex = torch.full((1,), -7, dtype=torch.int32, device="cuda"), torch.full((1,), 0xAB, dtype=torch.uint8, device="cuda")
        (sol.solve_ref if dtype == np.float32 else sol.solve_ref_f64)(dS, dP, dg, lam, r, p, None, None, it, ex, K, 0.0)
        torch.cuda.synchronize()
        assert int(it[0]) == K and int(ex[0]) == 1
        check_launch(sol, n, N, dtype)
        ref = gc.ref64(S[b], P[b], g[b], lam0[b], n, N, K, "ss")
        for vec, got in (("lam", lam), ("r", r), ("p", p)):
            got = got.cpu().numpy()
            tol = (gc.tol32 if dtype == np.float32 else gc.tol64)(S[b], P[b], g[b], lam0[b], n, N, K, "ss", ref[vec], vec=vec)
            e = relinf(got, ref[vec])
            print(f"12-argument entry n={n} N={N} {np.dtype(dtype).name} K={K} {vec}: error {e:.2e} tolerance {tol:.2e}")
            assert np.isfinite(got).all() and e <= tol, (K, vec, e, tol)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,m,N", [(7, 3, 128), (3, 1, 250)])
def test_bits_run_to_run_and_across_batch_compositions(orc, n, m, N, dtype):
    B = 5
    S, P, g = gc.system(n, m, N, B, gc.SEED, dtype, RHO, "ss")
    lam0 = gc.start(n, N, B, gc.SEED, dtype)
    K = gc.k_for(S, P, g, lam0, n, N, "ss")[1][-1]
    sol = solver(n, N, B)
    dS, dP, dg = dev(S), dev(P), dev(g)
    lam, it, ex = run(sol, dtype, dS, dP, dg, lam0, K, "ss")
    lam_again, it_again, _ = run(sol, dtype, dS, dP, dg, lam0, K, "ss")
    assert np.isfinite(lam).all() and (it == K).all()
    assert lam_again.tobytes() == lam.tobytes() and (it_again == it).all()
    one = solver(n, N, 1)
    for b in range(B):
        alone, it1, ex1 = run(one, dtype, dev(S[b:b + 1]), dev(P[b:b + 1]), dev(g[b:b + 1]), lam0[b:b + 1], K, "ss")
        assert alone.tobytes() == lam[b:b + 1].tobytes() and int(it1[0]) == K and int(ex1[0]) == 1, b


def test_more_workgroups_than_the_chip_holds_every_copy_bit_equal(orc):
    """(4, 1, N = 6), batch 3000 tiled from 6 distinct systems (warm starts included): workgroups b and b + 6 j must return the same bits, and
    the first six the oracle's iterate."""
    n, m, N, D, B = 4, 1, 6, 6, 3000
    S, P, g = gc.system(n, m, N, D, gc.SEED, np.float32, RHO, "jacobi")
    lam0 = gc.start(n, N, D, gc.SEED, np.float32)
    K = gc.k_for(S, P, g, lam0, n, N, "jacobi")[1][-1]
    tile = lambda a: np.tile(a, (B // D, 1))
    sol = solver(n, N, B)
    assert B > (32 // 4) * sol.get_option("num_cus")        # (a CU holds 32 wavefronts: eight of these 256-thread workgroups at the most)
    lam, it, ex = run(sol, np.float32, dev(tile(S)), dev(tile(P)), dev(tile(g)), tile(lam0), K, "jacobi")
    assert (it == K).all() and (ex == 1).all()
    copies = lam.reshape(B // D, D, n * N)
    assert all(copies[j].tobytes() == copies[0].tobytes() for j in range(1, B // D))
    for b in range(D):
        ref = gc.ref64(S[b], P[b], g[b], lam0[b], n, N, K, "jacobi")["lam"]
        assert relinf(lam[b], ref) <= gc.tol32(S[b], P[b], g[b], lam0[b], n, N, K, "jacobi", ref)


def test_shape_limits_of_mpcg_create():
    from mpcgpu_amd import PcgSolver, _lib
    lib = _lib.load()
    sol = PcgSolver(158, state_size=64)                 # 162,880 B of float iterates: the largest horizon at n = 64
    assert lib.mpcg_pcg_lds_bytes(64, 158) == gc.lds_bytes(64, 158) == 162880 <= gc.LDS_MAX < gc.lds_bytes(64, 159)
    sol.close()
    for n, N in ((64, 159), (65, 10), (0, 10)):
        with pytest.raises(_lib.MpcgError) as e:
            PcgSolver(N, state_size=n)
        assert e.value.code == _lib.MPCG_ERR_UNSUPPORTED, (n, N)
        assert lib.mpcg_pcg_lds_bytes(n, N) == 0 and lib.mpcg_pcg_lds_bytes_f64(n, N) == 0, (n, N)


def test_double_solve_refused_where_only_the_float_iterates_fit(orc):
    """(40, 10, 128): 82,624 B of float iterates, 165,248 B of double ones.  mpcg_create sizes the LDS for float, so the handle exists;
    mpcg_pcg_solve_f64 on it says MPCG_ERR_UNSUPPORTED and touches nothing, and the handle goes on solving in float."""
    from mpcgpu_amd import _lib, pcg_config
    n, m, N = 40, 10, 128
    S, P, g = gc.system(n, m, N, 2, gc.SEED, np.float32, RHO, "ss")
    lam0 = gc.start(n, N, 2, gc.SEED, np.float32)
    assert gc.lds_bytes(n, N, 4) == 82624 and gc.lds_bytes(n, N, 8) == 165248 > gc.LDS_MAX
    sol = solver(n, N)
    assert sol.lib.mpcg_pcg_lds_bytes_f64(n, N) == 0
    lam64 = torch.full((2, n * N), float("nan"), dtype=torch.float64, device="cuda")
    it = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    ex = torch.full((2,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.MpcgError) as e:
        sol.solve_f64(dev(S.astype(np.float64)), dev(P.astype(np.float64)), dev(g.astype(np.float64)), lam64,
                      pcg_config(pcg_exit_tol=0.0, pcg_max_iter=3), "ss", iters=it, exits=ex)
    torch.cuda.synchronize()
    assert e.value.code == _lib.MPCG_ERR_UNSUPPORTED and "160 KiB" in str(e.value), str(e.value)
    assert torch.isnan(lam64).all() and (it == -7).all() and (ex == 0xAB).all()
    K = 3
    lam, itf, exf = run(sol, np.float32, dev(S), dev(P), dev(g), lam0, K, "ss")
    assert (itf == K).all() and (exf == 1).all()
    check_launch(sol, n, N, np.float32)
    for b in range(2):
        ref = gc.ref64(S[b], P[b], g[b], lam0[b], n, N, K, "ss")["lam"]
        assert relinf(lam[b], ref) <= gc.tol32(S[b], P[b], g[b], lam0[b], n, N, K, "ss", ref)


@pytest.mark.parametrize("n,N", [(40, 128), (64, 158)])
def test_occupancy_with_large_dynamic_lds(n, N):
    """82 KiB and 159 KiB of dynamic LDS (the hipFuncSetAttribute path of mpcg_check_pcg_occupancy): a CU has 160 KiB, so exactly one
    workgroup fits and the call returns num_cus."""
    sol = solver(n, N)
    fit = gc.LDS_MAX // gc.lds_bytes(n, N)
    assert fit == 1
    occ = sol.checkPcgOccupancy()
    assert occ == fit * sol.get_option("num_cus") >= sol.get_option("num_cus"), occ


def test_seeded_fuzz_of_the_generic_kernel(orc):
    r = gc.fuzz(cases=80, seed=gc.FUZZ_SEED, gpu=True)
    print(r)
    assert r["mismatches"] == 0, r
    gc.check_fuzz_inputs(r)
    assert r["worst_error_over_tolerance"] <= 1.0, r
