"""GPU (MI355X): parity of the HIP path — called through the C ABI (libmpcg_hip.so via
mpcgpu_amd.PcgSolver) — against the CPU oracle and the committed golden vectors.

Stated fp32 tolerance, E = |lam_hip - lam_f64|_inf / |lam_f64|_inf against the
float64 iterate after the SAME number of iterations (exit_tol = 0):
  K <= 3  : E <= max(2e-5, 4*band), band < 5e-4 (before CG amplifies rounding: pins the arithmetic)
  K = 10  : E <= max(1e-4, 4*band) (the tier between: a 1e-4-level arithmetic slip no longer hides under the K <= 50 floor)
  K <= 50 : E <= max(1e-3, 4*band), band = util.fp32_band = what the CPU float32 restatement does on
            the same and on 1-ulp-perturbed inputs (fp32 CG at cond ~1e5 drifts 1e-4..4e-3 by K=25-50
            whatever the summation order).
With tolerance exit: flag 0, iteration count within 7 % (+-2) of the band of counts the CPU float32
restatement produces on the same and on 1-ulp-perturbed inputs (util.fp32_iters_band; the crossing
iteration of fp32 CG is erratic: 174..201 on the N=32 golden system vs 172 in float64), and the true
residual no worse than 2x the CPU float32 restatement's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mpcgpu_amd import synth
from util import exit_iter_bounds, fp32_band, fp32_iters_band, golden, relinf, rel_residual

pytestmark = pytest.mark.gpu
n = 14


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


@pytest.fixture(scope="module")
def P():
    from mpcgpu_amd import PcgSolver, pcg_config, _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    _lib.load()          # fails loudly if the extension is missing: there is no fallback
    return PcgSolver, pcg_config


def solve(P, N, S, Pinv, gamma, lam0, max_iter, tol, precond="ss", waves=None):
    PcgSolver, pcg_config = P
    B = S.shape[0]
    sol = PcgSolver(N, max_batch=B)
    if waves:          # explicit wave count = the pure streaming variant; waves=None = mpcg_create's default
        sol.set_option("pcg_waves", waves)
        sol.set_option("pcg_reg_rows", 0)
        sol.set_option("pcg_lds_rows", 0)
    lam = dev(lam0, torch.float32)
    it, ex = sol.solve(dev(S), dev(Pinv), dev(gamma), lam,
                       pcg_config(pcg_exit_tol=tol, pcg_max_iter=max_iter), precond)
    torch.cuda.synchronize()
    if waves:          # the kernel that ran is the one that was asked for: single-workgroup <waves, 0, 2>
        assert last_kernel(sol) == {"family": 0, "waves": waves, "reg_rows": 0, "lds_rows": 0, "stream_bufs": 2, "cluster": 0}
    return lam.cpu().numpy(), it.cpu().numpy(), ex.cpu().numpy()


def last_kernel(sol):
    """What the last solve on this handle launched (family 0 = single workgroup per trajectory, 1 = cluster,
    2 = lane per block)."""
    return {k: sol.get_option("last_kernel_" + k) for k in ("family", "waves", "reg_rows", "lds_rows", "stream_bufs", "cluster")}


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 32])
@pytest.mark.parametrize("cols", [3, 1])
def test_spmv_matches_golden_and_oracle(P, orc, N, cols):
    G = golden(N)
    M = G["S"].copy().reshape(N, 3, 196)
    M[0, 0] = np.nan          # never-written slots must not be read
    M[-1, 2] = np.nan
    sol = P[0](N, max_batch=1)
    y = sol.bt_spmv(dev(M.reshape(1, -1)), dev(G["spmv_x"].reshape(1, -1)), cols=cols).cpu().numpy()[0]
    ref = orc.bt_spmv(G["S"].astype(np.float64), G["spmv_x"], N, cols=cols)
    assert np.isfinite(y).all() and relinf(y, ref) < 2e-6
    if cols == 3:
        assert relinf(y, G["spmv_y"]) < 2e-6


@pytest.mark.parametrize("N,B", [(3, 1), (9, 3), (33, 5), (50, 7), (128, 3)])
def test_spmv_ragged_row_counts_and_output_bounds(P, orc, N, B):
    """The kernel walks spans of 16 block rows and stores a span's y as whole 128-byte lines: row counts that are no multiple of 16 (the last
    span is ragged, spans straddle trajectories), every trajectory against the oracle, and nothing written outside y (guard words on both sides,
    and an x whose neighbours in memory are NaN)."""
    k = synth.make_kkt(N, B, 77 + N)
    S, _, _ = synth.form_schur(k, poison_unused=True)
    rng = np.random.default_rng(N)
    x = rng.normal(size=(B, n * N)).astype(np.float32)
    sol = P[0](N, max_batch=B)
    xg = torch.full((B * n * N + 64,), float("nan"), device="cuda")
    xg[32:32 + B * n * N] = dev(x).reshape(-1)
    yg = torch.full((B * n * N + 64,), 12345.0, device="cuda")
    sol.bt_spmv(dev(S), xg[32:32 + B * n * N].view(B, -1), yg[32:32 + B * n * N].view(B, -1))
    torch.cuda.synchronize()
    out = yg.cpu().numpy()
    assert (out[:32] == 12345.0).all() and (out[-32:] == 12345.0).all()
    y = out[32:-32].reshape(B, -1)
    assert np.isfinite(y).all()
    for b in range(B):
        assert relinf(y[b], orc.bt_spmv(np.nan_to_num(S[b]).astype(np.float64), x[b], N)) < 5e-6


def test_spmv_batched_full_size_properties(P, orc):
    """N=128, batch 64: oracle parity on sampled trajectories + linearity + symmetry x^T S y = y^T S x."""
    N, B = 128, 64
    k = synth.make_kkt(N, B, 5)
    S, _, _ = synth.form_schur(k, poison_unused=True)
    rng = np.random.default_rng(0)
    x = rng.normal(size=(B, n * N)).astype(np.float32)
    z = rng.normal(size=(B, n * N)).astype(np.float32)
    sol = P[0](N, max_batch=B)
    dS = dev(S)
    yx = sol.bt_spmv(dS, dev(x)).cpu().numpy()
    yz = sol.bt_spmv(dS, dev(z)).cpu().numpy()
    yxz = sol.bt_spmv(dS, dev(2.0 * x - 0.5 * z)).cpu().numpy()
    assert np.isfinite(yx).all()
    for b in (0, 17, 63):
        assert relinf(yx[b], orc.bt_spmv(np.nan_to_num(S[b]).astype(np.float64), x[b], N)) < 5e-6
    assert relinf(yxz, 2.0 * yx - 0.5 * yz) < 5e-6
    a = np.einsum("bi,bi->b", z.astype(np.float64), yx.astype(np.float64))
    c = np.einsum("bi,bi->b", x.astype(np.float64), yz.astype(np.float64))
    assert np.abs(a - c).max() / np.abs(a).max() < 1e-5


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 32])
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
@pytest.mark.parametrize("waves", [4, 8, 16])
def test_pcg_fixed_iterations_vs_golden(P, orc, N, pc, waves):
    G = golden(N)
    Pm = G["Pinv"].copy().reshape(N, 3, 196)
    Sm = G["S"].copy().reshape(N, 3, 196)
    for M in (Pm, Sm):
        M[0, 0] = np.nan
        M[-1, 2] = np.nan
    if pc == "jacobi":        # block-Jacobi must not read the off-diagonal blocks at all
        Pm[:, 0] = np.nan
        Pm[:, 2] = np.nan
    for K in (5, 20, 50):
        lam, it, ex = solve(P, N, Sm.reshape(1, -1), Pm.reshape(1, -1), G["gamma"].reshape(1, -1),
                            np.zeros((1, n * N), np.float32), K, 0.0, pc, waves)
        want = G[f"lam_{pc}_K{K}"]
        band = fp32_band(orc, G["S"], G["Pinv"], G["gamma"], np.zeros(n * N), N, K, pc, want)
        assert it[0] == K and ex[0] == 1
        assert relinf(lam[0], want) <= max(1e-3, 4 * band), (K, relinf(lam[0], want), band)


@pytest.mark.parametrize("N", [8, 32, 128, 512])
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
def test_pcg_first_iterations_tight(P, orc, N, pc):
    """K = 1, 2, 3 from a random warm start: rounding has not been amplified yet, so the HIP arithmetic
    must agree with float64 to a few 1e-5 (4x what the CPU float32 restatement manages, itself
    < 5e-4) — a wrong block, row, sign or reduction would show as O(1)."""
    k = synth.make_kkt(N, 2, 31 + N)
    S, Pinv, g = synth.form_schur(k, poison_unused=True)
    lam0 = np.random.default_rng(N).normal(0, 0.5, (2, n * N)).astype(np.float32)
    for K in (1, 2, 3):
        lam, it, ex = solve(P, N, S, Pinv, g, lam0, K, 0.0, pc)
        for b in range(2):
            r64 = orc.pcg(np.nan_to_num(S[b]).astype(np.float64), np.nan_to_num(Pinv[b]).astype(np.float64),
                          g[b].astype(np.float64), lam0[b].astype(np.float64), N, K, 0.0, pc)
            band = fp32_band(orc, S[b], Pinv[b], g[b], lam0[b], N, K, pc, r64["lam"])
            assert band < 5e-4
            assert relinf(lam[b], r64["lam"]) <= max(2e-5, 4 * band), (K, b, relinf(lam[b], r64["lam"]), band)


@pytest.mark.parametrize("N", [8, 32, 128, 256, 512])
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
def test_pcg_ten_iterations_middle_tier(P, orc, N, pc):
    """K = 10 (VERDICT r04 #2c): E <= max(1e-4, 4 x band) — ten times tighter than the K <= 50 floor of 1e-3, on every kernel family of the
    default policy (N = 8 / 32: row-per-lane, 128: lane-pair, 256 / 512: clustered), cold and warm start."""
    B = 2
    k = synth.make_kkt(N, B, 77 + N)
    S, Pinv, g = synth.form_schur(k, poison_unused=True)
    rng = np.random.default_rng(10 + N)
    for lam0 in (np.zeros((B, n * N), np.float32), rng.normal(0, 0.3, (B, n * N)).astype(np.float32)):
        lam, it, ex = solve(P, N, S, Pinv, g, lam0, 10, 0.0, pc)
        assert (it == 10).all() and (ex == 1).all()
        for b in range(B):
            Sz, Pz = np.nan_to_num(S[b]), np.nan_to_num(Pinv[b])
            r64 = orc.pcg(Sz.astype(np.float64), Pz.astype(np.float64), g[b].astype(np.float64), lam0[b].astype(np.float64), N, 10, 0.0, pc)
            band = fp32_band(orc, Sz, Pz, g[b], lam0[b], N, 10, pc, r64["lam"])
            e = relinf(lam[b], r64["lam"])
            assert e <= max(1e-4, 4 * band), (N, pc, b, e, band)


@pytest.mark.parametrize("N", [8, 32])
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
def test_pcg_tolerance_exit_vs_golden(P, orc, N, pc):
    G = golden(N)
    want_it = int(G[f"iters_tol_{pc}"])
    lam, it, ex = solve(P, N, G["S"].reshape(1, -1), G["Pinv"].reshape(1, -1), G["gamma"].reshape(1, -1),
                        np.zeros((1, n * N), np.float32), 5000, 1e-4, pc)
    assert ex[0] == 0
    lo, hi = exit_iter_bounds(orc, G["S"], G["Pinv"], G["gamma"], np.zeros(n * N), N, 5000, 1e-4, pc)
    assert lo <= int(it[0]) <= hi and lo <= want_it <= hi, (int(it[0]), lo, hi, want_it)
    cpu32 = orc.pcg(G["S"], G["Pinv"], G["gamma"], np.zeros(n * N, np.float32), N, 5000, 1e-4, pc)
    r_hip = rel_residual(G["S"], G["gamma"], lam[0], N)
    r_cpu = rel_residual(G["S"], G["gamma"], cpu32["lam"], N)
    assert r_hip <= 2 * r_cpu + 1e-6
    assert relinf(lam[0], G["lam_direct"]) < 0.15        # loose tolerance => ~5 % from the exact solve


def test_pcg_max_iter_flag_and_warm_start(P, orc):
    G = golden(8)
    N = 8
    args = (G["S"].reshape(1, -1), G["Pinv"].reshape(1, -1), G["gamma"].reshape(1, -1))
    lam, it, ex = solve(P, N, *args, np.zeros((1, n * N), np.float32), 7, 1e-4)
    assert it[0] == 7 and ex[0] == 1                      # ran out of iterations (mpcsim.cuh:382-387)
    lam, it, ex = solve(P, N, *args, G["lam_warm"].reshape(1, -1), 20, 0.0)
    band = fp32_band(orc, G["S"], G["Pinv"], G["gamma"], G["lam_warm"], N, 20, "ss", G["lam_warm_ss_K20"])
    assert relinf(lam[0], G["lam_warm_ss_K20"]) <= max(1e-3, 4 * band)    # lambda is in/out: warm start honoured
    # already converged: no update, flag cleared, lambda untouched bit for bit
    lam0 = G["lam_direct"].astype(np.float32).reshape(1, -1)
    lam, it, ex = solve(P, N, *args, lam0, 50, 1e-2)
    assert it[0] == 0 and ex[0] == 0
    np.testing.assert_array_equal(lam, lam0)
    # max_iter = 0: setup only
    lam, it, ex = solve(P, N, *args, np.zeros((1, n * N), np.float32), 0, 1e-9)
    assert it[0] == 0 and ex[0] == 1 and (lam == 0).all()


@pytest.mark.parametrize("N,waves", [(2, 16), (3, 4), (5, 8), (17, 16), (33, 8), (64, 16), (100, 16), (128, 8),
                                     (128, 16), (256, 16), (512, 16)])
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
def test_pcg_shapes_vs_oracle(P, orc, N, waves, pc):
    """Ragged / odd / maximum horizon lengths, 3 trajectories each, vs the float32 and float64 oracle."""
    B, K = 3, 25
    k = synth.make_kkt(N, B, 1000 + N)
    S, Pinv, g = synth.form_schur(k, precond="ss", poison_unused=True)
    lam, it, ex = solve(P, N, S, Pinv, g, np.zeros((B, n * N), np.float32), K, 0.0, pc, waves)
    assert (it == K).all() and (ex == 1).all() and np.isfinite(lam).all()
    for b in range(B):
        Sz, Pz = np.nan_to_num(S[b]), np.nan_to_num(Pinv[b])
        r64 = orc.pcg(Sz.astype(np.float64), Pz.astype(np.float64), g[b].astype(np.float64), np.zeros(n * N), N, K, 0.0, pc)
        band = fp32_band(orc, Sz, Pz, g[b], np.zeros(n * N), N, K, pc, r64["lam"])
        assert relinf(lam[b], r64["lam"]) <= max(1e-3, 4 * band), (relinf(lam[b], r64["lam"]), band)


def test_pcg_batched_full_size(P, orc):
    """BASELINE config 3/4 shape: N=128, SS, max_iter 167, tol 1e-4, batch 96 with mixed warm starts so
    that trajectories leave the loop at different iterations; sampled oracle parity, residual
    decrease for all, bitwise run-to-run determinism, batch-composition independence."""
    N, B = 128, 96
    k = synth.make_kkt(N, B, 2024)
    S, Pinv, g = synth.form_schur(k, poison_unused=True)
    lam0 = np.zeros((B, n * N), np.float32)
    for b in range(0, B, 3):          # every third trajectory starts close to its solution
        exact = orc.direct_solve(S[b], g[b], N)
        lam0[b] = (exact * (1 + 1e-3 * np.sin(np.arange(n * N)))).astype(np.float32)
    lam, it, ex = solve(P, N, S, Pinv, g, lam0, 167, 1e-4)
    lam2, it2, ex2 = solve(P, N, S, Pinv, g, lam0, 167, 1e-4)
    np.testing.assert_array_equal(lam, lam2)
    np.testing.assert_array_equal(it, it2)
    assert len(set(it.tolist())) > 1 and (it[ex == 1] == 167).all() and (it[ex == 0] < 167 + 1).all()
    for b in (0, 1, 2, 47, 95):
        Sz, Pz = np.nan_to_num(S[b]), np.nan_to_num(Pinv[b])
        r32 = orc.pcg(Sz, Pz, g[b], lam0[b], N, 167, 1e-4, "ss")
        lo, hi = fp32_iters_band(orc, Sz, Pz, g[b], lam0[b], N, 167, 1e-4, "ss", trials=4)
        assert 0.93 * lo - 2 <= int(it[b]) <= 1.07 * hi + 2, (b, int(it[b]), lo, hi)
        assert ex[b] == (1 if it[b] == 167 and hi == 167 else ex[b])
        r_hip, r_cpu, r_0 = (rel_residual(S[b], g[b], v, N) for v in (lam[b], r32["lam"], lam0[b]))
        assert r_hip <= 2 * r_cpu + 1e-6 and (r_hip < r_0 or it[b] == 0)
    # a trajectory's result does not depend on what else is in the batch
    sub = [5, 6, 7]
    lam_s, it_s, _ = solve(P, N, S[sub], Pinv[sub], g[sub], lam0[sub], 167, 1e-4)
    np.testing.assert_array_equal(lam_s, lam[sub])
    np.testing.assert_array_equal(it_s, it[sub])


def test_solve_ref_twelve_argument_entry(P, orc):
    """The reference's kernel argument list (include/pcg/sqp.cuh:137-150), incl. d_r / d_p contents and
    the 1-byte bool exit flag."""
    G = golden(32)
    N = 32
    sol = P[0](N)
    d_S, d_Pinv, d_gamma = dev(G["S"]), dev(G["Pinv"]), dev(G["gamma"])
    d_lambda = torch.zeros(n * N, device="cuda")
    d_r = torch.full((n * N,), 7.0, device="cuda")
    d_p = torch.full((n * N,), 7.0, device="cuda")
    d_v_temp = torch.full((N,), 3.0, device="cuda")
    d_eta_new_temp = torch.full((N,), 3.0, device="cuda")
    d_iters = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_exit = torch.zeros(1, dtype=torch.bool, device="cuda")
    sol.solve_ref(d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, d_v_temp, d_eta_new_temp, d_iters, d_exit, 20, 0.0)
    torch.cuda.synchronize()
    r64 = orc.pcg(G["S"].astype(np.float64), G["Pinv"].astype(np.float64), G["gamma"].astype(np.float64),
                  np.zeros(n * N), N, 20, 0.0, "ss")
    assert int(d_iters.item()) == 20 and bool(d_exit.item()) is True
    band = fp32_band(orc, G["S"], G["Pinv"], G["gamma"], np.zeros(n * N), N, 20, "ss", G["lam_ss_K20"])
    assert relinf(d_lambda.cpu().numpy(), G["lam_ss_K20"]) <= max(1e-3, 4 * band)
    # d_r / d_p = r and p of the last completed update: inside the same float32 band as lambda (tests/test_gpu_invariants.py pins them much harder,
    # against the recurrences themselves)
    rb = max(relinf(orc.pcg(G["S"], G["Pinv"], G["gamma"], np.zeros(n * N, np.float32), N, 20, 0.0, "ss")[k_], r64[k_]) for k_ in ("r", "p"))
    assert relinf(d_r.cpu().numpy(), r64["r"]) <= max(1e-3, 4 * rb) and relinf(d_p.cpu().numpy(), r64["p"]) <= max(1e-3, 4 * rb)
    assert (d_v_temp == 3.0).all() and (d_eta_new_temp == 3.0).all()       # accepted, untouched
    # inputs are not modified
    np.testing.assert_array_equal(d_S.cpu().numpy(), G["S"])
    np.testing.assert_array_equal(d_gamma.cpu().numpy(), G["gamma"])


def test_error_behaviour(P):
    from mpcgpu_amd import _lib
    N = 8
    sol = P[0](N, max_batch=2)
    G = golden(N)
    S3 = np.tile(G["S"], (3, 1))
    g3 = np.tile(G["gamma"], (3, 1))
    with pytest.raises(_lib.MpcgError) as e:
        sol.solve(dev(S3), dev(S3), dev(g3), torch.zeros(3, n * N, device="cuda"))
    assert e.value.code == _lib.MPCG_ERR_INVALID and "max_batch" in str(e.value)
    lib = sol.lib
    buf = torch.zeros(4 * 3 * 196 * N + 64, device="cuda")
    it = torch.zeros(1, dtype=torch.int32, device="cuda")
    ex = torch.zeros(1, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    rc = lib.mpcg_pcg_solve(sol._h, C.c_void_p(p + 4), C.c_void_p(p), C.c_void_p(p), C.c_void_p(p), 1, 5, 0.0, 3,
                            C.c_void_p(it.data_ptr()), C.c_void_p(ex.data_ptr()), None)
    assert rc == _lib.MPCG_ERR_INVALID and b"aligned" in lib.mpcg_last_error(sol._h)
    # every alignment refusal of include/mpcg.h (ALIGNMENT), one pointer at a time short of what the entry asks for, inside a guard-banded arena
    # (tests/arena.py): the code, the word — and not one byte of the arena changed, so nothing was launched
    import arena
    import arena_specs
    for mode in arena.MODES:
        ar = arena.Arena(arena_specs.refusals(N), mode, "torch")
        for name in ("S", "Pinv", "gamma"):
            ar.put(name, G[name])
        at = lambda name, shift=0: C.c_void_p(ar.address(name) + shift)
        h = sol._h
        refused = [(lib.mpcg_pcg_solve, (h, at("S", s), at("Pinv", q), at("gamma"), at("lambda"), 1, 5, 0.0, 3, at("iters"), at("exits"), None))
                   for s, q in ((4, 0), (0, 4), (8, 0), (0, 8))]
        refused += [(lib.mpcg_pcg_solve_ref, (h, at("S", s), at("Pinv", q), at("gamma"), at("lambda"), at("r"), at("p"), at("r"), at("p"), at("iters"),
                                              at("exits"), 5, 0.0, None)) for s, q in ((4, 0), (0, 4))]
        refused += [(lib.mpcg_bt_spmv, (h, at("S", s), at("gamma", x), at("lambda", y), 1, 3, None)) for s, x, y in ((4, 0, 0), (8, 0, 0), (0, 4, 0), (0, 0, 4))]
        refused += [(lib.mpcg_convert_f32_to_f16, (h, at("S", s), at("S16", d), 64, None)) for s, d in ((4, 0), (0, 2), (0, 8))]
        refused += [(lib.mpcg_pcg_solve_f16, (h, at("S16", s), at("P16", q), at("gamma"), at("lambda"), 1, 5, 0.0, 3, at("iters"), at("exits"), None))
                    for s, q in ((2, 0), (0, 2))]
        refused += [(lib.mpcg_probe_hbm_read, (h, at("S", 4), 1024, at("sink"), None))]
        before = ar.snapshot()
        for fn, args in refused:
            rc = fn(*args)
            assert rc == _lib.MPCG_ERR_INVALID and b"aligned" in lib.mpcg_last_error(h), (mode, fn.__name__, rc, lib.mpcg_last_error(h))
        assert np.array_equal(ar.snapshot(), before), mode
    rc = lib.mpcg_pcg_solve(sol._h, None, C.c_void_p(p), C.c_void_p(p), C.c_void_p(p), 1, 5, 0.0, 3,
                            C.c_void_p(it.data_ptr()), C.c_void_p(ex.data_ptr()), None)
    assert rc == _lib.MPCG_ERR_INVALID
    rc = lib.mpcg_pcg_solve(sol._h, C.c_void_p(p), C.c_void_p(p), C.c_void_p(p), C.c_void_p(p), 1, 5, 0.0, 2,
                            C.c_void_p(it.data_ptr()), C.c_void_p(ex.data_ptr()), None)
    assert rc == _lib.MPCG_ERR_INVALID
    assert sol.checkPcgOccupancy() >= 256            # at least one trajectory per CU resident
    with pytest.raises(_lib.MpcgError):
        P[0](1024)                                    # vectors do not fit LDS -> unsupported, loudly


def test_runs_on_non_default_stream(P, orc):
    G = golden(8)
    N = 8
    sol = P[0](N)
    s = torch.cuda.Stream()
    lam = torch.zeros(1, n * N, device="cuda")
    dS, dP, dg = dev(G["S"].reshape(1, -1)), dev(G["Pinv"].reshape(1, -1)), dev(G["gamma"].reshape(1, -1))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        it, ex = sol.solve(dS, dP, dg, lam, P[1](pcg_exit_tol=0.0, pcg_max_iter=20))
    s.synchronize()
    band = fp32_band(orc, G["S"], G["Pinv"], G["gamma"], np.zeros(n * N), N, 20, "ss", G["lam_ss_K20"])
    assert relinf(lam.cpu().numpy()[0], G["lam_ss_K20"]) <= max(1e-3, 4 * band)


def test_cpp_callsite_over_shim_headers():
    """examples/sqp_pcg_callsite.cpp = the reference's call site (include/pcg/sqp.cuh:116-151, 230-232)
    compiled against include/gbd_pcg_compat/gpu_pcg.cuh and linked to libmpcg_hip.so; it checks its own
    residual on the CPU and exits non-zero on failure."""
    import json
    import os
    import subprocess
    from mpcgpu_amd import build
    exe = build.EXAMPLE_BIN
    if not os.path.exists(exe):
        exe = build.build_example()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["pcg_exit"] == 0 and 0 < out["pcg_iters"] < 200 and out["rel_residual"] < 1e-4
    assert out["two_threads_two_streams_same_bits"] == 1     # mpcgLaunchPcg(..., stream) from two host threads: a handle per thread, the same bits
    assert out["smem"] == 4 * (6 * (32 + 2) * 14 + 16)   # pcgSharedMemSize = the dynamic LDS of the launch a default solve makes (N = 32: the row-per-lane kernel, 8 waves)
    # the same source with -DUSE_DOUBLES: pcg<double, n, N>, mpcgLaunchPcg<double>
    exe64 = build.EXAMPLE_BIN64 if os.path.exists(build.EXAMPLE_BIN64) else build.build_example_f64()
    r = subprocess.run([exe64], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["pcg_exit"] == 0 and 0 < out["pcg_iters"] < 200 and out["rel_residual"] < 1e-4 and out["smem"] > 0
    # ... and at the BASELINE horizon: pcg<double, 14, 128> = the lane-quad kernel across two CUs behind the same call site (round 5)
    exe128 = build.EXAMPLE_BIN64_N128 if os.path.exists(build.EXAMPLE_BIN64_N128) else build.build_example_f64_n128()
    r = subprocess.run([exe128], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["pcg_exit"] == 0 and out["pcg_iters"] > 0 and out["rel_residual"] < 1e-4 and out["two_threads_two_streams_same_bits"] == 1
    assert out["smem"] == 93504                                   # a member of the clustered lane-quad kernel (mpcg_pcg_lds_bytes_f64)


@pytest.mark.parametrize("waves,reg_rows,lds_rows", [(16, 1, -1), (16, 1, 0), (16, 2, -1), (8, 2, 0), (8, 2, 1), (8, 3, -1), (4, 4, -1), (4, 6, 2), (4, 7, -1)])
@pytest.mark.parametrize("N", [5, 32, 128, 200])
def test_resident_row_variants_bitwise_equal_streaming(P, N, waves, reg_rows, lds_rows):
    """Keeping triples of block rows in registers / LDS across iterations changes where the matrix bytes
    come from, not the arithmetic: every variant that still streams part of the matrices must reproduce the
    streaming kernel of the same wave count bit for bit (reg_rows / lds_rows count TRIPLES per matrix per
    wave).  A variant that keeps EVERYTHING resident uses the other lane order (blocks of a row in adjacent
    lanes, DPP merge): same products and per-row sums, but the inner products are folded over differently
    placed lanes, so it agrees with the streaming kernel to fp32 round-off of two inner products per iteration
    (and bit for bit with itself from run to run)."""
    PcgSolver, pcg_config = P
    B = 3
    k = synth.make_kkt(N, B, 4242 + N)
    S, Pinv, g = synth.form_schur(k, poison_unused=True)
    dS, dP, dg = dev(S), dev(Pinv), dev(g)
    cfg = pcg_config(pcg_exit_tol=1e-5, pcg_max_iter=40)
    outs = []
    resident = False
    kernels_run = set()
    for rr, rl in ((0, 0), (reg_rows, lds_rows), (reg_rows, lds_rows)):
        for pc in ("ss", "jacobi"):
            sol = PcgSolver(N, max_batch=B)
            sol.set_option("pcg_waves", waves)
            sol.set_option("pcg_reg_rows", rr)
            sol.set_option("pcg_lds_rows", rl)
            lam = torch.zeros(B, n * N, device="cuda")
            it, ex = sol.solve(dS, dP, dg, lam, cfg, pc)
            torch.cuda.synchronize()
            lk = last_kernel(sol)        # the variant under test really ran (not the cluster / lane-per-block kernels)
            assert (lk["family"], lk["waves"], lk["reg_rows"], lk["cluster"]) == (0, waves, rr, 0), lk
            # a build without stream code (SB = 0) uses the adjacent-lane order; where no such build is compiled for
            # (waves, reg_rows) the launcher takes the streaming build of the same pair, whose stream is then idle
            resident = lk["stream_bufs"] == 0
            assert (not resident or sol.get_option("pcg_resident")) and (rl < 0 or rr == 0 or lk["lds_rows"] <= rl), lk
            kernels_run.add((lk["reg_rows"], lk["lds_rows"], lk["stream_bufs"], sol.get_option("last_kernel_lds_extra")))
            outs.append((lam.cpu().numpy(), it.cpu().numpy(), ex.cpu().numpy()))
    for a, b in ((outs[2], outs[4]), (outs[3], outs[5])):          # run-to-run determinism of the variant
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    for a, b in ((outs[0], outs[2]), (outs[1], outs[3])):          # variant against the streaming kernel
        if resident:
            assert np.abs(a[1].astype(int) - b[1].astype(int)).max() <= 2
            same = a[1] == b[1]
            assert relinf(a[0][same], b[0][same]) < 2e-2
        else:
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
            np.testing.assert_array_equal(a[2], b[2])
    assert np.isfinite(outs[0][0]).all()
    if N >= 128 and reg_rows > 0:
        # at these horizons every listed variant keeps part of the matrices on chip AND streams the rest: the
        # bitwise branch above compared two genuinely different data paths
        assert not resident and len(kernels_run) == 2, kernels_run


@pytest.mark.parametrize("N,B", [(37, 5), (512, 3)])
@pytest.mark.parametrize("cols", [3, 1])
def test_spmv_mfma_experiment_matches_valu_kernel(P, orc, cols, N, B):
    """BASELINE config 5's MFMA block-GEMV (v_mfma_f32_16x16x4_f32, blocks padded 14->16 in registers):
    same result as the VALU kernel up to fp32 summation order, unwritten blocks never read.  N = 512 is config 5 as written
    ("IIWA-14 N=512 long-horizon, MFMA per-knot block GEMV on"), N = 37 the ragged case."""
    k = synth.make_kkt(N, B, 9)
    S, _, _ = synth.form_schur(k, poison_unused=True)
    x = np.random.default_rng(3).normal(size=(B, n * N)).astype(np.float32)
    sol = P[0](N, max_batch=B)
    y0 = sol.bt_spmv(dev(S), dev(x), cols=cols).cpu().numpy()
    sol.set_option("spmv_mfma", 1)
    y1 = sol.bt_spmv(dev(S), dev(x), cols=cols).cpu().numpy()
    assert np.isfinite(y1).all() and relinf(y1, y0) < 5e-6
    for b in (0, B - 1):
        assert relinf(y1[b], orc.bt_spmv(np.nan_to_num(S[b]).astype(np.float64), x[b], N, cols=cols)) < 5e-6


def test_short_horizon_batches_run_two_trajectories_per_cu(P, orc):
    """The row-pair kernels' policy for N <= 36 (what runs with "pcg_rpl" = 0) with more trajectories than CUs: <4,3,0>, two
    workgroups per CU.  Same solve as the 8-wave kernel up to the summation order of the inner products, and inside the oracle's fp32 band."""
    PcgSolver, pcg_config = P
    N, B = 32, 300
    k = synth.make_kkt(N, B, 1234)
    S, Pinv, g = synth.form_schur(k, poison_unused=True)
    dS, dP, dg = dev(S), dev(Pinv), dev(g)
    cfg = pcg_config(pcg_exit_tol=1e-5, pcg_max_iter=173)
    sol = PcgSolver(N, max_batch=B)
    sol.set_option("pcg_rpl", 0)
    lam = torch.zeros(B, n * N, device="cuda")
    it, ex = sol.solve(dS, dP, dg, lam, cfg, "ss")
    torch.cuda.synchronize()
    lk = last_kernel(sol)
    assert (lk["family"], lk["waves"], lk["reg_rows"], lk["stream_bufs"]) == (0, 4, 3, 0), lk
    assert sol.checkPcgOccupancy() == 2 * sol.get_option("num_cus")
    assert sol.get_option("pcg_waves") == 8      # the handle's own knobs are not rewritten by a solve
    sol8 = PcgSolver(N, max_batch=B)
    sol8.set_option("pcg_waves", 8); sol8.set_option("pcg_reg_rows", 2); sol8.set_option("pcg_lds_rows", 0)
    lam8 = torch.zeros(B, n * N, device="cuda")
    it8, ex8 = sol8.solve(dS, dP, dg, lam8, cfg, "ss")
    torch.cuda.synchronize()
    it, it8, lam, lam8 = it.cpu().numpy(), it8.cpu().numpy(), lam.cpu().numpy(), lam8.cpu().numpy()
    assert np.abs(it.astype(int) - it8.astype(int)).max() <= max(3, int(0.05 * it8.max()))
    for b in (0, 1, 150, 299):
        Sz, Pz = np.nan_to_num(S[b]), np.nan_to_num(Pinv[b])
        lo, hi = fp32_iters_band(orc, Sz, Pz, g[b], np.zeros(n * N, np.float32), N, 173, 1e-5, "ss", trials=4)
        assert 0.93 * lo - 2 <= int(it[b]) <= 1.07 * hi + 2
        r_hip = rel_residual(S[b], g[b], lam[b], N)
        r_cpu = rel_residual(S[b], g[b], orc.pcg(Sz, Pz, g[b], np.zeros(n * N, np.float32), N, 173, 1e-5, "ss")["lam"], N)
        assert r_hip <= 2 * r_cpu + 1e-6


@pytest.mark.parametrize("N", [2, 7, 36, 37, 48, 49, 96, 97, 129, 200, 255, 256, 300, 729])
def test_default_configuration_across_horizons(P, orc, N):
    """Whatever the library picks by itself for a horizon (all-register kernels, LEAN streaming kernel with extra
    LDS slots, cluster kernel, single-workgroup fallback at the LDS limit N=729) solves the same system: 30 fixed
    iterations against the float64 oracle inside the fp32 band, for both preconditioners, and deterministically."""
    PcgSolver, pcg_config = P
    B, K = 3, 30
    k = synth.make_kkt(N, B, 7000 + N)
    S, Pinv, g = synth.form_schur(k, precond="ss", poison_unused=True)
    dS, dP, dg = dev(S), dev(Pinv), dev(g)
    cfg = pcg_config(pcg_exit_tol=0.0, pcg_max_iter=K)
    for pc in ("ss", "jacobi"):
        outs = []
        for rep in range(2):
            sol = PcgSolver(N, max_batch=B)
            lam = torch.zeros(B, n * N, device="cuda")
            it, ex = sol.solve(dS, dP, dg, lam, cfg, pc)
            torch.cuda.synchronize()
            assert (it.cpu().numpy() == K).all() and (ex.cpu().numpy() == 1).all()
            outs.append(lam.cpu().numpy())
        np.testing.assert_array_equal(outs[0], outs[1])
        for b in range(B):
            Sz, Pz = np.nan_to_num(S[b]), np.nan_to_num(Pinv[b])
            r64 = orc.pcg(Sz.astype(np.float64), Pz.astype(np.float64), g[b].astype(np.float64), np.zeros(n * N), N, K, 0.0, pc)
            band = fp32_band(orc, Sz, Pz, g[b], np.zeros(n * N), N, K, pc, r64["lam"])
            assert relinf(outs[0][b], r64["lam"]) <= max(1e-3, 4 * band), (N, pc, b, relinf(outs[0][b], r64["lam"]), band)
