"""GPU: Schur formation, dz recovery, the block-tridiagonal direct solve and the CSR emitter at ANY (state_size, control_size) — the
run-time-dimension kernels of mpcgpu_amd/csrc/schur_generic.hip.h behind mpcg_form_schur(_f64) / mpcg_compute_dz(_f64) / mpcg_block_solve —
against the CPU oracle, whose restatement takes (n, m) as parameters: the same operation order on both sides, so the comparison is BIT FOR
BIT, never-written bd slots included.  Option "producers_generic" = 1 sends the tuned 14 x 7 shape through the same kernels."""
import functools

import numpy as np
import pytest
import torch

from mpcgpu_amd import synth
from test_generic_producers_cpu import dense_kkt_solve, make_kkt_nm
from util import relinf

pytestmark = pytest.mark.gpu

FORM_SHAPES = [(1, 1), (4, 1), (6, 3), (13, 5), (14, 3), (17, 17), (32, 8)]
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
RHO = 1e-3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nans(*shape, dtype=np.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=TORCH[dtype])


@functools.lru_cache(maxsize=None)
def case(n, m, N, B, seed, dtype, rho=RHO):
    """Inputs and the oracle's outputs (symmetric-stair and block-Jacobi), computed once per shape and shared; nobody writes to them."""
    import oracle as orc
    k = make_kkt_nm(N, B, seed, n, m)
    packed = synth.pack_kkt_dense(k, dtype)
    G, C, g, c = packed
    ss = [orc.form_schur(G[b], C[b], g[b], c[b], N, dtype(rho), ss=True, n=n, m=m) for b in range(B)]
    jac = [orc.form_schur(G[b], C[b], g[b], c[b], N, dtype(rho), ss=False, n=n, m=m) for b in range(B)]
    return k, packed, ss, jac


def gpu_form(sol, packed, n, m, N, precond, dtype, rho=RHO):
    G, C, g, c = packed
    B = G.shape[0]
    dG = dev(G)
    S, P, gam = nans(B, 3 * n * n * N, dtype=dtype), nans(B, 3 * n * n * N, dtype=dtype), nans(B, n * N, dtype=dtype)
    sol.form_schur(dG, dev(C), dev(g), dev(c), rho, precond, S=S, Pinv=P, gamma=gam, control_size=m)
    torch.cuda.synchronize()
    return S.cpu().numpy(), P.cpu().numpy(), gam.cpu().numpy(), dG.cpu().numpy(), dG


def check_form(sol, n, m, N, B, precond, dtype, seed=7):
    _, packed, ss, jac = case(n, m, N, B, seed, dtype)
    S, P, gam, Ginv, _ = gpu_form(sol, packed, n, m, N, precond, dtype)
    assert sol.get_option("last_schur_chunk") == 0
    want = ss if precond == "ss" else jac
    for b in range(B):
        So, Po, go, Go = want[b]
        np.testing.assert_array_equal(S[b], So)              # NaN == NaN positions included: blocks (0, col 0) and (N-1, col 2)
        np.testing.assert_array_equal(gam[b], go)
        np.testing.assert_array_equal(Ginv[b], Go)
        if precond == "none":
            assert np.isnan(P[b]).all()
        else:
            np.testing.assert_array_equal(P[b], Po)          # block-Jacobi: the off-diagonal blocks stay NaN on both sides


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("precond", ["ss", "jacobi", "none"])
@pytest.mark.parametrize("N", [2, 3, 9])
@pytest.mark.parametrize("n,m", FORM_SHAPES)
def test_form_schur_bit_exact_vs_oracle_at_any_shape(orc, n, m, N, precond, dtype):
    """n = 1 (degenerate loops); 13 and 17 (no divisibility, n^2 no multiple of the workgroup); m = n (the lock-step inversion's boundary);
    (14, 3): the tuned handle with a foreign control size; 32: power-of-two strides; N = 2: first and last block row only."""
    from mpcgpu_amd import PcgSolver
    B = 5
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    check_form(sol, n, m, N, B, precond, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_form_schur_largest_lds_footprint(orc, dtype):
    """(32, 32): 10 n^2 elements of LDS per block row — 84 KiB in double, a launch beyond the kernel's default dynamic-LDS limit."""
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(3, max_batch=5, state_size=32, control_size=32)
    check_form(sol, 32, 32, 3, 5, "ss", dtype)


def test_form_schur_grid_stride_wraps(orc):
    """2048 x 9 block rows of (4, 1): more than num_cus x 64 workgroups, every workgroup walks several rows."""
    from mpcgpu_amd import PcgSolver
    n, m, N, B, reps = 4, 1, 9, 8, 256
    _, packed, ss, _ = case(n, m, N, B, 11, np.float32)
    sol = PcgSolver(N, max_batch=B * reps, state_size=n, control_size=m)
    assert B * reps * N > sol.get_option("num_cus") * 64
    tiled = tuple(np.tile(a, (reps, 1)) for a in packed)
    S, P, gam, Ginv, _ = gpu_form(sol, tiled, n, m, N, "ss", np.float32)
    for got, idx in ((S, 0), (P, 1), (gam, 2), (Ginv, 3)):
        want = np.stack([ss[b][idx] for b in range(B)])
        np.testing.assert_array_equal(got.reshape(reps, B, -1), np.broadcast_to(want, (reps,) + want.shape))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [2, 9])
@pytest.mark.parametrize("n,m", FORM_SHAPES)
def test_compute_dz_bit_exact_vs_oracle_at_any_shape(orc, n, m, N, dtype):
    from mpcgpu_amd import PcgSolver
    B = 5
    _, packed, _, _ = case(n, m, N, B, 7, dtype)
    G, C, g, c = packed
    lam = np.random.default_rng([N, n, m]).standard_normal((B, n * N)).astype(dtype)
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    _, _, _, Ginv, dG = gpu_form(sol, packed, n, m, N, "jacobi", dtype)
    dz = sol.compute_dz(dG, dev(C), dev(g), dev(lam))
    torch.cuda.synchronize()
    dz = dz.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(dz[b], orc.compute_dz(Ginv[b], C[b], g[b], lam[b], N, n=n, m=m))


@pytest.mark.parametrize("n,m", [(40, 10), (64, 64)])
def test_compute_dz_large_shapes_from_uploaded_inverses(orc, n, m):
    """dz recovery serves every state size a handle can have, also where the formation's operands no longer fit the LDS."""
    from mpcgpu_amd import PcgSolver
    N, B = 3, 2
    _, packed, _, jac = case(n, m, N, B, 7, np.float32)
    G, C, g, c = packed
    Ginv = np.stack([jac[b][3] for b in range(B)])
    lam = np.random.default_rng([N, n, m]).standard_normal((B, n * N)).astype(np.float32)
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    dz = sol.compute_dz(dev(Ginv), dev(C), dev(g), dev(lam))
    torch.cuda.synchronize()
    dz = dz.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(dz[b], orc.compute_dz(Ginv[b], C[b], g[b], lam[b], N, n=n, m=m))


@pytest.mark.parametrize("N", [2, 9])
@pytest.mark.parametrize("n", [1, 4, 6, 13, 17, 32, 40, 64])
def test_block_solve_bit_exact_vs_oracle_at_any_state_size(orc, n, N):
    from mpcgpu_amd import PcgSolver
    B, m = 5, max(1, n // 3)
    _, _, _, jac = case(n, m, N, B, 7, np.float32)
    S = np.stack([jac[b][0] for b in range(B)])
    gam = np.stack([jac[b][2] for b in range(B)])
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    lam = sol.block_solve(dev(S), dev(gam))
    torch.cuda.synchronize()
    lam = lam.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(lam[b], orc.block_solve(S[b], gam[b], N, n=n))
        assert relinf(lam[b], orc.direct_solve(S[b], gam[b], N, n=n)) <= 1e-4      # (measured <= 6e-6 on the CPU)


@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("n", [1, 6, 17, 40])
def test_csr_emitter_at_any_state_size(orc, n, N):
    from mpcgpu_amd import PcgSolver, QdldlSolver
    B, m = 3, max(1, n // 3)
    _, _, _, jac = case(n, m, N, B, 7, np.float32)
    S = np.stack([jac[b][0] for b in range(B)])
    gam = np.stack([jac[b][2] for b in range(B)])
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    col_ptr, row_ind = sol.prep_csr()
    val = sol.bd_to_csr_lowertri(dev(S))
    torch.cuda.synchronize()
    Ap, Ai = orc.prep_csr(N, n=n)
    np.testing.assert_array_equal(col_ptr.cpu().numpy(), Ap)
    np.testing.assert_array_equal(row_ind.cpu().numpy(), Ai)
    val = val.cpu().numpy()
    assert val.shape[1] == sol.csr_nnz() == len(Ai)
    ldl = QdldlSolver(N, state_size=n)
    for b in range(B):
        np.testing.assert_array_equal(val[b], orc.bd_to_csr_lowertri(np.nan_to_num(S[b]), N, n=n))
        assert relinf(ldl.solve_host(val[b], gam[b]), orc.direct_solve(S[b], gam[b], N, n=n)) <= 1e-3


@pytest.mark.parametrize("solver", ["pcg", "block_solve"])
@pytest.mark.parametrize("n,m", [(6, 3), (13, 5), (32, 8)])
def test_whole_step_at_a_foreign_shape_vs_float64_kkt_solve(orc, n, m, solver):
    """KKT blocks -> form_schur -> PCG (generic kernel) | block_solve -> compute_dz on the GPU against the dense float64 solve of the
    regularised KKT system (the CPU oracle's own chain: <= 4e-5 on these inputs, so 1e-3 leaves 25x)."""
    from mpcgpu_amd import PcgSolver, pcg_config
    N, B, rho = 16, 2, 1e-1
    k = make_kkt_nm(N, B, 31337, n, m)
    G, C, g, c = synth.pack_kkt_dense(k, np.float32)
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    dG, dC, dg, dc = dev(G), dev(C), dev(g), dev(c)
    S, P, gam = sol.form_schur(dG, dC, dg, dc, rho, "ss")
    if solver == "pcg":
        lam = torch.zeros(B, n * N, device="cuda")
        it, ex = sol.solve(S, P, gam, lam, pcg_config(pcg_exit_tol=1e-9, pcg_max_iter=2000), "ss")
    else:
        lam = sol.block_solve(S, gam)
    dz = sol.compute_dz(dG, dC, dg, lam)
    torch.cuda.synchronize()
    if solver == "pcg":
        assert (ex.cpu().numpy() == 0).all()
    dz, lam = dz.cpu().numpy(), lam.cpu().numpy()
    for b in range(B):
        dz64, lam64, Cm = dense_kkt_solve(k, b, rho)
        errs = relinf(lam[b], lam64), relinf(dz[b], dz64), np.abs(Cm @ dz[b].astype(np.float64) - k.c[b].reshape(-1)).max()
        print(n, m, solver, b, errs)
        assert max(errs) <= 1e-3, errs


@pytest.mark.parametrize("N", [3, 33])
def test_producers_generic_option_gives_the_tuned_bits_at_14_by_7(orc, N):
    from mpcgpu_amd import PcgSolver
    n, m, B = 14, 7, 5
    k = synth.make_kkt(N, B, 808 + N)
    sol = PcgSolver(N, max_batch=B)
    assert sol.get_option("producers_generic") == 0
    outs = {}
    for on in (0, 1):
        sol.set_option("producers_generic", on)
        assert sol.get_option("producers_generic") == on
        res = []
        for dtype in (np.float32, np.float64):
            packed = synth.pack_kkt_dense(k, dtype)
            lam = np.random.default_rng(N).standard_normal((B, n * N)).astype(dtype)
            for precond in ("ss", "jacobi", "none"):
                S, P, gam, Ginv, dG = gpu_form(sol, packed, n, m, N, precond, dtype)
                assert (sol.get_option("last_schur_chunk") == 0) == bool(on)
                res += [S, P, gam, Ginv]
            dz = sol.compute_dz(dG, dev(packed[1]), dev(packed[2]), dev(lam))
            res.append(dz.cpu().numpy())
            if dtype == np.float32:
                res.append(sol.block_solve(dev(np.nan_to_num(S)), dev(gam)).cpu().numpy())
        outs[on] = res
    for a0, a1 in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a0, a1)
    assert np.isfinite(outs[1][-1]).all()


def test_limits_and_messages(orc):
    from mpcgpu_amd import PcgSolver, _lib
    # (40, 10): the oracle's bits or a refusal that names the LDS limit — never a wrong answer
    for dtype in (np.float32, np.float64):
        sol = PcgSolver(3, max_batch=2, state_size=40, control_size=10)
        try:
            check_form(sol, 40, 10, 3, 2, "ss", dtype)
        except _lib.MpcgError as e:
            assert e.code == _lib.MPCG_ERR_UNSUPPORTED and "LDS" in str(e) and "160 KiB" in str(e)
    # (64, 64) in float: 10 n^2 elements are 160 KiB before the vectors
    n, N, B = 64, 2, 1
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=n)
    z = lambda cnt, dt=torch.float32: torch.zeros(B, cnt, device="cuda", dtype=dt)
    with pytest.raises(_lib.MpcgError) as e:
        sol.form_schur(z(2 * n * n * N - n * n), z(2 * n * n * (N - 1)), z(2 * n * N - n), z(n * N), RHO)
    assert e.value.code == _lib.MPCG_ERR_UNSUPPORTED and "LDS" in str(e.value) and "160 KiB" in str(e.value)
    # control_size 0 and state_size + 1
    n, N = 6, 4
    sol = PcgSolver(N, max_batch=B, state_size=n)
    for m in (0, n + 1):
        args = z((n * n + m * m) * N - m * m), z((n * n + n * m) * (N - 1)), z((n + m) * N - m)
        for dt in (torch.float32, torch.float64):
            a = [t.to(dt) for t in args]
            with pytest.raises(_lib.MpcgError) as e:
                sol.form_schur(a[0], a[1], a[2], z(n * N, dt), RHO, control_size=m)
            assert e.value.code == _lib.MPCG_ERR_INVALID and "control_size" in str(e.value)
            with pytest.raises(_lib.MpcgError) as e:
                sol.compute_dz(a[0], a[1], a[2], z(n * N, dt), control_size=m)
            assert e.value.code == _lib.MPCG_ERR_INVALID and "control_size" in str(e.value)
    # what stays n = 14 only says so
    with pytest.raises(_lib.MpcgError) as e:
        sol.bt_spmv(z(3 * n * n * N), z(n * N))
    assert e.value.code == _lib.MPCG_ERR_UNSUPPORTED
    # the option exists on every handle; unknown keys are still refused
    sol.set_option("producers_generic", 1)
    assert sol.get_option("producers_generic") == 1
    with pytest.raises(_lib.MpcgError):
        sol.set_option("producers_generic_", 1)


def test_a_larger_control_size_regrows_the_staging_buffer(orc):
    """The G^-1 staging buffer is sized from the largest control_size seen: a later call with a larger one re-allocates it (outside a capture)."""
    from mpcgpu_amd import PcgSolver
    n, N, B = 6, 3, 5
    sol = PcgSolver(N, max_batch=B, state_size=n)
    for m in (1, 6, 3):
        check_form(sol, n, m, N, B, "ss", np.float32)


def test_generic_chain_replays_from_a_hipgraph_and_first_calls_are_refused_inside_a_capture(orc):
    from mpcgpu_amd import PcgSolver, _lib, pcg_config
    n, m, N, B = 6, 3, 9, 3
    cfg = pcg_config(pcg_exit_tol=1e-9, pcg_max_iter=500)
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    sets = [synth.pack_kkt_dense(make_kkt_nm(N, B, 9000 + s, n, m), np.float32) for s in range(3)]
    zS = lambda: torch.zeros(B, 3 * n * n * N, device="cuda")

    def eager(G, C, g, c):
        dG, dC, dg, dc = dev(G), dev(C), dev(g), dev(c)
        S, P, gam = sol.form_schur(dG, dC, dg, dc, 1e-1, "ss", S=zS(), Pinv=zS())
        lam = torch.zeros(B, n * N, device="cuda")
        it, ex = sol.solve(S, P, gam, lam, cfg, "ss")
        dz = sol.compute_dz(dG, dC, dg, lam)
        lam_d = sol.block_solve(S, gam)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (S, P, gam, dG, lam, it, ex, dz, lam_d)]

    want = [eager(*s) for s in sets]                # also the one eager call of every entry point that sizes the handle's buffers
    assert all((w[6] == 0).all() for w in want)
    inG, inC, ing, inc = (dev(a) for a in sets[0])
    dG = torch.empty_like(inG)
    S, P = zS(), zS()
    gam, lam, lam_d = (torch.empty(B, n * N, device="cuda") for _ in range(3))
    dz = torch.empty(B, (n + m) * N - m, device="cuda")
    it = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex = torch.zeros(B, dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):                   # a linear chain
        dG.copy_(inG)
        lam.zero_()
        sol.form_schur(dG, inC, ing, inc, 1e-1, "ss", S=S, Pinv=P, gamma=gam)
        sol.solve(S, P, gam, lam, cfg, "ss", iters=it, exits=ex)
        sol.compute_dz(dG, inC, ing, lam, dz=dz)
        sol.block_solve(S, gam, lam_d)
    for rep in (1, 2):
        G, C, g, c = sets[rep]
        inG.copy_(dev(G)); inC.copy_(dev(C)); ing.copy_(dev(g)); inc.copy_(dev(c))
        graph.replay()
        torch.cuda.synchronize()
        for got, exp in zip((S, P, gam, dG, lam, it, ex, dz, lam_d), want[rep]):
            np.testing.assert_array_equal(got.cpu().numpy(), exp)
    # a fresh handle's first calls allocate: refused inside a capture, which stays usable
    fresh = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    graph2 = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph2):
        with pytest.raises(RuntimeError, match="outside the stream capture") as e:
            fresh.form_schur(dG, inC, ing, inc, 1e-1, "ss", S=S, Pinv=P, gamma=gam)
        assert e.value.code == _lib.MPCG_ERR_INVALID
        with pytest.raises(RuntimeError, match="outside the stream capture"):
            fresh.block_solve(S, gam, lam_d)
        lam.zero_()
    graph2.replay()
    torch.cuda.synchronize()
    assert (lam == 0).all()
