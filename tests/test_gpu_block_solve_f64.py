"""GPU: the block-tridiagonal direct solve with the sweep in double — mpcg_block_solve_f64 (linsys_t = double) and option
"block_solve_f64" = 1 of the float entry (float S / gamma widened on load, lambda rounded to float once on store) — against the CPU
oracle's restatement of the sweep, which dispatches on the dtype of S: the same operation order on both sides, so every comparison is BIT
FOR BIT.  State size 14 runs the register-resident kernel of csrc/block_solve.hip.h (one trajectory per wavefront at every batch; the
four-per-wavefront layout is not built in double, "block_solve_wide" is not read), every other state size — and 14 under
"producers_generic" = 1 — the run-time-dimension LDS kernel of csrc/schur_generic.hip.h in double."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from mpcgpu_amd import _lib, synth
from test_gpu_generic_producers import case
from util import GOLDEN, relinf

pytestmark = pytest.mark.gpu

n14 = 14


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def system14(N, B=7):
    """Float S / gamma of B trajectories at state size 14 with NaN in the two never-written blocks; shared, nobody writes to them."""
    S, _, g = synth.form_schur(synth.make_kkt(N, B, 6100 + N), poison_unused=True)
    assert S.dtype == np.float32 and np.isnan(S).any()
    return S, g


@functools.lru_cache(maxsize=None)
def generic_system(n, N, dtype, B=5):
    """S / gamma of the oracle's own formation in `dtype` (never-written blocks NaN), as test_gpu_generic_producers.py::case makes them."""
    m = max(1, n // 3)
    _, _, _, jac = case(n, m, N, B, 7, dtype)
    return np.stack([jac[b][0] for b in range(B)]), np.stack([jac[b][2] for b in range(B)])


@functools.lru_cache(maxsize=None)
def want14_f64(N):
    """The oracle's double sweep per trajectory of system14(N), widened."""
    import oracle as orc
    S, g = system14(N)
    return np.stack([orc.block_solve(S[b].astype(np.float64), g[b].astype(np.float64), N) for b in range(S.shape[0])])


# ---- 1. bit for bit against the oracle, state size 14 ----
@pytest.mark.parametrize("N", [2, 3, 9, 33, 128])
def test_f64_bit_exact_vs_oracle_n14(orc, N):
    """B = 7: no multiple of four.  N = 2: a first and a last knot only; N = 3: one interior knot.  The NaN of the two never-written blocks must
    not reach lambda.  (One layout in double: "block_solve_wide" 0 and 1 run the same kernel — asserted equal all the same.)"""
    from mpcgpu_amd import PcgSolver
    S, g = system14(N)
    S64, g64 = S.astype(np.float64), g.astype(np.float64)
    B = S.shape[0]
    sol = PcgSolver(N, max_batch=B)
    lam = sol.block_solve(dev(S64), dev(g64))
    assert lam.dtype == torch.float64
    sol.set_option("block_solve_wide", 0)
    lam0 = host(sol.block_solve(dev(S64), dev(g64)))
    sol.set_option("block_solve_wide", 1)
    lam1 = host(sol.block_solve(dev(S64), dev(g64)))
    lam = host(lam)
    assert np.isfinite(lam).all()
    np.testing.assert_array_equal(lam0, lam)
    np.testing.assert_array_equal(lam1, lam)
    for b in range(B):
        np.testing.assert_array_equal(lam[b], orc.block_solve(S64[b], g64[b], N))


# ---- 2. the same at any state size ----
@pytest.mark.parametrize("N", [2, 9])
@pytest.mark.parametrize("n", [1, 4, 6, 13, 17, 32, 40, 64])
def test_f64_bit_exact_vs_oracle_at_any_state_size(orc, n, N):
    """n = 64: 133,664 bytes of LDS, a launch beyond the kernel's default dynamic-LDS limit."""
    from mpcgpu_amd import PcgSolver
    S, g = generic_system(n, N, np.float64)
    assert S.dtype == np.float64
    B = S.shape[0]
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=max(1, n // 3))
    lam = host(sol.block_solve(dev(S), dev(g)))
    for b in range(B):
        np.testing.assert_array_equal(lam[b], orc.block_solve(S[b], g[b], N, n=n))


@pytest.mark.parametrize("N", [2, 9])
def test_f64_producers_generic_gives_the_register_kernels_bits_n14(orc, N):
    from mpcgpu_amd import PcgSolver
    S, g = system14(N)
    S64, g64 = dev(S.astype(np.float64)), dev(g.astype(np.float64))
    sol = PcgSolver(N, max_batch=S.shape[0])
    lam_reg = host(sol.block_solve(S64, g64))
    sol.set_option("producers_generic", 1)
    lam_gen = host(sol.block_solve(S64, g64))
    np.testing.assert_array_equal(lam_gen, lam_reg)
    np.testing.assert_array_equal(lam_gen, want14_f64(N))


# ---- 3. "block_solve_f64" = 1 on the float entry ----
@pytest.mark.parametrize("n,N", [(14, 2), (14, 9), (14, 33), (6, 9), (17, 9)])
def test_option_float_in_double_inside_float_out(orc, n, N):
    """Widening is exact and there is one rounding: the float result is the oracle's double sweep on the widened data, rounded — bit for bit.
    With the option back at 0 the float sweep's bits return."""
    from mpcgpu_amd import PcgSolver
    S, g = system14(N) if n == 14 else generic_system(n, N, np.float32)
    assert S.dtype == np.float32
    B = S.shape[0]
    sol = PcgSolver(N, max_batch=B, state_size=n, control_size=7 if n == 14 else max(1, n // 3))
    assert sol.get_option("block_solve_f64") == 0
    sol.set_option("block_solve_f64", 1)
    lam = sol.block_solve(dev(S), dev(g))
    assert lam.dtype == torch.float32
    lam = host(lam)
    for b in range(B):
        np.testing.assert_array_equal(lam[b], orc.block_solve(S[b].astype(np.float64), g[b].astype(np.float64), N, n=n).astype(np.float32))
    if n == 14:
        sol.set_option("producers_generic", 1)
        np.testing.assert_array_equal(host(sol.block_solve(dev(S), dev(g))), lam)
        sol.set_option("producers_generic", 0)
    sol.set_option("block_solve_f64", 0)
    lam = host(sol.block_solve(dev(S), dev(g)))
    for b in range(B):
        np.testing.assert_array_equal(lam[b], orc.block_solve(S[b], g[b], N, n=n))


def test_option_takes_0_and_1_only():
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(4, max_batch=1)
    lib = _lib.load()
    assert lib.mpcg_set_option(sol._h, b"block_solve_f64", 1) == _lib.MPCG_OK and sol.get_option("block_solve_f64") == 1
    for bad in (2, -1):
        assert lib.mpcg_set_option(sol._h, b"block_solve_f64", bad) == _lib.MPCG_ERR_INVALID
        assert b"block_solve_f64" in lib.mpcg_last_error(sol._h) and sol.get_option("block_solve_f64") == 1


def test_option_on_the_iiwa_systems_beats_the_float_sweep(orc):
    """tests/golden/iiwa_kkt_N128.npz s0 / s1 (cond 2.3e7 / 1.1e7): the option's result is the oracle expression bit for bit, and its error
    against the float64 direct solve is below the float sweep's on the same data (CPU figures: 3.0e-5 against 2.2e-3, 6.2e-5 against 1.6e-3)."""
    from mpcgpu_amd import PcgSolver
    N = 128
    d = np.load(os.path.join(GOLDEN, "iiwa_kkt_N128.npz"))
    S = np.stack([d["s0_S"], d["s1_S"]])
    g = np.stack([d["s0_gamma"], d["s1_gamma"]])
    sol = PcgSolver(N, max_batch=2)
    sol.set_option("block_solve_f64", 1)
    lam = host(sol.block_solve(dev(S), dev(g)))
    for b in range(2):
        np.testing.assert_array_equal(lam[b], orc.block_solve(S[b].astype(np.float64), g[b].astype(np.float64), N).astype(np.float32))
        x = orc.direct_solve(S[b], g[b], N)
        err, err_f32 = relinf(lam[b], x), relinf(orc.block_solve(S[b], g[b], N), x)
        print(f"s{b}: double inside {err:.3g}, float sweep {err_f32:.3g}")
        assert err < err_f32


# ---- 4. independence and repeatability ----
@pytest.mark.parametrize("route", ["f64", "option"])
def test_batch_equals_single_calls_and_runs_repeat(route):
    from mpcgpu_amd import PcgSolver
    N, B = 9, 5
    S, g = system14(N)
    S, g = S[:B], g[:B]
    sol = PcgSolver(N, max_batch=B)
    if route == "f64":
        S, g = S.astype(np.float64), g.astype(np.float64)
    else:
        sol.set_option("block_solve_f64", 1)
    dS, dg = dev(S), dev(g)
    lam = host(sol.block_solve(dS, dg))
    np.testing.assert_array_equal(host(sol.block_solve(dS, dg)), lam)                 # run against run
    for b in range(B):
        one = host(sol.block_solve(dS[b:b + 1].contiguous(), dg[b:b + 1].contiguous()))
        np.testing.assert_array_equal(one[0], lam[b])


# ---- 5. graphs ----
def test_first_f64_call_is_refused_inside_a_capture_then_captures_and_replays():
    """As the float case of tests/test_gpu_graph.py: the first call allocates the handle's double scratch (hipMalloc: not stream work)."""
    from mpcgpu_amd import PcgSolver
    N = 9
    S, g = system14(N)
    S64, g64 = dev(S.astype(np.float64)), dev(g.astype(np.float64))
    B = S.shape[0]
    sol = PcgSolver(N, max_batch=B)                     # fresh: no double scratch
    lam = torch.zeros(B, n14 * N, device="cuda", dtype=torch.float64)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="outside the stream capture"):
            sol.block_solve(S64, g64, lam)
        lam.zero_()
    graph.replay()
    sol.block_solve(S64, g64, lam)                      # one eager call
    want = host(lam).copy()
    np.testing.assert_array_equal(want, want14_f64(N))
    lam.zero_()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        sol.block_solve(S64, g64, lam)
    assert not host(lam).any()                          # (captured, not run)
    graph2.replay()
    np.testing.assert_array_equal(host(lam), want)


def test_a_captured_float_solve_survives_the_first_f64_call(orc):
    """The double sweeps have a scratch of their own: the float solve's buffer, whose address a captured float solve holds, is not touched."""
    from mpcgpu_amd import PcgSolver
    N = 9
    S, g = system14(N)
    B = S.shape[0]
    dS, dg = dev(S), dev(g)
    sol = PcgSolver(N, max_batch=B)
    lam = torch.zeros(B, n14 * N, device="cuda")
    sol.block_solve(dS, dg, lam)                        # eager: allocates the float scratch
    want = host(lam).copy()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        sol.block_solve(dS, dg, lam)
    graph.replay()
    np.testing.assert_array_equal(host(lam), want)
    lam64 = host(sol.block_solve(dev(S.astype(np.float64)), dev(g.astype(np.float64))))      # the handle's first double call
    np.testing.assert_array_equal(lam64, want14_f64(N))
    sol.set_option("block_solve_f64", 1)                # read when a call is made: the graph keeps what it was captured with
    lam.zero_()
    graph.replay()
    np.testing.assert_array_equal(host(lam), want)
    for b in range(B):
        np.testing.assert_array_equal(want[b], orc.block_solve(S[b], g[b], N))


# ---- 6. errors ----
def test_argument_errors_and_dtype_dispatch():
    from mpcgpu_amd import PcgSolver
    N, B = 3, 2
    S, g = system14(N)
    S64, g64 = dev(S[:B].astype(np.float64)), dev(g[:B].astype(np.float64))
    sol = PcgSolver(N, max_batch=B)
    lib = _lib.load()
    lam = torch.full((B, n14 * N), 7.0, device="cuda", dtype=torch.float64)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    INV, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_OK
    f = lambda S=S64, g=g64, lam=lam, batch=B: lib.mpcg_block_solve_f64(sol._h, p(S), p(g), p(lam), batch, None)
    assert lib.mpcg_block_solve_f64(None, p(S64), p(g64), p(lam), B, None) == INV
    for kw in ({"S": None}, {"g": None}, {"lam": None}):
        assert f(**kw) == INV and b"mpcg_block_solve_f64: null device pointer" in lib.mpcg_last_error(sol._h)
    assert f(S=None, batch=0) == INV                    # the null pointer comes first
    assert f(batch=0) == OK
    assert (host(lam) == 7.0).all()                     # nothing launched
    assert f(batch=B + 1) == INV and b"max_batch" in lib.mpcg_last_error(sol._h)
    assert f() == OK
    np.testing.assert_array_equal(host(lam), want14_f64(N)[:B])
    # PcgSolver.block_solve: float64 tensors no longer raise; mixed or other dtypes are a TypeError
    out = sol.block_solve(S64, g64)
    assert out.dtype == torch.float64
    dS32, dg32 = dev(S[:B]), dev(g[:B])
    with pytest.raises(TypeError):
        sol.block_solve(dS32, g64)
    with pytest.raises(TypeError):
        sol.block_solve(S64, dg32)
    with pytest.raises(TypeError):
        sol.block_solve(S64, g64, torch.empty(B, n14 * N, device="cuda"))
    with pytest.raises(TypeError):
        sol.block_solve(dS32.half(), dg32.half())
    assert sol.block_solve(dS32, dg32).dtype == torch.float32


# ---- 7. the call site ----
def test_cpp_sqp_linsys_chain_direct_with_use_doubles():
    """examples/sqp_linsys_chain.cpp built with -DUSE_DOUBLES, --direct: block_solve_schur<double> over the shim headers; the program checks
    the KKT conditions of the step on the CPU — to 1e-9, the limit tests/test_gpu_schur.py applies to the same binary's PCG route."""
    from mpcgpu_amd import build
    exe64 = build.build_chain_example_f64()
    r = subprocess.run([exe64, "--direct"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    assert out["constraint_err"] < 1e-9 and out["stationarity_err"] < 1e-9, out
