"""GPU: Schur formation, dz recovery, the direct solves, the CSR emitters and the half-precision conversion inside a guard-banded arena
(tests/arena.py), every case in both layouts and bit for bit against the same call on separately allocated tensors — the calls
tests/test_gpu_schur.py, tests/test_gpu_generic_producers.py, tests/test_gpu_f64.py and tests/test_gpu_rho.py pin to the oracle bit for bit.

What the masks state (include/mpcg.h): blocks (0, left) and (N-1, right) of d_S and d_Pinv are written by NO routing of mpcg_form_schur;
MPCG_PRECOND_JACOBI leaves every off-diagonal block of d_Pinv alone, MPCG_PRECOND_NONE all of d_Pinv; d_G is rewritten whole."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arena
import arena_specs as A
import generic_pcg_cases as gc
from mpcgpu_amd import synth
from test_generic_producers_cpu import make_kkt_nm

pytestmark = pytest.mark.gpu
B = A.B
RHO = 1e-3
RHOS = [1e-3, 0.5, 10.0, 3e-2, 1.7]                     # (tests/test_gpu_rho.py's: one rho per trajectory)
ROUTING_OPTS = {"auto": {}, "chunk1": {"schur_chunk": 1}, "chunk3": {"schur_chunk": 3}, "lds": {"schur_dpp": 0}, "generic": {"producers_generic": 1}}
ROUTING_CHUNK = {"chunk1": 1, "chunk3": 3, "lds": 0, "generic": 0}
PRECS = ("f32", "f64")


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def kkt(prec, n, m, N, Bt):
    """(G, C, g, c), read-only and shared: 14 x 7 from synth.make_kkt (tests/test_gpu_schur.py), other shapes from make_kkt_nm."""
    k = synth.make_kkt(N, Bt, 555 + N) if (n, m) == (14, 7) else make_kkt_nm(N, Bt, 7, n, m)
    out = synth.pack_kkt_dense(k, A.DT[prec])
    for a in out:
        a.flags.writeable = False
    return out


def solver(n, m, N, Bt, opts):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=Bt, state_size=n, control_size=m)
    for key, value in opts.items():
        sol.set_option(key, value)
    return sol


def schur_call(sol, m, Bt, pc, rho):
    def call(a):
        v = lambda name: a[name].view(Bt, -1)
        sol.form_schur(v("G"), v("C"), v("g"), v("c"), a["rho"] if rho is None else rho, pc, S=v("S"), Pinv=v("Pinv"), gamma=v("gamma"),
                       control_size=m)
    return call


def form(prec, n, m, N, pc, rhov, routing, mode):
    G, Cd, g, c = kkt(prec, n, m, N, B)
    sol = solver(n, m, N, B, ROUTING_OPTS[routing])
    inputs = {"G": G, "C": Cd, "g": g, "c": c}
    if rhov:
        inputs["rho"] = np.array(RHOS, A.DT[prec])
    tag = f"form_schur {prec} {n}x{m} N={N} {pc} rhov={rhov} {routing}"
    out = arena.both_ways(A.form_schur(prec, n, m, N, B, pc, rhov), mode, inputs, schur_call(sol, m, B, pc, None if rhov else RHO), tag)
    chunk = sol.get_option("last_schur_chunk")
    if (n, m) != (14, 7):
        assert chunk == 0, (tag, chunk)
    elif routing == "auto":
        assert chunk >= 1, (tag, chunk)
    else:
        assert chunk == ROUTING_CHUNK[routing], (tag, chunk)
    assert out["G"].tobytes() != np.ascontiguousarray(G).tobytes(), tag          # rewritten: the inverses
    return out


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("rhov", [False, True], ids=["rho", "rhov"])
@pytest.mark.parametrize("pc", A.PRECONDS)
@pytest.mark.parametrize("routing", A.SCHUR_ROUTINGS)
@pytest.mark.parametrize("N", A.SCHUR_N)
@pytest.mark.parametrize("prec", PRECS)
def test_form_schur_14x7_every_routing(prec, N, routing, pc, rhov, mode):
    """mpcg_form_schur, _rhov, _f64, _rhov_f64 at 14 x 7 with B = 5: N = 9 under "schur_chunk" = 3 is three chunks with a ragged last one, 15
    chunks for wavefronts of four; N = 2 is the first and the last block row alone."""
    form(prec, 14, 7, N, pc, rhov, routing, mode)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", A.SCHUR_N)
def test_form_schur_routings_write_the_same_elements(prec, N):
    """Every routing leaves blocks (0, left) and (N-1, right) of S and Pinv alone (the masks above) — and all of them give the same bits."""
    outs = [form(prec, 14, 7, N, "ss", False, routing, "minimal") for routing in A.SCHUR_ROUTINGS]
    for other in outs[1:]:
        for name in ("S", "Pinv", "gamma", "G"):
            assert other[name].tobytes() == outs[0][name].tobytes(), (prec, N, name)


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("rhov", [False, True], ids=["rho", "rhov"])
@pytest.mark.parametrize("pc", A.PRECONDS)
@pytest.mark.parametrize("n,m", A.GENERIC_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_form_schur_generic_shapes(prec, n, m, pc, rhov, mode):
    """The run-time-dimension kernels at the shapes of tests/test_gpu_generic_producers.py, N = 2 (their smallest)."""
    form(prec, n, m, 2, pc, rhov, "auto", mode)


@functools.lru_cache(maxsize=None)
def inverses(prec, n, m, N, Bt):
    """G^-1 as the formation leaves it (an ordinary call), for the dz cases."""
    G, Cd, g, c = kkt(prec, n, m, N, Bt)
    sol = solver(n, m, N, Bt, {})
    dG = torch.from_numpy(G.copy()).cuda()
    sol.form_schur(dG, *(torch.from_numpy(np.array(a)).cuda() for a in (Cd, g, c)), RHO, "jacobi", control_size=m)
    torch.cuda.synchronize()
    return dG.cpu().numpy()


def dz(prec, n, m, N, Bt, opts, mode):
    _, Cd, g, _ = kkt(prec, n, m, N, Bt)
    lam = np.random.default_rng([N, n, m]).standard_normal((Bt, n * N)).astype(A.DT[prec])
    sol = solver(n, m, N, Bt, opts)

    def call(a):
        v = lambda name: a[name].view(Bt, -1)
        sol.compute_dz(v("Ginv"), v("C"), v("g"), v("lambda"), dz=v("dz"), control_size=m)
    arena.both_ways(A.compute_dz(prec, n, m, N, Bt), mode, {"Ginv": inverses(prec, n, m, N, Bt), "C": Cd, "g": g, "lambda": lam}, call,
                    f"compute_dz {prec} {n}x{m} N={N} B={Bt} {opts}")


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("dz_dpp", [1, 0])
@pytest.mark.parametrize("N,Bt", [(5, 1), (3, B)])
@pytest.mark.parametrize("prec", PRECS)
def test_compute_dz_14x7(prec, N, Bt, dz_dpp, mode):
    """mpcg_compute_dz(_f64): four knots per wavefront ("dz_dpp" = 1; N = 5 with one trajectory leaves a ragged second wavefront, 15 knots a
    ragged fourth) and the LDS kernel."""
    dz(prec, 14, 7, N, Bt, {"dz_dpp": dz_dpp}, mode)


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("n,m", A.GENERIC_SHAPES)
@pytest.mark.parametrize("prec", PRECS)
def test_compute_dz_generic_shapes(prec, n, m, mode):
    dz(prec, n, m, 2, B, {}, mode)


@functools.lru_cache(maxsize=None)
def schur_system(prec, n, N):
    if n == 14:
        S, _, g = synth.form_schur(synth.make_kkt(N, B, 31 + N), dtype=A.DT[prec], poison_unused=True)
    else:
        S, _, g = gc.system(n, 5, N, B, gc.SEED, A.DT[prec], RHO, "ss")
    return S, g


BLOCK_SOLVES = [("f32", 14, 9, {"block_solve_wide": 0}), ("f32", 14, 9, {"block_solve_wide": 1}),
                ("f32", 14, 9, {"block_solve_wide": 0, "block_solve_f64": 1}), ("f32", 14, 9, {"block_solve_wide": 1, "block_solve_f64": 1}),
                ("f64", 14, 9, {}), ("f32", 14, 2, {"block_solve_wide": 0}), ("f64", 14, 2, {}),
                ("f32", 14, 9, {"producers_generic": 1}), ("f64", 14, 9, {"producers_generic": 1}), ("f32", 13, 2, {}), ("f64", 13, 2, {})]


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("prec,n,N,opts", BLOCK_SOLVES, ids=[f"{p}-n{n}-N{N}-" + "-".join(f"{k}{v}" for k, v in o.items()) for p, n, N, o in BLOCK_SOLVES])
def test_block_solve(prec, n, N, opts, mode):
    """mpcg_block_solve / _f64: four trajectories per wavefront ("block_solve_wide" = 0: B = 5 leaves three dead rows in the second wavefront,
    which redo the last trajectory and store nothing) and one; float64 inside; the run-time-dimension kernel.  S carries NaN in the two
    never-read blocks, d_lambda is output only."""
    S, g = schur_system(prec, n, N)
    sol = solver(n, 7 if n == 14 else 5, N, B, opts)

    def call(a):
        sol.block_solve(a["S"].view(B, -1), a["gamma"].view(B, -1), a["lambda"].view(B, -1))
    arena.both_ways(A.block_solve(prec, n, N, B), mode, {"S": S, "gamma": g}, call, f"block_solve {prec} n={n} N={N} {opts}")


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("n,N", [(14, 9), (13, 2)])
def test_csr_pattern_values_and_the_host_ldl_solve(n, N, mode):
    """mpcg_prep_csr, mpcg_bd_to_csr_lowertri and mpcg_qdldl_solve_schur (trajectory 0; its D2H / H2D copies are the accesses checked)."""
    from mpcgpu_amd import QdldlSolver
    S, g = schur_system("f32", n, N)
    sol = solver(n, 7 if n == 14 else 5, N, B, {})
    lib, h = sol.lib, sol._h
    pattern = arena.both_ways(A.prep_csr(n, N), mode, {}, lambda a: sol._check(lib.mpcg_prep_csr(h, ptr(a["col_ptr"]), ptr(a["row_ind"]), stream())),
                              f"prep_csr n={n} N={N}")
    q = QdldlSolver(N, n)
    assert np.array_equal(pattern["col_ptr"], q.col_ptr) and np.array_equal(pattern["row_ind"], q.row_ind)
    val = arena.both_ways(A.bd_to_csr(n, N, B), mode, {"S": S},
                          lambda a: sol._check(lib.mpcg_bd_to_csr_lowertri(h, ptr(a["S"]), ptr(a["val"]), 1.0, B, stream())),
                          f"bd_to_csr_lowertri n={n} N={N}")["val"].reshape(B, -1)
    arena.both_ways(A.qdldl(n, N), mode, {"val": val[0], "gamma": g[0]}, lambda a: q.solve_schur(sol, a["val"], a["gamma"], a["lambda"]),
                    f"qdldl_solve_schur n={n} N={N}")


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("count", A.CONVERT_COUNTS)
def test_convert_f32_to_f16_stops_at_count(count, mode):
    """mpcg_convert_f32_to_f16: eight elements per lane and a scalar tail; the tail must stop at count (the band behind d_dst stays 0xFF, the
    NaN behind d_src is never converted into it).  Both pointers at 16 (mod 32) in the minimal layout."""
    sol = solver(14, 7, 8, 1, {})
    src = (100.0 * np.random.default_rng(count).standard_normal(count)).astype(np.float32)
    out = arena.both_ways(A.convert(count), mode, {"src": src},
                          lambda a: sol._check(sol.lib.mpcg_convert_f32_to_f16(sol._h, ptr(a["src"]), ptr(a["dst"]), count, stream())),
                          f"convert {count}")
    assert out["dst"].tobytes() == src.astype(np.float16).tobytes()              # round to nearest even, as numpy's


@pytest.mark.parametrize("mode", arena.MODES)
def test_probe_hbm_read_writes_nothing(mode):
    """mpcg_probe_hbm_read: d_src (16-byte aligned, in the minimal layout at 16 mod 32) comes back intact and d_sink keeps its value."""
    sol = solver(14, 7, 8, 1, {})
    src = np.random.default_rng(3).standard_normal(A.PROBE_FLOATS).astype(np.float32)
    out = arena.both_ways(A.probe(), mode, {"src": src, "sink": [7.0]},
                          lambda a: sol._check(sol.lib.mpcg_probe_hbm_read(sol._h, ptr(a["src"]), 4 * A.PROBE_FLOATS, ptr(a["sink"]), stream())), "probe_hbm_read")
    assert out["sink"].tolist() == [7.0]


# ---- the torch-backed arena sees what the device did: defects planted with torch kernels fail, and name the array ----
def _fake(defect):
    def call(a):
        a["y"].copy_(2 * a["x"])
        defect(a)
    return call


def _grow(t, before, after):
    """The tensor's elements with `before` more in front and `after` more behind: the same memory, as a kernel with a wrong bound sees it."""
    return torch.as_strided(t, (before + t.numel() + after,), (1,), t.storage_offset() - before)


GPU_DEFECTS = [("past the end", lambda a: _grow(a["y"], 0, 1)[-1:].fill_(1.0), "after array 'y'"),
               ("before the start", lambda a: _grow(a["y"], 1, 0)[:1].fill_(1.0), "before array 'y'"),
               ("an input changed", lambda a: a["x"][3:4].mul_(2.0), "input array 'x'"),
               ("an element left unwritten", lambda a: a["y"][5:6].fill_(float("nan")).view(torch.int32).fill_(-1), "array 'y'"),
               ("read past an input", lambda a: a["y"][-1:].add_(0.0 * _grow(a["x"], 0, 1)[-1:]), "array 'y'")]


@pytest.mark.parametrize("mode", arena.MODES)
def test_planted_defects_on_the_device_are_caught(mode):
    specs = [arena.spec("x", np.float32, 37, "in"), arena.spec("y", np.float32, 37, "out")]
    x = np.random.default_rng(1).standard_normal(37).astype(np.float32)
    ar = arena.Arena(specs, mode, "torch")
    ar.put("x", x)
    assert ar.run(_fake(lambda a: None))["y"].tobytes() == (2 * x).tobytes()
    for what, defect, names in GPU_DEFECTS:
        ar = arena.Arena(specs, mode, "torch")
        ar.put("x", x)
        with pytest.raises(AssertionError) as e:
            ar.run(_fake(defect))
        assert names in str(e.value), (what, str(e.value))
