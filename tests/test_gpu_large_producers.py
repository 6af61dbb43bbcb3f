"""GPU: Schur formation and dz recovery on either side of their route switch at 2^31 bytes, formation with S past 2^32 bytes, and
mpcg_bt_spmv, mpcg_block_solve(_f64), mpcg_bd_to_csr_lowertri and mpcg_convert_f32_to_f16 past 2^32 bytes — tests/large_extents.py: a few
distinct trajectories tiled over the batch on the device, every tile of every output bit for bit the call on the distinct ones, which is held
to the oracle bit for bit here as in tests/test_gpu_schur.py, test_gpu_f64.py, test_gpu_rho.py and test_gpu_block_solve_f64.py.

Sizes: formation float N = 22, B = 41,502 / 41,503 (S 4,160 bytes below / 47,584 past 2^31), double N = 20,
B = 22,826 / 22,827 (13,568 below / 80,512 past); two 16-row chunks per trajectory below the line, so the seam kernel runs.  dz float N = 27,
B = 67,633 / 67,634 (knots x 1,176 bytes: 632 below / 31,120 past), double N = 22, B = 41,502 / 41,503 (4,160 below / 47,584 past)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import large_extents as le
from mpcgpu_amd import synth

pytestmark = pytest.mark.gpu
RHO = 1e-3
RHOS = [1e-3, 0.5, 10.0, 3e-2, 1.7]                     # (tests/test_gpu_rho.py's: one rho per trajectory)
DT = le.A.DT


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def solver(N, B, opts=()):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=B)
    for key, value in dict(opts).items():
        sol.set_option(key, value)
    return sol


@functools.lru_cache(maxsize=None)
def kkt(prec, N, D):
    out = synth.pack_kkt_dense(synth.make_kkt(N, D, 555 + N), DT[prec])
    for a in out:
        a.flags.writeable = False
    return out


def unmasked(spec, name):
    a = next(a for a in spec.arrays if a.name == name)
    return slice(None) if a.mask is None else ~a.mask


def form_call(sol, pc, rhov):
    def call(a, Bt):
        sol.form_schur(a["G"], a["C"], a["g"], a["c"], a["rho"].view(-1) if rhov else RHO, pc, S=a["S"], Pinv=a["Pinv"], gamma=a["gamma"])
    return call


def form_inputs(prec, N, D, rhov):
    G, Cd, g, c = kkt(prec, N, D)
    inputs = {"G": G, "C": Cd, "g": g, "c": c}
    if rhov:
        inputs["rho"] = np.array(RHOS[:D], DT[prec]).reshape(D, 1)
    return inputs


def form_against_the_oracle(orc, spec, prec, N, pc, rhov, inputs, out):
    """The call on D trajectories: the oracle's bits in every element the call writes (tests/test_gpu_schur.py, test_gpu_f64.py, test_gpu_rho.py)."""
    dt = DT[prec]
    for d in range(spec.D):
        rho = dt(RHOS[d]) if rhov else dt(RHO)
        So, Po, go, Go = orc.form_schur(inputs["G"][d], inputs["C"][d], inputs["g"][d], inputs["c"][d], N, rho, ss=(pc == "ss"))
        for name, want in (("S", So), ("Pinv", Po), ("gamma", go), ("G", Go)):
            m = unmasked(spec, name)
            np.testing.assert_array_equal(out[name][d][m], np.asarray(want).reshape(-1)[m], err_msg=f"{spec.label} {name} trajectory {d}")


FORM_SPECS = le.form_specs()


@pytest.mark.parametrize("spec", FORM_SPECS, ids=[s.label for s in FORM_SPECS])
def test_form_schur_either_side_of_2_31_and_past_2_32(orc, spec):
    """mpcg_form_schur(_rhov)(_f64): below the line the chunk-walking and the seam kernel with offsets in the top of their 31-bit range
    ("last_schur_chunk" = 16, two chunks), past it and past 2^32 bytes of S the LDS kernels and their max_batch-sized staging buffer
    ("last_schur_chunk" = 0) — the bits of the call on D trajectories, which runs one row per chunk, and of the oracle.  The first call of a
    handle on the LDS route allocates: inside a stream capture it is refused, not run."""
    _, prec, pc, rv, Ntag, Btag, *side = spec.label.split()
    N, rhov, below = int(Ntag[1:]), rv == "rhov", side == ["below", "2^31"]
    sol = solver(N, spec.B)
    inputs = form_inputs(prec, N, spec.D, rhov)

    def refused_in_a_capture(big, before, small):
        fresh = solver(N, spec.B)
        sm = {k: v.clone() for k, v in before.items()}
        form_call(fresh, pc, rhov)(sm, spec.D)                       # the register-resident route's buffer exists: only the staging buffer is missing
        torch.cuda.synchronize()
        assert fresh.get_option("last_schur_chunk") == 1
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sm["gamma"].zero_()                                      # (something to capture)
            with pytest.raises(RuntimeError, match="beyond the 31-bit offsets.*outside the stream capture"):
                form_call(fresh, pc, rhov)(big, spec.B)
        torch.cuda.synchronize()
        G = next(a for a in spec.arrays if a.name == "G")
        le.compare_tiled(G, big["G"], small["G"], spec.D, spec.B, "after the refused call: a second formation would have inverted it again", label=spec.label)
        fresh.close()
    capture = (prec, pc, below, spec.B < 50000) == ("f32", "ss", False, True)
    out = le.run(spec, inputs, form_call(sol, pc, rhov), refused_in_a_capture if capture else None)
    chunk = sol.get_option("last_schur_chunk")
    assert chunk == (16 if below else 0), (spec.label, chunk)
    sol.close()
    form_against_the_oracle(orc, spec, prec, N, pc, rhov, inputs, out)


@functools.lru_cache(maxsize=None)
def inverses(prec, N, D):
    """G^-1 as the formation leaves it (an ordinary call), for the dz cases."""
    G, Cd, g, c = kkt(prec, N, D)
    sol = solver(N, D)
    dG = torch.from_numpy(G.copy()).cuda()
    sol.form_schur(dG, *(torch.from_numpy(np.array(a)).cuda() for a in (Cd, g, c)), RHO, "jacobi")
    torch.cuda.synchronize()
    sol.close()
    return dG.cpu().numpy()


DZ_SPECS = le.dz_specs()


@pytest.mark.parametrize("spec", DZ_SPECS, ids=[s.label for s in DZ_SPECS])
def test_compute_dz_either_side_of_2_31(orc, spec):
    """mpcg_compute_dz(_f64): four knots per wavefront below the line ("last_dz_route" = 1), the LDS kernel past it (0); the oracle's bits."""
    _, prec, Ntag, Btag, *side = spec.label.split()
    N, below = int(Ntag[1:]), side == ["below", "2^31"]
    _, Cd, g, _ = kkt(prec, N, spec.D)
    Ginv = inverses(prec, N, spec.D)
    lam = np.random.default_rng([N, 14, 7]).standard_normal((spec.D, 14 * N)).astype(DT[prec])
    sol = solver(N, spec.B)
    out = le.run(spec, {"Ginv": Ginv, "C": Cd, "g": g, "lambda": lam},
                 lambda a, Bt: sol.compute_dz(a["Ginv"], a["C"], a["g"], a["lambda"], dz=a["dz"]))
    assert sol.get_option("last_dz_route") == (1 if below else 0), spec.label
    sol.compute_dz(*(torch.from_numpy(np.array(a)).cuda() for a in (Ginv, Cd, g, lam)))
    assert sol.get_option("last_dz_route") == 1                      # (the same handle, D trajectories: back on the four-knot route)
    sol.close()
    for d in range(spec.D):
        np.testing.assert_array_equal(out["dz"][d], orc.compute_dz(Ginv[d], Cd[d], g[d], lam[d], N), err_msg=f"{spec.label} trajectory {d}")


# ---- S past 2^32 bytes: mpcg_bt_spmv, mpcg_block_solve(_f64), mpcg_bd_to_csr_lowertri ----
@functools.lru_cache(maxsize=None)
def schur_system(prec, N, D):
    """(S, gamma) with NaN in the two never-read blocks, as tests/test_gpu_arena_producers.py's."""
    S, _, g = synth.form_schur(synth.make_kkt(N, D, 31 + N), dtype=DT[prec], poison_unused=True)
    S.flags.writeable = g.flags.writeable = False
    return S, g


@pytest.mark.parametrize("cols", [3, 1])
def test_bt_spmv_past_2_32(orc, cols):
    """mpcg_bt_spmv: one buffer resource per trajectory from a 64-bit base, x and y as flat [batch N][14] arrays indexed in long."""
    from util import relinf
    spec = le.spmv_spec(cols)
    N = le.LINALG_N
    S, _ = schur_system("f32", N, spec.D)
    M = np.nan_to_num(S)                                             # (cols = 3 multiplies the out-of-matrix blocks by the zero padding of x: keep them finite)
    x = np.random.default_rng(cols).standard_normal((spec.D, 14 * N)).astype(np.float32)
    sol = solver(N, spec.B)
    out = le.run(spec, {"M": M, "x": x}, lambda a, Bt: sol.bt_spmv(a["M"], a["x"], a["y"], cols))
    sol.close()
    for d in range(spec.D):                                          # tests/test_gpu_parity.py's limit against the float64 oracle
        assert relinf(out["y"][d], orc.bt_spmv(M[d].astype(np.float64), x[d].astype(np.float64), N, cols=cols)) < 5e-6, (cols, d)


@pytest.mark.parametrize("prec,opts", le.BLOCK_SOLVES, ids=[f"{p}-" + ("-".join(f"{k}{v}" for k, v in o.items()) or "default") for p, o in le.BLOCK_SOLVES])
def test_block_solve_past_2_32(orc, prec, opts):
    """mpcg_block_solve with four trajectories and one per wavefront, with the double sweep inside, and mpcg_block_solve_f64 — each with its
    max_batch-sized sweep scratch (1.5 GB in float, 3.1 GB in double) indexed next to S.  The oracle's bits (tests/test_gpu_schur.py,
    test_gpu_block_solve_f64.py)."""
    spec = le.block_solve_spec(prec, opts)
    N = le.LINALG_N
    S, g = schur_system(prec, N, spec.D)
    sol = solver(N, spec.B, tuple(opts.items()))
    out = le.run(spec, {"S": S, "gamma": g}, lambda a, Bt: sol.block_solve(a["S"], a["gamma"], a["lambda"]))
    sol.close()
    for d in range(spec.D):
        if opts.get("block_solve_f64"):
            want = orc.block_solve(S[d].astype(np.float64), g[d].astype(np.float64), N).astype(np.float32)
        else:
            want = orc.block_solve(S[d], g[d], N)
        np.testing.assert_array_equal(out["lambda"][d], want, err_msg=f"{spec.label} trajectory {d}")


def test_bd_to_csr_lowertri_past_2_32(orc):
    spec = le.csr_spec()
    N = le.LINALG_N
    S, _ = schur_system("f32", N, spec.D)
    sol = solver(N, spec.B)
    out = le.run(spec, {"S": S}, lambda a, Bt: sol._check(sol.lib.mpcg_bd_to_csr_lowertri(sol._h, ptr(a["S"]), ptr(a["val"]), 1.0, Bt, stream())))
    sol.close()
    for d in range(spec.D):
        np.testing.assert_array_equal(out["val"][d], orc.bd_to_csr_lowertri(np.nan_to_num(S[d]), N), err_msg=f"trajectory {d}")


def test_convert_f32_to_f16_past_2_31_elements():
    """count = 2^31 + 13: the element index passes int, the source 2^33 bytes, the destination 2^32 bytes, and the ragged tail (five elements)
    is the last thread's.  Reference: torch.Tensor.half() on the same data, slice by slice; the 0xFF behind the destination's last element stays."""
    count = le.CONVERT_COUNT
    need = le.convert_need()
    assert need <= le.CAP_BYTES
    free = torch.cuda.mem_get_info()[0]
    if free < 1.5 * need:
        pytest.skip(f"convert: needs {need} bytes of device memory (x 1.5 = {int(1.5 * need)}), {free} are free")
    sol = solver(8, 1)
    step = le.SLICE_BYTES // 4
    base = (100.0 * torch.randn(step + 12345, device="cuda")).float()            # not a divisor of anything: slices start at varying phases of it
    src = torch.empty(count + 8, dtype=torch.float32, device="cuda")
    for i0 in range(0, count + 8, step):
        i1 = min(count + 8, i0 + step)
        src[i0:i1] = base[(i0 // step) % 12345:][:i1 - i0]
    dst = torch.full((2 * (count + 8),), le.FILL, dtype=torch.uint8, device="cuda").view(torch.float16)
    keep = src[:4096].clone(), src[-4096:].clone()
    sol._check(sol.lib.mpcg_convert_f32_to_f16(sol._h, ptr(src), ptr(dst), count, stream()))
    torch.cuda.synchronize()
    for i0 in range(0, count, step):
        i1 = min(count, i0 + step)
        if not torch.equal(dst[i0:i1].view(torch.int16), src[i0:i1].half().view(torch.int16)):
            bad = int((dst[i0:i1].view(torch.int16) != src[i0:i1].half().view(torch.int16)).nonzero()[0, 0]) + i0
            raise AssertionError(f"array 'dst': first difference at element {bad}, byte offset {2 * bad} (mod 2^31: {2 * bad % 2 ** 31}, mod 2^32: {2 * bad % 2 ** 32}); "
                                 f"source byte offset {4 * bad}")
    assert (dst[count:].view(torch.int16) == -1).all(), "written past count"
    assert torch.equal(keep[0], src[:4096]) and torch.equal(keep[1], src[-4096:])
    for i0 in range(0, count, step):                                 # the source, slice by slice, still the pattern it was filled with
        i1 = min(count, i0 + step)
        assert torch.equal(src[i0:i1], base[(i0 // step) % 12345:][:i1 - i0]), f"array 'src' modified in elements {i0}..{i1}"
    sol.close()
    del src, dst, base
    torch.cuda.empty_cache()


# ---- the checker sees what the device did: wraps at 2^31 bytes planted with torch on the device fail, and name the array ----
def test_planted_wraps_on_the_device_are_caught():
    T, B, D = 1021, 525877, 3                                            # 4 T B = 2^31 + 198,020 bytes; B no multiple of 3 or 4
    spec = le.Spec("planted", [le.arr("x", np.float32, T, "in"), le.arr("y", np.float32, T, "out")], D, B, 0)
    assert 4 * T * B > 2 ** 31 and 4 * T * (B - 64) < 2 ** 31
    x = np.random.default_rng(1).standard_normal((D, T)).astype(np.float32)
    W = 2 ** 31 // 4                                                     # elements

    def kernel(defect):
        def call(a, Bt):
            a["y"].copy_(2 * a["x"])
            if Bt * T > W:
                xf, yf = a["x"].view(-1), a["y"].view(-1)
                if defect == "load offset wraps":
                    yf[W:] = 2 * xf[:Bt * T - W]
                elif defect == "store dropped":
                    yf[W:].view(torch.int32).fill_(-1)
        return call
    out = le.run(spec, {"x": x}, kernel(None))
    assert out["y"].tobytes() == (2 * x).tobytes()
    for defect, says in (("load offset wraps", "holds"), ("store dropped", "never written")):
        with pytest.raises(AssertionError) as e:
            le.run(spec, {"x": x}, kernel(defect))
        text = str(e.value)
        assert "array 'y'" in text and f"byte offset {2 ** 31} (mod {2 ** 31}: 0" in text and says in text, text
        torch.cuda.empty_cache()
