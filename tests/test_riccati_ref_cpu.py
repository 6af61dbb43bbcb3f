"""CPU: the reference of mpcg_riccati_gains (tests/riccati_ref.py) pinned before a GPU is involved — it IS the feedback law of the QP the two
linear solvers solve, float64 arithmetic is enough for it on every case the GPU tests use — and the second symbol table
(include/mpcg_riccati.h, _lib.SYMBOLS_RICCATI)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import riccati_ref as rr
from conftest import ROOT
from mpcgpu_amd import synth
from riccati_ref import feedback_residuals as _feedback_residuals, kkt_cond as _kkt_cond, perturbed as _perturbed
from test_abi import _abi_class_c, _abi_class_ctypes
from test_generic_producers_cpu import dense_kkt_solve, make_kkt_nm

HEADER = os.path.join(ROOT, "include", "mpcg_riccati.h")
ENTRIES = ["mpcg_riccati_gains", "mpcg_riccati_gains_f64"]
QP_SHAPES = [(14, 7, 9), (6, 3, 5), (17, 17, 4), (1, 1, 3)]


@pytest.mark.parametrize("n,m,N", QP_SHAPES)
def test_reference_is_the_feedback_law_of_the_qp(orc, n, m, N):
    """Two solves of the regularised QP that differ in c of knot 1: the difference obeys du_k = K_k dx_k and the dynamics for every k >= 1 —
    by a dense float64 solve of the KKT system, and through the project's own pipeline in double (Schur formation, direct solve, dz).
    Tolerance 64 cond(KKT) 2.2e-16, the condition number computed here."""
    rho = rr.RHO
    k0 = make_kkt_nm(N, 1, 900 + N, n, m)
    k1 = _perturbed(k0, 901)
    G, Cd, g, c0 = synth.pack_kkt_dense(k0, np.float64)
    c1 = synth.pack_kkt_dense(k1, np.float64)[3]
    K = rr.gains(G[0], Cd[0], n, m, N, rho, np.float64)
    dz0, _, Cm = dense_kkt_solve(k0, 0, rho)
    dz1, _, _ = dense_kkt_solve(k1, 0, rho)
    cond = _kkt_cond(k0, rho, Cm)
    tol = 64 * cond * rr.EPS64
    res = _feedback_residuals(dz0, dz1, K, k0)
    print(f"({n},{m},{N}) cond(KKT) {cond:.3g} tol {tol:.3g}: dense solve, feedback {res[0]:.3g} dynamics {res[1]:.3g}")
    assert max(res) <= tol, (res, tol)

    def pipeline(c):
        S, _, gam, Ginv = orc.form_schur(G[0], Cd[0], g[0], c, N, np.float64(rho), ss=False, n=n, m=m)
        lam = orc.direct_solve(S, gam, N, n=n)
        return orc.compute_dz(Ginv, Cd[0], g[0], lam, N, n=n, m=m)
    res = _feedback_residuals(pipeline(c0[0]), pipeline(c1[0]), K, k0)
    print(f"({n},{m},{N}) pipeline in double, feedback {res[0]:.3g} dynamics {res[1]:.3g}")
    assert max(res) <= tol, (res, tol)


@pytest.mark.parametrize("n,m,N,B", rr.ALL_CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_gpu_cases_have_small_e_ref(n, m, N, B, dtype):
    """Every synthetic case of tests/test_gpu_riccati.py, as the double entry sees it and as the float entry does (inputs rounded to float):
    float64 against 80-bit arithmetic on the same inputs stays under 6e-11, so 16 x e_ref there never admits an error above 1e-9."""
    G, Cd = rr.make_case(n, m, N, B, dtype)
    worst = 0.0
    for b in range(B):
        e, K64 = rr.e_ref(G[b], Cd[b], n, m, N, rr.RHO)
        assert np.isfinite(K64).all()
        worst = max(worst, e)
    print(f"({n},{m},{N},{B}) {np.dtype(dtype).name}: e_ref {worst:.3g}")
    assert worst < rr.E_REF_MAX


def test_spd_solve_both_dtypes():
    rng = np.random.default_rng(5)
    for dtype, tol in ((np.float64, 1e-13), (np.longdouble, 1e-16)):
        V = rng.standard_normal((7, 7))
        H = (V @ V.T + 7 * np.eye(7)).astype(dtype)
        Y = rng.standard_normal((7, 14)).astype(dtype)
        X = rr.spd_solve(H, Y)
        assert X.dtype == dtype and np.abs(H @ X - Y).max() <= tol * np.abs(Y).max() * 10


# ---- the second table ----
def _header_text():
    return open(HEADER).read()


def _declared():
    src = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(mpcg_[a-z0-9_]+)\s*\(", src)))


def _prototypes():
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S))
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(mpcg_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        assert name not in protos, name
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        protos[name] = (_abi_class_c(ret), [_abi_class_c(p) for p in params])
    return protos


def test_second_header_parses_and_matches_the_second_table():
    """include/mpcg_riccati.h under the regular expressions tests/test_abi.py reads include/mpcg.h with: exactly the two entries, each row of
    _lib.SYMBOLS_RICCATI of the prototype's ABI classes, none of them in _lib.SYMBOLS (whose count test_abi.py pins)."""
    from mpcgpu_amd import _lib
    protos = _prototypes()
    assert _declared() == sorted(protos) == sorted(ENTRIES) == sorted(_lib.SYMBOLS_RICCATI)
    assert not set(ENTRIES) & set(_lib.SYMBOLS)
    assert '#include "mpcg.h"' in _header_text()
    for name, (res, args) in _lib.SYMBOLS_RICCATI.items():
        assert (_abi_class_ctypes(res), [_abi_class_ctypes(a) for a in args]) == protos[name], name
    f32, f64 = protos["mpcg_riccati_gains"], protos["mpcg_riccati_gains_f64"]
    assert f32[1][4] == "f32" and f64[1][4] == "f64" and [a for i, a in enumerate(f32[1]) if i != 4] == [a for i, a in enumerate(f64[1]) if i != 4]


def test_second_table_exported_and_bound(hiplib):
    from mpcgpu_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in ENTRIES:
        assert name in exported
        fn = getattr(hiplib, name)
        assert fn.argtypes == _lib.SYMBOLS_RICCATI[name][1] and fn.restype is C.c_int
    assert hiplib.mpcg_abi_version() == 2


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_handle_is_refused_by_name(hiplib, entry):
    """The one MPCG_ERR_INVALID row that needs no device (a handle cannot exist without one: tests/test_abi.py::test_no_gpu_fails_loudly); the
    rest of the table is tests/test_gpu_riccati.py's."""
    from mpcgpu_amd import _lib
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    assert getattr(hiplib, entry)(None, 7, p, p, 1e-3, None, p, 1, None) == _lib.MPCG_ERR_INVALID
    msg = hiplib.mpcg_last_error(None).decode()
    assert msg.startswith(entry + ":"), msg
    assert all(v == 0 for v in buf)


def test_python_surface():
    import mpcgpu_amd
    assert "gain_blocks" in mpcgpu_amd.__all__ and callable(mpcgpu_amd.PcgSolver.riccati_gains)
    import torch
    n, m, N, B = 5, 2, 4, 3
    K = torch.arange(B * (N - 1) * m * n, dtype=torch.float64).reshape(B, -1)
    V = mpcgpu_amd.gain_blocks(K, n, m)
    assert V.shape == (B, N - 1, m, n) and V.data_ptr() == K.data_ptr()
    assert V[1, 2, 1, 3] == K[1, 2 * m * n + 3 * m + 1]       # column-major m x n blocks, leading dimension m
