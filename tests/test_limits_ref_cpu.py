"""CPU: the limits argument of tests/plant_ref.py, the float64 restatement of the soft-limits penalty (include/mpcg.h, LIMITS), against itself — the central differences of its own
cost sum are its q_k, r_k away from the bounds, the diagonal indicators are where the violations are, nothing moves when nothing is violated — and the new
symbols in the built library and in include/mpcg.h."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import iiwa_ref
import plant_ref as P
from mpcgpu_amd import iiwa

n, m, NJ, ROW = 14, 7, 7, 21
COST = P.Cost(0.0, 0.5, 2.0 ** -6, 2.0 ** -7, P.QD_RELATIVE | P.U_RELATIVE)
NO_DYNAMICS = lambda N: (np.zeros(0), np.zeros(ROW * N - m), np.zeros(0))          # ee_cost = 0: g needs no dynamics


def thirds(vals):
    """Bounds at the lower and upper third of each column of vals [rows, 7], nudged off every value."""
    s = np.sort(vals, axis=0)
    if len(s) < 2:                                             # one row: it lies below
        return s[0] + 0.5, s[0] + 1.0
    k = max(1, len(s) // 3)
    return 0.5 * (s[k - 1] + s[k]), 0.5 * (s[-k - 1] + s[-k])


def make(N, seed):
    xu, _, xs = iiwa.random_windows(N, 1, seed)
    xu = xu[0].astype(np.float64)
    x, u = P.split(xu, N)
    q_lo, q_hi = thirds(x[:, :NJ])
    qd_lo, qd_hi = thirds(x[:, NJ:])
    u_lo, u_hi = thirds(u)
    q_lo[2], u_lo[4] = -np.inf, -np.inf                       # one-sided
    lim = P.Limits(q_lo, q_hi, qd_lo, qd_hi, u_lo, u_hi, 3.0, 0.25, 0.125)
    plan = 0.5 * np.random.default_rng(seed).standard_normal((N + 1, ROW))
    return xu, xs[0], P.plan_rows(plan, 0, 0, N, N + 1), lim


def test_viol_is_strict_and_ignores_nan():
    lo, hi = np.array([-1.0, -np.inf, 0.0]), np.array([1.0, 2.0, np.inf])
    assert np.array_equal(P.viol([1.0, 2.0, 0.0], lo, hi), [0, 0, 0])                      # on a bound
    assert np.array_equal(P.viol([1.5, -1e30, -0.25], lo, hi), [0.5, 0, -0.25])
    assert np.array_equal(P.viol([np.nan, np.nan, np.nan], lo, hi), [0, 0, 0])
    assert np.array_equal(P.viol([np.inf, -np.inf, np.inf], lo, hi), [np.inf, 0, 0])
    assert np.array_equal(P.side([1.5, 0.0, -3.0], lo, hi), [1, 0, -1])


@pytest.mark.parametrize("N", [4, 9])
def test_central_differences_of_the_cost_sum_are_q_and_r(N):
    """ee_cost = 0: the cost sum is piecewise quadratic in xu; further than h from every bound its central differences are g of generate_kkt."""
    xu, xs, rows, lim = make(N, 30 + N)
    x, u = P.split(xu, N)
    h = 1e-5
    gap = min(np.abs(x[:, None] - np.stack([lim.x_lo, lim.x_hi])[None]).min(), np.abs(u[:, None] - np.stack([lim.u_lo, lim.u_hi])[None]).min())
    assert gap > 2 * h
    for name, vals, lo, hi in (("x", x, lim.x_lo, lim.x_hi), ("u", u, lim.u_lo, lim.u_hi)):
        s = P.side(vals, lo, hi)
        assert all((s == v).any() for v in (-1, 0, 1)), name
    g = P.generate_kkt(None, xu, None, xs, N, rows=rows, cost=COST, limits=lim, base=NO_DYNAMICS(N))[2]
    J = lambda z: P.joint_cost(z, rows, N, COST) + P.penalty(z, N, lim)
    num = np.array([(J(xu + h * e) - J(xu - h * e)) / (2 * h) for e in np.eye(len(xu))])
    assert np.abs(num - g).max() <= 1e-9 * max(1.0, np.abs(g).max())
    plain = P.generate_kkt(None, xu, None, xs, N, rows=rows, cost=COST, base=NO_DYNAMICS(N))[2]
    assert np.abs(g - plain).max() > 1e-3                       # (the penalty is in there)


@pytest.mark.parametrize("N", [2, 6])
def test_diagonal_indicators(N):
    """G gains w on exactly the diagonal entries whose variable violates a bound, and nothing off the diagonal; g gains w viol; C and c are those without limits."""
    xu, xs, rows, lim = make(N, 50 + N)
    G, _, g, _ = P.generate_kkt(None, xu, None, xs, N, rows=rows, cost=COST, limits=lim, base=NO_DYNAMICS(N))
    G0, _, g0, _ = P.generate_kkt(None, xu, None, xs, N, rows=rows, cost=COST, base=NO_DYNAMICS(N))
    x, u = P.split(xu, N)
    dG, dg = G - G0, g - g0
    for k in range(N):
        Q = dG[(n * n + m * m) * k:(n * n + m * m) * k + n * n].reshape(n, n)
        out = P.side(x[k], lim.x_lo, lim.x_hi) != 0
        assert np.array_equal(Q, np.diag(np.where(out, lim.x_weight, 0.0)))
        assert np.allclose(dg[ROW * k:ROW * k + n], lim.x_weight * P.viol(x[k], lim.x_lo, lim.x_hi), rtol=0, atol=1e-15)
        if k < N - 1:
            R = dG[(n * n + m * m) * k + n * n:(n * n + m * m) * (k + 1)].reshape(m, m)
            assert np.array_equal(R, np.diag(np.where(P.side(u[k], lim.u_lo, lim.u_hi) != 0, lim.u_weight, 0.0)))
    assert (dG != 0).any()


def test_nothing_violated_or_no_weight_changes_nothing():
    N = 5
    xu, xs, rows, lim = make(N, 77)
    base = P.generate_kkt(None, xu, None, xs, N, rows=rows, cost=COST, base=NO_DYNAMICS(N))
    wide = P.Limits(-100.0, 100.0, -1e3, None, None, 1e4, 3.0, 0.25, 0.125)
    zero = P.Limits(lim.q_lo, lim.q_hi, lim.qd_lo, lim.qd_hi, lim.u_lo, lim.u_hi, 0.0, 0.0, 0.0)
    for lm in (P.Limits(), wide, zero):
        got = P.generate_kkt(None, xu, None, xs, N, rows=rows, cost=COST, limits=lm, base=NO_DYNAMICS(N))
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[2], base[2])
        assert P.penalty(xu, N, lm) == 0.0
    bad = xu.copy()
    bad[3] = np.nan
    assert P.penalty(bad, N, P.Limits(-1.0, 1.0, q_weight=1.0)) == P.penalty(np.where(np.isnan(bad), 0.0, bad), N, P.Limits(-1.0, 1.0, q_weight=1.0))


def test_rounded_to_float():
    lim = P.Limits(0.1, 0.7, None, 1 / 3, -np.inf, np.inf, 0.1, 0.2, 0.3).rounded_to_float()
    assert lim.q_lo[0] == float(np.float32(0.1)) and lim.qd_hi[6] == float(np.float32(1 / 3)) and lim.qd_lo[0] == -np.inf and lim.u_weight == float(np.float32(0.3))


def test_symbols_in_the_library_and_in_the_header(hiplib):
    from mpcgpu_amd import _lib
    lib = hiplib
    hdr = open(os.path.join(ROOT, "include", "mpcg.h")).read()
    for name in ("mpcg_plant_clone_limits", "mpcg_plant_get_limits"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+MPCG_LIMITS_SIM_SATURATE\s+1u", hdr) and _lib.MPCG_LIMITS_SIM_SATURATE == 1
    import ctypes as C
    assert C.sizeof(_lib.mpcg_limits) == 6 * 7 * 8 + 3 * 8 + 8          # 42 bounds, 3 weights, the flags padded to 8
