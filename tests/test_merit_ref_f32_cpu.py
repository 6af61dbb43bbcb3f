"""CPU: the float32 restatement tests/merit_ref_f32.py against the float64 restatement tests/plant_ref.py and on the reference's own trajectory.
This pins the tolerance the tests of `"merit_f32"` = 1 use (tests/test_gpu_merit_f32.py): what plain float arithmetic makes of the merit on exactly
the inputs of those tests.  It needs no device code and passes with or without the option."""
import numpy as np
import pytest

import iiwa_ref
import plant_ref as P
import merit_ref_f32 as mf
from mpcgpu_amd import iiwa


@pytest.fixture(scope="module")
def models():
    M = iiwa_ref.Model()
    return M, mf.Model32(M)


@pytest.mark.parametrize("N,B", mf.SHAPES)
def test_float32_restatement_vs_float64(models, N, B):
    """|float32 - float64| <= 1e-5 max(1, |float64|) — the limit the project gives "kkt_f32" (tests/test_gpu_kkt.py) — on the five shapes and seeds of
    tests/test_gpu_merit.py::case, nine step sizes, mu = 10, xs given.
    Measured worst |f32 - f64| / max(1, |f64|): 2.5e-6 (N = 8, B = 3 and N = 32, B = 2); the others 1.9e-7 .. 8.3e-7: a 4x margin."""
    M, M32 = models
    xu, goals, xs, dz = mf.case_inputs(N, B)
    r = iiwa.r_cost(N)
    want = P.merits(M, xu, dz, mf.STEPS9, P.f32(goals), P.f32(xs), N, mf.MU, cost=P.Cost.plain(iiwa.QD_COST, r))
    got = mf.merits(M32, xu, dz, mf.STEPS9, goals, xs, N, mf.MU, iiwa.QD_COST, r)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"N={N} B={B}: merits {want.min():.3g} .. {want.max():.3g}, worst error of the float32 restatement {err.max():.2e}")
    assert np.isfinite(got).all() and err.max() <= 1e-5, (err.max(), got, want)


@pytest.mark.parametrize("t0,N", P.WINDOWS)
def test_float32_merit_vanishes_on_the_reference_trajectory(models, t0, N):
    """The windows and the bound of tests/test_merit_ref_cpu.py (step size 0, mu = 1, costs 0) in float32.
    Measured 9.6e-6 .. 5.0e-5 against 4.3e-4 / 8.8e-4."""
    _, M32 = models
    xu, goals, xs = P.reference_window(t0, N)
    got = mf.merits(M32, xu[None], None, [0.0], goals[None], xs[None], N, 1.0, 0.0, 0.0)[0, 0]
    print(f"rows {t0}..{t0 + N - 1}: float32 merit {got:.3e}, bound {14 * (N - 1) * 1e-6:.3e}")
    assert 0.0 <= got <= 14 * (N - 1) * 1e-6, got


@pytest.mark.parametrize("N,B,seed", [(8, 3, 19), (32, 2, 43)])
def test_decision_cases_have_no_close_ties(models, N, B, seed):
    """The inputs of tests/test_gpu_merit_f32.py::test_decisions (dz = the seeded perturbation below, eight step sizes, merit_ref = the merit at step
    size 0): in float64 every trajectory's candidates are separated from the winner by more than 2e-5 max(1, |merit|), so that test leaves none out."""
    M, _ = models
    xu, goals, xs, dz = mf.decision_inputs(N, B, seed)
    r = iiwa.r_cost(N)
    host = P.merits(M, xu, dz, [0.0] + mf.STEPS8, P.f32(goals), P.f32(xs), N, mf.MU, cost=P.Cost.plain(iiwa.QD_COST, r))
    for b in range(B):
        assert not mf.close_tie(host[b, 1:], host[b, 0]), (b, host[b])
