"""CPU: the double settings of schedule, simulate, tracking_error and advance of tests/plant_ref.py — the restatement that checks mpcg_simulate_f64 /
mpcg_advance_horizon_f64 — pinned against the float settings (pinned in tests/test_sim_ref_cpu.py) where the float and the double schedule agree, and
on the one place the reference's double schedule is surprising."""
import math

import numpy as np
import pytest

import iiwa_ref
import plant_ref as P

n, m = P.n, P.m
DT = 1.0 / 64
SS32 = float(np.float32(2e-4))           # the float entry's substep, as a double
# Simulated times [us] at which the float schedule (remainder rounded to float) and the double one (remainder as fmod gives it) are the same schedule at
# substep SS32: ten full substeps and NO remainder; no full substep and a remainder that is a float.
SIM_TEN, SIM_REM = 1999.9999494757503, 122.0703125


def test_the_two_shared_schedules_are_what_they_are_said_to_be():
    assert SIM_TEN * 1e-6 == 10 * SS32 and int(SIM_TEN * 1e-6 / SS32) == 10 and math.fmod(SIM_TEN * 1e-6, SS32) == 0.0
    rem = math.fmod(SIM_REM * 1e-6, SS32)
    assert int(SIM_REM * 1e-6 / SS32) == 0 and rem == 2.0 ** -13 and float(np.float32(rem)) == rem
    for sim in (SIM_TEN, SIM_REM):
        for toff in (0, 15000):
            S, idx, rem, ridx = P.schedule(toff, sim, DT, np.float32(2e-4))
            S64, idx64, rem64, ridx64 = P.schedule(toff, sim, DT, SS32, double=True)
            assert (S, idx, float(rem), ridx) == (S64, idx64, rem64, ridx64) and isinstance(rem64, float)
    assert P.schedule(15000, SIM_TEN, DT, SS32, double=True)[1] == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1]       # time offset 15,000 us: knot 0 to knot 1


@pytest.mark.parametrize("sim", [SIM_TEN, SIM_REM])
@pytest.mark.parametrize("toff", [0, 15000])
def test_simulate_equals_the_float_restatement_on_float_inputs(toff, sim):
    """Both carry the state in float64 through the same substeps: on float-representable inputs and a shared schedule the results are the same bits."""
    M = iiwa_ref.Model()
    rng = np.random.default_rng(5)
    N = 4
    xu = (0.4 * rng.standard_normal((n + m) * N - m)).astype(np.float32)
    xs = (0.4 * rng.standard_normal(n)).astype(np.float32)
    want = P.simulate(M, xs, xu, N, DT, toff, sim, np.float32(2e-4))
    got = P.simulate(M, xs.astype(np.float64), xu.astype(np.float64), N, DT, toff, sim, SS32, double=True)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.abs(got - xs).max() > 1e-6
    for flag in ("recompute_remainder_index", "ignore_crossing"):
        a = P.simulate(M, xs, xu, N, DT, toff, sim, np.float32(2e-4), **{flag: True})
        b = P.simulate(M, xs.astype(np.float64), xu.astype(np.float64), N, DT, toff, sim, SS32, double=True, **{flag: True})
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), flag


def test_double_inputs_are_not_rounded():
    M = iiwa_ref.Model()
    rng = np.random.default_rng(6)
    N = 4
    xu = 0.4 * rng.standard_normal((n + m) * N - m)
    xs = 0.4 * rng.standard_normal(n)
    got = P.simulate(M, xs, xu, N, DT, 0, SIM_TEN, SS32, double=True)
    through_float = P.simulate(M, xs, xu, N, DT, 0, SIM_TEN, np.float32(2e-4))
    assert 0 < np.abs(got - through_float).max() < 1e-6
    assert np.array_equal(P.simulate(M, xs, xu, N, DT, 4000, 0, double=True), xs)


@pytest.mark.parametrize("N,lead,off,done,shift", [(4, 0, 0, 0, True), (4, 3, 5, 0, True), (2, 1, 7, 0, True), (4, 0, 9, 0, True), (4, 0, 2, 7, True), (4, 0, 0, 0, False)])
def test_advance_equals_the_float_restatement_widened(N, lead, off, done, shift):
    """Copies only: on float inputs the three shifted arrays, the offset and the flag are the float advance's, widened."""
    T = N + 6
    rng = np.random.default_rng(100 * N + lead)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    args = [f((n + m) * N - m), f(n * N), f(6 * N), f(n), f(3), f(T, n + m), f(T, 6)]
    want = P.advance(shift, N, *args, T, off, done, lead)
    got = P.advance(shift, N, *[a.astype(np.float64) for a in args], T, off, done, lead, dtype=np.float64)
    for a, b in zip(got[:3], want[:3]):
        assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.astype(np.float64).view(np.uint64))
    assert got[3:5] == want[3:5] and (got[5] is None) == (want[5] is None)
    if got[5] is not None:
        ee, g = args[4].astype(np.float64), args[2].astype(np.float64)
        assert got[5] == (abs(ee[0] - g[0]) + abs(ee[1] - g[1])) + abs(ee[2] - g[2])


def test_the_reference_double_schedule_quirk_is_pinned():
    """ss = 2e-4 (integrator.cuh:304 with T = double) and 2,000 us: the quotient rounds to exactly 10, and fmod is exact — ten times the double 0.0002
    exceeds the double 0.002 — so ten full substeps AND a remainder of almost a whole substep."""
    S, idx, rem, ridx = P.schedule(0, 2000, DT, double=True)
    assert P.SIM_STEP == 2e-4 and 2000 * 1e-6 / 2e-4 == 10.0
    assert S == 10 and idx == [0] * 10 and ridx == 0
    assert rem == 0.00019999999999999996 and repr(rem) == "0.00019999999999999996"
    # the float entry's substep, widened, gives the ten substeps and the float schedule's 5e-11 s
    S, _, rem, _ = P.schedule(0, 2000, DT, SS32, double=True)
    assert S == 10 and abs(rem - 5.052425e-11) < 1e-16


def test_double_tracking_error_of_non_float_goals_differs_from_the_float_one():
    rng = np.random.default_rng(8)
    ee, goal = rng.standard_normal(3), rng.standard_normal(3)
    e64, e32 = P.tracking_error(ee, goal, dtype=np.float64), P.tracking_error(ee, goal)
    assert e64.dtype == np.float64 and e32.dtype == np.float32
    assert e64 == (abs(ee[0] - goal[0]) + abs(ee[1] - goal[1])) + abs(ee[2] - goal[2])
    assert float(e32) != float(e64) and abs(float(e32) - float(e64)) < 1e-6
    assert float(np.float32(e64)) != float(e64)
