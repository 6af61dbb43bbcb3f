"""CPU: tests/clock_ref.py — the restatement that checks mpcg_simulate_clk / mpcg_advance_horizon_clk — pinned on the sequences worked out by hand
for include/mpcsim.cuh:294-352 (the ShiftClock of examples/mpc_closed_loop.cpp) and on tests/plant_ref.py's schedule."""
import math

import numpy as np
import pytest

import clock_ref
import iiwa_ref
import plant_ref as P

n, m = P.n, P.m
DT = 1.0 / 64
# the schedules of tests/test_gpu_clocks.py: the five CASES of tests/test_gpu_simulate.py and a zero-time trajectory
SIX = [(0, 2000), (15000, 2100), (15000, 100), (46000, 2000), (15500, 300), (4000, 0)]


def test_constant_2000us_period_is_the_examples_shift_clock():
    """since accumulates 0.002 per update and first exceeds 1/64 = 0.015625 at the eighth: shifts at updates 7 and 15 (from 0) of 17, the clock
    wrapping in the same update (since > timestep), so `shifted` is 0 again at once and since restarts at fmod(0.016, 0.015625)."""
    c = clock_ref.Clock(DT)
    got, since = [], []
    for _ in range(17):
        got.append(c.update(2000.0))
        since.append(c.since_s)
    assert [u for u, s in enumerate(got) if s] == [7, 15] and c.shifts == 2
    acc = 0.0
    for _ in range(8):
        acc += 2000.0 * 1e-6
    assert since[7] == math.fmod(acc, DT) and abs(since[7] - math.fmod(0.016, 0.015625)) < 1e-15 and c.shifted == 0
    assert c.prev_sim_us == 2000.0
    assert clock_ref.shifts_of(2000.0, 17, DT) == got
    assert clock_ref.threshold(DT) == DT == clock_ref.threshold(DT, np.float64)
    assert clock_ref.threshold(0.01) == float(np.float32(0.01)) != clock_ref.threshold(0.01, np.float64)


def test_a_period_above_the_timestep_shifts_every_update():
    """20,000 us > 15,625 us: the reference's rule moves ONE knot per update, however long the update was (literal)."""
    assert clock_ref.shifts_of(20000.0, 9, DT) == [True] * 9
    c = clock_ref.Clock(DT)
    c.update(20000.0)
    assert c.since_s == math.fmod(20000.0 * 1e-6, DT) and c.shifted == 0


def test_period_zero_never_shifts_and_keeps_the_clock():
    c = clock_ref.Clock(DT, since_s=0.0131, shifted=0, prev_sim_us=0.0)
    assert [c.update(0.0) for _ in range(5)] == [False] * 5
    assert c.state() == (0.0131, 0, 0.0)
    c = clock_ref.Clock(DT, since_s=0.0151, shifted=1)
    assert not c.update(400.0) and c.shifted == 1            # already shifted in this timestep: not again before the wrap
    assert not c.update(400.0) and c.shifted == 0 and c.since_s == math.fmod(0.0151 + 400.0 * 1e-6 + 400.0 * 1e-6, DT)


@pytest.mark.parametrize("toff,sim", SIX)
def test_schedule_agrees_with_sim_ref(toff, sim):
    ss32 = np.float32(2e-4)
    valid, t, S, rem = clock_ref.schedule(toff, sim, ss32, np.float32)
    S0, _, rem0, _ = P.schedule(toff, sim, DT, ss32)
    assert valid and (t, S) == (toff * 1e-6, S0) and rem == float(rem0) and np.float32(rem) == rem0
    valid, t, S, rem = clock_ref.schedule(toff, sim, 2e-4, np.float64)
    S0, _, rem0, _ = P.schedule(toff, sim, DT, 2e-4, double=True)
    assert valid and (t, S) == (toff * 1e-6, S0) and rem == rem0


def test_schedule_refuses_what_is_no_schedule():
    ss = float(np.float32(2e-4))
    for toff, sim in ((float("nan"), 100.0), (100.0, float("nan")), (-1.0, 100.0), (100.0, -1.0), (float("inf"), 100.0), (100.0, float("inf")),
                      (0.0, 65537 * ss * 1e6 * (1 + 1e-12))):
        assert clock_ref.schedule(toff, sim, np.float32(2e-4))[0] is False, (toff, sim)
    assert clock_ref.schedule(0.0, 65536.5 * ss * 1e6, np.float32(2e-4))[:3:2] == (True, 65536)      # the cap is on sim / ss >= 65537


def test_control_update_composes_simulate_and_advance():
    """A zero-time update leaves the state and the clock as they are and copies the start state; an update that crosses the threshold is
    plant_ref.simulate from prev_sim_us followed by plant_ref.advance(shift = 1)."""
    M = iiwa_ref.Model()
    rng = np.random.default_rng(5)
    N, T = 4, 10
    f = lambda *s: (0.3 * rng.standard_normal(s)).astype(np.float32)
    xu, lam, goal, xs, plan, goals = f((n + m) * N - m), f(n * N), f(6 * N), f(n), f(T, n + m), f(T, 6)
    c = clock_ref.Clock(DT, since_s=0.015, prev_sim_us=1500.0)
    x, (xu1, lam1, goal1, off, done, err), shift = clock_ref.control_update(M, N, DT, c, 0.0, np.float32(2e-4), xs, xu, xu, lam, goal, plan, goals, T, 0, 0)
    assert not shift and err is None and off == 0 and np.array_equal(x, xs.astype(np.float64)) and np.array_equal(xu1[:n], xs)
    assert c.state() == (0.015, 0, 0.0)
    c = clock_ref.Clock(DT, since_s=0.015, prev_sim_us=1500.0)
    x, (xu1, lam1, goal1, off, done, err), shift = clock_ref.control_update(M, N, DT, c, 700.0, np.float32(2e-4), xs, xu, xu, lam, goal, plan, goals, T, 0, 0)
    want = P.simulate(M, xs, xu, N, DT, 1500.0, 700.0)
    assert shift and off == 1 and np.array_equal(x, want) and c.shifted == 0 and c.prev_sim_us == 700.0
    ref = P.advance(True, N, xu, lam, goal, want.astype(np.float32), M.ee_pos(want[:7]).astype(np.float32), plan, goals, T, 0, 0)
    assert np.array_equal(xu1, ref[0]) and np.array_equal(lam1, ref[1]) and np.array_equal(goal1, ref[2]) and err == ref[5]
