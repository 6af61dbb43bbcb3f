"""CPU: schedule, simulate and advance of tests/plant_ref.py — the float64 restatement that checks mpcg_simulate / mpcg_advance_horizon — pinned: the schedule on values worked out by
hand, the integration on the reference's own trajectory file, the horizon shift on a literal per-memcpy transcription of include/mpcsim.cuh:300-348."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import iiwa_ref
import plant_ref as P

n, m = P.n, P.m
DT = 1.0 / 64


def test_schedule_pinned_values():
    ss = np.float32(2e-4)
    S, idx, rem, ridx = P.schedule(0, 2000, float(np.float32(1 / 64)), ss)
    assert (S, idx, ridx) == (10, [0] * 10, 0) and rem.dtype == np.float32
    assert abs(float(rem) - 5.052425e-11) < 1e-16            # 2e-3 - 10 float32(2e-4): the float step is a little short of 2e-4
    S, idx, rem, ridx = P.schedule(15000, 2100, DT, ss)
    assert (S, idx, ridx) == (10, [0, 0, 0, 0, 1, 1, 1, 1, 1, 1], 1) and rem == np.float32(1.0000005e-4)
    S, idx, rem, ridx = P.schedule(15000, 100, DT, ss)
    assert (S, idx, ridx) == (0, [], 0) and rem == np.float32(1e-4)
    S, idx, rem, ridx = P.schedule(46000, 2000, DT, ss)                      # beyond the last control of N = 4: the clamp case
    assert (S, idx, ridx) == (10, [2] * 5 + [3] * 5, 3)
    S, idx, rem, ridx = P.schedule(0, 15625, DT, np.float32(1 / 64))
    assert (S, idx, ridx) == (1, [0], 0) and rem == 0.0


def test_simulate_reproduces_the_reference_trajectory():
    """One call with sim_step = sim_time = 1/64 is one Euler step of 1/64: the 656 in-segment transitions of the reference's own file, within the
    5e-6 tests/test_iiwa_plant.py holds euler_defect to (the 9 seam transitions are no dynamics: in_segment_transitions)."""
    M = iiwa_ref.Model()
    xu = np.load(os.path.join(GOLDEN, "iiwa_traj_0_0_full.npz"))["xu"]
    good = iiwa_ref.in_segment_transitions(xu.shape[0])
    assert len(good) == 656
    worst = 0.0
    for t in good:
        plan = np.concatenate([xu[t], xu[t + 1, :n]])
        got = P.simulate(M, xu[t, :n], plan, 2, DT, 0, 15625, np.float32(1 / 64))
        worst = max(worst, np.abs(got - xu[t + 1, :n]).max())
    assert worst < 5e-6, worst


def test_simulate_substeps_and_clamp():
    """Ten substeps and a remainder move the state as ONE Euler step of the same length does, to first order; an index beyond the last control
    reads the last control."""
    M = iiwa_ref.Model()
    rng = np.random.default_rng(3)
    N = 4
    xu = (0.3 * rng.standard_normal((n + m) * N - m)).astype(np.float32)
    xs = xu[:n].copy()
    fine = P.simulate(M, xs, xu, N, DT, 0, 2000)
    coarse = P.step(M, xs.astype(np.float64), xu[n:n + m].astype(np.float64), 2e-3)
    assert 0 < np.abs(fine - coarse).max() < 1e-4
    clamped = P.simulate(M, xs, xu, N, DT, 46000, 2000)
    same_u = xu.copy()
    same_u[n:n + m] = xu[2 * (n + m) + n:3 * (n + m)]
    np.testing.assert_array_equal(clamped, P.simulate(M, xs, same_u, N, DT, 0, 2000, ignore_crossing=True))


def literal_advance(N, xu, lam, goal, xs, ee, xu_traj, ee_traj, traj_steps, traj_offset):
    """include/mpcsim.cuh:300-348 memcpy by memcpy (just_shift: include/common/integrator.cuh:258-263), on flat float32 arrays, in place."""
    state_size, control_size, knot_points = n, m, N
    traj_len = (state_size + control_size) * knot_points - control_size

    def memcpy(dst, d0, src, s0, count):
        dst[d0:d0 + count] = src[s0:s0 + count].copy()

    def just_shift(ss_, cs_, arr):
        for knot in range(knot_points - 1):
            stepsize = ss_ + (cs_ if knot < knot_points - 2 else 0)
            memcpy(arr, knot * (ss_ + cs_), arr, (knot + 1) * (ss_ + cs_), stepsize)

    cur = np.float32(0.0)
    for i in range(3):
        cur = np.float32(cur + np.abs(np.float32(ee[i] - goal[i])))
    traj_offset += 1
    just_shift(state_size, control_size, xu)
    if traj_offset + knot_points < traj_steps:
        memcpy(xu, traj_len - (state_size + control_size), xu_traj, (state_size + control_size) * traj_offset - control_size, state_size + control_size)
    else:
        memcpy(xu, traj_len - state_size, xu_traj, (traj_steps - 1) * (state_size + control_size), state_size // 2)
        xu[traj_len - state_size // 2:traj_len] = 0
        xu[traj_len - (state_size + control_size):traj_len - state_size] = 0
    just_shift(6, 0, goal)
    if traj_offset + knot_points < traj_steps:
        memcpy(goal, (knot_points - 1) * 6, ee_traj, (traj_offset + knot_points - 1) * 6, 6)
    else:
        memcpy(goal, (knot_points - 1) * 6, ee_traj, (traj_steps - 1) * 6, 6)
    just_shift(state_size, 0, lam)
    memcpy(xu, 0, xs, 0, state_size)
    return traj_offset, cur


@pytest.mark.parametrize("N", [2, 3, 4, 7])
def test_advance_is_the_reference_memcpy_sequence(N):
    rng = np.random.default_rng(N)
    T = N + 6
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    plan, goals = f(T * (n + m)), f(T * 6)
    for off0 in range(T):                                     # inside the plan, the else branch from off0 + 1 + N == T on, the last shift
        xu, lam, goal, xs, ee = f((n + m) * N - m), f(n * N), f(6 * N), f(n), f(3)
        want_xu, want_lam, want_goal = xu.copy(), lam.copy(), goal.copy()
        want_off, want_err = literal_advance(N, want_xu, want_lam, want_goal, xs, ee, plan, goals, T, off0)
        got = P.advance(True, N, xu, lam, goal, xs, ee, plan, goals, T, off0, 0)
        for a, b in zip(got[:3], (want_xu, want_lam, want_goal)):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        assert got[3] == want_off and got[4] == (1 if want_off == T else 0)
        assert got[5].dtype == np.float32 and got[5] == want_err
        # the aligned fill row differs from the reference's only in the tail of xu, and only inside the plan
        lead = P.advance(True, N, xu, lam, goal, xs, ee, plan, goals, T, off0, 0, lead=N - 1)
        if off0 + 1 + N < T:
            o = (n + m) * (off0 + N) - m
            np.testing.assert_array_equal(lead[0][-(n + m):], plan[o:o + n + m])
            np.testing.assert_array_equal(lead[0][:-(n + m)], got[0][:-(n + m)])
        else:
            np.testing.assert_array_equal(lead[0], got[0])
    # shift = 0: the start-state copy alone; done != 0: nothing at all
    xu, lam, goal, xs, ee = f((n + m) * N - m), f(n * N), f(6 * N), f(n), f(3)
    got = P.advance(False, N, xu, lam, goal, xs, ee, plan, goals, T, 1, 0)
    np.testing.assert_array_equal(got[0], np.concatenate([xs, xu[n:]]))
    assert np.array_equal(got[1], lam) and np.array_equal(got[2], goal) and got[3:] == (1, 0, None)
    for shift in (False, True):
        got = P.advance(shift, N, xu, lam, goal, xs, ee, plan, goals, T, 1, 5)
        assert np.array_equal(got[0], xu) and np.array_equal(got[1], lam) and np.array_equal(got[2], goal) and got[3:] == (1, 5, None)
