"""Float64 restatement of the step between two SQP solves of the MPC loop — TEST INFRASTRUCTURE, the checker of mpcg_simulate and
mpcg_advance_horizon (mpcgpu_amd/csrc/sim_plant.hip.h).  Built on the pinned pieces of oracle/iiwa_ref.py.

    schedule   the substep schedule of simple_simulate (reference include/common/integrator.cuh:301-324) in IEEE double
    simulate   S Euler substeps of dt = sim_step and a remainder substep, the state carried in float64 (the library's stated departure from the
               reference, which rounds to float after every substep), control indices beyond the last control clamped to N - 2 (the second)
    advance    tracking error, traj_offset, just_shift of xu / goals / lambda with their tail fills, and the start-state copy of simulateMPC
               (include/mpcsim.cuh:300-348) as array operations on one trajectory, in float32 (copies only: nothing is rounded)"""
import math

import numpy as np

import iiwa_ref

n, m = 14, 7
SIM_STEP = np.float32(2e-4)              # integrator.cuh:304


def schedule(toff_us, sim_us, timestep, sim_step=SIM_STEP):
    """(S, [control index of every full substep], float32 remainder, control index of the remainder substep) — indices NOT clamped.
    The remainder keeps the index of the last full substep (the reference does not recompute it, :322-324), or (uint32)(toff / timestep) if S = 0."""
    ss = float(np.float32(sim_step))
    toff, sim = toff_us * 1e-6, sim_us * 1e-6
    S = int(sim / ss)
    idx = [int((toff + s * ss) / timestep) for s in range(S)]
    return S, idx, np.float32(math.fmod(sim, ss)), (idx[-1] if S else int(toff / timestep))


def euler_step(model, x, u, dt):
    """x + dt [qd; qdd] from the old values, qdd = forward dynamics without gravity: iiwa_ref.euler_defect with x_next = 0, negated."""
    return -iiwa_ref.euler_defect(model, x, u, np.zeros(n), dt)


def simulate(model, xs, xu, N, timestep, toff_us, sim_us, sim_step=SIM_STEP, recompute_remainder_index=False, ignore_crossing=False):
    """The new float64 state of ONE trajectory: xs [n], xu [(n+m)N - m] (float32 values, widened).  The two flags give the WRONG alternatives
    a test must be able to tell from the right one: a remainder substep whose index is recomputed at its own time, and a schedule that keeps
    the first index throughout."""
    S, idx, rem, rem_idx = schedule(toff_us, sim_us, timestep, sim_step)
    ss = float(np.float32(sim_step))
    if recompute_remainder_index:
        rem_idx = int((toff_us * 1e-6 + S * ss) / timestep)
    if ignore_crossing:
        first = int(toff_us * 1e-6 / timestep)
        idx, rem_idx = [first] * S, first
    x = np.asarray(xs, np.float32).astype(np.float64)
    xu = np.asarray(xu, np.float32).astype(np.float64)
    control = lambda i: xu[min(i, N - 2) * (n + m) + n:min(i, N - 2) * (n + m) + n + m]
    for i in idx:
        x = euler_step(model, x, control(i), ss)
    if rem != 0:
        x = euler_step(model, x, control(rem_idx), float(rem))
    return x


def tracking_error(ee, goal0):
    """(|ee0 - g0| + |ee1 - g1|) + |ee2 - g2| in float32, in that order (mpcsim.cuh:303-306)."""
    ee, g = np.asarray(ee, np.float32), np.asarray(goal0, np.float32)
    d = np.abs(ee[:3] - g[:3])
    return np.float32(np.float32(d[0] + d[1]) + d[2])


def advance(shift, N, xu, lam, goal, xs, ee, xu_traj, ee_traj, traj_steps, traj_offset, done, lead=0):
    """mpcg_advance_horizon on ONE trajectory.  xu [(n+m)N - m], lam [n N], goal [6 N], xs [n], ee [3], xu_traj [traj_steps, n+m], ee_traj
    [traj_steps, 6] float32.  Returns new (xu, lam, goal, traj_offset, done, tracking error or None); the inputs are not modified."""
    xu, lam, goal = (np.array(a, np.float32, copy=True).reshape(-1) for a in (xu, lam, goal))
    nm = n + m
    if done:
        return xu, lam, goal, traj_offset, done, None
    if not shift:
        xu[:n] = xs
        return xu, lam, goal, traj_offset, done, None
    plan, goals = np.asarray(xu_traj, np.float32).reshape(-1), np.asarray(ee_traj, np.float32).reshape(-1)
    err = tracking_error(ee, goal[:3])
    off = traj_offset + 1
    inside = off + N < traj_steps
    new_xu = xu.copy()
    new_xu[:len(xu) - nm] = xu[nm:]                           # knots 1..N-2 whole, then x_{N-1} alone: the last moved knot carries no control
    if inside:
        new_xu[len(xu) - nm:] = plan[nm * (off + lead) - m:nm * (off + lead) - m + nm]
    else:
        new_xu[len(xu) - nm:] = 0.0
        new_xu[len(xu) - n:len(xu) - n + n // 2] = plan[(traj_steps - 1) * nm:(traj_steps - 1) * nm + n // 2]
    new_goal = np.concatenate([goal[6:], goals[6 * ((off + N - 1) if inside else (traj_steps - 1)):][:6]])
    new_lam = np.concatenate([lam[n:], lam[-n:]])             # the last knot keeps its value
    new_xu[:n] = xs
    return new_xu, new_lam, new_goal, off, (1 if off >= traj_steps else 0), err
