"""Float64 restatement of the step between two SQP solves for linsys_t = double — TEST INFRASTRUCTURE, the checker of mpcg_simulate_f64 and
mpcg_advance_horizon_f64 (mpcgpu_amd/csrc/sim_plant.hip.h).  tests/sim_ref.py with every float32 replaced by float64 and the reference's schedule
with T = double (include/common/integrator.cuh:301-324):

    schedule        ss = sim_step as a double (NOT passed through float), S = (uint32)(sim / ss), idx_s = (uint32)((toff + s ss) / timestep), and the
                    remainder fmod(sim, ss) as a DOUBLE.  At the reference's 2e-4 and 2,000 us that is S = 10 AND a remainder of
                    0.00019999999999999996 (ten times the double 0.0002 exceeds the double 0.002): reproduced literally.
    simulate        the substeps of that schedule on float64 inputs used as they are (sim_ref.euler_step), indices clamped to N - 2
    tracking_error  (|ee0 - g0| + |ee1 - g1|) + |ee2 - g2| in float64, in that order
    advance         sim_ref.advance's array operations in float64 (copies only)"""
import math

import numpy as np

import sim_ref

n, m = sim_ref.n, sim_ref.m
SIM_STEP = 2e-4                          # integrator.cuh:304 with T = double


def schedule(toff_us, sim_us, timestep, sim_step=SIM_STEP):
    """(S, [control index of every full substep], float64 remainder, control index of the remainder substep) — indices NOT clamped."""
    ss = float(sim_step)
    toff, sim = toff_us * 1e-6, sim_us * 1e-6
    S = int(sim / ss)
    idx = [int((toff + s * ss) / timestep) for s in range(S)]
    return S, idx, math.fmod(sim, ss), (idx[-1] if S else int(toff / timestep))


def simulate(model, xs, xu, N, timestep, toff_us, sim_us, sim_step=SIM_STEP, recompute_remainder_index=False, ignore_crossing=False):
    """The new float64 state of ONE trajectory: xs [n], xu [(n+m)N - m] float64, used as they are.  The two flags give the WRONG alternatives of
    sim_ref.simulate."""
    S, idx, rem, rem_idx = schedule(toff_us, sim_us, timestep, sim_step)
    ss = float(sim_step)
    if recompute_remainder_index:
        rem_idx = int((toff_us * 1e-6 + S * ss) / timestep)
    if ignore_crossing:
        first = int(toff_us * 1e-6 / timestep)
        idx, rem_idx = [first] * S, first
    x = np.array(xs, np.float64)
    xu = np.asarray(xu, np.float64)
    control = lambda i: xu[min(i, N - 2) * (n + m) + n:min(i, N - 2) * (n + m) + n + m]
    for i in idx:
        x = sim_ref.euler_step(model, x, control(i), ss)
    if rem != 0:
        x = sim_ref.euler_step(model, x, control(rem_idx), rem)
    return x


def tracking_error(ee, goal0):
    ee, g = np.asarray(ee, np.float64), np.asarray(goal0, np.float64)
    d = np.abs(ee[:3] - g[:3])
    return np.float64(np.float64(d[0] + d[1]) + d[2])


def advance(shift, N, xu, lam, goal, xs, ee, xu_traj, ee_traj, traj_steps, traj_offset, done, lead=0):
    """mpcg_advance_horizon_f64 on ONE trajectory: sim_ref.advance with float64 arrays.  Returns new (xu, lam, goal, traj_offset, done, tracking error
    or None); the inputs are not modified."""
    xu, lam, goal = (np.array(a, np.float64, copy=True).reshape(-1) for a in (xu, lam, goal))
    nm = n + m
    if done:
        return xu, lam, goal, traj_offset, done, None
    if not shift:
        xu[:n] = xs
        return xu, lam, goal, traj_offset, done, None
    plan, goals = np.asarray(xu_traj, np.float64).reshape(-1), np.asarray(ee_traj, np.float64).reshape(-1)
    err = tracking_error(ee, goal[:3])
    off = traj_offset + 1
    inside = off + N < traj_steps
    new_xu = xu.copy()
    new_xu[:len(xu) - nm] = xu[nm:]
    if inside:
        new_xu[len(xu) - nm:] = plan[nm * (off + lead) - m:nm * (off + lead) - m + nm]
    else:
        new_xu[len(xu) - nm:] = 0.0
        new_xu[len(xu) - n:len(xu) - n + n // 2] = plan[(traj_steps - 1) * nm:(traj_steps - 1) * nm + n // 2]
    new_goal = np.concatenate([goal[6:], goals[6 * ((off + N - 1) if inside else (traj_steps - 1)):][:6]])
    new_lam = np.concatenate([lam[n:], lam[-n:]])
    new_xu[:n] = xs
    return new_xu, new_lam, new_goal, off, (1 if off >= traj_steps else 0), err
