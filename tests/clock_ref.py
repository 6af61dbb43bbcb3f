"""Restatement of the per-trajectory clocks of mpcg_simulate_clk and mpcg_advance_horizon_clk (mpcgpu_amd/csrc/sim_plant.hip.h) — TEST
INFRASTRUCTURE.  Python floats are IEEE doubles with one rounding per operation and math.fmod is exact, which is what the kernels are held to.

    threshold       the reference's SHIFT_THRESHOLD, (double)(T)(1 * timestep), T the arrays' type
    schedule        what the simulate kernel derives from one trajectory's (time offset, simulated time): valid?, toff [s], S, remainder
    update          the clock bookkeeping of include/mpcsim.cuh:294-352 for ONE trajectory and ONE control update
    Clock           that state carried over updates, counting shifts
    control_update  one control update of one trajectory composed from the restatements: simulate under the previous plan from the clock's
                    prev_sim_us, then advance with the clock's decision (tests/plant_ref.py in the arrays' precision)"""
import math

import numpy as np

import plant_ref

MAX_SUBSTEPS = 65536                     # MPCG_SIM_MAX_SUBSTEPS
DONE_BAD_CLOCK = 2                       # MPCG_DONE_BAD_CLOCK


def threshold(timestep, dtype=np.float32):
    return float(np.dtype(dtype).type(1 * timestep))


def bad_time(t_us):
    return not (math.isfinite(t_us) and t_us >= 0.0)


def schedule(toff_us, sim_us, sim_step, dtype=np.float32):
    """(valid, toff, S, rem): sim_step as the entry receives it (a float for float32 arrays, a double for float64); the remainder rounded to
    float32 for float32 arrays and fmod's value for float64.  Invalid: (False, None, 0, 0.0)."""
    ss = float(np.dtype(dtype).type(sim_step))
    if bad_time(toff_us) or bad_time(sim_us):
        return False, None, 0, 0.0
    toff, sim = toff_us * 1e-6, sim_us * 1e-6
    full = sim / ss
    if not full < MAX_SUBSTEPS + 1.0:
        return False, None, 0, 0.0
    return True, toff, int(full), float(np.dtype(dtype).type(math.fmod(sim, ss)))


def update(since_s, shifted, sim_us, timestep, shift_threshold_s):
    """-> (since_s, shifted, prev_sim_us, shift) after one control update of sim_us microseconds."""
    since = since_s + sim_us * 1e-6
    shift = (not shifted) and since > shift_threshold_s
    if shift:
        shifted = 1
    if since > timestep:
        shifted, since = 0, math.fmod(since, timestep)
    return since, int(shifted), float(sim_us), bool(shift)


class Clock:
    def __init__(self, timestep, dtype=np.float32, since_s=0.0, shifted=0, prev_sim_us=0.0):
        self.timestep, self.threshold = float(timestep), threshold(timestep, dtype)
        self.since_s, self.shifted, self.prev_sim_us, self.shifts = float(since_s), int(shifted), float(prev_sim_us), 0

    def update(self, sim_us):
        self.since_s, self.shifted, self.prev_sim_us, shift = update(self.since_s, self.shifted, sim_us, self.timestep, self.threshold)
        self.shifts += shift
        return shift

    def state(self):
        return self.since_s, self.shifted, self.prev_sim_us


def shifts_of(period_us, updates, timestep, dtype=np.float32):
    """[does update u shift] for a loop of constant period started from a zero clock"""
    c = Clock(timestep, dtype)
    return [c.update(period_us) for _ in range(updates)]


def control_update(model, N, timestep, clock, sim_us, sim_step, xs, xu_old, xu, lam, goal, xu_traj, ee_traj, traj_steps, traj_offset, done, lead=0,
                   dtype=np.float32):
    """One control update of ONE live trajectory.  -> (new xs (float64 values, as the restatement carries them), new (xu, lam, goal, traj_offset,
    done, tracking error or None), shift).  xs_new is rounded to `dtype` before it is handed to advance, as the entry stores it."""
    x = plant_ref.simulate(model, xs, xu_old, N, timestep, clock.prev_sim_us, sim_us, sim_step, double=np.dtype(dtype) == np.float64)
    ee = model.ee_pos(x[:7])
    shift = clock.update(sim_us)
    out = plant_ref.advance(shift, N, xu, lam, goal, np.asarray(x, dtype), np.asarray(ee, dtype), xu_traj, ee_traj, traj_steps, traj_offset, done, lead, dtype)
    return x, out, shift
