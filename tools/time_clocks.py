#!/usr/bin/env python3
"""Time the per-trajectory-clock entries against the scalar ones: (a) mpcg_simulate of the reference's schedule — 2,000 us at 0.2 ms — against
(b) mpcg_simulate_clk with uniform arrays (the same rounds, the schedule formed on the device), (c) mpcg_simulate_clk on a MIXED batch whose
trajectories run 1,000, 2,000, 3,000 and 4,000 us in turn (a wavefront takes as long as its longest trajectory: 20 substeps), and (d)
mpcg_advance_horizon(shift = 1) against (e) mpcg_advance_horizon_clk with every trajectory shifting.  At 1 x N=32 and 1024 x N=128; the five are
alternated in one process after 50 ms of warm-up, device events around `reps` back-to-back calls, medians of seven windows, and each entry's own
window spread (max / min).  Needs an MI355X:  python tools/time_clocks.py [reps]"""
import ctypes as C
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, min_max, select_build, windows_of

select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    plant = Plant()
    for N, B in ((32, 1), (128, 1024)):
        reps = reps_arg or (100 if B == 1 else 20)
        xu, ee, xs = iiwa.random_windows(N, B, seed=3)
        T = N + 8
        sol = PcgSolver(N, max_batch=B)
        d_xu, d_goal, d_xs0 = t(xu), t(ee).reshape(B, -1), t(xs)
        d_xs, d_lam, d_ee = d_xs0.clone(), torch.zeros(B, 14 * N, device=dev), torch.zeros(B, 3, device=dev)
        plan, plan_goals = torch.zeros(T, 21, device=dev), torch.zeros(T, 6, device=dev)
        i32 = lambda: torch.zeros(B, dtype=torch.int32, device=dev)
        off, done, shifted, did, err = i32(), i32(), i32(), i32(), torch.zeros(B, device=dev)
        toff, uniform = f64([2000.0] * B), f64([2000.0] * B)
        mixed = f64([1000.0 * (1 + b % 4) for b in range(B)])
        sim_adv, prev, since = f64([2000.0] * B), f64([0.0] * B), f64([0.0] * B)
        since0 = f64([0.015] * B)                        # 0.015 + 0.002 > 1/64: every trajectory shifts, and wraps
        lib, h, pl = sol.lib, sol._h, plant._p
        p = lambda x: C.c_void_p(x.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def scalar():
            assert lib.mpcg_simulate(h, pl, 7, p(d_xs), p(d_xu), iiwa.TIMESTEP, 2000.0, 2000.0, 2e-4, p(d_ee), B, stream) == 0

        def clk_uniform():
            assert lib.mpcg_simulate_clk(h, pl, 7, p(d_xs), p(d_xu), iiwa.TIMESTEP, p(toff), p(uniform), 2e-4, p(d_ee), p(done), B, stream) == 0

        def clk_mixed():
            assert lib.mpcg_simulate_clk(h, pl, 7, p(d_xs), p(d_xu), iiwa.TIMESTEP, p(toff), p(mixed), 2e-4, p(d_ee), p(done), B, stream) == 0

        def advance():
            off.zero_()                                  # (stay inside the plan; a 4-byte fill in front of every call)
            assert lib.mpcg_advance_horizon(h, 7, 1, p(d_xu), p(d_lam), p(d_goal), p(d_xs), p(d_ee), p(plan), p(plan_goals), T, 0, 0, p(off), p(done), p(err),
                                            B, stream) == 0

        def advance_clk():
            off.zero_()
            since.copy_(since0)                          # (every call shifts: the clock back in front of the threshold; 8 B per trajectory)
            assert lib.mpcg_advance_horizon_clk(h, 7, p(d_xu), p(d_lam), p(d_goal), p(d_xs), p(d_ee), p(plan), p(plan_goals), T, 0, 0, p(off), p(done), p(err),
                                                iiwa.TIMESTEP, iiwa.TIMESTEP, p(sim_adv), p(prev), p(since), p(shifted), p(did), B, stream) == 0

        def reset():
            d_xs.copy_(d_xs0)                            # (the plant must not drift away over thousands of timed steps)

        fns = (scalar, clk_uniform, clk_mixed, advance, advance_clk)
        med, rounds = alternate(fns, reps, reset=reset)
        assert int(did.sum()) == B and int(done.sum()) == 0
        spread = [hi / lo for lo, hi in (min_max(rounds, i) for i in range(len(fns)))]
        print(json.dumps({"knots": N, "batch": B, "reps": reps, "simulate_us": round(med[0], 2), "simulate_clk_uniform_us": round(med[1], 2),
                          "simulate_clk_mixed_1000_4000_us": round(med[2], 2), "advance_horizon_shift_us": round(med[3], 2),
                          "advance_horizon_clk_shift_us": round(med[4], 2), "clk_uniform_over_scalar": round(med[1] / med[0], 3),
                          "clk_mixed_over_scalar": round(med[2] / med[0], 3), "advance_clk_over_scalar": round(med[4] / med[3], 3),
                          "window_spread_max_over_min": [round(v, 3) for v in spread],
                          "windows": windows_of(rounds)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
