#!/usr/bin/env python3
"""Time the step between two SQP solves: (a) ONE mpcg_simulate call of the reference's schedule — 2,000 us at 0.2 ms: 10 substeps and the remainder —,
(b) the same number of dynamics rounds as 11 calls of one substep each (sim_time 100 us: no full substep, one remainder substep), which is the
reference's launch structure (simple_simulate launches a kernel per substep), and (c) one mpcg_advance_horizon(shift = 1).  At 1 x N=32 and
1024 x N=128; the three are alternated in one process after 50 ms of warm-up, device events around `reps` back-to-back calls, medians of seven
windows.  Needs an MI355X:  python tools/time_simulate.py [reps]"""
import ctypes as C
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, select_build, windows_of

select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    plant = Plant()
    for N, B in ((32, 1), (128, 1024)):
        reps = reps_arg or (100 if B == 1 else 20)
        xu, ee, xs = iiwa.random_windows(N, B, seed=3)
        T = N + 8
        sol = PcgSolver(N, max_batch=B)
        d_xu, d_goal, d_xs0 = t(xu), t(ee).reshape(B, -1), t(xs)
        d_xs, d_lam, d_ee = d_xs0.clone(), torch.zeros(B, 14 * N, device=dev), torch.zeros(B, 3, device=dev)
        plan, plan_goals = torch.zeros(T, 21, device=dev), torch.zeros(T, 6, device=dev)
        off, done, err = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, device=dev)
        lib, h, pl = sol.lib, sol._h, plant._p
        p = lambda x: C.c_void_p(x.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def one_call():
            assert lib.mpcg_simulate(h, pl, 7, p(d_xs), p(d_xu), iiwa.TIMESTEP, 2000.0, 2000.0, 2e-4, p(d_ee), B, stream) == 0

        def eleven_calls():
            for s in range(11):
                assert lib.mpcg_simulate(h, pl, 7, p(d_xs), p(d_xu), iiwa.TIMESTEP, 2000.0 + 200.0 * s, 100.0, 2e-4, p(d_ee) if s == 10 else None, B, stream) == 0

        def advance():
            off.zero_()                                  # (stay inside the plan; a 4-byte fill in front of every call)
            assert lib.mpcg_advance_horizon(h, 7, 1, p(d_xu), p(d_lam), p(d_goal), p(d_xs), p(d_ee), p(plan), p(plan_goals), T, 0, 0, p(off), p(done), p(err),
                                            B, stream) == 0

        def reset():
            d_xs.copy_(d_xs0)                            # (the plant must not drift away over thousands of timed steps)

        med, rounds = alternate((one_call, eleven_calls, advance), reps, reset=reset)
        print(json.dumps({"knots": N, "batch": B, "reps": reps, "simulate_one_call_us": round(med[0], 2), "simulate_eleven_calls_us": round(med[1], 2),
                          "advance_horizon_shift_us": round(med[2], 2), "eleven_over_one": round(med[1] / med[0], 2),
                          "windows": windows_of(rounds)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
