#!/usr/bin/env python3
"""Time mpcg_compute_merit in its two builds: the default (float64 inside — the baseline) and option "merit_f32" = 1 (packed float, two work items per
16-lane group: csrc/merit_plant_f32.hip.h), on one handle in ONE process, the two alternated window by window.  Shapes: 1024 trajectories x 128 knots
at nine and at eight step sizes (the line search of an SQP iteration with and without step size 0), and one trajectory x 32 knots x nine.  After 50 ms
of back-to-back warm-up launches of both builds: device events around `reps` back-to-back calls, medians of seven windows.  Before the timing the two
builds' merits of the timed inputs are compared (relative to max(1, |merit|)).  One JSON line per shape.  Needs an MI355X:
    python tools/time_merit_f32.py [reps]
(tools/time_merit.py is the older comparison of the merit call against nine KKT calls.)"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, select_build, windows_of

select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402

STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]
MU = 10.0


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    plant = Plant()
    for N, B, steps in ((128, 1024, STEPS9), (128, 1024, STEPS9[1:]), (32, 1, STEPS9)):
        reps = reps_arg or (200 if B == 1 else 20)
        xu, ee, xs = iiwa.random_windows(N, B, seed=3)
        dz = 0.05 * np.random.default_rng(4).standard_normal(xu.shape)
        sol = PcgSolver(N, max_batch=B)
        d_xu, d_dz, d_goal, d_xs = t(xu), t(dz), t(ee).reshape(B, -1), t(xs)
        merit = torch.empty(B, len(steps), device=dev)
        r = iiwa.r_cost(N)

        def call(f32):
            sol.set_option("merit_f32", f32)             # (read when the call is made)
            sol.compute_merit(plant, d_goal, d_xs, d_xu, d_dz, steps, iiwa.TIMESTEP, MU, iiwa.QD_COST, r, merit=merit)

        out = []
        for f32 in (0, 1):
            call(f32)
            torch.cuda.synchronize()
            out.append(merit.cpu().numpy().astype(np.float64))
        diff = float((np.abs(out[1] - out[0]) / np.maximum(1.0, np.abs(out[0]))).max())
        med, rounds = alternate([lambda f32=f32: call(f32) for f32 in (0, 1)], reps)
        print(json.dumps({"knots": N, "batch": B, "num_steps": len(steps), "reps": reps, "merit_default_us": round(med[0], 2),
                          "merit_f32_us": round(med[1], 2), "default_over_f32": round(med[0] / med[1], 3), "finite": bool(np.isfinite(out[1]).all()),
                          "worst_f32_vs_default": float(f"{diff:.3g}"), "windows": windows_of(rounds)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
