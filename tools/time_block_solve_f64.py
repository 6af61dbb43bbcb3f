#!/usr/bin/env python3
"""Time the block-tridiagonal direct solve in its three precisions on one handle in ONE process, alternated window by window:
    float     mpcg_block_solve, "block_solve_f64" = 0 — the baseline (the float kernels, untouched by the double paths)
    option    mpcg_block_solve, "block_solve_f64" = 1 — float S / gamma widened on load, the sweep in double, lambda rounded on store
    f64       mpcg_block_solve_f64 — linsys_t = double
Shapes: 1024 trajectories x 128 knots (the throughput call), one trajectory x 128 and one x 32 knots (the MPC loop's own call), state size 14.
After 50 ms of back-to-back warm-up launches of all three: device events around `reps` back-to-back calls, medians of seven windows.
Before the timing the three results are compared against the float64 result (relative to max |lambda|).  One JSON line per shape.
No ratio is promised: a knot's elimination is a dependent chain of fp64 operations at half the fp32 issue rate, with twice the scratch
traffic.  Needs an MI355X:
    [AB_LIB=<another build's libmpcg_hip.so>] python tools/time_block_solve_f64.py [reps]
(tools/time_block_solve.py is the older comparison of the float solve against PCG.)"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, select_build, windows_of

select_build()
import bench  # noqa: E402
from mpcgpu_amd import PcgSolver  # noqa: E402


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    for N, B in ((128, 1024), (128, 1), (32, 1)):
        reps = reps_arg or (200 if B == 1 else 20)
        sol = PcgSolver(N, max_batch=B)
        dS, _, dg = bench.build_inputs(sol, N, B, 0, "ss", dev)
        dS64, dg64 = dS.double(), dg.double()
        lam = torch.empty(B, 14 * N, device=dev)
        lam64 = torch.empty(B, 14 * N, device=dev, dtype=torch.float64)

        def call(which):
            if which == "f64":
                sol.block_solve(dS64, dg64, lam64)
            else:
                sol.set_option("block_solve_f64", 1 if which == "option" else 0)      # (read when the call is made)
                sol.block_solve(dS, dg, lam)

        names = ("float", "option", "f64")
        out = {}
        for w in names:
            call(w)
            torch.cuda.synchronize()
            out[w] = (lam64 if w == "f64" else lam).cpu().numpy().astype(np.float64)
        scale = np.abs(out["f64"]).max()
        diff = {w: float(f"{np.abs(out[w] - out['f64']).max() / scale:.3g}") for w in ("float", "option")}
        med, rounds = alternate([lambda w=w: call(w) for w in names], reps)
        print(json.dumps({"knots": N, "batch": B, "reps": reps, "float_us": round(med[0], 2), "option_us": round(med[1], 2), "f64_us": round(med[2], 2),
                          "option_over_float": round(med[1] / med[0], 3), "f64_over_float": round(med[2] / med[0], 3),
                          "finite": bool(all(np.isfinite(v).all() for v in out.values())), "float_vs_f64": diff["float"], "option_vs_f64": diff["option"],
                          "windows": windows_of(rounds)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
