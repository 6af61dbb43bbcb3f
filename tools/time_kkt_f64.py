#!/usr/bin/env python3
"""Time the double producer and consumer against their float twins: mpcg_generate_kkt (default: float64 inside, float arrays) against
mpcg_generate_kkt_f64 (double arrays), and mpcg_compute_merit against mpcg_compute_merit_f64 at nine step sizes — on one handle in ONE process, the two
alternated window by window.  Shapes: 1024 trajectories x 128 knots and one trajectory x 32 knots.  After 50 ms of back-to-back warm-up launches of
both: device events around `reps` back-to-back calls, medians of seven windows.  The double KKT entry writes twice the bytes (599 MB per
1024 x 128 knots) behind the same arithmetic: the figure to compare it with is the float entry timed in the same run.  Before the timing the double
outputs rounded to float are compared with the float entry's (the inputs are floats widened: KKT bitwise; the merits to float rounding, since the float
entry forms its trial iterate in float).  One JSON line per shape and call.  Needs an MI355X:
    python tools/time_kkt_f64.py [reps]"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, select_build, windows_of

select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402

STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]
MU = 10.0
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    plant = Plant()
    for N, B in ((128, 1024), (32, 1)):
        reps = reps_arg or (200 if B == 1 else 20)
        xu, ee, xs = (np.ascontiguousarray(a, np.float32) for a in iiwa.random_windows(N, B, seed=3))
        dz = (0.05 * np.random.default_rng(4).standard_normal(xu.shape)).astype(np.float32)
        sol = PcgSolver(N, max_batch=B)
        r, qd = float(np.float32(iiwa.r_cost(N))), float(np.float32(iiwa.QD_COST))
        d = {dt: tuple(torch.from_numpy(a.astype(dt)).to(dev) for a in (ee.reshape(B, -1), xs, xu, dz)) for dt in (np.float32, np.float64)}
        merit = {dt: torch.empty(B, len(STEPS9), device=dev, dtype=TORCH[dt]) for dt in d}

        def kkt(dt):
            goal, s, x, _ = d[dt]
            return sol.generate_kkt(plant, goal, s, x, iiwa.TIMESTEP, qd, r)

        def mer(dt):
            goal, s, x, z = d[dt]
            return sol.compute_merit(plant, goal, s, x, z, STEPS9, iiwa.TIMESTEP, MU, qd, r, merit=merit[dt])

        o32, o64 = kkt(np.float32), kkt(np.float64)
        m32, m64 = mer(np.float32).clone(), mer(np.float64).clone()
        torch.cuda.synchronize()
        same = all(torch.equal(a.to(torch.float32).view(torch.int32), b.view(torch.int32)) for a, b in zip(o64, o32))
        mdiff = float(((m64 - m32.double()).abs() / m64.abs().clamp(min=1.0)).max())
        out_bytes = sum(t.numel() * t.element_size() for t in o64)
        del o32, o64
        for name, fn in (("generate_kkt", kkt), ("compute_merit", mer)):
            med, rounds = alternate((lambda: fn(np.float32), lambda: fn(np.float64)), reps)
            rec = {"call": name, "knots": N, "batch": B, "reps": reps, "float_us": round(med[0], 2), "f64_us": round(med[1], 2),
                   "f64_over_float": round(med[1] / med[0], 3), "windows": windows_of(rounds)}
            if name == "generate_kkt":
                rec.update(f64_rounded_is_float_bitwise=bool(same), f64_output_bytes=out_bytes)
            else:
                rec.update(num_steps=len(STEPS9), worst_f64_vs_float=float(f"{mdiff:.3g}"))
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
