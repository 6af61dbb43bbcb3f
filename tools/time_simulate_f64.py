#!/usr/bin/env python3
"""Time the double step between two SQP solves against its float twin: mpcg_simulate against mpcg_simulate_f64 for one control update of 2,000 us, and
mpcg_advance_horizon against mpcg_advance_horizon_f64 (shift = 1) — on one handle in ONE process, the two alternated window by window.  Shapes: 1024
trajectories x 128 knots and one trajectory x 32 knots.  After a warm-up of back-to-back launches of both: device events around `reps` back-to-back
calls, medians of seven windows.  Both simulate entries run eleven substeps and the pose round per call: the float entry at 2e-4f ten and its remainder of
5e-11 s, the double entry at the reference's double 2e-4 ten and the remainder of almost a whole substep (include/mpcg.h).  The plant state is put back
before every window (a call integrates it in place), and so is the plan offset of the horizon shift, whose plan is long enough for a window.  Before the
timing the double simulate at the substep (double)2e-4f is compared with the float entry on the same float inputs (their remainders differ in the
rounding to float only: not bitwise).  One JSON line per shape and call.  Not a gate.  Needs an MI355X:
    python tools/time_simulate_f64.py [reps]"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, select_build, windows_of

select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402

WARMUP = 50
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
SIM_US = 2000.0
SS = {np.float32: float(np.float32(2e-4)), np.float64: 2e-4}
n, m = 14, 7


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    plant = Plant()
    for N, B in ((128, 1024), (32, 1)):
        reps = reps_arg or (200 if B == 1 else 20)
        T = N + max(reps, WARMUP) + 16
        xu, ee, xs = (np.ascontiguousarray(a, np.float32) for a in iiwa.random_windows(N, B, seed=3))
        rng = np.random.default_rng(4)
        plan, plan_goals = (0.3 * rng.standard_normal((T, n + m))).astype(np.float32), (0.3 * rng.standard_normal((T, 6))).astype(np.float32)
        lam = rng.standard_normal((B, n * N)).astype(np.float32)
        sol = PcgSolver(N, max_batch=B)
        d = {dt: {k: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
                  for k, a in (("xs", xs), ("xu", xu), ("goal", ee.reshape(B, -1)), ("lam", lam), ("plan", plan), ("plan_goals", plan_goals))} for dt in SS}
        for dt in d:
            d[dt].update(xs0=d[dt]["xs"].clone(), ee=torch.zeros(B, 3, device=dev, dtype=TORCH[dt]), err=torch.zeros(B, device=dev, dtype=TORCH[dt]))
        offset, done = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)

        def reset():
            for dt in d:
                d[dt]["xs"].copy_(d[dt]["xs0"])
            offset.zero_()
            done.zero_()

        def sim(dt, ss=None):
            t = d[dt]
            return sol.simulate(plant, t["xs"], t["xu"], iiwa.TIMESTEP, 0.0, SIM_US, SS[dt] if ss is None else ss, eePos=t["ee"])

        def adv(dt):
            t = d[dt]
            return sol.advance_horizon(True, t["xu"], t["xs"], t["lam"], t["goal"], t["ee"], t["plan"], t["plan_goals"], offset, done, t["err"])

        reset()
        x32 = sim(np.float32).clone()
        x64 = sim(np.float64, SS[np.float32]).clone()
        torch.cuda.synchronize()
        diff = float(((x64 - x32.double()).abs() / x64.abs().clamp(min=1.0)).max())
        for name, fn in (("simulate", sim), ("advance_horizon", adv)):
            med, rounds = alternate((lambda: fn(np.float32), lambda: fn(np.float64)), reps, reset=reset, warmup_rounds=WARMUP)
            assert int(done.max()) == 0                  # no trajectory used its plan up: every timed shift did the whole work
            rec = {"call": name, "knots": N, "batch": B, "reps": reps, "float_us": round(med[0], 2), "f64_us": round(med[1], 2),
                   "f64_over_float": round(med[1] / med[0], 3), "windows": windows_of(rounds)}
            if name == "simulate":
                rec.update(sim_time_us=SIM_US, substeps_per_call=11, worst_f64_vs_float=float(f"{diff:.3g}"))
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
