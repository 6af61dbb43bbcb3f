#!/usr/bin/env python3
"""Time the two integrators against each other: options "integrator" (mpcg_generate_kkt in the default build and with "kkt_f32" = 1, mpcg_compute_merit at
nine step sizes) and "sim_integrator" (mpcg_simulate over 2,000 us at the reference's substep) at 0 (explicit Euler) and 1 (semi-implicit Euler) — on one
handle in ONE process, the two settings alternated window by window (the options are read when a call is made).  Shapes: 1024 trajectories x 128 knots and one
trajectory x 32 knots.  After 50 ms of back-to-back warm-up launches of both: device events around `reps` back-to-back calls, medians of seven windows; the
spread of the seven windows of setting 0 (min .. max) is printed next to the medians: it is the margin a comparison between two builds of the library has.
One JSON line per shape and call.

--root DIR times the library of another checkout (DIR/mpcgpu_amd, built there).  A library without the options (a commit before them) is timed at its only
setting: that is how the default is compared with its parent, in the same session on the same box.  Needs an MI355X:
    python tools/time_integrator.py [--root DIR] [reps]"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, min_max, select_build, windows_of

select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402

STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]
MU = 10.0


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    plant = Plant()
    for N, B in ((128, 1024), (32, 1)):
        reps = reps_arg or (200 if B == 1 else 20)
        xu, ee, xs = (np.ascontiguousarray(a, np.float32) for a in iiwa.random_windows(N, B, seed=3))
        dz = (0.05 * np.random.default_rng(4).standard_normal(xu.shape)).astype(np.float32)
        sol = PcgSolver(N, max_batch=B)
        try:
            sol.set_option("integrator", 0)
            sol.set_option("sim_integrator", 0)
            settings = (0, 1)
        except RuntimeError:
            settings = (0,)                              # a library from before the options: its only setting
        r, qd = float(np.float32(iiwa.r_cost(N))), float(np.float32(iiwa.QD_COST))
        goal, s0, x, z = (torch.from_numpy(a).to(dev) for a in (ee.reshape(B, -1), xs, xu, dz))
        merit, s, pos = torch.empty(B, len(STEPS9), device=dev), s0.clone(), torch.zeros(B, 3, device=dev)

        def option(key, v):
            if len(settings) > 1:
                sol.set_option(key, v)

        def kkt():
            return sol.generate_kkt(plant, goal, s0, x, iiwa.TIMESTEP, qd, r)

        def mer():
            return sol.compute_merit(plant, goal, s0, x, z, STEPS9, iiwa.TIMESTEP, MU, qd, r, merit=merit)

        def sim():
            s.copy_(s0)                                  # (the plant must not drift away over thousands of timed steps; a 56 B x batch copy in front of every call)
            return sol.simulate(plant, s, x, iiwa.TIMESTEP, 2000.0, 2000.0, 2e-4, eePos=pos)

        for name, key, f32, fn in (("generate_kkt", "integrator", 0, kkt), ("generate_kkt kkt_f32=1", "integrator", 1, kkt), ("compute_merit", "integrator", 0, mer),
                                   ("simulate", "sim_integrator", 0, sim)):
            sol.set_option("kkt_f32", f32)
            outs = []
            for v in settings:
                option(key, v)
                outs.append(fn())
            torch.cuda.synchronize()
            finite = all(bool(torch.isfinite(t).all()) for o in outs for t in (o if isinstance(o, tuple) else (o,)) if t is not None)
            del outs
            # (a window's option is set in front of it, outside the timed region: at one trajectory the back-to-back calls are bound by the host's launch rate,
            # where a mpcg_set_option per call would cost the library that has the option 0.7 us a call)
            med, rounds = alternate([fn] * len(settings), reps, reset=[lambda v=v: option(key, v) for v in settings])
            option(key, 0)
            lo, hi = min_max(rounds, 0)
            rec = {"call": name, "knots": N, "batch": B, "reps": reps, "explicit_us": round(med[0], 2), "explicit_min_max_us": [round(lo, 2), round(hi, 2)],
                   "finite": finite, "windows": windows_of(rounds)}
            if len(settings) > 1:
                rec.update(semi_implicit_us=round(med[1], 2), semi_over_explicit=round(med[1] / med[0], 3))
            else:
                rec["library"] = "without the integrator options"
            if name == "compute_merit":
                rec["num_steps"] = len(STEPS9)
            print(json.dumps(rec), flush=True)
        sol.set_option("kkt_f32", 0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
