#!/usr/bin/env python3
"""Time the _xuref entries (the generalised running cost over a joint-space plan) against the entries they generalise, on one handle in ONE process, the two
alternated window by window: mpcg_generate_kkt_xuref against mpcg_generate_kkt in the default build and with "kkt_f32" = 1, mpcg_compute_merit_xuref against
mpcg_compute_merit at nine step sizes.  Shapes: 1024 trajectories x 128 knots and one trajectory x 32 knots.  The new calls run with every weight positive, both
flags, a shared plan of 2 N rows and per-trajectory offsets (84 more bytes read per knot).  After 50 ms of back-to-back warm-up launches of both: device events
around `reps` back-to-back calls, medians of seven windows; the spread of the seven windows of the plain entry (min .. max) is printed next to the medians: it is
the margin a comparison between two builds of the library has.  One JSON line per shape and call.  At one trajectory the back-to-back calls are bound by the
host's launch rate, and the Python wrapper of the new calls builds one more struct per call.

--root DIR times the library of another checkout (DIR/mpcgpu_amd, built there).  A library without the _xuref entries (the parent commit) is timed on its plain
entries only, and --plain-only times this library the same way (no alternation: at one trajectory the launch-bound figures depend on what the windows alternate
with): that is how the existing entries are compared with their parent, in the same session on the same box.  Needs an MI355X:
    python tools/time_xuref.py [--root DIR] [--plain-only] [reps]"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, min_max, select_build, windows_of

select_build()
PLAIN_ONLY = "--plain-only" in sys.argv
if PLAIN_ONLY:
    sys.argv.remove("--plain-only")
import mpcgpu_amd  # noqa: E402
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402

STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]
MU = 10.0


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    plant = Plant()
    has_xuref = hasattr(mpcgpu_amd, "XuRef") and not PLAIN_ONLY
    for N, B in ((128, 1024), (32, 1)):
        reps = reps_arg or (200 if B == 1 else 20)
        xu, ee, xs = (np.ascontiguousarray(a, np.float32) for a in iiwa.random_windows(N, B, seed=3))
        rng = np.random.default_rng(4)
        dz = (0.05 * rng.standard_normal(xu.shape)).astype(np.float32)
        sol = PcgSolver(N, max_batch=B)
        r, qd = float(np.float32(iiwa.r_cost(N))), float(np.float32(iiwa.QD_COST))
        goal, s0, x, z = (torch.from_numpy(a).to(dev) for a in (ee.reshape(B, -1), xs, xu, dz))
        merit = torch.empty(B, len(STEPS9), device=dev)
        calls = {"generate_kkt": [lambda: sol.generate_kkt(plant, goal, s0, x, iiwa.TIMESTEP, qd, r)],
                 "compute_merit": [lambda: sol.compute_merit(plant, goal, s0, x, z, STEPS9, iiwa.TIMESTEP, MU, qd, r, merit=merit)]}
        if has_xuref:
            plan = torch.from_numpy((0.5 * rng.standard_normal((2 * N, 21))).astype(np.float32)).to(dev)
            offs = torch.from_numpy(rng.integers(-2, N + 2, B).astype(np.int32)).to(dev)
            ref = mpcgpu_amd.XuRef(plan, offs, 0, 0.75, 0.5, True, True)
            calls["generate_kkt"].append(lambda: sol.generate_kkt_xuref(plant, goal, s0, x, iiwa.TIMESTEP, qd, r, ref))
            calls["compute_merit"].append(lambda: sol.compute_merit_xuref(plant, goal, s0, x, z, STEPS9, iiwa.TIMESTEP, MU, qd, r, ref, merit=merit))
        for name, key, f32 in (("generate_kkt", "generate_kkt", 0), ("generate_kkt kkt_f32=1", "generate_kkt", 1), ("compute_merit", "compute_merit", 0)):
            sol.set_option("kkt_f32", f32)
            outs = [c() for c in calls[key]]
            torch.cuda.synchronize()
            finite = all(bool(torch.isfinite(t).all()) for o in outs for t in (o if isinstance(o, tuple) else (o,)))
            del outs
            med, rounds = alternate(calls[key], reps)
            lo, hi = min_max(rounds, 0)
            rec = {"call": name, "knots": N, "batch": B, "reps": reps, "plain_us": round(med[0], 2), "plain_min_max_us": [round(lo, 2), round(hi, 2)],
                   "finite": finite, "windows": windows_of(rounds)}
            if has_xuref:
                rec.update(xuref_us=round(med[1], 2), xuref_over_plain=round(med[1] / med[0], 3))
            else:
                rec["library"] = "plain entries only" if PLAIN_ONLY else "without the _xuref entries"
            if key == "compute_merit":
                rec["num_steps"] = len(STEPS9)
            print(json.dumps(rec), flush=True)
        sol.set_option("kkt_f32", 0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
