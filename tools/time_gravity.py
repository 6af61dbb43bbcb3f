#!/usr/bin/env python3
"""Time a gravity clone against the plain plant (mpcg_plant_clone_gravity, include/mpcg.h GRAVITY): mpcg_generate_kkt in the default build and with
"kkt_f32" = 1, mpcg_compute_merit at nine step sizes and mpcg_simulate over 2,000 us at the reference's substep — on one handle in ONE process, the two
plants alternated window by window.  Shapes: 1024 trajectories x 128 knots and one trajectory x 32 knots.  After 50 ms of back-to-back warm-up launches of
both: device events around `reps` back-to-back calls, medians of seven windows; the spread of the seven windows of the plain plant (min .. max) is printed
next to the medians: it is the margin a comparison between two builds of the library has.  Then mpcg_inverse_dynamics for batch x knots states (131,072 at
the large shape), gravity torques only.  One JSON line per shape and call.

--root DIR times the library of another checkout (DIR/mpcgpu_amd, built there).  A library without the clone (a commit before it) is timed with its plain
plant alone: that is how the default is compared with its parent, in the same session on the same box.  Needs an MI355X:
    python tools/time_gravity.py [--root DIR] [reps]"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, min_max, select_build, windows_of

select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402

STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]
MU = 10.0
GRAVITY = (0.0, 0.0, 9.81)


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    plain = Plant()
    plants = [plain] + ([plain.with_gravity(GRAVITY)] if hasattr(plain, "with_gravity") else [])      # a library from before the clone: its plain plant alone
    for N, B in ((128, 1024), (32, 1)):
        reps = reps_arg or (200 if B == 1 else 20)
        xu, ee, xs = (np.ascontiguousarray(a, np.float32) for a in iiwa.random_windows(N, B, seed=3))
        dz = (0.05 * np.random.default_rng(4).standard_normal(xu.shape)).astype(np.float32)
        sol = PcgSolver(N, max_batch=B)
        r, qd = float(np.float32(iiwa.r_cost(N))), float(np.float32(iiwa.QD_COST))
        goal, s0, x, z = (torch.from_numpy(a).to(dev) for a in (ee.reshape(B, -1), xs, xu, dz))
        merit, s, pos = torch.empty(B, len(STEPS9), device=dev), s0.clone(), torch.zeros(B, 3, device=dev)

        def kkt(p):
            return sol.generate_kkt(p, goal, s0, x, iiwa.TIMESTEP, qd, r)

        def mer(p):
            return sol.compute_merit(p, goal, s0, x, z, STEPS9, iiwa.TIMESTEP, MU, qd, r, merit=merit)

        def sim(p):
            s.copy_(s0)                                  # (the plant must not drift away over thousands of timed steps; a 56 B x batch copy in front of every call)
            return sol.simulate(p, s, x, iiwa.TIMESTEP, 2000.0, 2000.0, 2e-4, eePos=pos)

        for name, f32, fn in (("generate_kkt", 0, kkt), ("generate_kkt kkt_f32=1", 1, kkt), ("compute_merit", 0, mer), ("simulate", 0, sim)):
            sol.set_option("kkt_f32", f32)
            outs = [fn(p) for p in plants]
            torch.cuda.synchronize()
            finite = all(bool(torch.isfinite(t).all()) for o in outs for t in (o if isinstance(o, tuple) else (o,)) if t is not None)
            del outs
            med, rounds = alternate([(lambda p=p: fn(p)) for p in plants], reps)
            lo, hi = min_max(rounds, 0)
            rec = {"call": name, "knots": N, "batch": B, "reps": reps, "plain_us": round(med[0], 2), "plain_min_max_us": [round(lo, 2), round(hi, 2)],
                   "finite": finite, "windows": windows_of(rounds)}
            if len(plants) > 1:
                rec.update(gravity_us=round(med[1], 2), gravity_over_plain=round(med[1] / med[0], 3))
            else:
                rec["library"] = "without mpcg_plant_clone_gravity"
            if name == "compute_merit":
                rec["num_steps"] = len(STEPS9)
            print(json.dumps(rec), flush=True)
        sol.set_option("kkt_f32", 0)
        if len(plants) > 1:
            count = B * N
            q = torch.from_numpy(np.ascontiguousarray(xu.reshape(-1)[:count * 7].reshape(count, 7))).to(dev)      # (any finite angles)
            tau = torch.empty(count, 7, device=dev)
            med, rounds = alternate([lambda: sol.inverse_dynamics(plants[1], q, tau=tau)], reps)
            lo, hi = min_max(rounds, 0)
            print(json.dumps({"call": "inverse_dynamics", "states": count, "reps": reps, "gravity_us": round(med[0], 2),
                              "min_max_us": [round(lo, 2), round(hi, 2)], "finite": bool(torch.isfinite(tau).all())}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
