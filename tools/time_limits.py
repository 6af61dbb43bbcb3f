#!/usr/bin/env python3
"""Time the calls that honour a plant's soft limits (mpcg_plant_clone_limits) against the same calls with the plain plant, on one handle in ONE process, the two
alternated window by window: mpcg_generate_kkt_xuref in the default build and with "kkt_f32" = 1, mpcg_compute_merit_xuref at nine step sizes — the COST = 2
against the COST = 1 instantiations — and mpcg_simulate over one control period (ten substeps of 2e-4 s) with MPCG_LIMITS_SIM_SATURATE against without.
Shapes: 1024 trajectories x 128 knots and one trajectory x 32 knots.  The limits are the terciles of the call's own states and controls per kind, so that about
a third of the values lies below, inside and above; every weight is positive.  After 50 ms of back-to-back warm-up launches of both: device events around
`reps` back-to-back calls, medians of seven windows; the spread of the seven windows of the plain plant's call (min .. max) is printed next to the medians.
One JSON line per shape and call.  At one trajectory the back-to-back calls are bound by the host's launch rate.  The existing entries are compared with their
parent by tools/time_xuref.py --root DIR --plain-only, as before.  Needs an MI355X:
    python tools/time_limits.py [--root DIR] [reps]"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, min_max, select_build, windows_of

select_build()
import mpcgpu_amd  # noqa: E402
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402

STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]
MU = 10.0


def terciles(vals):
    lo, hi = np.quantile(vals, [1 / 3, 2 / 3], axis=0)
    return [float(np.float32(v)) for v in lo], [float(np.float32(v)) for v in hi]


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    plant = Plant()
    for N, B in ((128, 1024), (32, 1)):
        reps = reps_arg or (200 if B == 1 else 20)
        xu, ee, xs = (np.ascontiguousarray(a, np.float32) for a in iiwa.random_windows(N, B, seed=3))
        rng = np.random.default_rng(4)
        dz = (0.05 * rng.standard_normal(xu.shape)).astype(np.float32)
        knots = np.concatenate([xu, np.zeros((B, 7), np.float32)], axis=1).reshape(B * N, 21)
        limits = dict(q=terciles(knots[:, :7]), qd=terciles(knots[:, 7:14]), u=terciles(knots.reshape(B, N, 21)[:, :N - 1, 14:].reshape(-1, 7)), q_weight=3.0, qd_weight=0.25, u_weight=0.125)
        limited, saturating = plant.with_limits(**limits), plant.with_limits(**limits, sim_saturate=True)
        sol = PcgSolver(N, max_batch=B)
        r, qd = float(np.float32(iiwa.r_cost(N))), float(np.float32(iiwa.QD_COST))
        goal, s0, x, z = (torch.from_numpy(a).to(dev) for a in (ee.reshape(B, -1), xs, xu, dz))
        merit = torch.empty(B, len(STEPS9), device=dev)
        plan = torch.from_numpy((0.5 * rng.standard_normal((2 * N, 21))).astype(np.float32)).to(dev)
        offs = torch.from_numpy(rng.integers(-2, N + 2, B).astype(np.int32)).to(dev)
        ref = mpcgpu_amd.XuRef(plan, offs, 0, 0.75, 0.5, True, True)
        state = s0.clone()

        def sim(pl):
            state.copy_(s0)
            sol.simulate(pl, state, x, iiwa.TIMESTEP, 0.0, 2000.0, 2e-4)
            return state
        calls = {"generate_kkt_xuref": [lambda pl=pl: sol.generate_kkt_xuref(pl, goal, s0, x, iiwa.TIMESTEP, qd, r, ref) for pl in (plant, limited)],
                 "compute_merit_xuref": [lambda pl=pl: sol.compute_merit_xuref(pl, goal, s0, x, z, STEPS9, iiwa.TIMESTEP, MU, qd, r, ref, merit=merit) for pl in (plant, limited)],
                 "simulate": [lambda pl=pl: sim(pl) for pl in (plant, saturating)]}
        for name, key, f32 in (("generate_kkt_xuref", "generate_kkt_xuref", 0), ("generate_kkt_xuref kkt_f32=1", "generate_kkt_xuref", 1),
                               ("compute_merit_xuref", "compute_merit_xuref", 0), ("simulate", "simulate", 0)):
            sol.set_option("kkt_f32", f32)
            outs = [c() for c in calls[key]]
            torch.cuda.synchronize()
            finite = all(bool(torch.isfinite(t).all()) for o in outs for t in (o if isinstance(o, tuple) else (o,)))
            del outs
            med, rounds = alternate(calls[key], reps)
            lo, hi = min_max(rounds, 0)
            rec = {"call": name, "knots": N, "batch": B, "reps": reps, "plain_us": round(med[0], 2), "plain_min_max_us": [round(lo, 2), round(hi, 2)],
                   "limits_us": round(med[1], 2), "limits_over_plain": round(med[1] / med[0], 3), "finite": finite,
                   "windows": windows_of(rounds)}
            if key == "compute_merit_xuref":
                rec["num_steps"] = len(STEPS9)
            print(json.dumps(rec), flush=True)
        sol.set_option("kkt_f32", 0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
