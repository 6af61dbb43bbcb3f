#!/usr/bin/env python3
"""Time mpcg_compute_merit with nine step sizes (0 and -1 / 2^p: merit_ref and the eight trials of the reference's line search) against the only
route to the same decision without it: nine mpcg_generate_kkt calls on the same nine iterates (what examples/mpcsim_iiwa_demo.cpp does per SQP
iteration, less its nine device-to-host copies).  1024 x 128 knots and 1 x 32; the two are alternated in one process, five rounds after warm-up,
device events around `reps` back-to-back calls.  Needs an MI355X:  python tools/time_merit.py [reps]"""
import ctypes as C
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, select_build

select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa  # noqa: E402

STEPS = [0.0] + [-1.0 / (1 << p) for p in range(8)]
ROUNDS = 5


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    plant = Plant()
    out = []
    for N, B in ((128, 1024), (32, 1)):
        reps = reps_arg or (20 if B > 1 else 200)
        xu, ee, xs = iiwa.random_windows(N, B, seed=3)
        dz = 0.05 * np.random.default_rng(4).standard_normal(xu.shape)
        sol = PcgSolver(N, max_batch=B)
        dxu, dee, dxs, ddz = t(xu), t(ee).reshape(B, -1), t(xs), t(dz)
        trials = [(dxu + a * ddz).contiguous() for a in STEPS]                  # the nine iterates the KKT route assembles at
        merit = torch.empty(B, len(STEPS), device=dev)
        args = (iiwa.TIMESTEP, 10.0, iiwa.QD_COST, iiwa.r_cost(N))
        G = torch.empty(B, (14 * 14 + 7 * 7) * N - 7 * 7, device=dev)
        Cd = torch.empty(B, (14 * 14 + 14 * 7) * (N - 1), device=dev)
        g = torch.empty(B, 21 * N - 7, device=dev)
        c = torch.empty(B, 14 * N, device=dev)
        lib, h, pl = sol.lib, sol._h, plant._p
        p = lambda x: C.c_void_p(x.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        steps = (C.c_float * len(STEPS))(*STEPS)

        def new():                                                              # (both straight through the C ABI: the same host cost per call)
            rc = lib.mpcg_compute_merit(h, pl, 7, args[0], p(dee), p(dxs), p(dxu), p(ddz), steps, len(STEPS), args[1], args[2], args[3], p(merit), B, stream)
            assert rc == 0

        def old():
            for z in trials:
                rc = lib.mpcg_generate_kkt(h, pl, 7, iiwa.TIMESTEP, p(dee), p(dxs), p(z), iiwa.QD_COST, iiwa.r_cost(N), p(G), p(Cd), p(g), p(c), B, stream)
                assert rc == 0

        _, rounds = alternate((new, old), reps, windows=ROUNDS, warmup_rounds=3)
        res = {"knots": N, "batch": B, "reps": reps, "compute_merit_us": [round(a, 2) for a, _ in rounds], "nine_kkt_calls_us": [round(b, 2) for _, b in rounds],
               "ratio": [round(b / a, 2) for a, b in rounds], "faster_in_every_round": all(a < b for a, b in rounds)}
        print(json.dumps(res), flush=True)
        out.append(res)
    return 0 if all(r["faster_in_every_round"] for r in out) else 1


if __name__ == "__main__":
    sys.exit(main())
