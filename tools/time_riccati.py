#!/usr/bin/env python3
"""Time the Riccati feedback gains against the sibling serial sweep of the path, on one handle in ONE process, alternated window by window:
    gains      mpcg_riccati_gains      — float blocks widened on load, float64 inside, K rounded on store
    gains_f64  mpcg_riccati_gains_f64
    block_f64  mpcg_block_solve_f64    — the block-tridiagonal direct solve in double: one dependent chain per trajectory too
Shapes: 1024 trajectories x 128 knots (the throughput call) and one trajectory x 32 knots (the MPC loop's own call), 14 x 7, synthetic
IIWA-shaped KKT blocks; the Schur system of the direct solve is formed from the same blocks (after the gains: the formation overwrites G).
After 50 ms of back-to-back warm-up launches of all three: device events around `reps` back-to-back calls, medians of seven windows.
Before the timing the float entry's gains are compared with the double entry's (relative to max |K|).  One JSON line per shape.  No time is
promised: nobody had measured this kernel.  Needs an MI355X:
    [AB_LIB=<another build's libmpcg_hip.so>] python tools/time_riccati.py [reps]"""
import json
import sys

import numpy as np
import torch

from ab_timing import alternate, select_build, windows_of

select_build()
from mpcgpu_amd import PcgSolver, synth  # noqa: E402

RHO = 1e-3


def main():
    reps_arg = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    dev = torch.device("cuda", 0)
    for N, B in ((128, 1024), (32, 1)):
        reps = reps_arg or (200 if B == 1 else 20)
        sol = PcgSolver(N, max_batch=B)
        parts = [synth.pack_kkt_dense(synth.make_kkt(N, min(128, B - lo), 900000 + lo), np.float64) for lo in range(0, B, 128)]
        G64, C64, g64, c64 = (torch.from_numpy(np.concatenate([p[i] for p in parts])).to(dev) for i in range(4))
        G32, C32 = G64.float(), C64.float()
        K32, K64 = torch.empty(B, (N - 1) * 98, device=dev), torch.empty(B, (N - 1) * 98, device=dev, dtype=torch.float64)
        sol.riccati_gains(G32, C32, RHO, K=K32)
        sol.riccati_gains(G64, C64, RHO, K=K64)
        torch.cuda.synchronize()
        k64 = K64.cpu().numpy()
        diff = float(np.abs(K32.cpu().numpy() - k64).max() / np.abs(k64).max())
        S, _, gam = sol.form_schur(G64.clone(), C64, g64, c64, RHO, "none")
        lam = torch.empty(B, 14 * N, device=dev, dtype=torch.float64)
        calls = [lambda: sol.riccati_gains(G32, C32, RHO, K=K32), lambda: sol.riccati_gains(G64, C64, RHO, K=K64), lambda: sol.block_solve(S, gam, lam)]
        med, rounds = alternate(calls, reps)
        print(json.dumps({"knots": N, "batch": B, "reps": reps, "gains_us": round(med[0], 2), "gains_f64_us": round(med[1], 2), "block_f64_us": round(med[2], 2),
                          "gains_f64_over_block_f64": round(med[1] / med[2], 3), "finite": bool(np.isfinite(k64).all() and torch.isfinite(lam).all()),
                          "float_vs_f64": float(f"{diff:.3g}"), "windows": windows_of(rounds)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
