#!/usr/bin/env python3
"""Time ONE batched SQP iteration as a hipGraph replay:  time_sqp_iteration.py [--knots N] [--batch B] [--json]
    generate_kkt -> form_schur (SS) -> pcg solve -> compute_dz -> compute_merit (8 step sizes) -> line-search step
in two builds of the same chain on the same iterate: "scalar" (mpcg_form_schur with a host rho + mpcg_line_search_step: what
examples/sqp_batched_iiwa runs without --adapt-rho) and "adaptive" (mpcg_form_schur_rhov reading the rho vector + mpcg_line_search_step_rho).
Each is captured once after an eager iteration; the replays are ALTERNATED in one process behind a common warm-up, every timed replay starts
from the same saved state (restored outside the timed region): median and min-max of seven replays each, device events."""
import argparse, json
import numpy as np, torch
from ab_timing import alternate, min_max, select_build
select_build()
from mpcgpu_amd import PcgSolver, Plant, iiwa, pcg_config

ap = argparse.ArgumentParser()
ap.add_argument("--knots", type=int, default=128)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--json", action="store_true")
a = ap.parse_args()
N, B = a.knots, a.batch
STEPS = [-1.0 / (1 << p) for p in range(8)]
plant = Plant()
cfg = pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=3000)
xu0, goals, xs = iiwa.random_windows(N, min(B, 16), 5)
up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda().repeat((B + 15) // 16, 1)[:B].contiguous()
goals, xs, xu0 = up(goals.reshape(len(goals), -1)), up(xs), up(xu0)
tail = (iiwa.TIMESTEP, 10.0, iiwa.QD_COST, iiwa.r_cost(N))


class Chain:
    def __init__(self, adaptive):
        self.adaptive, self.sol = adaptive, PcgSolver(N, max_batch=B)
        self.state = dict(xu=xu0.clone(), lam=torch.zeros(B, 14 * N, device="cuda"), rho=torch.full((B,), 1e-3, device="cuda"),
                          drho=torch.ones(B, device="cuda"), done=torch.zeros(B, dtype=torch.uint8, device="cuda"))
        self.state["ref"] = self.sol.compute_merit(plant, goals, xs, self.state["xu"], None, [0.0], *tail).reshape(B).clone()
        self.step = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.saved = {k: v.clone() for k, v in self.state.items()}
        self.iteration()                                     # eager: every handle-owned buffer exists before the capture
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.iteration()

    def iteration(self):
        s, st = self.sol, self.state
        G, Cd, g, c = s.generate_kkt(plant, goals, xs, st["xu"], iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(N))
        S, Pinv, gam = s.form_schur(G, Cd, g, c, st["rho"] if self.adaptive else 1e-3, "ss")
        s.solve(S, Pinv, gam, st["lam"], cfg, "ss")
        dz = s.compute_dz(G, Cd, g, st["lam"])
        merit = s.compute_merit(plant, goals, xs, st["xu"], dz, STEPS, *tail)
        if self.adaptive:
            s.line_search_step_rho(merit, STEPS, st["ref"], dz, st["xu"], st["rho"], st["drho"], st["done"], step=self.step)
        else:
            s.line_search_step(merit, STEPS, st["ref"], dz, st["xu"], step=self.step)

    def restore(self):
        for k, v in self.saved.items():
            self.state[k].copy_(v)


chains = {"scalar": Chain(False), "adaptive": Chain(True)}
med, rounds = alternate([ch.graph.replay for ch in chains.values()], 1, reset=[ch.restore for ch in chains.values()], warmup_s=0.2)
for i, k in enumerate(chains):
    lo, hi = min_max(rounds, i)
    rec = {"knots": N, "batch": B, "chain": k, "median_us": round(med[i], 2), "min_us": round(lo, 2), "max_us": round(hi, 2)}
    print(json.dumps(rec) if a.json else "%4d x %-4d %-8s iteration (graph replay)  median %9.1f us  (min %.1f, max %.1f)" % (B, N, k, rec["median_us"], rec["min_us"], rec["max_us"]))
