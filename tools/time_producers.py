#!/usr/bin/env python3
"""Time the steps either side of the solve at any (state_size, control_size):  time_producers.py [--state n] [--control m] [--knots N] [--batch B]
[--generic] [--rho-vector] [--json] — mpcg_form_schur (symmetric stair), mpcg_compute_dz and mpcg_block_solve, each with its rate on the shape's own
algorithmic HBM bytes (formation: G, C, g, c in, S, Pinv, gamma, G^-1 out; dz: G^-1, C, g, lambda in, dz out; block solve: S, gamma in,
lambda out).  At 14 x 7 the default (register-resident) kernels are timed and, with --generic, the run-time-dimension LDS kernels of
schur_generic.hip.h ("producers_generic" = 1) every other shape runs anyway (for formation and dz also what "schur_dpp" = "dz_dpp" = 0 runs).
Every figure is the median of seven timed calls behind 50 ms of back-to-back calls.
--rho-vector times the formation alone, float and double: mpcg_form_schur(_f64) with a scalar rho against mpcg_form_schur_rhov(_f64) with a device
vector of the same value, ALTERNATED call by call in one process behind a common warm-up — median and min-max of seven calls each."""
import argparse, json, sys, time
import numpy as np, torch
from ab_timing import alternate, min_max, select_build
select_build()
from mpcgpu_amd import PcgSolver, synth

ap = argparse.ArgumentParser()
ap.add_argument("--state", type=int, default=14)
ap.add_argument("--control", type=int, default=7)
ap.add_argument("--knots", type=int, default=128)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--generic", action="store_true", help="14 x 7 only: also time the run-time-dimension kernels")
ap.add_argument("--rho-vector", action="store_true", help="formation only: the scalar entry against the rho-vector entry, alternated, float and double")
ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth the achieved fraction refers to (TB/s)")
ap.add_argument("--json", action="store_true")
a = ap.parse_args()
n, m, N, B = a.state, a.control, a.knots, a.batch
tuned = (n, m) == (14, 7)


def make(Bs):
    """Well-conditioned blocks for any 1 <= m <= n (the generator of tests/test_generic_producers_cpu.py)."""
    rng = np.random.default_rng([1, n, m])
    W = rng.standard_normal((Bs, N, n, n)); Q = np.einsum("bkia,bkja->bkij", W, W) / n + 0.5 * np.eye(n)
    V = rng.standard_normal((Bs, N - 1, m, m)); R = np.einsum("bkia,bkja->bkij", V, V) / m + 0.5 * np.eye(m)
    A = np.eye(n) + 0.3 * rng.standard_normal((Bs, N - 1, n, n)) / np.sqrt(n)
    Bm = 0.5 * rng.standard_normal((Bs, N - 1, n, m))
    c = np.zeros((Bs, N, n)); c[:, 1:] = 0.1 * rng.standard_normal((Bs, N - 1, n))
    return synth.KKT(Q, R, A, Bm, rng.standard_normal((Bs, N, n)), rng.standard_normal((Bs, N - 1, m)), c)


sol = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
Bs = min(B, 16)
rep = (B + Bs - 1) // Bs
G, C, g, c = (torch.from_numpy(x).cuda().repeat(rep, 1)[:B].contiguous() for x in synth.pack_kkt_dense(make(Bs), np.float32))
G0 = G.clone()
S = torch.zeros(B, 3 * n * n * N, device="cuda"); P = torch.zeros_like(S); gm = torch.empty(B, n * N, device="cuda")
lam = torch.randn(B, n * N, device="cuda"); dz = torch.empty(B, (n + m) * N - m, device="cuda"); lam_d = torch.empty_like(lam)


def t(fn, restore=False, reps=9):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.05:           # back-to-back warm-up: the clocks are up before anything is timed
        fn()
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        if restore:
            G.copy_(G0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    return float(np.median(ts[2:])) * 1e3            # us


def rho_vector_ab():
    for dt in (torch.float32, torch.float64):
        Gd, Cd, gd, cd = (x.to(dt) for x in (G0, C, g, c))
        G0d = Gd.clone()
        Sd = torch.zeros(B, 3 * n * n * N, device="cuda", dtype=dt); Pd = torch.zeros_like(Sd); gmd = torch.empty(B, n * N, device="cuda", dtype=dt)
        vec = torch.full((B,), 1e-3, device="cuda", dtype=dt)
        calls = {"scalar": lambda: sol.form_schur(Gd, Cd, gd, cd, 1e-3, "ss", S=Sd, Pinv=Pd, gamma=gmd),
                 "vector": lambda: sol.form_schur(Gd, Cd, gd, cd, vec, "ss", S=Sd, Pinv=Pd, gamma=gmd)}
        med, rounds = alternate(list(calls.values()), 1, reset=lambda: Gd.copy_(G0d), warmup_s=0.1)      # (the formation works on G in place)
        for i, k in enumerate(calls):
            lo, hi = min_max(rounds, i)
            rec = {"state": n, "control": m, "knots": N, "batch": B, "dtype": str(dt).split(".")[1], "rho": k, "step": "form_schur", "chunk": sol.get_option("last_schur_chunk"),
                   "median_us": round(med[i], 2), "min_us": round(lo, 2), "max_us": round(hi, 2)}
            print(json.dumps(rec) if a.json else "(%2d,%2d) %4d x %-4d %-8s rho %-7s form_schur  median %9.1f us  (min %.1f, max %.1f)"
                  % (n, m, B, N, rec["dtype"], k, rec["median_us"], rec["min_us"], rec["max_us"]))


if a.rho_vector:
    rho_vector_ab()
    sys.exit(0)

nn, mm, nm = n * n, m * m, n * m
model = {"form_schur": 4 * (9 * nn + 2 * mm + nm + 3 * n + m), "compute_dz": 4 * (2 * nn + mm + nm + 3 * n + 2 * m), "block_solve": 4 * (3 * nn + 2 * n)}
routes = [("default", {})]
if tuned:
    routes = [("default", {"schur_dpp": 1, "dz_dpp": 1, "producers_generic": 0})]
    if a.generic:
        routes.append(("generic", {"producers_generic": 1}))
for route, opts in routes:
    for key, v in opts.items():
        sol.set_option(key, v)
    us = {"form_schur": t(lambda: sol.form_schur(G, C, g, c, 1e-3, "ss", S=S, Pinv=P, gamma=gm), restore=True)}
    G.copy_(G0); sol.form_schur(G, C, g, c, 1e-3, "ss", S=S, Pinv=P, gamma=gm)
    us["compute_dz"] = t(lambda: sol.compute_dz(G, C, g, lam, dz=dz))
    us["block_solve"] = t(lambda: sol.block_solve(S, gm, lam_d))
    for step, u in us.items():
        tbs = B * N * model[step] / u / 1e6
        rec = {"state": n, "control": m, "knots": N, "batch": B, "route": route, "step": step, "us": round(u, 2), "bytes_per_knot": model[step],
               "tb_per_s": round(tbs, 4), "hbm_fraction": round(tbs / a.hbm_tbs, 4)}
        print(json.dumps(rec) if a.json else "(%2d,%2d) %4d x %-4d %-8s %-12s %9.1f us  %7.3f TB/s = %5.1f %% of %.1f TB/s on %d B/knot"
              % (n, m, B, N, route, step, u, tbs, 100 * tbs / a.hbm_tbs, a.hbm_tbs, model[step]))
