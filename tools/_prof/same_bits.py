#!/usr/bin/env python3
"""Do two builds of the library compute the same bits in the lane-pair / lane-quad PCG kernels (families 6, 7, 9, 10)?  For a change that
re-arranges their source without meaning to change a result.  One process per build, then a byte compare:
    AB_LIB=old/libmpcg_hip.so python tools/_prof/same_bits.py old.npz
    AB_LIB=new/libmpcg_hip.so python tools/_prof/same_bits.py new.npz
    python tools/_prof/same_bits.py --compare old.npz new.npz          (or cmp: the files carry no time stamps)
Cases: seeded mpcgpu_amd.synth systems, batch 3, lambda0 = 0, "assume_symmetric" = 1, SS and block-Jacobi, exit_tol 0 at max_iter 1 and 10, at the
smallest horizons at which each build of each kernel can go wrong; fp16 storage (lane-pair); "cluster_l2" 1 and 0 (clustered); one tolerance
exit and one solve_ref call (d_r, d_p) per kernel.  last_kernel_family is asserted in every case.  Stored: lambda, iterations, exit flags."""
import os, sys, zipfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

B = 3
# family: (double?, options, horizons)
KERNELS = {
    6: (False, {"pcg_lpk": 1, "pcg_lqb": 0}, (2, 17, 32, 33, 64, 65, 100, 128)),      # lane-pair: half build | 64 knots | 128 knots
    7: (False, {}, (129, 300, 64)),                                                    # clustered lane-pair: automatic; N = 64: "cluster" = 2
    9: (True, {"pcg_lqk": 1}, (2, 31, 32, 33, 57, 64)),                                # lane-quad double: 32 knots | 64 knots
    10: (True, {}, (65, 100, 200, 512)),                                               # clustered lane-quad double
}
EXTRA = {6: 100, 7: 129, 9: 57, 10: 100}                                               # horizon of the tolerance exit and of solve_ref


def compare(a, b):
    fa, fb = np.load(a), np.load(b)
    bad = [k for k in sorted(set(fa.files) | set(fb.files))
           if k not in fa.files or k not in fb.files or fa[k].dtype != fb[k].dtype or fa[k].tobytes() != fb[k].tobytes()]
    same_file = open(a, "rb").read() == open(b, "rb").read()
    print(f"{a} vs {b}: {len(fa.files)} / {len(fb.files)} arrays, {len(bad)} differ; files byte-identical: {same_file}")
    for k in bad[:20]:
        print("   differs:", k)
    sys.exit(1 if bad or not same_file else 0)


if sys.argv[1] == "--compare":
    compare(sys.argv[2], sys.argv[3])
import torch
from mpcgpu_amd import _lib
if os.environ.get("AB_LIB"):
    _lib.LIB_PATH = os.environ["AB_LIB"]
from mpcgpu_amd import PcgSolver, pcg_config, synth
out, systems = {}, {}


def system(N, pc, dbl):
    if (N, pc, dbl) not in systems:
        k = synth.make_kkt(N, B, 7000 + 2 * N + (pc == "jacobi"))
        systems[(N, pc, dbl)] = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda()
                                      for a in synth.form_schur(k, precond=pc, dtype=np.float64 if dbl else np.float32))
    return systems[(N, pc, dbl)]


def solver(fam, N, l2, batch=B):
    sol = PcgSolver(N, max_batch=batch)
    sol.set_option("assume_symmetric", 1)
    for o, v in KERNELS[fam][1].items():
        sol.set_option(o, v)
    if fam == 7 and N <= 128:
        sol.set_option("cluster", 2)
    if fam in (7, 10):
        sol.set_option("cluster_l2", l2)
    return sol


def put(key, sol, fam, *arrays):
    torch.cuda.synchronize()
    assert sol.get_option("last_kernel_family") == fam, (key, sol.get_option("last_kernel_family"))
    for nm, a in zip(("lambda", "iters", "exit", "d_r", "d_p"), arrays):
        out[f"{key}_{nm}"] = a.cpu().numpy()


for fam, (dbl, _, horizons) in KERNELS.items():
    dt = torch.float64 if dbl else torch.float32
    for N in horizons:
        for l2 in ((1, 0) if fam in (7, 10) else (1,)):
            sol = solver(fam, N, l2)
            run = sol.solve_f64 if dbl else sol.solve
            for pc in ("ss", "jacobi"):
                S, P, g = system(N, pc, dbl)
                cases = [(f"K{K}", run, (S, P), K, 0.0) for K in (1, 10)]
                if fam == 6 and N == 64:
                    cases += [(f"f16_K{K}", sol.solve_f16, (sol.to_f16(S), sol.to_f16(P)), K, 0.0) for K in (1, 10)]
                if N == EXTRA[fam] and pc == "ss":
                    cases += [("tol", run, (S, P), 5000 if dbl else 400, 1e-10 if dbl else 1e-5)]
                for name, fn, (dS, dP), K, tol in cases:
                    lam = torch.zeros(B, 14 * N, dtype=dt, device="cuda")
                    it, ex = fn(dS, dP, g, lam, pcg_config(pcg_exit_tol=tol, pcg_max_iter=K), pc)
                    put(f"fam{fam}_N{N}_l2{l2}_{pc}_{name}", sol, fam, lam, it, ex)
                    if name == "tol":
                        print(f"family {fam} N={N} l2={l2}: tolerance {tol:g} -> iterations {it.tolist()} exit {ex.tolist()}")
            sol.close()
    # the reference-style entry on trajectory 0 (SS, 10 iterations): d_r and d_p
    N = EXTRA[fam]
    sol = solver(fam, N, 1, batch=1)
    S, P, g = system(N, "ss", dbl)
    d_lam = torch.zeros(14 * N, dtype=dt, device="cuda")
    d_r, d_p = (torch.full((14 * N,), 7.0, dtype=dt, device="cuda") for _ in range(2))
    scr = torch.zeros(14 * N, dtype=dt, device="cuda")
    d_it = torch.zeros(1, dtype=torch.int32, device="cuda"); d_ex = torch.zeros(1, dtype=torch.uint8, device="cuda")
    (sol.solve_ref_f64 if dbl else sol.solve_ref)(S[0].contiguous(), P[0].contiguous(), g[0].contiguous(), d_lam, d_r, d_p, scr, scr, d_it, d_ex, 10, 0.0)
    put(f"fam{fam}_N{N}_ref", sol, fam, d_lam, d_it, d_ex, d_r, d_p)
    sol.close()

assert all(np.isfinite(a).all() for a in out.values())
with zipfile.ZipFile(sys.argv[1], "w") as z:                       # (np.savez stamps every member with the time of day)
    for k in sorted(out):
        with z.open(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as f:
            np.lib.format.write_array(f, np.ascontiguousarray(out[k]), allow_pickle=False)
print(f"wrote {sys.argv[1]}: {len(out)} arrays, library {_lib.LIB_PATH}")
