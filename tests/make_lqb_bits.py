#!/usr/bin/env python3
"""Record the bits of the lane-quad PCG kernel (pcg_lqb.hip.h, family 11) for tests/test_gpu_lqb_bits.py.

Run ONCE, on the GPU, on the commit whose results a re-scheduling of the kernel's loop has to reproduce bit for bit:
    python tests/make_lqb_bits.py [--commit HASH]      ->  tests/golden/lqb_bits_parent.npz
(HASH defaults to `git rev-parse HEAD`; it is stored in the file.)

Cases: seeded mpcgpu_amd.synth systems at N = 128, 64, 32 and the ragged horizon 100, SS and block-Jacobi, four trajectories,
"pcg_lqb" = 1 (family 11 at every size), exit_tol 0 at max_iter 1, 10 and 167; one tolerance exit per preconditioner; and d_r / d_p of the
reference-style entry (solve_ref) for N = 128.  Stored: lambda, pcg_iters, pcg_exit (and d_r, d_p) — outputs only; the inputs are rebuilt
from the seed, and a digest of them is stored so that a replay on other inputs is told apart from a kernel that computes other bits.

The inputs are formed in float64 by numpy (LAPACK inverses) and cast to float32.  Their low eight mantissa bits are cleared, so that a
LAPACK build that differs in the last bits of a double still gives the same float32 inputs (a change of the rounded value would need the
double to sit within 2^-29 relative of a break point).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "lqb_bits_parent.npz")

BATCH = 4
HORIZONS = (128, 64, 32, 100)
PRECONDS = ("ss", "jacobi")
MAX_ITERS = (1, 10, 167)
TOL_CASES = ((128, "ss"), (64, "jacobi"))      # one tolerance exit per preconditioner
TOL_LADDER = tuple(10.0 ** -e for e in range(1, 16))
REF_CASE = (128, 20)                          # solve_ref: horizon, iterations (SS, trajectory 0)


def seed_of(N, pc):
    return 9000 + 2 * N + (pc == "jacobi")


def _mask8(a):
    a = np.ascontiguousarray(a, np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)


def inputs(N, pc):
    """(S, Pinv, gamma) float32 [BATCH, ...] of the seeded system + the digest of their bytes."""
    from mpcgpu_amd import synth
    k = synth.make_kkt(N, BATCH, seed_of(N, pc))
    S, Pinv, g = (_mask8(a) for a in synth.form_schur(k, precond=pc))
    h = hashlib.sha256()
    for a in (S, Pinv, g):
        h.update(a.tobytes())
    return S, Pinv, g, h.hexdigest()


def key(N, pc, what):
    return f"N{N}_{pc}_{what}"


def solve(N, pc, S, Pinv, g, max_iter, tol):
    """Batched PcgSolver.solve from lambda = 0 with the lane-quad kernel pinned: (lambda, pcg_iters, pcg_exit) as numpy."""
    import torch
    from mpcgpu_amd import PcgSolver, pcg_config
    sol = PcgSolver(N, max_batch=BATCH)
    sol.set_option("pcg_lpk", 1)
    sol.set_option("pcg_lqb", 1)
    sol.set_option("assume_symmetric", 1)
    lam = torch.zeros(BATCH, 14 * N, device="cuda")
    it, ex = sol.solve(torch.from_numpy(S).cuda(), torch.from_numpy(Pinv).cuda(), torch.from_numpy(g).cuda(), lam,
                       pcg_config(pcg_exit_tol=tol, pcg_max_iter=max_iter), pc)
    torch.cuda.synchronize()
    assert sol.get_option("last_kernel_family") == 11, (N, pc, sol.get_option("last_kernel_family"))
    return lam.cpu().numpy(), it.cpu().numpy().astype(np.int32), ex.cpu().numpy().astype(np.uint8)


def solve_ref(N, S, Pinv, g, max_iter):
    """The reference-style entry on trajectory 0 (SS): (lambda, d_r, d_p, iters, exit)."""
    import torch
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N)
    sol.set_option("pcg_lpk", 1)
    sol.set_option("pcg_lqb", 1)
    sol.set_option("assume_symmetric", 1)
    d_lambda = torch.zeros(14 * N, device="cuda")
    d_r = torch.full((14 * N,), 7.0, device="cuda")
    d_p = torch.full((14 * N,), 7.0, device="cuda")
    d_it = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_ex = torch.zeros(1, dtype=torch.bool, device="cuda")
    sol.solve_ref(torch.from_numpy(S[0].copy()).cuda(), torch.from_numpy(Pinv[0].copy()).cuda(), torch.from_numpy(g[0].copy()).cuda(),
                  d_lambda, d_r, d_p, torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), d_it, d_ex, max_iter, 0.0)
    torch.cuda.synchronize()
    assert sol.get_option("last_kernel_family") == 11
    return (d_lambda.cpu().numpy(), d_r.cpu().numpy(), d_p.cpu().numpy(), d_it.cpu().numpy().astype(np.int32),
            d_ex.cpu().numpy().astype(np.uint8))


def main():
    commit = None
    if "--commit" in sys.argv:
        commit = sys.argv[sys.argv.index("--commit") + 1]
    else:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    out = {"commit": np.array(commit)}
    for N in HORIZONS:
        for pc in PRECONDS:
            S, Pinv, g, digest = inputs(N, pc)
            out[key(N, pc, "inputs_sha256")] = np.array(digest)
            for K in MAX_ITERS:
                lam, it, ex = solve(N, pc, S, Pinv, g, K, 0.0)
                assert (it == K).all() and (ex == 1).all(), (N, pc, K, it, ex)
                assert np.isfinite(lam).all()
                out[key(N, pc, f"K{K}_lambda")], out[key(N, pc, f"K{K}_iters")], out[key(N, pc, f"K{K}_exit")] = lam, it, ex
            if (N, pc) in TOL_CASES:
                # the first tolerance of the ladder that every trajectory meets strictly inside the loop
                for tol in TOL_LADDER:
                    lam, it, ex = solve(N, pc, S, Pinv, g, 167, tol)
                    if (ex == 0).all() and (it >= 3).all() and (it < 160).all():
                        break
                else:
                    raise SystemExit(f"no tolerance of the ladder exits inside the loop for N={N} {pc}")
                print(f"N={N} {pc}: tolerance {tol:g} -> iterations {it.tolist()}")
                out[key(N, pc, "tol")] = np.array(tol, np.float64)
                out[key(N, pc, "tol_lambda")], out[key(N, pc, "tol_iters")], out[key(N, pc, "tol_exit")] = lam, it, ex
    N, K = REF_CASE
    S, Pinv, g, _ = inputs(N, "ss")
    lam, r, p, it, ex = solve_ref(N, S, Pinv, g, K)
    assert it[0] == K and np.isfinite(r).all() and np.isfinite(p).all()
    out["ref_lambda"], out["ref_d_r"], out["ref_d_p"], out["ref_iters"], out["ref_exit"] = lam, r, p, it, ex
    np.savez(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes, commit", commit)


if __name__ == "__main__":
    main()
