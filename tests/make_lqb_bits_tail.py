#!/usr/bin/env python3
"""Record the bits of the lane-quad PCG kernel (pcg_lqb.hip.h, family 11) on the paths tests/make_lqb_bits.py leaves out, for
tests/test_gpu_lqb_bits_tail.py.

Run ONCE, on the GPU, on the commit whose results a re-cut of a pass's tail has to reproduce bit for bit:
    python tests/make_lqb_bits_tail.py [--commit HASH]      ->  tests/golden/lqb_bits_tail_parent.npz
(HASH defaults to `git rev-parse HEAD`; it is stored in the file.)

The first record starts every solve from lambda = 0 (so the set-up S pass multiplies zeros) and, at the ragged horizon, has four trajectories
of one seed.  Here: batch 3, "pcg_lqb" = 1, a seeded RANDOM lambda0 everywhere, and horizons whose last wavefront is partly or almost
wholly empty, so that the masked publishing stores and the zeroed sub-blocks of absent knots are on the compared path:
  * N = 128 and N = 100 (four of the last wavefront's 16 knots), SS, exit_tol 0 at max_iter 1, 2 and 167;
  * N = 113 (one knot in the last wavefront), block-Jacobi, max_iter 2;
  * N = 17 (the 32-knot build; one knot in its second wavefront), SS, max_iter 10;
  * N = 128, SS, the reference-style entry (solve_ref) with d_r / d_p: at an iteration-cap exit, where the last update of p is still pending
    and the write-back forms it, and at a tolerance exit, where it is not — the tolerance chosen from a ladder as make_lqb_bits.py does.
Stored: outputs only, a digest of the inputs (lambda0 included) and the commit hash.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_lqb_bits as M0  # noqa: E402  (the input masking and the tolerance ladder of the first record)

OUT = os.path.join(ROOT, "tests", "golden", "lqb_bits_tail_parent.npz")

BATCH = 3
# (horizon, preconditioner, iteration caps) of the batched solves
CASES = ((128, "ss", (1, 2, 167)), (100, "ss", (1, 2, 167)), (113, "jacobi", (2,)), (17, "ss", (10,)))
REF_N, REF_CAP = 128, 5                       # solve_ref at a cap exit: horizon, iterations (SS, trajectory 1)
REF_TRAJ = 1


def seed_of(N, pc):
    return 7000 + 2 * N + (pc == "jacobi")


def inputs(N, pc):
    """(S, Pinv, gamma, lambda0) float32 [BATCH, ...] of the seeded system + the digest of their bytes."""
    from mpcgpu_amd import synth
    k = synth.make_kkt(N, BATCH, seed_of(N, pc))
    S, Pinv, g = (M0._mask8(a) for a in synth.form_schur(k, precond=pc))
    lam0 = M0._mask8(np.random.default_rng(seed_of(N, pc) + 100000).standard_normal((BATCH, 14 * N)))
    assert (lam0 != 0).all()
    h = hashlib.sha256()
    for a in (S, Pinv, g, lam0):
        h.update(a.tobytes())
    return S, Pinv, g, lam0, h.hexdigest()


def key(N, pc, what):
    return f"N{N}_{pc}_{what}"


def solve(N, pc, S, Pinv, g, lam0, max_iter, tol):
    """Batched PcgSolver.solve from lambda0 with the lane-quad kernel pinned: (lambda, pcg_iters, pcg_exit) as numpy."""
    import torch
    from mpcgpu_amd import PcgSolver, pcg_config
    sol = PcgSolver(N, max_batch=BATCH)
    sol.set_option("pcg_lpk", 1)
    sol.set_option("pcg_lqb", 1)
    sol.set_option("assume_symmetric", 1)
    lam = torch.from_numpy(lam0.copy()).cuda()
    it, ex = sol.solve(torch.from_numpy(S).cuda(), torch.from_numpy(Pinv).cuda(), torch.from_numpy(g).cuda(), lam,
                       pcg_config(pcg_exit_tol=tol, pcg_max_iter=max_iter), pc)
    torch.cuda.synchronize()
    assert sol.get_option("last_kernel_family") == 11, (N, pc, sol.get_option("last_kernel_family"))
    return lam.cpu().numpy(), it.cpu().numpy().astype(np.int32), ex.cpu().numpy().astype(np.uint8)


def solve_ref(N, S, Pinv, g, lam0, max_iter, tol):
    """The reference-style entry on trajectory REF_TRAJ (SS) from lambda0: (lambda, d_r, d_p, iters, exit)."""
    import torch
    from mpcgpu_amd import PcgSolver
    t = REF_TRAJ
    sol = PcgSolver(N)
    sol.set_option("pcg_lpk", 1)
    sol.set_option("pcg_lqb", 1)
    sol.set_option("assume_symmetric", 1)
    d_lambda = torch.from_numpy(lam0[t].copy()).cuda()
    d_r = torch.full((14 * N,), 7.0, device="cuda")
    d_p = torch.full((14 * N,), 7.0, device="cuda")
    d_it = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_ex = torch.zeros(1, dtype=torch.bool, device="cuda")
    sol.solve_ref(torch.from_numpy(S[t].copy()).cuda(), torch.from_numpy(Pinv[t].copy()).cuda(), torch.from_numpy(g[t].copy()).cuda(),
                  d_lambda, d_r, d_p, torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), d_it, d_ex, max_iter, tol)
    torch.cuda.synchronize()
    assert sol.get_option("last_kernel_family") == 11
    return (d_lambda.cpu().numpy(), d_r.cpu().numpy(), d_p.cpu().numpy(), d_it.cpu().numpy().astype(np.int32),
            d_ex.cpu().numpy().astype(np.uint8))


REF_NAMES = ("lambda", "d_r", "d_p", "iters", "exit")


def main():
    if "--commit" in sys.argv:
        commit = sys.argv[sys.argv.index("--commit") + 1]
    else:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    out = {"commit": np.array(commit)}
    for N, pc, caps in CASES:
        S, Pinv, g, lam0, digest = inputs(N, pc)
        out[key(N, pc, "inputs_sha256")] = np.array(digest)
        for K in caps:
            lam, it, ex = solve(N, pc, S, Pinv, g, lam0, K, 0.0)
            assert (it == K).all() and (ex == 1).all(), (N, pc, K, it, ex)
            assert np.isfinite(lam).all() and (lam != lam0).any()
            out[key(N, pc, f"K{K}_lambda")], out[key(N, pc, f"K{K}_iters")], out[key(N, pc, f"K{K}_exit")] = lam, it, ex
    S, Pinv, g, lam0, _ = inputs(REF_N, "ss")
    res = solve_ref(REF_N, S, Pinv, g, lam0, REF_CAP, 0.0)
    assert res[3][0] == REF_CAP and res[4][0] == 1 and all(np.isfinite(a).all() for a in res[:3])
    for name, a in zip(REF_NAMES, res):
        out["refcap_" + name] = a
    # the first tolerance of the ladder that the trajectory meets strictly inside the loop
    for tol in M0.TOL_LADDER:
        res = solve_ref(REF_N, S, Pinv, g, lam0, 167, tol)
        if res[4][0] == 0 and 3 <= res[3][0] < 160:
            break
    else:
        raise SystemExit("no tolerance of the ladder exits inside the loop")
    print(f"solve_ref N={REF_N}: tolerance {tol:g} -> {int(res[3][0])} iterations")
    assert all(np.isfinite(a).all() for a in res[:3])
    out["reftol_tol"] = np.array(tol, np.float64)
    for name, a in zip(REF_NAMES, res):
        out["reftol_" + name] = a
    np.savez(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes, commit", commit)


if __name__ == "__main__":
    main()
