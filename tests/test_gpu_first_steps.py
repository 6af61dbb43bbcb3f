"""GPU: the first two iterations of the BATCHED entries (mpcg_pcg_solve, mpcg_pcg_solve_f16, mpcg_pcg_solve_f64), which return only lambda,
against their prediction from the inputs alone — first_steps_quantities of tests/pcg_step_model.py: lambda after max_iter = 1 and after
max_iter = 2 (exit_tol = 0), the difference divided ELEMENTWISE by u x the size of the terms at that element, so a wrong value at a knot whose
entries are 100 x smaller than the vector's largest fails as it would at the largest.  Rows: tests/pcg_step_cases.py, the inputs the CPU test
tests/test_pcg_step_model_cpu.py runs the oracle on.

What only these entries reach: the block-Jacobi BUILDS (MPCG_PRECOND_JACOBI; every off-diagonal block of Pinv is NaN here, so a build that
reads one returns NaN), fp16 storage, trajectories that are not workgroup 0 of their launch, and workgroups sharing a CU.

Measured worst values per family on an MI355X: profiles/pcg_step_model.txt."""
import numpy as np
import pytest
import torch

import pcg_step_cases as cases
from pcg_step_model import EPS32, FIRST_STEPS_LIMIT, HP, first_steps_quantities

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
ROWS14 = [r for r in cases.ROWS if r.n == 14]
ROWS_GENERIC = [r for r in cases.ROWS if r.n != 14]
TILED = [r for r in cases.ROWS32 if r.n == 14 and r.family in (5, 6, 11) and r.N in (17, 33)]


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()              # (a copy: the shared systems are read-only)


def solver(r, max_batch):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(r.N, max_batch=max_batch, state_size=r.n)
    for key, value in r.opts:
        sol.set_option(key, value)
    if cases.reads_lower(r):                               # the caller vouches for block symmetry: no guard launch next to the kernel under test
        sol.set_option("assume_symmetric", 1)
    return sol


def solve(sol, entry, dS, dP, dg, dlam0, K, pc):
    """One call of the batched entry from lambda0 (device, not touched): lambda on the host; iteration counts and flags asserted."""
    from mpcgpu_amd import pcg_config
    lam = dlam0.clone()
    it, ex = getattr(sol, entry)(dS, dP, dg, lam, pcg_config(pcg_exit_tol=0.0, pcg_max_iter=K), pc)
    torch.cuda.synchronize()
    assert (it.cpu().numpy() == K).all() and (ex.cpu().numpy() == 1).all(), (K, it.cpu().numpy(), ex.cpu().numpy())
    return lam.cpu().numpy()


def launched(sol, family, waves, tag):
    assert sol.get_option("last_kernel_family") == family and sol.get_option("last_kernel_waves") == waves, \
        (tag, sol.get_option("last_kernel_family"), sol.get_option("last_kernel_waves"))
    if family in cases.CLUSTERED:
        assert sol.get_option("cluster_fixups") == 0, tag


def check(tag, S, P, g, lam0, lam1, lam2, N, n, pc, u):
    """first_steps_quantities of every trajectory; S, P: the host's matrices (cases.host_matrices, cases.applied)."""
    worst = {"lam1": 0.0, "lam2": 0.0}
    for b in range(lam0.shape[0]):
        assert np.isfinite(lam1[b]).all() and np.isfinite(lam2[b]).all(), (tag, b, "a never-read slot was read")
        q = first_steps_quantities(S[b], P[b], g[b], lam0[b], lam1[b], lam2[b], N, n, pc, u)
        worst = {k: max(worst[k], q[k]) for k in worst}
        for key, v in q.items():
            assert v <= FIRST_STEPS_LIMIT, (tag, b, key, v, FIRST_STEPS_LIMIT)
    print(f"{tag}: " + " ".join(f"{k} {v:.2g}" for k, v in worst.items()))


def first_steps_of_a_row(r, B):
    if r.prec == "f64" and np.finfo(np.longdouble).eps > 2.0 ** -60:
        pytest.skip("no extended-precision long double on this host")
    S, P, g, lam0 = (a[:B] for a in cases.device_matrices(r))
    sol = solver(r, B)
    entry, u = ("solve", EPS32) if r.prec == "f32" else ("solve_f64", U64)
    dS, dP, dg, dlam0 = dev(S), dev(P), dev(g), dev(lam0)
    tag = cases.row_id(r)
    lam = {}
    for K in (1, 2):
        lam[K] = solve(sol, entry, dS, dP, dg, dlam0, K, r.pc)
        launched(sol, r.family, r.waves, tag)
    HP[0] = np.float64 if r.prec == "f32" else np.longdouble
    try:
        Sh, Ph = cases.host_matrices(r)[:2]
        check(tag, Sh, Ph, g, lam0, lam[1], lam[2], r.N, r.n, r.pc, u)
    finally:
        HP[0] = np.float64
    return sol, (dS, dP, dg, dlam0), lam


@pytest.mark.parametrize("r", ROWS14, ids=cases.row_id)
def test_first_two_iterations_of_the_batched_entries(r):
    """Every n = 14 row under its own preconditioner BUILD, five different systems per launch."""
    first_steps_of_a_row(r, cases.B)


@pytest.mark.parametrize("r", ROWS_GENERIC, ids=cases.row_id)
def test_first_two_iterations_of_the_generic_kernel(r):
    """State sizes other than 14, float and double, both preconditioners, three systems per launch."""
    first_steps_of_a_row(r, 3)


@pytest.mark.parametrize("r", TILED, ids=cases.row_id)
def test_workgroups_that_are_not_the_first_return_the_bits_of_their_originals(r):
    """2 x num_cus + 3 trajectories tiled from the row's five: more workgroups than CUs, so workgroups share a CU and most are not the first of
    the launch.  The five originals are checked by the model, every copy must carry the bits of its original."""
    sol5, (dS, dP, dg, dlam0), lam = first_steps_of_a_row(r, cases.B)
    total = 2 * sol5.get_option("num_cus") + 3
    reps = -(-total // cases.B)
    tile = lambda t: t.repeat(reps, 1)[:total].contiguous()
    sol = solver(r, total)
    tS, tP, tg, tlam0 = tile(dS), tile(dP), tile(dg), tile(dlam0)
    for K in (1, 2):
        out = solve(sol, "solve", tS, tP, tg, tlam0, K, r.pc)
        launched(sol, r.family, r.waves, cases.row_id(r))
        for b in range(total):
            assert out[b].tobytes() == lam[K][b % cases.B].tobytes(), (cases.row_id(r), K, b)


@pytest.mark.parametrize("pc", ["ss", "jacobi"])
@pytest.mark.parametrize("N,opts,family,waves", cases.F16_CASES, ids=[f"N{c[0]}-family{c[2]}" for c in cases.F16_CASES])
def test_first_two_iterations_with_fp16_storage(N, opts, family, waves, pc):
    """The arithmetic is float on matrices rounded to half precision once: predicted from the rounded matrices (S16.float(), as
    tests/test_gpu_f16.py), u = 2^-24."""
    S, P, g, lam0 = cases.f16_system(N, pc)
    r = cases.Row("f32", 14, 7, N, pc, family, opts, waves)
    sol = solver(r, cases.B)
    S16, P16 = sol.to_f16(dev(S)), sol.to_f16(dev(P))
    dg, dlam0 = dev(g), dev(lam0)
    tag = f"fp16 storage N={N} {pc} family {family}"
    lam = {}
    for K in (1, 2):
        lam[K] = solve(sol, "solve_f16", S16, P16, dg, dlam0, K, pc)
        launched(sol, family, waves, tag)
    Sh, Ph = (np.stack([cases.applied(M[b], 14, N, cases.reads_lower(r)) for b in range(cases.B)]) for M in (S16.float().cpu().numpy(), P16.float().cpu().numpy()))
    check(tag, Sh, Ph, g, lam0, lam[1], lam[2], N, 14, pc, EPS32)
