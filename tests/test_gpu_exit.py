"""GPU: the tolerance exit |eta'| < exit_tol of every PCG kernel family — the path every caller leaves the loop through — checked EXACTLY.
Cases, predictions and assertions: tests/pcg_exit_cases.py (pinned without a GPU by tests/test_pcg_exit_cases_cpu.py, where six planted
defects of the exit path fail these very assertions).

Batched entries (mpcg_pcg_solve, _f16, _f64), one test per row and both ladders: under (cap_hi, exit_tol) and (cap_mid, exit_tol) every
trajectory's iteration count and exit flag equal the prediction; its lambda carries the BITS of the launch with max_iter = that count and
exit_tol = 0 on the same handle (the fixed-count path of tests/test_gpu_first_steps.py and tests/test_gpu_invariants.py: one update too many
or too few shows with no tolerance at all), a count of 0 the bits of lambda0; everything twice on one handle, the same counts and bits.

Tiled: the cold ladder repeated to 2 x num_cus + 3 trajectories, one case per family — workgroups that take their next trajectory after one
that left at the setup step; every copy returns its original's count, flag and bits.

12-argument entries (mpcg_pcg_solve_ref, _ref_f64), one trajectory at a time from the warm ladder — the 0 exit, the deepest tolerance exit, the
trajectory that never crosses under cap_mid: d_pcg_iters and d_pcg_exit exact, d_lambda, d_r and d_p against the float64 oracle's state at that
exit (p left as it is on a tolerance exit, updated on a cap exit: the kernels' p_pending), d_r and d_p prefilled with 7."""
import numpy as np
import pytest
import torch

import pcg_exit_cases as ec
import pcg_step_cases as sc

pytestmark = pytest.mark.gpu

ENTRY = {"f32": "solve", "f64": "solve_f64", "f16": "solve_f16"}
deep_enough = [r for r in ec.ROWS if not ec.too_fast(r)]
TILED = [min((r for r in deep_enough if (r.prec, r.family) == pf), key=lambda r: r.N) for pf in sorted({(r.prec, r.family) for r in ec.ROWS})]


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()              # (a copy: the shared cases are read-only)


def solver(r, max_batch):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(r.N, max_batch=max_batch, state_size=r.n)
    for key, value in r.opts:
        sol.set_option(key, value)
    if sc.reads_lower(r):                                  # the caller vouches for block symmetry: no guard launch next to the kernel under test
        sol.set_option("assume_symmetric", 1)
    return sol


def launched(sol, r, tag):
    assert sol.get_option("last_kernel_family") == r.family and sol.get_option("last_kernel_waves") == r.waves, \
        (tag, sol.get_option("last_kernel_family"), sol.get_option("last_kernel_waves"))
    if r.family in sc.CLUSTERED:
        assert sol.get_option("cluster_fixups") == 0, tag


def launch(sol, r, dS, dP, dg, dlam0, cap, tol):
    """One call of the row's batched entry from lambda0 (device, not touched): (lambda, iters, flags) on the host."""
    from mpcgpu_amd import pcg_config
    lam = dlam0.clone()
    it, ex = getattr(sol, ENTRY[r.prec])(dS, dP, dg, lam, pcg_config(pcg_exit_tol=tol, pcg_max_iter=cap), r.pc)
    torch.cuda.synchronize()
    return lam.cpu().numpy(), it.cpu().numpy().astype(np.int64), ex.cpu().numpy().astype(np.int64)


def tiled_matrices(r, total):
    S, P = ec.base(r)[:2]
    return tuple(dev(M)[None].expand(total, -1).contiguous() for M in (S, P))


def ladder_on_the_gpu(sol, r, lad, tag, dS, dP):
    """Every launch of one ladder; returns what it read back, for the comparison of the second pass with the first."""
    dg, dlam0 = dev(lad.gamma), dev(lad.lam0)
    seen, fixed = [], {}
    for k in ec.distinct_counts(lad):
        lam, it, ex = launch(sol, r, dS, dP, dg, dlam0, k, 0.0)
        launched(sol, r, tag)
        assert (it == k).all() and (ex == 1).all(), (tag, "max_iter", k, it, ex)
        fixed[k] = lam
        seen.append(lam)
    for cap in (lad.cap_hi, lad.cap_mid):
        lam, it, ex = launch(sol, r, dS, dP, dg, dlam0, cap, lad.tol)
        launched(sol, r, tag)
        ec.check_counts(tag, lad, cap, it, ex)
        ec.check_lambda_bits(tag, lad, cap, lam, fixed)
        seen += [lam, it, ex]
    return seen


@pytest.mark.parametrize("r", ec.ALL_ROWS, ids=lambda r: f"{ec.row_id(r)}-{r.prec}")
def test_exact_counts_flags_and_lambda_bits_of_the_batched_entries(r):
    tag = ec.row_id(r)
    ladders = [ec.ladder(r, warm) for warm in (False, True)]
    B = max(len(lad.pred) for lad in ladders)
    sol = solver(r, B)
    passes = []
    for _ in range(2):
        seen = []
        for lad, name in zip(ladders, ("cold", "warm")):
            dS, dP = tiled_matrices(r, len(lad.pred))
            seen += ladder_on_the_gpu(sol, r, lad, f"{tag} {name}", dS, dP)
        passes.append(seen)
    for a, b in zip(*passes):
        assert a.tobytes() == b.tobytes(), (tag, "the second pass on the same handle differs from the first")
    print(f"{tag}: " + "; ".join(f"exit_tol {lad.tol:.3g} counts {lad.pred[:-1]} caps {lad.cap_mid}, {lad.cap_hi}" for lad in ladders))


@pytest.mark.parametrize("r", TILED, ids=lambda r: f"{ec.row_id(r)}-{r.prec}")
def test_copies_across_more_workgroups_than_cus_return_their_originals(r):
    tag = ec.row_id(r)
    lad = ec.ladder(r, False)
    B = len(lad.pred)
    sol = solver(r, B)
    total = 2 * sol.get_option("num_cus") + 3
    reps = -(-total // B)
    tile = lambda t: t.repeat(reps, 1)[:total].contiguous()
    dg, dlam0 = dev(lad.gamma), dev(lad.lam0)
    big = solver(r, total)
    tS, tP = tiled_matrices(r, total)
    for cap in (lad.cap_hi, lad.cap_mid):
        lam, it, ex = launch(sol, r, *tiled_matrices(r, B), dg, dlam0, cap, lad.tol)
        ec.check_counts(tag, lad, cap, it, ex)
        tlam, tit, tex = launch(big, r, tS, tP, tile(dg), tile(dlam0), cap, lad.tol)
        launched(big, r, tag)
        for b in range(total):
            assert (tit[b], tex[b]) == (it[b % B], ex[b % B]) and tlam[b].tobytes() == lam[b % B].tobytes(), (tag, cap, b, tit[b], tex[b], it[b % B], ex[b % B])


def state_of_a_twelve_argument_call(sol, dS, dP, g, lam0, cap, tol):
    N, n, dt = sol.N, sol.n, dS.dtype
    d_lam = dev(lam0)
    d_r = torch.full((n * N,), 7.0, device="cuda", dtype=dt)
    d_p = torch.full((n * N,), 7.0, device="cuda", dtype=dt)
    scratch = torch.zeros(N, device="cuda", dtype=dt)
    d_it = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    d_ex = torch.zeros(1, dtype=torch.bool, device="cuda")
    (sol.solve_ref if dt == torch.float32 else sol.solve_ref_f64)(dS, dP, dev(g), d_lam, d_r, d_p, scratch, scratch, d_it, d_ex, cap, tol)
    torch.cuda.synchronize()
    return int(d_it.item()), int(bool(d_ex.item())), d_lam.cpu().numpy(), d_r.cpu().numpy(), d_p.cpu().numpy()


@pytest.mark.parametrize("r", ec.ROWS, ids=ec.row_id)
def test_iters_flag_lambda_r_and_p_of_the_twelve_argument_entries(r):
    """Measured on an MI355X, worst error / tolerance over the rows: 0.17 in float, 0.35 in double (tolerances 3.7e-14 ... 1.9e-12 over bands of
    3.4e-16 ... 3.3e-14, pcg_exit_cases.band64).  Before the clustered lane-pair and lane-quad kernels stored r at a setup exit, their rows
    failed here with an error of 0.8 in d_r (d_r = gamma)."""
    from mpcgpu_amd import PcgSolver
    tag = ec.row_id(r)
    lad = ec.ladder(r, True)
    sol = PcgSolver(r.N, max_batch=1, state_size=r.n)
    for key, value in r.opts:
        sol.set_option(key, value)
    dS, dP = (dev(M) for M in ec.three_column(r))
    worst = 0.0
    for b, cap in ec.state_trajectories(lad):
        ref, tols = ec.state_reference(r, lad, b, cap)
        it, ex, lam, res, p = state_of_a_twelve_argument_call(sol, dS, dP, lad.gamma[b], lad.lam0[b], cap, lad.tol)
        launched(sol, r, tag)
        assert (it, ex) == (ref["iters"], int(ref["max_iter_exit"])), (tag, lad.kinds[b], cap, it, ex, ref["iters"], ref["max_iter_exit"])
        if it == 0:
            assert lam.tobytes() == lad.lam0[b].tobytes(), (tag, "a zero-iteration exit must leave lambda0 as it is")
        worst = max(worst, ec.check_state(f"{tag} {lad.kinds[b]} count {it} cap {cap}", ref, tols, lam, res, p))
    print(f"{tag}: worst error / tolerance {worst:.3g}; tolerances " + " ".join(f"{k} {v[0]:.2g} (band {v[1]:.2g})" for k, v in tols.items()))
