"""GPU: the PCG recurrences checked on the kernel's OWN outputs, in float64 on the host — no oracle, no same-author restatement on the
comparison side (VERDICT r04 #2b).  The 12-argument entry (include/pcg/sqp.cuh:137-150) returns lambda, d_r and d_p of the last completed
update; the kernels are deterministic, so a run capped at K - 1 iterations IS the state the K-iteration run passed through.  From the two
states, with S / Pinv / gamma promoted to float64 and nothing but textbook preconditioned CG (what pcg<> computes):

  step      lambda_K = lambda_{K-1} + alpha p_{K-1};   r_K = r_{K-1} - alpha S p_{K-1};   p_K = Pinv r_K + beta p_{K-1}, with the alpha / beta the kernel
            itself used (recovered from its updates), each within a few float32 ulps (u = 2^-24) of the SIZE OF ITS TERMS (|S||p|, |Pinv||r|:
            cancellation inside the three-block sums is accounted for, so the limits are O(1) x u whatever N, K or the conditioning);
  scalars   that alpha = (r' Pinv r) / (p' S p) and beta = (r_K' Pinv r_K) / (r_{K-1}' Pinv r_{K-1}) of the float64 evaluation, within a
            few u x the cancellation of the inner products
            — ONE iteration of float32 arithmetic against its float64 evaluation: rounding has not been amplified by CG, so an error of a few
            ulps in one update fails (the K-iterate comparisons of test_gpu_parity.py, with max(1e-3, 4 x band), would pass a 1e-4 slip);
  gap       || d_r - (gamma - S lambda_K) || <= 2 K u ||S||_inf max ||lambda|| (the classical bound on the drift of the updated residual);
  conjugacy | p_K' S p_{K-1} | / sqrt((p_K' S p_K)(p_{K-1}' S p_{K-1})) <= 2e-3 (local conjugacy survives finite precision);
  orthogonality  | r_K' Pinv r_{K-1} | / sqrt(eta_K eta_{K-1}) <= 2e-3.

K = 10, 50, 167 for N = 32 (row-per-lane kernel), 128 (lane-pair kernel), 512 (clustered kernel); symmetric-stair and block-Jacobi Pinv.
The "jacobi" parameter is block-Jacobi DATA (zeros in the off-diagonal blocks of Pinv) through the symmetric-stair builds: the 12-argument
entries always apply three columns of Pinv.  The block-Jacobi builds proper are reached only by the batched entries: tests/test_gpu_first_steps.py.

test_one_step_at_ragged_horizons and its double twin run the same checks over tests/pcg_step_cases.py: horizons that are no multiple of a
kernel's knots per wavefront or workgroup, every family and workgroup width the launch plan has, state sizes other than 14, K from 1 upwards
(K by the rule of that module), and the K = 0 state — max_iter = 0 returns 0 iterations, exit flag 1, lambda0 bit for bit, d_r = gamma - S lambda0
and d_p = Pinv d_r, each compared directly with its float64 evaluation in the "r" / "p" scalings.  The checkers themselves:
tests/pcg_step_model.py, pinned without a GPU by tests/test_pcg_step_model_cpu.py."""
import numpy as np
import pytest
import torch

import pcg_step_cases as cases
from mpcgpu_amd import synth
from pcg_step_model import EPS32, HP, LIMITS, initial_state_quantities, step_quantities

pytestmark = pytest.mark.gpu
n = 14


def state(sol, dS, dP, dg, lam0, K):
    N, n = sol.N, sol.n
    dt = dS.dtype                                          # float32, or float64 = linsys_t double (the same checks at u = 2^-53)
    d_lam = torch.from_numpy(lam0.copy()).cuda()
    d_r = torch.full((n * N,), float("nan"), device="cuda", dtype=dt)
    d_p = torch.full((n * N,), float("nan"), device="cuda", dtype=dt)
    scratch = torch.zeros(N, device="cuda", dtype=dt)
    d_it = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_ex = torch.zeros(1, dtype=torch.bool, device="cuda")
    (sol.solve_ref if dt == torch.float32 else sol.solve_ref_f64)(dS, dP, dg, d_lam, d_r, d_p, scratch, scratch, d_it, d_ex, K, 0.0)
    torch.cuda.synchronize()
    assert int(d_it.item()) == K and bool(d_ex.item()) is True
    out = [t.cpu().numpy().astype(HP[0]) for t in (d_lam, d_r, d_p)]
    assert all(np.isfinite(v).all() for v in out)
    return out


@pytest.mark.parametrize("N,family", [(32, 5), (64, 11), (128, 11), (128, 6), (512, 7)])
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
def test_one_step_of_the_recurrences_and_the_cg_invariants(N, family, pc):
    from mpcgpu_amd import PcgSolver
    k = synth.make_kkt(N, 1, 9000 + N)
    S, P, g = synth.form_schur(k, precond=pc)                # (block-Jacobi: the off-diagonal blocks of Pinv are zeros; the entry applies three columns)
    S, P, g = S[0], P[0], g[0]
    rng = np.random.default_rng(N)
    lam0 = (0.1 * rng.standard_normal(n * N)).astype(np.float32)
    sol = PcgSolver(N, max_batch=1)
    if family in (6, 11):                                      # (the lane-pair / the lane-quad kernel, pinned: the policy picks by horizon and preconditioner)
        sol.set_option("pcg_lpk", 1); sol.set_option("pcg_lqb", int(family == 11))
    dS, dP, dg = (torch.from_numpy(a).cuda() for a in (S, P, g))
    for K in (10, 50, 167):
        st_a = state(sol, dS, dP, dg, lam0, K - 1)
        assert sol.get_option("last_kernel_family") == family
        st_b = state(sol, dS, dP, dg, lam0, K)
        q = step_quantities(S, P, g, lam0, st_a, st_b, N, K)
        print(f"N={N} {pc} K={K}: " + " ".join(f"{a} {b:.2g}" for a, b in q.items()))
        for key, lim in LIMITS.items():
            assert q[key] <= lim, (N, pc, K, key, q[key], lim)


@pytest.mark.parametrize("N,family", [(32, 5), (64, 9), (64, 8), (128, 10), (128, 8)])
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
def test_the_same_invariants_in_double(N, family, pc):
    """linsys_t = double: the row-per-lane kernel (N = 32), the lane-quad kernel (N = 64) and the clustered row-per-lane kernel across 2 / 4 CUs
    (N = 64 / 128) against the same
    recurrences at u = 2^-53, the host side evaluated in the x87 80-bit long double (u = 2^-64; numpy's longdouble on x86-64) so that it is
    again the more precise side; same limits as the float test."""
    from mpcgpu_amd import PcgSolver
    k = synth.make_kkt(N, 1, 9100 + N)
    S, P, g = synth.form_schur(k, precond=pc, dtype=np.float64)
    S, P, g = S[0], P[0], g[0]
    rng = np.random.default_rng(N)
    lam0 = 0.1 * rng.standard_normal(n * N)
    sol = PcgSolver(N, max_batch=1)
    if family == 8:
        sol.set_option("pcg_lqk", 0)                      # (the clustered row-per-lane kernel instead of the lane-quad kernel)
    dS, dP, dg = (torch.from_numpy(a).cuda() for a in (S, P, g))
    U64 = 2.0 ** -53
    if np.finfo(np.longdouble).eps > 2.0 ** -60:
        pytest.skip("no extended-precision long double on this host")
    HP[0] = np.longdouble
    try:
        _double_invariants(sol, dS, dP, dg, S, P, g, lam0, N, family, pc, U64)
    finally:
        HP[0] = np.float64


def _double_invariants(sol, dS, dP, dg, S, P, g, lam0, N, family, pc, U64):
    for K in (10, 50, 167):
        st_a = state(sol, dS, dP, dg, lam0, K - 1)
        assert sol.get_option("last_kernel_family") == family and sol.get_option("cluster_fixups") == 0
        st_b = state(sol, dS, dP, dg, lam0, K)
        q = step_quantities(S, P, g, lam0, st_a, st_b, N, K, EPS32=U64)
        print(f"double N={N} {pc} K={K}: " + " ".join(f"{a} {b:.2g}" for a, b in q.items()))
        for key, lim in LIMITS.items():
            scale = 1.0 if key in ("lam", "r", "p", "alpha", "beta", "gap") else 2.0 ** -29      # (conjugacy / orthogonality scale with u: float32's limit x 2^-29)
            assert q[key] <= lim * scale, (N, pc, K, key, q[key], lim * scale)


def ragged_one_step(r, u):
    """One row of tests/pcg_step_cases.py through the 12-argument entry (trajectory 0): the launch, the K = 0 state, then one step at every K."""
    from mpcgpu_amd import PcgSolver
    S, P, g, lam0 = (np.array(a[0]) for a in cases.three_column_matrices(r))
    Sh, Ph = (a[0] for a in cases.host_matrices(r)[:2])   # (the host side: the never-read slots as zeros, the matrices as the row's kernel applies them)
    sol = PcgSolver(r.N, max_batch=1, state_size=r.n)
    for key, value in r.opts:
        sol.set_option(key, value)
    dS, dP, dg = (torch.from_numpy(a).cuda() for a in (S, P, g))
    scale = lambda key: 1.0 if u == EPS32 or key not in ("conjugacy", "orthogonality") else 2.0 ** -29      # (as the double test above)
    tag = cases.row_id(r)

    def launched():
        assert sol.get_option("last_kernel_family") == r.family and sol.get_option("last_kernel_waves") == r.waves, \
            (tag, sol.get_option("last_kernel_family"), sol.get_option("last_kernel_waves"))
        if r.family in cases.CLUSTERED:
            assert sol.get_option("cluster_fixups") == 0, tag

    st = {0: state(sol, dS, dP, dg, lam0, 0)}             # (state() asserts iters = K and the exit flag)
    launched()
    same = np.array_equal(st[0][0], lam0.astype(HP[0])) and np.array_equal(np.signbit(st[0][0]), np.signbit(lam0))     # (the widening is exact)
    assert same, (tag, "max_iter = 0 must hand lambda0 back bit for bit")
    q0 = initial_state_quantities(Sh, Ph, g, lam0, st[0][1], st[0][2], r.N, r.n, "ss", u)
    print(f"{tag} K=0: " + " ".join(f"{a} {b:.2g}" for a, b in q0.items()))
    for key, v in q0.items():
        assert v <= LIMITS[key], (tag, "K = 0", key, v, LIMITS[key])
    for K in cases.ks(r, 0)[1]:
        for k_ in (K - 1, K):
            if k_ not in st:
                st[k_] = state(sol, dS, dP, dg, lam0, k_)
                launched()
        q = step_quantities(Sh, Ph, g, lam0, st[K - 1], st[K], r.N, K, EPS32=u, n=r.n)
        print(f"{tag} K={K}: " + " ".join(f"{a} {b:.2g}" for a, b in q.items()))
        for key, lim in LIMITS.items():
            assert q[key] <= lim * scale(key), (tag, K, key, q[key], lim * scale(key))


@pytest.mark.parametrize("r", cases.ROWS32, ids=cases.row_id)
def test_one_step_at_ragged_horizons(r):
    """Float rows.  Worst values per family on an MI355X: profiles/pcg_step_model.txt."""
    ragged_one_step(r, EPS32)


@pytest.mark.parametrize("r", cases.ROWS64, ids=cases.row_id)
def test_one_step_at_ragged_horizons_in_double(r):
    """Double rows, u = 2^-53, the host in long double; conjugacy and orthogonality at float32's limit x 2^-29 as above."""
    if np.finfo(np.longdouble).eps > 2.0 ** -60:
        pytest.skip("no extended-precision long double on this host")
    HP[0] = np.longdouble
    try:
        ragged_one_step(r, 2.0 ** -53)
    finally:
        HP[0] = np.float64
