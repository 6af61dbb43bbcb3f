"""The two one-step checkers of the PCG kernels, host side only (numpy; no GPU, no oracle).  Both evaluate textbook preconditioned CG on the
bd layout in a precision above the kernel's (float64 for the float kernels, the x87 80-bit long double for the double kernels: the HP switch)
and divide every checked quantity by the size its first-order rounding model gives it, in units of u (2^-24, 2^-53).

  step_quantities        for entries that return lambda, r and p (the 12-argument entries): one step of the recurrences between the states of a
                         run capped at K - 1 and of one capped at K, the scalars the kernel used, the residual gap, local conjugacy and
                         orthogonality.  The vector updates are scaled by the LARGEST term of the vector.
  first_steps_quantities for entries that return only lambda (the batched entries): lambda after one and after two iterations predicted from
                         the inputs alone, the difference divided ELEMENTWISE by the size of the terms at that element — a wrong value at a
                         knot whose entries are 100 x smaller than the vector's largest shows as it would at the largest.

Cases: tests/pcg_step_cases.py; the limits are pinned on the CPU by tests/test_pcg_step_model_cpu.py."""
import numpy as np

EPS32 = 2.0 ** -24

HP = [np.float64]          # the host's evaluation precision: float64 for the float kernels, the x87 80-bit long double for the double kernels


def bt_matvec(M, x, N, n=14, cols=3):
    """Block-tridiagonal product from the bd layout in HP[0] precision (numpy): y_k = M[k,0] x_{k-1} + M[k,1] x_k + M[k,2] x_{k+1}, blocks column-major
    (cols = 1: the diagonal blocks only)."""
    B = np.nan_to_num(np.asarray(M, HP[0])).reshape(N, 3, n, n).transpose(0, 1, 3, 2)       # [k][col] as row-major matrices
    X = np.asarray(x, HP[0]).reshape(N, n)
    y = np.einsum("kij,kj->ki", B[:, 1], X)
    if cols == 3:
        y[1:] += np.einsum("kij,kj->ki", B[1:, 0], X[:-1])
        y[:-1] += np.einsum("kij,kj->ki", B[:-1, 2], X[1:])
    return y.reshape(-1)


def abs_matvec(M, x, N, n=14, cols=3):
    """|M| |x|: the size of the terms a float32 evaluation of M x rounds (cancellation inside the three-block sums shows here, not in |M x|)."""
    return bt_matvec(np.abs(np.nan_to_num(M)), np.abs(x), N, n, cols)


def step_quantities(S, P, g, lam0, st_a, st_b, N, K, EPS32=EPS32, n=14):
    """Every checked quantity DIVIDED BY the scale its float32 rounding model gives it (u = 2^-24): a correct kernel lands at O(1..30)
    whatever N, K, the preconditioner or the conditioning; tools/_prof/inv_probe.py prints them for 96 (system, K) pairs."""
    (lam_a, r_a, p_a), (lam_b, r_b, p_b) = st_a, st_b
    inf = lambda x: np.abs(x).max()
    Sp, z_a, z_b = bt_matvec(S, p_a, N, n), bt_matvec(P, r_a, N, n), bt_matvec(P, r_b, N, n)
    eta_a, eta_b, v = r_a @ z_a, r_b @ z_b, p_a @ Sp
    assert eta_a < 0 and eta_b < 0 and v < 0             # S and Pinv are stored negated (include/pcg/linsys_setup.cuh:15-19): eta = r' Pinv r < 0
    alpha, beta = eta_a / v, eta_b / eta_a
    # what the kernel itself used, recovered from its own updates (least squares along p_{K-1})
    alpha_hat = ((lam_b - lam_a) @ p_a) / (p_a @ p_a)
    beta_hat = ((p_b - z_b) @ p_a) / (p_a @ p_a)
    # cancellation of the three inner products: sum |terms| / |sum|
    c_eta_a = (np.abs(r_a) @ abs_matvec(P, r_a, N, n)) / abs(eta_a)
    c_eta_b = (np.abs(r_b) @ abs_matvec(P, r_b, N, n)) / abs(eta_b)
    c_v = (np.abs(p_a) @ abs_matvec(S, p_a, N, n)) / abs(v)
    q = {
        # the update directions, with the kernel's own scalars: pure axpy / matvec rounding
        "lam": inf(lam_b - (lam_a + alpha_hat * p_a)) / (EPS32 * (inf(lam_b) + abs(alpha_hat) * inf(p_a))),
        "r": inf(r_b - (r_a - alpha_hat * Sp)) / (EPS32 * (inf(r_a) + abs(alpha_hat) * inf(abs_matvec(S, p_a, N, n)))),
        "p": inf(p_b - (z_b + beta_hat * p_a)) / (EPS32 * (inf(abs_matvec(P, r_b, N, n)) + abs(beta_hat) * inf(p_a))),
        # the scalars: float32 inner products of ~14 N terms against their float64 values, scaled by the cancellation of the sums
        "alpha": abs(alpha_hat / alpha - 1) / (EPS32 * (c_eta_a + c_v)),
        "beta": abs(beta_hat / beta - 1) / (EPS32 * (c_eta_a + c_eta_b)),
    }
    Snorm = float(np.abs(np.nan_to_num(S).astype(np.float64).reshape(N, 3, n, n)).sum(axis=(1, 2)).max())      # ||S||_inf (a block row's three blocks, summed along rows)
    true_r = g.astype(HP[0]) - bt_matvec(S, lam_b, N, n)
    nrm = lambda x: float(np.sqrt(float(x @ x)))
    q["gap"] = nrm(r_b - true_r) / (K * EPS32 * Snorm * max(nrm(lam_b), nrm(np.asarray(lam0, HP[0]))))
    q["conjugacy"] = abs(p_b @ Sp) / np.sqrt((p_b @ bt_matvec(S, p_b, N, n)) * v)
    q["orthogonality"] = abs(r_b @ z_a) / np.sqrt(eta_a * eta_b)
    return {k_: float(v_) for k_, v_ in q.items()}


# Worst over 96 (system, K) pairs on an MI355X (tools/_prof/inv_probe.py -> profiles/r05_invariants.txt): lam 0.89 u, r 1.67 u, p 0.95 u of their update's
# terms; alpha 0.57, beta 1.26 u x the cancellation of their inner products; gap 0.30 of K u ||S|| ||lambda||; conjugacy 1.7e-4, orthogonality 3.4e-4.
# The limits leave a factor 4-6: an error of a few float32 ulps in ONE update of ONE iteration fails.
LIMITS = {"lam": 4.0, "r": 8.0, "p": 8.0, "alpha": 8.0, "beta": 8.0, "gap": 2.0, "conjugacy": 2e-3, "orthogonality": 2e-3}


def initial_state(S, P, g, lam0, N, n, pc):
    """The K = 0 state in HP[0] precision, with the size of the terms each element rounds: (r0, size of r0's terms, p0, size of p0's terms);
    r0 = gamma - S lambda0, p0 = Pinv r0 ("jacobi": the diagonal blocks only)."""
    cols = 3 if pc == "ss" else 1
    g, lam0 = np.asarray(g, HP[0]), np.asarray(lam0, HP[0])
    r0 = g - bt_matvec(S, lam0, N, n)
    e_r0 = np.abs(g) + abs_matvec(S, lam0, N, n)
    p0 = bt_matvec(P, r0, N, n, cols)
    e_p0 = abs_matvec(P, e_r0, N, n, cols)
    return r0, e_r0, p0, e_p0


def _worst(diff, scale, u):
    """max over the elements of |diff| / (u scale); an element without terms (scale 0) must agree exactly."""
    diff, scale = np.abs(diff), np.asarray(scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(scale > 0, diff / (u * scale), np.where(diff > 0, np.inf, 0.0))
    return float(q.max())


# Limit of both keys of first_steps_quantities, in units of u x the size of the element's terms.  Measured worst of the float32 oracle over every row
# of tests/pcg_step_cases.py: see FIRST_STEPS_ORACLE_WORST and profiles/pcg_step_model.txt; the limit is 6 x that, rounded up to one digit — the
# margin LIMITS has over its measured worst, for the device's other summation orders.  Double: the same number at u = 2^-53.
# (The fp16-storage systems are no rows of the table; the float32 oracle on their rounded matrices reaches 3.6 / 0.95, inside the same limit.)
FIRST_STEPS_ORACLE_WORST = {"lam1": 2.97, "lam2": 0.76}       # (float32; the float64 oracle in long double: 2.58, 0.75)
FIRST_STEPS_LIMIT = 20.0                                        # 6 x 2.97 = 17.8


def first_steps_quantities(S, P, g, lam0, lam1, lam2, N, n, pc, u):
    """For entries that return only lambda.  lam1 / lam2: the entry's lambda after max_iter = 1 / 2 from lam0 (exit_tol = 0).  From the inputs
    alone, in HP[0] precision: r0, p0 = Pinv r0, alpha0, the predicted lambda1; r1, beta1, p1, alpha1, the predicted lambda2 ("jacobi": the
    diagonal blocks of Pinv only).  Returns {"lam1", "lam2"}: the largest ELEMENTWISE |lambda_K - prediction| / (u x the size of the terms at
    that element), the size of the terms a first-order rounding model:
      lambda1   |lambda1| + |alpha0| E(p0) + |alpha0| |p0| (c_eta0 + c_v0)
                E(r0) = |gamma| + |S| |lambda0|, E(p0) = |Pinv| E(r0); c_eta, c_v: sum |terms| / |sum| of the inner products r' Pinv r, p' S p
      lambda2   |lambda2| + E(lambda1) + |alpha1| E(p1) + |alpha1| |p1| (c_eta1 + c_v1), with the same model one step on:
                E(r1) = E(r0) + |alpha0| |S| (E(p0) + |p0|) + |alpha0| |S p0| (c_eta0 + c_v0),
                E(p1) = |Pinv| (E(r1) + |r1|) + |beta1| E(p0) + |beta1| |p0| (c_eta0 + c_eta1) + |p1|."""
    cols = 3 if pc == "ss" else 1
    A = np.abs
    lam0h = np.asarray(lam0, HP[0])
    r0, e_r0, p0, e_p0 = initial_state(S, P, g, lam0, N, n, pc)
    Sp0 = bt_matvec(S, p0, N, n)
    eta0, v0 = r0 @ p0, p0 @ Sp0
    assert eta0 < 0 and v0 < 0                         # (S and Pinv are stored negated)
    alpha0 = eta0 / v0
    c_eta0 = (A(r0) @ abs_matvec(P, r0, N, n, cols)) / abs(eta0)
    c_v0 = (A(p0) @ abs_matvec(S, p0, N, n)) / abs(v0)
    pred1 = lam0h + alpha0 * p0
    e_lam1 = A(pred1) + abs(alpha0) * e_p0 + abs(alpha0) * A(p0) * (c_eta0 + c_v0)
    r1 = r0 - alpha0 * Sp0
    z1 = bt_matvec(P, r1, N, n, cols)
    eta1 = r1 @ z1
    assert eta1 < 0
    beta1 = eta1 / eta0
    p1 = z1 + beta1 * p0
    Sp1 = bt_matvec(S, p1, N, n)
    v1 = p1 @ Sp1
    assert v1 < 0
    alpha1 = eta1 / v1
    c_eta1 = (A(r1) @ abs_matvec(P, r1, N, n, cols)) / abs(eta1)
    c_v1 = (A(p1) @ abs_matvec(S, p1, N, n)) / abs(v1)
    pred2 = pred1 + alpha1 * p1
    e_r1 = e_r0 + abs(alpha0) * abs_matvec(S, e_p0 + A(p0), N, n) + abs(alpha0) * A(Sp0) * (c_eta0 + c_v0)
    e_p1 = abs_matvec(P, e_r1 + A(r1), N, n, cols) + abs(beta1) * e_p0 + abs(beta1) * A(p0) * (c_eta0 + c_eta1) + A(p1)
    e_lam2 = A(pred2) + e_lam1 + abs(alpha1) * e_p1 + abs(alpha1) * A(p1) * (c_eta1 + c_v1)
    return {"lam1": _worst(np.asarray(lam1, HP[0]) - pred1, e_lam1, u), "lam2": _worst(np.asarray(lam2, HP[0]) - pred2, e_lam2, u)}


def initial_state_quantities(S, P, g, lam0, r, p, N, n, pc, u):
    """The K = 0 state an entry returns (d_r = gamma - S lambda0, d_p = Pinv d_r) against its HP[0] evaluation, in the "r" and "p" scalings of
    step_quantities: the largest difference over u x the largest term of the vector."""
    inf = lambda x: np.abs(x).max()
    cols = 3 if pc == "ss" else 1
    r0, e_r0, _, _ = initial_state(S, P, g, lam0, N, n, pc)
    r, p = np.asarray(r, HP[0]), np.asarray(p, HP[0])
    return {"r": float(inf(r - r0) / (u * inf(e_r0))),
            "p": float(inf(p - bt_matvec(P, r, N, n, cols)) / (u * inf(abs_matvec(P, r, N, n, cols))))}
