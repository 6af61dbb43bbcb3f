"""The numpy restatement of the backward Riccati sweep of include/mpcg_riccati.h, generic in dtype (float64 and np.longdouble), on the packed
arrays the library reads (G_dense, C_dense of ONE trajectory), and the cases the GPU tests of mpcg_riccati_gains(_f64) use.  No GPU here.

    P_{N-1} = Q_{N-1} + rho I
    k = N-2 .. 0:   H_uu = R_k + rho I + B_k^T P_{k+1} B_k,   H_ux = B_k^T P_{k+1} A_k,   K_k = -H_uu^-1 H_ux,
                    P_k  = Q_k + rho I + A_k^T P_{k+1} A_k + H_ux^T K_k     (the lower triangle, mirrored)

The H_uu solve is a hand-written Cholesky factorisation with two triangular solves (np.linalg has no longdouble).  e_ref is what float64
arithmetic costs on a case: the float64 restatement against the 80-bit one on the same inputs."""
import numpy as np

assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not the 80-bit extended type here: e_ref would measure nothing"

RHO = 1e-3
EPS64 = 2.2e-16
E_REF_MAX = 6e-11            # every case below stays under it (tests/test_riccati_ref_cpu.py), so 16 x e_ref < 1e-9

# (n, m, N, B) of tests/test_gpu_riccati.py, by what each is the smallest shape to break
CASES = {
    "one step": [(14, 7, 2, 1), (3, 2, 2, 1)],                                                       # a single K_0: terminal block only
    "carried P": [(14, 7, 3, 5), (14, 7, 33, 5)],                                                    # mirror, prefetch of knot k-1, odd batch
    "run-time dims": [(1, 1, 3, 5), (6, 3, 5, 5), (13, 5, 4, 5), (17, 17, 3, 5), (32, 8, 3, 2), (32, 32, 2, 2)],
    "foreign m": [(14, 3, 4, 3)],                                                                    # a 14-state handle, not the tuned control size
    "never computed": [                                    # the smallest shape at which ... (LDS bytes), each with P carried over two knots
        (3, 2, 4, 3),                                      # odd n, even m: the tile row of phase 3 that straddles A and B feeds a second and a third knot (704)
        (18, 18, 3, 2),                                    # tot = 1296: the first shape past the 1280-element prefetch, a tail of 16 lanes (23,360)
        (34, 32, 3, 2),                                    # w = 66: one column on the second trip of the elimination's strided loop; first above 64 KiB (73,984)
        (40, 30, 3, 2),                                    # w = 70, LM = 32 != m, LD = n (85,760)
        (64, 1, 3, 2),                                     # the widest P with one control: LM = 4 is three quarters pad (103,456)
        (64, 28, 3, 2),                                    # the last shape that fits the 160 KiB, on numbers (161,920)
    ],
}
ALL_CASES = [c for group in CASES.values() for c in group]


def make_case(n, m, N, B, dtype=np.float64):
    """(G, C) [B, ...] of a case in `dtype` (float32: the float64 blocks rounded).  Trajectory b depends only on (n, m, N, b)."""
    from mpcgpu_amd import synth
    from test_generic_producers_cpu import make_kkt_nm
    G, C, _, _ = synth.pack_kkt_dense(make_kkt_nm(N, B, 700 + N, n, m), dtype)
    return G, C


def unpack(G, C, n, m, N, dtype):
    """(Q [N, n, n], R [N-1, m, m], A [N-1, n, n], B [N-1, n, m]) of one trajectory's packed arrays, in dtype (widening is exact)."""
    gs, cs, nn = n * n + m * m, n * n + n * m, n * n
    G, C = np.asarray(G).astype(dtype), np.asarray(C).astype(dtype)
    assert G.size == gs * N - m * m and C.size == cs * (N - 1)
    Q = np.stack([G[k * gs:k * gs + nn].reshape(n, n).T for k in range(N)])
    R = np.stack([G[k * gs + nn:(k + 1) * gs].reshape(m, m).T for k in range(N - 1)]) if N > 1 else np.zeros((0, m, m), dtype)
    A = np.stack([-C[k * cs:k * cs + nn].reshape(n, n).T for k in range(N - 1)]) if N > 1 else np.zeros((0, n, n), dtype)
    Bm = np.stack([-C[k * cs + nn:(k + 1) * cs].reshape(m, n).T for k in range(N - 1)]) if N > 1 else np.zeros((0, n, m), dtype)
    return Q, R, A, Bm


def spd_solve(H, Y):
    """H^-1 Y for a symmetric positive definite H by Cholesky H = L L^T and two triangular solves, in the dtype of H."""
    m = H.shape[0]
    L = np.zeros_like(H)
    for j in range(m):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    Z = np.zeros_like(Y)
    for i in range(m):
        Z[i] = (Y[i] - L[i, :i] @ Z[:i]) / L[i, i]
    X = np.zeros_like(Y)
    for i in range(m - 1, -1, -1):
        X[i] = (Z[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def gains(G, C, n, m, N, rho, dtype=np.float64):
    """K [N-1, m, n] of one trajectory (matrices, not the column-major storage), every operation in `dtype`."""
    Q, R, A, Bm = unpack(G, C, n, m, N, dtype)
    rho = dtype(rho)
    In, Im = np.eye(n, dtype=dtype), np.eye(m, dtype=dtype)
    K = np.zeros((N - 1, m, n), dtype)
    P = Q[N - 1] + rho * In
    for k in range(N - 2, -1, -1):
        PA, PB = P @ A[k], P @ Bm[k]
        Huu = R[k] + rho * Im + Bm[k].T @ PB
        Hux = Bm[k].T @ PA
        K[k] = -spd_solve(Huu, Hux)
        Pn = Q[k] + rho * In + A[k].T @ PA + Hux.T @ K[k]
        P = np.tril(Pn) + np.tril(Pn, -1).T
    assert K.dtype == dtype
    return K


def flat(K):
    """[N-1, m, n] matrices -> the library's [N-1][m n] column-major storage, flattened."""
    return np.swapaxes(K, -1, -2).reshape(-1)


def knot_err(K, Kref):
    """max_k ||K_k - Kref_k||_max / max(1, ||Kref_k||_max), in the wider of the two dtypes."""
    if K.shape[0] == 0:
        return 0.0
    d = np.abs(K - Kref).reshape(K.shape[0], -1).max(axis=1)
    s = np.maximum(1, np.abs(Kref).reshape(K.shape[0], -1).max(axis=1))
    return float((d / s).max())


def e_ref(G, C, n, m, N, rho):
    """(e_ref, K64) of one trajectory: the float64 restatement against the 80-bit one on the same inputs."""
    K64 = gains(G, C, n, m, N, rho, np.float64)
    Kld = gains(G, C, n, m, N, rho, np.longdouble)
    return knot_err(K64.astype(np.longdouble), Kld), K64


# ---- the gains as the sensitivity of the QP's solution (tests/test_riccati_ref_cpu.py on the host, tests/test_gpu_riccati.py on the device) ----
def kkt_cond(k, rho, Cm):
    """cond_2 of the regularised KKT matrix dense_kkt_solve factors."""
    N, n, m = k.Q.shape[1], k.Q.shape[2], k.R.shape[-1]
    nz = (n + m) * N - m
    Gm = np.zeros((nz, nz))
    for kk in range(N):
        o = kk * (n + m)
        Gm[o:o + n, o:o + n] = k.Q[0, kk] + rho * np.eye(n)
        if kk < N - 1:
            Gm[o + n:o + n + m, o + n:o + n + m] = k.R[0, kk] + rho * np.eye(m)
    return float(np.linalg.cond(np.block([[Gm, Cm.T], [Cm, np.zeros((n * N, n * N))]])))


def perturbed(k, seed):
    """The same QP with another c in knot 1 only."""
    from mpcgpu_amd import synth
    c = k.c.copy()
    c[0, 1] += np.random.default_rng(seed).standard_normal(c.shape[-1])
    return synth.KKT(k.Q, k.R, k.A, k.Bm, k.q, k.r, c)


def feedback_residuals(dz0, dz1, K, k):
    """The two relative residuals of a solution difference caused in knot 1: du_k - K_k dx_k and dx_{k+1} - A_k dx_k - B_k du_k, k >= 1,
    against the largest entry of the difference."""
    N, n, m = k.Q.shape[1], k.Q.shape[2], k.R.shape[-1]
    d = dz1 - dz0
    dx = [d[kk * (n + m):kk * (n + m) + n] for kk in range(N)]
    du = [d[kk * (n + m) + n:(kk + 1) * (n + m)] for kk in range(N - 1)]
    scale = np.abs(d).max()
    assert scale > 1e-3, "the perturbation did not reach the solution"
    assert np.abs(dx[0]).max() <= 1e-9 * scale                 # x_0 is pinned: what hides K_0 from every right-hand side
    r_fb = max(np.abs(du[kk] - K[kk] @ dx[kk]).max() for kk in range(1, N - 1))
    r_dyn = max(np.abs(dx[kk + 1] - k.A[0, kk] @ dx[kk] - k.Bm[0, kk] @ du[kk]).max() for kk in range(1, N - 1))
    return r_fb / scale, r_dyn / scale


def kkt_of_packed(G, C, g, c, n, m, N):
    """One trajectory's packed (G, C, g, c) — what mpcg_generate_kkt_f64 leaves on the device — as a synth.KKT of batch 1 in float64 (exact:
    synth.pack_kkt_dense of the result gives the same arrays back)."""
    from mpcgpu_amd import synth
    Q, R, A, Bm = unpack(G, C, n, m, N, np.float64)
    gz = np.zeros((n + m) * N)
    gz[:(n + m) * N - m] = np.asarray(g, np.float64)
    gz = gz.reshape(N, n + m)
    return synth.KKT(Q[None], R[None], A[None], Bm[None], gz[None, :, :n].copy(), gz[None, :N - 1, n:].copy(), np.asarray(c, np.float64).reshape(1, N, n).copy())
