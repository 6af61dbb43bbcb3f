"""The case table of the one-step checkers (tests/pcg_step_model.py), shared by tests/test_pcg_step_model_cpu.py (the reference alone stays
inside the limits on these very inputs, no GPU), tests/test_gpu_invariants.py (the 12-argument entries) and tests/test_gpu_first_steps.py (the
batched entries).  CPU only.

A row is (precision, n, m, N, preconditioner, family, pinning options, expected "last_kernel_waves"): the smallest horizons that are no multiple
of a kernel's knots per wavefront or workgroup, in every build the launch plan (mpcg_pcg.hip: plan_f32, plan_f64) can reach, each pinned by the
options the plan reads so that a row cannot silently run another kernel.

Systems: n = 14 synth.make_kkt + synth.form_schur (float seed 9000 + N, double 9100 + N, as tests/test_gpu_invariants.py), n != 14
generic_pcg_cases.system.  Five trajectories per row; trajectory 0 is the one the single-trajectory tests use.  lambda0 = 0.1 x randn seeded by
(n, N).  Never-read slots — block (0, left), block (N-1, right), under block-Jacobi every off-diagonal block of Pinv — are NaN for the GPU
(device_matrices) and zeros for the host (host_matrices).  The host evaluates the matrices AS THE ROW'S KERNEL APPLIES THEM: a kernel that reads
only the lower block triangle applies block (k+1, left)^T where the stored block (k, right) stands — for the symmetric-stair Pinv the same triple
product associated the other way, equal to a few u of the data's precision, which in double is the size of what the checkers measure (predicted
from the stored right blocks, the double lane-quad kernels sit at 20-48 u of first_steps_quantities; from the blocks they apply, at 1.8).

K of a row: those of {1, 2, 10, 50, 167} with K <= it64 / 4, it64 the float64 oracle's iterations to |eta| < 1e-8 from the row's own lambda0
(generic_pcg_cases.k_for's count).  Measured with the float32 oracle as the only implementation: nearer convergence CG itself leaves the
limits (N = 3, K = 10 of it64 = 13: orthogonality 1.9e-3; N = 17, K = 167: conjugacy 1.6e-3, r 5.1) — no defect, so such pairs stay out."""
import collections
import functools

import numpy as np

import generic_pcg_cases as gc
from mpcgpu_amd import synth

B = 5
KS = (1, 2, 10, 50, 167)
RHO = 1e-3                  # (the generic systems: generic_pcg_cases' value)
DTYPE = {"f32": np.float32, "f64": np.float64}
LOWER_FAMILIES = (6, 7, 9, 10, 11)        # read only the left and diagonal block columns (include/mpcg.h, BLOCK SYMMETRY)
CLUSTERED = (7, 8, 10)

Row = collections.namedtuple("Row", "prec n m N pc family opts waves")


def row_id(r):
    opts = "-".join(f"{k}{v}" for k, v in r.opts) or "default"
    return f"{r.prec}-n{r.n}-N{r.N}-{r.pc}-family{r.family}-{opts}"


def _rows():
    out = []
    both = lambda prec, N, family, opts, waves: [out.append(Row(prec, 14, 7, N, pc, family, opts, waves)) for pc in ("ss", "jacobi")]
    ragged = (3, 17, 31, 33, 63, 65, 100, 127)          # the 32-, 64- and 128-knot builds of the lane-pair and lane-quad kernels
    for N in ragged:                                    # family 11: the lane-quad kernel, 16 knots per wavefront (128 knots: the split epilogue)
        both("f32", N, 11, (("pcg_lpk", 1), ("pcg_lqb", 1)), 2 if N <= 32 else 4 if N <= 64 else 8)
    for N in ragged:                                    # family 6: the lane-pair kernel (N <= 32: the half build, one wavefront per matrix)
        both("f32", N, 6, (("pcg_lpk", 1), ("pcg_lqb", 0)), 2 if N <= 32 else 4 if N <= 64 else 8)
    for N in (3, 17, 31, 33, 63):                       # family 5: four knots per wavefront slot; compiled (waves, slots): (4, 1..2), (8, 1..2), (16, 1)
        for w in (4, 8, 16):
            slots = -(-(-(-N // 4)) // w)                 # ceil(ceil(N / 4) / w) slots per wavefront
            if (w, slots) in ((4, 1), (4, 2), (8, 1), (8, 2), (16, 1)):
                both("f32", N, 5, (("pcg_rpl", 1), ("rpl_waves", w)), w)
    for N in (3, 33, 100, 129):                         # family 0: a compiled (waves, register triples) pair of each width, LDS rows as they fit
        for w, rt in ((4, 7), (8, 3), (16, 1)):
            both("f32", N, 0, (("pcg_lpk", 0), ("cluster", 0), ("pcg_waves", w), ("pcg_reg_rows", rt), ("pcg_lds_rows", -1)), w)
    for N in (129, 200, 257):                           # family 7: 128 knots per member, the last member of 2 and of 3 CUs ragged, nearly empty
        both("f32", N, 7, (), 8)
    for n, m, N in ((1, 1, 5), (7, 3, 127), (7, 3, 128), (13, 5, 9), (15, 7, 9), (33, 11, 40)):      # family 3: generic_pcg_cases' branch points
        for prec in ("f32", "f64"):
            for pc in ("ss", "jacobi"):
                out.append(Row(prec, n, m, N, pc, 3, (), gc.waves(n, N)))
    for N in (3, 17, 31):                               # double: the row-per-lane kernel, one slot per wavefront
        both("f64", N, 5, (), 4 if N <= 16 else 8)
    for N in (17, 33, 63):                              # the lane-quad kernel of one CU (32 knots per four wavefronts)
        both("f64", N, 9, (("pcg_lqk", 1),), 4 if N <= 32 else 8)
    for N in (33, 65, 100):                             # the clustered row-per-lane kernel: ceil(N / 32) members
        both("f64", N, 8, (("pcg_lqk", 0),), 8)
    for N in (65, 100, 129):                            # the clustered lane-quad kernel: ceil(N / 64) members
        both("f64", N, 10, (), 8)
    both("f64", 100, 3, (("cluster", 0),), 16)          # the streaming kernel at n = 14 (1400 rows: the wide workgroup)
    return out


ROWS = _rows()
ROWS32 = [r for r in ROWS if r.prec == "f32"]
ROWS64 = [r for r in ROWS if r.prec == "f64"]


@functools.lru_cache(maxsize=None)
def _raw(prec, n, m, N, pc):
    dt = DTYPE[prec]
    if n == 14:
        k = synth.make_kkt(N, B, (9000 if prec == "f32" else 9100) + N)
        S, P, g = synth.form_schur(k, precond=pc, dtype=dt, poison_unused=True)
        if pc == "jacobi":
            Pb = P.reshape(B, N, 3, n * n)
            Pb[:, :, 0] = np.nan
            Pb[:, :, 2] = np.nan
    else:
        S, P, g = gc.system(n, m, N, B, gc.SEED, dt, RHO, pc)
    lam0 = (0.1 * np.random.default_rng([n, N]).standard_normal((B, n * N))).astype(dt)
    for a in (S, P, g, lam0):
        a.flags.writeable = False
    return S, P, g, lam0


# fp16 matrix storage (mpcg_pcg_solve_f16; arithmetic in float): (N, options, family, waves).  N = 17 and 33: below the N = 36 boundary of the
# automatic lane-pair kernel, so the row-pair kernel's fp16 build <8, 6, 0>; 33 with the lane-pair kernel pinned: its 64-knot build; 100: the
# 128-knot build; 200: the clustered lane-pair kernel, two members.
F16_CASES = [(17, (), 0, 8), (33, (), 0, 8), (33, (("pcg_lpk", 1),), 6, 4), (100, (), 6, 8), (200, (), 7, 8)]
F16_RHO = 1e-2              # (tests/test_gpu_f16.py's: the systems stay definite after the rounding to half precision)


@functools.lru_cache(maxsize=None)
def f16_system(N, pc):
    """(S, Pinv, gamma, lambda0) in float, [B, ...], NaN in the never-read slots; the caller rounds S and Pinv to half precision."""
    k = synth.make_kkt(N, B, 9000 + N)
    S, P, g = synth.form_schur(k, rho=F16_RHO, precond=pc, poison_unused=True)
    if pc == "jacobi":
        Pb = P.reshape(B, N, 3, 14 * 14)
        Pb[:, :, 0] = np.nan
        Pb[:, :, 2] = np.nan
    lam0 = (0.1 * np.random.default_rng([14, N]).standard_normal((B, 14 * N))).astype(np.float32)
    for a in (S, P, g, lam0):
        a.flags.writeable = False
    return S, P, g, lam0


def device_matrices(r):
    """(S, Pinv, gamma, lambda0), [B, ...], for the batched entries: NaN in every slot the row's preconditioner never reads.  Read-only, shared."""
    return _raw(r.prec, r.n, r.m, r.N, r.pc)


def three_column_matrices(r):
    """The same for the 12-argument entries, which apply three columns of Pinv whatever the data (a block-Jacobi row: the off-diagonal blocks
    are zeros); block (0, left) and block (N-1, right) stay NaN."""
    S, P, g, lam0 = device_matrices(r)
    if r.pc == "jacobi":
        P = P.copy()
        Pb = P.reshape(B, r.N, 3, r.n * r.n)
        Pb[:, 1:, 0] = 0
        Pb[:, :-1, 2] = 0
    return S, P, g, lam0


def reads_lower(r):
    """The row's kernel reads only the left and diagonal block columns and applies block (k+1, left)^T where the stored block (k, right) stands
    (include/mpcg.h, BLOCK SYMMETRY): the lane-pair / lane-quad kernels and their clusters, and in double the streaming kernel at n = 14 once
    the handle's latch says block-symmetric."""
    return r.family in LOWER_FAMILIES or (r.prec == "f64" and r.family == 3 and r.n == 14)


def applied(M, n, N, lower):
    """One trajectory's matrix as the kernel applies it, never-read slots as zeros: for a lower-triangle kernel every right block is the next
    row's left block transposed.  The two are the same product associated two ways — equal to a few u, which is the size of what is checked."""
    M = np.nan_to_num(M)
    return gc.symmetrised(M, n, N) if lower else M


@functools.lru_cache(maxsize=None)
def host_matrices(r):
    """What the host side gets, [B, ...]: the matrices as the row's kernel applies them (applied), gamma, lambda0.  Read-only, shared."""
    S, P, g, lam0 = device_matrices(r)
    S, P = (np.stack([applied(M[b], r.n, r.N, reads_lower(r)) for b in range(B)]) for M in (S, P))
    S.flags.writeable = P.flags.writeable = False
    return S, P, g, lam0


@functools.lru_cache(maxsize=None)
def ks(r, b=None):
    """(it64, Ks) of the row: over the whole batch (b = None, the smallest count) or of trajectory b alone."""
    S, P, g, lam0 = host_matrices(r)
    sel = range(B) if b is None else (b,)
    it64 = min(gc.ref64(S[i], P[i], g[i], lam0[i], r.n, r.N, 2000, r.pc, tol=1e-8)["iters"] for i in sel)
    return it64, tuple(K for K in KS if 4 * K <= it64)
