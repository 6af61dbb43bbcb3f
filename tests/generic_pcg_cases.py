"""The cases of the generic-state-size PCG kernel (pcg_generic_kernel<T, 0, NTHR>, mpcgpu_amd/csrc/pcg_f64.hip.h: every handle with
state_size != 14) — shared by tests/test_generic_pcg_cpu.py (pins these inputs to what the reference arithmetic can do, no GPU),
tests/test_gpu_generic_pcg.py (the kernel against the float64 oracle) and tools/fuzz_families.py --generic.  CPU only, except fuzz(gpu=True).

The systems are real Schur complements: KKT blocks for any 1 <= m <= n (test_generic_producers_cpu.make_kkt_nm) through the ORACLE's formation,
whose never-written slots — block (0, left), block (N-1, right), and under block-Jacobi every off-diagonal block of Pinv — stay NaN.  The GPU gets
them raw, the oracle PCG gets nan_to_num: a kernel that reads a slot it must not read returns NaN."""
import collections
import functools
import time

import numpy as np

import oracle as orc
from mpcgpu_amd import synth
from test_generic_producers_cpu import make_kkt_nm
from util import fp32_band, relinf

SEED = 5                    # make_kkt_nm seed of the fixed cases
FUZZ_SEED = 20261018        # the seeded slice inside the `-m gpu` suite (and its CPU twin)
LDS_MAX = 160 * 1024
RHOS = (1e-3, 1e-1)
PCS = ("ss", "jacobi")

# (n, m, N, what the shape is for).  Rows = n * N; 256 threads below 896 rows, 1024 from there (pcg_generic_threads).
SHAPES = [
    (1, 1, 2, "two rows: one wavefront partly idle, fifteen slots of red[] idle, every row skips a neighbour"),
    (1, 1, 5, "smallest interior"),
    (7, 3, 127, "889 rows: the last shape on 256 threads, 4 trips of the row loop"),
    (7, 3, 128, "896 rows: the first shape on 1024 threads, under one trip"),
    (13, 5, 9, "neighbour of the tuned size"),
    (15, 7, 9, "neighbour of the tuned size"),
    (3, 1, 250, "750 rows on 256 threads: 3 trips, long thin horizon"),
    (33, 11, 40, "1320 rows on 1024 threads: 2 trips, odd n"),
    (64, 20, 39, "2496 rows: 3 trips; 41 KiB float, 82 KiB double: the attribute path above 64 KiB"),
    (40, 10, 128, "float 82 KiB; double 165,248 B: the double refusal"),
    (64, 21, 158, "162,880 B: the largest horizon mpcg_create accepts at n = 64; float only"),
]
ASYM_SHAPES = [(7, 3, 128), (13, 5, 9), (33, 11, 40)]
ASYM_KS = (1, 3)            # (an asymmetric S is no CG system: later iterates are chaotic in any arithmetic, tests/test_generic_pcg_cpu.py)


def lds_bytes(n, N, esz=4):
    """pcg_generic_lds_elems x the element size: p and r padded by a zero knot either side, lambda, the product, 16 partial sums."""
    return esz * (2 * (N + 2) * n + 2 * N * n + 16)


def waves(n, N):
    return 16 if n * N >= 896 else 4


def fits_double(n, N):
    return lds_bytes(n, N, 8) <= LDS_MAX


def build_system(n, m, N, B, seed, dtype, rho, pc):
    k = make_kkt_nm(N, B, seed, n, m)
    G, C, g, c = synth.pack_kkt_dense(k, dtype)
    out = [orc.form_schur(G[b], C[b], g[b], c[b], N, dtype(rho), ss=(pc == "ss"), n=n, m=m)[:3] for b in range(B)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


@functools.lru_cache(maxsize=None)
def system(n, m, N, B, seed, dtype, rho, pc):
    """(S, Pinv, gamma), [B, 3 n n N] / [B, n N], in `dtype` arithmetic of the oracle's formation; NaN where the oracle never writes.
    Computed once per argument tuple and shared: read-only."""
    arrs = build_system(n, m, N, B, seed, dtype, rho, pc)
    for a in arrs:
        a.flags.writeable = False
    return arrs


def start(n, N, B, seed, dtype):
    """Trajectory 0 starts cold, every other one from 0.1 * randn."""
    lam0 = (0.1 * np.random.default_rng([seed, n, N, 77]).standard_normal((B, n * N))).astype(dtype)
    lam0[0] = 0
    return lam0


def z(a, dtype=None):
    """What the oracle's PCG gets: the never-written slots as zeros."""
    a = np.nan_to_num(a)
    return a if dtype is None else a.astype(dtype)


def ref64(S, P, g, lam0, n, N, K, pc, tol=0.0, hist=False):
    """The float64 oracle on one trajectory's inputs as given (float inputs widened exactly)."""
    return orc.pcg(z(S, np.float64), z(P, np.float64), np.asarray(g, np.float64), np.asarray(lam0, np.float64), N, K, tol, pc, n=n, hist=hist)


def k_for(S, P, g, lam0, n, N, pc):
    """(it64, Ks) of a batch [B, ...] or of one trajectory.  it64: the float64 oracle's iterations to |eta| < 1e-8 from the case's own start
    vector (the smallest over the batch).  Fixed-count CG past exact convergence is 0 / 0 by construction ((1, 1, N = 2) under "ss" has
    converged after 1 iteration; K = 3 is non-finite in the float32 oracle), so fixed-count runs use
    K in {1, 3, min(25, it64 - 3)} within [1, it64 - 3], and K = 1 alone when it64 <= 3."""
    S, P, g, lam0 = (np.atleast_2d(a) for a in (S, P, g, lam0))
    it64 = min(ref64(S[b], P[b], g[b], lam0[b], n, N, 2000, pc, tol=1e-8)["iters"] for b in range(S.shape[0]))
    if it64 <= 3:
        return it64, [1]
    return it64, sorted({K for K in (1, 3, min(25, it64 - 3)) if 1 <= K <= it64 - 3} or {1})


def tol32(S, P, g, lam0, n, N, K, pc, ref, vec="lam"):
    """The suite's tight tier for float (tests/util.py): max(2e-5, 4 x the CPU float32 band) around the float64 vector `ref`."""
    return max(2e-5, 4 * fp32_band(orc, S, P, g, lam0, N, K, pc, ref, n=n, vec=vec))


def tol64(S, P, g, lam0, n, N, K, pc, ref, vec="lam"):
    """tests/test_gpu_f64.py's rule: max(1e-10, 20 x band), band = the float64 oracle under a one-ulp change of gamma in either direction."""
    Sz, Pz = z(S), z(P)
    band = max(relinf(orc.pcg(Sz, Pz, np.nextafter(g, s), lam0, N, K, 0.0, pc, n=n)[vec], ref) for s in (np.inf, -np.inf))
    return max(1e-10, 20 * band)


def _blocks(M, n, N):
    return M.reshape(N, 3, n, n)          # [knot][block column][c][i]: column-major blocks


def symmetrised(M, n, N):
    """A copy with every right block := the next row's left block transposed — what a kernel that never reads the right block column solves."""
    out = np.array(M, copy=True)
    b = _blocks(out, n, N)
    b[:-1, 2] = np.swapaxes(b[1:, 0], -1, -2)
    return out


def _asym(M, n, N, rng):
    out = symmetrised(M, n, N)
    b = _blocks(out, n, N)
    scale = 0.2 * np.abs(b[1:, 0]).max(axis=(-1, -2), keepdims=True)
    b[:-1, 2] += scale * rng.uniform(-1.0, 1.0, size=(N - 1, n, n)).astype(M.dtype)
    return out


def asymmetric(S, Pinv, n, N, seed):
    """One trajectory ("ss": Pinv has off-diagonal blocks).  {"pinv": (S, Pinv'), "s": (S', Pinv)}: in the primed matrix every right block
    (k, 2) is block (k+1, 0)^T + E, E a structural perturbation of 20 % of that block's largest entry; the left blocks are untouched.
    The oracle's PCG reads all three block columns, as the kernel must on a generic handle (PcgArgsG::lower stays 0)."""
    rng = np.random.default_rng([seed, n, N, 1234])
    return {"pinv": (np.array(S, copy=True), _asym(Pinv, n, N, rng)), "s": (_asym(S, n, N, rng), np.array(Pinv, copy=True))}


def fuzz_draw(rng):
    """One random case: n in 1..64 without 14, m in 1..n, N in three bands (2..8, 9..64, up to the LDS limit of a float handle) with
    n * N <= 2600 (CPU time of the oracle), B in 1..4, preconditioner, warm or cold start, float or double (about 70 / 30)."""
    n = int(rng.choice([v for v in range(1, 65) if v != 14]))
    m = int(rng.integers(1, n + 1))
    n_max = max(2, min(2048, 2600 // n, (LDS_MAX // 4 - 16 - 4 * n) // (4 * n)))
    lo, hi = [(2, 8), (9, 64), (65, 2048)][int(rng.choice(3, p=[0.2, 0.3, 0.5]))]
    N = int(rng.integers(min(lo, n_max), min(hi, n_max) + 1))
    return dict(n=n, m=m, N=N, B=int(rng.integers(1, 5)), pc=str(rng.choice(PCS)), warm=bool(rng.random() < 0.5),
                dtype=np.float32 if rng.random() < 0.7 else np.float64, seed=int(rng.integers(1 << 30)))


def fuzz(cases=80, seed=FUZZ_SEED, gpu=None, verbose=True):
    """Seeded random cases through the oracle — and, with gpu=True, through the generic kernel: every trajectory against the float64 oracle
    iterate after the same K iterations (K from k_for), inside tol32 / tol64; iteration counts, exit flags, kernel family and workgroup width
    checked.  Counters in the style of tests/fuzz_cases.py."""
    orc.build()
    rng = np.random.default_rng(seed)
    width, warm_cases, double_cases, breakdown, worst, bad = collections.Counter(), 0, 0, 0, 0.0, 0
    if gpu:
        import torch
        from mpcgpu_amd import PcgSolver, pcg_config
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t0 = time.time()
    for ci in range(cases):
        c = fuzz_draw(rng)
        n, m, N, B, pc, dt = c["n"], c["m"], c["N"], c["B"], c["pc"], c["dtype"]
        S, P, g = build_system(n, m, N, B, c["seed"], dt, 1e-3, pc)
        lam0 = (0.1 * rng.standard_normal((B, n * N))).astype(dt) if c["warm"] else np.zeros((B, n * N), dt)
        it64, Ks = k_for(S, P, g, lam0, n, N, pc)
        K = int(rng.choice(Ks))
        width[64 * waves(n, N)] += 1
        warm_cases += int(c["warm"])
        double_cases += int(dt == np.float64)
        refs, tols = [], []
        for b in range(B):
            ref = ref64(S[b], P[b], g[b], lam0[b], n, N, K, pc)["lam"]
            own = orc.pcg(z(S[b]), z(P[b]), g[b], lam0[b], N, K, 0.0, pc, n=n)["lam"]
            if not (np.isfinite(ref).all() and np.isfinite(own).all()):
                breakdown += 1
            refs.append(ref)
            tols.append((tol32 if dt == np.float32 else tol64)(S[b], P[b], g[b], lam0[b], n, N, K, pc, ref))
        if not gpu:
            continue
        sol = PcgSolver(N, max_batch=B, state_size=n)
        lam = dev(lam0.copy())
        it, ex = (sol.solve if dt == np.float32 else sol.solve_f64)(dev(S), dev(P), dev(g), lam, pcg_config(pcg_exit_tol=0.0, pcg_max_iter=K), pc)
        torch.cuda.synchronize()
        lam_h, it_h, ex_h = lam.cpu().numpy(), it.cpu().numpy(), ex.cpu().numpy()
        ok = (it_h == K).all() and (ex_h == 1).all() and sol.get_option("last_kernel_family") == 3 \
            and sol.get_option("last_kernel_waves") == waves(n, N) and sol.get_option("last_kernel_lds_bytes") == lds_bytes(n, N, np.dtype(dt).itemsize)
        for b in range(B):
            e = relinf(lam_h[b], refs[b]) if np.isfinite(lam_h[b]).all() else np.inf
            worst = max(worst, e / tols[b])
            ok = ok and e <= tols[b]
        sol.close()
        if not ok:
            bad += 1
            if verbose:
                print(f"MISMATCH case {ci}: n={n} m={m} N={N} B={B} {pc} {np.dtype(dt).name} warm={c['warm']} K={K} (it64 {it64}): iters {it_h.tolist()} "
                      f"exit {ex_h.tolist()} finite {bool(np.isfinite(lam_h).all())}", flush=True)
    return {"cases": cases, "seed": seed, "seconds": time.time() - t0, "widths": dict(sorted(width.items())), "warm_start_cases": warm_cases,
            "double_cases": double_cases, "reference_breakdowns": breakdown, "worst_error_over_tolerance": worst, "mismatches": bad}


def check_fuzz_inputs(r):
    """What a fuzz seed must cover (conditions on the inputs: tests/test_generic_pcg_cpu.py)."""
    assert r["reference_breakdowns"] == 0, r
    assert set(r["widths"]) == {256, 1024} and min(r["widths"].values()) >= 15, r
    assert r["warm_start_cases"] >= 25 and r["double_cases"] >= 15, r
