"""The cases of the tolerance exit |eta'| < exit_tol, shared by tests/test_pcg_exit_cases_cpu.py (the reference alone meets every exact count;
planted defects fail; no GPU) and tests/test_gpu_exit.py (every kernel family).  CPU only.

Why the counts can be EXACT here: the systems are formed at rho = 1.0, where eta falls almost monotonically over the first iterations —
consecutive values 10 % to 7 x apart, float32 and float64 within 2.1e-5 relative of each other — and exit_tol is placed inside such a gap
with a margin of 1.05 on either side (about 2500 x that disagreement).  Every correct implementation, in either precision and any summation
order, then leaves at the same iteration.  (At rho = 1e-3 the crossing is erratic: tests/util.py, fp32_iters_band.)

Rows: those of tests/pcg_step_cases.py at which a (precision, family, workgroup width, pinning options) combination stands at its smallest
ragged horizon — for the lane-pair and lane-quad kernels that includes their 128-knot builds (N = 65), whose epilogue is code of its own — every
row of the generic kernel's branch points, and the fp16-storage cases.  (Where the smallest horizon's system converges faster than a ladder
needs, the build stands at its next horizon, or keeps a shallower ladder: too_fast, SHALLOW.)  One BASE trajectory per row: n = 14 synth.make_kkt(N, 1, 900 + N) +
synth.form_schur, n != 14 generic_pcg_cases.system, never-read slots NaN for the device and zeros for the host, the host's matrices as the row's
kernel applies them (pcg_step_cases.applied).

A LADDER is a batch built from the base trajectory: trajectory b is the base with gamma and lambda0 multiplied by 2^e_b, so its eta history is
the base's times 4^e_b and it crosses the call's one exit_tol at another iteration.  The predicted count of every trajectory is read from the
float64 oracle's eta history ON THAT TRAJECTORY'S OWN INPUTS.  Two ladders per row: cold (lambda0 = 0) and warm (lambda0 = 0.1 x randn, the row's
recipe).  Each holds
  * trajectories with at least four distinct predicted counts, one of them 0 and one >= 4 (search: e in -5..5, exit_tol one of 600 log-spaced
    values in [1e-5 eta_0, 2 eta_0], crossings at k <= 24 with eta_k >= 1e-5 x the trajectory's eta_0 and
    min(min_{j<k} eta_j / tol, tol / eta_k) >= 1.05);
  * one trajectory with gamma = 0 (cold: lambda0 = 0 too, eta = 0: leaves at 0 with flag 0, lambda untouched; warm: lambda0 kept, a crossing of
    its own inside the same margin);
  * one trajectory scaled up until eta_j >= 1.05 exit_tol for every j <= cap_hi: it reports iters = cap and flag 1.
Two caps per ladder: cap_hi = the largest predicted count + 3 and cap_mid = a middle predicted count — the trajectory predicted to cross at
exactly cap_mid still reports flag 0 (the tolerance is tested before the cap ends the loop, oracle/mpcg_oracle_impl.inc), later ones
iters = cap_mid and flag 1.

MARGIN, KMAX and DEPTH are conditions, not tunables: a row that cannot find its four counts gets another seed (SEED_SHIFT), never a smaller margin."""
import collections
import functools

import numpy as np

import generic_pcg_cases as gc
import oracle as orc
import pcg_step_cases as sc
from mpcgpu_amd import synth
from util import fp32_band, relinf

RHO = 1.0
MARGIN = 1.05
KMAX = 24
DEPTH = 1e-5                # a crossing no deeper than this below the trajectory's own eta_0
ES = tuple(range(-5, 6))
NTOL = 600
HMAX = KMAX + 4             # iterations of the eta history: cap_hi <= KMAX + 3
NEVER_DEPTH = {np.float32: 1e-10, np.float64: 1e-24}      # eta is a squared norm: u^2 = 3.6e-15 / 1.2e-32 relative is rounding noise; 3e4 / 1e8 x that
NEVER = 10 ** 6             # the predicted count of the trajectory that never crosses
SEED_SHIFT = {}             # row id -> added to the seed (empty: every row finds its counts at the first seed)
DTYPE = {"f32": np.float32, "f64": np.float64, "f16": np.float32}

Row = sc.Row
F16_ROWS = [Row("f16", 14, 7, N, pc, family, opts, waves) for N, opts, family, waves in sc.F16_CASES for pc in ("ss", "jacobi")]


def _key(r):
    """What a row is in the table for: the build (n = 14) or the branch point of the generic kernel (every one of them stays)."""
    return (r.prec, r.family, r.waves, r.opts) if r.n == 14 else (r.prec, r.n, r.m, r.N)


def too_fast(r):
    """Under the symmetric stair the systems of three knots (and of five scalar knots) converge faster than a ladder needs: eta_4 / eta_0 =
    1.2e-6 at n = 14, N = 3 (eta_3 / eta_0 = 8e-5), and (1, 1, N = 5) has converged exactly after 3 iterations (eta_3 / eta_0 = 2e-16) — at
    sixty seeds each, so no seed helps: there is no crossing at k >= 4 above DEPTH.  Block-Jacobi at the same sizes has them, but at
    (1, 1, N = 5) iteration 5 solves the five unknowns exactly: nothing can be predicted past it."""
    return (r.pc == "ss" and r.N <= 5) or r.n * r.N <= 5


# Rows that stand at a too_fast system because their build has no larger horizon in the table (the double row-per-lane kernel on four
# wavefronts: N <= 16; the generic kernel's smallest branch point): (distinct counts, deepest count, cap_hi - deepest count) of their ladders
# instead of (4, 4, 3).  (1, 1, N = 5): iteration 3 (block-Jacobi: 5) solves the five unknowns exactly, in float to a residual of 0 — no
# trajectory can be kept from crossing past it, so cap_hi is the deepest count itself.  Every other condition — margin, depth, the 0 exit, zero gamma, the trajectory
# that never crosses, cap_mid — holds for them as for the rest.
SHALLOW = {("f64", 14, 3, "ss"): (4, 3, 3), ("f32", 1, 5, "ss"): (3, 2, 0), ("f64", 1, 5, "ss"): (3, 2, 0),
           ("f32", 1, 5, "jacobi"): (4, 4, 0), ("f64", 1, 5, "jacobi"): (4, 4, 0)}


def need(r):
    return SHALLOW.get((r.prec, r.n, r.N, r.pc), (4, 4, 3))


def _rows():
    groups = {}
    for r in sc.ROWS:
        groups.setdefault((_key(r), r.pc), []).append(r)
    # the smallest horizon of every build and preconditioner at which a ladder fits the system (where none does: the smallest, a SHALLOW row)
    picked = [min([r for r in rows if not too_fast(r)] or rows, key=lambda r: r.N) for rows in groups.values()]
    return sorted(picked, key=sc.ROWS.index)


ROWS = _rows()
ROWS32 = [r for r in ROWS if r.prec == "f32"]
ROWS64 = [r for r in ROWS if r.prec == "f64"]
ALL_ROWS = ROWS + F16_ROWS
row_id = sc.row_id


def _freeze(*arrs):
    for a in arrs:
        a.flags.writeable = False
    return arrs


@functools.lru_cache(maxsize=None)
def base(r):
    """(S, Pinv, gamma, lambda0) of the row's base trajectory as the DEVICE gets it: NaN in every slot the row's preconditioner never reads;
    fp16 rows: S and Pinv rounded to half precision (numpy's conversion is the device's, tests/test_gpu_f16.py) and held in float16."""
    dt = DTYPE[r.prec]
    shift = SEED_SHIFT.get(row_id(r), 0)
    if r.n == 14:
        k = synth.make_kkt(r.N, 1, 900 + r.N + shift)
        S, P, g = synth.form_schur(k, rho=RHO, precond=r.pc, dtype=dt, poison_unused=True)
    else:
        S, P, g = (np.array(a) for a in gc.system(r.n, r.m, r.N, 1, gc.SEED + shift, dt, RHO, r.pc))
    S, P, g = S[0], P[0], g[0]
    if r.pc == "jacobi":
        Pb = P.reshape(r.N, 3, r.n * r.n)
        Pb[:, 0] = np.nan
        Pb[:, 2] = np.nan
    if r.prec == "f16":
        S, P = S.astype(np.float16), P.astype(np.float16)
        assert not np.isinf(S).any() and not np.isinf(P).any()
    lam0 = (0.1 * np.random.default_rng([r.n, r.N]).standard_normal((sc.B, r.n * r.N))).astype(dt)[0]
    return _freeze(S, P, g, lam0)


@functools.lru_cache(maxsize=None)
def host(r):
    """(S, Pinv) for the host side, in the row's arithmetic type: the never-read slots as zeros, the matrices as the row's kernel applies them."""
    S, P = base(r)[:2]
    dt = DTYPE[r.prec]
    return _freeze(*(sc.applied(M.astype(dt), r.n, r.N, sc.reads_lower(r)) for M in (S, P)))


def three_column(r):
    """(S, Pinv) of the base trajectory for the 12-argument entries, which apply three columns of Pinv whatever the data: under block-Jacobi the
    off-diagonal blocks are zeros; block (0, left) and block (N-1, right) stay NaN."""
    S, P = base(r)[:2]
    if r.pc == "jacobi":
        P = P.copy()
        Pb = P.reshape(r.N, 3, r.n * r.n)
        Pb[1:, 0] = 0
        Pb[:-1, 2] = 0
    return S, P


def run_oracle(r, g, lam0, cap, tol, dtype=None, S=None, P=None, hist=False):
    """The oracle's PCG on the row's host matrices (or S, P) in `dtype` (default: the row's arithmetic type)."""
    dt = dtype or DTYPE[r.prec]
    Sh, Ph = host(r) if S is None else (S, P)
    return orc.pcg(Sh.astype(dt), Ph.astype(dt), np.asarray(g, dt), np.asarray(lam0, dt), r.N, cap, tol, r.pc, n=r.n, hist=hist)


def _hist(r, g, lam0):
    """|eta| after setup and after each of HMAX iterations, float64 oracle, exit_tol = 0."""
    with np.errstate(all="ignore"):
        return np.array(run_oracle(r, g, lam0, HMAX, 0.0, np.float64, hist=True)["eta_hist"], np.float64)


def crossing(h, tol):
    """(k, margin) of the first eta_k < tol of the history h if it is a crossing every correct implementation must agree on, else None."""
    below = ~(h >= tol)                                   # (a NaN past exact convergence counts as below)
    if not below.any():
        return None
    k = int(np.argmax(below))
    if k > KMAX or not np.isfinite(h[k]) or not h[k] >= DEPTH * h[0]:
        return None
    margin = min(np.min(h[:k]) / tol if k else np.inf, tol / h[k] if h[k] > 0 else np.inf)
    return (k, margin) if margin >= MARGIN else None


Ladder = collections.namedtuple("Ladder", "tol gamma lam0 pred kinds cap_hi cap_mid")


def predicted(lad, cap):
    """(iters, flags) every implementation must report under max_iter = cap."""
    k = np.array(lad.pred)
    return np.minimum(k, cap).astype(np.int64), (k > cap).astype(np.int64)


def distinct_counts(lad):
    """Every count some trajectory reports under one of the two caps."""
    return sorted({int(v) for cap in (lad.cap_hi, lad.cap_mid) for v in predicted(lad, cap)[0]})


@functools.lru_cache(maxsize=None)
def ladder(r, warm):
    S, P, g, lam0 = base(r)
    dt = DTYPE[r.prec]
    l0 = lam0 if warm else np.zeros_like(lam0)
    scaled = lambda v, e: (v.astype(np.float64) * 2.0 ** e).astype(dt)          # (exact: a power of two, no underflow at these sizes)
    hists = {}

    def hist(e, with_gamma=True):
        key = (e, with_gamma)
        if key not in hists:
            hists[key] = _hist(r, scaled(g, e) if with_gamma else np.zeros_like(g), scaled(l0, e))
        return hists[key]

    eta0 = hist(0)[0]
    huge = 1e30 if dt == np.float32 else 1e280             # eta of the scaled-up trajectory stays far inside the format's range ...
    floor = NEVER_DEPTH[dt]                                # ... and above what the row's arithmetic resolves
    ranked = []
    for tol in np.geomspace(DEPTH * eta0, 2 * eta0, NTOL):
        found = {}
        for e in ES:
            c = crossing(hist(e), tol)
            if c and c[0] not in found:
                found[c[0]] = (e, c[1])
        if len(found) >= need(r)[0] and 0 in found and max(found) >= need(r)[1]:
            ranked.append((len(found), min(m for _, m in found.values()), tol, found))
    ranked.sort(key=lambda t: (-t[0], -t[1]))
    for _, _, tol, found in ranked:
        counts = sorted(found)
        cap_hi, cap_mid = counts[-1] + need(r)[2], counts[len(counts) // 2]
        never = next((e for e in range(6, 64) if np.isfinite(hist(e)[: cap_hi + 1]).all() and hist(e)[: cap_hi + 1].min() >= MARGIN * tol
                      and hist(e)[: cap_hi + 1].max() < huge and hist(e)[: cap_hi + 1].min() >= floor * hist(e)[0]), None)
        if warm:
            order = [0] + [s * e for e in range(1, 11) for s in (-1, 1)]
            zero_g = next(((e, crossing(hist(e, False), tol)) for e in order if crossing(hist(e, False), tol)), None)
        else:
            zero_g = (0, (0, np.inf))
        if never is None or zero_g is None:
            continue
        gam = [scaled(g, found[k][0]) for k in counts] + [np.zeros_like(g), scaled(g, never)]
        lam = [scaled(l0, found[k][0]) for k in counts] + [scaled(l0, zero_g[0]), scaled(l0, never)]
        pred = tuple(counts) + (zero_g[1][0], NEVER)
        kinds = ("search",) * len(counts) + ("zero_gamma", "never")
        gam, lam = _freeze(np.stack(gam), np.stack(lam))
        return Ladder(float(tol), gam, lam, pred, kinds, cap_hi, cap_mid)
    raise AssertionError(f"{row_id(r)} {'warm' if warm else 'cold'}: no exit_tol gives {need(r)[0]} distinct counts with a 0 and a >= {need(r)[1]} — another seed (SEED_SHIFT)")


def check_structure(lad, distinct=4, deepest=4, above=3):
    """The conditions of a ladder (module docstring); distinct, deepest, above: need(r)."""
    counts = [k for k, kind in zip(lad.pred, lad.kinds) if kind == "search"]
    assert len(set(counts)) == len(counts) >= distinct and 0 in counts and deepest <= max(counts) <= KMAX, counts
    assert lad.kinds.count("zero_gamma") == 1 and lad.kinds.count("never") == 1
    zg, nv = lad.kinds.index("zero_gamma"), lad.kinds.index("never")
    assert not lad.gamma[zg].any() and lad.pred[nv] == NEVER
    assert lad.cap_hi == max(counts) + above and lad.cap_mid in counts and 0 < lad.cap_mid < max(counts)
    assert np.isfinite(lad.gamma).all() and np.isfinite(lad.lam0).all() and lad.tol > 0


# ---- the assertions of the GPU tests (tests/test_pcg_exit_cases_cpu.py runs planted defects against these very functions) ---------------------------

def check_counts(tag, lad, cap, iters, flags):
    """Exact: the iteration count and the exit flag of every trajectory of the ladder under max_iter = cap."""
    it, fl = predicted(lad, cap)
    assert np.array_equal(np.asarray(iters, np.int64), it) and np.array_equal(np.asarray(flags, np.int64), fl), \
        (tag, "cap", cap, "exit_tol", lad.tol, "iters", list(map(int, iters)), "predicted", it.tolist(), "flags", list(map(int, flags)), "predicted", fl.tolist())


def check_lambda_bits(tag, lad, cap, lam, fixed):
    """lambda of the tolerance launch under `cap` carries, for every trajectory, the bits of the launch with max_iter = its predicted count and
    exit_tol = 0 (fixed[k]: lambda of that launch, [B, n N]); a count of 0: the bits of lambda0."""
    it, _ = predicted(lad, cap)
    for b, k in enumerate(it):
        want = lad.lam0[b] if k == 0 else fixed[int(k)][b]
        assert np.asarray(lam[b]).tobytes() == np.asarray(want).tobytes(), (tag, "cap", cap, "trajectory", b, lad.kinds[b], "count", int(k))
        if k == 0 and 0 in fixed:
            assert np.asarray(fixed[0][b]).tobytes() == np.asarray(want).tobytes(), (tag, "max_iter = 0 must hand lambda0 back", b)


def state_trajectories(lad):
    """[(trajectory, cap)] of the 12-argument checks: the 0 exit, the deepest tolerance exit (k >= 2), the one that never crosses under cap_mid."""
    search = [b for b, kind in enumerate(lad.kinds) if kind == "search"]
    deep = max(search, key=lambda b: lad.pred[b])
    assert lad.pred[deep] >= 2
    return [(lad.pred.index(0), lad.cap_hi), (deep, lad.cap_hi), (lad.kinds.index("never"), lad.cap_mid)]


def state_reference(r, lad, b, cap):
    """What the 12-argument entry must return for trajectory b under (cap, exit_tol): the float64 oracle's state at that exit, and the
    tolerance of each vector by the suite's rule max(2e-5 if k <= 3 else 1e-3, 4 x band) (tests/fuzz_cases.py), the band measured from the
    oracle in the row's own precision, never from a kernel.  lambda and r of a tolerance exit after k iterations are those of k fixed iterations;
    p is left as the k-th iteration used it (the reference's rule) — the p of k - 1 fixed iterations — and after a cap exit it is updated.
    Double rows: the float64 oracle on inputs perturbed by 1e-16 relative against the unperturbed float64 run, the floors x 2^-29 (u64 / u32)."""
    g, lam0 = lad.gamma[b], lad.lam0[b]
    ref = run_oracle(r, g, lam0, cap, lad.tol, np.float64)
    k, capped = ref["iters"], ref["max_iter_exit"]
    assert (k, int(capped)) == tuple(int(v[b]) for v in predicted(lad, cap))
    tols = {}
    for vec in ("lam", "r", "p"):
        K = k - 1 if vec == "p" and not capped and k > 0 else k
        floor = 2e-5 if k <= 3 else 1e-3
        if r.prec == "f64":
            band, floor = band64(r, g, lam0, K, ref[vec], vec), floor * 2.0 ** -29
        else:
            Sh, Ph = host(r)
            band = fp32_band(orc, Sh, Ph, g, lam0, r.N, K, r.pc, ref[vec], n=r.n, vec=vec)
        tols[vec] = (max(floor, 4 * band), band)
    return ref, tols


def perturbed(a, rel, rng, dtype):
    return (a.astype(np.longdouble) * (1 + np.longdouble(rel) * rng.standard_normal(a.shape))).astype(dtype)


def band64(r, g, lam0, K, ref, vec, trials=4):
    """util.fp32_band's measurement one precision up: the float64 oracle after K fixed iterations on S and gamma perturbed by 1e-16 relative."""
    Sh, Ph = host(r)
    rng = np.random.default_rng(K * 1000 + r.N)
    return max(relinf(run_oracle(r, perturbed(g, 1e-16, rng, np.float64), lam0, K, 0.0, S=perturbed(Sh, 1e-16, rng, np.float64), P=Ph)[vec], ref)
               for _ in range(trials))


def check_state(tag, ref, tols, lam, res, p):
    """lambda, d_r and d_p of a 12-argument call against state_reference; returns the worst error / tolerance."""
    worst = 0.0
    for vec, got in (("lam", lam), ("r", res), ("p", p)):
        got = np.asarray(got, np.float64)
        assert np.isfinite(got).all(), (tag, vec, "not finite")
        scale = np.abs(ref[vec]).max()
        err = relinf(got, ref[vec]) if scale > 0 else np.abs(got).max()
        assert err <= tols[vec][0], (tag, vec, "error", err, "tolerance", tols[vec][0], "band", tols[vec][1])
        worst = max(worst, err / tols[vec][0])
    return worst
