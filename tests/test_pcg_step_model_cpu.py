"""CPU: the one-step checkers (tests/pcg_step_model.py) on the case table of the GPU tests (tests/pcg_step_cases.py), no GPU.

  * The reference alone stays inside the limits: the oracle's PCG (float32 for the float rows, float64 for the double rows) through both checkers
    on every row and K the GPU tests use — a limit a correct sequential implementation does not meet would say nothing about a kernel.
  * The checkers see what they are for: a numpy float32 restatement of PCG on the bd layout passes; with ONE defect of the kind a hand-scheduled
    kernel can have (a block left out at a ragged end, a share left out of an inner product, a stale scalar, one matrix entry from the
    neighbouring column) it fails."""
import numpy as np
import pytest

import pcg_step_cases as pc_cases
from pcg_step_model import EPS32, FIRST_STEPS_LIMIT, FIRST_STEPS_ORACLE_WORST, HP, LIMITS, first_steps_quantities, initial_state_quantities, step_quantities

U64 = 2.0 ** -53
f32 = np.float32


def limits_for(prec):
    """(u, LIMITS at that u): conjugacy and orthogonality scale with u (float32's limit x 2^-29 in double, as tests/test_gpu_invariants.py)."""
    if prec == "f32":
        return EPS32, dict(LIMITS)
    return U64, {k: v * (2.0 ** -29 if k in ("conjugacy", "orthogonality") else 1.0) for k, v in LIMITS.items()}


def high_precision(prec):
    if prec == "f64" and np.finfo(np.longdouble).eps > 2.0 ** -60:
        pytest.skip("no extended-precision long double on this host")
    return np.float64 if prec == "f32" else np.longdouble


def oracle_quantities(orc, r):
    """Every checked quantity of the oracle's own PCG on the row: {(K, key): value} of step_quantities for trajectory 0 (the trajectory of the
    12-argument tests), {(b, key): value} of first_steps_quantities for all five, {key: value} of the K = 0 state."""
    S, P, g, lam0 = pc_cases.host_matrices(r)
    u, _ = limits_for(r.prec)
    run = lambda b, K: orc.pcg(S[b], P[b], g[b], lam0[b], r.N, K, 0.0, r.pc, n=r.n)
    state = lambda o: [o[k].astype(HP[0]) for k in ("lam", "r", "p")]
    steps, first = {}, {}
    o0 = run(0, 0)
    assert o0["iters"] == 0 and o0["max_iter_exit"] and o0["lam"].tobytes() == lam0[0].tobytes()
    init = initial_state_quantities(S[0], P[0], g[0], lam0[0], o0["r"], o0["p"], r.N, r.n, r.pc, u)
    for K in pc_cases.ks(r, 0)[1]:
        q = step_quantities(S[0], P[0], g[0], lam0[0], state(run(0, K - 1)), state(run(0, K)), r.N, K, EPS32=u, n=r.n)
        steps.update({(K, k): v for k, v in q.items()})
    for b in range(pc_cases.B):
        q = first_steps_quantities(S[b], P[b], g[b], lam0[b], run(b, 1)["lam"], run(b, 2)["lam"], r.N, r.n, r.pc, u)
        first.update({(b, k): v for k, v in q.items()})
    return steps, first, init


@pytest.mark.parametrize("r", pc_cases.ROWS, ids=pc_cases.row_id)
def test_the_reference_alone_stays_inside_the_limits(orc, r):
    HP[0] = high_precision(r.prec)
    try:
        steps, first, init = oracle_quantities(orc, r)
    finally:
        HP[0] = np.float64
    _, lim = limits_for(r.prec)
    print(f"{pc_cases.row_id(r)}: it64 {pc_cases.ks(r, 0)[0]} K {pc_cases.ks(r, 0)[1]} "
          + " ".join(f"{k} {max([v for (_, k2), v in steps.items() if k2 == k], default=0):.2g}" for k in LIMITS)
          + " | " + " ".join(f"{k} {max(v for (_, k2), v in first.items() if k2 == k):.2g}" for k in ("lam1", "lam2"))
          + " | K=0 " + " ".join(f"{k} {v:.2g}" for k, v in init.items()))
    for (K, key), v in steps.items():
        assert v <= lim[key], (K, key, v, lim[key])
    for (b, key), v in first.items():
        assert v <= FIRST_STEPS_LIMIT, (b, key, v, FIRST_STEPS_LIMIT)
    for key, v in init.items():
        assert v <= lim[key], ("K = 0", key, v, lim[key])


@pytest.mark.parametrize("pc", ["ss", "jacobi"])
@pytest.mark.parametrize("N", sorted({c[0] for c in pc_cases.F16_CASES}))
def test_the_reference_stays_inside_the_first_steps_limit_on_half_precision_matrices(orc, N, pc):
    """The fp16-storage systems of tests/test_gpu_first_steps.py: the float32 oracle on the matrices rounded to half precision (numpy's
    conversion is the device's: tests/test_gpu_f16.py)."""
    S, P, g, lam0 = pc_cases.f16_system(N, pc)
    S, P = (np.nan_to_num(M).astype(np.float16).astype(f32) for M in (S, P))
    assert np.isfinite(S).all() and np.isfinite(P).all()
    for b in range(pc_cases.B):
        lam = [orc.pcg(S[b], P[b], g[b], lam0[b], N, K, 0.0, pc)["lam"] for K in (1, 2)]
        q = first_steps_quantities(S[b], P[b], g[b], lam0[b], lam[0], lam[1], N, 14, pc, EPS32)
        print(f"fp16 storage N={N} {pc} trajectory {b}: " + " ".join(f"{k} {v:.2g}" for k, v in q.items()))
        for key, v in q.items():
            assert v <= FIRST_STEPS_LIMIT, (b, key, v)


def test_every_row_has_a_k_and_the_table_covers_the_builds():
    """The K rule leaves at least K = 1 on every row but (1, 1, N = 5) under the symmetric stair, whose five unknowns converge in it64 = 3
    iterations: that row keeps the K = 0 state and the first-steps check.  The table holds every family and workgroup width it is for."""
    for r in pc_cases.ROWS:
        it64, Ks = pc_cases.ks(r, 0)
        assert Ks[:1] == (1,) or ((r.n, r.N, r.pc) == (1, 5, "ss") and it64 < 4), (pc_cases.row_id(r), it64, Ks)
    have = {(r.prec, r.family) for r in pc_cases.ROWS}
    assert have == {("f32", f) for f in (0, 3, 5, 6, 7, 11)} | {("f64", f) for f in (3, 5, 8, 9, 10)}
    assert {r.waves for r in pc_cases.ROWS if r.prec == "f32" and r.family == 5} == {4, 8, 16}
    assert {r.waves for r in pc_cases.ROWS if r.family == 0} == {4, 8, 16}
    assert {r.waves for r in pc_cases.ROWS if r.family == 11} == {2, 4, 8}
    assert len({pc_cases.row_id(r) for r in pc_cases.ROWS}) == len(pc_cases.ROWS)
    worst = max(FIRST_STEPS_ORACLE_WORST.values())              # the limit is 6 x the oracle's recorded worst, rounded up to one digit
    assert 6 * worst <= FIRST_STEPS_LIMIT == 20.0 and 6 * worst > 10.0


# ---- the checkers see what they are for --------------------------------------------------------------------------------------------------------

def host_pcg(S, P, g, lam0, N, K, pc, defect=None, knot=None, Pss=None, n=14):
    """Textbook PCG in float32 numpy on the bd layout (include/mpcg.h, THE HOT PATH), K iterations, exit_tol = 0: (lambda, r, p).
    `defect` at block row `knot`: one slip of the kind a hand-scheduled kernel can make (see DEFECTS)."""
    Sb = np.array(S, f32).reshape(N, 3, n, n).transpose(0, 1, 3, 2).copy()          # [k][col] as row-major matrices
    Pb = np.array(P, f32).reshape(N, 3, n, n).transpose(0, 1, 3, 2).copy()
    if defect == "entry_from_neighbouring_column":      # row 6 of the knot's diagonal block of S: column 9 holds column 10's entry
        Sb[knot, 1, 6, 9] = Sb[knot, 1, 6, 10]
    if defect == "entry_from_neighbouring_column_row7":
        Sb[knot, 1, 7, 3] = Sb[knot, 1, 7, 2]

    def mv(Mb, x, cols, is_S):
        X = x.reshape(N, n)
        y = np.einsum("kij,kj->ki", Mb[:, 1], X)
        if is_S and defect == "diagonal_block_on_shifted_vector":         # the last knot's diagonal block meets x one entry on
            y[N - 1] = Mb[N - 1, 1] @ np.roll(X[N - 1], 1)
        if cols == 3:
            y[1:] += np.einsum("kij,kj->ki", Mb[1:, 0], X[:-1])
            up = np.einsum("kij,kj->ki", Mb[:-1, 2], X[1:])
            if is_S and defect == "transposed_block_left_out":            # L_{knot+1}^T x_{knot+1} never reaches row `knot`
                up[knot] = 0
            y[:-1] += up
        if not is_S and defect == "jacobi_applies_a_left_block":          # block-Jacobi: only the diagonal blocks may be applied
            y[knot] += (np.array(Pss, f32).reshape(N, 3, n, n)[knot, 0].T @ X[knot - 1]).astype(f32)
        return y.reshape(-1).astype(f32)

    def dot(a, b, skip):
        t = (a * b).reshape(N, n).sum(axis=1, dtype=f32)
        if skip:
            t[knot] = 0
        return t.sum(dtype=f32)

    pcols = 3 if pc == "ss" else 1
    g, lam = np.asarray(g, f32), np.array(lam0, f32)
    r = g - mv(Sb, lam, 3, True)
    z = mv(Pb, r, pcols, False)
    p = z.copy()
    eta = dot(r, z, defect == "share_left_out_of_r_rtilde")
    eta_before = eta
    for _ in range(K):
        ups = mv(Sb, p, 3, True)
        alpha = f32(eta / dot(p, ups, defect == "share_left_out_of_p_Sp"))
        lam = lam + alpha * p
        r = r - alpha * ups
        z = mv(Pb, r, pcols, False)
        eta_new = dot(r, z, defect == "share_left_out_of_r_rtilde")
        beta = f32(eta_new / (eta_before if defect == "beta_from_the_previous_eta" else eta))
        p = z + beta * p
        eta_before, eta = eta, eta_new
    return lam, r, p


# (defect, preconditioner, touches the first two iterations' lambda)
DEFECTS = [
    ("transposed_block_left_out", "ss", True),
    ("diagonal_block_on_shifted_vector", "ss", True),
    ("share_left_out_of_p_Sp", "ss", True),
    ("share_left_out_of_r_rtilde", "ss", True),
    ("beta_from_the_previous_eta", "ss", False),       # beta_1 = eta_1 / eta_0 either way: lambda_3 is the first to differ
    ("entry_from_neighbouring_column", "ss", True),
    ("entry_from_neighbouring_column_row7", "ss", True),
    ("jacobi_applies_a_left_block", "jacobi", True),
]


def checker_verdicts(S, P, g, lam0, N, pc, Ks, **kw):
    """(keys of step_quantities over their limit at any K of Ks, keys of first_steps_quantities over theirs) of host_pcg."""
    run = lambda K: [v.astype(np.float64) for v in host_pcg(S, P, g, lam0, N, K, pc, **kw)]
    bad = set()
    for K in Ks:
        try:
            q = step_quantities(S, P, g, lam0, run(K - 1), run(K), N, K)
        except AssertionError:                          # (eta or p' S p of the wrong sign: the checker refuses the state outright)
            bad.add("sign")
            continue
        bad |= {k for k, lim in LIMITS.items() if not q[k] <= lim}
    try:
        q = first_steps_quantities(S, P, g, lam0, run(1)[0], run(2)[0], N, 14, pc, EPS32)
    except AssertionError:
        return bad, {"sign"}
    return bad, {k for k, v in q.items() if not v <= FIRST_STEPS_LIMIT}


@pytest.mark.parametrize("N", [17, 33])
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
def test_the_restatement_passes_both_checkers(N, pc):
    r = next(x for x in pc_cases.ROWS32 if x.n == 14 and x.N == N and x.pc == pc)
    S, P, g, lam0 = (a[0] for a in pc_cases.host_matrices(r))
    Ks = [K for K in pc_cases.ks(r, 0)[1] if K >= 2]
    assert Ks
    assert checker_verdicts(S, P, g, lam0, N, pc, Ks) == (set(), set())


NO_KNOT_OF_ITS_OWN = ("diagonal_block_on_shifted_vector", "beta_from_the_previous_eta")      # (the last knot by definition / a scalar)
DEFECT_CASES = [(d, pc, early, N, where) for d, pc, early in DEFECTS for N in (17, 33) for where in ("last", "interior")
                if where == "last" or d not in NO_KNOT_OF_ITS_OWN]


@pytest.mark.parametrize("defect,pc,early,N,where", DEFECT_CASES, ids=[f"{c[0]}-N{c[3]}-{c[4]}" for c in DEFECT_CASES])
def test_one_defect_fails_the_checkers(defect, pc, early, N, where):
    """Each defect at the last block row it can sit in (the ragged end) and, where it has a knot of its own, at an interior one."""
    last = N - 2 if defect == "transposed_block_left_out" else N - 1
    knot = last if where == "last" else N // 2
    r = next(x for x in pc_cases.ROWS32 if x.n == 14 and x.N == N and x.pc == pc)
    S, P, g, lam0 = (a[0] for a in pc_cases.host_matrices(r))
    Pss = pc_cases.host_matrices(r._replace(pc="ss"))[1][0]
    Ks = [K for K in pc_cases.ks(r, 0)[1] if K >= 2]
    steps_bad, first_bad = checker_verdicts(S, P, g, lam0, N, pc, Ks, defect=defect, knot=knot, Pss=Pss)
    print(defect, N, where, sorted(steps_bad), sorted(first_bad))
    assert steps_bad, "step_quantities passes the defect"
    if early:
        assert first_bad, "first_steps_quantities passes the defect"
