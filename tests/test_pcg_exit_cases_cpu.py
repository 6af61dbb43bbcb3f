"""CPU: the tolerance-exit cases (tests/pcg_exit_cases.py) hold without a GPU.

  * The reference alone meets every exact count: the oracle's PCG in the row's own precision, on every row, ladder and trajectory, on the same
    inputs and on three copies perturbed by one ulp (float: util.fp32_band's perturbation of S and gamma; double: 1e-16 relative), under both
    caps — exactly the predicted iteration count and exit flag.  A prediction the sequential reference misses under rounding-level noise would
    say nothing about a kernel.
  * The ladders have what they are for: distinct counts, a 0 exit, a deep exit, the zero-gamma entry, the entry that never crosses.
  * The assertions of tests/test_gpu_exit.py see what they are for: a numpy float32 restatement of the loop passes them; with ONE planted defect
    of the exit path it fails."""
import numpy as np
import pytest

import pcg_exit_cases as ec
import pcg_step_cases as sc

f32 = np.float32
LADDERS = [(r, warm) for r in ec.ALL_ROWS for warm in (False, True)]
ladder_id = lambda c: f"{ec.row_id(c[0])}-{c[0].prec}-{'warm' if c[1] else 'cold'}"


@pytest.mark.parametrize("case", LADDERS, ids=ladder_id)
def test_the_reference_alone_meets_every_exact_count(orc, case):
    r, warm = case
    lad = ec.ladder(r, warm)
    ec.check_structure(lad, *ec.need(r))
    Sh, Ph = ec.host(r)
    dt = ec.DTYPE[r.prec]
    rel = 6e-8 if dt == f32 else 1e-16
    rng = np.random.default_rng(r.N + 1000 * int(warm))
    for trial in range(4):
        for b in range(len(lad.pred)):
            S, g = (Sh, lad.gamma[b]) if trial == 0 else (ec.perturbed(Sh, rel, rng, dt), ec.perturbed(lad.gamma[b], rel, rng, dt))
            for cap in (lad.cap_hi, lad.cap_mid):
                o = ec.run_oracle(r, g, lad.lam0[b], cap, lad.tol, S=S, P=Ph)
                want = tuple(int(v[b]) for v in ec.predicted(lad, cap))
                assert (o["iters"], int(o["max_iter_exit"])) == want, (trial, b, lad.kinds[b], cap, o["iters"], o["max_iter_exit"], want)
                assert np.isfinite(o["lam"]).all()
                if want[0] == 0:
                    assert o["lam"].tobytes() == lad.lam0[b].tobytes()
    print(f"{ladder_id(case)}: exit_tol {lad.tol:.3g} counts {lad.pred[:-1]} caps {lad.cap_mid}, {lad.cap_hi}")


def test_the_rows_cover_every_build_of_the_launch_plan():
    """Every family the launch plan can return, in both precisions, at every workgroup width the step table pins, under both preconditioners;
    the 128-knot builds of the lane-pair and lane-quad kernels; the generic kernel's branch points; the fp16-storage cases."""
    fam = lambda rows: {(r.prec, r.family) for r in rows}
    assert fam(ec.ROWS) == fam(sc.ROWS)
    build = lambda rows: {(r.prec, r.family, r.waves, r.opts, r.pc) for r in rows if r.n == 14}
    assert build(ec.ROWS) == build(sc.ROWS)
    assert {(r.prec, r.n, r.m, r.N, r.pc) for r in ec.ROWS if r.n != 14} == {(r.prec, r.n, r.m, r.N, r.pc) for r in sc.ROWS if r.n != 14}
    assert set(ec.ROWS) <= set(sc.ROWS) and len(set(ec.ROWS)) == len(ec.ROWS)
    for family in (6, 11):
        assert {r.N for r in ec.ROWS32 if r.family == family and r.waves == 8} == {65}
    assert len(ec.F16_ROWS) == 2 * len(sc.F16_CASES)
    for r in sc.ROWS:                                       # a row left for a larger horizon of its build: only where no ladder fits its system
        twin = next(x for x in ec.ROWS if (ec._key(x), x.pc) == (ec._key(r), r.pc))
        assert twin.N == r.N or twin.N > r.N and ec.too_fast(r) or twin.N < r.N
    assert {(r.prec, r.n, r.N, r.pc) for r in ec.ROWS if ec.too_fast(r)} == set(ec.SHALLOW)


@pytest.mark.parametrize("r", [r for r in sc.ROWS if ec.too_fast(r) and r.prec == "f32" and r.family in (5, 3)][:3], ids=sc.row_id)
def test_a_too_fast_system_has_no_crossing_at_four(r):
    """What too_fast says, on the systems themselves: below DEPTH by the fourth iteration, cold and warm."""
    g, lam0 = ec.base(r)[2:]
    for l0 in (np.zeros_like(lam0), lam0):
        h = ec._hist(r, g, l0)
        assert not h[4] >= ec.DEPTH * h[0], h[:6] / h[0]


# ---- the assertions see what they are for --------------------------------------------------------------------------------------------------------------

def host_exit_pcg(S, P, g, lam0, N, n, pc, cap, tol, defect=None):
    """Textbook PCG with the reference's exit rules (oracle/mpcg_oracle_impl.inc) in float32 numpy on the bd layout:
    (lambda, r, p, iters, flag).  `defect`: one slip of the exit path (DEFECTS)."""
    Sb = np.array(S, f32).reshape(N, 3, n, n).transpose(0, 1, 3, 2).copy()
    Pb = np.array(P, f32).reshape(N, 3, n, n).transpose(0, 1, 3, 2).copy()

    def mv(Mb, x, cols):
        X = x.reshape(N, n)
        y = np.einsum("kij,kj->ki", Mb[:, 1], X)
        if cols == 3:
            y[1:] += np.einsum("kij,kj->ki", Mb[1:, 0], X[:-1])
            y[:-1] += np.einsum("kij,kj->ki", Mb[:-1, 2], X[1:])
        return y.reshape(-1).astype(f32)

    dot = lambda a, b: (a * b).reshape(N, n).sum(axis=1, dtype=f32).sum(dtype=f32)
    pcols = 3 if pc == "ss" else 1
    g, lam, tol = np.asarray(g, f32), np.array(lam0, f32), f32(tol)
    r = g - mv(Sb, lam, 3)
    z = mv(Pb, r, pcols)
    p = z.copy()
    eta = dot(r, z)
    iters, flag = 0, 1
    if abs(eta) < tol:
        return lam, (g.copy() if defect == "r_is_gamma_at_a_zero_iteration_exit" else r), p, 0, 0
    tested = eta
    with np.errstate(all="ignore"):                        # (gamma = 0 at exit_tol = 0 is 0 / 0 by construction; its lambda is never compared)
        for it in range(cap):
            cap_first = defect == "cap_before_tolerance" and it == cap - 1
            ups = mv(Sb, p, 3)
            alpha = f32(eta / dot(p, ups))
            lam = lam + alpha * p
            r = r - alpha * ups
            z = mv(Pb, r, pcols)
            eta_new = dot(r, z)
            iters = it if defect == "iters_is_it" else it + 1
            crossed = abs(tested if defect == "exit_test_on_the_old_eta" else eta_new) < tol
            tested = eta_new
            if crossed and not cap_first:
                flag = 0
                if defect == "lambda_updated_once_more":
                    lam = lam + alpha * p
                if defect == "p_updated_on_a_tolerance_exit":
                    p = z + f32(eta_new / eta) * p
                break
            p = z + f32(eta_new / eta) * p
            eta = eta_new
    return lam, r, p, iters, flag


DEFECTS = ["iters_is_it", "exit_test_on_the_old_eta", "lambda_updated_once_more", "cap_before_tolerance",
           "r_is_gamma_at_a_zero_iteration_exit", "p_updated_on_a_tolerance_exit"]
DEFECT_ROWS = [r for r in ec.ROWS32 if r.n == 14 and r.N == 17 and r.family == 5 and r.waves == 4]


def gpu_test_assertions(r, warm, defect):
    """What tests/test_gpu_exit.py asserts of a batched entry and of the 12-argument entry, with host_exit_pcg in the kernel's place."""
    lad = ec.ladder(r, warm)
    Sh, Ph = ec.host(r)
    B = len(lad.pred)
    run = lambda b, cap, tol, d=defect: host_exit_pcg(Sh, Ph, lad.gamma[b], lad.lam0[b], r.N, r.n, r.pc, cap, tol, d)
    fixed = {k: [run(b, k, 0.0)[0] for b in range(B)] for k in ec.distinct_counts(lad)}
    for cap in (lad.cap_hi, lad.cap_mid):
        out = [run(b, cap, lad.tol) for b in range(B)]
        ec.check_counts(defect, lad, cap, [o[3] for o in out], [o[4] for o in out])
        ec.check_lambda_bits(defect, lad, cap, [o[0] for o in out], fixed)
    for b, cap in ec.state_trajectories(lad):
        ref, tols = ec.state_reference(r, lad, b, cap)
        lam, res, p, iters, flag = run(b, cap, lad.tol)
        assert (iters, flag) == (ref["iters"], int(ref["max_iter_exit"]))
        ec.check_state(defect, ref, tols, lam, res, p)


@pytest.mark.parametrize("r", DEFECT_ROWS, ids=ec.row_id)
def test_the_restatement_passes_the_assertions_of_the_gpu_test(orc, r):
    for warm in (False, True):
        gpu_test_assertions(r, warm, None)


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("r", DEFECT_ROWS, ids=ec.row_id)
def test_one_planted_defect_fails_them(orc, r, defect):
    """The warm ladder: the one the 12-argument checks read."""
    with pytest.raises(AssertionError):
        gpu_test_assertions(r, True, defect)
