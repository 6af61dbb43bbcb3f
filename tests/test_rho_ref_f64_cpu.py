"""CPU: the double setting of the rho restatement tests/rho_ref.py (dtype = np.float64) pinned (a) to its float setting on sequences where float and double
arithmetic agree exactly — a dyadic factor and dyadic starts: every product and quotient is exact in both — and (b) to a hand-written list for the
reference's constants (include/pcg/sqp.cuh:304-320: factor 1.2, rho_min 1e-3, rho_max 10).  The decimal strings are the shortest that identify the
double (repr): equality is exact.  Also the exactly rounded fma the step restatement uses."""
from fractions import Fraction

import numpy as np

import rho_ref

f64 = np.float64


def test_dyadic_sequences_agree_with_the_float_restatement_exactly():
    """factor 2, rho_min 2^-10, rho_max 16, starts 2^-10, 0.5, 3: every value is a small dyadic number, exact in float and in double."""
    kw = dict(factor=2.0, rho_min=2.0 ** -10, rho_max=16.0, rho_reset=0.25)
    outcomes = [-1, -1, 0, 3, -1, 0, 0, 0, -1, -1, -1, -1, -1, -1]
    for rho0 in (2.0 ** -10, 0.5, 3.0):
        a, b = (rho0, 1.0), (rho0, 1.0)
        gave_up = False
        for p in outcomes:
            ra, da, xa = rho_ref.update(*a, p, **kw)
            rb, db, xb = rho_ref.update(*b, p, dtype=np.float64, **kw)
            assert ra.dtype == np.float32 and rb.dtype == f64
            assert (float(ra), float(da), xa) == (float(rb), float(db), xb), (rho0, p)
            a, b = (ra, da), (rb, db)
            if xa:
                gave_up = True
                break
        assert gave_up                                         # every start ends in a give-up: the failure path, the reset and the flag are all compared


def test_the_reference_constants_against_a_hand_written_list():
    """1.2, 1e-3, 10 from rho = 1e-3, drho = 1: fail, fail, success, then failures to the give-up.  Double arithmetic by hand:
    fail: drho 1.2, rho 1e-3 x 1.2; fail: drho 1.44, rho x 1.44; success: drho = min(1.44 / 1.2, 1 / 1.2) = 0.8333.., rho x that;
    then drho = 1.2 (max(0.8333 x 1.2, 1.2)), 1.44, 1.728, ... and rho x drho each time until the product exceeds 10."""
    seq = []
    rho, drho = 1e-3, 1.0
    for p in [-1, -1, 0] + [-1] * 12:
        rho, drho, done = rho_ref.update(rho, drho, p, dtype=np.float64)
        seq.append((repr(float(rho)), repr(float(drho)), done))
        if done:
            break
    want = [("0.0012", "1.2", False),
            ("0.001728", "1.44", False),
            ("0.00144", "0.8333333333333334", False),
            ("0.001728", "1.2", False),
            ("0.00248832", "1.44", False),
            ("0.00429981696", "1.728", False)]
    # the decimal strings above are what exact decimal arithmetic gives; a double product may differ from them in the last place, so the list is
    # checked to one unit in the last place and the rest of the walk against the rule restated with Fractions rounded once per operation
    for (r, d, x), (wr, wd, wx) in zip(seq, want):
        assert abs(float(r) - float(wr)) <= np.spacing(float(wr)) and abs(float(d) - float(wd)) <= np.spacing(float(wd)) and x == wx, (r, d, wr, wd)
    F = Fraction
    rho, drho = F(1e-3), F(1.0)
    f, lo, hi = F(1.2), F(1e-3), F(10.0)
    rnd = lambda q: F(float(q))                                # one rounding to double
    exact = []
    for p in [-1, -1, 0] + [-1] * 12:
        if p < 0:
            drho = max(rnd(drho * f), f)
            rho = max(rnd(rho * drho), lo)
            if rho > hi:
                exact.append((repr(1e-3), repr(float(drho)), True))
                break
        else:
            drho = min(rnd(drho / f), rnd(F(1) / f))
            rho = max(rnd(rho * drho), lo)
        exact.append((repr(float(rho)), repr(float(drho)), False))
    assert seq == exact
    # the walk: 2 failures, 1 success, then failures; rho = 1.44e-3 x 1.2^(k (k + 1) / 2) first exceeds 10 at k = 10 (1.2^55 = 2.26e4 -> 32.6)
    assert len(seq) == 13 and seq[-1][2] and not any(x for _, _, x in seq[:-1])
    assert seq[-1][0] == "0.001" and float(seq[-2][0]) < 10.0


def test_fma_is_rounded_once():
    """x + a d where the product needs more than 53 bits: the fused result differs from the two-rounding one."""
    a, d, x = 1.0 + 2.0 ** -30, np.array([1.0 + 2.0 ** -30]), np.array([-1.0])
    got = rho_ref.fma(a, d, x)[0]
    assert got == 2.0 ** -29 + 2.0 ** -60                      # exact: (1 + e)^2 - 1 = 2 e + e^2
    assert f64(a) * d[0] + x[0] == 2.0 ** -29                  # the separate product lost e^2
    nan = rho_ref.fma(-0.5, np.array([np.nan, 1.0]), np.array([1.0, 1.0]))
    assert np.isnan(nan[0]) and nan[1] == 0.5


def test_step_without_rho_is_the_plain_step():
    nan = float("nan")
    merit = np.array([[5, 6], [3, 2], [nan, nan]], f64)
    ref = np.full(3, 4.0)
    xu, dz = np.ones((3, 3)), np.full((3, 3), 2.0)
    got = rho_ref.step(merit, [-1.0, -0.3], ref, dz, xu, dtype=np.float64)
    assert got.tolist() == [-1, 1, -1] and ref.tolist() == [4.0, 2.0, 4.0]
    assert xu[1, 0] == float(Fraction(-0.3) * 2 + 1) and xu[0, 0] == 1.0
