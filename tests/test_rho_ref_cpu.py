"""CPU: the rho restatement tests/rho_ref.py pinned on sequences that follow from the reference's constants (include/pcg/sqp.cuh:304-320:
factor 1.2, rho_min 1e-3, rho_max 10) in float arithmetic.  The decimal strings are the shortest that identify the float: equality is exact."""
import numpy as np

import rho_ref

f32 = np.float32


def run(rho, drho, outcomes, **kw):
    """[(rho, drho, done)] after each line search; stops behind a give-up."""
    out = []
    for p in outcomes:
        rho, drho, done = rho_ref.update(rho, drho, p, **kw)
        out.append((rho, drho, done))
        if done:
            break
    return out


def test_failures_from_the_initial_rho_give_up_at_the_tenth():
    """drho grows 1.2, 1.44, ...; rho = 1e-3 x 1.2^(k (k + 1) / 2).  The tenth product, 22.644842, exceeds rho_max: reset and done."""
    seq = run(1e-3, 1.0, [-1] * 12)
    assert len(seq) == 10
    want = ["0.0012", "0.0017280001", "0.0029859846", "0.0061917384", "0.015407029", "0.04600515", "0.1648448", "0.70880264", "3.657267"]
    assert [r for r, _, _ in seq[:9]] == [f32(w) for w in want]
    assert not any(d for _, _, d in seq[:9])
    assert [d for _, d, _ in seq[:3]] == [f32("1.2"), f32("1.44"), f32("1.7280002")]
    # the product that exceeded rho_max, restated: rho_9 * drho_10
    assert f32(seq[8][0] * seq[9][1]) == f32("22.644842") and f32("22.644842") > f32(10.0)
    assert seq[9] == (f32(1e-3), f32("6.1917386"), True)


def test_failures_from_rho_5_give_up_at_the_third():
    seq = run(5.0, 1.0, [-1] * 5, rho_reset=0.25)
    assert [r for r, _, _ in seq[:2]] == [f32(6.0), f32("8.64")]
    assert f32(seq[1][0] * seq[2][1]) == f32("14.929922")
    assert len(seq) == 3 and seq[2] == (f32(0.25), f32("1.7280002"), True)          # the caller's rho_reset


def test_successes_shrink_rho_to_its_floor_and_drho_beyond():
    seq = run(1e-3, 1.0, [-1] * 4 + [0, 3, 7, 0, 0, 0])
    assert seq[3][:2] == (f32("0.0061917384"), f32("2.0736003"))
    assert [r for r, _, _ in seq[4:]] == [f32("0.005159782"), f32("0.0035831816"), f32("0.0020736002"), f32(1e-3), f32(1e-3), f32(1e-3)]
    # the first success caps drho at 1 / 1.2 (2.07 / 1.2 is above it); from there it keeps shrinking while rho stays clamped
    assert seq[4][1] == f32(f32(1.0) / f32(1.2)) == f32("0.8333333")
    d = [x for _, x, _ in seq[4:]]
    assert all(a > b for a, b in zip(d, d[1:])) and d[-1] == f32("0.3348979")
    assert not any(x for _, _, x in seq)


def test_an_alternating_trajectory_stays_bounded():
    seq = run(1e-3, 1.0, [-1, 0] * 10)
    assert all(r <= f32(0.0012) and not d for r, _, d in seq)
    assert seq[0][0] == f32("0.0012") and seq[1][:2] == (f32(1e-3), f32("0.8333333"))


def test_step_freezes_and_follows_the_selection_rule():
    """rho_ref.step: the selection of plant_ref.select (strict, first of equals, a NaN never wins), the update, and the freeze."""
    nan = float("nan")
    merit = np.array([[5, 6], [3, 2], [nan, nan], [1, 1]], f32)
    ref = np.full(4, 4.0, f32)
    xu, dz = np.ones((4, 3), f32), np.full((4, 3), 2.0, f32)
    rho, drho = np.full(4, 9.0, f32), np.ones(4, f32)
    done = np.array([0, 0, 0, 7], np.uint8)
    got = rho_ref.step(merit, [-1.0, -0.5], ref, dz, xu, rho, drho, done, rho_reset=0.5)
    assert got.tolist() == [-1, 1, -1, rho_ref.STEP_FROZEN]
    assert ref.tolist() == [4.0, 2.0, 4.0, 4.0]
    assert xu[:, 0].tolist() == [1.0, 0.0, 1.0, 1.0]
    assert rho.tolist() == [0.5, 7.5, 0.5, 9.0] and done.tolist() == [1, 0, 1, 7]          # 9 x 1.2 > 10: given up; 9 / 1.2 = 7.5
    assert drho.tolist() == [f32(1.2), f32("0.8333333"), f32(1.2), 1.0]
