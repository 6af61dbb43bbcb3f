"""CPU: the merit restatement of tests/plant_ref.py pinned on REFERENCE-HELD data.  The reference's precomputed trajectory
(tests/golden/iiwa_traj_0_0_full.npz = examples/trajfiles/0_0_traj.csv + 0_0_eepos.traj) was integrated by its own forward dynamics and its
end-effector rows by its own kinematics: inside a segment every integrator defect and every tracking error vanishes to the print precision of the
files, so with goals = the file's own end-effector rows, qd_cost = r_cost = 0, mu = 1 and xs = x_0 the merit of a window IS that residue."""
import pytest

import iiwa_ref
import plant_ref as P


@pytest.mark.parametrize("t0,N", P.WINDOWS)
def test_merit_vanishes_on_the_reference_trajectory(t0, N):
    """Bound: 14 (N - 1) defects of at most 1e-6 each — the 3e-7 print precision of the csv (tests/test_iiwa_plant.py) times three for the float32
    rounding of the inputs; the cost term is the square of a 3e-6 tracking error.  Measured 1.4e-5 .. 5.0e-5 against 4.3e-4 / 8.8e-4."""
    good = set(iiwa_ref.in_segment_transitions())
    assert all(t in good for t in range(t0, t0 + N - 1))
    xu, goals, xs = P.reference_window(t0, N)
    got = P.merit_at(iiwa_ref.Model(), P.trial(xu, None, 0.0), P.f32(goals), P.f32(xs), N, 1.0, cost=P.Cost.plain(0.0, 0.0))
    print(f"rows {t0}..{t0 + N - 1}: merit {got:.3e}, bound {14 * (N - 1) * 1e-6:.3e}")
    assert 0.0 <= got <= 14 * (N - 1) * 1e-6, got


def test_select_is_the_references_rule():
    assert P.select([3.0, 2.0, 2.0, 5.0], 4.0) == (1, 2.0)          # the first of equals
    assert P.select([4.0, 5.0], 4.0) == (-1, 4.0)                  # equal to merit_ref: no step
    assert P.select([float("nan"), 3.0], 4.0) == (1, 3.0)          # a NaN never wins
