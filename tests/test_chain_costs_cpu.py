"""CPU: the conditions under which tests/test_gpu_chain_costs.py means anything (tests/chain_cost_cases.py).  The cases are valid — every side of every
kind of limit occurs, no value on or near a bound, offsets at both clamps, the simulate times what they claim; the restatement's cost path on a random
chain is consistent with itself — the central differences of its merit are its KKT gradient; a single wrong table entry moves the restated COST = 2 KKT
arrays and merits by more than 1e-3, a hundred and more times the limits the kernels are held to; and the restatements are cheap enough to share."""
import time

import numpy as np
import pytest

import chain_cost_cases as K
import chain_models as cm
import clock_ref
import plant_ref as P

n, m, NJ, ROW = K.n, K.m, K.NJ, K.ROW


# ---- 1. the cases are valid ----
@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("seed,N,B", K.CASES)
def test_limits_have_every_side_and_no_value_on_a_bound(seed, N, B, double):
    """Below, inside and above occur for q, qd and u, at the iterate (the KKT's limits) and over the trial iterates (the merit's); no value equals a bound —
    under the double perturbation of 1e-12 too, where the bounds stay floats halfway between two neighbours."""
    cs, modest = K.case(seed, N, B, "large", double), K.case(seed, N, B, "modest", double)          # (the modest set: the difference route's KKT alone)
    for cs, steps, lim in ((cs, [0.0], cs.kkt_limits), (cs, K.STEPS3, cs.merit_limits), (modest, [0.0], modest.kkt_limits)):
        xs, us = cs.states_controls(steps)
        x, u = np.concatenate(xs), np.concatenate(us)
        for name, vals, lo, hi in (("q", x[:, :NJ], lim.q_lo, lim.q_hi), ("qd", x[:, NJ:], lim.qd_lo, lim.qd_hi), ("u", u, lim.u_lo, lim.u_hi)):
            s = P.side(vals, lo, hi)
            gap = min(np.abs(vals - lo).min(), np.abs(vals - hi).min())
            print(f"seed {seed} ({N}, {B}) {cs.size} {'double' if double else 'float'} {name} x{len(steps)}: below {(s < 0).sum()} inside {(s == 0).sum()} above {(s > 0).sum()}, nearest bound {gap:.1e}")
            assert all((s == v).any() for v in (-1, 0, 1)), name
            assert gap > 1e-9                                  # a thousand times the double perturbation: the side is the float case's
            assert np.array_equal(np.float32(lo).astype(np.float64), lo) and np.array_equal(np.float32(hi).astype(np.float64), hi)
        assert lim.q_lo[1] == lim.qd_lo[1] == lim.u_lo[1] == -np.inf


def test_far_limits_keep_every_value_further_than_two_steps_from_a_bound():
    """Test d of the GPU file: with every value further than 2 h from every bound no perturbed copy crosses a kink, and every side still occurs."""
    cs, lim = K.case(1, 3, 5, "large", True), K.far_limits()
    xs, us = cs.states_controls([0.0])
    x, u = np.concatenate(xs), np.concatenate(us)
    for vals, lo, hi in ((x[:, :NJ], lim.q_lo, lim.q_hi), (x[:, NJ:], lim.qd_lo, lim.qd_hi), (u, lim.u_lo, lim.u_hi)):
        assert min(np.abs(vals - lo).min(), np.abs(vals - hi).min()) > 2 * K.H
        s = P.side(vals, lo, hi)
        assert all((s == v).any() for v in (-1, 0, 1))


@pytest.mark.parametrize("seed,N,B", K.CASES)
def test_plans_and_offsets(seed, N, B):
    """Offsets hit both clamps and an inside row wherever the batch has three trajectories; (3, 5) has a plan per trajectory with NaN rows between the plans,
    and no reference row is one of them."""
    cs = K.case(seed, N, B)
    T = cs.T
    assert (cs.stride == T + 2) == ((N, B) == (3, 5)) and cs.plan.shape == ((B * cs.stride) if cs.stride else T, ROW)
    idx = [[P.row_index(cs.offsets[b], k, T) for k in range(N)] for b in range(B)]
    assert idx[0][0] == 0 and cs.offsets[0] + 0 < 0                                            # clamped at the first row
    if B >= 3:
        assert cs.offsets[1] + N - 1 > T - 1 and idx[1][-1] == T - 1                              # clamped at the last row
        assert all(0 <= cs.offsets[2] + k <= T - 1 for k in range(N))                             # inside
    for b in range(B):
        assert np.isfinite(cs.rows(b)).all() and np.array_equal(cs.rows(b), cs.own_plan(b)[idx[b]])
    if cs.stride:
        assert np.isnan(cs.plan).sum() == 2 * B * ROW and not np.array_equal(cs.own_plan(0), cs.own_plan(1))
    assert K.COSTS["joint"].ee_cost == 0.0 and K.COSTS["all"].ee_cost > 0 and all(c.q_cost > 0 for c in K.COSTS.values())


@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
def test_simulate_cases_are_what_they_claim(double):
    """The times of the clocked test: a zero time (no substep, no remainder), a knot crossing with a remainder, a remainder alone among full substeps; the
    torque limits clamp a control of every trajectory in the knots the crossing schedule applies, and the clamped controls stay inside the bounds."""
    dtype = np.float64 if double else np.float32
    ss = 2e-4 if double else float(np.float32(2e-4))
    zero, crossing = K.TIMES[0], K.CROSSING
    assert clock_ref.schedule(*zero, ss, dtype)[2:] == (0, 0.0) and K.TIMES[K.FROZEN] == crossing and crossing in K.TIMES[:K.FROZEN]
    S, idx, rem, rem_idx = P.schedule(*crossing, K.DT, ss, double)
    assert sorted(set(idx)) == [0, 1] and rem != 0 and rem_idx == 1
    assert any(P.schedule(t, s, K.DT, ss, double)[2] != 0 and P.schedule(t, s, K.DT, ss, double)[0] > 0 for t, s in K.TIMES)
    assert all(clock_ref.schedule(t, s, ss, dtype)[0] for t, s in K.TIMES)
    for B in (3, 5):
        sc = K.sim_case(B, double)
        lo, hi = sc.limits.u_lo, sc.limits.u_hi
        for b in range(B):
            for arr, inside in ((sc.xu, False), (sc.clamped, True)):
                u = P.split(arr[b], K.N4)[1][:2]
                assert ((u >= lo) & (u <= hi)).all() == inside
        assert not (np.concatenate([P.split(z, K.N4)[1] for z in sc.xu]) == lo).any()


# ---- 2. the restatement's cost path on a chain is consistent with itself ----
def differences(mdl, z, goals, N, rows, cost, limits, h):
    L = len(z)
    e = np.eye(L)
    f = lambda v: P.merit_at(mdl, v, goals, None, N, 0.0, cost=cost, rows=rows, limits=limits, dt=K.DT)
    return np.array([(f(z + h * e[i]) - f(z - h * e[i])) / (2 * h) for i in range(L)])


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_merit_differences_are_the_kkt_gradient_on_a_chain(seed):
    """Cost "joint" (no end-effector term: the cost sum is piecewise quadratic), mu = 0: the central differences (h = 1e-3) of plant_ref.merit_at equal g of
    plant_ref.generate_kkt to 1e-9 max(1, |g|), without limits and with bounds further than 2 h from every value.  (The defects are still evaluated — mu = 0
    multiplies them — so a chain whose dynamics went non-finite would show.)"""
    cs, co = K.case(seed, 3, 5, "large", True), K.COSTS["joint"]
    xs, us = cs.states_controls([0.0])
    x, u = np.concatenate(xs), np.concatenate(us)
    far = P.Limits(*K.far_bounds(x[:, :NJ]), *K.far_bounds(x[:, NJ:]), *K.far_bounds(u), *K.WEIGHTS)
    zero = (np.zeros(0), np.zeros(ROW * cs.N - m), np.zeros(0))
    for lim in (None, far):
        worst = 0.0
        for b in range(cs.B):
            g = P.generate_kkt(K.chain(seed), cs.xu[b], None, cs.xs[b], cs.N, rows=cs.rows(b), cost=co, limits=lim, dt=K.DT, base=zero)[2]
            num = differences(K.chain(seed), cs.xu[b], None, cs.N, cs.rows(b), co, lim, K.H)
            worst = max(worst, np.abs(num - g).max() / max(1.0, np.abs(g).max()))
        print(f"seed {seed} joint cost, {'far limits' if lim else 'no limits'}: central differences off by {worst:.2e}")
        assert worst <= 1e-9, worst


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_merit_differences_with_the_end_effector_term(seed):
    """Cost "all": the end-effector term is not quadratic, so the differences carry their own truncation error h^2 |f'''| / 6, printed at h and 2 h; a
    second-order scheme loses a factor of four from one to the other, which is what is asserted (between 3 and 5), and that the figure at h is below 1e-5 of
    max(1, |g|).  Knots 0 .. N - 2 only: the last block's end-effector part is the pose of x_{N-2} against goal_{N-1} (tests/plant_ref.py, KKT), which no merit
    differentiates."""
    cs, co = K.case(seed, 3, 5, "large", True), K.COSTS["all"]
    keep = ROW * (cs.N - 1)
    err = {}
    for h in (K.H, 2 * K.H):
        worst = 0.0
        for b in range(2):
            g = cs.want_kkt(b, "all")[2]
            num = differences(K.chain(seed), cs.xu[b], cs.goals[b], cs.N, cs.rows(b), co, None, h)
            worst = max(worst, np.abs(num - g)[:keep].max() / max(1.0, np.abs(g).max()))
        err[h] = worst
    print(f"seed {seed} cost all: central differences off by {err[K.H]:.2e} at h = 1e-3, {err[2 * K.H]:.2e} at 2 h (ratio {err[2 * K.H] / err[K.H]:.2f})")
    assert err[K.H] <= 1e-5 and 3.0 <= err[2 * K.H] / err[K.H] <= 5.0, err


# ---- 3. a single wrong table entry is visible through the COST = 2 restatements ----
def rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_a_single_wrong_table_entry_moves_the_cost_2_restatements(seed):
    """(3, 5), "large", cost "all" with the case's limits, both integrators: every entry of chain_models.CORRUPTIONS moves the worst KKT array by more than 1e-3
    of max(1, |array|) and some merit by more than 1e-3 of max(1, |merit|).  Measured, worst array (always C): 0.49 .. 2.3; G and g move only under the two
    kinematic corruptions."""
    cs, co = K.case(seed, 3, 5), K.COSTS["all"]
    for integrator in (0, 1):
        good = [cs.want_kkt(b, "all", integrator, limits=True) for b in range(cs.B)]
        good_merit = cs.want_merits("all", True, integrator, limits=True)
        for name, corrupt in cm.CORRUPTIONS.items():
            bad = corrupt(K.chain(seed))
            moved = [P.generate_kkt(bad, cs.xu[b], cs.goals[b], cs.xs[b], cs.N, rows=cs.rows(b), cost=co, limits=cs.kkt_limits, dt=K.DT, integrator=integrator)
                     for b in range(cs.B)]
            moves = [max(rel(moved[b][i], good[b][i]) for b in range(cs.B)) for i in range(4)]
            bad_merit = P.merits(bad, cs.xu, cs.dz, K.STEPS3, cs.goals, cs.xs, cs.N, K.MU, rows_of=cs.rows, cost=co, limits=cs.merit_limits, dt=K.DT, integrator=integrator)
            merit_move = float((np.abs(bad_merit - good_merit) / np.maximum(1.0, np.abs(good_merit))).max())
            print(f"seed {seed} integrator {integrator}: {name:26s} G {moves[0]:.1e}  C {moves[1]:.1e}  g {moves[2]:.1e}  c {moves[3]:.1e}  merit {merit_move:.1e}")
            assert max(moves) > 1e-3, (name, moves)
            assert merit_move > 1e-3, (name, merit_move)
            if name in ("link-offset x dropped", "one ET_k transposed"):
                assert moves[0] > 1e-3 and moves[2] > 1e-3, (name, moves)
            else:
                assert moves[0] == 0.0 and moves[2] == 0.0, (name, moves)


# ---- 4. the restatements are cheap enough to share ----
def test_the_restatements_of_one_seed_and_shape_are_quick():
    """Everything tests/test_gpu_chain_costs.py asks of the restatement for one seed at (3, 5): KKT in float and double on the large set, and on the modest set
    for the difference route, both integrators, both costs, with and without limits; the merits likewise.  Under 30 s, loosely: measured 3 s."""
    start = time.perf_counter()
    for size, double in (("large", False), ("large", True), ("modest", False), ("modest", True)):
        cs = K.ChainCase(3, 3, 5, size, double)                # (not the cached case: nothing of it has been computed yet)
        for integrator in (0, 1):
            for cost in K.COSTS:
                for limits in (False, True):
                    for b in range(cs.B):
                        cs.want_kkt(b, cost, integrator, limits)
                    if size == "large":
                        for with_xs in (True, False):
                            cs.want_merits(cost, with_xs, integrator, limits)
    took = time.perf_counter() - start
    print(f"restatements of one seed at (3, 5): {took:.1f} s")
    assert took < 30.0

