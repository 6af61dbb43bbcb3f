"""CPU: the non-iiwa robots of tests/chain_models.py — what tests/test_gpu_chain_plants.py checks the plant kernels against.  The geometric model
reproduces the iiwa restatement exactly, the exported tables are the geometry, the random chains are physical, no worse conditioned than the iiwa
(so the limits the kernels are held to on the iiwa carry over), the restatement's own difference noise lies far below those limits, and — the point —
a single wrong table entry moves the restatement's KKT blocks by more than 1e-3 on every random chain, where the iiwa hardly notices."""
import functools

import numpy as np
import pytest

import chain_models as cm
import iiwa_ref
from mpcgpu_amd import iiwa

NJ, n, m = cm.NJ, cm.n, cm.m
Q_GENERIC = np.array([0.3, -0.7, 1.1, 0.5, -1.3, 0.9, 0.2]) * 2.3


@functools.lru_cache(maxsize=None)
def chain(seed):
    return cm.random_chain(seed)


def test_iiwa_from_geometry_is_the_iiwa_restatement():
    """Measured difference: 0.0 exactly (the iiwa's rotations are signed permutations: every product is exact)."""
    M, ch = iiwa_ref.Model(), cm.Chain.from_iiwa()
    for q in (Q_GENERIC, -1.7 * Q_GENERIC, np.zeros(NJ)):
        dX, dH = np.abs(ch.X(q) - M.X(q)).max(), np.abs(ch.Xhom(q) - M.Xhom(q)).max()
        print(f"iiwa from geometry: |dX| {dX:.1e} |dXhom| {dH:.1e}")
        assert dX <= 1e-15 and dH <= 1e-15


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_tables_are_the_geometry(seed):
    """Measured: 5.6e-17 in X (one rounding of -(E skew(p)) against the sum of the two rounded table terms), 0.0 in Xhom."""
    ch = chain(seed)
    t = cm.tables(ch)
    for q in (Q_GENERIC, -1.7 * Q_GENERIC):
        X, H = cm.eval_tables(t.X_const, t.X_trig, t.Xhom_const, t.Xhom_trig, q)
        dX, dH = np.abs(X - ch.X(q)).max(), np.abs(H - ch.Xhom(q)).max()
        print(f"seed {seed}: tables against geometry |dX| {dX:.1e} |dXhom| {dH:.1e}")
        assert dX <= 1e-15 and dH <= 1e-15
    assert np.array_equal(t.I, ch.I)
    # the format: every index of rows 0 / 1 carries exactly one sine and one cosine entry of its own joint
    for trig, per in ((t.X_trig, 36), (t.Xhom_trig, 16)):
        kinds = {}
        for i, _, j in trig:
            assert j % NJ == i // per
            kinds.setdefault(i, []).append(j // NJ)
        assert all(sorted(v) == [0, 1] for v in kinds.values())
    assert len(t.X_trig) == NJ * 24 and len(t.Xhom_trig) == NJ * 12


def test_tables_of_the_iiwa_from_geometry_are_the_committed_tables():
    """Evaluated, both table sets give the same transforms bit for bit, and the constants outside the trig indices are the committed ones."""
    M = iiwa.Model()
    t = cm.tables(cm.Chain.from_iiwa())
    for q in (Q_GENERIC, -1.7 * Q_GENERIC, np.zeros(NJ)):
        mine = cm.eval_tables(t.X_const, t.X_trig, t.Xhom_const, t.Xhom_trig, q)
        theirs = cm.eval_tables(M.X_const, M.X_trig, M.Xhom_const, M.Xhom_trig, q)
        assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
    assert np.array_equal(t.I, M.I)
    for mine, theirs, trig in ((t.X_const, M.X_const, M.X_trig), (t.Xhom_const, M.Xhom_const, M.Xhom_trig)):
        keep = np.ones(theirs.size, bool)
        keep[[i for i, _, _ in trig]] = False
        assert np.array_equal(mine.reshape(-1)[keep], theirs.reshape(-1)[keep])
    # and the committed trig entries are among the exported ones (the exported set also lists the entries whose coefficient is 0 on the iiwa)
    for theirs, mine in ((M.X_trig, t.X_trig), (M.Xhom_trig, t.Xhom_trig)):
        assert set(theirs) <= set(mine)
        assert all(c == 0.0 for e in set(mine) - set(theirs) for c in (e[1],))


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_random_chain_is_what_it_says(seed):
    """Nothing in the tables sits below the tolerances of the GPU tests."""
    ch = chain(seed)
    assert np.abs(ch.ET).min() > 0.02 and np.abs(ch.BT()).min() > 0.02
    for k in range(NJ):
        assert abs(np.linalg.det(ch.ET[k]) - 1.0) < 1e-12 and np.abs(ch.ET[k] @ ch.ET[k].T - np.eye(3)).max() < 1e-12
        assert (0.08 <= np.abs(ch.p[k])).all() and (np.abs(ch.p[k]) <= 0.25).all()
        I = ch.I[k]
        mass = I[3, 3]
        h = np.array([I[2, 4], I[0, 5], I[1, 3]])
        assert 1.0 <= mass <= 6.0 and (np.abs(h) > 1e-2).all() and (np.abs(h / mass) <= 0.1).all()
        assert min(abs(I[0, 1]), abs(I[0, 2]), abs(I[1, 2])) > 1e-3
        pr = np.linalg.eigvalsh(I[:3, :3] - mass * ((h / mass) @ (h / mass) * np.eye(3) - np.outer(h / mass, h / mass)))
        assert pr.min() > 0.005 - 1e-12 and pr.max() < 0.05 + 1e-12 and 2 * pr.max() < pr.sum()
    assert not any(np.array_equal(ch.ET, chain(s).ET) for s in cm.SEEDS if s != seed)


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_physical_identities(seed):
    ch = chain(seed)
    for q, qd, u in cm.states(4, 50 + seed):
        M = ch.mass_matrix(q)
        assert np.linalg.eigvalsh(M).min() > 0
        raw = np.array([ch.rnea(q, np.zeros(NJ), e) for e in np.eye(NJ)]).T
        assert np.abs(raw - raw.T).max() < 1e-12 * np.abs(raw).max()         # symmetric before mass_matrix symmetrises it
        qdd = np.linalg.solve(M, u - ch.rnea(q, qd, np.zeros(NJ)))
        assert np.abs(ch.rnea(q, qd, qdd) - u).max() < 1e-8
        J = ch.ee_jac(q)
        for d in np.eye(NJ):                                                 # ee_jac is the derivative of ee_pos (a different step and scheme)
            fd = (8 * (ch.ee_pos(q + 1e-3 * d) - ch.ee_pos(q - 1e-3 * d)) - (ch.ee_pos(q + 2e-3 * d) - ch.ee_pos(q - 2e-3 * d))) / 12e-3
            assert np.abs(J @ d - fd).max() < 1e-8


@functools.lru_cache(maxsize=None)
def iiwa_condition():
    """cond(M(q)) of the iiwa over the states the suite's KKT tests use (the windows of tests/test_gpu_kkt.py at N = 32)."""
    M = iiwa_ref.Model()
    xu, _, _ = iiwa.random_windows(32, 5, 11 + 32)
    conds = [np.linalg.cond(M.mass_matrix(w[k * (n + m):k * (n + m) + NJ])) for w in xu for k in range(0, 32, 4)]
    return min(conds), max(conds)


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_conditioning_is_no_worse_than_the_iiwas(seed):
    """The condition under which the limits held on the iiwa carry over: the kernels invert M explicitly.  Measured: 70 .. 563, 39 .. 387, 46 .. 837 for the three chains against 1178 .. 1583 for the iiwa
    on the windows of tests/test_gpu_kkt.py."""
    ch = chain(seed)
    conds = [np.linalg.cond(ch.mass_matrix(q)) for q, _, _ in cm.states(40, 60 + seed)]
    lo, hi = iiwa_condition()
    print(f"seed {seed}: cond(M) {min(conds):.0f} .. {max(conds):.0f}; iiwa {lo:.0f} .. {hi:.0f}")
    assert max(conds) < hi


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_restatement_noise_is_below_a_tenth_of_the_tightest_limit(seed):
    """The restatement differentiates the inverse dynamics by central differences: its dqdd Jacobians at h = 1e-6 against h = 2e-6, scaled by dt and by
    max(1, |block|) as the C array is, on the large set.  Limit 1e-7: a tenth of the 1e-6 the double builds are held to.  Measured: 1.3e-9, 2.2e-9, 2.0e-9."""
    ch = chain(seed)
    worst = 0.0
    for q, qd, u in cm.states(6, 70 + seed):
        a, b = ch.forward_dynamics_and_gradient(q, qd, u, h=1e-6), ch.forward_dynamics_and_gradient(q, qd, u, h=2e-6)
        for x, y in zip(a[1:3], b[1:3]):
            worst = max(worst, iiwa_ref.TIMESTEP * np.abs(x - y).max() / max(1.0, iiwa_ref.TIMESTEP * np.abs(x).max()))
    print(f"seed {seed}: central-difference noise of dt dqdd/d(q, qd) {worst:.1e}")
    assert worst <= 1e-7


class CoarserDifferences(cm.Chain):
    """The same chain with every central difference of the restatement at twice the step."""

    def ee_jac(self, q, h=2e-6):
        return super().ee_jac(q, h)

    def forward_dynamics_and_gradient(self, q, qd, u, h=2e-6):
        return super().forward_dynamics_and_gradient(q, qd, u, h)


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_restatement_noise_of_the_cost_arrays(seed):
    """G = blkdiag(g g^T, ..) and g = J^T (ee - goal) take J from central differences of ee_pos: the restatement at h = 1e-6 against h = 2e-6 on the
    inputs the GPU tests use (both sets, every shape), relative to max(1, |array|).  The double entry's limit for these two arrays on these chains is
    ten times the worst figure (chain_models.KKT_F64_LIMIT_Gg) and must stay below the 2e-7 rounding of a float store, which that entry exists to
    remove.  c carries no derivative: its figure is 0."""
    ch = chain(seed)
    coarse = CoarserDifferences(ch.ET, ch.p, ch.I)
    worst = [0.0] * 4
    for size in cm.SETS:
        for N, B in cm.SHAPES:
            xu, goals, xs = cm.hard_inputs(N, B, cm.input_seed(seed), size)
            for b in range(B):
                fine, other = (iiwa_ref.generate_kkt(c, xu[b], goals[b], xs[b], N) for c in (ch, coarse))
                worst = [max(w, np.abs(x - y).max() / max(1.0, np.abs(x).max())) for w, x, y in zip(worst, fine, other)]
    print(f"seed {seed}: restatement at h against 2h: G {worst[0]:.2e}  C {worst[1]:.2e}  g {worst[2]:.2e}  c {worst[3]:.2e}")
    assert worst[3] == 0.0
    assert max(worst[0], worst[2]) <= cm.KKT_F64_LIMIT_Gg / 5 and cm.KKT_F64_LIMIT_Gg < 2e-7
    assert worst[1] <= 1e-7


@functools.lru_cache(maxsize=None)
def sensitivity(which):
    """Per corruption: the four relative moves of G, C, g, c (max over the trajectories of the large set at N = 2, B = 2)."""
    ch = cm.Chain.from_iiwa() if which == "iiwa" else chain(which)
    xu, goals, xs = cm.hard_inputs(2, 2, 80, "large")
    base = [iiwa_ref.generate_kkt(ch, xu[b], goals[b], xs[b], 2) for b in range(2)]
    out = {}
    for name, corrupt in cm.CORRUPTIONS.items():
        bad = corrupt(ch)
        moved = [iiwa_ref.generate_kkt(bad, xu[b], goals[b], xs[b], 2) for b in range(2)]
        out[name] = [max(np.abs(x[i] - y[i]).max() / max(1.0, np.abs(x[i]).max()) for x, y in zip(base, moved)) for i in range(4)]
    return out


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_a_single_wrong_table_entry_is_visible_on_a_random_chain(seed):
    """What makes the GPU tests meaningful: every corruption moves some block of the restatement's KKT arrays by more than 1e-3 of max(1, |block|) —
    a hundred and more times the limits the kernels are held to.  Measured: 0.20 at least (the largest array per corruption; DESIGN.md §4 has the table)."""
    for name, moves in sensitivity(seed).items():
        print(f"seed {seed}: {name:26s} G {moves[0]:.1e}  C {moves[1]:.1e}  g {moves[2]:.1e}  c {moves[3]:.1e}")
        assert max(moves) > 1e-3, (name, moves)


def test_the_same_entries_on_the_iiwa_are_printed_not_asserted():
    """The figures DESIGN.md quotes: on the iiwa three of the five corruptions move nothing or next to nothing."""
    for name, moves in sensitivity("iiwa").items():
        print(f"iiwa:   {name:26s} G {moves[0]:.1e}  C {moves[1]:.1e}  g {moves[2]:.1e}  c {moves[3]:.1e}")


@pytest.mark.parametrize("which", ("iiwa",) + cm.SEEDS)
def test_host_checks_accept_the_chain(which):
    """mpcg_plant_create's host checks (rotz form, rigid-body inertia, Xhom / X consistency) pass: the call succeeds, or fails only where it reaches
    for the device — never MPCG_ERR_INVALID or MPCG_ERR_UNSUPPORTED."""
    from mpcgpu_amd import Plant, _lib
    ch = cm.Chain.from_iiwa() if which == "iiwa" else chain(which)
    try:
        Plant(cm.tables(ch), device=0).close()
    except _lib.MpcgError as e:
        assert e.code == _lib.MPCG_ERR_HIP and "cannot place the model on the device" in str(e), e
