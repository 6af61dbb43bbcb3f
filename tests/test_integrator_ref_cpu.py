"""CPU: integrator 1 of tests/plant_ref.py — the restatement of semi-implicit Euler the GPU tests of options "integrator" / "sim_integrator" compare against
(tests/test_gpu_integrator.py) — pinned against the step map itself, and the cases of those GPU tests shown to tell the two integrators apart by far
more than their tolerances.  No GPU."""
import functools

import numpy as np
import pytest

import chain_models as cm
import iiwa_ref
import plant_ref as P
from mpcgpu_amd import iiwa

n, m = 14, 7
N, B = 8, 3
DT = iiwa_ref.TIMESTEP
MODELS = ("iiwa", 3)                     # the iiwa and tests/chain_models.py::random_chain(3)
KKT_MODELS = ("iiwa", 2)                 # the plants of the KKT and merit cases of tests/test_gpu_integrator.py: the iiwa and random_chain(2)
GPU_TOL = 1e-6                           # the tightest float-entry tolerance of tests/test_gpu_integrator.py (KKT analytic, merit default, simulate)
# the simulate case of tests/test_gpu_integrator.py that the two integrators must differ on: four substeps of 2e-3 s (not the reference's 2e-4: ten of
# those differ by 4e-7 .. 1.9e-6, which 1e-6 cannot tell apart)
SIM_CASE = dict(toff_us=0, sim_us=8000, sim_step=np.float32(2e-3))


@functools.lru_cache(maxsize=None)
def model(which):
    return iiwa_ref.Model() if which == "iiwa" else cm.random_chain(which)


@functools.lru_cache(maxsize=None)
def windows():
    """The windows of the GPU tests, rounded to float32 as the float entries see them."""
    return tuple(np.asarray(a, np.float32).astype(np.float64) for a in iiwa.random_windows(N, B, 5))


@functools.lru_cache(maxsize=None)
def restated(which, integrator):
    xu, goals, xs = windows()
    return [P.generate_kkt(model(which), xu[b], goals[b], xs[b], N, dt=DT, integrator=integrator) for b in range(B)]


def knots(b):
    xu = windows()[0][b]
    for k in range(N - 1):
        yield k, xu[k * (n + m):k * (n + m) + n], xu[k * (n + m) + n:(k + 1) * (n + m)], xu[(k + 1) * (n + m):(k + 1) * (n + m) + n]


@pytest.mark.parametrize("which", MODELS)
def test_restated_A_and_B_are_the_derivative_of_the_step_map(which):
    """A and B of plant_ref.generate_kkt (out of the dense C) against central differences, h = 1e-6, of step(..., 1) itself, on every knot of
    the windows.  Limit 1e-8: 14 to 30 times the worst measured (3.2e-10 on the iiwa, 7.1e-10 on the chain), to absorb BLAS differences between machines —
    and 1e5 times below what separates the integrators (next test).  The defect is the step map by construction: checked to be exactly x_{k+1} - step."""
    M = model(which)
    h, worst = 1e-6, 0.0
    for b in range(B):
        _, C, _, c = restated(which, 1)[b]
        A, Bm, cc = P.blocks(C, c, N)
        for k, x, u, xn in knots(b):
            z = np.concatenate([x, u])
            J = np.zeros((n, n + m))
            for j in range(n + m):
                e = np.zeros(n + m)
                e[j] = h
                J[:, j] = (P.step(M, (z + e)[:n], (z + e)[n:], DT, 1) - P.step(M, (z - e)[:n], (z - e)[n:], DT, 1)) / (2 * h)
            worst = max(worst, np.abs(A[k] - J[:, :n]).max(), np.abs(Bm[k] - J[:, n:]).max())
            assert np.array_equal(cc[k + 1], xn - P.step(M, x, u, DT, 1))
    print(f"INTEGRATOR-FIG {which}: restated A, B against central differences of the step map, worst {worst:.2e}")
    assert worst <= 1e-8, worst


@pytest.mark.parametrize("which", MODELS)
def test_integrator_0_is_the_existing_restatement_exactly(which):
    xu, goals, xs = windows()
    for b in range(B):
        for a, w in zip(restated(which, 0)[b], iiwa_ref.generate_kkt(model(which), xu[b], goals[b], xs[b], N)):
            assert np.array_equal(a, w)
    x, u = xu[0, :n], xu[0, n:n + m]
    assert np.array_equal(P.step(model(which), x, u, DT, 0), -iiwa_ref.euler_defect(model(which), x, u, np.zeros(n), DT))
    assert np.array_equal(P.defect(model(which), x, u, xu[0, n + m:2 * n + m], DT, 0), iiwa_ref.euler_defect(model(which), x, u, xu[0, n + m:2 * n + m], DT))
    A, Bm, _ = P.blocks(*restated(which, 0)[0][1::2], N)
    assert all(np.array_equal(a, w) for a, w in zip(P.AB(model(which), x, u, DT, 0), (A[0], Bm[0])))


@pytest.mark.parametrize("which", KKT_MODELS)
def test_the_kkt_cases_tell_the_integrators_apart(which):
    """On every knot of the windows the explicit and the semi-implicit outputs differ by at least 100 times the GPU tolerance of 1e-6, relative to
    max(1, |block|) as the GPU tests measure: the top rows of A (dt^2 dqdd/dx), the top rows of B (dt^2 Minv) and the q half of the defect (dt^2 qdd).
    Measured on the iiwa: A 1.4e-3 .. 1.1e-2, B 5.3e-2 .. 5.5e-2 (absolute; 1.6e-2 of the block at least), defect 1.6e-4 .. 1.25e-3; least on chain 2: A 3.9e-4,
    B 3.8e-3, defect 2.0e-4.  (The q-defect differs by dt^2 |qdd|: chain 3 passes one knot of these windows with |qdd| < 0.3 rad/s^2, 7.3e-5 — below the
    factor of 100 —, chain 1 has 1.1e-4; the GPU cases therefore use chain 2.)  G, g and c_0 do not depend on the integrator: equal."""
    lo = {"A": np.inf, "B": np.inf, "c": np.inf}
    for b in range(B):
        (G0, C0, g0, c0), (G1, C1, g1, c1) = restated(which, 0)[b], restated(which, 1)[b]
        assert np.array_equal(G0, G1) and np.array_equal(g0, g1) and np.array_equal(c0[:n], c1[:n])
        (A0, B0, d0), (A1, B1, d1) = P.blocks(C0, c0, N), P.blocks(C1, c1, N)
        assert np.array_equal(A0[:, 7:], A1[:, 7:]) and np.array_equal(B0[:, 7:], B1[:, 7:])         # the lower halves are explicit Euler's
        for k in range(N - 1):
            lo["A"] = min(lo["A"], np.abs(A0[k, :7] - A1[k, :7]).max() / max(1.0, np.abs(A1[k]).max()))
            lo["B"] = min(lo["B"], np.abs(B0[k, :7] - B1[k, :7]).max() / max(1.0, np.abs(B1[k]).max()))
            lo["c"] = min(lo["c"], np.abs(d0[k + 1, :7] - d1[k + 1, :7]).max() / max(1.0, np.abs(d1).max()))
    print(f"INTEGRATOR-FIG {which}: least difference per knot, A {lo['A']:.2e} B {lo['B']:.2e} q-defect {lo['c']:.2e}")
    assert min(lo.values()) >= 100 * GPU_TOL, lo


def test_the_simulate_cases_tell_the_integrators_apart(which="iiwa"):
    """sim_step = 2e-3 over 8000 us (four substeps), and one substep of dt = 1/64: on every trajectory the two integrators' new states differ by at
    least 10 times the 1e-6 of the GPU test, relative to max(1, |x|) — on the iiwa, the plant of the GPU simulate cases.  Measured: 1.7e-5 .. 6.0e-5 for the former.  The reference's own
    schedule (ten substeps of 2e-4) is printed for the record: 4e-7 .. 1.9e-6, NOT distinguishable, which is why the GPU test does not use it."""
    xu, _, xs = windows()
    M = model(which)
    rel = lambda a, w: float((np.abs(a - w) / np.maximum(1.0, np.abs(w))).max())
    gaps = {"2e-3 x 4": [], "1/64 x 1": [], "2e-4 x 10": []}
    for b in range(B):
        gaps["2e-3 x 4"].append(rel(P.simulate(M, xs[b], xu[b], N, DT, integrator=0, **SIM_CASE), P.simulate(M, xs[b], xu[b], N, DT, integrator=1, **SIM_CASE)))
        gaps["1/64 x 1"].append(rel(P.simulate(M, xs[b], xu[b], N, DT, 0, 15625, 1 / 64, 0), P.simulate(M, xs[b], xu[b], N, DT, 0, 15625, 1 / 64, 1)))
        gaps["2e-4 x 10"].append(rel(P.simulate(M, xs[b], xu[b], N, DT, 0, 2000, P.SIM_STEP, 0), P.simulate(M, xs[b], xu[b], N, DT, 0, 2000, P.SIM_STEP, 1)))
    print(f"INTEGRATOR-FIG {which}: simulate gaps per trajectory", {k: [f"{g:.1e}" for g in v] for k, v in gaps.items()})
    assert P.schedule(SIM_CASE["toff_us"], SIM_CASE["sim_us"], DT, SIM_CASE["sim_step"])[0] in (3, 4)
    assert min(gaps["2e-3 x 4"]) >= 10 * GPU_TOL and min(gaps["1/64 x 1"]) >= 10 * GPU_TOL, gaps


def test_merit_restatement_measures_the_kkt_restatements_defect():
    """merit(mu = 2) - merit(mu = 1) of plant_ref.merits is the 1-norm of plant_ref.generate_kkt's c, for either integrator (d_xs given, step 0)."""
    xu, goals, xs = windows()
    M = model("iiwa")
    for integrator in (0, 1):
        tail = dict(cost=P.Cost.plain(iiwa.QD_COST, iiwa.r_cost(N)), dt=DT, integrator=integrator)
        m2, m1 = (P.merits(M, xu[:1], None, [0.0], goals[:1], xs[:1], N, mu, **tail)[0, 0] for mu in (2.0, 1.0))
        want = np.abs(restated("iiwa", integrator)[0][3]).sum()
        assert abs((m2 - m1) - want) <= 1e-12 * max(1.0, m2), (integrator, m2 - m1, want)
