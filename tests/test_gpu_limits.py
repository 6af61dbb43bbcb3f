"""GPU: soft joint, velocity and torque limits as model data of a plant (include/mpcg.h, LIMITS; mpcg_plant_clone_limits) — the COST = 2 instantiations of the
KKT and merit kernels behind the _xuref entries, and the saturating instantiation of simulate_kernel — against the float64 restatement tests/plant_ref.py,
against the _xuref results with the plain plant where nothing is violated, against each other on the device, for independence of the batch and containment of
a NaN trajectory, inside a hipGraph, and through the error table.  Inputs and shapes: the cases of tests/test_gpu_xuref.py (shared, read-only); the bounds
come from each case's own values — per kind and joint the lower and upper third, nudged off every value — so that below, inside and above all occur and the
indicator is decided from identical numbers in the kernel and in the restatement."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import plant_ref as P
from chain_cost_cases import WEIGHTS, bounds_of, f32, limits_of
from mpcgpu_amd import XuRef, _lib, iiwa
from test_gpu_xuref import COSTS, DT, KKT_BUILDS, LIMIT_C, LIMIT_Ggc, MERIT_BUILDS, MU, SHAPES, STEPS8, STEPS9, bits, case, dev, model, plant, solver, want_merits

pytestmark = pytest.mark.gpu
n, m, NJ, ROW = 14, 7, 7, 21


def states_controls(cs, steps):
    """The states and controls of every trajectory of a case at the trial iterates of `steps` (step size 0: the iterate itself)."""
    xs, us = [], []
    for b in range(cs.B):
        for a in steps:
            x, u = P.split(P.trial(cs.xu[b], cs.dz[b], a, cs.double), cs.N)
            xs.append(x)
            us.append(u)
    return xs, us


@functools.lru_cache(maxsize=None)
def kkt_limits(N, B, double=False):
    return limits_of(*states_controls(case(N, B, double), [0.0]))


@functools.lru_cache(maxsize=None)
def merit_limits(N, B, double=False):
    return limits_of(*states_controls(case(N, B, double), STEPS9))


def with_limits(lim, base=None, sim_saturate=False):
    fin = lambda a: [float(v) for v in a]
    return (base or plant()).with_limits(q=(fin(lim.q_lo), fin(lim.q_hi)), qd=(fin(lim.qd_lo), fin(lim.qd_hi)), u=(fin(lim.u_lo), fin(lim.u_hi)),
                                         q_weight=lim.q_weight, qd_weight=lim.qd_weight, u_weight=lim.u_weight, sim_saturate=sim_saturate)


@functools.lru_cache(maxsize=None)
def kkt_plant(N, B, double=False):
    return with_limits(kkt_limits(N, B, double))


@functools.lru_cache(maxsize=None)
def merit_plant(N, B, double=False):
    return with_limits(merit_limits(N, B, double))


def kkt(cs, sol, co, pl, dtype=np.float32, xu=None):
    out = sol.generate_kkt_xuref(pl, None if co.ee_cost == 0 else dev(cs.goals, dtype), dev(cs.xs, dtype), dev(cs.xu if xu is None else xu, dtype), DT, co.qd_cost,
                                 co.r_cost, cs.xuref(co, dtype))
    torch.cuda.synchronize()
    return out


def merit(cs, sol, co, pl, steps, dtype=np.float32, with_xs=True, xu=None, dz="own"):
    out = sol.compute_merit_xuref(pl, None if co.ee_cost == 0 else dev(cs.goals, dtype), dev(cs.xs, dtype) if with_xs else None,
                                  dev(cs.xu, dtype) if xu is None else xu, dev(cs.dz, dtype) if isinstance(dz, str) else dz, steps, DT, MU, co.qd_cost, co.r_cost,
                                  cs.xuref(co, dtype))
    torch.cuda.synchronize()
    return out


# ---- 1. KKT against the restatement ----
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("build", list(KKT_BUILDS))
@pytest.mark.parametrize("N,B", SHAPES)
def test_kkt_vs_host_restatement(N, B, build, integrator):
    """|got - want| <= tol max(1, max |want array|) for G, C, g, c of every trajectory, every build, both integrators, at the limits tests/test_gpu_xuref.py
    holds the plain plant to; C and c are bit for bit those of the same call with the plain plant."""
    opts, tol = KKT_BUILDS[build]
    cs, co, lim = case(N, B), COSTS["all"], kkt_limits(N, B)
    sol = solver(N, B, opts, integrator)
    out = kkt(cs, sol, co, kkt_plant(N, B))
    base = kkt(cs, sol, co, plant())
    assert np.array_equal(bits(out[1]), bits(base[1])) and np.array_equal(bits(out[3]), bits(base[3]))
    assert not np.array_equal(bits(out[0]), bits(base[0])) and not np.array_equal(bits(out[2]), bits(base[2]))
    got = [t.cpu().numpy() for t in out]
    assert all(np.isfinite(a).all() for a in got)
    worst = 0.0
    for b in range(B):
        want = P.generate_kkt(model(), cs.xu[b], cs.goals[b], cs.xs[b], N, rows=cs.rows(b), cost=co, limits=lim, dt=DT, integrator=integrator, base=cs.dynamics(b, integrator))
        for a, w, name in zip(got, want, "GCgc"):
            err = np.abs(a[b] - w).max() / max(1.0, np.abs(w).max())
            worst = max(worst, err)
            print(f"kkt limits N={N} B={B} {build} integrator={integrator} b={b} {name}: {err:.2e} (limit {tol:.0e})")
            assert err <= tol, (b, name, err)


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("analytic", [1, 0])
@pytest.mark.parametrize("N,B", [(2, 1), (5, 3)])
def test_double_entry_vs_host_restatement(N, B, analytic, integrator):
    """mpcg_generate_kkt_xuref_f64 on genuinely double inputs with a limits plant: the limits of tests/test_gpu_xuref.py's double test, G, g, c 8.8e-11, C 8.9e-7
    (analytic route; the difference route's own limits are those of its float twin's test, 3e-6)."""
    cs, co, lim = case(N, B, True), COSTS["all"], kkt_limits(N, B, True)
    sol = solver(N, B, (("kkt_analytic", analytic),), integrator)
    out = kkt(cs, sol, co, kkt_plant(N, B, True), np.float64)
    base = kkt(cs, sol, co, plant(), np.float64)
    assert np.array_equal(bits(out[1]), bits(base[1])) and np.array_equal(bits(out[3]), bits(base[3]))
    assert not np.array_equal(bits(out[0]), bits(base[0])) and not np.array_equal(bits(out[2]), bits(base[2]))
    got = [t.cpu().numpy() for t in out]
    assert all(np.isfinite(a).all() for a in got)
    worst = {"Ggc": 0.0, "C": 0.0}
    for b in range(B):
        want = P.generate_kkt(model(), cs.xu[b], cs.goals[b], cs.xs[b], N, rows=cs.rows(b), cost=co, limits=lim, dt=DT, integrator=integrator, base=cs.dynamics(b, integrator))
        for a, w, name in zip(got, want, "GCgc"):
            key = "C" if name == "C" else "Ggc"
            worst[key] = max(worst[key], np.abs(a[b] - w).max() / max(1.0, np.abs(w).max()))
    print(f"kkt limits f64 N={N} B={B} analytic={analytic} integrator={integrator}: worst G,g,c {worst['Ggc']:.3e}  C {worst['C']:.3e}")
    if analytic:
        assert worst["Ggc"] <= LIMIT_Ggc and worst["C"] <= LIMIT_C, worst
    else:
        assert worst["Ggc"] <= 3e-6 and worst["C"] <= 3e-6, worst


# ---- 2. merit against the restatement ----
@pytest.mark.parametrize("with_xs", [True, False])
@pytest.mark.parametrize("build", list(MERIT_BUILDS))
@pytest.mark.parametrize("N,B", SHAPES)
def test_merit_vs_host_restatement(N, B, build, with_xs):
    """Nine step sizes: |got - want| <= limit max(1, |want|) — 1e-6, 1e-5 with "merit_f32", 1.2e-13 for the double entry on double inputs."""
    opts, limit, dtype = MERIT_BUILDS[build]
    double = dtype == np.float64
    cs, co, lim = case(N, B, double), COSTS["all"], merit_limits(N, B, double)
    got = merit(cs, solver(N, B, opts), co, merit_plant(N, B, double), STEPS9, dtype, with_xs).cpu().numpy().astype(np.float64)
    base = want_merits(N, B, "all", with_xs, 0, double)
    w = P.merits(model(), cs.xu, cs.dz, STEPS9, cs.goals, cs.xs if with_xs else None, N, MU, rows_of=cs.rows, cost=co, limits=lim, dt=DT, integrator=0, double=double, base=base)
    assert got.shape == (B, 9) and np.isfinite(got).all() and (w > base).all()
    err = np.abs(got - w) / np.maximum(1.0, np.abs(w))
    print(f"merit limits N={N} B={B} {build} xs={with_xs}: merits {w.min():.3g} .. {w.max():.3g} (penalty up to {(w - base).max():.3g}), worst {err.max():.2e} (limit {limit:.1e})")
    assert err.max() <= limit, (err.max(), got, w)


@pytest.mark.parametrize("build", list(MERIT_BUILDS))
def test_merit_semi_implicit_integrator(build):
    opts, limit, dtype = MERIT_BUILDS[build]
    N, B, double = 3, 2, dtype == np.float64
    cs, co, lim = case(N, B, double), COSTS["all"], merit_limits(N, B, double)
    got = merit(cs, solver(N, B, opts, 1), co, merit_plant(N, B, double), STEPS9, dtype).cpu().numpy().astype(np.float64)
    w = P.merits(model(), cs.xu, cs.dz, STEPS9, cs.goals, cs.xs, N, MU, rows_of=cs.rows, cost=co, limits=lim, dt=DT, integrator=1, double=double, base=want_merits(N, B, "all", True, 1, double))
    assert (np.abs(got - w) / np.maximum(1.0, np.abs(w))).max() <= limit


# ---- 3. equality with the xu_ref results when nothing is violated ----
def quiet_plants(N, B):
    lim = merit_limits(N, B)
    return {"infinite": with_limits(P.Limits(None, None, None, None, None, None, *WEIGHTS)),
            "wide": with_limits(P.Limits(-64.0, 64.0, -1024.0, None, None, 4096.0, *WEIGHTS)),
            "zero weights": with_limits(P.Limits(lim.q_lo, lim.q_hi, lim.qd_lo, lim.qd_hi, lim.u_lo, lim.u_hi, 0.0, 0.0, 0.0))}


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("build", list(KKT_BUILDS) + ["f64"])
@pytest.mark.parametrize("N,B", [(2, 1), (5, 3)])
def test_kkt_equals_the_plain_plants_when_nothing_is_violated(N, B, build, integrator):
    """Infinite bounds, finite bounds nothing violates, and violated bounds at zero weights: every output equals (==: a -0 may become +0) the same call's with
    the plain plant — G's off-diagonal and g away from nothing included, i.e. everywhere."""
    opts = KKT_BUILDS[build][0] if build != "f64" else ()
    dtype = np.float64 if build == "f64" else np.float32
    cs, co = case(N, B), COSTS["all"]
    x, u = zip(*[P.split(cs.xu[b], N) for b in range(B)])
    assert np.abs(np.concatenate(x)[:, :NJ]).max() < 64 and np.abs(np.concatenate(x)[:, NJ:]).max() < 1024 and np.abs(np.concatenate(u)).max() < 4096
    sol = solver(N, B, opts, integrator)
    base = [t.cpu().numpy() for t in kkt(cs, sol, co, plant(), dtype)]
    for name, pl in quiet_plants(N, B).items():
        for a, w, arr in zip(kkt(cs, sol, co, pl, dtype), base, "GCgc"):
            assert np.array_equal(a.cpu().numpy(), w), (name, arr)


@pytest.mark.parametrize("build", list(MERIT_BUILDS))
@pytest.mark.parametrize("N,B", [(2, 1), (8, 3)])
def test_merit_equals_the_plain_plants_when_nothing_is_violated(N, B, build):
    opts, _, dtype = MERIT_BUILDS[build]
    cs, co = case(N, B), COSTS["all"]
    xs, us = states_controls(cs, STEPS9)
    assert np.abs(np.concatenate(xs)[:, :NJ]).max() < 64 and np.abs(np.concatenate(xs)[:, NJ:]).max() < 1024 and np.abs(np.concatenate(us)).max() < 4096
    sol = solver(N, B, opts)
    base = merit(cs, sol, co, plant(), STEPS9, dtype).cpu().numpy()
    for name, pl in quiet_plants(N, B).items():
        assert np.array_equal(merit(cs, sol, co, pl, STEPS9, dtype).cpu().numpy(), base), name


# ---- 4. the two entries agree on the device, in double ----
def test_merit_differences_are_the_kkt_gradient():
    """ee_cost = 0, mu = 0, N = 4, as tests/test_gpu_xuref.py: the cost sum with the penalty is piecewise quadratic in xu, and with every value further than 2 h
    from every bound no perturbed copy crosses a kink — the central differences of ONE compute_merit_xuref_f64 call equal g of generate_kkt_xuref_f64 to 1e-9."""
    from mpcgpu_amd import PcgSolver
    N, Lz, h = 4, 77, 1e-3
    cs = case(8, 3, True)
    xu = cs.xu[0, :Lz].copy()
    x, u = P.split(xu, N)

    def far_bounds(vals):                                      # per joint: its smallest value below, its largest above, the rest inside
        lo, hi = np.zeros(NJ), np.zeros(NJ)
        for i in range(NJ):
            s = np.sort(vals[:, i])
            lo[i], hi[i] = 0.5 * (s[0] + s[1]), 0.5 * (s[-2] + s[-1])
            if min(s[1] - s[0], s[-1] - s[-2]) <= 5 * h:        # values too close together for that: one bound, below all of them by 1/4
                lo[i], hi[i] = -np.inf, s[0] - 0.25
        return f32(lo), f32(hi)
    (q_lo, q_hi), (qd_lo, qd_hi), (u_lo, u_hi) = far_bounds(x[:, :NJ]), far_bounds(x[:, NJ:]), far_bounds(u)
    lim = P.Limits(q_lo, q_hi, qd_lo, qd_hi, u_lo, u_hi, *WEIGHTS)
    for vals, lo, hi in ((x[:, :NJ], q_lo, q_hi), (x[:, NJ:], qd_lo, qd_hi), (u, u_lo, u_hi)):
        assert min(np.abs(vals - lo).min(), np.abs(vals - hi).min()) > 2 * h               # further than 2 h from every bound
        s = P.side(vals, lo, hi)
        assert all((s == v).any() for v in (-1, 0, 1))
    pl = with_limits(lim)
    co = P.Cost(0.0, 0.5, 2.0 ** -6, 2.0 ** -7, P.QD_RELATIVE | P.U_RELATIVE)
    plan = dev(cs.plan, np.float64)
    sol = PcgSolver(N, max_batch=2 * Lz)
    ref = lambda B: XuRef(plan, torch.full((B,), 2, dtype=torch.int32, device="cuda"), 0, 0.0, co.q_cost, True, True)
    _, _, g, _ = sol.generate_kkt_xuref(pl, None, dev(cs.xs[:1], np.float64), dev(xu[None], np.float64), DT, co.qd_cost, co.r_cost, ref(1))
    pert = np.concatenate([xu + h * np.eye(Lz), xu - h * np.eye(Lz)])
    mer = sol.compute_merit_xuref(pl, None, None, dev(pert, np.float64), None, [0.0], DT, 0.0, co.qd_cost, co.r_cost, ref(2 * Lz))
    torch.cuda.synchronize()
    g, mer = g.cpu().numpy()[0], mer.cpu().numpy()[:, 0]
    num = (mer[:Lz] - mer[Lz:]) / (2 * h)
    err = np.abs(num - g).max() / max(1.0, np.abs(g).max())
    print(f"limits: |g| up to {np.abs(g).max():.3g}, central differences off by {err:.2e}")
    assert err <= 1e-9, err
    rows = P.plan_rows(cs.plan, 0, 2, N, cs.T)
    want = P.generate_kkt(model(), xu, None, cs.xs[0], N, rows=rows, cost=co, limits=lim, base=(np.zeros(0), np.zeros(ROW * N - m), np.zeros(0)))[2]
    assert np.abs(g - want).max() <= 1e-12
    assert np.abs(want - P.generate_kkt(model(), xu, None, cs.xs[0], N, rows=rows, cost=co, base=(np.zeros(0), np.zeros(ROW * N - m), np.zeros(0)))[2]).max() > 1e-2


# ---- 5. the line search ----
@pytest.mark.parametrize("build", list(MERIT_BUILDS))
def test_accepted_merit_is_the_merit_of_the_new_iterate(build):
    """After line_search_step on the merits of a limits plant, the merit at step size 0 of the new xu is d_merit_ref bit for bit."""
    opts, _, dtype = MERIT_BUILDS[build]
    N, B = 8, 3
    cs, co, pl = case(N, B), COSTS["all"], merit_plant(8, 3)
    sol = solver(N, B, opts)
    td = torch.float32 if dtype == np.float32 else torch.float64
    d_xu, d_dz = dev(cs.xu, dtype), dev(cs.dz, dtype)
    mer = merit(cs, sol, co, pl, STEPS8, dtype, xu=d_xu, dz=d_dz)
    ref = torch.full((B,), float("inf"), device="cuda", dtype=td)
    step = sol.line_search_step(mer, STEPS8, ref, d_dz, d_xu)
    again = merit(cs, sol, co, pl, [0.0], dtype, xu=d_xu, dz=None)
    assert (step.cpu().numpy() >= 0).all()
    assert np.array_equal(bits(again)[:, 0], bits(ref))
    assert np.array_equal(ref.cpu().numpy(), mer.cpu().numpy().min(axis=1))
    assert not np.array_equal(bits(mer), bits(merit(cs, sol, co, plant(), STEPS8, dtype)))


# ---- 6. batch independence and containment ----
def batch_of_70(seed):
    N, B = 4, 70
    small = case(8, 3)
    pick = np.random.default_rng(seed).integers(0, 3, B)
    Lz = ROW * N - m
    return N, B, small, small.xu[pick, :Lz].copy(), small.dz[pick, :Lz], small.goals[pick, :6 * N], small.xs[pick]


@pytest.mark.parametrize("f32_build", [0, 1])
def test_kkt_does_not_depend_on_the_batch_and_a_nan_is_contained(f32_build):
    """A trajectory alone and inside a batch of 70, "kkt_f32" = 0 and 1 (two knots per lane: its partner changes); and with trajectory 36 all NaN every other
    trajectory keeps every bit."""
    N, B, small, xu, _, goals, xs = batch_of_70(72)
    pl, co = merit_plant(8, 3), COSTS["all"]
    sol = solver(N, B, (("kkt_f32", f32_build),))
    plan = dev(small.plan)

    def call(sel, xu_):
        ref = XuRef(plan, None, 0, co.ee_cost, co.q_cost, True, True)
        out = sol.generate_kkt_xuref(pl, dev(goals[sel]), dev(xs[sel]), dev(xu_[sel]), DT, co.qd_cost, co.r_cost, ref)
        torch.cuda.synchronize()
        return [bits(t) for t in out]
    full = call(slice(0, B), xu)
    for b in (0, 37, 69):
        for a, f, name in zip(call(slice(b, b + 1), xu), full, "GCgc"):
            assert np.array_equal(a[0], f[b]), (b, name)
    bad = xu.copy()
    bad[36] = np.nan
    others = np.arange(B) != 36
    for f, p, name in zip(full, call(slice(0, B), bad), "GCgc"):
        assert np.array_equal(f[others], p[others]), name
    assert not np.array_equal(full[2], bits(sol.generate_kkt_xuref(plant(), dev(goals), dev(xs), dev(xu), DT, co.qd_cost, co.r_cost, XuRef(plan, None, 0, co.ee_cost, co.q_cost, True, True))[2]))


@pytest.mark.parametrize("f32_build", [0, 1])
def test_merit_does_not_depend_on_the_batch_and_a_nan_is_contained(f32_build):
    N, B, small, xu, dz, goals, xs = batch_of_70(73)
    pl, co = merit_plant(8, 3), COSTS["all"]
    sol = solver(N, B, (("merit_f32", f32_build),))
    plan = dev(small.plan)

    def call(sel, xu_, plant_=pl):
        ref = XuRef(plan, None, 0, co.ee_cost, co.q_cost, True, True)
        out = sol.compute_merit_xuref(plant_, dev(goals[sel]), dev(xs[sel]), dev(xu_[sel]), dev(dz[sel]), STEPS9, DT, MU, co.qd_cost, co.r_cost, ref)
        torch.cuda.synchronize()
        return bits(out)
    full = call(slice(0, B), xu)
    for b in (0, 37, 69):
        assert np.array_equal(call(slice(b, b + 1), xu)[0], full[b]), b
    bad = xu.copy()
    bad[36] = np.nan
    others = np.arange(B) != 36
    poisoned = call(slice(0, B), bad)
    assert np.array_equal(poisoned[others], full[others]) and np.isnan(poisoned[36].view(np.float32)).all()
    assert not np.array_equal(full, call(slice(0, B), xu, plant()))


# ---- 7. simulate ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("sim_integrator", [0, 1])
def test_simulate_saturates_at_the_torque_limits(sim_integrator, dtype):
    """Two substeps and a remainder: with sim_saturate the state and end-effector position are bit for bit mpcg_simulate(_f64)'s of the plain plant on controls
    clamped on the host; without the flag they are the plain plant's on the controls as they are.  (5, 3): a wavefront with an idle group."""
    N, B = 5, 3
    cs, lim = case(N, B), kkt_limits(5, 3)
    sol = solver(N, B)
    sol.set_option("sim_integrator", sim_integrator)
    clamped = cs.xu.copy()
    for k in range(N - 1):
        u = clamped[:, ROW * k + n:ROW * (k + 1)]
        u[:] = np.minimum(np.maximum(u, lim.u_lo), lim.u_hi)              # bounds that are floats: the clamped controls are floats too
    assert (clamped != cs.xu).any() and np.array_equal(clamped, f32(clamped))
    td = torch.float32 if dtype == np.float32 else torch.float64

    def run(pl, xu):
        xs, ee = dev(cs.xs, dtype), torch.zeros(B, 3, device="cuda", dtype=td)
        sol.simulate(pl, xs, dev(xu, dtype), DT, 14000.0, 2.5e6 / 64 / 2, 1 / 128, eePos=ee)      # the call starts inside knot 0 and crosses into knot 1: 2 substeps of 1/128 s + 1/256 s
        torch.cuda.synchronize()
        return bits(xs), bits(ee)
    sat, flagless = with_limits(lim, sim_saturate=True), kkt_plant(5, 3)
    want, plain = run(plant(), clamped), run(plant(), cs.xu)
    assert not np.array_equal(want[0], plain[0])
    for got, w in ((run(sat, cs.xu), want), (run(flagless, cs.xu), plain), (run(sat, clamped), want)):
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])


# ---- 8. errors, clones, the Python layer, a captured graph ----
def c_limits(**kw):
    lim = _lib.mpcg_limits()
    for name in ("q", "qd", "u"):
        setattr(lim, name + "_lo", (C.c_double * 7)(*([-math.inf] * 7)))
        setattr(lim, name + "_hi", (C.c_double * 7)(*([math.inf] * 7)))
    lim.q_weight, lim.qd_weight, lim.u_weight, lim.flags = 1.0, 2.0, 3.0, 0
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(lim, k)[v[0]] = v[1]
        else:
            setattr(lim, k, v)
    return lim


def test_clone_refusals_and_round_trip():
    lib = _lib.load()
    INV, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_OK
    src = plant()._p
    nan, inf = math.nan, math.inf
    bad = [dict(q_lo=(3, nan)), dict(u_hi=(0, nan)), dict(qd_lo=(6, 1.0), qd_hi=(6, 0.5)), dict(q_lo=(0, inf)), dict(u_hi=(2, -inf)), dict(q_lo=(1, inf), q_hi=(1, inf)),
           dict(q_weight=-1e-300), dict(qd_weight=inf), dict(u_weight=nan), dict(flags=2), dict(flags=0x80000001)]
    for kw in bad:
        out = C.c_void_p(1234)
        assert lib.mpcg_plant_clone_limits(C.byref(out), src, C.byref(c_limits(**kw))) == INV and not out.value, kw
    out = C.c_void_p(1234)
    assert lib.mpcg_plant_clone_limits(C.byref(out), None, C.byref(c_limits())) == INV and not out.value
    out = C.c_void_p(1234)
    assert lib.mpcg_plant_clone_limits(C.byref(out), src, None) == INV and not out.value
    assert lib.mpcg_plant_clone_limits(None, src, C.byref(c_limits())) == INV
    # what it allows: lo == hi, -0 weights, one-sided and two-sided infinities; and the round trip
    given = c_limits(q_lo=(2, 0.5), q_hi=(2, 0.5), u_lo=(5, -176.0), u_hi=(5, 176.0), qd_hi=(0, 0.1), q_weight=-0.0, flags=1)
    out = C.c_void_p()
    assert lib.mpcg_plant_clone_limits(C.byref(out), src, C.byref(given)) == OK and out.value
    back, has = _lib.mpcg_limits(), C.c_int(-1)
    assert lib.mpcg_plant_get_limits(out, C.byref(back), C.byref(has)) == OK and has.value == 1
    assert bytes(back)[:6 * 7 * 8 + 3 * 8 + 4] == bytes(given)[:6 * 7 * 8 + 3 * 8 + 4]
    assert lib.mpcg_plant_get_limits(None, C.byref(back), C.byref(has)) == INV and lib.mpcg_plant_get_limits(out, None, C.byref(has)) == INV
    assert lib.mpcg_plant_get_limits(out, C.byref(back), None) == INV
    lib.mpcg_plant_destroy(out)
    assert lib.mpcg_plant_get_limits(src, C.byref(back), C.byref(has)) == OK and has.value == 0
    assert list(back.q_lo) == [-inf] * 7 and list(back.u_hi) == [inf] * 7 and back.u_weight == 0.0 and back.flags == 0


def test_limits_and_gravity_survive_each_other():
    lim = kkt_limits(5, 3)
    a = with_limits(lim, sim_saturate=True)
    assert plant().limits is None and a.gravity == (0.0, 0.0, 0.0)
    g = a.with_gravity((0.0, 0.0, 9.81))
    b = plant().with_gravity((0.5, 0.0, 9.81)).with_limits(u=(-176.0, 176.0), u_weight=2.0)
    assert g.limits == a.limits and g.gravity == (0.0, 0.0, 9.81) and a.limits["sim_saturate"] is True
    assert a.limits["q"] == (tuple(lim.q_lo), tuple(lim.q_hi)) and a.limits["q"][0][1] == -math.inf and a.limits["u_weight"] == lim.u_weight
    assert b.gravity == (0.5, 0.0, 9.81) and b.limits["u"] == ((-176.0,) * 7, (176.0,) * 7) and b.limits["q"] == ((-math.inf,) * 7, (math.inf,) * 7)
    assert b.limits["q_weight"] == 0.0 and b.limits["sim_saturate"] is False
    # the clone is the gravity plant's twin in what limits do not touch: C, c of a KKT call
    N, B = 3, 2
    cs, co, sol = case(N, B), COSTS["all"], solver(N, B)
    heavy = kkt(cs, sol, co, plant().with_gravity((0.5, 0.0, 9.81)))
    for i in (1, 3):
        assert np.array_equal(bits(kkt(cs, sol, co, b)[i]), bits(heavy[i])) and not np.array_equal(bits(heavy[i]), bits(kkt(cs, sol, co, plant())[i]))
    assert np.array_equal(bits(kkt(cs, sol, co, g)[0]), bits(kkt(cs, sol, co, a)[0]))          # G (the pose and the penalty) does not depend on gravity


def test_python_layer_type_errors():
    p = plant()
    for kw in (dict(q=(0.0,)), dict(q=0.5), dict(u=([0.0] * 6, None)), dict(qd=(None, [1.0] * 8)), dict(u=("a", None)), dict(q=(None, [None] * 7)), dict(u=(-1.0, 1.0, 2.0)),
               dict(q=([[0.0] * 7], None)), dict(u=(True, None))):
        with pytest.raises(TypeError):
            p.with_limits(**kw)
    with pytest.raises(_lib.MpcgError):
        p.with_limits(u=(1.0, -1.0))
    with pytest.raises(_lib.MpcgError):
        p.with_limits(u_weight=-1.0)
    ok = p.with_limits(u=(-1, np.float32(2.0) * np.ones(7, np.float32)), qd=(None, 3))
    assert ok.limits["u"] == ((-1.0,) * 7, (2.0,) * 7) and ok.limits["qd"] == ((-math.inf,) * 7, (3.0,) * 7)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plain_entries_refuse_a_limits_plant(prec):
    """mpcg_generate_kkt(_f64) and mpcg_compute_merit(_f64) given a plant with limits: MPCG_ERR_UNSUPPORTED, a message that names the _xuref entries, and the
    NaN-filled outputs keep every bit; mpcg_inverse_dynamics(_f64) ignores the limits."""
    N, B = 4, 2
    td = torch.float32 if prec == "f32" else torch.float64
    dtype = np.float32 if prec == "f32" else np.float64
    cs = case(8, 3)
    Lz = ROW * N - m
    sol, pl = solver(N, B), kkt_plant(5, 3)
    goals, xs, xu, dz = dev(cs.goals[:B, :6 * N], dtype), dev(cs.xs[:B], dtype), dev(cs.xu[:B, :Lz], dtype), dev(cs.dz[:B, :Lz], dtype)
    with pytest.raises(_lib.MpcgError) as e:
        sol.generate_kkt(pl, goals, xs, xu, DT, 1e-4, 1e-4)
    assert e.value.code == _lib.MPCG_ERR_UNSUPPORTED and "_xuref" in str(e.value) and "ee_cost = 1" in str(e.value)
    mer = torch.full((B, 9), float("nan"), device="cuda", dtype=td)
    keep = bits(mer).copy()
    with pytest.raises(_lib.MpcgError) as e:
        sol.compute_merit(pl, goals, xs, xu, dz, STEPS9, DT, MU, 1e-4, 1e-4, merit=mer)
    assert e.value.code == _lib.MPCG_ERR_UNSUPPORTED and "_xuref" in str(e.value)
    torch.cuda.synchronize()
    assert np.array_equal(bits(mer), keep)
    # raw: the KKT outputs stay as they were
    lib = _lib.load()
    nan = lambda k: torch.full((B, k), float("nan"), device="cuda", dtype=td)
    outs = [nan((n * n + m * m) * N - m * m), nan((n * n + n * m) * (N - 1)), nan(Lz), nan(n * N)]
    kept = [bits(t).copy() for t in outs]
    p = lambda t: C.c_void_p(t.data_ptr())
    fn = lib.mpcg_generate_kkt if prec == "f32" else lib.mpcg_generate_kkt_f64
    assert fn(sol._h, pl._p, 7, DT, p(goals), p(xs), p(xu), 1e-4, 1e-4, *(p(t) for t in outs), B, None) == _lib.MPCG_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for t, k in zip(outs, kept):
        assert np.array_equal(bits(t), k)
    q = dev(cs.xu[:B, :NJ], dtype)
    assert np.array_equal(bits(sol.inverse_dynamics(pl, q)), bits(sol.inverse_dynamics(plant(), q)))


def test_captured_graph_of_a_limits_call_replays():
    """One KKT + merit + simulate call with limits plants is captured (the merit scratch allocated before); replays give an eager call's bits."""
    N, B = 5, 3
    cs, co, pl = case(N, B), COSTS["all"], merit_plant(5, 3)
    sat = with_limits(merit_limits(5, 3), sim_saturate=True)
    sol = solver(N, B)
    goals, xs, xu, dz = (dev(a) for a in (cs.goals, cs.xs, cs.xu, cs.dz))
    ref = cs.xuref(co, np.float32)
    g_merit, state = torch.zeros(B, 9, device="cuda"), dev(cs.xs)
    sol.compute_merit_xuref(pl, goals, xs, xu, dz, STEPS9, DT, MU, co.qd_cost, co.r_cost, ref, merit=g_merit)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_kkt = sol.generate_kkt_xuref(pl, goals, xs, xu, DT, co.qd_cost, co.r_cost, ref)
        sol.compute_merit_xuref(pl, goals, xs, xu, dz, STEPS9, DT, MU, co.qd_cost, co.r_cost, ref, merit=g_merit)
        sol.simulate(sat, state, xu, DT, 0.0, 15625.0, 1 / 128)
    e_kkt, e_merit = kkt(cs, sol, co, pl), merit(cs, sol, co, pl, STEPS9)
    e_state = dev(cs.xs)
    sol.simulate(sat, e_state, xu, DT, 0.0, 15625.0, 1 / 128)
    for _ in range(2):
        for t in (*g_kkt, g_merit):
            t.fill_(float("nan"))
        state.copy_(xs)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip((*g_kkt, g_merit, state), (*e_kkt, e_merit, e_state)):
            assert torch.isfinite(got).all() and np.array_equal(bits(got), bits(want))


# ---- 9. the closed loop over the C ABI ----
@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
def test_closed_loop_example_with_torque_limits(double):
    """examples/mpc_closed_loop(_f64) --gravity 9.81 --u-max X --u-weight W --sim-saturate runs and prints finite numbers; --u-max inf prints, character for
    character, what the run without the flags prints."""
    import json
    import subprocess
    from mpcgpu_amd import build
    exe = build.build_mpc_closed_loop_f64() if double else build.build_mpc_closed_loop()
    small = ("--batch", "3", "--knots", "8", "--updates", "9", "--mpc-steps", "12", "--gravity", "9.81")

    def run(*flags):
        r = subprocess.run([exe, *small, *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        line = r.stdout.strip().splitlines()[-1]
        return line, json.loads(line)
    plain, unbounded = run(), run("--u-max", "inf", "--u-weight", "4", "--sim-saturate")
    assert plain[0] == unbounded[0] and "u_max" not in plain[1]
    out = run("--u-max", "40", "--u-weight", "4", "--sim-saturate")[1]
    assert out["ok"] is True and out["u_max"] == 40 and out["u_weight"] == 4 and out["sim_saturate"] == 1 and out["shifts"] == plain[1]["shifts"] == [1, 1, 1]
    assert np.isfinite(np.array(out["tracking_errors"])).all() and math.isfinite(out["u_excess_peak"]) and out["u_excess_peak"] >= 0
    assert out["tracking_errors"] != plain[1]["tracking_errors"] and out["simulate_mpc"] == plain[1]["simulate_mpc"]
    print(f"u_excess_peak with --u-weight 4: {out['u_excess_peak']:.4g}; with --u-weight 0: {run('--u-max', '40', '--u-weight', '0')[1]['u_excess_peak']:.4g}")
