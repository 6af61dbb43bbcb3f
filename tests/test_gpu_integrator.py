"""GPU: options "integrator" and "sim_integrator" = 1 — semi-implicit (symplectic) Euler, the reference's INTEGRATOR_TYPE == 1 (include/common/integrator.cuh),
as a compile-time parameter of the KKT, merit and simulate kernels (mpcgpu_amd/csrc/kkt_plant.hip.h, merit_plant.hip.h, merit_plant_f32.hip.h, sim_plant.hip.h) —
against the float64 restatement tests/plant_ref.py (pinned in tests/test_integrator_ref_cpu.py, which also shows that the cases here tell the two
integrators apart by 100 x / 10 x their tolerances), across kernels (the merit measures the map the KKT kernel linearised; one simulated step is that map),
in a hipGraph and in a closed SQP iteration; and both options at 0 set explicitly give the bits of a handle on which they were never set.

Every tolerance is the existing one of the same entry and build, by value, relative to max(1, |reference array|) as there."""
import functools
import json
import subprocess

import numpy as np
import pytest
import torch

import chain_models as cm
import iiwa_ref
import plant_ref as P
from mpcgpu_amd import _lib, iiwa

pytestmark = pytest.mark.gpu
n, m = 14, 7
f32, f64 = np.float32, np.float64
NAN = float("nan")
DT = iiwa.TIMESTEP
MU = 10.0
STEPS3 = [0.0, -1.0, -0.5]
STEPS8 = [-1.0 / (1 << p) for p in range(8)]
CHAIN = 2                                # tests/chain_models.py::random_chain(2): every knot of the windows separates the integrators by 100 x (tests/test_integrator_ref_cpu.py)

TOL_KKT = 1e-6                           # tests/test_gpu_kkt.py:55 (analytic), :85
TOL_KKT_DIFFERENCE = 3e-6                # tests/test_gpu_kkt.py:55 ("kkt_analytic" = 0)
TOL_KKT_F32 = 1e-5                       # tests/test_gpu_kkt.py:88 ("kkt_f32" = 1 and 2)
LIMIT_Ggc = 8.8e-11                      # tests/test_gpu_kkt_f64.py::LIMIT_Ggc
LIMIT_C = 8.9e-7                         # tests/test_gpu_kkt_f64.py::LIMIT_C
LIMIT_Gg_CHAIN = cm.KKT_F64_LIMIT_Gg     # tests/test_gpu_chain_plants.py::LIMIT_Gg_CHAIN: G and g of the _f64 entry on a random chain (the restatement's ee_jac noise)
TOL_MERIT = 1e-6                         # tests/test_gpu_merit.py::test_merit_vs_host_restatement
TOL_MERIT_F32 = 1e-5                     # tests/test_gpu_merit_f32.py::TOL
LIMIT_MERIT_F64 = 1.2e-13                # tests/test_gpu_merit_f64.py::LIMIT
TOL_SIM = 1e-6                           # tests/test_gpu_simulate.py::test_simulate_vs_host_restatement
LIMIT_SIM = 5.7e-15                      # tests/test_gpu_simulate_f64.py::LIMIT_SIM
LIMIT_KKT_STEP = 0.0                     # tests/test_gpu_simulate_f64.py::LIMIT_KKT_STEP
F32_ROUNDING = 2.0 ** -24                # tests/test_gpu_simulate_f64.py::F32_ROUNDING
# (options, dtype, tolerance of G g c, tolerance of C) of the six builds of the KKT kernel
KKT_BUILDS = {"default": ({}, f32, TOL_KKT, TOL_KKT), "difference": ({"kkt_analytic": 0}, f32, TOL_KKT_DIFFERENCE, TOL_KKT_DIFFERENCE),
              "kkt_f32=1": ({"kkt_f32": 1}, f32, TOL_KKT_F32, TOL_KKT_F32), "kkt_f32=2": ({"kkt_f32": 2}, f32, TOL_KKT_F32, TOL_KKT_F32),
              "f64": ({}, f64, LIMIT_Ggc, LIMIT_C), "f64 difference": ({"kkt_analytic": 0}, f64, LIMIT_Ggc, LIMIT_C)}
MERIT_BUILDS = {"default": ({}, f32, TOL_MERIT), "merit_f32": ({"merit_f32": 1}, f32, TOL_MERIT_F32), "f64": ({}, f64, LIMIT_MERIT_F64)}


def dev(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rel(got, want):
    return float((np.abs(np.asarray(got, f64) - want) / np.maximum(1.0, np.abs(want))).max())


def rel_block(got, want):
    return float(np.abs(np.asarray(got, f64) - want).max() / max(1.0, np.abs(want).max()))


def fig(*a):
    print("INTEGRATOR-FIG", *a)


# ---- plants, inputs and restatements: built once, never written to ----
@functools.lru_cache(maxsize=None)
def model(which):
    return iiwa_ref.Model() if which == "iiwa" else cm.random_chain(which)


@functools.lru_cache(maxsize=None)
def plant(which):
    from mpcgpu_amd import Plant
    return Plant() if which == "iiwa" else Plant(cm.tables(model(which)))


def solver(N, B, **options):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=B)
    for key, v in options.items():
        sol.set_option(key, v)
        assert sol.get_option(key) == v
    return sol


@functools.lru_cache(maxsize=None)
def inputs(N, B, dtype):
    """(xu, goals [B, 6N], xs, dz) of mpcgpu_amd.iiwa.random_windows(N, B, 5) and a seeded step: float32, or (dtype = f64) genuinely double xu, xs and
    dz — the float32 values times (1 + 1e-12 r), as tests/test_gpu_kkt_f64.py::windows64 — with goals that stay floats."""
    xu, goals, xs = (np.ascontiguousarray(a, f32) for a in iiwa.random_windows(N, B, 5))
    rng = np.random.default_rng([9, N, B])
    dz = (0.05 * rng.standard_normal(xu.shape)).astype(f32)
    goals = goals.reshape(B, -1)
    if dtype == f32:
        return xu, goals, xs, dz
    wide = lambda a: a.astype(f64) * (1.0 + 1e-12 * rng.uniform(-1, 1, a.shape))
    out = wide(xu), goals.astype(f64), wide(xs), wide(dz)
    assert all((a != a.astype(f32)).mean() > 0.9 for a in (out[0], out[2], out[3]))
    return out


@functools.lru_cache(maxsize=None)
def kkt_restated(which, N, B, dtype, integrator):
    xu, goals, xs, _ = (np.asarray(a, f64) for a in inputs(N, B, dtype))
    return [P.generate_kkt(model(which), xu[b], goals[b].reshape(N, 6), xs[b], N, dt=DT, integrator=integrator) for b in range(B)]


@functools.lru_cache(maxsize=None)
def merits_restated(which, N, B, dtype, with_xs, integrator, mu=MU):
    xu, goals, xs, dz = inputs(N, B, dtype)
    if dtype == f64:
        xs = xs.astype(f32)              # (the merit cases give the _f64 entry a float-representable x_s)
    return P.merits(model(which), xu, dz, STEPS3, goals.reshape(B, N, 6), xs if with_xs else None, N, mu, cost=P.Cost.plain(iiwa.QD_COST, iiwa.r_cost(N)), dt=DT,
                    integrator=integrator, double=dtype == f64)


def costs(N, dtype):
    """QD_COST and R_COST as tests/test_gpu_kkt_f64.py gives them: float-rounded to the float entry, the exact doubles to the _f64 entry."""
    return (float(f32(iiwa.QD_COST)), float(f32(iiwa.r_cost(N)))) if dtype == f32 else (iiwa.QD_COST, iiwa.r_cost(N))


def run_kkt(which, N, B, dtype, **options):
    """One generate_kkt call on a fresh handle -> [G, C, g, c] as numpy; the device outputs are left NaN-filled for the next call's allocations."""
    sol = solver(N, B, **options)
    xu, goals, xs, _ = (dev(a, dtype) for a in inputs(N, B, dtype))
    out = sol.generate_kkt(plant(which), goals, xs, xu, DT, *costs(N, dtype))
    torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in out]
    for t in out:
        t.fill_(NAN)
    torch.cuda.synchronize()
    assert all(a.dtype == dtype and np.isfinite(a).all() for a in res), (which, N, B, options)
    return res


def run_merit(which, N, B, dtype, with_xs, mu=MU, steps=STEPS3, **options):
    sol = solver(N, B, **options)
    xu, goals, xs, dz = inputs(N, B, dtype)
    if dtype == f64:
        xs = xs.astype(f32)
    out = torch.full((B, len(steps)), NAN, dtype=torch.float32 if dtype == f32 else torch.float64, device="cuda")
    sol.compute_merit(plant(which), dev(goals, dtype), dev(xs, dtype) if with_xs else None, dev(xu, dtype), dev(dz, dtype), steps, DT, mu, iiwa.QD_COST,
                      iiwa.r_cost(N), merit=out)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.isfinite(res).all(), (which, N, B, options)
    return res


def run_simulate(N, B, dtype, toff, sim, sim_step, xs=None, xu=None, **options):
    """One simulate call on a fresh handle -> (new state, end-effector position) as numpy."""
    sol = solver(N, B, **options)
    if xu is None:
        xu, _, xs, _ = inputs(N, B, dtype)
    d_xs = dev(np.array(xs, copy=True), dtype)
    ee = torch.full((len(xu), 3), NAN, dtype=d_xs.dtype, device="cuda")
    sol.simulate(plant("iiwa"), d_xs, dev(xu, dtype), DT, toff, sim, sim_step, eePos=ee)
    torch.cuda.synchronize()
    return d_xs.cpu().numpy(), ee.cpu().numpy()


# ---- 1. the option table ----
def test_options():
    """Both keys default to 0, take 0 and 1, refuse -1 and 2 with MPCG_ERR_INVALID and a message that names the key (the value stays), and are independent
    of each other, of "kkt_f32" and of "merit_f32"."""
    lib = _lib.load()
    sol = solver(4, 2)
    INV, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_OK
    for key, other in (("integrator", "sim_integrator"), ("sim_integrator", "integrator")):
        assert sol.get_option(key) == 0
        assert lib.mpcg_set_option(sol._h, key.encode(), 1) == OK and sol.get_option(key) == 1 and sol.get_option(other) == 0
        for bad in (-1, 2):
            assert lib.mpcg_set_option(sol._h, key.encode(), bad) == INV
            msg = lib.mpcg_last_error(sol._h)
            assert msg.startswith(key.encode()) and sol.get_option(key) == 1, msg
        sol.set_option("kkt_f32", 2)
        sol.set_option("merit_f32", 1)
        assert sol.get_option(key) == 1 and sol.get_option("kkt_f32") == 2 and sol.get_option("merit_f32") == 1
        sol.set_option("kkt_f32", 0)
        sol.set_option("merit_f32", 0)
        assert sol.get_option(key) == 1
        assert lib.mpcg_set_option(sol._h, key.encode(), 0) == OK and sol.get_option(key) == 0
        assert sol.get_option("kkt_f32") == 0 and sol.get_option("merit_f32") == 0


# ---- 2. mpcg_generate_kkt(_f64) against the restatement ----
# (8, 3); (2, 1): the only block is first and last at once; (8, 5): 35 items — an odd count and one half-empty lane pair in the packed build
@pytest.mark.parametrize("which,N,B", [("iiwa", 8, 3), (CHAIN, 8, 3), ("iiwa", 2, 1), ("iiwa", 8, 5)])
def test_kkt_vs_restatement(which, N, B):
    """"integrator" = 1 in all six builds, all four outputs, each at the tolerance the same build has under explicit Euler.  G and g of the _f64 entry on the
    chain: the limit the same entry has on random chains (the restatement's ee_jac noise at |ee - goal| ~ 1, tests/test_gpu_chain_plants.py) — they do not
    depend on the integrator, and are also held bit-equal to the explicit build's.  The explicit restatement must NOT fit: on the (8, 3) windows, where
    tests/test_integrator_ref_cpu.py has pinned it per knot, C and c are off by more than 100 x the tolerance of 1e-6 (the other shapes print the figure)."""
    for name, (opts, dtype, tol, tol_C) in KKT_BUILDS.items():
        got = run_kkt(which, N, B, dtype, integrator=1, **opts)
        want, other = kkt_restated(which, N, B, dtype, 1), kkt_restated(which, N, B, dtype, 0)
        err = [max(rel_block(got[i][b], want[b][i]) for b in range(B)) for i in range(4)]
        off = [min(rel_block(got[i][b], other[b][i]) for b in range(B)) for i in range(4)]
        fig(f"kkt {which} N {N} B {B} {name}: G C g c", " ".join(f"{e:.2e}" for e in err), "| to the explicit restatement, C c", f"{off[1]:.2e} {off[3]:.2e}")
        tol_Gg = LIMIT_Gg_CHAIN if (dtype == f64 and which != "iiwa") else tol
        assert err[0] <= tol_Gg and err[2] <= tol_Gg and err[3] <= tol and err[1] <= tol_C, (name, err)
        assert (N, B) != (8, 3) or (off[1] > 100 * TOL_KKT and off[3] > 100 * TOL_KKT), (name, off)
        if which != "iiwa":
            explicit = run_kkt(which, N, B, dtype, **opts)
            assert same(got[0], explicit[0]) and same(got[2], explicit[2]), name


def test_integrator_0_set_explicitly_is_the_untouched_handle():
    """Every build of the three entries: the options at 0 set by the caller, and a handle on which they were never set — the same bits."""
    N, B = 8, 3
    for name, (opts, dtype, _, _) in KKT_BUILDS.items():
        for x, y in zip(run_kkt("iiwa", N, B, dtype, **opts), run_kkt("iiwa", N, B, dtype, integrator=0, sim_integrator=0, **opts)):
            assert same(x, y), name
    for name, (opts, dtype, _) in MERIT_BUILDS.items():
        assert same(run_merit("iiwa", N, B, dtype, True, **opts), run_merit("iiwa", N, B, dtype, True, integrator=0, sim_integrator=0, **opts)), name
    for dtype, ss in ((f32, 2e-3), (f64, 2e-3)):
        for x, y in zip(run_simulate(N, B, dtype, 0, 8000, ss), run_simulate(N, B, dtype, 0, 8000, ss, integrator=0, sim_integrator=0)):
            assert same(x, y), dtype
    # and each option is read by its own entries only
    for x, y in zip(run_kkt("iiwa", N, B, f32), run_kkt("iiwa", N, B, f32, sim_integrator=1)):
        assert same(x, y)
    for x, y in zip(run_simulate(N, B, f32, 0, 8000, 2e-3), run_simulate(N, B, f32, 0, 8000, 2e-3, integrator=1)):
        assert same(x, y)


# ---- 3. mpcg_compute_merit(_f64) against the restatement ----
@pytest.mark.parametrize("which,N,B", [("iiwa", 8, 3), (CHAIN, 8, 3), ("iiwa", 2, 1), ("iiwa", 8, 5)])
def test_merit_vs_restatement(which, N, B):
    """"integrator" = 1 in the default build, "merit_f32" = 1 and the _f64 entry; step sizes 0, -1, -1/2; d_xs given and NULL.  How far the explicit restatement is
    off is printed (a sum of absolute values can move either way under dt^2 qdd: test 4 is the assertion that tells the two maps apart)."""
    for name, (opts, dtype, tol) in MERIT_BUILDS.items():
        for with_xs in (True, False):
            got = run_merit(which, N, B, dtype, with_xs, integrator=1, **opts)
            want, other = merits_restated(which, N, B, dtype, with_xs, 1), merits_restated(which, N, B, dtype, with_xs, 0)
            err = rel(got, want)
            off = float((np.abs(got.astype(f64) - other) / np.maximum(1.0, np.abs(other))).min())
            fig(f"merit {which} N {N} B {B} {name} xs={with_xs}: merits {want.min():.3g} .. {want.max():.3g}, worst {err:.2e} | to the explicit restatement at least {off:.2e}")
            assert err <= tol, (name, with_xs, err)
    # the initial-state term is there (the windows start at x_0 = x_s: it shows once the iterate has moved)
    assert (merits_restated(which, N, B, f32, True, 1)[:, 1:] > merits_restated(which, N, B, f32, False, 1)[:, 1:]).all()


# ---- 4. the merit measures the map the KKT kernel linearised ----
@pytest.mark.parametrize("which", ["iiwa", CHAIN])
def test_kkt_and_merit_are_the_same_map(which):
    """The _f64 entries with "integrator" = 1, step size 0, d_xs given: merit(mu = 2) - merit(mu = 1) is the 1-norm of mpcg_generate_kkt_f64's d_c, within
    tests/test_gpu_merit_f64.py's LIMIT of max(1, merit(mu = 2)).  With the option at 0 for one of the two calls the gap exceeds 100 x that limit."""
    N, B = 8, 3
    xu, goals, xs, _ = inputs(N, B, f64)

    def viol(integrator):
        sol = solver(N, B, integrator=integrator)
        args = (plant(which), dev(goals, f64), dev(xs, f64), dev(xu, f64), None, [0.0], DT)
        m2, m1 = (sol.compute_merit(*args, mu, iiwa.QD_COST, iiwa.r_cost(N)).cpu().numpy()[:, 0] for mu in (2.0, 1.0))
        return m2 - m1, m2

    def defect(integrator):
        return np.abs(run_kkt(which, N, B, f64, integrator=integrator)[3]).sum(axis=1)

    (v1, m2), (v0, _) = viol(1), viol(0)
    c1, c0 = defect(1), defect(0)
    gap = np.abs(v1 - c1) / np.maximum(1.0, m2)
    cross = np.minimum(np.abs(v1 - c0), np.abs(v0 - c1)) / np.maximum(1.0, m2)
    fig(f"same map {which}: |c|_1 {c1.tolist()}, gap {gap.max():.2e}, with the options apart at least {cross.min():.2e}")
    assert gap.max() <= LIMIT_MERIT_F64, gap
    assert cross.min() > 100 * LIMIT_MERIT_F64, cross
    assert (np.abs(v0 - c0) / np.maximum(1.0, m2)).max() <= LIMIT_MERIT_F64                       # (and the explicit pair agrees as before)


# ---- 5. mpcg_simulate(_f64) ----
def test_one_step_is_the_kkt_kernels_semi_implicit_step():
    """tests/test_gpu_simulate.py::test_one_step_is_the_kkt_kernels_integrator with "integrator" = "sim_integrator" = 1: mpcg_generate_kkt on [x, u, 0]
    stores c_1 = 0 - step(x, u); one mpcg_simulate substep of dt = timestep is -c_1 to at most one float32 ulp."""
    B = 64
    xu = np.ascontiguousarray(iiwa.random_windows(2, B, 5)[0], f32)
    xu[:, n + m:] = 0.0
    xs = np.ascontiguousarray(xu[:, :n])
    sol = solver(2, B, integrator=1, sim_integrator=1)
    c = sol.generate_kkt(plant("iiwa"), torch.zeros(B, 12, device="cuda"), dev(xs), dev(xu), DT, iiwa.QD_COST, iiwa.r_cost(2))[3]
    d_xs = dev(xs.copy())
    sol.simulate(plant("iiwa"), d_xs, dev(xu), DT, 0, 15625, 1 / 64)
    torch.cuda.synchronize()
    step, kkt = d_xs.cpu().numpy(), -c.cpu().numpy().reshape(B, 2, n)[:, 1]
    gap = np.abs(step.astype(f64) - kkt.astype(f64)) / np.spacing(np.maximum(np.abs(step), np.abs(kkt)))
    explicit = run_simulate(2, B, f32, 0, 15625, 1 / 64, xs=xs, xu=xu)[0]
    fig(f"one step against the KKT kernel, float32 ulps: {gap.max()}, exactly equal {(gap == 0).mean():.2f}; to the explicit step {np.abs(step - explicit).max():.2e}")
    assert np.abs(step - xs).max() > 1e-3 and np.abs(step - explicit)[:, :7].max() > 100 * TOL_SIM
    assert gap.max() <= 1.0, gap.max()


def test_one_step_is_the_double_kkt_kernels_semi_implicit_step():
    """tests/test_gpu_simulate_f64.py::test_one_step_is_the_double_kkt_kernels_integrator with both options at 1: below 2^-24 and below LIMIT_KKT_STEP."""
    B = 64
    xu32 = np.asarray(iiwa.random_windows(2, B, 5)[0], f32).astype(f64)
    xu = xu32 * (1.0 + 1e-12 * np.random.default_rng(45).uniform(-1, 1, xu32.shape))
    xu[:, n + m:] = 0.0
    xs = np.ascontiguousarray(xu[:, :n])
    sol = solver(2, B, integrator=1, sim_integrator=1)
    c = sol.generate_kkt(plant("iiwa"), torch.zeros(B, 12, dtype=torch.float64, device="cuda"), dev(xs, f64), dev(xu, f64), DT, iiwa.QD_COST, iiwa.r_cost(2))[3]
    d_xs = dev(xs.copy(), f64)
    sol.simulate(plant("iiwa"), d_xs, dev(xu, f64), DT, 0, 15625, 1 / 64)
    torch.cuda.synchronize()
    step, kkt = d_xs.cpu().numpy(), -c.cpu().numpy().reshape(B, 2, n)[:, 1]
    assert step.dtype == f64 and kkt.dtype == f64 and np.abs(step - xs).max() > 1e-3
    gap = rel(step, kkt)
    fig(f"one step against the double KKT kernel: {gap:.3e}, exactly equal {(step == kkt).mean():.2f}")
    assert gap < F32_ROUNDING, gap
    assert gap <= LIMIT_KKT_STEP, gap


@pytest.mark.parametrize("dtype", [f32, f64])
def test_simulate_vs_restatement(dtype):
    """sim_step = 2e-3 over 8000 us — the case on which the integrators differ by 1.7e-5 .. 6.0e-5 per trajectory (tests/test_integrator_ref_cpu.py) — under
    "sim_integrator" = 1, both entries: the state within 1e-6 (float) / LIMIT_SIM (double) of max(1, |x|), the end-effector output likewise against the
    kinematics of the restated state."""
    N, B = 8, 3
    tol = TOL_SIM if dtype == f32 else LIMIT_SIM
    xu, _, xs, _ = inputs(N, B, dtype)
    ss = f32(2e-3) if dtype == f32 else 2e-3
    got, ee = run_simulate(N, B, dtype, 0, 8000, float(ss), sim_integrator=1)
    want = np.array([P.simulate(model("iiwa"), xs[b], xu[b], N, DT, 0, 8000, ss, 1, double=dtype == f64) for b in range(B)])
    other = np.array([P.simulate(model("iiwa"), xs[b], xu[b], N, DT, 0, 8000, ss, 0, double=dtype == f64) for b in range(B)])
    assert got.dtype == dtype and np.isfinite(got).all() and np.isfinite(ee).all()
    err = rel(got, want)
    ee_err = max(rel(ee[b], model("iiwa").ee_pos(want[b, :7])) for b in range(B))
    off = min(rel(got[b], other[b]) for b in range(B))
    fig(f"simulate {np.dtype(dtype).name} 2e-3 x 8000 us: state {err:.2e} end effector {ee_err:.2e} | to the explicit restatement at least {off:.2e}")
    assert err <= tol, err
    assert ee_err <= tol, ee_err
    assert off > 10 * TOL_SIM, off


@pytest.mark.parametrize("dtype", [f32, f64])
def test_simulate_zero_time_and_batch_independence(dtype):
    """"sim_integrator" = 1: a zero time leaves d_xs bitwise as it is; a batch of five equals five single calls."""
    N = 4
    xu5, _, xs5, _ = inputs(N, 5, dtype)
    got, _ = run_simulate(N, 5, dtype, 3000, 0, 2e-4, sim_integrator=1)
    assert same(got, xs5)
    ss = float(f32(2e-4)) if dtype == f32 else 2e-4
    full, ee = run_simulate(N, 5, dtype, 15000, 2100, ss, sim_integrator=1)
    assert not same(full, xs5)
    assert not same(full, run_simulate(N, 5, dtype, 15000, 2100, ss)[0])
    for b in range(5):
        one, ee1 = run_simulate(N, 1, dtype, 15000, 2100, ss, xs=xs5[b:b + 1], xu=xu5[b:b + 1], sim_integrator=1)
        assert same(one[0], full[b]) and same(ee1[0], ee[b]), b


# ---- 6. a captured graph keeps the integrator it was captured with ----
def test_capture_keeps_the_integrator():
    N, B = 8, 3
    xu, goals, xs, dz = (dev(a) for a in inputs(N, B, f32))
    sol = solver(N, B, integrator=1)
    tail = (DT, MU, iiwa.QD_COST, iiwa.r_cost(N))
    e_kkt = [t.clone() for t in sol.generate_kkt(plant("iiwa"), goals, xs, xu, DT, iiwa.QD_COST, iiwa.r_cost(N))]
    e_merit = sol.compute_merit(plant("iiwa"), goals, xs, xu, dz, STEPS8, *tail).clone()      # (the first call allocates the handle's scratch: before the capture)
    torch.cuda.synchronize()
    g_merit = torch.zeros(B, 8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_kkt = sol.generate_kkt(plant("iiwa"), goals, xs, xu, DT, iiwa.QD_COST, iiwa.r_cost(N))
        sol.compute_merit(plant("iiwa"), goals, xs, xu, dz, STEPS8, *tail, merit=g_merit)
    sol.set_option("integrator", 0)
    for _ in range(2):
        g_merit.fill_(NAN)
        for t in g_kkt:
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert same(g_merit, e_merit) and all(same(a, b) for a, b in zip(g_kkt, e_kkt))
    now = sol.generate_kkt(plant("iiwa"), goals, xs, xu, DT, iiwa.QD_COST, iiwa.r_cost(N))     # an eager call reads the option as it is now
    torch.cuda.synchronize()
    assert not same(now[1], e_kkt[1]) and not same(now[3], e_kkt[3]) and same(now[0], e_kkt[0])


# ---- 7. a closed SQP iteration, and the examples' flags ----
@pytest.mark.parametrize("dtype", [f32, f64])
def test_closed_sqp_iteration(dtype):
    """KKT -> Schur (SS) -> PCG (1e-7 / 3000) -> dz -> merit -> step with "integrator" = 1, N = 8, B = 3, three iterations, float and double: everything
    finite, merit_ref never increases and ends below its start, and the first merits are the restatement's."""
    from mpcgpu_amd import pcg_config
    N, B = 8, 3
    tdt = torch.float32 if dtype == f32 else torch.float64
    xu, goals, xs, _ = inputs(N, B, dtype)
    if dtype == f64:
        xs = xs.astype(f32).astype(f64)
    sol = solver(N, B, integrator=1)
    cfg = pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=3000)
    d_goals, d_xs, d_xu = dev(goals, dtype), dev(xs, dtype), dev(xu, dtype)
    lam = torch.zeros(B, n * N, dtype=tdt, device="cuda")
    tail = (DT, MU, iiwa.QD_COST, iiwa.r_cost(N))
    d_ref = sol.compute_merit(plant("iiwa"), d_goals, d_xs, d_xu, None, [0.0], *tail).reshape(B).clone()
    hist = [d_ref.cpu().numpy().copy()]
    want = merits_restated("iiwa", N, B, dtype, True, 1)[:, 0]
    first = rel(hist[0], want)
    assert first <= (TOL_MERIT if dtype == f32 else LIMIT_MERIT_F64), first
    for it in range(3):
        G, Cd, g, c = sol.generate_kkt(plant("iiwa"), d_goals, d_xs, d_xu, DT, iiwa.QD_COST, iiwa.r_cost(N))
        S, Pinv, gam = sol.form_schur(G, Cd, g, c, 1e-3, "ss")
        (sol.solve if dtype == f32 else sol.solve_f64)(S, Pinv, gam, lam, cfg, "ss")
        dz = sol.compute_dz(G, Cd, g, lam)
        merit = sol.compute_merit(plant("iiwa"), d_goals, d_xs, d_xu, dz, STEPS8, *tail)
        step = sol.line_search_step(merit, STEPS8, d_ref, dz, d_xu)
        torch.cuda.synchronize()
        for t in (dz, merit, d_xu, d_ref):
            assert torch.isfinite(t).all(), it
        hist.append(d_ref.cpu().numpy().copy())
    hist = np.array(hist)
    fig(f"closed iteration {np.dtype(dtype).name}: first merits {first:.2e} off the restatement, merit_ref per iteration {hist.T.tolist()}, last steps {step.cpu().numpy().tolist()}")
    assert (np.diff(hist, axis=0) <= 0).all() and (hist[-1] < hist[0]).all()


def run_example(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("double", [False, True])
def test_examples_take_the_flags(double):
    """sqp_batched_iiwa(_f64) --integrator 1 and mpc_closed_loop(_f64) --integrator 1 --sim-integrator 1 (the three use_mpcg_* stages with their new trailing
    argument): the runs succeed, the JSON lines carry the values, and the figures differ from the run without the flag, whose line has no such key."""
    from mpcgpu_amd import build
    exe = build.build_sqp_batched_f64() if double else build.build_sqp_batched()
    small = ("--batch", "3", "--knots", "8", "--iters", "2")
    plain, semi = run_example(exe, *small), run_example(exe, *small, "--integrator", "1")
    assert "integrator" not in plain and semi["integrator"] == 1 and plain["ok"] is True and semi["ok"] is True
    a, b = np.array(plain["merit"]), np.array(semi["merit"])
    assert a.shape == b.shape == (3, 3) and (a[:, 0] != b[:, 0]).all()
    exe = build.build_mpc_closed_loop_f64() if double else build.build_mpc_closed_loop()
    small = ("--batch", "3", "--knots", "8", "--updates", "9", "--mpc-steps", "12")
    plain, semi = run_example(exe, *small), run_example(exe, *small, "--integrator", "1", "--sim-integrator", "1")
    assert "integrator" not in plain and "sim_integrator" not in plain and semi["integrator"] == 1 and semi["sim_integrator"] == 1
    assert plain["ok"] is True and semi["ok"] is True and semi["shifts"] == plain["shifts"] == [1, 1, 1]
    assert np.isfinite(semi["simulate_mpc"]["tracking_errors"]).all() and len(semi["simulate_mpc"]["tracking_errors"]) == 12
    assert semi["tracking_errors"] != plain["tracking_errors"] and semi["simulate_mpc"]["tracking_errors"] != plain["simulate_mpc"]["tracking_errors"]
