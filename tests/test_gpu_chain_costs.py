"""GPU: the COST = 1 and COST = 2 instantiations of the KKT and merit kernels (mpcg_generate_kkt_xuref(_f64), mpcg_compute_merit_xuref(_f64)) and the
SATURATE = 1 / CLOCK = 1 instantiations of simulate_kernel (mpcg_simulate with a saturating plant, mpcg_simulate_clk(_f64)) on robots OTHER than the iiwa:
the random chains of tests/chain_models.py, where no table entry the recursions multiply is zero.  tests/test_gpu_xuref.py, test_gpu_limits.py and
test_gpu_clocks.py run these kernels on Plant() alone; tests/test_gpu_chain_plants.py runs the chains through COST = 0 alone.

Every comparison is |got - want| <= limit max(1, max |want array|) per trajectory, want = tests/plant_ref.py on the same chain and on exactly the numbers the
entry sees (tests/chain_cost_cases.py: rounded to float for the float entries, float weights).  No limit is new: each build keeps the one the project
already holds it to on these chains against the same restatement (tests/test_gpu_chain_plants.py).  Every figure is printed, as
`observed (limit)`, before it is asserted; output arrays start NaN-poisoned."""
import functools

import numpy as np
import pytest
import torch

import chain_cost_cases as K
import chain_models as cm
import plant_ref as P
from chain_cost_cases import CASES, COSTS, DT, MU, N4, ROW, STEPS3, case, n, m
from mpcgpu_amd import XuRef, iiwa
from test_gpu_chain_plants import LIMIT_Gg_CHAIN, bits, poison, rel
from test_gpu_kkt_f64 import LIMIT_C, LIMIT_Ggc
from test_gpu_merit_f64 import LIMIT as LIMIT_MERIT_F64
from test_gpu_simulate_f64 import LIMIT_SIM

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NAN = float("nan")
assert DT == iiwa.TIMESTEP
# build: (options, dtype, limit of G and g with ee_cost > 0, with cost "joint", of c, of C, the set it is asserted on)
KKT_BUILDS = {"default": ((), f32, 1e-6, 1e-6, 1e-6, 1e-6, "large"),
              "difference": ((("kkt_analytic", 0),), f32, 3e-6, 3e-6, 3e-6, 3e-6, "modest"),          # on the large set: printed only (tests/test_gpu_chain_plants.py)
              "kkt_f32=1": ((("kkt_f32", 1),), f32, 1e-5, 1e-5, 1e-5, 1e-5, "large"),
              "kkt_f32=2": ((("kkt_f32", 2),), f32, 1e-5, 1e-5, 1e-5, 1e-5, "large"),
              "f64": ((), f64, LIMIT_Gg_CHAIN, LIMIT_Ggc, LIMIT_Ggc, LIMIT_C, "large"),                # 6.9e-9 (the restatement's ee_jac noise) / 8.8e-11 (no Jacobian enters) / 8.8e-11 / 8.9e-7
              "f64 difference": ((("kkt_analytic", 0),), f64, 3e-6, 3e-6, 3e-6, 3e-6, "modest")}
MERIT_BUILDS = {"default": ((), f32, 1e-6), "merit_f32": ((("merit_f32", 1),), f32, 1e-5), "f64": ((), f64, LIMIT_MERIT_F64)}
TOL_SIM = 1e-6                                                # tests/test_gpu_chain_plants.py::test_simulate_vs_host_restatement
SS = {f32: float(np.float32(2e-4)), f64: 2e-4}                # the reference's substep in either type (tests/test_gpu_clocks.py)


def fig(*a):
    print("CHAIN-COST-FIG", *a)


def tdt(dtype):
    return torch.float32 if dtype == f32 else torch.float64


def dev(a, dtype=f32):
    return None if a is None else torch.from_numpy(np.array(a, dtype)).cuda()          # (a copy: the cases' arrays are read-only)


# ---- plants and handles: built once ----
@functools.lru_cache(maxsize=None)
def plant(seed, corruption=None):
    from mpcgpu_amd import Plant
    chain = K.chain(seed)
    return Plant(cm.tables(chain if corruption is None else cm.CORRUPTIONS[corruption](chain)))


def with_limits(base, lim, sim_saturate=False):
    fin = lambda a: [float(v) for v in a]
    return base.with_limits(q=(fin(lim.q_lo), fin(lim.q_hi)), qd=(fin(lim.qd_lo), fin(lim.qd_hi)), u=(fin(lim.u_lo), fin(lim.u_hi)),
                            q_weight=lim.q_weight, qd_weight=lim.qd_weight, u_weight=lim.u_weight, sim_saturate=sim_saturate)


@functools.lru_cache(maxsize=None)
def limits_plant(seed, N, B, size, double, which, corruption=None, gravity=None):
    """The chain plant with the case's own limits: which = "kkt" (from the iterate) or "merit" (from every trial iterate)."""
    cs = case(seed, N, B, size, double)
    base = plant(seed, corruption)
    return with_limits(base if gravity is None else base.with_gravity(gravity), cs.kkt_limits if which == "kkt" else cs.merit_limits)


@functools.lru_cache(maxsize=None)
def solver(N, B, opts=(), integrator=0, sim_integrator=0):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=B)
    for key, v in opts + (("integrator", integrator), ("sim_integrator", sim_integrator)):
        sol.set_option(key, v)
        assert sol.get_option(key) == v
    return sol


def xuref(cs, co, dtype, b=None):
    """The plan and weights of a call on the whole batch, or (b) on trajectory b alone with its own plan."""
    flags = (bool(co.flags & P.QD_RELATIVE), bool(co.flags & P.U_RELATIVE))
    if b is None:
        return XuRef(dev(cs.plan, dtype), dev(cs.offsets, np.int32), cs.stride, co.ee_cost, co.q_cost, *flags, traj_steps=cs.T)
    return XuRef(dev(cs.own_plan(b), dtype), dev(cs.offsets[b:b + 1], np.int32), 0, co.ee_cost, co.q_cost, *flags, traj_steps=cs.T)


def run_kkt(cs, pl, cost, dtype, sol, b=None):
    """One generate_kkt_xuref call (the batch, or trajectory b alone) -> [G, C, g, c] as numpy; the outputs are allocated over NaN and left NaN-filled."""
    co, N = COSTS[cost], cs.N
    sel = slice(None) if b is None else slice(b, b + 1)
    B = len(cs.xu[sel])
    poison([(B, (n * n + m * m) * N - m * m), (B, (n * n + n * m) * (N - 1)), (B, ROW * N - m), (B, n * N)], tdt(dtype))
    out = sol.generate_kkt_xuref(pl, None if co.ee_cost == 0 else dev(cs.goals[sel], dtype), dev(cs.xs[sel], dtype), dev(cs.xu[sel], dtype), DT, co.qd_cost, co.r_cost,
                                 xuref(cs, co, dtype, b))
    torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in out]
    for t in out:
        t.fill_(NAN)
    torch.cuda.synchronize()
    assert all(a.dtype == dtype and np.isfinite(a).all() for a in res), (cs.seed, N, cost)
    return res


def run_merit(cs, pl, cost, dtype, sol, with_xs=True, b=None, mu=MU, steps=STEPS3):
    co = COSTS[cost]
    sel = slice(None) if b is None else slice(b, b + 1)
    out = torch.full((len(cs.xu[sel]), len(steps)), NAN, dtype=tdt(dtype), device="cuda")
    sol.compute_merit_xuref(pl, None if co.ee_cost == 0 else dev(cs.goals[sel], dtype), dev(cs.xs[sel], dtype) if with_xs else None, dev(cs.xu[sel], dtype),
                            dev(cs.dz[sel], dtype), steps, DT, mu, co.qd_cost, co.r_cost, xuref(cs, co, dtype, b), merit=out)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert res.dtype == dtype and np.isfinite(res).all(), (cs.seed, cs.N, cost)
    return res


def worst_per_array(got, want):
    """[G, C, g, c] worst error over the batch, each relative to max(1, |that trajectory's array|)."""
    return [max(rel(got[i][b], want[b][i]) for b in range(len(want))) for i in range(4)]


def rel_each(got, want):
    return float((np.abs(np.asarray(got, f64) - want) / np.maximum(1.0, np.abs(want))).max())


# ---- a, b. mpcg_generate_kkt_xuref(_f64): COST = 1 on the chain plant, COST = 2 on the chain plant with limits ----
@pytest.mark.parametrize("limits", [False, True], ids=["COST=1", "COST=2"])
@pytest.mark.parametrize("seed,N,B", CASES)
def test_kkt_vs_host_restatement(seed, N, B, limits):
    """Every build, both integrators, both costs ("joint": ee_cost = 0 and a NULL goal pointer).  The difference route is asserted on the modest set and
    printed on the large one, as tests/test_gpu_chain_plants.py holds it.  With limits, C and c are bit for bit those of the same call with the plain chain
    plant and G and g are not."""
    failed = []
    for build, (opts, dtype, tol_Gg, tol_Gg_joint, tol_c, tol_C, asserted_on) in KKT_BUILDS.items():
        for size in dict.fromkeys(("large", asserted_on)):
            cs = case(seed, N, B, size, dtype == f64)
            pl = limits_plant(seed, N, B, size, dtype == f64, "kkt") if limits else plant(seed)
            for integrator in (0, 1):
                sol = solver(N, B, opts, integrator)
                for cost in COSTS:
                    got = run_kkt(cs, pl, cost, dtype, sol)
                    err = worst_per_array(got, [cs.want_kkt(b, cost, integrator, limits) for b in range(B)])
                    tol = [tol_Gg_joint if cost == "joint" else tol_Gg, tol_C, tol_Gg_joint if cost == "joint" else tol_Gg, tol_c]
                    held = size == asserted_on
                    fig(f"kkt seed {seed} ({N}, {B}) {size} COST={1 + limits} {build} integrator {integrator} {cost}:",
                        "  ".join(f"{a} {e:.2e} ({t:.1e})" for a, e, t in zip("GCgc", err, tol)), "" if held else "[printed only]")
                    if held and any(e > t for e, t in zip(err, tol)):
                        failed.append((build, size, integrator, cost, err))
                    if limits:
                        base = run_kkt(cs, plant(seed), cost, dtype, sol)
                        assert np.array_equal(bits(got[1]), bits(base[1])) and np.array_equal(bits(got[3]), bits(base[3])), (build, size, integrator, cost)
                        assert not np.array_equal(bits(got[0]), bits(base[0])) and not np.array_equal(bits(got[2]), bits(base[2])), (build, size, integrator, cost)
    assert not failed, failed


# ---- c. mpcg_compute_merit_xuref(_f64) ----
@pytest.mark.parametrize("limits", [False, True], ids=["COST=1", "COST=2"])
@pytest.mark.parametrize("seed,N,B", CASES)
def test_merit_vs_host_restatement(seed, N, B, limits):
    """Step sizes 0, -1, -1/2, d_xs given and NULL, both integrators, both costs: default 1e-6, "merit_f32" 1e-5, the _f64 entry on double inputs 1.2e-13, of
    max(1, |merit|).  With limits every merit lies above the plain one (the penalty is there)."""
    failed = []
    for build, (opts, dtype, limit) in MERIT_BUILDS.items():
        cs = case(seed, N, B, "large", dtype == f64)
        pl = limits_plant(seed, N, B, "large", dtype == f64, "merit") if limits else plant(seed)
        for integrator in (0, 1):
            sol = solver(N, B, opts, integrator)
            for cost in COSTS:
                for with_xs in (True, False):
                    got = run_merit(cs, pl, cost, dtype, sol, with_xs)
                    want = cs.want_merits(cost, with_xs, integrator, limits)
                    err = rel_each(got, want)
                    fig(f"merit seed {seed} ({N}, {B}) COST={1 + limits} {build} integrator {integrator} {cost} xs={with_xs}: merits {want.min():.3g} .. {want.max():.3g}, "
                        f"{err:.2e} ({limit:.1e})")
                    if err > limit:
                        failed.append((build, integrator, cost, with_xs, err))
                    if limits:
                        assert (want > cs.want_merits(cost, with_xs, integrator, False)).all()
    assert not failed, failed


# ---- d. device against device, no restatement ----
@pytest.mark.parametrize("limits", [False, True], ids=["COST=1", "COST=2"])
def test_merit_differences_are_the_kkt_gradient(limits):
    """Seed 1, N = 3, cost "joint" (ee_cost = 0: the cost sum is piecewise quadratic in xu), mu = 0, bounds further than 2 h from every value
    (tests/test_chain_costs_cpu.py): the central differences (h = 1e-3) of ONE compute_merit_xuref_f64 call over the 2 x 56 perturbed copies of a trajectory
    equal g of generate_kkt_xuref_f64 to 1e-9 max(1, |g|) — the assertion and limit of tests/test_gpu_limits.py's test of this name, for each of the five
    trajectories."""
    cs, co = case(1, 3, 5, "large", True), COSTS["joint"]
    N, L, h = cs.N, ROW * cs.N - m, K.H
    pl = with_limits(plant(1), K.far_limits()) if limits else plant(1)
    sol = solver(N, 2 * L)
    worst = 0.0
    for b in range(cs.B):
        ref = lambda count: XuRef(dev(cs.own_plan(b), f64), torch.full((count,), int(cs.offsets[b]), dtype=torch.int32, device="cuda"), 0, 0.0, co.q_cost,
                                  bool(co.flags & P.QD_RELATIVE), bool(co.flags & P.U_RELATIVE), traj_steps=cs.T)
        g = sol.generate_kkt_xuref(pl, None, dev(cs.xs[b:b + 1], f64), dev(cs.xu[b:b + 1], f64), DT, co.qd_cost, co.r_cost, ref(1))[2]
        pert = np.concatenate([cs.xu[b] + h * np.eye(L), cs.xu[b] - h * np.eye(L)])
        mer = torch.full((2 * L, 1), NAN, dtype=torch.float64, device="cuda")
        sol.compute_merit_xuref(pl, None, None, dev(pert, f64), None, [0.0], DT, 0.0, co.qd_cost, co.r_cost, ref(2 * L), merit=mer)
        torch.cuda.synchronize()
        g, mer = g.cpu().numpy()[0], mer.cpu().numpy()[:, 0]
        assert np.isfinite(g).all() and np.isfinite(mer).all()
        err = np.abs((mer[:L] - mer[L:]) / (2 * h) - g).max() / max(1.0, np.abs(g).max())
        fig(f"central differences seed 1 COST={1 + limits} trajectory {b}: |g| up to {np.abs(g).max():.3g}, off by {err:.2e} (1.0e-09)")
        worst = max(worst, err)
        if limits:                                             # the penalty is in g: the plain plant's differs by far more than the limit
            plain = sol.generate_kkt_xuref(plant(1), None, dev(cs.xs[b:b + 1], f64), dev(cs.xu[b:b + 1], f64), DT, co.qd_cost, co.r_cost, ref(1))[2].cpu().numpy()[0]
            assert np.abs(plain - g).max() > 1e-2
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("limits", [False, True], ids=["COST=1", "COST=2"])
def test_kkt_and_merit_measure_the_same_defect(limits, integrator):
    """The _f64 entries, step size 0, d_xs given: merit(mu = 2) - merit(mu = 1) is the 1-norm of the d_c mpcg_generate_kkt_xuref_f64 stores, within
    tests/test_gpu_merit_f64.py's limit of max(1, merit(mu = 2)) — tests/test_gpu_integrator.py::test_kkt_and_merit_are_the_same_map on a chain."""
    seed, N, B = CASES[0]
    cs = case(seed, N, B, "large", True)
    pl = limits_plant(seed, N, B, "large", True, "merit") if limits else plant(seed)
    sol = solver(N, B, (), integrator)
    m2, m1 = (run_merit(cs, pl, "all", f64, sol, mu=mu, steps=[0.0])[:, 0] for mu in (2.0, 1.0))
    c1 = np.abs(run_kkt(cs, pl, "all", f64, sol)[3]).sum(axis=1)
    gap = np.abs((m2 - m1) - c1) / np.maximum(1.0, m2)
    fig(f"same defect seed {seed} COST={1 + limits} integrator {integrator}: |c|_1 {c1.min():.3g} .. {c1.max():.3g}, gap {gap.max():.2e} ({LIMIT_MERIT_F64:.1e})")
    assert c1.min() > 1e-2 and gap.max() <= LIMIT_MERIT_F64, gap


# ---- e. the packed builds do not depend on the batch ----
def test_packed_builds_do_not_depend_on_the_batch():
    """"kkt_f32" = 1 and "merit_f32" = 1, COST = 2, seed 2 at (3, 5): which knot (which step size) shares a lane with which depends on the batch, the arithmetic
    of a half does not — each trajectory alone, with its own plan and offset, has the bits it has inside the batch."""
    seed, N, B = CASES[1]
    cs = case(seed, N, B)
    kkt_pl, merit_pl = limits_plant(seed, N, B, "large", False, "kkt"), limits_plant(seed, N, B, "large", False, "merit")
    packed_kkt, packed_merit = (("kkt_f32", 1),), (("merit_f32", 1),)
    full = run_kkt(cs, kkt_pl, "all", f32, solver(N, B, packed_kkt))
    full_merit = run_merit(cs, merit_pl, "all", f32, solver(N, B, packed_merit))
    for b in range(B):
        for x, y, arr in zip(full, run_kkt(cs, kkt_pl, "all", f32, solver(N, 1, packed_kkt), b=b), "GCgc"):
            assert np.array_equal(bits(x[b]), bits(y[0])), (b, arr)
        assert np.array_equal(bits(full_merit[b]), bits(run_merit(cs, merit_pl, "all", f32, solver(N, 1, packed_merit), b=b)[0])), b


# ---- f, g. simulate: saturating and clocked ----
def simulate(pl, xs, xu, dtype, toff, sim, sim_integrator=0):
    """One mpcg_simulate(_f64) call -> (new state [B, n], end-effector position [B, 3]) as numpy."""
    B = len(xs)
    d_xs, ee = dev(xs, dtype), torch.full((B, 3), NAN, dtype=tdt(dtype), device="cuda")
    solver(N4, B, (), 0, sim_integrator).simulate(pl, d_xs, dev(xu, dtype), DT, toff, sim, SS[dtype], eePos=ee)
    torch.cuda.synchronize()
    return d_xs.cpu().numpy(), ee.cpu().numpy()


def simulate_clk(pl, xs, xu, dtype, times, done=None, sim_integrator=0):
    B = len(xs)
    d_xs, ee = dev(xs, dtype), torch.full((B, 3), NAN, dtype=tdt(dtype), device="cuda")
    solver(N4, B, (), 0, sim_integrator).simulate_clk(pl, d_xs, dev(xu, dtype), DT, dev([t[0] for t in times], f64), dev([t[1] for t in times], f64), SS[dtype],
                                                       eePos=ee, done=done)
    torch.cuda.synchronize()
    return d_xs.cpu().numpy(), ee.cpu().numpy()


def restated_state(xs, xu, dtype, toff, sim, sim_integrator=0):
    return P.simulate(K.chain(1), xs, xu, N4, DT, toff, sim, dtype(SS[dtype]), sim_integrator, double=dtype == f64)


@pytest.mark.parametrize("dtype", [f32, f64], ids=["float", "double"])
@pytest.mark.parametrize("sim_integrator", [0, 1])
def test_simulate_saturates_at_the_torque_limits(sim_integrator, dtype):
    """Chain seed 1, B = 3, a knot crossing and a remainder, u bounds at the thirds of the controls: the state is the restatement's under the clamped controls
    within 1e-6 (float) / tests/test_gpu_simulate_f64.py's limit 3 (double) of max(1, |x|), and bit for bit the plain chain plant's on controls clamped on
    the host (what tests/test_gpu_limits.py holds the saturating simulate to); every trajectory's state differs from the non-saturating plant's."""
    sc = K.sim_case(3, dtype == f64)
    sat, flagless = with_limits(plant(1), sc.limits, sim_saturate=True), with_limits(plant(1), sc.limits)
    tol = TOL_SIM if dtype == f32 else LIMIT_SIM
    got, ee = simulate(sat, sc.xs, sc.xu, dtype, *K.CROSSING, sim_integrator)
    assert np.isfinite(got).all() and np.isfinite(ee).all()
    errs = []
    for b in range(sc.B):
        want = restated_state(sc.xs[b], sc.clamped[b], dtype, *K.CROSSING, sim_integrator)
        err, ee_err = rel_each(got[b], want), np.abs(ee[b] - K.chain(1).ee_pos(want[:7])).max()
        loose = rel_each(got[b], restated_state(sc.xs[b], sc.xu[b], dtype, *K.CROSSING, sim_integrator))
        fig(f"saturating simulate {np.dtype(dtype).name} sim_integrator {sim_integrator} trajectory {b}: state {err:.2e} ({tol:.1e}), eePos {ee_err:.2e}; unclamped restatement off by {loose:.1e}")
        errs.append(err)
        assert loose > 1e-4                                    # the clamp was reached
    on_host, plain = simulate(plant(1), sc.xs, sc.clamped, dtype, *K.CROSSING, sim_integrator), simulate(plant(1), sc.xs, sc.xu, dtype, *K.CROSSING, sim_integrator)
    without_flag = simulate(flagless, sc.xs, sc.xu, dtype, *K.CROSSING, sim_integrator)
    assert max(errs) <= tol, errs
    assert np.array_equal(bits(got), bits(on_host[0])) and np.array_equal(bits(ee), bits(on_host[1]))
    assert np.array_equal(bits(without_flag[0]), bits(plain[0])) and all(not np.array_equal(bits(got[b]), bits(plain[0][b])) for b in range(sc.B))


@pytest.mark.parametrize("saturate", [False, True], ids=["CLOCK=1", "SATURATE=1,CLOCK=1"])
@pytest.mark.parametrize("dtype", [f32, f64], ids=["float", "double"])
def test_simulate_clk_equals_the_scalar_entry_and_the_restatement(dtype, saturate):
    """Chain seed 1, B = 5, a time pair per trajectory — a zero time, a knot crossing with a remainder, ten substeps, three substeps and a remainder, and one
    frozen on entry: each trajectory is bit for bit the scalar entry's batch-of-1 call with its times on the same plant, and within the scalar chain test's
    limit of the restatement; the frozen one and the zero-time one keep their state.  Once on the chain plant, once on the saturating one."""
    sc = K.sim_case(5, dtype == f64)
    pl = with_limits(plant(1), sc.limits, sim_saturate=True) if saturate else plant(1)
    applied = sc.clamped if saturate else sc.xu
    tol = TOL_SIM if dtype == f32 else LIMIT_SIM
    done = dev([int(b == K.FROZEN) for b in range(sc.B)], np.int32)
    got, ee = simulate_clk(pl, sc.xs, sc.xu, dtype, K.TIMES, done)
    assert done.tolist() == [int(b == K.FROZEN) for b in range(sc.B)]
    assert np.array_equal(bits(got[K.FROZEN]), bits(sc.xs[K.FROZEN].astype(dtype))) and np.isnan(ee[K.FROZEN]).all()
    assert np.array_equal(bits(got[0]), bits(sc.xs[0].astype(dtype)))
    errs = []
    for b in range(sc.B):
        if b == K.FROZEN:
            continue
        one, one_ee = simulate(pl, sc.xs[b:b + 1], sc.xu[b:b + 1], dtype, *K.TIMES[b])
        assert np.array_equal(bits(got[b]), bits(one[0])) and np.array_equal(bits(ee[b]), bits(one_ee[0])), b
        want = restated_state(sc.xs[b], applied[b], dtype, *K.TIMES[b])
        err, ee_err = rel_each(got[b], want), np.abs(ee[b] - K.chain(1).ee_pos(want[:7])).max()
        fig(f"simulate_clk {np.dtype(dtype).name} saturate {saturate} trajectory {b} {K.TIMES[b]}: state {err:.2e} ({tol:.1e}), eePos {ee_err:.2e}")
        errs.append(err)
        assert b == 0 or np.abs(got[b] - sc.xs[b]).max() > 1e-4                              # it moved
        if saturate and b != 0:
            assert rel_each(got[b], restated_state(sc.xs[b], sc.xu[b], dtype, *K.TIMES[b])) > 1e-5          # and the clamp was reached
    assert max(errs) <= tol, errs


# ---- h. gravity with limits ----
def test_gravity_with_limits():
    """plant(1).with_gravity((0.5, 0, 9.81)) with limits, the restatement on tests/gravity_ref.py's chain of the same base acceleration: COST = 2 KKT in the
    default build and the _f64 entry, the merit in the default build, at their limits; and gravity is really on — C and c of the limits plant without it are
    off by more than 1e-3."""
    seed, N, B = CASES[0]
    g = K.G_LIMITS
    failed = []
    for build in ("default", "f64"):
        opts, dtype, tol_Gg, _, tol_c, tol_C, _ = KKT_BUILDS[build]
        cs = case(seed, N, B, "large", dtype == f64)
        want = [cs.want_kkt(b, "all", 0, True, gravity=g) for b in range(B)]
        err = worst_per_array(run_kkt(cs, limits_plant(seed, N, B, "large", dtype == f64, "kkt", None, g), "all", dtype, solver(N, B, opts)), want)
        tol = [tol_Gg, tol_C, tol_Gg, tol_c]
        fig(f"gravity with limits kkt {build}:", "  ".join(f"{a} {e:.2e} ({t:.1e})" for a, e, t in zip("GCgc", err, tol)))
        failed += [(build, err)] if any(e > t for e, t in zip(err, tol)) else []
        off = worst_per_array(run_kkt(cs, limits_plant(seed, N, B, "large", dtype == f64, "kkt"), "all", dtype, solver(N, B, opts)), want)
        assert off[1] > 1e-3 and off[3] > 1e-3, off
    cs = case(seed, N, B)
    for with_xs in (True, False):
        got = run_merit(cs, limits_plant(seed, N, B, "large", False, "merit", None, g), "all", f32, solver(N, B), with_xs)
        err = rel_each(got, cs.want_merits("all", with_xs, 0, True, gravity=g))
        fig(f"gravity with limits merit default xs={with_xs}: {err:.2e} (1.0e-06)")
        failed += [("merit", with_xs, err)] if err > 1e-6 else []
    assert not failed, failed


# ---- i. the test of the tests ----
@pytest.mark.parametrize("name", ["Ixy <-> Ixz", "one ET_k transposed"])
def test_a_wrong_table_entry_is_seen_through_these_builds(name):
    """tests/test_gpu_chain_plants.py::test_a_wrong_table_entry_is_seen_on_the_device through COST = 2: the default KKT and merit builds given a chain with ONE
    kind of table entry wrong (still a valid chain: mpcg_plant_create accepts it) against the restatement of the right chain — the worst KKT array is off by
    more than 1e-3 of max(1, |array|) and some merit by more than 1e-3 of max(1, |merit|), a thousand times the limits above."""
    seed, N, B = CASES[0]
    cs = case(seed, N, B)
    off = worst_per_array(run_kkt(cs, limits_plant(seed, N, B, "large", False, "kkt", name), "all", f32, solver(N, B)), [cs.want_kkt(b, "all", 0, True) for b in range(B)])
    merit_off = rel_each(run_merit(cs, limits_plant(seed, N, B, "large", False, "merit", name), "all", f32, solver(N, B)), cs.want_merits("all", True, 0, True))
    fig(f"wrong table ({name}) COST=2: G C g c", " ".join(f"{e:.2e}" for e in off), f"merit {merit_off:.2e}")
    assert max(off) > 1e-3, off
    assert merit_off > 1e-3, merit_off
