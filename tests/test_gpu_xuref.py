"""GPU: mpcg_generate_kkt_xuref(_f64) and mpcg_compute_merit_xuref(_f64) — the generalised running cost over a joint-space plan (include/mpcg.h;
mpcgpu_amd/csrc/kkt_plant.hip.h, merit_plant.hip.h, merit_plant_f32.hip.h, COST = 1) — against the float64 restatement tests/plant_ref.py, against the
existing entries where the cost reduces to theirs, against each other on the device (the merit's central differences are the KKT gradient), for
independence of the batch, inside a hipGraph that follows d_traj_offset, and through the error table.  Inputs: iiwa.random_windows; the plan is
random rows of 21."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iiwa_ref
import plant_ref as X
from chain_cost_cases import COSTS                              # "all" (every weight positive, both flags) and "joint" (ee_cost = 0 with a NULL goal pointer)
from mpcgpu_amd import XuRef, _lib, iiwa

pytestmark = pytest.mark.gpu
n, m, NJ, ROW = 14, 7, 7, 21
DT = iiwa.TIMESTEP
MU = 10.0
STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]          # 0, -1, -1/2, ..., -1/128
STEPS8 = STEPS9[1:]
SHAPES = ((2, 1), (3, 2), (5, 3), (8, 3))                     # (2, 1): one block that is first and last; B (N - 1) = 1 and 21 are odd: the packed build has an idle half
# limits of the existing entries' tests: tests/test_gpu_kkt.py (1e-6; 3e-6 with differences; 1e-5 in float arithmetic), tests/test_gpu_kkt_f64.py,
# tests/test_gpu_merit.py (1e-6), tests/test_gpu_merit_f32.py (1e-5), tests/test_gpu_merit_f64.py (1.2e-13) — all relative to max(1, |reference|)
KKT_BUILDS = {"default": ((), 1e-6), "difference": ((("kkt_analytic", 0),), 3e-6), "kkt_f32=1": ((("kkt_f32", 1),), 1e-5), "kkt_f32=2": ((("kkt_f32", 2),), 1e-5)}
LIMIT_Ggc, LIMIT_C = 8.8e-11, 8.9e-7
MERIT_BUILDS = {"default": ((), 1e-6, np.float32), "merit_f32": ((("merit_f32", 1),), 1e-5, np.float32), "f64": ((), 1.2e-13, np.float64)}


def dev(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.array(a, dtype)).cuda()          # (a copy: the cases' arrays are read-only)


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def plant():
    from mpcgpu_amd import Plant
    return Plant()


@functools.lru_cache(maxsize=None)
def model():
    return iiwa_ref.Model()


def solver(N, B, opts=(), integrator=0):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=B)
    for k, v in opts:
        sol.set_option(k, v)
    if integrator:
        sol.set_option("integrator", integrator)
    return sol


class Case:
    """Inputs of one shape, made once and never written to: float32-representable windows (as float64 arrays), a plan of T = N + 1 rows — shared by the
    batch, or (shapes (3, 2) and (5, 3)) one per trajectory at a stride of T + 2 rows with NaN in the two rows between the plans — and offsets
    -1 (clamps at the first row), T - 2 (clamps at the last row from knot 1 on) and 1 (inside)."""

    def __init__(self, N, B, double=False):
        self.N, self.B, self.double = N, B, double
        xu, goals, xs = iiwa.random_windows(N, B, 500 + N)
        rng = np.random.default_rng(900 + N)
        dz = 0.05 * rng.standard_normal(xu.shape)
        self.T = T = N + 1
        self.stride = T + 2 if (N, B) in ((3, 2), (5, 3)) else 0
        plan = 0.5 * rng.standard_normal((B * self.stride if self.stride else T, ROW))
        f32 = lambda a: np.ascontiguousarray(a, np.float32).astype(np.float64)
        arrs = [f32(a) for a in (xu, goals.reshape(B, -1), xs, dz, plan)]
        if double:                                             # genuinely double: none of the values is a float
            arrs = [a * (1.0 + 1e-12 * rng.uniform(-1, 1, a.shape)) for a in arrs]
        self.xu, self.goals, self.xs, self.dz, self.plan = arrs
        if self.stride:
            for b in range(B):
                self.plan[b * self.stride + T:(b + 1) * self.stride] = np.nan
        self.offsets = np.array([-1, T - 2, 1][:B], np.int32)
        for a in arrs + [self.offsets]:
            a.setflags(write=False)
        self._dyn = {}

    def rows(self, b, offsets=None):
        off = self.offsets if offsets is None else offsets
        return X.plan_rows(self.plan, b, off[b], self.N, self.T, self.stride)

    def dynamics(self, b, integrator):
        """The cost-independent part of the restatement (the slow part), once per trajectory and integrator."""
        if (b, integrator) not in self._dyn:
            self._dyn[(b, integrator)] = X.dynamics(model(), self.xu[b], self.goals[b], self.xs[b], self.N, DT, integrator)
        return self._dyn[(b, integrator)]

    def want_kkt(self, b, cost, integrator=0):
        return X.generate_kkt(model(), self.xu[b], None if cost.ee_cost == 0 else self.goals[b], self.xs[b], self.N, rows=self.rows(b), cost=cost, dt=DT, integrator=integrator,
                              base=self.dynamics(b, integrator))

    def xuref(self, cost, dtype, offsets=None, plan=None):
        off = self.offsets if offsets is None else offsets
        return XuRef(dev(self.plan if plan is None else plan, dtype), None if off is None else dev(off, np.int32),
                     self.stride, cost.ee_cost, cost.q_cost, bool(cost.flags & X.QD_RELATIVE), bool(cost.flags & X.U_RELATIVE), traj_steps=self.T)

    def kkt(self, sol, cost, dtype=np.float32, **kw):
        out = sol.generate_kkt_xuref(plant(), None if cost.ee_cost == 0 else dev(self.goals, dtype), dev(self.xs, dtype), dev(self.xu, dtype), DT, cost.qd_cost,
                                     cost.r_cost, self.xuref(cost, dtype, **kw))
        torch.cuda.synchronize()
        return out

    def merit(self, sol, cost, steps, dtype=np.float32, with_xs=True, xu=None, dz="own", **kw):
        out = sol.compute_merit_xuref(plant(), None if cost.ee_cost == 0 else dev(self.goals, dtype), dev(self.xs, dtype) if with_xs else None,
                                      dev(self.xu, dtype) if xu is None else xu, dev(self.dz, dtype) if isinstance(dz, str) else dz, steps, DT, MU, cost.qd_cost,
                                      cost.r_cost, self.xuref(cost, dtype, **kw))
        torch.cuda.synchronize()
        return out


@functools.lru_cache(maxsize=None)
def case(N, B, double=False):
    return Case(N, B, double)


# ---- 1. KKT against the restatement ----
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("build", list(KKT_BUILDS))
@pytest.mark.parametrize("cost", list(COSTS))
@pytest.mark.parametrize("N,B", SHAPES)
def test_kkt_vs_host_restatement(N, B, cost, build, integrator):
    """|got - want| <= tol max(1, max |want array|) for G, C, g, c of every trajectory: both gradient routes and the two float builds, both integrators,
    both cost settings; offsets that clamp at either end of the plan; shared and per-trajectory plans."""
    opts, tol = KKT_BUILDS[build]
    cs, co = case(N, B), COSTS[cost]
    got = [t.cpu().numpy() for t in cs.kkt(solver(N, B, opts, integrator), co)]
    assert all(np.isfinite(a).all() for a in got)
    worst = 0.0
    for b in range(B):
        for a, w, name in zip(got, cs.want_kkt(b, co, integrator), "GCgc"):
            err = np.abs(a[b] - w).max() / max(1.0, np.abs(w).max())
            worst = max(worst, err)
            assert err <= tol, (b, name, err)
    print(f"kkt_xuref N={N} B={B} {cost} {build} integrator={integrator}: worst {worst:.2e} (limit {tol:.0e})")


# ---- 2. the double entry ----
@pytest.mark.parametrize("cost", list(COSTS))
@pytest.mark.parametrize("N,B", [(2, 1), (5, 3)])
def test_double_entry_vs_host_restatement(N, B, cost):
    """mpcg_generate_kkt_xuref_f64 on genuinely double inputs (plan included), held to the limits of tests/test_gpu_kkt_f64.py: G, g, c 8.8e-11, C 8.9e-7
    (the restatement's central differences)."""
    cs, co = case(N, B, True), COSTS[cost]
    assert (cs.plan[np.isfinite(cs.plan)] != cs.plan[np.isfinite(cs.plan)].astype(np.float32)).mean() > 0.9
    got = [t.cpu().numpy() for t in cs.kkt(solver(N, B), co, np.float64)]
    worst = {"Ggc": 0.0, "C": 0.0}
    for b in range(B):
        for a, w, name in zip(got, cs.want_kkt(b, co), "GCgc"):
            key = "C" if name == "C" else "Ggc"
            worst[key] = max(worst[key], np.abs(a[b] - w).max() / max(1.0, np.abs(w).max()))
    print(f"kkt_xuref_f64 N={N} B={B} {cost}: worst G,g,c {worst['Ggc']:.3e}  C {worst['C']:.3e}")
    assert worst["Ggc"] <= LIMIT_Ggc and worst["C"] <= LIMIT_C, worst


@pytest.mark.parametrize("analytic", [1, 0])
@pytest.mark.parametrize("cost", list(COSTS))
@pytest.mark.parametrize("N,B", [(2, 1), (3, 2), (5, 3)])
def test_double_outputs_rounded_to_float_are_the_float_entry(N, B, cost, analytic):
    """Float-representable inputs, plan and weights, timestep 1/64: rounding the double entry's outputs to float gives the float entry's bits."""
    cs, co = case(N, B), COSTS[cost]
    sol = solver(N, B, (("kkt_analytic", analytic),))
    o32, o64 = cs.kkt(sol, co, np.float32), cs.kkt(sol, co, np.float64)
    for a32, a64, name in zip(o32, o64, "GCgc"):
        assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and torch.isfinite(a64).all()
        assert torch.equal(a64.to(torch.float32).view(torch.int32), a32.view(torch.int32)), name


# ---- 3. the reduction to the existing entry ----
@pytest.mark.parametrize("integrator", [0, 1])
@pytest.mark.parametrize("build", list(KKT_BUILDS) + ["f64"])
@pytest.mark.parametrize("N,B", [(2, 1), (5, 3)])
def test_reduces_to_generate_kkt(N, B, build, integrator):
    """ee_cost = 1, q_cost = 0, no flags: mpcg_generate_kkt's numbers (np.array_equal: a -0 may have become +0) in every build, except the seven qd entries
    of q_{N-1}, which are qd_cost qd_{N-1} here (one product, in the build's arithmetic) and qd_cost qd_{N-2} there."""
    opts = KKT_BUILDS[build][0] if build != "f64" else ()
    dtype = np.float64 if build == "f64" else np.float32
    cs = case(N, B)
    qd_cost, r_cost = float(np.float32(iiwa.QD_COST)), float(np.float32(iiwa.r_cost(N)))
    co = X.Cost(1.0, 0.0, qd_cost, r_cost, 0)
    sol = solver(N, B, opts, integrator)
    got = [t.cpu().numpy() for t in cs.kkt(sol, co, dtype)]
    old = sol.generate_kkt(plant(), dev(cs.goals, dtype), dev(cs.xs, dtype), dev(cs.xu, dtype), DT, qd_cost, r_cost)
    torch.cuda.synchronize()
    old = [t.cpu().numpy() for t in old]
    last = slice(ROW * (N - 1) + NJ, ROW * (N - 1) + n)
    qd_last = cs.xu[:, ROW * (N - 1) + NJ:ROW * (N - 1) + n]
    if build.startswith("kkt_f32"):
        want_last = np.float32(qd_cost) * qd_last.astype(np.float32)
    else:
        want_last = (qd_cost * qd_last).astype(dtype)            # float64 inside, rounded on the way out (the double entry: not at all)
    assert np.array_equal(got[2][:, last], want_last)
    if N > 2:
        assert not np.array_equal(got[2][:, last], old[2][:, last])
    got[2][:, last] = old[2][:, last]
    for a, w, name in zip(got, old, "GCgc"):
        assert np.array_equal(a, w), name


# ---- 4. merit against the restatement ----
@functools.lru_cache(maxsize=None)
def want_merits(N, B, cost, with_xs, integrator, double):
    cs, co = case(N, B, double), COSTS[cost]
    return X.merits(model(), cs.xu, cs.dz, STEPS9, None if co.ee_cost == 0 else cs.goals, cs.xs if with_xs else None, N, MU, rows_of=cs.rows, cost=co, dt=DT, integrator=integrator, double=double)


@pytest.mark.parametrize("with_xs", [True, False])
@pytest.mark.parametrize("build", list(MERIT_BUILDS))
@pytest.mark.parametrize("cost", list(COSTS))
@pytest.mark.parametrize("N,B", [(2, 1), (3, 2), (8, 3)])
def test_merit_vs_host_restatement(N, B, cost, build, with_xs):
    """Step sizes 0 and -1/2^p: |got - want| <= limit max(1, |want|), the limits the existing entries are held to (1e-6; 1e-5 with "merit_f32"; 1.2e-13 for the
    double entry on double inputs).  (3, 2) x 9 = 54 items: the last wavefront is partly idle."""
    opts, limit, dtype = MERIT_BUILDS[build]
    double = dtype == np.float64
    cs, co = case(N, B, double), COSTS[cost]
    got = cs.merit(solver(N, B, opts), co, STEPS9, dtype, with_xs).cpu().numpy().astype(np.float64)
    w = want_merits(N, B, cost, with_xs, 0, double)
    assert got.shape == (B, 9) and np.isfinite(got).all()
    err = np.abs(got - w) / np.maximum(1.0, np.abs(w))
    print(f"merit_xuref N={N} B={B} {cost} {build} xs={with_xs}: merits {w.min():.3g} .. {w.max():.3g}, worst {err.max():.2e} (limit {limit:.1e})")
    assert err.max() <= limit, (err.max(), got, w)


@pytest.mark.parametrize("build", list(MERIT_BUILDS))
def test_merit_semi_implicit_integrator(build):
    """"integrator" = 1 reaches the new instantiations too: the violation terms are the semi-implicit step's."""
    opts, limit, dtype = MERIT_BUILDS[build]
    N, B, double = 3, 2, dtype == np.float64
    cs = case(N, B, double)
    got = cs.merit(solver(N, B, opts, 1), COSTS["all"], STEPS9, dtype).cpu().numpy().astype(np.float64)
    w = want_merits(N, B, "all", True, 1, double)
    assert (np.abs(w - want_merits(N, B, "all", True, 0, double)) > 1e-4).any()
    assert (np.abs(got - w) / np.maximum(1.0, np.abs(w))).max() <= limit


@pytest.mark.parametrize("build", list(MERIT_BUILDS))
def test_accepted_merit_is_the_merit_of_the_new_iterate(build):
    """After line_search_step on the _xuref merits, the _xuref merit at step size 0 of the new xu is d_merit_ref bit for bit."""
    opts, _, dtype = MERIT_BUILDS[build]
    N, B = 8, 3
    cs, co = case(N, B), COSTS["all"]
    sol = solver(N, B, opts)
    td = torch.float32 if dtype == np.float32 else torch.float64
    d_xu, d_dz = dev(cs.xu, dtype), dev(cs.dz, dtype)
    merit = cs.merit(sol, co, STEPS8, dtype, xu=d_xu, dz=d_dz)
    ref = torch.full((B,), float("inf"), device="cuda", dtype=td)
    step = sol.line_search_step(merit, STEPS8, ref, d_dz, d_xu)
    again = cs.merit(sol, co, [0.0], dtype, xu=d_xu, dz=None)
    assert (step.cpu().numpy() >= 0).all()
    assert np.array_equal(bits(again)[:, 0], bits(ref))
    assert np.array_equal(ref.cpu().numpy(), merit.cpu().numpy().min(axis=1))


# ---- 5. the two entries agree on the device, in double ----
@pytest.mark.parametrize("flags", [0, X.QD_RELATIVE | X.U_RELATIVE])
def test_merit_differences_are_the_kkt_gradient(flags):
    """ee_cost = 0, mu = 0, N = 4: the cost sum is quadratic in xu, so the central differences (h = 1e-3) of ONE compute_merit_xuref_f64 call over the
    2 x 77 perturbed copies of a trajectory equal g of generate_kkt_xuref_f64 to 1e-9 max(1, |g|) — the last block's joint-space terms included, which
    is why they are evaluated at x_{N-1}."""
    from mpcgpu_amd import PcgSolver
    N, L, h = 4, 77, 1e-3
    cs = case(8, 3, True)                                      # (its first trajectory's first four knots; a shared plan of 9 rows)
    xu = cs.xu[0, :L].copy()
    co = X.Cost(0.0, 0.5, 2.0 ** -6, 2.0 ** -7, flags)
    plan = dev(cs.plan, np.float64)
    sol = PcgSolver(N, max_batch=2 * L)
    ref = lambda B: XuRef(plan, torch.full((B,), 2, dtype=torch.int32, device="cuda"), 0, 0.0, co.q_cost, bool(flags & 1), bool(flags & 2))
    G, _, g, _ = sol.generate_kkt_xuref(plant(), None, dev(cs.xs[:1], np.float64), dev(xu[None], np.float64), DT, co.qd_cost, co.r_cost, ref(1))
    pert = np.concatenate([xu + h * np.eye(L), xu - h * np.eye(L)])
    merit = sol.compute_merit_xuref(plant(), None, None, dev(pert, np.float64), None, [0.0], DT, 0.0, co.qd_cost, co.r_cost, ref(2 * L))
    torch.cuda.synchronize()
    g, merit = g.cpu().numpy()[0], merit.cpu().numpy()[:, 0]
    num = (merit[:L] - merit[L:]) / (2 * h)
    err = np.abs(num - g).max() / max(1.0, np.abs(g).max())
    print(f"flags={flags}: |g| up to {np.abs(g).max():.3g}, central differences off by {err:.2e}")
    assert err <= 1e-9, err
    rows = X.plan_rows(cs.plan, 0, 2, N, cs.T)
    assert np.abs(g - X.generate_kkt(model(), xu, None, cs.xs[0], N, rows=rows, cost=co, base=(np.zeros(0), np.zeros(ROW * N - m), np.zeros(0)))[2]).max() <= 1e-12


# ---- 6. a trajectory's outputs do not depend on the batch ----
@pytest.mark.parametrize("f32", [0, 1])
def test_kkt_does_not_depend_on_the_batch(f32):
    """A trajectory alone and inside a batch of 70, "kkt_f32" = 0 and 1 (two knots per lane: its partner changes), and whatever offsets the others have."""
    N, B = 4, 70
    small = case(8, 3)
    rng = np.random.default_rng(70)
    pick = rng.integers(0, 3, B)
    xu, goals, xs = small.xu[pick, :ROW * N - m], small.goals[pick, :6 * N], small.xs[pick]
    offs = rng.integers(-3, small.T + 2, B).astype(np.int32)
    plan = dev(small.plan)
    co = COSTS["all"]
    sol = solver(N, B, (("kkt_f32", f32),))

    def call(sel, offsets):
        ref = XuRef(plan, torch.from_numpy(np.ascontiguousarray(offsets[sel])).cuda(), 0, co.ee_cost, co.q_cost, True, True)
        out = sol.generate_kkt_xuref(plant(), dev(goals[sel]), dev(xs[sel]), dev(xu[sel]), DT, co.qd_cost, co.r_cost, ref)
        torch.cuda.synchronize()
        return [bits(t) for t in out]
    full = call(slice(0, B), offs)
    others = offs.copy()
    others[np.arange(B) != 37] = rng.integers(-3, small.T + 2, B - 1)
    moved = call(slice(0, B), others)
    for b in (0, 37, 69):
        alone = call(slice(b, b + 1), offs)
        for a, f, name in zip(alone, full, "GCgc"):
            assert np.array_equal(a[0], f[b]), (b, name)
    for f, mv, name in zip(full, moved, "GCgc"):
        assert np.array_equal(f[37], mv[37]), name
    assert not np.array_equal(full[2], moved[2])                  # (the others did move: g follows the rows)


@pytest.mark.parametrize("f32", [0, 1])
def test_merit_does_not_depend_on_the_batch(f32):
    N, B = 4, 70
    small = case(8, 3)
    rng = np.random.default_rng(71)
    pick = rng.integers(0, 3, B)
    L = ROW * N - m
    xu, dz, goals, xs = small.xu[pick, :L], small.dz[pick, :L], small.goals[pick, :6 * N], small.xs[pick]
    offs = rng.integers(-3, small.T + 2, B).astype(np.int32)
    plan = dev(small.plan)
    co = COSTS["all"]
    sol = solver(N, B, (("merit_f32", f32),))

    def call(sel, offsets):
        ref = XuRef(plan, torch.from_numpy(np.ascontiguousarray(offsets[sel])).cuda(), 0, co.ee_cost, co.q_cost, True, True)
        out = sol.compute_merit_xuref(plant(), dev(goals[sel]), dev(xs[sel]), dev(xu[sel]), dev(dz[sel]), STEPS9, DT, MU, co.qd_cost, co.r_cost, ref)
        torch.cuda.synchronize()
        return bits(out)
    full = call(slice(0, B), offs)
    for b in (0, 37, 69):
        assert np.array_equal(call(slice(b, b + 1), offs)[0], full[b]), b
    others = offs.copy()
    others[np.arange(B) != 37] = rng.integers(-3, small.T + 2, B - 1)
    moved = call(slice(0, B), others)
    assert np.array_equal(moved[37], full[37]) and not np.array_equal(moved, full)


# ---- 7. a captured graph follows d_traj_offset ----
def test_graph_follows_the_offsets():
    """The first merit call (it allocates the handle's scratch) is made outside the capture; one KKT + merit call is captured; traj_offset += 1 on the
    device, replay: the outputs are an eager call's at the new offsets, bit for bit — the struct's pointers were copied into the launch, the offsets are
    read when the kernels run."""
    N, B = 5, 3
    cs, co = case(N, B), COSTS["all"]
    sol = solver(N, B)
    goals, xs, xu, dz = (dev(a) for a in (cs.goals, cs.xs, cs.xu, cs.dz))
    off = torch.from_numpy(cs.offsets.copy()).cuda()
    ref = XuRef(dev(cs.plan), off, cs.stride, co.ee_cost, co.q_cost, True, True, traj_steps=cs.T)
    tail = (DT, MU, co.qd_cost, co.r_cost, ref)
    g_merit = torch.zeros(B, 9, device="cuda")
    sol.compute_merit_xuref(plant(), goals, xs, xu, dz, STEPS9, *tail, merit=g_merit)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_kkt = sol.generate_kkt_xuref(plant(), goals, xs, xu, DT, co.qd_cost, co.r_cost, ref)
        sol.compute_merit_xuref(plant(), goals, xs, xu, dz, STEPS9, *tail, merit=g_merit)
    for shift in (0, 1, 2):
        if shift:
            off += 1
        for t in (*g_kkt, g_merit):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        e_kkt = cs.kkt(sol, co, offsets=cs.offsets + shift)
        e_merit = cs.merit(sol, co, STEPS9, offsets=cs.offsets + shift)
        for got, want in zip((*g_kkt, g_merit), (*e_kkt, e_merit)):
            assert torch.isfinite(got).all() and np.array_equal(bits(got), bits(want)), shift
        if shift:
            assert not np.array_equal(bits(g_merit), first)
        first = bits(g_merit).copy()


# ---- 8. the error table ----
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_argument_errors_leave_the_outputs_untouched(prec):
    """Every MPCG_ERR_INVALID row of include/mpcg.h's table, for both calls: nothing is launched, the NaN-filled outputs keep every bit.  MPCG_ERR_UNSUPPORTED
    off 14 x 7; batch == 0 is MPCG_OK and writes nothing either."""
    from mpcgpu_amd import PcgSolver
    lib = _lib.load()
    N, B, T = 4, 2, 5
    td, ct = (torch.float32, C.c_float) if prec == "f32" else (torch.float64, C.c_double)
    sol = PcgSolver(N, max_batch=B)
    L = ROW * N - m
    z = lambda k: torch.zeros(B, k, device="cuda", dtype=td)
    goals, xs, xu, dz, plan = z(6 * N), z(n), z(L), z(L), torch.zeros(T, ROW, device="cuda", dtype=td)
    off = torch.zeros(B, dtype=torch.int32, device="cuda")
    nan = lambda k: torch.full((B, k), float("nan"), device="cuda", dtype=td)
    outs = [nan((n * n + m * m) * N - m * m), nan((n * n + n * m) * (N - 1)), nan(L), nan(n * N), nan(2)]
    keep = [bits(t).copy() for t in outs]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    kkt_fn = lib.mpcg_generate_kkt_xuref if prec == "f32" else lib.mpcg_generate_kkt_xuref_f64
    merit_fn = lib.mpcg_compute_merit_xuref if prec == "f32" else lib.mpcg_compute_merit_xuref_f64
    steps = (ct * 2)(0.0, -1.0)

    def struct(plan=plan, steps_=T, stride=0, off=off, ee=1.0, q=0.5, flags=3):
        return _lib.mpcg_xuref(plan.data_ptr() if plan is not None else None, steps_, stride, off.data_ptr() if off is not None else None, ee, q, flags)

    def both(h=sol._h, pl=plant()._p, cs=7, goals=goals, ref="default", batch=B, **kw):
        r = struct(**kw) if ref == "default" else ref
        rp = C.byref(r) if r is not None else None
        a = kkt_fn(h, pl, cs, DT, p(goals), p(xs), p(xu), 1e-4, 1e-4, rp, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), batch, None)
        b = merit_fn(h, pl, cs, DT, p(goals), p(xs), p(xu), p(dz), steps, 2, MU, 1e-4, 1e-4, rp, p(outs[4]), batch, None)
        return a, b

    INV, UNS, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_ERR_UNSUPPORTED, _lib.MPCG_OK
    inf, nanv = float("inf"), float("nan")
    invalid = [dict(ref=None), dict(plan=None), dict(steps_=0), dict(stride=T - 1), dict(stride=1), dict(ee=-1.0), dict(q=-1e-300), dict(ee=inf), dict(q=nanv),
               dict(ee=nanv), dict(q=inf), dict(flags=4), dict(flags=0x80000001), dict(goals=None), dict(goals=None, ee=1e-300),
               dict(h=None), dict(pl=None), dict(batch=B + 1)]                                # ... and what the parent entries refuse
    for kw in invalid:
        assert both(**kw) == (INV, INV), kw
    assert b"max_batch" in lib.mpcg_last_error(sol._h)
    small = PcgSolver(N, max_batch=B, state_size=6, control_size=3)
    assert both(cs=6) == (UNS, UNS) and both(h=small._h, cs=3) == (UNS, UNS)
    assert both(batch=0) == (OK, OK)
    torch.cuda.synchronize()
    for t, k in zip(outs, keep):
        assert np.array_equal(bits(t), k)
    # and the calls the table allows: NULL goals with ee_cost == 0 (-0 too), NULL offsets, a stride equal to traj_steps with a plan per trajectory
    two = torch.zeros(2 * T, ROW, device="cuda", dtype=td)
    for kw in (dict(), dict(goals=None, ee=0.0), dict(goals=None, ee=-0.0), dict(off=None), dict(plan=two, stride=T), dict(flags=0), dict(q=0.0, ee=0.0, goals=None)):
        assert both(**kw) == (OK, OK), kw
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in outs), kw
        for t in outs:
            t.fill_(float("nan"))


def test_python_layer_type_errors():
    """Mixed dtypes raise TypeError, as simulate does: the plan has the dtype of the other tensors."""
    N, B = 3, 2
    cs, co = case(N, B), COSTS["all"]
    sol = solver(N, B)
    bad = XuRef(dev(cs.plan, np.float64), None, cs.stride, co.ee_cost, co.q_cost, traj_steps=cs.T)
    with pytest.raises(TypeError):
        sol.generate_kkt_xuref(plant(), dev(cs.goals), dev(cs.xs), dev(cs.xu), DT, co.qd_cost, co.r_cost, bad)
    with pytest.raises(TypeError):
        sol.compute_merit_xuref(plant(), dev(cs.goals), dev(cs.xs), dev(cs.xu), None, [0.0], DT, MU, co.qd_cost, co.r_cost, bad)
    good = XuRef(dev(cs.plan), None, cs.stride, co.ee_cost, co.q_cost, traj_steps=cs.T)
    with pytest.raises(TypeError):
        sol.generate_kkt_xuref(plant(), dev(cs.goals), dev(cs.xs, np.float64), dev(cs.xu), DT, co.qd_cost, co.r_cost, good)
    with pytest.raises(ValueError):
        sol.generate_kkt_xuref(plant(), dev(cs.goals), dev(cs.xs), dev(cs.xu), DT, co.qd_cost, co.r_cost, XuRef(dev(cs.plan), None, cs.stride, traj_steps=cs.T + 3))


# ---- 9. the closed loop over the C ABI ----
@pytest.mark.parametrize("double", [False, True], ids=["float", "double"])
def test_closed_loop_example_tracks_the_plan(double):
    """examples/mpc_closed_loop(_f64) --q-cost / --u-relative: the batched run's KKT blocks and merits come from the _xuref entries, the reference rows from each
    trajectory's own plan at the offsets mpcg_advance_horizon advances.  Without the flags the JSON line is what it was; --q-cost 0 --u-relative 0 is the plain run; with
    them every tracking error is finite, every trajectory shifts as before, the batched run differs and simulateMPC (which has no such stage) does not."""
    import json
    import subprocess
    from mpcgpu_amd import build
    exe = build.build_mpc_closed_loop_f64() if double else build.build_mpc_closed_loop()
    small = ("--batch", "3", "--knots", "8", "--updates", "9", "--mpc-steps", "12")

    def run(*flags):
        r = subprocess.run([exe, *small, *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        line = r.stdout.strip().splitlines()[-1]
        return line, json.loads(line)
    plain, off, posture = run(), run("--q-cost", "0", "--u-relative", "0"), run("--q-cost", "0.5", "--u-relative", "1", "--gravity", "9.81")
    heavy = run("--gravity", "9.81")
    assert plain[0] == off[0] and "q_cost" not in plain[1]
    out = posture[1]
    assert out["ok"] is True and out["q_cost"] == 0.5 and out["u_relative"] == 1 and out["shifts"] == plain[1]["shifts"] == [1, 1, 1]
    assert np.isfinite(np.array(out["tracking_errors"])).all()
    assert out["tracking_errors"] != heavy[1]["tracking_errors"] and out["simulate_mpc"] == heavy[1]["simulate_mpc"]
