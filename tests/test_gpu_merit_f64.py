"""GPU: mpcg_compute_merit_f64, mpcg_line_search_step_f64 and mpcg_line_search_step_rho_f64 (mpcgpu_amd/csrc/merit_plant.hip.h: merit_points_kernel, merit_sum_kernel and line_search_step_kernel in double) — the
double consumers behind mpcg_compute_dz_f64.  The merit: the float entry's arithmetic bit for bit where the float trial iterate is exact; against
tests/plant_ref.py::merit_at at the correctly rounded double trial iterate (plant_ref.trial, double); the accepted merit is the merit of the new
iterate; bit-stability.  The step and the rho rule: tests/rho_ref.py in double, bit for bit.  The closed loop: one whole batched adaptive SQP iteration in
double — generate_kkt_f64 -> form_schur_rhov_f64 -> block_solve_f64 -> compute_dz_f64 -> compute_merit_f64 -> line_search_step_rho_f64 — against
single-trajectory loops and as one captured iteration replayed; the -DUSE_DOUBLES build of examples/sqp_batched_iiwa against the same loop in Python."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import iiwa_ref
import plant_ref as P
import rho_ref
from mpcgpu_amd import _lib, iiwa

pytestmark = pytest.mark.gpu
n, m = 14, 7
STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]          # 0, -1, -1/2, ..., -1/128
STEPS8 = STEPS9[1:]
MU = 10.0
f64 = np.float64


def dev(a, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def env():
    from mpcgpu_amd import PcgSolver, Plant
    return PcgSolver, Plant(), iiwa_ref.Model()


def tail(N):
    return (iiwa.TIMESTEP, MU, iiwa.QD_COST, iiwa.r_cost(N))


def merit_call(sol, plant, N, goals, xs, xu, dz, steps, dtype=np.float64, tl=None):
    B = len(xu)
    return sol.compute_merit(plant, dev(goals.reshape(B, -1), dtype), None if xs is None else dev(xs, dtype), dev(xu, dtype),
                             None if dz is None else dev(dz, dtype), steps, *(tl or tail(N)))


# ---- 1. the float entry's arithmetic ----
def dyadic_case(N, B):
    """xu, dz, xs: multiples of 2^-8 below 2 in magnitude; with step sizes 0 and -1 / 2^p, p <= 7, the trial iterate alpha dz + xu needs 17 bits: the float
    fmaf is exact and equals the double fma.  Goals: floats."""
    rng = np.random.default_rng(40 + N + 100 * B)
    L = (n + m) * N - m
    grid = lambda *shape: rng.integers(-511, 512, shape) / 256.0
    return grid(B, L), grid(B, L), grid(B, n), rng.uniform(-1, 1, (B, N, 6)).astype(np.float32).astype(f64)


STEPS = {1: [-0.25], 9: STEPS9, 16: STEPS9 + [-0.5, -1.0 / 128, 0.0, -1.0, -0.0625, -0.125, -0.25]}
F32_TAIL = lambda N: (iiwa.TIMESTEP, MU, float(np.float32(iiwa.QD_COST)), float(np.float32(iiwa.r_cost(N))))      # costs the float entry can be given


@pytest.mark.parametrize("with_xs", [True, False])
@pytest.mark.parametrize("N,B,As", [(2, 1, (1, 9, 16)), (2, 3, (1, 9, 16)), (3, 1, (1, 9, 16)), (3, 3, (1, 9, 16)), (9, 1, (1, 9, 16)), (9, 3, (1, 9, 16)),
                                    (128, 17, (16,))])
def test_merit_rounded_to_float_is_the_float_entry(env, N, B, As, with_xs):
    """merit64.astype(float32) equals mpcg_compute_merit's merit bitwise: the same point merits in the same order, the float entry rounding the row sum
    once.  (128, 17, 16) = 34,816 items: over the grid cap of 32 x num_cus workgroups of four items, a workgroup runs more than one trip."""
    PcgSolver, plant, _ = env
    xu, dz, xs, goals = dyadic_case(N, B)
    sol = PcgSolver(N, max_batch=B)
    for A in As:
        args = (sol, plant, N, goals, xs if with_xs else None, xu, dz, STEPS[A])
        m32 = merit_call(*args, dtype=np.float32, tl=F32_TAIL(N))
        m64 = merit_call(*args, dtype=np.float64, tl=F32_TAIL(N))
        torch.cuda.synchronize()
        assert m64.dtype == torch.float64 and m64.shape == (B, A) and torch.isfinite(m64).all()
        assert np.array_equal(bits(m64.to(torch.float32)), bits(m32)), (N, B, A)
        assert (m64.to(torch.float32).to(torch.float64) != m64).any()          # the row sums are stored as they are


# ---- 2. against merit_at at the correctly rounded double trial iterate ----
# The limit: ten times the measured worst of the first measured run (below and DESIGN.md §3.12); the margin covers other seeds.
LIMIT = 1.2e-13


@functools.lru_cache(maxsize=None)
def case(N, B):
    """Genuinely double xu and dz (the float test's windows and step, perturbed by 1e-12 relative), float-representable goals and xs, and the host's merits for them — computed once per shape."""
    xu, goals, xs = iiwa.random_windows(N, B, 11 + N)
    rng = np.random.default_rng(1000 + N)
    dz = 0.05 * rng.standard_normal(xu.shape)
    xu = xu.astype(np.float32).astype(f64) * (1.0 + 1e-12 * rng.uniform(-1, 1, xu.shape))
    goals, xs = goals.astype(np.float32).astype(f64), xs.astype(np.float32).astype(f64)
    M = iiwa_ref.Model()
    want = {w: P.merits(M, xu, dz, STEPS9, goals, xs if w else None, N, MU, cost=P.Cost.plain(iiwa.QD_COST, iiwa.r_cost(N)), double=True) for w in (True, False)}
    return xu, goals, xs, dz, want


@pytest.mark.parametrize("with_xs", [True, False])
@pytest.mark.parametrize("N,B", [(2, 1), (3, 2), (8, 3), (9, 1), (32, 2)])
def test_merit_vs_host_restatement(env, N, B, with_xs):
    """|got - want| <= LIMIT max(1, |want|) over the ten cases of tests/test_gpu_merit.py::test_merit_vs_host_restatement, on double inputs.  The float
    entry's 5.4e-8 was its final float rounding; here nothing is rounded behind the double sums.
    Measured worst: 1.15e-14 (N = 8, B = 3, both with and without d_xs); the ten cases 4.6e-16 .. 1.15e-14 — the rounding of double sums over N knots
    of seven shares each, six orders below the float entry."""
    PcgSolver, plant, _ = env
    xu, goals, xs, dz, want = case(N, B)
    sol = PcgSolver(N, max_batch=B)
    got = merit_call(sol, plant, N, goals, xs if with_xs else None, xu, dz, STEPS9).cpu().numpy()
    assert got.dtype == f64 and got.shape == (B, 9) and np.isfinite(got).all()
    w = want[with_xs]
    err = np.abs(got - w) / np.maximum(1.0, np.abs(w))
    print(f"N={N} B={B} xs={with_xs}: merits {w.min():.3g} .. {w.max():.3g}, worst error {err.max():.2e}")
    assert err.max() <= LIMIT, (err.max(), got, w)


# ---- 3. the accepted merit is the merit of the new iterate ----
def test_accepted_merit_is_the_merit_of_the_new_iterate(env):
    """compute_merit_f64 -> line_search_step_f64 -> compute_merit_f64 with step 0 on the new xu: the new merit_ref, bit for bit — the step kernel stores
    the very double the merit kernel evaluated.  Step sizes that are no powers of two: the product alpha dz is not exact, the fma rounds once."""
    PcgSolver, plant, _ = env
    N, B = 8, 3
    xu, goals, xs, dz, _ = case(N, B)
    steps = [-1.0, -0.7, -0.3, -0.1, -1.0 / 3]
    sol = PcgSolver(N, max_batch=B)
    d_xu, d_dz, d_goals, d_xs = dev(xu), dev(dz), dev(goals.reshape(B, -1)), dev(xs)
    merit = sol.compute_merit(plant, d_goals, d_xs, d_xu, d_dz, steps, *tail(N))
    ref = torch.full((B,), float("inf"), device="cuda", dtype=torch.float64)          # anything is better: every trajectory steps
    step = sol.line_search_step(merit, steps, ref, d_dz, d_xu)
    again = sol.compute_merit(plant, d_goals, d_xs, d_xu, None, [0.0], *tail(N))
    torch.cuda.synchronize()
    p = step.cpu().numpy()
    assert (p >= 0).all() and again.dtype == torch.float64
    assert np.array_equal(bits(again)[:, 0], bits(ref))
    assert np.array_equal(ref.cpu().numpy(), merit.cpu().numpy().min(axis=1))
    for b in range(B):
        assert np.array_equal(bits(d_xu)[b], bits(rho_ref.fma(steps[p[b]], dz[b], xu[b]))), b


# ---- 4. bit-stability ----
def test_merit_bits(env):
    """The same call twice; a trajectory inside a batch of 7 and alone; num_steps 1, 9 and 16 for the step sizes they share; a NaN in one trajectory's dz
    stays in that trajectory (and out of its step size 0)."""
    PcgSolver, plant, _ = env
    N, B = 8, 7
    xu, goals, xs = iiwa.random_windows(N, B, 77)
    dz = 0.05 * np.random.default_rng(78).standard_normal(xu.shape)
    sol = PcgSolver(N, max_batch=B)
    call = lambda lo, hi, steps, d=dz: bits(merit_call(sol, plant, N, goals[lo:hi], xs[lo:hi], xu[lo:hi], d[lo:hi], steps))
    full = call(0, B, STEPS9)
    assert np.array_equal(full, call(0, B, STEPS9))
    for b in (0, 3, 6):
        assert np.array_equal(call(b, b + 1, STEPS9)[0], full[b]), b
    assert np.array_equal(call(0, B, [-0.25])[:, 0], full[:, STEPS9.index(-0.25)])
    steps16 = STEPS9 + [-0.75, 0.5, -0.3, 1e-3, -1.0, 0.0, -2.0]
    sixteen = call(0, B, steps16)
    assert np.array_equal(sixteen[:, :9], full)
    assert np.array_equal(sixteen[:, 13], full[:, 1]) and np.array_equal(sixteen[:, 14], full[:, 0])
    bad = dz.copy()
    bad[2, 5 * (n + m) + 3] = np.nan
    got = call(0, B, STEPS9, bad)
    keep = [b for b in range(B) if b != 2]
    assert np.array_equal(got[keep], full[keep])
    assert np.isnan(got[2, 1:].view(f64)).all() and got[2, 0] == full[2, 0]


# ---- 5. the step on synthetic merits ----
SYN_STEPS = [-1.0, -0.3, -0.25, -0.7]                           # two of them no powers of two


@pytest.mark.parametrize("nn,mm", [(14, 7), (6, 3), (1, 1)])
def test_line_search_step_on_synthetic_merits(nn, mm):
    """Ties (the first wins), a value equal to merit_ref (no improvement), NaN rows, a row without improvement; step, merit_ref and every element of xu
    bit for bit against the exactly rounded fma; -1 leaves xu and merit_ref unwritten."""
    from mpcgpu_amd import PcgSolver
    N, B = 4, 6
    L = (nn + mm) * N - mm
    rng = np.random.default_rng(5)
    xu0, dz = rng.standard_normal((B, L)), rng.standard_normal((B, L))
    nan = float("nan")
    merit = np.array([[5, 6, 7, 8], [3, 2, 2, 9], [4, 4, 4, 4], [nan, 3, nan, 1], [nan, nan, nan, nan], [9, 9, 9, 3.5]], f64)
    merit[1, 1:3] = 2.0 + 2.0 ** -40                            # a tie no float can hold
    ref0 = np.full(B, 4.0)
    sol = PcgSolver(N, max_batch=B, state_size=nn, control_size=mm)
    d_xu, d_ref = dev(xu0), dev(ref0)
    step = sol.line_search_step(dev(merit), SYN_STEPS, d_ref, dev(dz), d_xu)
    torch.cuda.synchronize()
    h_xu, h_ref = xu0.copy(), ref0.copy()
    want = rho_ref.step(merit, SYN_STEPS, h_ref, dz, h_xu, dtype=np.float64)
    assert want.tolist() == [-1, 1, -1, 3, -1, 3]
    assert step.dtype == torch.int32 and np.array_equal(step.cpu().numpy(), want)
    assert np.array_equal(bits(d_xu), bits(h_xu)) and np.array_equal(bits(d_ref), bits(h_ref))
    for b in (0, 2, 4):
        assert np.array_equal(bits(d_xu)[b], bits(xu0)[b]) and bits(d_ref)[b] == bits(ref0)[b]


# ---- 6. the rho rule ----
@pytest.mark.parametrize("nn,mm", [(14, 7), (6, 3)])
def test_line_search_step_rho_on_synthetic_merits(nn, mm):
    """14 consecutive calls against tests/rho_ref.py in double after every one (the scenario of tests/test_gpu_rho.py): rho, drho, merit_ref and xu as integer
    views, done and step exact.  Trajectory 0 always fails from rho = 1e-3 and gives up; 1 starts at rho = 5 and gives up at the third call (rho grows
    beyond rho_max: reset, done = 1); 2 always succeeds; 3 alternates; 4 sees NaN rows only; 5 comes frozen by the caller: MPCG_STEP_FROZEN, nothing
    written."""
    from mpcgpu_amd import PcgSolver
    N, B, calls = 4, 6, 14
    L = (nn + mm) * N - mm
    rng = np.random.default_rng(12)
    reset = 0.25
    h = dict(xu=rng.standard_normal((B, L)), ref=np.full(B, 100.0), rho=np.array([1e-3, 5.0, 1e-3, 1e-3, 5e-3, 0.7]),
             drho=np.array([1.0, 1, 1, 1, 1, 3]), done=np.array([0, 0, 0, 0, 0, 3], np.uint8))
    sol = PcgSolver(N, max_batch=B, state_size=nn, control_size=mm)
    d = {k: dev(v.copy(), v.dtype) for k, v in h.items()}
    d_step = torch.zeros(B, dtype=torch.int32, device="cuda")
    frozen_at = {}
    for t in range(calls):
        dz = rng.standard_normal((B, L))
        merit = np.full((B, 4), 200.0)
        merit[2] = [150, 99 - t, 99 - t, 160] if t % 2 else [99 - t, 120, 99.5 - t, 98.5 - t]
        if t % 2:
            merit[3, t % 4] = 99.0 - t
        merit[4] = np.nan
        merit[5] = 1.0
        sol.line_search_step_rho(dev(merit), SYN_STEPS, d["ref"], dev(dz), d["xu"], d["rho"], d["drho"], d["done"], rho_reset=reset, step=d_step)
        torch.cuda.synchronize()
        want = rho_ref.step(merit, SYN_STEPS, h["ref"], dz, h["xu"], h["rho"], h["drho"], h["done"], rho_reset=reset, dtype=np.float64)
        got = d_step.cpu().numpy()
        assert np.array_equal(got, want), (t, got, want)
        for k in h:
            assert np.array_equal(bits(d[k]), bits(h[k])), (t, k, d[k].cpu().numpy(), h[k])
        for b in range(B):
            if h["done"][b] and b not in frozen_at:
                frozen_at[b] = (t, {k: bits(d[k])[b].copy() for k in h})
            elif b in frozen_at:
                assert got[b] == _lib.MPCG_STEP_FROZEN
                for k in h:
                    assert np.array_equal(bits(d[k])[b], frozen_at[b][1][k]), (t, b, k)
    assert {b: t for b, (t, _) in frozen_at.items()} == {0: 9, 1: 2, 5: 0, 4: 8}
    assert h["rho"][0] == reset and h["done"].tolist() == [1, 1, 0, 0, 1, 3] and h["rho"][5] == 0.7
    assert h["rho"][2] == 1e-3 and h["drho"][2] < 0.1
    assert d["rho"].dtype == torch.float64 and (h["drho"][[0, 1]] != h["drho"][[0, 1]].astype(np.float32)).all()      # doubles, not floats widened


def test_step_argument_errors():
    """The float twins' table for mpcg_line_search_step_f64 and mpcg_line_search_step_rho_f64, and for mpcg_compute_merit_f64."""
    from mpcgpu_amd import PcgSolver, Plant
    lib = _lib.load()
    plant = Plant()
    N, B = 4, 2
    sol = PcgSolver(N, max_batch=B)
    L = (n + m) * N - m
    z = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.float64)
    goals, xs, xu, dz, merit, ref = z(B, 6 * N), z(B, n), z(B, L), z(B, L), z(B, 16), z(B)
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    rho, drho = torch.full((B,), 1e-3, device="cuda", dtype=torch.float64), torch.ones(B, device="cuda", dtype=torch.float64)
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    arr = lambda v: (C.c_double * len(v))(*v)

    def cm(h=sol._h, pl=plant._p, cs=7, goals=goals, xs=xs, xu=xu, dz=dz, steps=arr([0.0, -1.0]), A=2, merit=merit, batch=B):
        return lib.mpcg_compute_merit_f64(h, pl, cs, 1 / 64, p(goals), p(xs), p(xu), p(dz), steps, A, 10.0, 1e-4, 1e-4, p(merit), batch, None)

    def ls(h=sol._h, cs=7, merit=merit, steps=arr([-1.0, -0.5]), A=2, ref=ref, dz=dz, xu=xu, step=step, batch=B):
        return lib.mpcg_line_search_step_f64(h, cs, p(merit), steps, A, p(ref), p(dz), p(xu), p(step), batch, None)

    def lr(h=sol._h, cs=7, merit=merit, steps=arr([-1.0, -0.5]), A=2, ref=ref, dz=dz, xu=xu, step=step, rho=rho, drho=drho, done=done,
           factor=1.2, lo=1e-3, hi=10.0, reset=1e-3, batch=B):
        return lib.mpcg_line_search_step_rho_f64(h, cs, p(merit), steps, A, p(ref), p(dz), p(xu), p(step), p(rho), p(drho), p(done), factor, lo, hi, reset,
                                                 batch, None)

    INV, UNS, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_ERR_UNSUPPORTED, _lib.MPCG_OK
    assert cm() == OK and ls() == OK and lr() == OK
    assert cm(xs=None) == OK and cm(dz=None, steps=arr([0.0, -0.0])) == OK
    assert cm(h=None) == INV and cm(pl=None) == INV and ls(h=None) == INV and lr(h=None) == INV
    for kw in ("goals", "xu", "merit", "steps"):
        assert cm(**{kw: None}) == INV, kw
    assert cm(dz=None) == INV
    for kw in ("merit", "steps", "ref", "dz", "xu", "step"):
        assert ls(**{kw: None}) == INV and lr(**{kw: None}) == INV, kw
    for kw in ("rho", "drho", "done"):
        assert lr(**{kw: None}) == INV, kw
    assert b"mpcg_line_search_step_rho_f64: null device pointer" in lib.mpcg_last_error(sol._h)
    big = arr([-1.0] * 17)
    for f in (cm, ls, lr):
        assert f(A=0) == INV and f(steps=big, A=17) == INV and f(steps=arr([-1.0] * 16), A=16) == OK
        assert f(batch=B + 1) == INV
        assert b"max_batch" in lib.mpcg_last_error(sol._h)
        assert f(batch=0) == OK
    assert ls(cs=0) == INV and ls(cs=15) == INV and lr(cs=0) == INV and lr(cs=15) == INV
    assert cm(cs=6) == UNS
    small = PcgSolver(N, max_batch=B, state_size=6, control_size=3)
    assert cm(h=small._h, cs=3) == UNS
    for kw in ("factor", "lo", "hi", "reset"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert lr(**{kw: bad}) == INV, (kw, bad)
    assert lr(factor=1.0) == INV and lr(factor=0.5) == INV and lr(factor=1.0 + 2.0 ** -40) == OK      # (a factor no float tells from 1)
    assert lr(lo=0.0) == INV and lr(lo=-1.0) == INV
    assert lr(lo=2.0, hi=1.0) == INV and lr(lo=2.0, hi=2.0) == OK
    assert lr(reset=0.0) == OK and lr(reset=100.0) == OK
    dev_field = C.cast(plant._p, C.POINTER(C.c_int))
    own = dev_field[0]
    dev_field[0] = own + 1
    try:
        assert cm() == INV
        assert b"different devices" in lib.mpcg_last_error(sol._h)
    finally:
        dev_field[0] = own
    torch.cuda.synchronize()


# ---- 7. the closed loop, all in double ----
ITERS = 4
RHO0 = [1e-3, 5.0, 0.1]
RESET = 2e-3


@functools.lru_cache(maxsize=None)
def loop_inputs():
    N, B = 8, 3
    xu, goals, xs = iiwa.random_windows(N, B, 19)
    return N, B, xu, goals.reshape(B, -1), xs


class Loop:
    """A batched adaptive loop in double on one handle: six calls per iteration, nothing read back."""

    def __init__(self, plant, N, xu, goals, xs, rho0, zero_ref=()):
        from mpcgpu_amd import PcgSolver
        B = len(xu)
        self.sol, self.plant, self.N, self.B = PcgSolver(N, max_batch=B), plant, N, B
        self.goals, self.xs, self.xu = dev(goals), dev(xs), dev(xu)
        self.ref = self.sol.compute_merit(plant, self.goals, self.xs, self.xu, None, [0.0], *tail(N)).reshape(B).clone()
        for b in zero_ref:
            self.ref[b] = 0.0                                   # merits are non-negative and the comparison is strict: every search of b fails
        self.rho = torch.tensor(rho0, dtype=torch.float64, device="cuda")
        self.drho = torch.ones(B, device="cuda", dtype=torch.float64)
        self.done = torch.zeros(B, dtype=torch.uint8, device="cuda")
        self.step = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.lam = torch.zeros(B, n * N, device="cuda", dtype=torch.float64)
        self.names = ("xu", "ref", "rho", "drho", "done", "step")
        torch.cuda.synchronize()
        self.start = {k: getattr(self, k).clone() for k in self.names}

    def iteration(self):
        s, N = self.sol, self.N
        G, Cd, g, c = s.generate_kkt(self.plant, self.goals, self.xs, self.xu, iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(N))
        S, _, gam = s.form_schur(G, Cd, g, c, self.rho, "ss")
        s.block_solve(S, gam, self.lam)
        dz = s.compute_dz(G, Cd, g, self.lam)
        assert dz.dtype == torch.float64
        merit = s.compute_merit(self.plant, self.goals, self.xs, self.xu, dz, STEPS8, *tail(N))
        s.line_search_step_rho(merit, STEPS8, self.ref, dz, self.xu, self.rho, self.drho, self.done, rho_reset=RESET, step=self.step)

    def rewind(self):
        for k in self.names:
            getattr(self, k).copy_(self.start[k])

    def state(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in self.names}


@functools.lru_cache(maxsize=None)
def eager_batched():
    """(the batched loop's state after every eager iteration, its start merit_ref) — computed once, shared by the two tests below."""
    from mpcgpu_amd import Plant
    N, B, xu, goals, xs = loop_inputs()
    loop = Loop(Plant(), N, xu, goals, xs, RHO0, zero_ref=(1,))
    first = loop.state()["ref"]
    states = []
    for _ in range(ITERS):
        loop.iteration()
        states.append(loop.state())
    return states, first


def test_closed_loop_batched_vs_single_trajectory_loops(env):
    """B = 3, N = 8, four adaptive iterations: the batched loop equals three independent single-trajectory loops (max_batch = 1, the same six calls) bit
    for bit — no tolerance.  Trajectory 1 starts at rho = 5 with merit_ref = 0: every search fails, rho grows 6, 8.64, 14.93 > 10: it gives up at the
    third iteration and is frozen in the fourth.  In every iteration the merit decreases or the step is negative and merit_ref stays."""
    _, plant, _ = env
    N, B, xu, goals, xs = loop_inputs()
    got, first = eager_batched()
    final = got[-1]
    for b in range(B):
        one = Loop(plant, N, xu[b:b + 1], goals[b:b + 1], xs[b:b + 1], RHO0[b:b + 1], zero_ref=(0,) if b == 1 else ())
        for it in range(ITERS):
            one.iteration()
            st = one.state()
            for k in one.names:
                assert np.array_equal(bits(st[k])[0], bits(got[it][k])[b]), (b, it, k)
    assert [int(s["step"][1]) for s in got] == [-1, -1, -1, _lib.MPCG_STEP_FROZEN] and final["done"].tolist() == [0, 1, 0]
    assert np.array_equal(bits(final["xu"][1]), bits(np.ascontiguousarray(xu[1]))) and final["rho"][1] == RESET
    prev = first
    for s in got:
        for b in range(B):
            if s["step"][b] >= 0:
                assert s["ref"][b] < prev[b], (b, s["step"][b])
            else:
                assert bits(s["ref"])[b] == bits(prev)[b], b
        prev = s["ref"]
    assert (final["ref"][[0, 2]] < first[[0, 2]]).all() and all(s["xu"].dtype == f64 and s["rho"].dtype == f64 for s in got)
    assert len({float(s["rho"][2]) for s in got}) > 1          # rho moved between iterations


def test_one_captured_iteration_replays_for_the_whole_solve(env):
    """After one eager iteration (the handle-owned buffers of form_schur_f64, block_solve_f64 and compute_merit_f64 exist) the state is rewound and the six
    calls are captured ONCE; four replays from the same start give the eager loop's state after each iteration, bit for bit."""
    _, plant, _ = env
    N, B, xu, goals, xs = loop_inputs()
    want, _ = eager_batched()
    loop = Loop(plant, N, xu, goals, xs, RHO0, zero_ref=(1,))
    loop.iteration()
    torch.cuda.synchronize()
    loop.rewind()
    loop.lam.zero_()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        loop.iteration()
    loop.rewind()
    loop.lam.zero_()
    for it in range(ITERS):
        graph.replay()
        got = loop.state()
        for k in got:
            assert np.array_equal(bits(got[k]), bits(want[it][k])), (it, k)


# ---- 8. the example ----
def example_inputs(B=8, N=32):
    """The inputs of examples/sqp_batched_iiwa.cpp, restated: windows of mpcgpu_amd/data/iiwa_traj_0_0.f32 perturbed by its LCG in float arithmetic."""
    rows = np.fromfile(os.path.join(os.path.dirname(iiwa.__file__), "data", "iiwa_traj_0_0.f32"), np.float32).reshape(400, 27)
    L = (n + m) * N - m
    f32 = np.float32
    xu, goals, xs = np.zeros((B, L), f32), np.zeros((B, N, 6), f32), np.zeros((B, n), f32)
    s = 99

    def rnd():
        nonlocal s
        s = (s * 1664525 + 1013904223) & 0xffffffff
        return f32(f32((s >> 8) & 0xffff) / f32(65536.0) - f32(0.5))

    for b in range(B):
        t0 = (b * 37) % (400 - N)
        for k in range(N):
            r = rows[t0 + k]
            xu[b, k * (n + m):k * (n + m) + n] = r[:n]
            if k < N - 1:
                xu[b, k * (n + m) + n:(k + 1) * (n + m)] = r[n:n + m]
            goals[b, k] = r[n + m:]
        for i in range(n):
            xs[b, i] = f32(xu[b, i] + f32(f32(0.04) * rnd()))
        for e in range(n, L):
            xu[b, e] = f32(xu[b, e] + f32(f32(0.02) * rnd()))
    return xu.astype(f64), goals.reshape(B, -1).astype(f64), xs.astype(f64)


def test_batched_sqp_example_in_double(env):
    """examples/sqp_batched_iiwa_f64 (-DUSE_DOUBLES): builds, runs, every merit goes down — and reports the accepted step exponents, and the merits to the
    last bit, of the same six double calls made from Python on the same inputs (rho = 1e-3, PCG in double to 1e-7)."""
    from mpcgpu_amd import PcgSolver, build, pcg_config
    _, plant, _ = env
    exe = build.build_sqp_batched_f64()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["batch"] == 8 and out["knots"] == 32 and out["iters"] == 4
    merit = np.array(out["merit"])
    assert merit.shape == (8, 5) and (merit[:, -1] < merit[:, 0]).all() and (np.diff(merit, axis=1) <= 0).all()
    B, N, K = 8, 32, 4
    xu, goals, xs = example_inputs(B, N)
    sol = PcgSolver(N, max_batch=B)
    d_xu, d_goals, d_xs = dev(xu), dev(goals), dev(xs)
    tl = (iiwa.TIMESTEP, MU, 1e-4, 1e-4)
    ref = sol.compute_merit(plant, d_goals, d_xs, d_xu, None, [0.0], *tl).reshape(B).clone()
    lam = torch.zeros(B, n * N, device="cuda", dtype=torch.float64)
    hist, expo = [ref.cpu().numpy().copy()], []
    for _ in range(K):
        G, Cd, g, c = sol.generate_kkt(plant, d_goals, d_xs, d_xu, iiwa.TIMESTEP, 1e-4, 1e-4)
        S, Pinv, gam = sol.form_schur(G, Cd, g, c, 1e-3, "ss")
        sol.solve_f64(S, Pinv, gam, lam, pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=3000), "ss")
        dz = sol.compute_dz(G, Cd, g, lam)
        mer = sol.compute_merit(plant, d_goals, d_xs, d_xu, dz, STEPS8, *tl)
        expo.append(sol.line_search_step(mer, STEPS8, ref, dz, d_xu).cpu().numpy().copy())
        hist.append(ref.cpu().numpy().copy())
    assert np.array_equal(np.array(out["exponents"]), np.array(expo).T)
    assert np.array_equal(bits(merit), bits(np.ascontiguousarray(np.array(hist).T)))          # %.17g round-trips a double


# ---- the Python surface ----
def test_python_dispatch_on_dtype(env):
    """float64 tensors reach the _f64 entries (result dtype; the bit checks above); mixed float32 / float64 arguments raise TypeError; float32 calls return
    what they returned before a float64 call on the same solver, bit for bit."""
    PcgSolver, plant, _ = env
    N, B = 8, 3
    xu, goals, xs, dz, _ = case(N, B)
    sol = PcgSolver(N, max_batch=B)
    f = lambda dt: (dev(goals.reshape(B, -1), dt), dev(xs, dt), dev(xu, dt), dev(dz, dt))
    g32, s32, x32, z32 = f(np.float32)
    g64, s64, x64, z64 = f(np.float64)
    before_m = bits(sol.compute_merit(plant, g32, s32, x32, z32, STEPS8, *tail(N)))
    before_k = [bits(t) for t in sol.generate_kkt(plant, g32, s32, x32, iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(N))]
    m64 = sol.compute_merit(plant, g64, s64, x64, z64, STEPS8, *tail(N))
    k64 = sol.generate_kkt(plant, g64, s64, x64, iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(N))
    assert m64.dtype == torch.float64 and all(t.dtype == torch.float64 for t in k64)
    after_m = sol.compute_merit(plant, g32, s32, x32, z32, STEPS8, *tail(N))
    after_k = sol.generate_kkt(plant, g32, s32, x32, iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(N))
    assert after_m.dtype == torch.float32 and np.array_equal(bits(after_m), before_m)
    assert all(np.array_equal(bits(a), b) for a, b in zip(after_k, before_k))
    with pytest.raises(TypeError):
        sol.compute_merit(plant, g64, s64, x64, z32, STEPS8, *tail(N))
    with pytest.raises(TypeError):
        sol.compute_merit(plant, g32, s64, x64, z64, STEPS8, *tail(N))
    with pytest.raises(TypeError):
        sol.compute_merit(plant, g64, None, x64, None, [0.0], *tail(N), merit=torch.zeros(B, 1, device="cuda"))
    ref32, ref64 = torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda", dtype=torch.float64)
    with pytest.raises(TypeError):
        sol.line_search_step(m64, STEPS8, ref32, z64, x64.clone())
    with pytest.raises(TypeError):
        sol.line_search_step(m64, STEPS8, ref64, z32, x64.clone())
    rho, drho, done = torch.ones(B, device="cuda"), torch.ones(B, device="cuda", dtype=torch.float64), torch.zeros(B, dtype=torch.uint8, device="cuda")
    with pytest.raises(TypeError):
        sol.line_search_step_rho(m64, STEPS8, ref64, z64, x64.clone(), rho, drho, done)
    st = sol.line_search_step_rho(m64, STEPS8, ref64, z64, x64.clone(), rho.double(), drho, done)
    torch.cuda.synchronize()
    assert st.dtype == torch.int32
