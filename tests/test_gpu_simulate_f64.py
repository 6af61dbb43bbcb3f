"""GPU: mpcg_simulate_f64 and mpcg_advance_horizon_f64 (mpcgpu_amd/csrc/sim_plant.hip.h: simulate_kernel and advance_horizon_kernel with IO = double) — the step between two SQP
solves with double arrays in and out, which closes the double MPC loop on the device.  The arithmetic is the float entries' (float64 inside): on
float-representable inputs and a shared substep schedule the outputs rounded to float ARE the float entry's bits; on genuinely double inputs nothing
passes through float; against the float64 restatement tests/plant_ref.py in double (pinned in tests/test_sim_ref_f64_cpu.py) and against the double KKT
kernel's integrator the state agrees far below the float rounding this entry removes.  Bit-stability over the batch, runs and graph replays, the
horizon shift bit for bit, a chain that is not the iiwa, the closed loop in double, refusals, the Python dispatch on dtype and the -DUSE_DOUBLES example."""
import ctypes as C
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
from test_gpu_simulate import CASES, five, plan4

pytestmark = pytest.mark.gpu
n, m = 14, 7
N4 = 4
DT = 1.0 / 64
SS = 2e-4                                # integrator.cuh:304 with T = double
SS32 = float(np.float32(2e-4))           # the float entry's substep, as a double
SIM_TEN, SIM_REM = 1999.9999494757503, 122.0703125       # [us] the two schedules the float and the double entry share at SS32 (tests/test_sim_ref_f64_cpu.py)
STEPS8 = [-1.0 / (1 << p) for p in range(8)]
F32_ROUNDING = 2.0 ** -24                # the relative rounding of a float store: what these entries remove
f32, f64 = np.float32, np.float64
NAN = float("nan")

# Worst |got - want| / max(1, |want|) of the new state and the end-effector position against tests/plant_ref.py, ten times the worst figure
# measured over the five schedules of test 3 (the margin covers other seeds, as in tests/test_gpu_kkt_f64.py).  Measured: 5.63e-16 (that test's docstring).
LIMIT_SIM = 5.7e-15
# Worst gap of one step to -c_1 of mpcg_generate_kkt_f64, ten times the measured worst (test 4's docstring).  Measured: 0 — all 896 values equal in every
# bit, as between the float pair of entries: the two kernels run the same statements on the same doubles — and ten times nothing is nothing.
LIMIT_KKT_STEP = 0.0


def dev(a, dtype=f64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def not_a_float(a):
    """The share of entries a float cannot hold."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return float((a.astype(f32).astype(f64) != a).mean())


def rel(got, want):
    return float((np.abs(np.asarray(got, f64) - want) / np.maximum(1.0, np.abs(want))).max())


@functools.lru_cache(maxsize=None)
def plant():
    from mpcgpu_amd import Plant
    return Plant()


@functools.lru_cache(maxsize=None)
def model():
    return iiwa_ref.Model()


@functools.lru_cache(maxsize=None)
def solver(N, B, state_size=14, control_size=None):
    from mpcgpu_amd import PcgSolver
    return PcgSolver(N, max_batch=B, state_size=state_size, control_size=control_size)


def doubles(a, seed):
    """Genuinely double values, as tests/test_gpu_kkt_f64.py::windows64: the float32 values times (1 + 1e-12 r), r uniform in [-1, 1]."""
    a = np.asarray(a, f32).astype(f64)
    out = a * (1.0 + 1e-12 * np.random.default_rng(seed).uniform(-1, 1, a.shape))
    assert not_a_float(out[out != 0]) > 0.9
    return out


@functools.lru_cache(maxsize=None)
def five64():
    xu, xs = five()
    return doubles(xu, 41), doubles(xs, 42)


def simulate(B, xs, xu, toff, sim, ss, dtype=f64, ee=True, N=N4, pl=None):
    """One simulate call -> (new xs, eePos) as numpy; the outputs start NaN-filled (eePos) / as the inputs (xs)."""
    d_xs = dev(xs, dtype)
    d_ee = torch.full((B, 3), NAN, dtype=d_xs.dtype, device="cuda") if ee else None
    solver(N, B).simulate(plant() if pl is None else pl, d_xs, dev(xu, dtype), DT, toff, sim, ss, eePos=d_ee)
    torch.cuda.synchronize()
    return d_xs.cpu().numpy(), (d_ee.cpu().numpy() if ee else None)


# ---- 1. rounded to float it is the float entry ----
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("toff,sim", [(15000, SIM_TEN), (15000, SIM_REM)])
def test_outputs_rounded_to_float_are_the_float_entry(toff, sim, B):
    """Inputs that are floats widened, the substep (double)2e-4f and the two schedules whose remainder is the same in float and in double: ten full
    substeps and none (with the offset of 15,000 us they cross from knot 0 to knot 1), and no full substep and a remainder of 2^-13 s.  B = 5 is no
    multiple of a wavefront's four trajectories."""
    S32, idx32, rem32, _ = P.schedule(toff, sim, DT, f32(2e-4))
    assert P.schedule(toff, sim, DT, SS32, double=True)[:3] == (S32, idx32, float(rem32))      # the same schedule in both entries
    xu, xs = (a[:B] for a in five())
    xs32, ee32 = simulate(B, xs, xu, toff, sim, SS32, f32)
    xs64, ee64 = simulate(B, xs, xu, toff, sim, SS32, f64)
    assert xs64.dtype == f64 and ee64.dtype == f64 and np.isfinite(xs64).all() and np.isfinite(ee64).all()
    assert not same(xs32, xs)
    assert same(xs64.astype(f32), xs32) and same(ee64.astype(f32), ee32)
    share = not_a_float(np.concatenate([xs64.reshape(-1), ee64.reshape(-1)]))
    print(f"toff {toff} sim {sim} B {B}: {share:.2f} of the double outputs are no floats")
    assert share > 0.3, share


# ---- 2. double inputs are used as they are ----
def test_double_inputs_are_used_as_they_are():
    """Copies show it bit for bit: sim_time_us = 0 leaves xs as it is, and advance_horizon(shift = False) makes xu[:, :14] the same doubles — through
    float either would be the rounded values."""
    xu, xs = five64()
    assert not same(xs.astype(f32).astype(f64), xs)            # squeezed through float the values would differ
    got, _ = simulate(5, xs, xu, 4000, 0, SS, ee=False)
    assert same(got, xs)
    d_xu = dev(xu)
    solver(N4, 5).advance_horizon(False, d_xu, dev(xs))
    torch.cuda.synchronize()
    assert same(d_xu[:, :n], xs) and same(d_xu[:, n:], xu[:, n:])
    assert not same(d_xu[:, :n].cpu().numpy().astype(f32).astype(f64), xs)


# ---- 3. against the float64 restatement, the reference's double schedule ----
@functools.lru_cache(maxsize=None)
def plan4_64():
    xu, xs = plan4()
    return doubles(xu, 43), doubles(xs, 44)


def clamped_schedule(toff, sim, recompute=False, ignore=False):
    S, idx, rem, ridx = P.schedule(toff, sim, DT, SS, double=True)
    if recompute:
        ridx = int((toff * 1e-6 + S * SS) / DT)
    if ignore:
        idx, ridx = [int(toff * 1e-6 / DT)] * S, int(toff * 1e-6 / DT)
    return [min(i, N4 - 2) for i in idx], (min(ridx, N4 - 2) if rem != 0 else None)


@pytest.mark.parametrize("toff,sim", CASES)
def test_simulate_vs_host_restatement(toff, sim):
    """The five schedules of tests/test_gpu_simulate.py::CASES at the reference's double substep 2e-4 (at 2,000 us: ten substeps and a remainder of almost a
    whole one), on double inputs.  The plan is a view into a larger NaN-filled buffer: an index beyond the last control that was not clamped reads NaN.
    Where the schedule of a WRONG alternative (remainder index recomputed at its own time; the crossing ignored) differs from the right one, its result
    is more than 1e-4 away.  The state and the end-effector position, relative to max(1, |value|): below 2^-24 — the float rounding this entry
    removes — whatever was measured, and below LIMIT_SIM = ten times the measured worst.
    Measured on the MI355X, state / end effector: (0, 2000) 1.11e-16 / 1.88e-16, (15000, 2100) 1.11e-16 / 3.75e-16, (15000, 100) 0 / 1.88e-16, (46000, 2000)
    3.10e-16 / 5.63e-16, (15500, 300) 1.39e-17 / 3.75e-16: worst 5.63e-16 (the float entry against its restatement: 4.2e-8)."""
    xu, xs = plan4_64()
    big = torch.full((len(xu) + 64,), NAN, dtype=torch.float64, device="cuda")
    view = big[16:16 + len(xu)]
    view.copy_(dev(xu))
    d_xs, ee = dev(xs.copy()), torch.full((3,), NAN, dtype=torch.float64, device="cuda")
    solver(N4, 1).simulate(plant(), d_xs, view, DT, toff, sim, SS, eePos=ee)
    torch.cuda.synchronize()
    got, ee = d_xs.cpu().numpy(), ee.cpu().numpy()
    want = P.simulate(model(), xs, xu, N4, DT, toff, sim, SS, double=True)
    assert np.isfinite(got).all() and np.isfinite(ee).all()
    err, ee_err = rel(got, want), rel(ee, model().ee_pos(want[:7]))
    print(f"SIM64-FIG toff {toff} sim {sim}: worst relative error {err:.3e}, end effector {ee_err:.3e}")
    for flag in ("recompute_remainder_index", "ignore_crossing"):
        kw = {"recompute": flag[0] == "r", "ignore": flag[0] == "i"}
        if clamped_schedule(toff, sim, **kw) != clamped_schedule(toff, sim):
            other = P.simulate(model(), xs, xu, N4, DT, toff, sim, SS, double=True, **{flag: True})
            assert np.abs(other - want).max() > 1e-4, flag
    assert max(err, ee_err) < F32_ROUNDING, (err, ee_err)
    assert LIMIT_SIM <= F32_ROUNDING and max(err, ee_err) <= LIMIT_SIM, (err, ee_err)


def test_the_cases_tell_both_wrong_schedules_apart():
    right = [clamped_schedule(*c) for c in CASES]
    assert any(clamped_schedule(*c, recompute=True) != r for c, r in zip(CASES, right))
    assert any(clamped_schedule(*c, ignore=True) != r for c, r in zip(CASES, right))
    assert clamped_schedule(46000, 2000) == ([2] * 10, 2)                       # the clamp case, and the quirk: a remainder substep behind ten full ones
    assert clamped_schedule(0, 2000) == ([0] * 10, 0)


# ---- 4. one step is the double KKT kernel's integrator ----
def test_one_step_is_the_double_kkt_kernels_integrator():
    """mpcg_generate_kkt_f64 on [x, u, 0] (N = 2) stores c_1 = 0 - (x + dt f(x, u)); one mpcg_simulate_f64 step of the same dt is -c_1 up to summation
    noise in double (the float pair of entries agrees to one float ulp: two roundings of such values).  Relative to max(1, |value|): below 2^-24 whatever was
    measured, and below LIMIT_KKT_STEP = ten times the measured worst.
    Measured worst over the 64 windows on the MI355X: 0 (all 896 values equal in every bit)."""
    B = 64
    xu_w, _, _ = iiwa.random_windows(2, B, 5)
    xu = doubles(xu_w, 45)
    xu[:, n + m:] = 0.0
    xs = np.ascontiguousarray(xu[:, :n])
    sol = solver(2, 64)
    goals = torch.zeros(B, 12, dtype=torch.float64, device="cuda")
    _, _, _, c = sol.generate_kkt(plant(), goals, dev(xs), dev(xu), DT, iiwa.QD_COST, iiwa.r_cost(2))
    d_xs = dev(xs.copy())
    sol.simulate(plant(), d_xs, dev(xu), DT, 0, 15625, 1 / 64)
    torch.cuda.synchronize()
    step, kkt = d_xs.cpu().numpy(), -c.cpu().numpy().reshape(B, 2, n)[:, 1]
    assert step.dtype == f64 and kkt.dtype == f64 and np.abs(step - xs).max() > 1e-3
    gap = rel(step, kkt)
    print(f"SIM64-FIG worst gap to the double KKT kernel's integrator: {gap:.3e}, exactly equal: {(step == kkt).mean():.2f}")
    assert gap < F32_ROUNDING, gap
    assert LIMIT_KKT_STEP <= F32_ROUNDING and gap <= LIMIT_KKT_STEP, gap


# ---- 5. bits ----
def test_batch_of_five_equals_five_single_calls_and_runs_repeat():
    xu, xs = five64()
    out = [simulate(5, xs, xu, 15000, 2100, SS) for _ in range(2)]
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1])
    assert not same(out[0][0], xs)
    for b in range(5):
        one = simulate(1, xs[b:b + 1], xu[b:b + 1], 15000, 2100, SS)
        assert same(one[0], out[0][0][b:b + 1]) and same(one[1], out[0][1][b:b + 1]), b


class Mpc:
    """tests/test_gpu_simulate.py::Mpc with every tensor float64: device state of B trajectories of an MPC loop at horizon N over per-trajectory plans cut
    from the reference trajectory (floats, widened)."""

    def __init__(self, N, starts, T, perturb=0.02, seed=1, ss=SS):
        d = np.load(iiwa.TRAJ_FIXTURE)
        B = len(starts)
        self.N, self.B, self.T, self.ss = N, B, T, ss
        self.sol = solver(N, B)
        self.plan = dev([d["xu"][t:t + T] for t in starts])                       # [B, T, 21]
        self.plan_goals = dev([d["eepos"][t:t + T] for t in starts])              # [B, T, 6]
        L = (n + m) * N - m
        self.xu = self.plan[:, :N].reshape(B, -1)[:, :L].clone()
        self.xu_old = self.xu.clone()
        self.goals = self.plan_goals[:, :N].reshape(B, -1).clone()
        noise = np.array([np.random.default_rng(seed + t).standard_normal(n) for t in starts])
        self.xs = dev(self.xu[:, :n].cpu().numpy() + perturb * noise)
        self.lam = torch.zeros(B, n * N, dtype=torch.float64, device="cuda")
        self.ee = torch.zeros(B, 3, dtype=torch.float64, device="cuda")
        self.offset = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.err = torch.full((B,), NAN, dtype=torch.float64, device="cuda")

    def simulate(self, toff, sim):
        self.sol.simulate(plant(), self.xs, self.xu_old, DT, toff, sim, self.ss, eePos=self.ee)
        self.xu_old.copy_(self.xu)                                                # (mpcsim.cuh:291)

    def advance(self, shift, lead=0):
        self.sol.advance_horizon(shift, self.xu, self.xs, self.lam, self.goals, self.ee, self.plan, self.plan_goals, self.offset, self.done,
                                 self.err, xu_fill_lead=lead)

    def state(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("xu", "xu_old", "xs", "lam", "goals", "ee", "offset", "done", "err")}


@pytest.mark.parametrize("shift", [True, False])
def test_captured_simulate_and_advance_replay_the_eager_steps(shift):
    """simulate_f64 -> advance_horizon_f64 captured ONCE on a fresh pair of calls and replayed three times is three eager steps, bit for bit, with either
    shift value: both calls are pure stream work."""
    make = lambda: Mpc(N4, (2, 150, 300, 40, 200), 12)
    eager = make()
    want = []
    for _ in range(3):
        eager.simulate(1000, 2100)
        eager.advance(shift)
        want.append(eager.state())
    assert want[-1]["offset"].tolist() == [3 if shift else 0] * 5 and not same(want[0]["xs"], want[1]["xs"])
    assert same(want[-1]["xu"][:, :n], want[-1]["xs"])
    rep = make()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        rep.simulate(1000, 2100)
        rep.advance(shift)
    rep2 = make()                                              # (capture runs nothing: the state is still the initial one)
    assert all(same(a, b) for a, b in zip(rep.state().values(), rep2.state().values()))
    for i in range(3):
        graph.replay()
        got = rep.state()
        for k in got:
            assert same(got[k], want[i][k]), (i, k)


# ---- 6. advance_horizon_f64 bit for bit against the restatement ----
def advance_case(N, shared, lead, shift=True, dtype=f64):
    """tests/test_gpu_simulate.py::advance_case in `dtype`; float64: genuinely double values."""
    B, T = 4, N + 6
    rng = np.random.default_rng(100 * N + 10 * shared + lead)
    f = lambda *s: rng.standard_normal(s).astype(f32).astype(dtype) if dtype == f32 else rng.standard_normal(s)
    L = (n + m) * N - m
    plan, goals = (f(T, n + m), f(T, 6)) if shared else (f(B, T, n + m), f(B, T, 6))
    h = {"xu": f(B, L), "lam": f(B, n * N), "goal": f(B, 6 * N), "xs": f(B, n), "ee": f(B, 3)}
    # inside the plan; exactly offset + N == T after the increment (the else branch); reaches T (done becomes 1); frozen on entry
    off0 = np.array([0, T - N - 1, T - 1, 2], np.int32)
    done0 = np.array([0, 0, 0, 7], np.int32)
    d = {k: dev(v, dtype) for k, v in h.items()}
    d_off, d_done = torch.from_numpy(off0).cuda(), torch.from_numpy(done0).cuda()
    d_err = torch.full((B,), NAN, dtype=d["xu"].dtype, device="cuda")
    solver(N, B).advance_horizon(shift, d["xu"], d["xs"], d["lam"], d["goal"], d["ee"], dev(plan, dtype), dev(goals, dtype), d_off, d_done, d_err,
                                 xu_fill_lead=lead)
    torch.cuda.synchronize()
    for b in range(B):
        p, g = (plan, goals) if shared else (plan[b], goals[b])
        xu, lam, goal, off, done, err = P.advance(shift, N, h["xu"][b], h["lam"][b], h["goal"][b], h["xs"][b], h["ee"][b], p, g, T, int(off0[b]),
                                                  int(done0[b]), lead, dtype)
        assert same(d["xu"][b], xu) and same(d["lam"][b], lam) and same(d["goal"][b], goal), (b, N, shared, lead)
        assert int(d_off[b]) == off and int(d_done[b]) == done, (b, int(d_off[b]), int(d_done[b]))
        if err is None:
            assert np.isnan(d_err[b].item())
        else:
            assert same(d_err[b:b + 1], np.array([err], dtype)), b
    assert same(d["xs"], h["xs"]) and same(d["ee"], h["ee"])
    if shift:
        assert d_done.tolist() == [0, 0, 1, 7] and d_off.tolist() == [1, T - N, T, 2]
        assert same(d["xu"][3], h["xu"][3]) and same(d["lam"][3], h["lam"][3]) and same(d["goal"][3], h["goal"][3])       # frozen: nothing of it is written
    return d, h


@pytest.mark.parametrize("N", [4, 2])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("lead", ["0", "N-1"])
def test_advance_horizon_shift_vs_restatement(N, shared, lead):
    """A shared and a per-trajectory plan; both fill rows; an offset inside the plan, one taking the else branch, one using the plan up (done is set) and
    a frozen trajectory of which nothing is written.  The tracking error is the restatement's double, bit for bit."""
    d, h = advance_case(N, shared, 0 if lead == "0" else N - 1)
    assert not_a_float(h["xu"]) > 0.9 and not_a_float(d["lam"]) > 0.9


def test_advance_horizon_long_horizon_sweeps_in_chunks():
    """N = 128: xu (2,681 doubles) and lambda (1,792) are longer than one sweep chunk of 2,048 elements — the kernel's second trip through load, barrier, store."""
    advance_case(128, False, 127)


def test_advance_horizon_on_float_inputs_is_the_float_entry_widened():
    for N, shared, lead in ((4, True, 0), (4, False, 3)):
        d32, _ = advance_case(N, shared, lead, dtype=f32)
        rng = np.random.default_rng(100 * N + 10 * shared + lead)              # advance_case's inputs again, widened
        B, T, L = 4, N + 6, (n + m) * N - m
        f = lambda *s: rng.standard_normal(s).astype(f32).astype(f64)
        plan, goals = (f(T, n + m), f(T, 6)) if shared else (f(B, T, n + m), f(B, T, 6))
        h = {"xu": f(B, L), "lam": f(B, n * N), "goal": f(B, 6 * N), "xs": f(B, n), "ee": f(B, 3)}
        d64 = {k: dev(v) for k, v in h.items()}
        off = torch.from_numpy(np.array([0, T - N - 1, T - 1, 2], np.int32)).cuda()
        done = torch.from_numpy(np.array([0, 0, 0, 7], np.int32)).cuda()
        err = torch.full((B,), NAN, dtype=torch.float64, device="cuda")
        solver(N, B).advance_horizon(True, d64["xu"], d64["xs"], d64["lam"], d64["goal"], d64["ee"], dev(plan), dev(goals), off, done, err, xu_fill_lead=lead)
        torch.cuda.synchronize()
        for k in ("xu", "lam", "goal"):
            assert same(d64[k], d32[k].cpu().numpy().astype(f64)), (N, shared, lead, k)


# ---- 7. a chain that is not the iiwa ----
def test_simulate_on_a_random_chain_vs_host_restatement():
    """tests/chain_models.py: no zero among the numbers the recursions multiply.  B = 3 (three live groups of a wavefront and an idle one), a schedule with
    a knot crossing and a remainder, both input sets of tests/chain_models.py, under the limit of test 3.
    Measured worst on the MI355X: 1.22e-15 (large set), 7.8e-16 (modest set)."""
    from mpcgpu_amd import Plant
    seed, B = cm.SEEDS[0], 3
    chain = cm.random_chain(seed)
    assert clamped_schedule(15000, 2100) == ([0] * 4 + [1] * 6, 1)
    worst = 0.0
    for size in ("large", "modest"):
        xu32, _, xs32 = cm.hard_inputs(N4, B, cm.input_seed(seed), size)
        xu, xs = doubles(xu32, 46), doubles(xs32, 47)
        got, ee = simulate(B, xs, xu, 15000, 2100, SS, pl=Plant(cm.tables(chain)))
        for b in range(B):
            want = P.simulate(chain, xs[b], xu[b], N4, DT, 15000, 2100, SS, double=True)
            assert np.abs(want - xs[b]).max() > 1e-4
            err = max(rel(got[b], want), rel(ee[b], chain.ee_pos(want[:7])))
            print(f"SIM64-FIG random chain {size} trajectory {b}: worst relative error {err:.3e}")
            worst = max(worst, err)
    assert worst < F32_ROUNDING and worst <= LIMIT_SIM, worst


# ---- 8. the closed loop in double ----
MU = 10.0


def closed_loop(starts, updates=8):
    """tests/test_gpu_simulate.py::closed_loop with every tensor float64 and the eight _f64 entries; the substep is (double)2e-4f, so that a 2,000 us update is
    ten substeps and the update count and the single shift are the float test's."""
    from mpcgpu_amd import pcg_config
    N = 8
    s = Mpc(N, starts, 20, ss=SS32)
    B, sol, cfg = s.B, s.sol, pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=3000)
    f8 = {"dtype": torch.float64, "device": "cuda"}
    rho, drho = torch.full((B,), 1e-3, **f8), torch.ones(B, **f8)
    sqp_done, step = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    tail = (DT, MU, iiwa.QD_COST, iiwa.r_cost(N))
    prev, since, shifted, shifts, errs = 0.0, 0.0, False, 0, []
    for _ in range(updates):
        ref = sol.compute_merit(plant(), s.goals, s.xs, s.xu, None, [0.0], *tail).reshape(B)
        G, Cd, g, c = sol.generate_kkt(plant(), s.goals, s.xs, s.xu, DT, iiwa.QD_COST, iiwa.r_cost(N))
        S, Pinv, gam = sol.form_schur(G, Cd, g, c, rho, "ss")
        sol.solve_f64(S, Pinv, gam, s.lam, cfg, "ss")
        dz = sol.compute_dz(G, Cd, g, s.lam)
        merit = sol.compute_merit(plant(), s.goals, s.xs, s.xu, dz, STEPS8, *tail)
        sol.line_search_step_rho(merit, STEPS8, ref, dz, s.xu, rho, drho, sqp_done, step=step)
        sim = 2000.0
        s.simulate(prev, sim)
        since += sim * 1e-6
        shift = not shifted and since > DT                   # SHIFT_THRESHOLD = one timestep
        s.advance(shift)
        if shift:
            shifted, shifts = True, shifts + 1
            errs.append(s.err.clone())
        if since > DT:
            shifted, since = False, np.fmod(since, DT)
        prev = sim
    out = s.state()
    out["errs"] = torch.stack(errs).cpu().numpy() if errs else np.zeros((0, B), f64)
    out["rho"] = rho.cpu().numpy()
    return out, shifts


def test_closed_loop_batched_vs_single_trajectory_loops():
    """B = 3 windows, N = 8, eight control updates of 2,000 us at timestep 1/64, nothing but float64 tensors and _f64 entries: every trajectory shifts once,
    the batched run equals the three single-trajectory runs bit for bit, every tracking error is finite and positive, and what the loop leaves behind
    are doubles that no float holds."""
    starts = (2, 150, 300)
    got, shifts = closed_loop(starts)
    assert shifts == 1 and got["offset"].tolist() == [1, 1, 1] and got["done"].tolist() == [0, 0, 0]
    assert got["errs"].shape == (1, 3) and np.isfinite(got["errs"]).all() and (got["errs"] > 0).all()
    print("tracking errors at the shift:", got["errs"])
    for k in ("xu", "lam", "xs"):
        assert got[k].dtype == f64 and np.isfinite(got[k]).all() and not_a_float(got[k]) > 0.3, (k, not_a_float(got[k]))
    for b, t0 in enumerate(starts):
        one, _ = closed_loop((t0,))
        for k in one:
            mine = got[k][:, b:b + 1] if k == "errs" else got[k][b:b + 1]
            assert same(one[k].reshape(-1), np.ascontiguousarray(mine).reshape(-1)), (b, k)


# ---- 9. refusals ----
def test_refusals_write_nothing():
    xu, xs = five64()
    sol, lib = solver(N4, 5), _lib.load()
    nan = lambda *s: torch.full(s, NAN, dtype=torch.float64, device="cuda")
    d_xs, d_xu, ee = dev(xs.copy()), dev(xu), nan(5, 3)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def sim(h=sol, xs_=d_xs, xu_=d_xu, control=7, dt=DT, toff=0.0, t=2000.0, ss=2e-4, batch=5, pl=plant()):
        rc = lib.mpcg_simulate_f64(h._h, pl._p, control, p(xs_), p(xu_), dt, toff, t, ss, p(ee), batch, None)
        return rc, lib.mpcg_last_error(h._h).decode()

    other = solver(N4, 5, 12, 6)
    for what, (rc, msg), code in (("null xs", sim(xs_=None), -1), ("null xu", sim(xu_=None), -1), ("batch", sim(batch=6), -1),
                                  ("control size", sim(control=6), -2), ("state size", sim(h=other), -2), ("sim_step 0", sim(ss=0.0), -1),
                                  ("negative step", sim(ss=-2e-4), -1), ("negative time", sim(t=-1.0), -1), ("negative offset", sim(toff=-1.0), -1),
                                  ("nan", sim(t=NAN), -1), ("inf", sim(toff=float("inf")), -1), ("nan step", sim(ss=NAN), -1),
                                  ("timestep 0", sim(dt=0.0), -1), ("over the cap", sim(t=1e9), -1)):
        assert rc == code and "mpcg_simulate_f64" in msg, (what, rc, msg)
    assert lib.mpcg_simulate_f64(None, plant()._p, 7, p(d_xs), p(d_xu), DT, 0.0, 2000.0, 2e-4, None, 5, None) == -1
    assert lib.mpcg_simulate_f64(sol._h, plant()._p, 7, p(d_xs), p(d_xu), DT, 0.0, 2000.0, 2e-4, p(ee), 0, None) == 0        # batch == 0: nothing to do
    torch.cuda.synchronize()
    assert same(d_xs, xs) and np.isnan(ee.cpu().numpy()).all()

    L = (n + m) * N4 - m
    a = {"xu": nan(5, L), "lam": nan(5, n * N4), "goal": nan(5, 6 * N4), "plan": nan(9, n + m), "goals": nan(9, 6), "err": nan(5)}
    off, done = torch.zeros(5, dtype=torch.int32, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")

    def adv(h=sol, control=7, shift=1, xu_=a["xu"], ee_=ee, T=9, stride=0, lead=0, batch=5, off_=off):
        rc = lib.mpcg_advance_horizon_f64(h._h, control, shift, p(xu_), p(a["lam"]), p(a["goal"]), p(d_xs), p(ee_), p(a["plan"]), p(a["goals"]), T, stride, lead,
                                          p(off_), p(done), p(a["err"]), batch, None)
        return rc, lib.mpcg_last_error(h._h).decode()

    for what, (rc, msg), code in (("shift without eePos", adv(ee_=None), -1), ("null xu", adv(xu_=None), -1), ("null offset", adv(off_=None), -1),
                                  ("batch", adv(batch=6), -1), ("control size", adv(control=6), -2), ("state size", adv(h=other), -2),
                                  ("shift 2", adv(shift=2), -1), ("no plan", adv(T=0), -1), ("lead", adv(lead=N4), -1), ("stride", adv(stride=8), -1)):
        assert rc == code and "mpcg_advance_horizon_f64" in msg, (what, rc, msg)
    assert "d_eePos" in adv(ee_=None)[1] and "mpcg_simulate_f64" in adv(ee_=None)[1]
    assert adv(batch=0)[0] == 0
    torch.cuda.synchronize()
    assert all(np.isnan(t.cpu().numpy()).all() for t in a.values()) and off.tolist() == [0] * 5 and done.tolist() == [0] * 5


# ---- 10. the Python dispatch on dtype ----
def test_python_dispatch_on_dtype():
    """float64 tensors reach the _f64 entries (before they existed PcgSolver.simulate refused float64 tensors), float32 tensors still give the float entries'
    bits, mixed dtypes raise TypeError."""
    lib, sol = _lib.load(), solver(N4, 5)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    xu, xs = five64()
    for dtype, fn, ss in ((f64, lib.mpcg_simulate_f64, SS), (f32, lib.mpcg_simulate, SS32)):
        got_xs, got_ee = simulate(5, xs, xu, 15000, 2100, ss, dtype)
        d_xs, d_xu = dev(xs, dtype), dev(xu, dtype)
        ee = torch.full((5, 3), NAN, dtype=d_xs.dtype, device="cuda")
        assert fn(sol._h, plant()._p, 7, p(d_xs), p(d_xu), DT, 15000.0, 2100.0, ss, p(ee), 5, None) == 0
        torch.cuda.synchronize()
        assert got_xs.dtype == dtype and same(got_xs, d_xs) and same(got_ee, ee) and np.isfinite(got_ee).all()
    d32, _ = advance_case(4, True, 0, dtype=f32)                                # (against the float restatement: the float entry's bits)
    assert d32["xu"].dtype == torch.float32
    d64, _ = advance_case(4, True, 0, dtype=f64)
    assert d64["xu"].dtype == torch.float64
    x64, u64, x32, u32 = dev(xs), dev(xu), dev(xs, f32), dev(xu, f32)
    with pytest.raises(TypeError):
        sol.simulate(plant(), x64, u32, DT, 0, 2000)
    with pytest.raises(TypeError):
        sol.simulate(plant(), x32, u32, DT, 0, 2000, eePos=torch.zeros(5, 3, dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        sol.advance_horizon(False, u64, x32)
    with pytest.raises(TypeError):
        sol.advance_horizon(False, u32.to(torch.int32), x32.to(torch.int32))
    torch.cuda.synchronize()
    assert same(x64, xs) and same(u32, xu.astype(f32))


# ---- 11. the example ----
def test_mpc_closed_loop_f64_example():
    """examples/mpc_closed_loop.cpp compiled with -DUSE_DOUBLES: simulateMPC<double> of the shim headers with all three library stages, then B windows through
    several control updates over the eight _f64 entries.  The assertions of tests/test_gpu_simulate.py::test_mpc_closed_loop_example."""
    from mpcgpu_amd import build
    exe = build.build_mpc_closed_loop_f64()
    r = subprocess.run([exe, "--batch", "3", "--knots", "8", "--updates", "9", "--mpc-steps", "12"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["batch"] == 3 and out["knots"] == 8 and out["updates"] == 9
    assert out["shifts"] == [1, 1, 1] and out["expected_shifts"] == 1
    err = np.array(out["tracking_errors"])
    assert err.shape == (1, 3) and np.isfinite(err).all()
    assert np.isfinite(out["simulate_mpc"]["tracking_errors"]).all() and len(out["simulate_mpc"]["tracking_errors"]) == 12
