"""GPU: the step between two SQP solves on the device — mpcg_simulate (simple_simulate, reference include/common/integrator.cuh:295-325, one launch
for the batch and all substeps) and mpcg_advance_horizon (tracking error, just_shift, tail fills, start-state copy: include/mpcsim.cuh:300-348).
Pinned on the reference's own trajectory file, against the float64 restatement tests/plant_ref.py (pinned in tests/test_sim_ref_cpu.py), against the
KKT kernel's integrator defect, and bit for bit across batch sizes, runs, graph replays and a closed MPC loop."""
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
from conftest import GOLDEN
from mpcgpu_amd import _lib, iiwa

pytestmark = pytest.mark.gpu
n, m = 14, 7
DT = 1.0 / 64
SS = np.float32(2e-4)
STEPS8 = [-1.0 / (1 << p) for p in range(8)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


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


# ---- 1. pinned on reference-held data ----
def test_one_step_reproduces_the_reference_trajectory():
    """The 656 in-segment transitions of the reference's trajectory file as ONE batch: N = 2, xu = [x_t, u_t, x_{t+1}], one Euler step of 1/64.
    The new state is the file's next row within the 5e-6 tests/test_iiwa_plant.py holds euler_defect to, the end-effector output the file's eepos row
    of that state within that test's 2e-5."""
    d = np.load(os.path.join(GOLDEN, "iiwa_traj_0_0_full.npz"))
    rows, eep = d["xu"], d["eepos"]
    good = iiwa_ref.in_segment_transitions(rows.shape[0])
    assert len(good) == 656
    xu = np.array([np.concatenate([rows[t], rows[t + 1, :n]]) for t in good], np.float32)
    xs, ee = dev(xu[:, :n].copy()), torch.full((656, 3), float("nan"), device="cuda")
    solver(2, 656).simulate(plant(), xs, dev(xu), DT, 0, 15625, 1 / 64, eePos=ee)
    worst = np.abs(xs.cpu().numpy() - rows[[t + 1 for t in good], :n]).max()
    worst_ee = np.abs(ee.cpu().numpy() - eep[[t + 1 for t in good], :3]).max()
    print("one step against the file: state", worst, "end effector", worst_ee)
    assert worst < 5e-6, worst
    assert worst_ee < 2e-5, worst_ee


# ---- 2. against the float64 restatement, on the pinned schedules ----
N4 = 4
# (time offset, simulated time) in us at timestep 1/64 and the reference's substep: no crossing; a knot crossing and a non-zero remainder; S = 0;
# indices 2 and 3 at N = 4 (the clamp); and a remainder behind a crossing its own time would see but the last full substep does not
CASES = [(0, 2000), (15000, 2100), (15000, 100), (46000, 2000), (15500, 300)]


@functools.lru_cache(maxsize=None)
def plan4():
    """One trajectory at N = 4 with three clearly different controls, and its start state."""
    rng = np.random.default_rng(11)
    xu = (0.4 * rng.standard_normal((n + m) * N4 - m)).astype(np.float32)
    scale = np.array([20, 20, 10, 10, 2, 2, 0.2])
    for k, sign in enumerate(((1, -1, 1, -1, 1, -1, 1), (-1, 1, -1, 1, -1, 1, -1), (1, 1, -1, -1, 1, 1, -1))):
        xu[k * (n + m) + n:(k + 1) * (n + m)] = scale * np.array(sign) * (1 + 0.25 * k)
    xs = (0.4 * rng.standard_normal(n)).astype(np.float32)
    return xu, xs


def clamped_schedule(toff, sim, recompute=False, ignore=False):
    S, idx, rem, ridx = P.schedule(toff, sim, DT, SS)
    if recompute:
        ridx = int((toff * 1e-6 + S * float(SS)) / DT)
    if ignore:
        idx, ridx = [int(toff * 1e-6 / DT)] * S, int(toff * 1e-6 / DT)
    return [min(i, N4 - 2) for i in idx], (min(ridx, N4 - 2) if rem != 0 else None)


@pytest.mark.parametrize("toff,sim", CASES)
def test_simulate_vs_host_restatement(toff, sim):
    """Relative to max(1, |x|) within 1e-6: the limit tests/test_gpu_merit.py::test_merit_vs_host_restatement sets for the same dynamics code against
    the same kind of restatement.  Where the schedule of a WRONG alternative (remainder index recomputed at its own time; the crossing ignored)
    differs from the right one, its result is more than 1e-4 away: the comparison tells them apart.  The plan is a view into a larger NaN-filled
    buffer: an index beyond the last control that was not clamped reads NaN."""
    xu, xs = plan4()
    big = torch.full((len(xu) + 64,), float("nan"), device="cuda")
    view = big[16:16 + len(xu)]
    view.copy_(dev(xu))
    d_xs, ee = dev(xs.copy()), torch.zeros(3, device="cuda")
    solver(N4, 1).simulate(plant(), d_xs, view, DT, toff, sim, float(SS), eePos=ee)
    got = d_xs.cpu().numpy().astype(np.float64)
    want = P.simulate(model(), xs, xu, N4, DT, toff, sim, SS)
    assert np.isfinite(got).all() and np.isfinite(ee.cpu().numpy()).all()
    err = (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()
    ee_err = np.abs(ee.cpu().numpy() - model().ee_pos(want[:7])).max()
    print(f"toff {toff} sim {sim}: worst relative error {err:.3e}, end effector {ee_err:.3e}")
    assert err < 1e-6, err
    assert ee_err < 1e-6, ee_err
    for flag in ("recompute_remainder_index", "ignore_crossing"):
        kw = {"recompute": flag[0] == "r", "ignore": flag[0] == "i"}
        if clamped_schedule(toff, sim, **kw) != clamped_schedule(toff, sim):
            other = P.simulate(model(), xs, xu, N4, DT, toff, sim, SS, **{flag: True})
            assert np.abs(other - want).max() > 1e-4, flag


def test_the_cases_tell_both_wrong_schedules_apart():
    right = [clamped_schedule(*c) for c in CASES]
    assert any(clamped_schedule(*c, recompute=True) != r for c, r in zip(CASES, right))
    assert any(clamped_schedule(*c, ignore=True) != r for c, r in zip(CASES, right))
    assert clamped_schedule(46000, 2000) == ([2] * 10, None if P.schedule(46000, 2000, DT, SS)[2] == 0 else 2)      # the clamp case


# ---- 3. against existing device code ----
def test_one_step_is_the_kkt_kernels_integrator():
    """mpcg_generate_kkt on [x, u, 0] (N = 2) stores c_1 = 0 - (x + dt f(x, u)); one mpcg_simulate step of the same dt is -c_1 to at most one
    float32 ulp: two float roundings of float64 values that differ by summation noise only."""
    B = 64
    xu_w, _, xs_w = iiwa.random_windows(2, B, 5)
    xu = np.ascontiguousarray(xu_w, np.float32)
    xu[:, n + m:] = 0.0
    xs = np.ascontiguousarray(xu[:, :n])
    sol = solver(2, 656)
    goals = torch.zeros(B, 12, device="cuda")
    _, _, _, c = sol.generate_kkt(plant(), goals, dev(xs), dev(xu), DT, iiwa.QD_COST, iiwa.r_cost(2))
    d_xs = dev(xs.copy())
    sol.simulate(plant(), d_xs, dev(xu), DT, 0, 15625, 1 / 64)
    step, kkt = d_xs.cpu().numpy(), -c.cpu().numpy().reshape(B, 2, n)[:, 1]
    gap = np.abs(step.astype(np.float64) - kkt.astype(np.float64)) / np.spacing(np.maximum(np.abs(step), np.abs(kkt)))
    print("worst gap to the KKT kernel's integrator in float32 ulps:", gap.max(), "exactly equal:", (gap == 0).mean())
    assert gap.max() <= 1.0, gap.max()


# ---- 4. bits ----
def five():
    xu_w, _, xs_w = iiwa.random_windows(N4, 5, 23)
    return np.ascontiguousarray(xu_w, np.float32), np.ascontiguousarray(xs_w, np.float32)


def test_batch_of_five_equals_five_single_calls_and_runs_repeat():
    xu, xs = five()
    sol = solver(N4, 5)
    out = []
    for _ in range(2):
        d_xs, ee = dev(xs.copy()), torch.zeros(5, 3, device="cuda")
        sol.simulate(plant(), d_xs, dev(xu), DT, 15000, 2100, float(SS), eePos=ee)
        out.append((d_xs.cpu().numpy(), ee.cpu().numpy()))
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1])
    assert not same(out[0][0], xs)
    for b in range(5):
        d_xs, ee = dev(xs[b:b + 1].copy()), torch.zeros(1, 3, device="cuda")
        solver(N4, 1).simulate(plant(), d_xs, dev(xu[b:b + 1]), DT, 15000, 2100, float(SS), eePos=ee)
        assert same(d_xs, out[0][0][b:b + 1]) and same(ee, out[0][1][b:b + 1]), b


def test_zero_time_leaves_the_state_bitwise_unchanged():
    xu, xs = five()
    xs[0, 3], xs[2, 9] = -0.0, 0.0
    d_xs = dev(xs.copy())
    solver(N4, 5).simulate(plant(), d_xs, dev(xu), DT, 4000, 0, float(SS))
    assert same(d_xs, xs)


class Mpc:
    """Device state of B trajectories of an MPC loop at horizon N over per-trajectory plans cut from the reference trajectory."""

    def __init__(self, N, starts, T, perturb=0.02, seed=1):
        d = np.load(iiwa.TRAJ_FIXTURE)
        B = len(starts)
        f = lambda a: np.ascontiguousarray(a, np.float32)
        self.N, self.B, self.T = N, B, T
        self.sol = solver(N, B)
        self.plan = dev(f([d["xu"][t:t + T] for t in starts]))                    # [B, T, 21]
        self.plan_goals = dev(f([d["eepos"][t:t + T] for t in starts]))           # [B, T, 6]
        L = (n + m) * N - m
        self.xu = self.plan[:, :N].reshape(B, -1)[:, :L].clone()                # (a copy: for B = 1 the slice is contiguous and would alias the plan)
        self.xu_old = self.xu.clone()
        self.goals = self.plan_goals[:, :N].reshape(B, -1).clone()
        # the measured state is off the plan; a trajectory's perturbation depends on its own window only (a batch and a single run agree)
        noise = np.array([np.random.default_rng(seed + t).standard_normal(n) for t in starts])
        self.xs = dev(f(self.xu[:, :n].cpu().numpy() + perturb * noise))
        self.lam = torch.zeros(B, n * N, device="cuda")
        self.ee = torch.zeros(B, 3, device="cuda")
        self.offset = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.err = torch.full((B,), float("nan"), device="cuda")

    def simulate(self, toff, sim):
        self.sol.simulate(plant(), self.xs, self.xu_old, DT, toff, sim, float(SS), eePos=self.ee)
        self.xu_old.copy_(self.xu)                                                # (mpcsim.cuh:291)

    def advance(self, shift, lead=0):
        self.sol.advance_horizon(shift, self.xu, self.xs, self.lam, self.goals, self.ee, self.plan, self.plan_goals, self.offset, self.done,
                                 self.err, xu_fill_lead=lead)

    def state(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("xu", "xu_old", "xs", "lam", "goals", "ee", "offset", "done", "err")}


def test_captured_simulate_and_advance_replay_the_eager_steps():
    """simulate -> advance_horizon(shift = 1) captured ONCE and replayed three times is three eager steps, bit for bit: both calls are pure stream work
    and every operand of the schedule that changes between steps (the state, the plan offset) lives in device memory."""
    make = lambda: Mpc(N4, (2, 150, 300, 40, 200), 12)
    eager = make()
    want = []
    for _ in range(3):
        eager.simulate(1000, 2100)
        eager.advance(True)
        want.append(eager.state())
    assert want[-1]["offset"].tolist() == [3] * 5 and not same(want[0]["xs"], want[1]["xs"])
    rep = make()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        rep.simulate(1000, 2100)
        rep.advance(True)
    rep2 = make()                                              # (capture runs nothing: the state is still the initial one)
    assert all(same(a, b) for a, b in zip(rep.state().values(), rep2.state().values()))
    for i in range(3):
        graph.replay()
        got = rep.state()
        for k in got:
            assert same(got[k], want[i][k]), (i, k)


# ---- 5. advance_horizon bit for bit against the restatement ----
def advance_case(N, shared, lead, shift=True):
    B, T = 4, N + 6
    rng = np.random.default_rng(100 * N + 10 * shared + lead)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    L = (n + m) * N - m
    plan, goals = (f(T, n + m), f(T, 6)) if shared else (f(B, T, n + m), f(B, T, 6))
    h = {"xu": f(B, L), "lam": f(B, n * N), "goal": f(B, 6 * N), "xs": f(B, n), "ee": f(B, 3)}
    # inside the plan; exactly offset + N == T after the increment (the else branch); reaches T (done becomes 1); frozen on entry
    off0 = np.array([0, T - N - 1, T - 1, 2], np.int32)
    done0 = np.array([0, 0, 0, 7], np.int32)
    d = {k: dev(v) for k, v in h.items()}
    d_off, d_done, d_err = dev(off0), dev(done0), torch.full((B,), float("nan"), device="cuda")
    solver(N, B).advance_horizon(shift, d["xu"], d["xs"], d["lam"], d["goal"], d["ee"], dev(plan), dev(goals), d_off, d_done, d_err, xu_fill_lead=lead)
    torch.cuda.synchronize()
    for b in range(B):
        p, g = (plan, goals) if shared else (plan[b], goals[b])
        xu, lam, goal, off, done, err = P.advance(shift, N, h["xu"][b], h["lam"][b], h["goal"][b], h["xs"][b], h["ee"][b], p, g, T, int(off0[b]),
                                                        int(done0[b]), lead)
        assert same(d["xu"][b], xu) and same(d["lam"][b], lam) and same(d["goal"][b], goal), (b, N, shared, lead)
        assert int(d_off[b]) == off and int(d_done[b]) == done, (b, int(d_off[b]), int(d_done[b]))
        if err is None:
            assert np.isnan(d_err[b].item())
        else:
            assert same(d_err[b:b + 1], np.array([err], np.float32)), b
    assert same(d["xs"], h["xs"]) and same(d["ee"], h["ee"])
    if shift:
        assert d_done.tolist() == [0, 0, 1, 7] and d_off.tolist() == [1, T - N, T, 2]
    return d, h


@pytest.mark.parametrize("N", [4, 2])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("lead", ["0", "N-1"])
def test_advance_horizon_shift_vs_restatement(N, shared, lead):
    advance_case(N, shared, 0 if lead == "0" else N - 1)


def test_advance_horizon_without_shift_writes_the_start_state_only():
    """shift = 0: 14 floats per live trajectory; lambda, the goals, the offsets, the flags and the error keep every bit (compared whole), and the call
    needs nothing but xu and xs."""
    d, h = advance_case(4, True, 0, shift=False)
    assert same(d["xu"][:3, n:], h["xu"][:3, n:]) and same(d["xu"][:3, :n], h["xs"][:3]) and same(d["xu"][3], h["xu"][3])
    xu = dev(h["xu"])
    solver(4, 4).advance_horizon(False, xu, dev(h["xs"]))
    assert same(xu[:, :n], h["xs"]) and same(xu[:, n:], h["xu"][:, n:])


def test_advance_horizon_long_horizon_sweeps_in_chunks():
    """N = 128: xu (2,681 floats) and lambda (1,792) are longer than one sweep chunk of 2,048 elements — the size at which the kernel takes its
    second trip through load, barrier, store."""
    advance_case(128, False, 127)


# ---- 6. the closed loop ----
MU = 10.0


def closed_loop(starts, updates=8):
    """`updates` control updates of 2,000 us (CONST_UPDATE_FREQ) with the host bookkeeping of include/mpcsim.cuh:280-352; one SQP iteration of the six
    device calls per update, then simulate under the PREVIOUS plan and advance.  Nothing is read back inside the loop."""
    from mpcgpu_amd import pcg_config
    N = 8
    s = Mpc(N, starts, 20)
    B, sol, cfg = s.B, s.sol, pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=3000)
    rho, drho = torch.full((B,), 1e-3, device="cuda"), torch.ones(B, device="cuda")
    sqp_done, step = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    tail = (DT, MU, iiwa.QD_COST, iiwa.r_cost(N))
    prev, since, shifted, shifts, errs = 0.0, 0.0, False, 0, []
    for _ in range(updates):
        ref = sol.compute_merit(plant(), s.goals, s.xs, s.xu, None, [0.0], *tail).reshape(B)
        G, Cd, g, c = sol.generate_kkt(plant(), s.goals, s.xs, s.xu, DT, iiwa.QD_COST, iiwa.r_cost(N))
        S, Pinv, gam = sol.form_schur(G, Cd, g, c, rho, "ss")
        sol.solve(S, Pinv, gam, s.lam, cfg, "ss")
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
    out["errs"] = torch.stack(errs).cpu().numpy() if errs else np.zeros((0, B), np.float32)
    out["rho"] = rho.cpu().numpy()
    return out, shifts


def test_closed_loop_batched_vs_single_trajectory_loops():
    """B = 3 windows, N = 8, eight control updates of 2,000 us at timestep 1/64: the eighth crosses the shift threshold, so every trajectory shifts
    once.  The batched run equals the three single-trajectory runs bit for bit (every stage is batch-independent by its own tests), and every tracking
    error is finite."""
    starts = (2, 150, 300)
    got, shifts = closed_loop(starts)
    assert shifts == 1 and got["offset"].tolist() == [1, 1, 1] and got["done"].tolist() == [0, 0, 0]
    assert got["errs"].shape == (1, 3) and np.isfinite(got["errs"]).all() and (got["errs"] > 0).all()
    print("tracking errors at the shift:", got["errs"])
    for b, t0 in enumerate(starts):
        one, _ = closed_loop((t0,))
        for k in one:
            mine = got[k][:, b:b + 1] if k == "errs" else got[k][b:b + 1]
            assert same(one[k].reshape(-1), np.ascontiguousarray(mine).reshape(-1)), (b, k)


# ---- 7. refusals ----
def test_refusals_write_nothing():
    xu, xs = five()
    sol, lib = solver(N4, 5), _lib.load()
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    d_xs, d_xu, ee = dev(xs.copy()), dev(xu), nan(5, 3)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def sim(h=sol, xs_=d_xs, xu_=d_xu, control=7, dt=DT, toff=0.0, t=2000.0, ss=2e-4, batch=5, pl=plant()):
        rc = lib.mpcg_simulate(h._h, pl._p, control, p(xs_), p(xu_), dt, toff, t, ss, p(ee), batch, None)
        return rc, lib.mpcg_last_error(h._h).decode()

    other = solver(N4, 5, 12, 6)
    for what, (rc, msg), code in (("null xs", sim(xs_=None), -1), ("null xu", sim(xu_=None), -1), ("batch", sim(batch=6), -1),
                                  ("control size", sim(control=6), -2), ("state size", sim(h=other), -2), ("sim_step 0", sim(ss=0.0), -1),
                                  ("negative step", sim(ss=-2e-4), -1), ("negative time", sim(t=-1.0), -1), ("negative offset", sim(toff=-1.0), -1),
                                  ("nan", sim(t=float("nan")), -1), ("inf", sim(toff=float("inf")), -1), ("timestep 0", sim(dt=0.0), -1),
                                  ("over the cap", sim(t=1e9), -1)):
        assert rc == code and "mpcg_simulate" in msg, (what, rc, msg)
    assert _lib.MPCG_SIM_MAX_SUBSTEPS == 65536
    assert lib.mpcg_simulate(None, plant()._p, 7, p(d_xs), p(d_xu), DT, 0.0, 2000.0, 2e-4, None, 5, None) == -1
    torch.cuda.synchronize()
    assert same(d_xs, xs) and np.isnan(ee.cpu().numpy()).all()

    L = (n + m) * N4 - m
    a = {"xu": nan(5, L), "lam": nan(5, n * N4), "goal": nan(5, 6 * N4), "plan": nan(9, n + m), "goals": nan(9, 6), "err": nan(5)}
    off, done = torch.zeros(5, dtype=torch.int32, device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")

    def adv(h=sol, control=7, shift=1, xu_=a["xu"], ee_=ee, T=9, stride=0, lead=0, batch=5, off_=off):
        rc = lib.mpcg_advance_horizon(h._h, control, shift, p(xu_), p(a["lam"]), p(a["goal"]), p(d_xs), p(ee_), p(a["plan"]), p(a["goals"]), T, stride, lead,
                                      p(off_), p(done), p(a["err"]), batch, None)
        return rc, lib.mpcg_last_error(h._h).decode()

    for what, (rc, msg), code in (("shift without eePos", adv(ee_=None), -1), ("null xu", adv(xu_=None), -1), ("null offset", adv(off_=None), -1),
                                  ("batch", adv(batch=6), -1), ("control size", adv(control=6), -2), ("state size", adv(h=other), -2),
                                  ("shift 2", adv(shift=2), -1), ("no plan", adv(T=0), -1), ("lead", adv(lead=N4), -1), ("stride", adv(stride=8), -1)):
        assert rc == code and "mpcg_advance_horizon" in msg, (what, rc, msg)
    assert "d_eePos" in adv(ee_=None)[1]
    torch.cuda.synchronize()
    assert all(np.isnan(t.cpu().numpy()).all() for t in a.values()) and off.tolist() == [0] * 5 and done.tolist() == [0] * 5


# ---- 8. the example ----
def test_mpc_closed_loop_example():
    """examples/mpc_closed_loop.cpp: simulateMPC of the shim headers with all three library stages on the reference trajectory, then B windows
    through several control updates with no synchronisation inside an update."""
    from mpcgpu_amd import build
    exe = build.build_mpc_closed_loop()
    r = subprocess.run([exe, "--batch", "3", "--knots", "8", "--updates", "9", "--mpc-steps", "12"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["batch"] == 3 and out["knots"] == 8 and out["updates"] == 9
    assert out["shifts"] == [1, 1, 1] and out["expected_shifts"] == 1
    err = np.array(out["tracking_errors"])
    assert err.shape == (1, 3) and np.isfinite(err).all()
    assert np.isfinite(out["simulate_mpc"]["tracking_errors"]).all() and len(out["simulate_mpc"]["tracking_errors"]) == 12
