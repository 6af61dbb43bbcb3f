"""GPU: per-trajectory clocks — mpcg_simulate_clk(_f64) and mpcg_advance_horizon_clk(_f64) (mpcgpu_amd/csrc/sim_plant.hip.h: simulate_kernel with
CLOCK = 1, advance_horizon_clk_kernel).  Trajectory b of a call gets, BIT FOR BIT, what the scalar entries give it with its own times and the shift
decision of tests/clock_ref.py (pinned in tests/test_clock_ref_cpu.py): mixed schedules in one wavefront, frozen and invalid trajectories, a loop of 40
updates at four rates, one captured update replayed under changing times, refusals, guard bands and the example's --periods-us."""
import ctypes as C
import functools
import json
import math
import subprocess

import numpy as np
import pytest
import torch

import arena
import arena_specs as A
import clock_ref
import plant_ref as P
import test_gpu_simulate as t32
import test_gpu_simulate_f64 as t64
from mpcgpu_amd import Clocks, _lib
from test_gpu_simulate import CASES, bits, model, plan4, plant, same

pytestmark = pytest.mark.gpu
n, m = 14, 7
N4 = 4
DT = 1.0 / 64
L4 = (n + m) * N4 - m
PRECS = ("f32", "f64")
NP = {"f32": np.float32, "f64": np.float64}
TD = {"f32": torch.float32, "f64": torch.float64}
SS = {"f32": float(np.float32(2e-4)), "f64": 2e-4}          # the reference's substep in either type (include/mpcg.h, mpcg_simulate_f64)
MPC = {"f32": t32.Mpc, "f64": t64.Mpc}
NAN = float("nan")
# the five schedules of tests/test_gpu_simulate.py and a zero-time trajectory: mixed S in a wavefront, a half-filled last wavefront
SIX = list(CASES) + [(4000, 0)]
assert len(SIX) == 6


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def f64s(values):
    return dev(np.asarray(values, np.float64))


@functools.lru_cache(maxsize=None)
def solver(N, B, state_size=14, control_size=None):
    from mpcgpu_amd import PcgSolver
    return PcgSolver(N, max_batch=B, state_size=state_size, control_size=control_size)


@functools.lru_cache(maxsize=None)
def six(prec):
    """Six trajectories at N = 4 over plan4's three clearly different controls, each with its own start state (and its own plan values in double)."""
    xu, xs = plan4()
    xu6 = np.stack([xu] * 6).astype(np.float64)
    xs6 = np.stack([xs + np.float32(0.01 * b) for b in range(6)]).astype(np.float64)
    if prec == "f64":
        xu6, xs6 = t64.doubles(xu6, 71), t64.doubles(xs6, 72)
    return np.ascontiguousarray(xu6, NP[prec]), np.ascontiguousarray(xs6, NP[prec])


@functools.lru_cache(maxsize=None)
def scalar_single(prec, b, toff, sim):
    """Trajectory b of six() through a batch-of-1 call of the scalar entry: (xs, eePos) as numpy — computed once, shared, never changed."""
    xu, xs = six(prec)
    d_xs, ee = dev(xs[b:b + 1].copy()), torch.full((1, 3), NAN, dtype=TD[prec], device="cuda")
    solver(N4, 1).simulate(plant(), d_xs, dev(xu[b:b + 1]), DT, float(toff), float(sim), SS[prec], eePos=ee)
    out = d_xs.cpu().numpy(), ee.cpu().numpy()
    for a in out:
        a.flags.writeable = False
    return out


def clk(prec, rows, times, done=None, with_ee=True, xs_rows=None, xu_dev=None):
    """mpcg_simulate_clk on trajectories `rows` of six() with `times` = [(toff, sim)]: (xs, eePos or None) as numpy.  eePos starts NaN-filled."""
    xu, xs = six(prec)
    B = len(rows)
    d_xs = dev(xs[list(rows)].copy() if xs_rows is None else xs_rows)
    ee = torch.full((B, 3), NAN, dtype=TD[prec], device="cuda") if with_ee else None
    solver(N4, 8).simulate_clk(plant(), d_xs, dev(xu[list(rows)]) if xu_dev is None else xu_dev, DT, f64s([t[0] for t in times]), f64s([t[1] for t in times]),
                               SS[prec], eePos=ee, done=done)
    torch.cuda.synchronize()
    return d_xs.cpu().numpy(), (ee.cpu().numpy() if with_ee else None)


# ---- 1. a mixed batch is the scalar entry per trajectory, bit for bit ----
@pytest.mark.parametrize("prec", PRECS)
def test_mixed_batch_equals_single_scalar_calls(prec):
    """B = 6 at N = 4: two wavefronts, the first with four different schedules (S = 10, 10 and a remainder, 0 and a remainder, 10 clamped), the second
    half filled, a zero-time trajectory beside a moving one.  Also in reversed order (other wavefront mates), and every state has moved but the
    zero-time one."""
    for order in (range(6), range(5, -1, -1)):
        order = list(order)
        xs, ee = clk(prec, order, [SIX[b] for b in order])
        for i, b in enumerate(order):
            want_xs, want_ee = scalar_single(prec, b, *SIX[b])
            assert same(xs[i:i + 1], want_xs) and same(ee[i:i + 1], want_ee), (prec, order, b)
    assert same(scalar_single(prec, 5, *SIX[5])[0], six(prec)[1][5:6]) and not same(scalar_single(prec, 0, *SIX[0])[0], six(prec)[1][0:1])


@pytest.mark.parametrize("toff,sim", SIX)
@pytest.mark.parametrize("prec", PRECS)
def test_uniform_arrays_equal_the_scalar_entry(prec, toff, sim):
    xu, xs = six(prec)
    d_xs, ee = dev(xs.copy()), torch.full((6, 3), NAN, dtype=TD[prec], device="cuda")
    solver(N4, 8).simulate(plant(), d_xs, dev(xu), DT, float(toff), float(sim), SS[prec], eePos=ee)
    got_xs, got_ee = clk(prec, range(6), [(toff, sim)] * 6)
    assert same(got_xs, d_xs) and same(got_ee, ee)
    got_xs, got_ee = clk(prec, range(6), [(toff, sim)] * 6, with_ee=False)
    assert same(got_xs, d_xs) and got_ee is None


# ---- 2. against the float64 restatement ----
@pytest.mark.parametrize("prec", PRECS)
def test_mixed_batch_vs_host_restatement(prec):
    """Each of the six within the 1e-6 (relative to max(1, |x|)) of tests/test_gpu_simulate.py::test_simulate_vs_host_restatement.  The plans are a
    view in a NaN-filled buffer and the clamp case (46000, 2000) is the LAST trajectory: an index that was not clamped reads NaN there, and a
    neighbour's state elsewhere."""
    order = [0, 1, 2, 4, 5, 3]
    xu, xs = six(prec)
    big = torch.full((6 * L4 + 128,), NAN, dtype=TD[prec], device="cuda")
    view = big[32:32 + 6 * L4].view(6, L4)
    view.copy_(dev(xu[order]))
    got, ee = clk(prec, order, [SIX[b] for b in order], xu_dev=view)
    assert np.isfinite(got).all() and np.isfinite(ee).all()
    for i, b in enumerate(order):
        want = P.simulate(model(), xs[b], xu[b], N4, DT, *SIX[b], NP[prec](SS[prec]), double=prec == "f64")
        err = (np.abs(got[i].astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max()
        ee_err = np.abs(ee[i].astype(np.float64) - model().ee_pos(want[:7])).max()
        print(f"{prec} trajectory {b} {SIX[b]}: worst relative error {err:.3e}, end effector {ee_err:.3e}")
        assert err < 1e-6 and ee_err < 1e-6, (b, err, ee_err)


# ---- 3. frozen and invalid trajectories ----
@pytest.mark.parametrize("prec", PRECS)
def test_frozen_and_invalid_trajectories_write_nothing(prec):
    """Eight trajectories: valid ones (0, 4, 7) among one frozen on entry (1) and four whose times are no schedule — sim NaN (2), offset -1 (3),
    sim +inf (5), sim / ss = 65537 (6).  The bad rows of xs and eePos are NaN canaries with a payload: they keep every bit.  done becomes 2
    exactly for the invalid ones; without d_done they are skipped silently; the valid ones equal a call of the three alone."""
    ss = SS[prec]
    over = 65537 * ss * 1e6 * (1 + 1e-9)
    assert clock_ref.schedule(0.0, over, ss, NP[prec])[0] is False
    rows = [0, 1, 2, 3, 4, 5, 0, 1]
    times = [SIX[0], (1000.0, 2000.0), (0.0, NAN), (-1.0, 2000.0), SIX[1], (0.0, math.inf), (0.0, over), SIX[2]]
    valid, frozen, invalid = [0, 4, 7], [1], [2, 3, 5, 6]
    xu, xs = six(prec)
    canary = np.frombuffer(np.array([0x7FC12345 if prec == "f32" else 0x7FF8000012345678], np.uint32 if prec == "f32" else np.uint64).tobytes(), NP[prec])[0]
    xs_in = xs[rows].copy()
    xs_in[frozen + invalid] = canary
    alone_xs, alone_ee = clk(prec, [rows[v] for v in valid], [times[v] for v in valid])
    for with_done in (True, False):
        start = xs_in.copy()
        if not with_done:
            start[frozen] = xs[[rows[f] for f in frozen]]          # (without d_done nothing marks it: a trajectory like any other)
        d_xs = dev(start)
        ee = dev(np.full((8, 3), canary, NP[prec]))
        done = dev(np.array([0, 1, 0, 0, 0, 0, 0, 0], np.int32)) if with_done else None
        solver(N4, 8).simulate_clk(plant(), d_xs, dev(xu[rows]), DT, f64s([t[0] for t in times]), f64s([t[1] for t in times]), ss, eePos=ee, done=done)
        torch.cuda.synchronize()
        keep = invalid + (frozen if with_done else [])
        assert same(d_xs[keep], start[keep]) and same(ee[keep], np.full((len(keep), 3), canary, NP[prec])), with_done
        assert same(d_xs[valid], alone_xs) and same(ee[valid], alone_ee), with_done
        if with_done:
            assert done.tolist() == [0, 1, 2, 2, 0, 2, 2, 0]
        else:
            assert np.isfinite(d_xs[frozen].cpu().numpy()).all()


# ---- 4. advance ----
def advance_case(prec, N, shared, lead):
    """Five trajectories under one call at shift_threshold_s = timestep / 2: 0 shifts and wraps; 1 neither; 2 has shifted in this timestep already
    and wraps (shifted back to 0); 3 is frozen; 4 shifts without a wrap, at the end of its plan (done becomes 1).  Against single-trajectory
    mpcg_advance_horizon calls with clock_ref's decision, and clock_ref's clock, bit for bit."""
    B, T, dt = 5, N + 6, NP[prec]
    rng = np.random.default_rng(1000 * N + 10 * shared + lead)
    f = lambda *s: rng.standard_normal(s).astype(dt)
    L = (n + m) * N - m
    plan, goals = (f(T, n + m), f(T, 6)) if shared else (f(B, T, n + m), f(B, T, 6))
    h = {"xu": f(B, L), "lam": f(B, n * N), "goal": f(B, 6 * N), "xs": f(B, n), "ee": f(B, 3)}
    off0, done0 = np.array([0, 3, 1, 2, T - 1], np.int32), np.array([0, 0, 0, 7, 0], np.int32)
    since0, shifted0 = [0.0150, 0.002, 0.0150, 0.0150, 0.008], [0, 0, 1, 0, 0]
    prev0, sim = [500.0, 600.0, 700.0, 800.0, 900.0], [1000.0, 2000.0, 1000.0, 1000.0, 1000.0]
    thr = DT / 2
    want_clock = [clock_ref.update(since0[b], shifted0[b], sim[b], DT, thr) for b in range(B)]
    assert [w[3] for w in want_clock] == [True, False, False, True, True] and [w[1] for w in want_clock] == [0, 0, 0, 0, 1]
    assert since0[0] + sim[0] * 1e-6 > DT and since0[2] + sim[2] * 1e-6 > DT > since0[4] + sim[4] * 1e-6 > thr
    d = {k: dev(v) for k, v in h.items()}
    d_off, d_done, d_err = dev(off0), dev(done0), torch.full((B,), NAN, dtype=TD[prec], device="cuda")
    ck = Clocks(B)
    ck.prev_sim_us.copy_(f64s(prev0)); ck.since_s.copy_(f64s(since0)); ck.shifted.copy_(dev(np.array(shifted0, np.int32)))
    did = torch.full((B,), -5, dtype=torch.int32, device="cuda")
    d_plan, d_goals = dev(plan), dev(goals)
    solver(N, B).advance_horizon_clk(d["xu"], d["xs"], d["lam"], d["goal"], d["ee"], d_plan, d_goals, d_off, d_done, d_err, DT, f64s(sim), ck, did_shift=did,
                                     shift_threshold_s=thr, xu_fill_lead=lead)
    torch.cuda.synchronize()
    for b in range(B):
        frozen = done0[b] != 0
        shift = want_clock[b][3] and not frozen
        one = {k: dev(v[b:b + 1].copy()) for k, v in h.items()}
        o_off, o_done, o_err = dev(off0[b:b + 1].copy()), dev(done0[b:b + 1].copy()), torch.full((1,), NAN, dtype=TD[prec], device="cuda")
        p, g = (d_plan, d_goals) if shared else (dev(plan[b:b + 1].copy()), dev(goals[b:b + 1].copy()))
        solver(N, 1).advance_horizon(shift, one["xu"], one["xs"], one["lam"], one["goal"], one["ee"], p, g, o_off, o_done, o_err, xu_fill_lead=lead)
        torch.cuda.synchronize()
        for k in ("xu", "lam", "goal"):
            assert same(d[k][b:b + 1], one[k]), (prec, N, shared, lead, b, k)
        assert int(d_off[b]) == int(o_off[0]) and int(d_done[b]) == int(o_done[0]) and same(d_err[b:b + 1], o_err), b
        if not shift:
            assert np.isnan(d_err[b].item()) and int(d_off[b]) == off0[b]                  # the canary; the offset
        since, shifted, prev, _ = (since0[b], shifted0[b], prev0[b], 0) if frozen else want_clock[b]
        assert same(ck.since_s[b:b + 1], np.array([since])) and same(ck.prev_sim_us[b:b + 1], np.array([prev])), (b, float(ck.since_s[b]), since)
        assert int(ck.shifted[b]) == shifted and int(did[b]) == int(shift), (b, ck.shifted.tolist(), did.tolist())
    assert same(d["xs"], h["xs"]) and same(d["ee"], h["ee"])
    assert d_done.tolist() == [0, 0, 0, 7, 1] and d_off.tolist() == [1, 3, 1, 2, T] and did.tolist() == [1, 0, 0, 0, 1]


@pytest.mark.parametrize("N", [4, 2])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("lead", ["0", "N-1"])
@pytest.mark.parametrize("prec", PRECS)
def test_advance_horizon_clk_vs_scalar_entry_and_clock_ref(prec, N, shared, lead):
    advance_case(prec, N, shared, 0 if lead == "0" else N - 1)


@pytest.mark.parametrize("N", [40, 128])
def test_advance_horizon_clk_longer_horizons(N):
    """N = 40, and N = 128, where xu (2,681 elements) and lambda (1,792) are longer than one sweep chunk of 2,048: the second trip through load,
    barrier, store (tests/test_gpu_simulate.py::test_advance_horizon_long_horizon_sweeps_in_chunks; at N = 40 every array still fits one chunk)."""
    advance_case("f32", N, False, N - 1)


# ---- 5. the loop ----
PERIODS = (1000.0, 2000.0, 3000.0, 20000.0)
STARTS = (2, 150, 300, 40)
LOOP_T = 46


def run_loop(prec, starts, periods, updates=40):
    """No SQP: per update xu_old <- xu, simulate under xu_old, advance.  One trajectory: the scalar entries and a host clock (clock_ref); several: the
    _clk entries and clocks on the device.  -> (final state arrays, [tracking errors at its shifts] per trajectory, shift counts)."""
    s = MPC[prec](N4, tuple(starts), LOOP_T)
    B, ss = s.B, SS[prec]
    errs = [[] for _ in range(B)]
    if B == 1:
        c = clock_ref.Clock(DT, NP[prec])
        for _ in range(updates):
            s.xu_old.copy_(s.xu)
            s.sol.simulate(plant(), s.xs, s.xu_old, DT, c.prev_sim_us, periods[0], ss, eePos=s.ee)
            shift = c.update(periods[0])
            s.advance(shift)
            if shift:
                errs[0].append(s.err.cpu().numpy().copy())
        out = s.state()
        out.update(since=np.array([c.since_s]), shifted=np.array([c.shifted], np.int32), prev=np.array([c.prev_sim_us]))
        return out, errs, [c.shifts]
    ck, sim_us = Clocks(B), f64s(periods)
    did = torch.zeros(B, dtype=torch.int32, device="cuda")
    hist_err, hist_did = [], []
    for _ in range(updates):
        s.xu_old.copy_(s.xu)
        s.sol.simulate_clk(plant(), s.xs, s.xu_old, DT, ck.prev_sim_us, sim_us, ss, eePos=s.ee, done=s.done)
        s.sol.advance_horizon_clk(s.xu, s.xs, s.lam, s.goals, s.ee, s.plan, s.plan_goals, s.offset, s.done, s.err, DT, sim_us, ck, did_shift=did)
        hist_err.append(s.err.clone()); hist_did.append(did.clone())
    out = s.state()
    out.update(since=ck.since_s.cpu().numpy(), shifted=ck.shifted.cpu().numpy(), prev=ck.prev_sim_us.cpu().numpy())
    hist_err, hist_did = torch.stack(hist_err).cpu().numpy(), torch.stack(hist_did).cpu().numpy()
    for b in range(B):
        errs[b] = [hist_err[u, b:b + 1].copy() for u in range(updates) if hist_did[u, b]]
    return out, errs, hist_did.sum(axis=0).tolist()


@pytest.mark.parametrize("prec", PRECS)
def test_loop_at_four_rates_vs_single_trajectory_loops(prec):
    """B = 4, N = 4, 40 updates at 1,000, 2,000, 3,000 and 20,000 us per update: 2, 5, 7 and 40 shifts.  Every state array, the clocks and every
    tracking error equal the four single-trajectory loops over the scalar entries with a host clock, bit for bit."""
    got, errs, shifts = run_loop(prec, STARTS, PERIODS)
    want_shifts = [sum(clock_ref.shifts_of(p, 40, DT, NP[prec])) for p in PERIODS]
    assert shifts == want_shifts == got["offset"].tolist() and want_shifts[3] == 40 and want_shifts[0] < want_shifts[1] < want_shifts[2]
    assert got["done"].tolist() == [0] * 4
    for b in range(4):
        one, one_errs, one_shifts = run_loop(prec, STARTS[b:b + 1], PERIODS[b:b + 1])
        assert one_shifts == [shifts[b]]
        for k in one:
            assert same(one[k].reshape(-1), np.ascontiguousarray(got[k][b:b + 1]).reshape(-1)), (prec, b, k)
        assert len(errs[b]) == len(one_errs[0]) == shifts[b] and all(same(x, y) and np.isfinite(x).all() for x, y in zip(errs[b], one_errs[0])), b


# ---- 6. capture ----
@pytest.mark.parametrize("prec", PRECS)
def test_one_captured_update_follows_the_times_in_device_memory(prec):
    """xu_old <- xu, simulate_clk, advance_horizon_clk captured ONCE; replayed 12 times with d_sim_time_us rewritten on the stream in front of each replay.
    The times differ per trajectory and per update (0 us among them; several wraps): every array equals the eager sequence after every update."""
    starts, U = (2, 150, 300, 40, 200), 12
    rng = np.random.default_rng(8)
    times = rng.choice([0.0, 300.0, 1000.0, 2100.0, 4000.0, 9000.0, 16000.0], size=(U, len(starts)))
    d_times = f64s(times)
    host = [clock_ref.Clock(DT, NP[prec]) for _ in starts]
    for u in range(U):
        for b, c in enumerate(host):
            c.update(times[u, b])
    assert all(c.shifts >= 1 for c in host) and len({c.shifts for c in host}) > 1

    def make():
        s = MPC[prec](N4, starts, 20)
        s.ck, s.sim_us, s.did = Clocks(s.B), torch.zeros(s.B, dtype=torch.float64, device="cuda"), torch.zeros(s.B, dtype=torch.int32, device="cuda")
        return s

    def update(s):
        s.xu_old.copy_(s.xu)
        s.sol.simulate_clk(plant(), s.xs, s.xu_old, DT, s.ck.prev_sim_us, s.sim_us, SS[prec], eePos=s.ee, done=s.done)
        s.sol.advance_horizon_clk(s.xu, s.xs, s.lam, s.goals, s.ee, s.plan, s.plan_goals, s.offset, s.done, s.err, DT, s.sim_us, s.ck, did_shift=s.did)

    def state(s):
        out = s.state()
        out.update({k: getattr(s.ck, k).cpu().numpy() for k in ("prev_sim_us", "since_s", "shifted")}, did=s.did.cpu().numpy())
        return out

    eager, want = make(), []
    for u in range(U):
        eager.sim_us.copy_(d_times[u])
        update(eager)
        want.append(state(eager))
    assert want[-1]["offset"].tolist() == [c.shifts for c in host]
    rep = make()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        update(rep)
    for u in range(U):
        rep.sim_us.copy_(d_times[u])
        graph.replay()
        got = state(rep)
        for k in got:
            assert same(got[k], want[u][k]), (prec, u, k)


# ---- 7. refusals ----
def test_refusals_write_nothing():
    xu, xs = six("f32")
    xu, xs = xu[:5], xs[:5]
    sol, lib = solver(N4, 5), _lib.load()
    other = solver(N4, 5, 12, 6)
    nan = lambda *s: torch.full(s, NAN, device="cuda")
    d_xs, d_xu, ee = dev(xs.copy()), dev(xu), nan(5, 3)
    toff, sim, done = f64s([0.0] * 5), f64s([2000.0] * 5), torch.zeros(5, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    def simc(h=sol, xs_=d_xs, xu_=d_xu, control=7, dt=DT, toff_=toff, sim_=sim, ss=2e-4, batch=5, fn=lib.mpcg_simulate_clk):
        rc = fn(h._h, plant()._p, control, p(xs_), p(xu_), dt, p(toff_), p(sim_), ss, p(ee), p(done), batch, None)
        return rc, lib.mpcg_last_error(h._h).decode()

    for what, (rc, msg), code in (("null offsets", simc(toff_=None), -1), ("null times", simc(sim_=None), -1), ("null xs", simc(xs_=None), -1),
                                  ("null xu", simc(xu_=None), -1), ("batch", simc(batch=6), -1), ("control size", simc(control=6), -2),
                                  ("state size", simc(h=other), -2), ("sim_step 0", simc(ss=0.0), -1), ("timestep nan", simc(dt=NAN), -1),
                                  ("timestep 0", simc(dt=0.0), -1)):
        assert rc == code and "mpcg_simulate_clk" in msg, (what, rc, msg)
    assert simc(toff_=None, fn=lib.mpcg_simulate_clk_f64)[1].startswith("mpcg_simulate_clk_f64")
    assert simc(batch=0)[0] == 0
    torch.cuda.synchronize()
    assert same(d_xs, xs) and np.isnan(ee.cpu().numpy()).all() and done.tolist() == [0] * 5

    a = {"xu": nan(5, L4), "lam": nan(5, n * N4), "goal": nan(5, 6 * N4), "plan": nan(9, n + m), "goals": nan(9, 6), "err": nan(5),
         "prev": nan(5).double(), "since": nan(5).double()}
    off, shifted, did = (torch.full((5,), v, dtype=torch.int32, device="cuda") for v in (0, 0, -5))

    def adv(h=sol, control=7, xu_=a["xu"], ee_=ee, T=9, stride=0, lead=0, batch=5, off_=off, dt=DT, thr=DT, sim_=sim, prev_=a["prev"], since_=a["since"],
            shifted_=shifted, done_=done, fn=lib.mpcg_advance_horizon_clk):
        rc = fn(h._h, control, p(xu_), p(a["lam"]), p(a["goal"]), p(d_xs), p(ee_), p(a["plan"]), p(a["goals"]), T, stride, lead, p(off_), p(done_), p(a["err"]),
                dt, thr, p(sim_), p(prev_), p(since_), p(shifted_), p(did), batch, None)
        return rc, lib.mpcg_last_error(h._h).decode()

    for what, (rc, msg), code in (("null times", adv(sim_=None), -1), ("null prev", adv(prev_=None), -1), ("null since", adv(since_=None), -1),
                                  ("null shifted", adv(shifted_=None), -1), ("null eePos", adv(ee_=None), -1), ("null xu", adv(xu_=None), -1),
                                  ("null offset", adv(off_=None), -1), ("null done", adv(done_=None), -1), ("batch", adv(batch=6), -1),
                                  ("control size", adv(control=6), -2), ("state size", adv(h=other), -2), ("no plan", adv(T=0), -1), ("lead", adv(lead=N4), -1),
                                  ("stride", adv(stride=8), -1), ("timestep 0", adv(dt=0.0), -1), ("threshold nan", adv(thr=NAN), -1)):
        assert rc == code and "mpcg_advance_horizon_clk" in msg, (what, rc, msg)
    assert adv(sim_=None, fn=lib.mpcg_advance_horizon_clk_f64)[1].startswith("mpcg_advance_horizon_clk_f64")
    assert adv(batch=0)[0] == 0
    torch.cuda.synchronize()
    assert all(np.isnan(t.cpu().numpy()).all() for t in a.values()) and off.tolist() == [0] * 5 and done.tolist() == [0] * 5
    assert shifted.tolist() == [0] * 5 and did.tolist() == [-5] * 5 and same(d_xs, xs)


def test_python_checks_dtypes_and_shapes():
    xu, xs = six("f32")
    sol = solver(N4, 8)
    t, s = f64s([0.0] * 6), f64s([100.0] * 6)
    with pytest.raises(TypeError):
        sol.simulate_clk(plant(), dev(xs).double(), dev(xu), DT, t, s)
    with pytest.raises(ValueError):
        sol.simulate_clk(plant(), dev(xs), dev(xu), DT, t.float(), s)
    with pytest.raises(ValueError):
        sol.simulate_clk(plant(), dev(xs), dev(xu), DT, t, s[:5])
    z = lambda *sh: torch.zeros(*sh, device="cuda")
    i32 = lambda: torch.zeros(6, dtype=torch.int32, device="cuda")
    args = lambda lam: (dev(xu), dev(xs), lam, z(6, 6 * N4), z(6, 3), z(9, n + m), z(9, 6), i32(), i32(), z(6), DT, s)
    with pytest.raises(TypeError):
        sol.advance_horizon_clk(*args(z(6, n * N4).double()), Clocks(6))
    bad = Clocks(6)
    bad.shifted = bad.shifted.long()
    with pytest.raises(ValueError):
        sol.advance_horizon_clk(*args(z(6, n * N4)), bad)
    with pytest.raises(ValueError):
        sol.advance_horizon_clk(*args(z(6, n * N4)), Clocks(5))


# ---- 8. guard bands ----
@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("prec", PRECS)
def test_simulate_clk_in_the_arena(prec, mode):
    """N = 3, B = 5: trajectory 1 frozen, trajectory 3 with a NaN time (done becomes 2); their rows of xs and eePos are never written."""
    N, Bt, dt = 3, 5, NP[prec]
    xu, xs = (np.ascontiguousarray(a, dt) for a in _windows(N, Bt))
    Lz = A.zlen(n, m, N)
    bad = (1, 3)
    done_mask = np.ones(Bt, bool)
    done_mask[3] = False
    specs = [arena.spec("xs", dt, Bt * n, "inout", None, n, n, A.rows_mask(Bt, n, bad)), arena.spec("xu", dt, Bt * Lz, "in", None, n + m, Lz),
             arena.spec("toff", np.float64, Bt, "in"), arena.spec("sim", np.float64, Bt, "in"),
             arena.spec("eePos", dt, Bt * 3, "out", None, 3, 3, A.rows_mask(Bt, 3, bad)), arena.spec("done", np.int32, Bt, "inout", None, 1, 1, done_mask)]
    sol = solver(N, Bt)

    def call(a):
        sol.simulate_clk(plant(), a["xs"].view(Bt, -1), a["xu"].view(Bt, -1), DT, a["toff"], a["sim"], SS[prec], eePos=a["eePos"].view(Bt, 3), done=a["done"])
    out = arena.both_ways(specs, mode, {"xs": xs, "xu": xu, "toff": [0.0, 0.0, 15000.0, 0.0, 200.0], "sim": [650.0, 650.0, 2100.0, NAN, 0.0],
                                        "done": np.array([0, 1, 0, 0, 0], np.int32)}, call, f"simulate_clk {prec}")
    assert out["done"].tolist() == [0, 1, 0, 2, 0]
    assert out["xs"].reshape(Bt, n)[4].tobytes() == xs[4].tobytes() and out["xs"].reshape(Bt, n)[0].tobytes() != xs[0].tobytes()


@functools.lru_cache(maxsize=None)
def _windows(N, Bt):
    from mpcgpu_amd import iiwa
    xu, _, xs = iiwa.random_windows(N, Bt, 11 + N)
    return xu, xs


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("per_traj", [False, True], ids=["shared-plan", "plan-per-trajectory"])
@pytest.mark.parametrize("prec", PRECS)
def test_advance_horizon_clk_in_the_arena(prec, per_traj, mode):
    """N = 3, four trajectories: 0 shifts (and wraps), 1 does not shift (x_0 and its clock only), 2 shifts at the end of its plan, 3 is frozen (did_shift
    only)."""
    N, Bt, T, dt = 3, 4, 9, NP[prec]
    rng = np.random.default_rng([N, int(per_traj), 7])
    f = lambda *s: rng.standard_normal(s).astype(dt)
    Lz, rows = A.zlen(n, m, N), (Bt if per_traj else 1)
    keep = lambda per, head=0: _mask(Bt, per, (1, 3), head)
    lam_mask = keep(n * N)
    lam_mask[:, n * (N - 1):] = True
    specs = [arena.spec("xu", dt, Bt * Lz, "inout", None, n + m, Lz, _mask(Bt, Lz, (3,), 0) | _mask(Bt, Lz, (1,), n)),
             arena.spec("lambda", dt, Bt * n * N, "inout", None, n, n * N, lam_mask), arena.spec("goal", dt, Bt * 6 * N, "inout", None, 6, 6 * N, keep(6 * N)),
             arena.spec("xs", dt, Bt * n, "in", None, n, n), arena.spec("eePos", dt, Bt * 3, "in", None, 3, 3),
             arena.spec("xu_traj", dt, rows * T * (n + m), "in", None, n + m, T * (n + m)), arena.spec("goal_traj", dt, rows * T * 6, "in", None, 6, T * 6),
             arena.spec("traj_offset", np.int32, Bt, "inout", None, 1, 1, keep(1)), arena.spec("done", np.int32, Bt, "inout", None, 1, 1, keep(1)),
             arena.spec("tracking_error", dt, Bt, "out", None, 1, 1, keep(1)), arena.spec("sim", np.float64, Bt, "in"),
             arena.spec("prev", np.float64, Bt, "inout", None, 1, 1, _mask(Bt, 1, (3,), 0)), arena.spec("since", np.float64, Bt, "inout", None, 1, 1, _mask(Bt, 1, (3,), 0)),
             arena.spec("shifted", np.int32, Bt, "inout", None, 1, 1, _mask(Bt, 1, (3,), 0)), arena.spec("did_shift", np.int32, Bt, "out")]
    inputs = {"xu": f(Bt, Lz), "lambda": f(Bt, n * N), "goal": f(Bt, 6 * N), "xs": f(Bt, n), "eePos": f(Bt, 3), "xu_traj": f(rows, T, n + m),
              "goal_traj": f(rows, T, 6), "traj_offset": np.array([0, 1, T - 1, 2], np.int32), "done": np.array([0, 0, 0, 7], np.int32),
              "sim": [2000.0, 2000.0, 3000.0, 2000.0], "prev": [0.0, 100.0, 200.0, 300.0], "since": [0.0150, 0.001, 0.0140, 0.0150],
              "shifted": np.array([0, 0, 0, 0], np.int32)}
    sol = solver(N, Bt)

    def call(a):
        v = lambda name: a[name].view(Bt, -1)
        plan = lambda name, w: a[name].view(Bt, T, w) if per_traj else a[name].view(T, w)
        ck = Clocks(Bt)
        ck.prev_sim_us, ck.since_s, ck.shifted = a["prev"], a["since"], a["shifted"]
        sol.advance_horizon_clk(v("xu"), v("xs"), v("lambda"), v("goal"), v("eePos"), plan("xu_traj", n + m), plan("goal_traj", 6), a["traj_offset"], a["done"],
                                a["tracking_error"], DT, a["sim"], ck, did_shift=a["did_shift"], xu_fill_lead=N - 1 if per_traj else 0)
    out = arena.both_ways(specs, mode, inputs, call, f"advance_horizon_clk {prec} per_traj={per_traj}")
    assert out["did_shift"].tolist() == [1, 0, 1, 0] and out["traj_offset"].tolist() == [1, 1, T, 2] and out["done"].tolist() == [0, 0, 1, 7]
    assert out["prev"].tolist() == [2000.0, 2000.0, 3000.0, 300.0] and out["shifted"].tolist() == [0, 0, 0, 0]


def _mask(Bt, per, rows, head):
    """[Bt, per] bool: True (never written) for `rows`, from element `head` of each on"""
    mk = np.zeros((Bt, per), bool)
    mk[list(rows), head:] = True
    return mk


# ---- 9. the example ----
@pytest.mark.parametrize("f64", [False, True], ids=["float", "double"])
def test_mpc_closed_loop_example_with_periods(f64):
    """examples/mpc_closed_loop.cpp --periods-us: the batched run keeps its clocks on the device and calls the _clk entries; 17 updates at 1,000, 2,000,
    3,000 and 20,000 us shift 1, 2, 3 and 17 times — what the host ShiftClock gives for each period."""
    from mpcgpu_amd import build
    exe = build.build_mpc_closed_loop_f64() if f64 else build.build_mpc_closed_loop()
    r = subprocess.run([exe, "--batch", "4", "--knots", "16", "--updates", "17", "--periods-us", "1000,2000,3000,20000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    want = [sum(clock_ref.shifts_of(p, 17, float(np.float32(1.0 / 64)), np.float64 if f64 else np.float32)) for p in PERIODS]
    assert want == [1, 2, 3, 17]
    assert out["ok"] is True and out["periods_us"] == list(PERIODS) and out["shifts"] == want == out["expected_shifts"]
    errs = out["tracking_errors"]
    assert [len(e) for e in errs] == want and all(np.isfinite(e).all() for e in errs)
