"""GPU: non-finite containment of the plant and MPC-loop kernels — mpcg_generate_kkt, mpcg_compute_merit (their _xuref forms, every build, the
double entries), mpcg_simulate, mpcg_advance_horizon, mpcg_inverse_dynamics and mpcg_line_search_step(_rho), iiwa plant, once more with a
gravity clone; the _xuref forms with a limits clone (COST = 2), mpcg_simulate with a saturating plant, mpcg_simulate_clk and
mpcg_advance_horizon_clk.  N = 4, B = 6: three KKT items per trajectory, so a wavefront of four 16-lane items and a packed pair ("kkt_f32" = 1,
"merit_f32" = 1) both straddle trajectories, and the last wavefront has dead rows that redo trajectory 5.

One floating-point input array of trajectories {1}, {5} or {0, 3} is poisoned (tests/containment.py); every output of every other trajectory
must carry the bits of the same call on healthy data.  Integer arrays are never poisoned and, where they are outputs, are checked too.  No
tolerance.  The trip counts of these kernels come from host arguments (containment table)."""
import functools

import numpy as np
import pytest
import torch

import arena_specs as A
import containment as ct
from mpcgpu_amd import iiwa
from test_gpu_clocks import SIX
from test_gpu_containment_linsys import ids, runner, solver

pytestmark = pytest.mark.gpu
n, m, N, B = 14, 7, 4, ct.B
L = (n + m) * N - m
DT = iiwa.TIMESTEP
MU = 10.0
SS = float(np.float32(2e-4))
NP = {"f32": np.float32, "f64": np.float64}
T_PLAN = N + 6
QC, EE = 0.5, 0.75


@functools.lru_cache(maxsize=None)
def plant(gravity=False):
    from mpcgpu_amd import Plant
    return Plant().with_gravity((0.0, 0.0, 9.81)) if gravity else Plant()


@functools.lru_cache(maxsize=None)
def windows(prec):
    """(xu, goals [B, 6 N], xs, dz, plan [B, T, 21]) in the entry's type, read-only and shared."""
    xu, goals, xs = iiwa.random_windows(N, B, 11 + N)
    rng = np.random.default_rng(3000 + N)
    dz = 0.05 * rng.standard_normal(xu.shape)
    plan = 0.5 * rng.standard_normal((B, T_PLAN, n + m))
    out = tuple(np.ascontiguousarray(a, NP[prec]) for a in (xu, goals.reshape(B, -1), xs, dz, plan))
    for a in out:
        a.flags.writeable = False
    return out


OFFSETS = np.array([0, T_PLAN - 2, 2, -3, 1, 3], np.int32)      # rows inside the plan, clamped at its end and below its start


def xuref(d):
    from mpcgpu_amd import XuRef
    return XuRef(d["plan"], traj_offset=d["traj_offset"], ee_cost=EE, q_cost=QC, qd_relative=True, u_relative=True)


# ---- KKT assembly ----
KKT_CASES = [("f32", o + (("integrator", i),)) for o in A.KKT_BUILDS for i in (0, 1)] + \
            [("f64", (("kkt_analytic", a), ("integrator", i))) for a in (1, 0) for i in (0, 1)]


@functools.lru_cache(maxsize=None)
def window_bounds(prec):
    """((q_lo, q_hi), (qd_lo, qd_hi), (u_lo, u_hi)) from the windows' own values: per joint the lower and upper third of what the six trajectories
    visit (tests/chain_cost_cases.py::bounds_of), so every kind of limit is violated by some knots and the violations are non-zero."""
    from chain_cost_cases import bounds_of
    rows = np.concatenate([windows(prec)[0].astype(np.float64), np.zeros((B, m))], axis=1).reshape(B, N, n + m)
    return bounds_of(rows[:, :, :7].reshape(-1, 7)), bounds_of(rows[:, :, 7:n].reshape(-1, 7)), bounds_of(rows[:, :N - 1, n:].reshape(-1, 7))


@functools.lru_cache(maxsize=None)
def limits_plant(prec, gravity=False, sim_saturate=False):
    """A limits clone (COST = 2 in the KKT and merit kernels) of the plain or the gravity plant; sim_saturate: simulate clamps the controls."""
    from chain_cost_cases import WEIGHTS
    q, qd, u = (tuple([float(v) for v in side] for side in pair) for pair in window_bounds(prec))
    return plant(gravity).with_limits(q=q, qd=qd, u=u, q_weight=WEIGHTS[0], qd_weight=WEIGHTS[1], u_weight=WEIGHTS[2], sim_saturate=sim_saturate)


def kkt_sweep(prec, opts, form, gravity, limits=False):
    xu, goals, xs, _, plan = windows(prec)
    dt = NP[prec]
    sol = solver(N, opts)
    pl = limits_plant(prec, gravity) if limits else plant(gravity)
    inputs = {"xu": xu, "xs": xs, "goals": goals}
    if form == "xuref":
        inputs.update(plan=plan, traj_offset=OFFSETS)
    names = ("G", "C", "g", "c")

    def call(d):
        if form == "xuref":
            out = sol.generate_kkt_xuref(pl, d["goals"], d["xs"], d["xu"], DT, iiwa.QD_COST, iiwa.r_cost(N), xuref(d))
        else:
            out = sol.generate_kkt(pl, d["goals"], d["xs"], d["xu"], DT, iiwa.QD_COST, iiwa.r_cost(N))
        d.update(zip(names, out))
    ct.sweep(f"generate_kkt{'_xuref' if form == 'xuref' else ''} {prec} {ids(opts)} gravity={gravity} limits={limits}", inputs,
             ["xu", "xs", "goals"] + (["plan"] if form == "xuref" else []), runner(call, dict.fromkeys(names)), blocks={"xu": n + m, "goals": 6, "plan": n + m})


@pytest.mark.parametrize("form", ["plain", "xuref"])
@pytest.mark.parametrize("prec,opts", KKT_CASES, ids=[p + "-" + ids(o) for p, o in KKT_CASES])
def test_generate_kkt(prec, opts, form):
    """Both gradient routes, the float builds with one and with two knots per lane, both integrators, the double entries; xu, xs, the goals and —
    the _xuref form, a plan per trajectory — the plan rows poisoned in turn.  (Every element of the four outputs is written by every call.)"""
    kkt_sweep(prec, opts, form, False)


@pytest.mark.parametrize("prec,opts", [("f32", ()), ("f32", (("kkt_f32", 1),)), ("f64", ())], ids=["f32", "f32-packed", "f64"])
def test_generate_kkt_with_a_gravity_clone(prec, opts):
    kkt_sweep(prec, opts, "plain", True)


@pytest.mark.parametrize("prec,opts", KKT_CASES, ids=[p + "-" + ids(o) for p, o in KKT_CASES])
def test_generate_kkt_xuref_with_a_limits_clone(prec, opts):
    """COST = 2 of every build: bounds of every kind inside the range the windows visit (window_bounds), so the indicator of a poisoned value
    decides between a violation and none next to healthy violations."""
    kkt_sweep(prec, opts, "xuref", False, True)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_gravity_and_limits_together(prec):
    """A limits clone of the gravity clone, KKT and merit."""
    kkt_sweep(prec, (), "xuref", True, True)
    merit_sweep(prec, (), "xuref", True, True)


# ---- merit ----
MERIT_CASES = [("f32", ()), ("f32", (("merit_f32", 1),)), ("f64", ()), ("f32", (("integrator", 1),)), ("f32", (("merit_f32", 1), ("integrator", 1)))]
STEPS3 = (0.0, -1.0, -0.5)


def merit_sweep(prec, opts, form, gravity, limits=False):
    xu, goals, xs, dz, plan = windows(prec)
    sol = solver(N, opts)
    pl = limits_plant(prec, gravity) if limits else plant(gravity)
    inputs = {"xu": xu, "dz": dz, "xs": xs, "goals": goals}
    if form == "xuref":
        inputs.update(plan=plan, traj_offset=OFFSETS)

    def call(d):
        args = (pl, d["goals"], d["xs"], d["xu"], d["dz"], STEPS3, DT, MU, iiwa.QD_COST, iiwa.r_cost(N))
        if form == "xuref":
            sol.compute_merit_xuref(*args, xuref(d), merit=d["merit"])
        else:
            sol.compute_merit(*args, merit=d["merit"])
    ct.sweep(f"compute_merit{'_xuref' if form == 'xuref' else ''} {prec} {ids(opts)} gravity={gravity} limits={limits}", inputs,
             ["xu", "dz", "xs", "goals"] + (["plan"] if form == "xuref" else []), runner(call, {"merit": ((B, len(STEPS3)), NP[prec])}),
             blocks={"xu": n + m, "dz": n + m, "goals": 6, "plan": n + m})


@pytest.mark.parametrize("form", ["plain", "xuref"])
@pytest.mark.parametrize("prec,opts", MERIT_CASES, ids=[p + "-" + ids(o) for p, o in MERIT_CASES])
def test_compute_merit(prec, opts, form):
    """Three step sizes, 0 among them: 72 items of one 16-lane group each, two to a group in packed float; the knots of a (trajectory, step size)
    row are summed across groups."""
    merit_sweep(prec, opts, form, False)


@pytest.mark.parametrize("prec,opts", [("f32", ()), ("f32", (("merit_f32", 1),)), ("f64", ())], ids=["f32", "f32-packed", "f64"])
def test_compute_merit_with_a_gravity_clone(prec, opts):
    merit_sweep(prec, opts, "plain", True)


@pytest.mark.parametrize("prec,opts", MERIT_CASES, ids=[p + "-" + ids(o) for p, o in MERIT_CASES])
def test_compute_merit_xuref_with_a_limits_clone(prec, opts):
    """COST = 2 of every merit build, at the three trial iterates."""
    merit_sweep(prec, opts, "xuref", False, True)


# ---- plant simulation ----
@pytest.mark.parametrize("gravity", [False, True], ids=["plain", "gravity"])
@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_simulate(prec, integ, gravity):
    """Three full substeps and a remainder, four trajectories per wavefront; the plant states and the plans poisoned; eePos checked as well."""
    xu, _, xs, _, _ = windows(prec)
    sol = solver(N, (("sim_integrator", integ),))
    run = runner(lambda d: sol.simulate(plant(gravity), d["xs"], d["xu"], DT, 0.0, 650.0, SS, eePos=d["eePos"]), {"xs": None, "eePos": ((B, 3), NP[prec])})
    ct.sweep(f"simulate {prec} sim_integrator={integ} gravity={gravity}", {"xs": xs, "xu": xu}, ["xs", "xu"], run, blocks={"xu": n + m})


def clamped(prec, knots):
    """Do the bounds of limits_plant clamp some, and not all, of the controls of these knots?"""
    lo, hi = window_bounds(prec)[2]
    u = np.concatenate([windows(prec)[0].astype(np.float64), np.zeros((B, m))], axis=1).reshape(B, N, n + m)[:, knots, n:]
    out = (u < lo) | (u > hi)
    return out.any() and not out.all()


@pytest.mark.parametrize("integ", [0, 1])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_simulate_with_a_saturating_plant(prec, integ):
    """SATURATE = 1: the control applied (knot 0 of each plan) is clamped for some joints of some trajectories and passes for others; a NaN passes
    the clamp."""
    xu, _, xs, _, _ = windows(prec)
    assert clamped(prec, [0])
    pl = limits_plant(prec, sim_saturate=True)
    sol = solver(N, (("sim_integrator", integ),))
    run = runner(lambda d: sol.simulate(pl, d["xs"], d["xu"], DT, 0.0, 650.0, SS, eePos=d["eePos"]), {"xs": None, "eePos": ((B, 3), NP[prec])})
    plain = runner(lambda d: sol.simulate(plant(), d["xs"], d["xu"], DT, 0.0, 650.0, SS, eePos=d["eePos"]), {"xs": None, "eePos": ((B, 3), NP[prec])})
    assert not np.array_equal(run({"xs": xs, "xu": xu})["xs"], plain({"xs": xs, "xu": xu})["xs"])          # (the clamp acted)
    ct.sweep(f"simulate saturating {prec} sim_integrator={integ}", {"xs": xs, "xu": xu}, ["xs", "xu"], run, blocks={"xu": n + m})


# Six (time offset, simulated time) pairs [us], tests/test_gpu_clocks.py's SIX: with an end-effector output the four groups of the first wavefront
# have 11, 12, 2 and 11 rounds, the second 3 and 1 — a poisoned time ends its trajectory's schedule (no rounds) and so changes the trip count of
# the wavefront it shares with healthy trajectories.
assert SIX == [(0, 2000), (15000, 2100), (15000, 100), (46000, 2000), (15500, 300), (4000, 0)]
ONE =("nan_one@first", "inf_one@first", "huge")               # what tests/containment.py offers for an array of one element per trajectory


@pytest.mark.parametrize("saturate", [False, True], ids=["plain", "saturating"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_simulate_clk(prec, saturate):
    """CLOCK = 1 (and with SATURATE = 1): the one plant kernel whose wavefront trip count depends on other trajectories' floating-point data, the
    maximum of four groups' round counts.  xs, xu and the two double time arrays poisoned; xs, eePos and done of the healthy trajectories.  A
    NaN, infinite or 1e308 simulated time is no schedule (done = 2, nothing else written); a 1e308 offset is clamped to the last control."""
    xu, _, xs, _, _ = windows(prec)
    assert not saturate or clamped(prec, [0, 1, 2])
    pl = limits_plant(prec, sim_saturate=True) if saturate else plant()
    sol = solver(N)
    inputs = {"xs": xs, "xu": xu, "toff": np.array([t[0] for t in SIX], np.float64), "sim": np.array([t[1] for t in SIX], np.float64),
              "done": np.zeros(B, np.int32)}
    run = runner(lambda d: sol.simulate_clk(pl, d["xs"], d["xu"], DT, d["toff"], d["sim"], SS, eePos=d["eePos"], done=d["done"]),
                 {"xs": None, "eePos": ((B, 3), NP[prec]), "done": None})
    clean = run(inputs)
    assert clean["done"].tolist() == [0] * B and np.isfinite(clean["xs"]).all() and np.isfinite(clean["eePos"]).all()
    tag = f"simulate_clk {prec} saturate={saturate}"

    def own(out, pset, case):
        if "[sim <-" in case or ("[toff <-" in case and "huge" not in case):          # times that are no schedule
            assert all(out["done"][b] == 2 and np.array_equal(out["xs"][b], xs[b]) and np.isnan(out["eePos"][b]).all() for b in pset), (case, pset)
    ct.sweep(tag, inputs, ["xs", "xu"], run, blocks={"xu": n + m})
    ct.sweep(tag, inputs, ["toff", "sim"], run, only=ONE, own=own)


# ---- horizon shift ----
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_advance_horizon_shift(prec):
    """shift = 1 with a plan per trajectory: every float array of one trajectory poisoned in turn; the integer arrays of the healthy ones
    (traj_offset, done) are outputs like the rest.  Trajectory 2 is frozen on entry, 3 uses its plan up."""
    dt = NP[prec]
    rng = np.random.default_rng(N)
    f = lambda *s: rng.standard_normal(s).astype(dt)
    inputs = {"xu": f(B, L), "lambda": f(B, n * N), "goal": f(B, 6 * N), "xs": f(B, n), "eePos": f(B, 3), "xu_traj": f(B, T_PLAN, n + m),
              "goal_traj": f(B, T_PLAN, 6), "traj_offset": np.array([0, T_PLAN - N - 1, 2, T_PLAN - 1, 1, 3], np.int32),
              "done": np.array([0, 0, 7, 0, 0, 0], np.int32)}
    sol = solver(N)

    def call(d):
        sol.advance_horizon(True, d["xu"], d["xs"], d["lambda"], d["goal"], d["eePos"], d["xu_traj"], d["goal_traj"], d["traj_offset"], d["done"],
                            d["tracking_error"], xu_fill_lead=N - 1)
    outs = {"xu": None, "lambda": None, "goal": None, "traj_offset": None, "done": None, "tracking_error": ((B,), dt)}
    run = runner(call, outs)
    clean = run(inputs)
    assert clean["traj_offset"].tolist() == [1, T_PLAN - N, 2, T_PLAN, 2, 4] and clean["done"].tolist() == [0, 0, 7, 1, 0, 0]
    ct.sweep(f"advance_horizon shift {prec}", inputs, ["xu", "lambda", "goal", "xs", "eePos", "xu_traj", "goal_traj"], run,
             blocks={"xu": n + m, "goal": 6, "xu_traj": n + m, "goal_traj": 6})


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_advance_horizon_without_shift(prec):
    dt = NP[prec]
    rng = np.random.default_rng(N + 1)
    inputs = {"xu": rng.standard_normal((B, L)).astype(dt), "xs": rng.standard_normal((B, n)).astype(dt), "done": np.array([0, 0, 7, 0, 0, 0], np.int32)}
    sol = solver(N)
    run = runner(lambda d: sol.advance_horizon(False, d["xu"], d["xs"], done=d["done"]), {"xu": None, "done": None})
    ct.sweep(f"advance_horizon no shift {prec}", inputs, ["xu", "xs"], run, blocks={"xu": n + m})


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_advance_horizon_clk(prec):
    """The shift decided per trajectory from clock state on the device, shift_threshold_s = timestep / 2: trajectory 0 shifts and wraps, 1 does
    neither, 2 has shifted in this timestep and only wraps, 3 shifts at the end of its plan (done becomes 1), 4 shifts without a wrap, 5 is
    frozen on entry.  Every float array of test_advance_horizon_shift and the three double clock arrays poisoned in turn; traj_offset, done,
    shifted and did_shift are never poisoned and are outputs like the rest.  (prev_sim_us is written, never read: only the frozen trajectory 5
    keeps a poisoned value, which is what reaches an output.)"""
    from mpcgpu_amd import Clocks
    dt = NP[prec]
    rng = np.random.default_rng(N + 2)
    f = lambda *s: rng.standard_normal(s).astype(dt)
    thr = DT / 2
    since0, sim = [0.0150, 0.002, 0.0150, 0.008, 0.008, 0.0150], [1000.0, 2000.0, 1000.0, 1000.0, 1000.0, 1000.0]
    assert since0[0] + 1e-3 > DT and thr < since0[3] + 1e-3 < DT and since0[1] + 2e-3 < thr
    inputs = {"xu": f(B, L), "lambda": f(B, n * N), "goal": f(B, 6 * N), "xs": f(B, n), "eePos": f(B, 3), "xu_traj": f(B, T_PLAN, n + m),
              "goal_traj": f(B, T_PLAN, 6), "traj_offset": np.array([0, T_PLAN - N - 1, 2, T_PLAN - 1, 1, 3], np.int32),
              "done": np.array([0, 0, 0, 0, 0, 7], np.int32), "sim": np.array(sim), "prev": np.array([500.0, 600.0, 700.0, 800.0, 900.0, 950.0]),
              "since": np.array(since0), "shifted": np.array([0, 0, 1, 0, 0, 0], np.int32)}
    sol = solver(N)

    def call(d):
        ck = Clocks(B)
        ck.prev_sim_us, ck.since_s, ck.shifted = d["prev"], d["since"], d["shifted"]
        sol.advance_horizon_clk(d["xu"], d["xs"], d["lambda"], d["goal"], d["eePos"], d["xu_traj"], d["goal_traj"], d["traj_offset"], d["done"],
                                d["tracking_error"], DT, d["sim"], ck, did_shift=d["did_shift"], shift_threshold_s=thr, xu_fill_lead=N - 1)
    outs = {"xu": None, "lambda": None, "goal": None, "traj_offset": None, "done": None, "tracking_error": ((B,), dt), "prev": None, "since": None,
            "shifted": None, "did_shift": ((B,), np.int32)}
    run = runner(call, outs)
    clean = run(inputs)
    assert clean["did_shift"].tolist() == [1, 0, 0, 1, 1, 0] and clean["shifted"].tolist() == [0, 0, 0, 1, 1, 0]
    assert clean["traj_offset"].tolist() == [1, T_PLAN - N - 1, 2, T_PLAN, 2, 3] and clean["done"].tolist() == [0, 0, 0, 1, 0, 7]
    assert clean["prev"].tolist() == sim[:5] + [950.0] and clean["since"][5] == since0[5] and (clean["since"][[0, 2]] < 1e-3).all()
    tag = f"advance_horizon_clk {prec}"
    ct.sweep(tag, inputs, ["xu", "lambda", "goal", "xs", "eePos", "xu_traj", "goal_traj"], run,
             blocks={"xu": n + m, "goal": 6, "xu_traj": n + m, "goal_traj": 6})
    ct.sweep(tag, inputs, ["sim", "prev", "since"], run, only=ONE)


# ---- inverse dynamics ----
@pytest.mark.parametrize("gravity", [False, True], ids=["plain", "gravity"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_inverse_dynamics(prec, gravity):
    """count = 6 independent states, four per wavefront: q, qd and qdd of one state poisoned."""
    rng = np.random.default_rng(7)
    inputs = {k: rng.standard_normal((B, 7)).astype(NP[prec]) for k in ("q", "qd", "qdd")}
    sol = solver(N)
    run = runner(lambda d: sol.inverse_dynamics(plant(gravity), d["q"], d["qd"], d["qdd"], tau=d["tau"]), {"tau": ((B, 7), NP[prec])})
    ct.sweep(f"inverse_dynamics {prec} gravity={gravity}", inputs, ["q", "qd", "qdd"], run, blocks={"q": 7, "qd": 7, "qdd": 7})


# ---- line-search step ----
LS_STEPS = (-1.0, -0.5, -0.25)


@pytest.mark.parametrize("rho", [False, True], ids=["step", "step_rho"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_line_search_step(prec, rho):
    """A merit row, merit_ref[b], dz, xu and — _rho — rho[b] and drho[b] of the poisoned trajectories; step, xu, merit_ref, rho, drho and done of
    the healthy ones.  Healthy trajectories take every outcome: a step at each index, no step, and (under _rho) frozen."""
    dt = NP[prec]
    rng = np.random.default_rng(21)
    merit = np.array([[12, 8, 9], [11, 12, 13], [5, 7, 6], [10, 9.5, 10], [3, 2, 1], [11, 8, 8]], dt)
    inputs = {"merit": merit, "merit_ref": np.full(B, 10, dt), "dz": rng.standard_normal((B, L)).astype(dt), "xu": rng.standard_normal((B, L)).astype(dt)}
    poisonable = ["merit", "merit_ref", "dz", "xu"]
    outs = {"step": ((B,), np.int32), "xu": None, "merit_ref": None}
    if rho:
        inputs.update(rho=np.array([1e-3, 9.9, 0.5, 3e-2, 1.7, 5.0], dt), drho=np.array([1, 1.3, 1.2, 0.9, 1.0, 2.0], dt),
                      done=np.array([0, 0, 0, 0, 1, 0], np.uint8))
        poisonable += ["rho", "drho"]
        outs.update(rho=None, drho=None, done=None)
    sol = solver(N)

    def call(d):
        if rho:
            sol.line_search_step_rho(d["merit"], LS_STEPS, d["merit_ref"], d["dz"], d["xu"], d["rho"], d["drho"], d["done"], step=d["step"])
        else:
            sol.line_search_step(d["merit"], LS_STEPS, d["merit_ref"], d["dz"], d["xu"], step=d["step"])
    run = runner(call, outs)
    assert run(inputs)["step"].tolist() == [1, -1, 0, 1, -2 if rho else 2, 1]
    ct.sweep(f"line_search_step{'_rho' if rho else ''} {prec}", inputs, poisonable, run, blocks={"dz": n + m, "xu": n + m})
