"""GPU: non-finite containment of the plant and MPC-loop kernels — mpcg_generate_kkt, mpcg_compute_merit (their _xuref forms, every build, the
double entries), mpcg_simulate, mpcg_advance_horizon, mpcg_inverse_dynamics and mpcg_line_search_step(_rho), iiwa plant, once more with a
gravity clone.  N = 4, B = 6: three KKT items per trajectory, so a wavefront of four 16-lane items and a packed pair ("kkt_f32" = 1,
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


def kkt_sweep(prec, opts, form, gravity):
    xu, goals, xs, _, plan = windows(prec)
    dt = NP[prec]
    sol = solver(N, opts)
    inputs = {"xu": xu, "xs": xs, "goals": goals}
    if form == "xuref":
        inputs.update(plan=plan, traj_offset=OFFSETS)
    names = ("G", "C", "g", "c")

    def call(d):
        if form == "xuref":
            out = sol.generate_kkt_xuref(plant(gravity), d["goals"], d["xs"], d["xu"], DT, iiwa.QD_COST, iiwa.r_cost(N), xuref(d))
        else:
            out = sol.generate_kkt(plant(gravity), d["goals"], d["xs"], d["xu"], DT, iiwa.QD_COST, iiwa.r_cost(N))
        d.update(zip(names, out))
    ct.sweep(f"generate_kkt{'_xuref' if form == 'xuref' else ''} {prec} {ids(opts)} gravity={gravity}", inputs,
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


# ---- merit ----
MERIT_CASES = [("f32", ()), ("f32", (("merit_f32", 1),)), ("f64", ()), ("f32", (("integrator", 1),)), ("f32", (("merit_f32", 1), ("integrator", 1)))]
STEPS3 = (0.0, -1.0, -0.5)


def merit_sweep(prec, opts, form, gravity):
    xu, goals, xs, dz, plan = windows(prec)
    sol = solver(N, opts)
    inputs = {"xu": xu, "dz": dz, "xs": xs, "goals": goals}
    if form == "xuref":
        inputs.update(plan=plan, traj_offset=OFFSETS)

    def call(d):
        args = (plant(gravity), d["goals"], d["xs"], d["xu"], d["dz"], STEPS3, DT, MU, iiwa.QD_COST, iiwa.r_cost(N))
        if form == "xuref":
            sol.compute_merit_xuref(*args, xuref(d), merit=d["merit"])
        else:
            sol.compute_merit(*args, merit=d["merit"])
    ct.sweep(f"compute_merit{'_xuref' if form == 'xuref' else ''} {prec} {ids(opts)} gravity={gravity}", inputs,
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
