"""GPU: the plant and MPC-loop kernels (KKT assembly, merit, line-search step, plant simulation, horizon shift, inverse dynamics) inside a
guard-banded arena (tests/arena.py): 14 x 7 at (N, B) = (2, 1), the smallest horizon, and (3, 5), an odd number of knots — with two knots per
lane ("kkt_f32" = 1) or two items per lane group ("merit_f32" = 1) the last lane or group is half empty.  Every case in both layouts, and bit
for bit against the same call on separately allocated tensors, which the suites of each entry pin to their float64 restatements
(tests/test_gpu_kkt.py, _merit.py, _merit_f32.py, _merit_f64.py, _rho.py, _simulate.py, _simulate_f64.py, _gravity.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arena
import arena_specs as A
from mpcgpu_amd import iiwa

pytestmark = pytest.mark.gpu
n, m = 14, 7
PRECS = ("f32", "f64")
DT = iiwa.TIMESTEP
MU = 10.0
SS = float(np.float32(2e-4))                            # the substep both precisions take ten of per 2,000 us (include/mpcg.h, mpcg_simulate_f64)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def plant():
    from mpcgpu_amd import Plant
    return Plant()


def solver(N, Bt, opts=(), state_size=14, control_size=None):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=Bt, state_size=state_size, control_size=control_size)
    for key, value in opts:
        sol.set_option(key, value)
    return sol


@functools.lru_cache(maxsize=None)
def windows(prec, N, Bt):
    """(xu, goals [Bt, 6 N], xs, dz) in the entry's type, read-only and shared."""
    xu, goals, xs = iiwa.random_windows(N, Bt, 11 + N)
    dz = 0.05 * np.random.default_rng(1000 + N).standard_normal(xu.shape)
    out = tuple(np.ascontiguousarray(a, A.DT[prec]) for a in (xu, goals.reshape(Bt, -1), xs, dz))
    for a in out:
        a.flags.writeable = False
    return out


KKT_CASES = [("f32", opts) for opts in A.KKT_BUILDS] + [("f64", ())]


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("N,Bt", A.PLANT_NB)
@pytest.mark.parametrize("prec,opts", KKT_CASES, ids=[p + "-" + ("-".join(f"{k}{v}" for k, v in o) or "default") for p, o in KKT_CASES])
def test_generate_kkt(prec, opts, N, Bt, mode):
    """mpcg_generate_kkt under both gradient routes and the three arithmetic builds (15 knots with two knots per lane: ragged), and the double
    entry: the four outputs written whole, the three inputs untouched."""
    xu, goals, xs, _ = windows(prec, N, Bt)
    sol = solver(N, Bt, opts)
    fn = sol.lib.mpcg_generate_kkt if prec == "f32" else sol.lib.mpcg_generate_kkt_f64

    def call(a):
        sol._check(fn(sol._h, plant()._p, m, DT, ptr(a["goals"]), ptr(a["xs"]), ptr(a["xu"]), iiwa.QD_COST, iiwa.r_cost(N),
                      ptr(a["G"]), ptr(a["C"]), ptr(a["g"]), ptr(a["c"]), Bt, stream()))
    arena.both_ways(A.generate_kkt(prec, N, Bt), mode, {"goals": goals, "xs": xs, "xu": xu}, call, f"generate_kkt {prec} {opts} N={N} B={Bt}")


MERIT_BUILDS = [("f32", ()), ("f32", (("merit_f32", 1),)), ("f64", ())]
MERIT_ARGS = [((-0.5,), True, True), ((0.0, -1.0, -0.5), True, True), ((0.0, -1.0, -0.5), False, True), ((0.0,), True, False)]


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("steps,with_xs,with_dz", MERIT_ARGS, ids=["1step", "3steps", "3steps-noxs", "step0-nodz"])
@pytest.mark.parametrize("N,Bt", A.PLANT_NB)
@pytest.mark.parametrize("prec,opts", MERIT_BUILDS, ids=["f32", "merit_f32", "f64"])
def test_compute_merit(prec, opts, N, Bt, steps, with_xs, with_dz, mode):
    """mpcg_compute_merit (float64 inside and packed float) and _f64: 1 and 3 step sizes (15 and 45 items: an odd count leaves half a lane
    group empty), d_xs given and NULL, d_dz NULL at step size 0."""
    xu, goals, xs, dz = windows(prec, N, Bt)
    sol = solver(N, Bt, opts)
    inputs = {"goals": goals, "xu": xu}
    if with_xs:
        inputs["xs"] = xs
    if with_dz:
        inputs["dz"] = dz

    def call(a):
        v = lambda name: a[name].view(Bt, -1) if name in a else None
        sol.compute_merit(plant(), v("goals"), v("xs"), v("xu"), v("dz"), steps, DT, MU, iiwa.QD_COST, iiwa.r_cost(N), merit=v("merit"))
    arena.both_ways(A.compute_merit(prec, N, Bt, len(steps), with_xs, with_dz), mode, inputs, call,
                    f"compute_merit {prec} {opts} N={N} B={Bt} {steps} xs={with_xs} dz={with_dz}")


LS_STEP_SIZES = (-1.0, -0.5, -0.25)


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("rho", [False, True], ids=["step", "step_rho"])
@pytest.mark.parametrize("nn,mm", [(14, 7), (6, 3)])
@pytest.mark.parametrize("prec", PRECS)
def test_line_search_step(prec, nn, mm, rho, mode):
    """mpcg_line_search_step(_f64) and _rho(_f64), N = 3, five trajectories: 0 and 3 take a step; 1 and 4 take none (all merits worse; equal to
    the reference merit and a NaN) — d_xu and d_merit_ref are not written; 2 is frozen under _rho although its merits improve — nothing of it
    but d_step is written — and without rho takes no step.  -1 is a legitimate d_step: a sentinel marks the unwritten."""
    N, Bt = 3, A.LS_B
    dt = A.DT[prec]
    rng = np.random.default_rng([nn, mm])
    L = A.zlen(nn, mm, N)
    merit = np.array([[12, 8, 9], [11, 12, 13], [1, 2, 3] if rho else [11, 12, 13], [5, 7, 6], [10, np.nan, 10]], dt)
    inputs = {"merit": merit, "merit_ref": np.full(Bt, 10, dt), "dz": rng.standard_normal((Bt, L)).astype(dt),
              "xu": rng.standard_normal((Bt, L)).astype(dt), "step": np.full(Bt, -7, np.int32)}
    if rho:
        inputs.update(rho=np.array([1e-3, 0.5, 9.9, 3e-2, 1.7], dt), drho=np.array([1, 1.2, 1.3, 0.9, 1.0], dt),
                      done=np.array([0, 0, 1, 0, 0], np.uint8))
    sol = solver(N, Bt, (), nn, mm)

    def call(a):
        v = lambda name: a[name].view(Bt, -1)
        if rho:
            sol.line_search_step_rho(v("merit"), LS_STEP_SIZES, a["merit_ref"], v("dz"), v("xu"), a["rho"], a["drho"], a["done"], step=a["step"],
                                     control_size=mm)
        else:
            sol.line_search_step(v("merit"), LS_STEP_SIZES, a["merit_ref"], v("dz"), v("xu"), step=a["step"], control_size=mm)
    out = arena.both_ways(A.line_search(prec, nn, mm, N, rho), mode, inputs, call, f"line_search {prec} {nn}x{mm} rho={rho}")
    assert out["step"].tolist() == [1, -1, -2 if rho else -1, 0, -1], out["step"]
    assert out["merit_ref"].tolist() == [8, 10, 10, 5, 10]
    if rho:
        assert out["done"].tolist() == [0, 0, 1, 0, 0]


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("sim_us,with_ee", [(650, True), (650, False), (0, True)], ids=["3substeps+remainder-ee", "3substeps+remainder", "zero-time"])
@pytest.mark.parametrize("N,Bt", A.PLANT_NB)
@pytest.mark.parametrize("prec", PRECS)
def test_simulate(prec, N, Bt, sim_us, with_ee, mode):
    """mpcg_simulate(_f64): 650 us at a substep of 200 us is three full substeps and a remainder; sim_time_us = 0 leaves d_xs bitwise unchanged.
    B = 5 leaves lane groups of the last wavefront without a trajectory: they redo the last one and store nothing."""
    xu, _, xs, _ = windows(prec, N, Bt)
    sol = solver(N, Bt)

    def call(a):
        sol.simulate(plant(), a["xs"].view(Bt, -1), a["xu"].view(Bt, -1), DT, 0.0, float(sim_us), SS, eePos=a["eePos"].view(Bt, 3) if with_ee else None)
    out = arena.both_ways(A.simulate(prec, N, Bt, with_ee), mode, {"xs": xs, "xu": xu}, call, f"simulate {prec} N={N} B={Bt} {sim_us} us ee={with_ee}")
    assert (out["xs"].tobytes() == xs.tobytes()) == (sim_us == 0)


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("per_traj", [False, True], ids=["shared-plan", "plan-per-trajectory"])
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("prec", PRECS)
def test_advance_horizon_shift(prec, N, per_traj, mode):
    """mpcg_advance_horizon(_f64), shift = 1, traj_batch_stride 0 and = traj_steps (xu_fill_lead 0 and N - 1), four trajectories: inside the plan;
    offset + N = traj_steps after the increment (the else branch: the plan's last row, NaN behind it); the plan used up (done becomes 1); frozen
    on entry (nothing of it is written).  The plan arrays are inputs."""
    Bt, T = A.ADV_B, N + 6
    dt = A.DT[prec]
    rng = np.random.default_rng([N, int(per_traj)])
    f = lambda *s: rng.standard_normal(s).astype(dt)
    L = A.zlen(n, m, N)
    rows = Bt if per_traj else 1
    inputs = {"xu": f(Bt, L), "lambda": f(Bt, n * N), "goal": f(Bt, 6 * N), "xs": f(Bt, n), "eePos": f(Bt, 3), "xu_traj": f(rows, T, n + m),
              "goal_traj": f(rows, T, 6), "traj_offset": np.array([0, T - N - 1, T - 1, 2], np.int32), "done": np.array([0, 0, 0, 7], np.int32)}
    sol = solver(N, Bt)

    def call(a):
        v = lambda name: a[name].view(Bt, -1)
        plan = lambda name, w: a[name].view(Bt, T, w) if per_traj else a[name].view(T, w)
        sol.advance_horizon(True, v("xu"), v("xs"), v("lambda"), v("goal"), v("eePos"), plan("xu_traj", n + m), plan("goal_traj", 6), a["traj_offset"],
                            a["done"], a["tracking_error"], xu_fill_lead=N - 1 if per_traj else 0)
    out = arena.both_ways(A.advance_shift(prec, N, T, per_traj), mode, inputs, call, f"advance_horizon shift {prec} N={N} per_traj={per_traj}")
    assert out["traj_offset"].tolist() == [1, T - N, T, 2] and out["done"].tolist() == [0, 0, 1, 7]


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("prec", PRECS)
def test_advance_horizon_without_shift(prec, mode):
    """shift = 0: 14 elements per live trajectory and nothing else; the frozen trajectory keeps every bit."""
    N, Bt = 3, A.ADV_B
    dt = A.DT[prec]
    rng = np.random.default_rng(N)
    xu, xs = rng.standard_normal((Bt, A.zlen(n, m, N))).astype(dt), rng.standard_normal((Bt, n)).astype(dt)
    sol = solver(N, Bt)

    def call(a):
        sol.advance_horizon(False, a["xu"].view(Bt, -1), a["xs"].view(Bt, -1), done=a["done"])
    out = arena.both_ways(A.advance_noshift(prec, N), mode, {"xu": xu, "xs": xs, "done": np.array([0, 0, 0, 7], np.int32)}, call,
                          f"advance_horizon no shift {prec}")
    assert out["xu"].reshape(Bt, -1)[:3, :n].tobytes() == xs[:3].tobytes()


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("with_qd,with_qdd", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("prec", PRECS)
def test_inverse_dynamics(prec, with_qd, with_qdd, mode):
    """mpcg_inverse_dynamics(_f64), count 5 (lane groups without a state behind the last one), d_qd / d_qdd given and NULL."""
    dt = A.DT[prec]
    rng = np.random.default_rng(7)
    inputs = {"q": rng.standard_normal((A.INVDYN_COUNT, 7)).astype(dt)}
    if with_qd:
        inputs["qd"] = rng.standard_normal((A.INVDYN_COUNT, 7)).astype(dt)
    if with_qdd:
        inputs["qdd"] = rng.standard_normal((A.INVDYN_COUNT, 7)).astype(dt)
    sol = solver(3, 5)
    pl = plant().with_gravity((0.0, 0.0, 9.81))            # (the gravity torques are not zero: with both NULL the output is still written numbers)

    def call(a):
        sol.inverse_dynamics(pl, a["q"], a.get("qd"), a.get("qdd"), tau=a["tau"])
    arena.both_ways(A.invdyn(prec, with_qd, with_qdd), mode, inputs, call, f"inverse_dynamics {prec} qd={with_qd} qdd={with_qdd}")
