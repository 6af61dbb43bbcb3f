"""GPU: mpcg_generate_kkt_xuref(_f64) and mpcg_compute_merit_xuref(_f64) inside a guard-banded arena (tests/arena.py, as it is): every array of the
call — the plan and d_traj_offset included — in ONE allocation at its smallest alignment (and at 256 bytes), bands of 0xFF bytes (NaN / -1) around each.
The offsets clamp at both ends of the plan, so a row index that escaped the clamp would read a band and surface as a NaN; no band byte may change, no
input may change, every output element is written, and the outputs are bit for bit those of the same call on separately allocated tensors (which
tests/test_gpu_xuref.py pins to the float64 restatement)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import arena
import arena_specs as A
from mpcgpu_amd import _lib, iiwa

pytestmark = pytest.mark.gpu
n, m, ROW = 14, 7, 21
DT = iiwa.TIMESTEP
MU = 10.0
QD, R, EE, QC = 2.0 ** -6, 2.0 ** -7, 0.75, 0.5
# (N, B) of tests/test_gpu_arena_plant.py -> (traj_steps, plan per trajectory, offsets): (2, 1) a plan of ONE row — knot 1 and the last block's row clamp at
# its end; (3, 5) plans of four rows at a stride of four — offsets below the plan, at its last row, inside, far beyond it, and the extremes an int32 holds
PLANS = {(2, 1): (1, False, (0,)), (3, 5): (4, True, (-3, 3, 1, 9, -2 ** 31))}
PLANS_HIGH = {(2, 1): (1, False, (2 ** 31 - 1,)), (3, 5): (4, True, (2 ** 31 - 1, 2, 0, -1, 4))}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def plant():
    from mpcgpu_amd import Plant
    return Plant()


def solver(N, Bt, opts=()):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=Bt)
    for key, value in opts:
        sol.set_option(key, value)
    return sol


@functools.lru_cache(maxsize=None)
def inputs(prec, N, Bt, high):
    """(xu, goals, xs, dz, plan, offsets) in the entry's type, read-only and shared."""
    T, per_traj, offs = (PLANS_HIGH if high else PLANS)[(N, Bt)]
    xu, goals, xs = iiwa.random_windows(N, Bt, 11 + N)
    rng = np.random.default_rng(2000 + N)
    dz = 0.05 * rng.standard_normal(xu.shape)
    plan = 0.5 * rng.standard_normal(((Bt if per_traj else 1) * T, ROW))
    out = tuple(np.ascontiguousarray(a, A.DT[prec]) for a in (xu, goals.reshape(Bt, -1), xs, dz, plan)) + (np.array(offs, np.int32),)
    for a in out:
        a.flags.writeable = False
    return out


def plan_specs(prec, N, Bt, high):
    T, per_traj, _ = (PLANS_HIGH if high else PLANS)[(N, Bt)]
    rows = (Bt if per_traj else 1) * T
    return [arena.spec("xu_traj", A.DT[prec], rows * ROW, "in", None, ROW, T * ROW), arena.spec("traj_offset", np.int32, Bt, "in", None, 1, 1)]


def xuref(a, N, Bt, high, ee=EE):
    T, per_traj, _ = (PLANS_HIGH if high else PLANS)[(N, Bt)]
    return _lib.mpcg_xuref(a["xu_traj"].data_ptr(), T, T if per_traj else 0, a["traj_offset"].data_ptr(), ee, QC, _lib.MPCG_XUREF_QD_RELATIVE | _lib.MPCG_XUREF_U_RELATIVE)


KKT_CASES = [("f32", opts) for opts in A.KKT_BUILDS] + [("f64", ())]


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("high", [False, True], ids=["offsets-low", "offsets-high"])
@pytest.mark.parametrize("N,Bt", A.PLANT_NB)
@pytest.mark.parametrize("prec,opts", KKT_CASES, ids=[p + "-" + ("-".join(f"{k}{v}" for k, v in o) or "default") for p, o in KKT_CASES])
def test_generate_kkt_xuref(prec, opts, N, Bt, high, mode):
    """Both gradient routes, the three arithmetic builds (the packed one reads two knots' rows; 10 knots at B = 5 and 1 at B = 1) and the double entry: the
    four outputs written whole, the five inputs untouched, nothing read outside them."""
    xu, goals, xs, _, plan, offs = inputs(prec, N, Bt, high)
    sol = solver(N, Bt, opts)
    fn = sol.lib.mpcg_generate_kkt_xuref if prec == "f32" else sol.lib.mpcg_generate_kkt_xuref_f64

    def call(a):
        ref = xuref(a, N, Bt, high)
        sol._check(fn(sol._h, plant()._p, m, DT, ptr(a["goals"]), ptr(a["xs"]), ptr(a["xu"]), QD, R, C.byref(ref), ptr(a["G"]), ptr(a["C"]), ptr(a["g"]), ptr(a["c"]),
                      Bt, stream()))
    arena.both_ways(A.generate_kkt(prec, N, Bt) + plan_specs(prec, N, Bt, high), mode,
                    {"goals": goals, "xs": xs, "xu": xu, "xu_traj": plan, "traj_offset": offs}, call, f"generate_kkt_xuref {prec} {opts} N={N} B={Bt} high={high}")


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("N,Bt", A.PLANT_NB)
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_generate_kkt_xuref_without_goals(prec, N, Bt, mode):
    """ee_cost = 0 and d_eePos_traj = NULL: the goals are not in the arena at all."""
    xu, _, xs, _, plan, offs = inputs(prec, N, Bt, False)
    sol = solver(N, Bt)
    fn = sol.lib.mpcg_generate_kkt_xuref if prec == "f32" else sol.lib.mpcg_generate_kkt_xuref_f64

    def call(a):
        ref = xuref(a, N, Bt, False, 0.0)
        sol._check(fn(sol._h, plant()._p, m, DT, None, ptr(a["xs"]), ptr(a["xu"]), QD, R, C.byref(ref), ptr(a["G"]), ptr(a["C"]), ptr(a["g"]), ptr(a["c"]), Bt, stream()))
    arena.both_ways(A.generate_kkt(prec, N, Bt)[1:] + plan_specs(prec, N, Bt, False), mode, {"xs": xs, "xu": xu, "xu_traj": plan, "traj_offset": offs}, call,
                    f"generate_kkt_xuref no goals {prec} N={N} B={Bt}")


MERIT_BUILDS = [("f32", ()), ("f32", (("merit_f32", 1),)), ("f64", ())]
MERIT_ARGS = [((0.0, -1.0, -0.5), True, True, True), ((-0.5,), False, True, False), ((0.0,), True, False, True)]


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("steps,with_xs,with_dz,with_goals", MERIT_ARGS, ids=["3steps", "1step-noxs-nogoals", "step0-nodz"])
@pytest.mark.parametrize("high", [False, True], ids=["offsets-low", "offsets-high"])
@pytest.mark.parametrize("N,Bt", A.PLANT_NB)
@pytest.mark.parametrize("prec,opts", MERIT_BUILDS, ids=["f32", "merit_f32", "f64"])
def test_compute_merit_xuref(prec, opts, N, Bt, high, steps, with_xs, with_dz, with_goals, mode):
    """Float64 inside, packed float (an odd item count leaves half a lane group empty; a cost-only half reads its row's 21 entries) and the double entry;
    d_xs, d_dz and d_eePos_traj given and NULL."""
    xu, goals, xs, dz, plan, offs = inputs(prec, N, Bt, high)
    sol = solver(N, Bt, opts)
    fn = sol.lib.mpcg_compute_merit_xuref if prec == "f32" else sol.lib.mpcg_compute_merit_xuref_f64
    ct = C.c_float if prec == "f32" else C.c_double
    arr = (ct * len(steps))(*steps)
    ins = {"xu": xu, "xu_traj": plan, "traj_offset": offs}
    if with_goals:
        ins["goals"] = goals
    if with_xs:
        ins["xs"] = xs
    if with_dz:
        ins["dz"] = dz

    def call(a):
        p = lambda name: ptr(a[name]) if name in a else None
        ref = xuref(a, N, Bt, high, EE if with_goals else 0.0)
        sol._check(fn(sol._h, plant()._p, m, DT, p("goals"), p("xs"), p("xu"), p("dz"), arr, len(steps), MU, QD, R, C.byref(ref), p("merit"), Bt, stream()))
    specs = A.compute_merit(prec, N, Bt, len(steps), with_xs, with_dz)
    if not with_goals:
        specs = specs[1:]
    arena.both_ways(specs + plan_specs(prec, N, Bt, high), mode, ins, call, f"compute_merit_xuref {prec} {opts} N={N} B={Bt} high={high} {steps}")
