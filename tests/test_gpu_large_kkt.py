"""GPU: mpcg_generate_kkt(_f64) at the first batch whose C passes 2^32 bytes (3.65 M knots in float at N = 5, 1.83 M in double at N = 3; G is
as large as C at these horizons) under "kkt_f32" = 0 and 1 and both integrators, and mpcg_generate_kkt_xuref_f64 with a limits plant and one
plan per trajectory, so that the plan-row index ((size_t)b * traj_stride + r) * 21 and traj_offset[b] run with b up to 456 k.
tests/large_extents.py: three distinct windows tiled over the batch on the device, every tile of G, C, g and c bit for bit the call on the
three; that call is held to the float64 restatements at the limits of tests/test_gpu_integrator.py (the plain entries, each build's own
tolerance) and tests/test_gpu_limits.py (the _xuref entry with limits)."""
import ctypes as C

import numpy as np
import pytest
import torch

import large_extents as le
import plant_ref as P
import test_gpu_integrator as ti
import test_gpu_limits as tl
from mpcgpu_amd import iiwa
from test_gpu_xuref import COSTS, LIMIT_C, LIMIT_Ggc, case, model

pytestmark = pytest.mark.gpu
DT = iiwa.TIMESTEP


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


PLAIN = [c for c in le.KKT_CASES if not c[3]]
XUREF = [c for c in le.KKT_CASES if c[3]]
ident = lambda c: f"{c[0]}-N{c[1]}-" + "-".join(f"{k}{v}" for k, v in c[2])


@pytest.mark.parametrize("prec,N,opts,xuref", PLAIN, ids=[ident(c) for c in PLAIN])
def test_generate_kkt_with_c_past_2_32(prec, N, opts, xuref):
    spec = le.kkt_spec(prec, N, opts, xuref)
    dtype = le.A.DT[prec]
    o = dict(opts)
    xu, goals, xs, _ = ti.inputs(N, spec.D, dtype)
    sol = ti.solver(N, spec.B, **o)
    costs = ti.costs(N, dtype)

    def call(a, Bt):
        fn = sol.lib.mpcg_generate_kkt if prec == "f32" else sol.lib.mpcg_generate_kkt_f64
        sol._check(fn(sol._h, ti.plant("iiwa")._p, 7, float(DT), ptr(a["goals"]), ptr(a["xs"]), ptr(a["xu"]), float(costs[0]), float(costs[1]),
                      ptr(a["G"]), ptr(a["C"]), ptr(a["g"]), ptr(a["c"]), Bt, stream()))
    out = le.run(spec, {"goals": goals, "xs": xs, "xu": xu}, call)
    sol.close()
    build = "f64" if prec == "f64" else "kkt_f32=1" if o.get("kkt_f32") == 1 else "default"
    _, _, tol, tol_C = ti.KKT_BUILDS[build]
    want = ti.kkt_restated("iiwa", N, spec.D, dtype, o.get("integrator", 0))
    for d in range(spec.D):
        for name, w in zip(("G", "C", "g", "c"), want[d]):
            err = ti.rel_block(out[name][d], w)
            print(f"{spec.label} trajectory {d} {name}: {err:.2e}")
            assert err <= (tol_C if name == "C" else tol), (spec.label, d, name, err)


@pytest.mark.parametrize("prec,N,opts,xuref", XUREF, ids=[ident(c) for c in XUREF])
def test_generate_kkt_xuref_with_limits_and_a_plan_per_trajectory(prec, N, opts, xuref):
    from mpcgpu_amd import XuRef
    assert prec == "f64" and N == 5
    spec = le.kkt_spec(prec, N, opts, xuref)
    integrator = dict(opts).get("integrator", 0)
    cs, co, lim = case(N, spec.D, True), COSTS["all"], tl.kkt_limits(N, spec.D, True)
    assert cs.stride == N + 3 and cs.stride * 21 == spec.arrays[3].traj
    pl = tl.kkt_plant(N, spec.D, True)
    sol = tl.solver(N, spec.B, (), integrator)
    plan = cs.plan.reshape(spec.D, cs.stride * 21)

    def call(a, Bt):
        ref = XuRef(a["xu_traj"].view(-1, 21), a["traj_offset"].view(-1), cs.stride, co.ee_cost, co.q_cost, bool(co.flags & P.QD_RELATIVE), bool(co.flags & P.U_RELATIVE),
                    traj_steps=cs.T)
        x = sol._xuref("generate_kkt_xuref", ref, torch.float64, Bt, 14, 7)          # (the C entry itself: the wrapper would allocate the outputs)
        sol._check(sol.lib.mpcg_generate_kkt_xuref_f64(sol._h, pl._p, 7, float(DT), ptr(a["goals"]), ptr(a["xs"]), ptr(a["xu"]), float(co.qd_cost), float(co.r_cost),
                                                       C.byref(x), ptr(a["G"]), ptr(a["C"]), ptr(a["g"]), ptr(a["c"]), Bt, stream()))
    out = le.run(spec, {"goals": cs.goals, "xs": cs.xs, "xu": cs.xu, "xu_traj": plan, "traj_offset": cs.offsets.reshape(spec.D, 1)}, call)
    sol.close()
    worst = {"Ggc": 0.0, "C": 0.0}
    for b in range(spec.D):
        want = P.generate_kkt(model(), cs.xu[b], cs.goals[b], cs.xs[b], N, rows=cs.rows(b), cost=co, limits=lim, dt=DT, integrator=integrator, base=cs.dynamics(b, integrator))
        for name, w in zip(("G", "C", "g", "c"), want):
            key = "C" if name == "C" else "Ggc"
            worst[key] = max(worst[key], np.abs(out[name][b] - w).max() / max(1.0, np.abs(w).max()))
    print(f"{spec.label}: worst G,g,c {worst['Ggc']:.3e}  C {worst['C']:.3e}")
    assert worst["Ggc"] <= LIMIT_Ggc and worst["C"] <= LIMIT_C, worst
