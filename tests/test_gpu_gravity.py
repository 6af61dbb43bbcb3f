"""GPU: gravity as immutable model data of the plant (mpcg_plant_clone_gravity, include/mpcg.h GRAVITY) in every build of the KKT, merit and simulate
kernels, and the batched inverse dynamics mpcg_inverse_dynamics(_f64) — against the float64 restatements run on tests/gravity_ref.py's models
(pinned on the CPU in tests/test_gravity_ref_cpu.py, which also shows that a negated vector or swapped axes move C and c by more than 1e-3: a thousand
times the limits here).

Plants: the random chains of chain_models.SEEDS cloned with gravity_ref.G_CHAIN = (1.7, -2.9, 9.2), the built-in iiwa cloned with (0, 0, 9.81).
Inputs: chain_models.hard_inputs, both sets; shapes chain_models.SHAPES.  Every tolerance is the one the same entry and build already has without
gravity, by value, measured as there (KKT arrays: of max(1, |block|) per trajectory; merits, states and torques: of max(1, |value|))."""
import ctypes as C
import functools
import json
import subprocess

import numpy as np
import pytest
import torch

import chain_models as cm
import gravity_ref as gr
import plant_ref as P
from mpcgpu_amd import _lib, iiwa

pytestmark = pytest.mark.gpu
n, m, NJ = cm.n, cm.m, cm.NJ
f32, f64 = np.float32, np.float64
NAN = float("nan")
DT = iiwa.TIMESTEP
MU = 10.0
STEPS3 = [0.0, -1.0, -0.5]
SHAPES = list(cm.SHAPES)
SIZES = ("large", "modest")
WHICH = list(cm.SEEDS) + ["iiwa"]
N4 = 4

TOL_KKT = 1e-6                           # tests/test_gpu_integrator.py:31 (analytic)
TOL_KKT_DIFFERENCE = 3e-6                # :32 ("kkt_analytic" = 0)
TOL_KKT_F32 = 1e-5                       # :33 ("kkt_f32" = 1 and 2)
LIMIT_Ggc = 8.8e-11                      # tests/test_gpu_kkt_f64.py::LIMIT_Ggc
LIMIT_C = 8.9e-7                         # tests/test_gpu_kkt_f64.py::LIMIT_C (the float link-force records of the analytic route: gravity does not change them)
LIMIT_Gg = cm.KKT_F64_LIMIT_Gg           # G and g of the _f64 entry at |ee - goal| ~ 1: the cost does not see gravity
TOL_MERIT, TOL_MERIT_F32, LIMIT_MERIT_F64 = 1e-6, 1e-5, 1.2e-13
TOL_SIM, LIMIT_SIM = 1e-6, 5.7e-15
TOL_ID, LIMIT_ID = 1e-6, 8.8e-11
# (options, dtype, tolerance of G and g, of c, of C)
KKT_BUILDS = {"default": ({}, f32, TOL_KKT, TOL_KKT, TOL_KKT), "difference": ({"kkt_analytic": 0}, f32, TOL_KKT_DIFFERENCE, TOL_KKT_DIFFERENCE, TOL_KKT_DIFFERENCE),
              "kkt_f32=1": ({"kkt_f32": 1}, f32, TOL_KKT_F32, TOL_KKT_F32, TOL_KKT_F32), "kkt_f32=2": ({"kkt_f32": 2}, f32, TOL_KKT_F32, TOL_KKT_F32, TOL_KKT_F32),
              "f64": ({}, f64, LIMIT_Gg, LIMIT_Ggc, LIMIT_C)}
ALL_KKT = dict(KKT_BUILDS, **{"f64 difference": ({"kkt_analytic": 0}, f64, None, None, None)})
MERIT_BUILDS = {"default": ({}, f32, TOL_MERIT), "merit_f32": ({"merit_f32": 1}, f32, TOL_MERIT_F32), "f64": ({}, f64, LIMIT_MERIT_F64)}


def dev(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def tdt(dtype):
    return torch.float32 if dtype == f32 else torch.float64


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rel_block(got, want):
    return float(np.abs(np.asarray(got, f64) - want).max() / max(1.0, np.abs(want).max()))


def rel(got, want):
    want = np.asarray(want, f64)
    return float((np.abs(np.asarray(got, f64) - want) / np.maximum(1.0, np.abs(want))).max())


def fig(*a):
    print("GRAVITY-FIG", *a)


# ---- plants, models, inputs and restatements: built once, never written to ----
@functools.lru_cache(maxsize=None)
def model(which):
    return gr.chain(which)


@functools.lru_cache(maxsize=None)
def plain_plant(which):
    from mpcgpu_amd import Plant
    return Plant() if which == "iiwa" else Plant(cm.tables(cm.random_chain(which)))


@functools.lru_cache(maxsize=None)
def plant(which):
    return plain_plant(which).with_gravity(gr.G_IIWA if which == "iiwa" else gr.G_CHAIN)


def input_seed(which):
    return 0 if which == "iiwa" else cm.input_seed(which)


@functools.lru_cache(maxsize=None)
def inputs(which, N, B, size, dtype):
    """(xu, goals [B, 6N], xs, dz): float32, or (dtype = f64) genuinely double xu, xs, dz — the float32 values times (1 + 1e-12 r) — with goals and (for the
    merit) an x_s that stay float-representable."""
    xu, goals, xs = (np.ascontiguousarray(a, f32) for a in cm.hard_inputs(N, B, input_seed(which), size))
    rng = np.random.default_rng([9, N, input_seed(which)])
    dz = (0.05 * rng.standard_normal(xu.shape)).astype(f32)
    goals = goals.reshape(B, -1)
    if dtype == f32:
        return xu, goals, xs, dz
    wide = lambda a: a.astype(f64) * (1.0 + 1e-12 * rng.uniform(-1, 1, a.shape))
    out = wide(xu), goals.astype(f64), wide(xs), wide(dz)
    assert all((a != a.astype(f32)).mean() > 0.9 for a in (out[0], out[2], out[3]))
    return out


@functools.lru_cache(maxsize=None)
def kkt_restated(which, N, B, size, dtype, integrator):
    xu, goals, xs, _ = (np.asarray(a, f64) for a in inputs(which, N, B, size, dtype))
    return [P.generate_kkt(model(which), xu[b], goals[b].reshape(N, 6), xs[b], N, dt=DT, integrator=integrator) for b in range(B)]


@functools.lru_cache(maxsize=None)
def merits_restated(which, N, B, size, dtype, with_xs, mu=MU):
    xu, goals, xs, dz = inputs(which, N, B, size, dtype)
    return P.merits(model(which), xu, dz, STEPS3, goals.reshape(B, N, 6), xs.astype(f32) if with_xs else None, N, mu, cost=P.Cost.plain(iiwa.QD_COST, iiwa.r_cost(N)),
                    dt=DT, integrator=0, double=dtype == f64)


def solver(N, B, **options):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=B)
    for key, v in options.items():
        sol.set_option(key, v)
        assert sol.get_option(key) == v
    return sol


def costs(N, dtype):
    return (float(f32(iiwa.QD_COST)), float(f32(iiwa.r_cost(N)))) if dtype == f32 else (iiwa.QD_COST, iiwa.r_cost(N))


def run_kkt(pl, N, arrs, dtype, **options):
    """One generate_kkt call on a fresh handle -> [G, C, g, c] as numpy; the device outputs are left NaN-filled for the next call's allocations."""
    xu, goals, xs = (dev(a, dtype) for a in arrs[:3])
    out = solver(N, len(arrs[0]), **options).generate_kkt(pl, goals, xs, xu, DT, *costs(N, dtype))
    torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in out]
    for t in out:
        t.fill_(NAN)
    torch.cuda.synchronize()
    assert all(a.dtype == dtype and np.isfinite(a).all() for a in res), (N, options)
    return res


def kkt_args(which, N, B, size, dtype):
    xu, goals, xs, _ = inputs(which, N, B, size, dtype)
    return xu, goals, xs


def run_merit(pl, N, goals, xs, xu, dz, dtype, steps=STEPS3, mu=MU, **options):
    B = len(xu)
    out = torch.full((B, len(steps)), NAN, dtype=tdt(dtype), device="cuda")
    solver(N, B, **options).compute_merit(pl, dev(goals, dtype), None if xs is None else dev(xs, dtype), dev(xu, dtype), None if dz is None else dev(dz, dtype),
                                          steps, DT, mu, iiwa.QD_COST, iiwa.r_cost(N), merit=out)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.isfinite(res).all(), (N, options)
    return res


def run_simulate(pl, N, xs, xu, dtype, toff, sim, ss, **options):
    """One simulate call on a fresh handle -> (new state [B, n], end-effector position [B, 3]) as numpy."""
    B = len(xu)
    d_xs = dev(np.array(xs, copy=True), dtype)
    ee = torch.full((B, 3), NAN, dtype=d_xs.dtype, device="cuda")
    solver(N, B, **options).simulate(pl, d_xs, dev(xu, dtype), DT, toff, sim, ss, eePos=ee)
    torch.cuda.synchronize()
    return d_xs.cpu().numpy(), ee.cpu().numpy()


def worst_per_array(got, want):
    return [max(rel_block(got[i][b], want[b][i]) for b in range(len(want))) for i in range(4)]


# ---- 1. the ABI ----
def test_abi_of_the_clone():
    """mpcg_plant_clone_gravity round-trips through mpcg_plant_get_gravity ({0, 0, 0} for a created plant; -0 reads back as +0), rejects NULL and non-finite
    input with MPCG_ERR_INVALID and *out = NULL, and source and clone are destroyed in either order — the survivor still computes."""
    lib = _lib.load()
    INV, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_OK
    vec = lambda *v: (C.c_double * 3)(*v)
    src = C.c_void_p()
    assert lib.mpcg_plant_create_iiwa14(C.byref(src), -1) == OK
    out3 = vec(NAN, NAN, NAN)
    assert lib.mpcg_plant_get_gravity(src, out3) == OK and tuple(out3) == (0.0, 0.0, 0.0)
    a, b = C.c_void_p(), C.c_void_p()
    assert lib.mpcg_plant_clone_gravity(C.byref(a), src, vec(1.7, -2.9, 9.2)) == OK and a.value and a.value != src.value
    assert lib.mpcg_plant_get_gravity(a, out3) == OK and tuple(out3) == (1.7, -2.9, 9.2)
    assert lib.mpcg_plant_get_gravity(src, out3) == OK and tuple(out3) == (0.0, 0.0, 0.0)                 # the source is not touched
    assert lib.mpcg_plant_clone_gravity(C.byref(b), a, vec(-0.0, 0.0, -9.81)) == OK                         # a clone of a clone
    assert lib.mpcg_plant_get_gravity(b, out3) == OK and tuple(out3) == (0.0, 0.0, -9.81) and np.signbit(out3[0]) == False
    bad = C.c_void_p(12345)
    assert lib.mpcg_plant_clone_gravity(None, src, vec(0, 0, 1)) == INV
    assert lib.mpcg_plant_clone_gravity(C.byref(bad), None, vec(0, 0, 1)) == INV and not bad.value
    bad = C.c_void_p(12345)
    assert lib.mpcg_plant_clone_gravity(C.byref(bad), src, None) == INV and not bad.value
    for v in ((NAN, 0, 0), (0, float("inf"), 0), (0, 0, -float("inf"))):
        bad = C.c_void_p(12345)
        assert lib.mpcg_plant_clone_gravity(C.byref(bad), src, vec(*v)) == INV and not bad.value
    assert lib.mpcg_plant_get_gravity(None, out3) == INV and lib.mpcg_plant_get_gravity(src, None) == INV
    # either order: the source first, then its clone's clone; the survivors still give their own torques
    sol = solver(4, 2)
    q = dev(np.array([gr.Q_PRINTED], f64), f64)
    tau = lambda p: (torch.cuda.synchronize(), _id(lib, sol, p, q))[1]
    want = model("iiwa").gravity_torques(np.array(gr.Q_PRINTED))
    assert lib.mpcg_plant_destroy(src) == OK
    assert rel(tau(b), -want) <= LIMIT_ID
    assert lib.mpcg_plant_destroy(b) == OK
    c = C.c_void_p()
    assert lib.mpcg_plant_clone_gravity(C.byref(c), a, vec(0, 0, 9.81)) == OK
    assert lib.mpcg_plant_destroy(a) == OK                                                                   # the clone first, then ITS clone
    assert rel(tau(c), want) <= LIMIT_ID
    assert np.abs(tau(c) - np.array(gr.TAU_PRINTED)).max() <= 5.1e-4
    assert lib.mpcg_plant_destroy(c) == OK


def _id(lib, sol, p, q):
    out = torch.full((q.shape[0], NJ), NAN, dtype=torch.float64, device="cuda")
    assert lib.mpcg_inverse_dynamics_f64(sol._h, p, q.data_ptr(), None, None, out.data_ptr(), q.shape[0], None) == _lib.MPCG_OK
    torch.cuda.synchronize()
    return out.cpu().numpy()[0]


@pytest.mark.parametrize("dtype", [f32, f64])
def test_abi_of_inverse_dynamics(dtype):
    """The documented errors: NULL handle, plant, d_q or d_tau and count > max_batch x knot_points give MPCG_ERR_INVALID, a handle of another state size
    MPCG_ERR_UNSUPPORTED, count == 0 MPCG_OK with nothing written; d_qd and d_qdd may be NULL.  (A plant on another device needs a second device:
    not run here.)  The Python mirror returns the dtype of q and refuses mixed dtypes."""
    from mpcgpu_amd import PcgSolver
    lib = _lib.load()
    fn = lib.mpcg_inverse_dynamics if dtype == f32 else lib.mpcg_inverse_dynamics_f64
    INV, OK, UNS = _lib.MPCG_ERR_INVALID, _lib.MPCG_OK, _lib.MPCG_ERR_UNSUPPORTED
    sol, pl = solver(4, 2), plant("iiwa")
    q = dev(np.tile(np.array(gr.Q_PRINTED), (9, 1)), dtype)
    tau = torch.full((9, NJ), NAN, dtype=q.dtype, device="cuda")
    qp, tp = q.data_ptr(), tau.data_ptr()
    assert fn(None, pl._p, qp, None, None, tp, 8, None) == INV
    assert fn(sol._h, None, qp, None, None, tp, 8, None) == INV
    assert fn(sol._h, pl._p, None, None, None, tp, 8, None) == INV and b"mpcg_inverse_dynamics" in lib.mpcg_last_error(sol._h)
    assert fn(sol._h, pl._p, qp, None, None, None, 8, None) == INV
    assert fn(sol._h, pl._p, qp, None, None, tp, 9, None) == INV and b"max_batch" in lib.mpcg_last_error(sol._h)          # 9 > 2 x 4
    assert fn(sol._h, pl._p, qp, None, None, tp, 0, None) == OK
    other = PcgSolver(4, max_batch=2, state_size=6, control_size=3)
    assert fn(other._h, pl._p, qp, None, None, tp, 8, None) == UNS
    torch.cuda.synchronize()
    assert torch.isnan(tau).all()                                                                             # nothing was written by any of these
    assert fn(sol._h, pl._p, qp, None, None, tp, 8, None) == OK
    torch.cuda.synchronize()
    got = tau.cpu().numpy()
    assert np.isfinite(got[:8]).all() and np.isnan(got[8]).all()
    out = sol.inverse_dynamics(pl, q[:8])
    assert out.dtype == q.dtype and out.shape == (8, NJ) and same(out, tau[:8])
    with pytest.raises(TypeError):
        sol.inverse_dynamics(pl, q[:8], qd=q[:8].to(torch.float64 if dtype == f32 else torch.float32))
    assert plant("iiwa").gravity == gr.G_IIWA and plain_plant("iiwa").gravity == (0.0, 0.0, 0.0) and plant(1).gravity == gr.G_CHAIN


def test_python_plant_takes_gravity():
    from mpcgpu_amd import Plant
    a = Plant(gravity=(0, 0, 9.81))
    b = Plant(cm.tables(cm.random_chain(1)), gravity=gr.G_CHAIN)
    assert a.gravity == gr.G_IIWA and b.gravity == gr.G_CHAIN
    sol = solver(4, 2)
    q = dev(np.array([gr.Q_PRINTED], f64), f64)
    assert same(sol.inverse_dynamics(a, q), sol.inverse_dynamics(plant("iiwa"), q)) and same(sol.inverse_dynamics(b, q), sol.inverse_dynamics(plant(1), q))
    with pytest.raises(ValueError):
        Plant(gravity=(0, 9.81))
    with pytest.raises(_lib.MpcgError):
        a.with_gravity((0, NAN, 0))


# ---- 2. a zero-gravity clone is the source plant ----
@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("which", [1, "iiwa"])
def test_a_zero_gravity_clone_is_the_source_plant(which, N, B):
    """Every entry, every build: byte-equal outputs."""
    src = plain_plant(which)
    zero = src.with_gravity((0.0, -0.0, 0.0))
    for name, (opts, dtype, *_) in ALL_KKT.items():
        arrs = kkt_args(which, N, B, "large", dtype)
        for x, y, arr in zip(run_kkt(zero, N, arrs, dtype, **opts), run_kkt(src, N, arrs, dtype, **opts), "GCgc"):
            assert same(x, y), (name, arr)
    for name, (opts, dtype, _) in MERIT_BUILDS.items():
        xu, goals, xs, dz = inputs(which, N, B, "large", dtype)
        for sx in (xs.astype(f32), None):
            assert same(run_merit(zero, N, goals, sx, xu, dz, dtype, **opts), run_merit(src, N, goals, sx, xu, dz, dtype, **opts)), name
    for dtype in (f32, f64):
        xu, _, xs, _ = inputs(which, N, B, "large", dtype)
        for si in (0, 1):
            for x, y in zip(run_simulate(zero, N, xs, xu, dtype, 0, 2100, 2e-4, sim_integrator=si), run_simulate(src, N, xs, xu, dtype, 0, 2100, 2e-4, sim_integrator=si)):
                assert same(x, y), (dtype, si)
    sol = solver(N, B)
    q = dev(inputs(which, N, B, "large", f64)[2][:, :NJ], f64)
    assert same(sol.inverse_dynamics(zero, q, q, q), sol.inverse_dynamics(src, q, q, q))


# ---- 3. mpcg_generate_kkt(_f64) against the restatement ----
@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("which", WHICH)
def test_kkt_vs_restatement(which, N, B):
    """Both integrators, both sets, the five builds.  The difference route ("kkt_analytic" = 0) is held to its 3e-6 on the modest set, as
    tests/test_gpu_chain_plants.py holds it: on the large set its quotient amplifies ID(FD(u)) - u with |u| and the assertion is test 4's, over the set."""
    for integrator in (0, 1):
        for size in SIZES:
            for name, (opts, dtype, tol_Gg, tol_c, tol_C) in KKT_BUILDS.items():
                got = run_kkt(plant(which), N, kkt_args(which, N, B, size, dtype), dtype, integrator=integrator, **opts)
                err = worst_per_array(got, kkt_restated(which, N, B, size, dtype, integrator))
                fig(f"kkt {which} N {N} B {B} {size} integrator {integrator} {name}: G C g c", " ".join(f"{e:.2e}" for e in err))
                if name == "difference" and size == "large":
                    continue
                assert err[0] <= tol_Gg and err[2] <= tol_Gg and err[3] <= tol_c and err[1] <= tol_C, (name, size, integrator, err)
    # gravity is really on: the plain plant's c is far from the restatement with gravity
    off = worst_per_array(run_kkt(plain_plant(which), N, kkt_args(which, N, B, "large", f32), f32), kkt_restated(which, N, B, "large", f32, 0))
    assert off[1] > 1e-3 and off[3] > 1e-3, off


# ---- 4. the two gradient routes agree with gravity on ----
def test_the_two_gradient_routes_agree():
    """Analytic against "kkt_analytic" = 0 within the sum of their tolerances on the modest set, every array; and worst[analytic] <= worst[difference] + 1e-9 on
    C with each worst taken over the whole large set (every plant, shape and trajectory), as
    tests/test_gpu_chain_plants.py::test_analytic_gradient_is_never_worse_than_the_difference_quotient_on_the_large_set takes it."""
    worst = {1: 0.0, 0: 0.0}
    for which in WHICH:
        for N, B in SHAPES:
            arrs = kkt_args(which, N, B, "modest", f32)
            ana, dif = run_kkt(plant(which), N, arrs, f32), run_kkt(plant(which), N, arrs, f32, kkt_analytic=0)
            gap = [max(rel_block(ana[i][b], dif[i][b].astype(f64)) for b in range(B)) for i in range(4)]
            assert max(gap) <= TOL_KKT + TOL_KKT_DIFFERENCE, (which, N, gap)
            arrs, want = kkt_args(which, N, B, "large", f32), kkt_restated(which, N, B, "large", f32, 0)
            for analytic in (1, 0):
                worst[analytic] = max(worst[analytic], worst_per_array(run_kkt(plant(which), N, arrs, f32, kkt_analytic=analytic), want)[1])
    fig(f"kkt large set with gravity, C: analytic {worst[1]:.2e} difference {worst[0]:.2e}")
    assert worst[1] <= TOL_KKT, worst
    assert worst[1] <= worst[0] + 1e-9, worst


# ---- 5. the packed build ----
@pytest.mark.parametrize("which", WHICH)
def test_packed_float_bits_do_not_depend_on_the_batch(which):
    """"kkt_f32" = 1 with gravity: trajectory 0 alone against inside the batch of five (the record sharing of the packed analytic round rests on a column's
    link forces being zero below its own joint, which gravity leaves true: it enters the nominal lane only)."""
    N, B = 3, 5
    arrs = kkt_args(which, N, B, "large", f32)
    full = run_kkt(plant(which), N, arrs, f32, kkt_f32=1)
    one = run_kkt(plant(which), N, tuple(a[:1] for a in arrs), f32, kkt_f32=1)
    for x, y, arr in zip(full, one, "GCgc"):
        assert same(x[0], y[0]), arr


# ---- 6. mpcg_compute_merit(_f64) ----
@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("which", WHICH)
def test_merit_vs_restatement(which, N, B):
    """Step sizes 0, -1, -1/2, d_xs given and NULL, both sets: default 1e-6, "merit_f32" 1e-5, _f64 1.2e-13 of max(1, |merit|)."""
    worst = {k: 0.0 for k in MERIT_BUILDS}
    for size in SIZES:
        for name, (opts, dtype, tol) in MERIT_BUILDS.items():
            xu, goals, xs, dz = inputs(which, N, B, size, dtype)
            for with_xs in (True, False):
                got = run_merit(plant(which), N, goals, xs.astype(f32) if with_xs else None, xu, dz, dtype, **opts)
                worst[name] = max(worst[name], rel(got, merits_restated(which, N, B, size, dtype, with_xs)))
    fig(f"merit {which} N {N} B {B}:", " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, (_, _, tol) in MERIT_BUILDS.items():
        assert worst[name] <= tol, worst
    xu, goals, xs, dz = inputs(which, N, B, "large", f32)
    assert rel(run_merit(plain_plant(which), N, goals, xs, xu, dz, f32), merits_restated(which, N, B, "large", f32, True)) > 1e-3      # gravity is really on


@pytest.mark.parametrize("which", WHICH)
def test_kkt_and_merit_measure_the_same_defect(which):
    """The _f64 entries on one gravity clone, step size 0, d_xs given: merit(mu + 1) - merit(mu) is the 1-norm of the d_c mpcg_generate_kkt_f64 stores, within
    tests/test_gpu_merit_f64.py's limit of max(1, merit(mu + 1)) (tests/test_gpu_integrator.py::test_kkt_and_merit_are_the_same_map); with the plain plant
    for one of the two calls the gap exceeds 100 x that."""
    N, B = SHAPES[2]
    xu, goals, xs, _ = inputs(which, N, B, "modest", f64)

    def viol(pl):
        m2, m1 = (run_merit(pl, N, goals, xs, xu, None, f64, steps=[0.0], mu=mu)[:, 0] for mu in (2.0, 1.0))
        return m2 - m1, m2

    defect = lambda pl: np.abs(run_kkt(pl, N, (xu, goals, xs), f64)[3]).sum(axis=1)
    (v, m2), c, c_plain = viol(plant(which)), defect(plant(which)), defect(plain_plant(which))
    gap, cross = np.abs(v - c) / np.maximum(1.0, m2), np.abs(v - c_plain) / np.maximum(1.0, m2)
    fig(f"same defect {which}: |c|_1 {c.tolist()}, gap {gap.max():.2e}, against the plain plant's c at least {cross.min():.2e}")
    assert gap.max() <= LIMIT_MERIT_F64, gap
    assert cross.min() > 100 * LIMIT_MERIT_F64, cross


def test_accepted_merit_is_the_merit_of_the_new_iterate():
    """compute_merit -> line_search_step -> compute_merit with step 0 on the new xu equals the new d_merit_ref bit for bit, on a gravity clone
    (tests/test_gpu_chain_plants.py's test of that name)."""
    which, (N, B) = 1, SHAPES[2]
    xu, goals, xs, dz = inputs(which, N, B, "modest", f32)
    sol = solver(N, B)
    d_xu, d_dz = dev(xu), dev(dz)
    args, tail = (plant(which), dev(goals), dev(xs)), (DT, MU, iiwa.QD_COST, iiwa.r_cost(N))
    steps = STEPS3[1:]
    mer = sol.compute_merit(*args, d_xu, d_dz, steps, *tail)
    ref = torch.full((B,), float("inf"), device="cuda")
    step = sol.line_search_step(mer, steps, ref, d_dz, d_xu)
    again = sol.compute_merit(*args, d_xu, None, [0.0], *tail)
    torch.cuda.synchronize()
    assert (step.cpu().numpy() >= 0).all() and np.isfinite(again.cpu().numpy()).all()
    assert np.array_equal(bits(again)[:, 0], bits(ref))
    assert np.array_equal(ref.cpu().numpy(), mer.cpu().numpy().min(axis=1))


# ---- 7. mpcg_simulate(_f64) ----
@pytest.mark.parametrize("dtype", [f32, f64])
@pytest.mark.parametrize("toff,sim", [(0, 2000), (15000, 2100)])
@pytest.mark.parametrize("which", WHICH)
def test_simulate_vs_restatement(which, toff, sim, dtype):
    """Ten substeps under one control; a knot crossing and a non-zero remainder; both "sim_integrator" values.  State within 1e-6 (float) / 5.7e-15 (double) of
    max(1, |x|); d_eePos as tests/test_gpu_chain_plants.py::test_simulate_vs_host_restatement holds it: against the kinematics of the restated state within
    2e-5 and of the returned state within 1e-6 (float), in double both within LIMIT_Ggc."""
    xu, _, xs, _ = inputs(which, N4, 1, "large", dtype)
    ss = f32(2e-4) if dtype == f32 else float(f32(2e-4))
    for si in (0, 1):
        got, ee = run_simulate(plant(which), N4, xs, xu, dtype, toff, sim, float(ss), sim_integrator=si)
        want = P.simulate(model(which), xs[0], xu[0], N4, DT, toff, sim, ss, si, double=dtype == f64)
        assert got.dtype == dtype and np.isfinite(got).all() and np.isfinite(ee).all()
        err = rel(got[0], want)
        ee_want, ee_got = np.abs(ee[0] - model(which).ee_pos(want[:7])).max(), np.abs(ee[0] - model(which).ee_pos(got[0, :7].astype(f64))).max()
        plain = run_simulate(plain_plant(which), N4, xs, xu, dtype, toff, sim, float(ss), sim_integrator=si)[0]
        fig(f"simulate {which} {np.dtype(dtype).name} toff {toff} sim {sim} sim_integrator {si}: state {err:.2e} eePos {ee_want:.2e} / {ee_got:.2e}; "
            f"plain plant off by {np.abs(plain - got).max():.1e}")
        assert np.abs(got - xs).max() > 1e-4 and np.abs(plain - got).max() > 1e-4                                  # it moved, and gravity moved it
        assert err <= (TOL_SIM if dtype == f32 else LIMIT_SIM), err
        if dtype == f32:
            assert ee_want <= 2e-5 and ee_got <= 1e-6, (ee_want, ee_got)
        else:
            assert ee_want <= LIMIT_Ggc and ee_got <= LIMIT_Ggc, (ee_want, ee_got)


# ---- 8. static equilibrium ----
@pytest.mark.parametrize("which", WHICH)
def test_static_equilibrium(which):
    """qd = 0 and u = mpcg_inverse_dynamics_f64(q), batch 5, one update of 2,000 us in double: every |qd| <= 1e-9 and q has moved by at most 1e-9 (u - c is
    the rounding of torques below 100 Nm, 1e-14; times Minv <= 1e3, times 2e-3 s: 2e-14 — four decades of room).  The un-cloned plant under the same u
    takes off: some |qd| > 1e-3."""
    B = 5
    q = inputs(which, 2, B, "large", f64)[2][:, :NJ]
    sol = solver(N4, B)
    u = sol.inverse_dynamics(plant(which), dev(q, f64)).cpu().numpy()
    xs = np.concatenate([q, np.zeros_like(q)], axis=1)
    xu = np.tile(np.concatenate([xs, u], axis=1), (1, N4))[:, :(n + m) * N4 - m]
    held, _ = run_simulate(plant(which), N4, xs, xu, f64, 0, 2000, 2e-4)
    loose, _ = run_simulate(plain_plant(which), N4, xs, xu, f64, 0, 2000, 2e-4)
    fig(f"equilibrium {which}: |u| up to {np.abs(u).max():.1f} Nm, held |qd| {np.abs(held[:, NJ:]).max():.1e} |dq| {np.abs(held[:, :NJ] - q).max():.1e}; "
        f"plain plant |qd| {np.abs(loose[:, NJ:]).max():.1e}")
    assert np.abs(u).max() > 5.0
    assert np.abs(held[:, NJ:]).max() <= 1e-9 and np.abs(held[:, :NJ] - q).max() <= 1e-9
    assert np.abs(loose[:, NJ:]).max() > 1e-3


# ---- 9. mpcg_inverse_dynamics(_f64) ----
@pytest.mark.parametrize("dtype", [f32, f64])
@pytest.mark.parametrize("count", [1, 5, 67])
@pytest.mark.parametrize("which", WHICH)
def test_inverse_dynamics_vs_restatement(which, count, dtype):
    """One group, a ragged wavefront, more than one wavefront: full (q, qd, qdd), qdd NULL, both NULL against gravity_ref's rnea on the values the entry
    reads.  Float 1e-6, double 8.8e-11 of max(1, |tau|).  With both NULL on the un-cloned plant the result is exactly zero."""
    st = cm.states(count, 300 + input_seed(which))
    wide = (lambda a: np.asarray(a, f32).astype(f64)) if dtype == f32 else (lambda a: np.asarray(a, f64) * (1.0 + 1e-12 * np.cos(np.arange(a.size).reshape(a.shape))))
    q, qd, qdd = (wide(np.array([s[i] for s in st])) for i in range(3))
    sol = solver(8, 9)                                                   # count <= 72
    z = np.zeros(NJ)
    mdl = model(which)
    tol = TOL_ID if dtype == f32 else LIMIT_ID
    for name, a_qd, a_qdd in (("full", qd, qdd), ("qdd NULL", qd, None), ("both NULL", None, None)):
        out = torch.full((count + 1, NJ), NAN, dtype=tdt(dtype), device="cuda")
        sol.inverse_dynamics(plant(which), dev(q, dtype), None if a_qd is None else dev(a_qd, dtype), None if a_qdd is None else dev(a_qdd, dtype), tau=out[:count])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        want = np.array([mdl.rnea(q[i], z if a_qd is None else a_qd[i], z if a_qdd is None else a_qdd[i]) for i in range(count)])
        err = rel(got[:count], want)
        fig(f"inverse dynamics {which} count {count} {np.dtype(dtype).name} {name}: |tau| up to {np.abs(want).max():.1f}, worst {err:.2e}")
        assert got.dtype == dtype and np.isnan(got[count]).all()                                               # (nothing behind the last state is written)
        assert err <= tol, (name, err)
    none = sol.inverse_dynamics(plain_plant(which), dev(q, dtype)).cpu().numpy()
    assert (none == 0).all()


# ---- 10. the reference's own trajectory stays a solution once compensated ----
def test_the_reference_trajectory_stays_a_solution_once_compensated():
    """A window of the reference's trajectory (plant_ref.reference_window(2, 16)), the iiwa with (0, 0, 9.81), in double: u' = u + mpcg_inverse_dynamics_f64(q).
    d_c of mpcg_generate_kkt_f64 with (clone, u') equals d_c with (plain plant, u) within LIMIT_Ggc = 8.8e-11 (the rounding of u' ~ 50 Nm: 7e-15, times
    Minv <= 1e3, times dt: 3e-13).  Not in float: rounding a 50 Nm control to float moves c by 5e-5."""
    N = 16
    xu, goals, xs = (np.asarray(a, f64) for a in P.reference_window(2, N))
    sol = solver(N, 1)
    z = np.concatenate([xu, np.zeros(m)]).reshape(N, n + m)
    tau = sol.inverse_dynamics(plant("iiwa"), dev(z[:, :NJ], f64)).cpu().numpy()
    z2 = z.copy()
    z2[:, n:] += tau
    xu2 = z2.reshape(-1)[:(n + m) * N - m]
    arrs = lambda a: (a[None], goals.reshape(1, -1), xs[None])
    c_plain = run_kkt(plain_plant("iiwa"), N, arrs(xu), f64)[3]
    c_comp = run_kkt(plant("iiwa"), N, arrs(xu2), f64)[3]
    c_raw = run_kkt(plant("iiwa"), N, arrs(xu), f64)[3]
    gap = rel_block(c_comp, c_plain)
    fig(f"compensated reference window: |tau_g| up to {np.abs(tau).max():.1f} Nm, |c| {np.abs(c_plain).max():.2e}, gap {gap:.2e}, uncompensated {rel_block(c_raw, c_plain):.2e}")
    assert np.abs(tau).max() > 10.0 and np.abs(c_plain).max() <= 5e-6
    assert gap <= LIMIT_Ggc, gap
    assert rel_block(c_raw, c_plain) > 1e-3


# ---- 11. isolation and capture ----
def test_two_clones_on_one_handle_keep_their_own_results():
    N, B = SHAPES[1]
    xu, goals, xs, dz = (dev(a) for a in inputs(1, N, B, "modest", f32))
    a, b = plant(1), plain_plant(1).with_gravity((-3.0, 0.5, -9.0))
    sol = solver(N, B)
    tail = (DT, MU, iiwa.QD_COST, iiwa.r_cost(N))

    def everything(pl):
        kkt = [t.clone() for t in sol.generate_kkt(pl, goals, xs, xu, DT, iiwa.QD_COST, iiwa.r_cost(N))]
        mer = sol.compute_merit(pl, goals, xs, xu, dz, STEPS3, *tail).clone()
        x = xs.clone()
        sol.simulate(pl, x, xu, DT, 0, 2000, 2e-4)
        tau = sol.inverse_dynamics(pl, xs[:, :NJ].contiguous())
        torch.cuda.synchronize()
        return kkt + [mer, x, tau]

    first = {id(p): everything(p) for p in (a, b)}
    for p in (b, a, a, b):
        for x, y in zip(everything(p), first[id(p)]):
            assert same(x, y)
    assert not same(first[id(a)][3], first[id(b)][3]) and not same(first[id(a)][-1], first[id(b)][-1])


def test_a_captured_sequence_replays_the_bits_of_the_eager_run():
    """KKT + merit + simulate + inverse dynamics on a gravity clone captured into one graph (the merit's scratch allocated by the eager call before): two replays
    give the eager bits."""
    N, B = 8, 3
    xu, goals, xs, dz = (dev(a) for a in inputs(2, N, B, "modest", f32))
    pl, sol = plant(2), solver(N, B)
    tail = (DT, MU, iiwa.QD_COST, iiwa.r_cost(N))
    q = xs[:, :NJ].contiguous()
    e_kkt = [t.clone() for t in sol.generate_kkt(pl, goals, xs, xu, DT, iiwa.QD_COST, iiwa.r_cost(N))]
    e_merit = sol.compute_merit(pl, goals, xs, xu, dz, STEPS3, *tail).clone()
    e_x = xs.clone()
    sol.simulate(pl, e_x, xu, DT, 0, 2000, 2e-4)
    e_tau = sol.inverse_dynamics(pl, q).clone()
    torch.cuda.synchronize()
    g_merit, g_x0, g_x, g_tau = torch.zeros(B, 3, device="cuda"), xs.clone(), xs.clone(), torch.zeros(B, NJ, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_kkt = sol.generate_kkt(pl, goals, xs, xu, DT, iiwa.QD_COST, iiwa.r_cost(N))
        sol.compute_merit(pl, goals, xs, xu, dz, STEPS3, *tail, merit=g_merit)
        g_x.copy_(g_x0)
        sol.simulate(pl, g_x, xu, DT, 0, 2000, 2e-4)
        sol.inverse_dynamics(pl, q, tau=g_tau)
    for _ in range(2):
        for t in [g_merit, g_x, g_tau] + list(g_kkt):
            t.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert same(g_merit, e_merit) and same(g_x, e_x) and same(g_tau, e_tau) and all(same(a, b) for a, b in zip(g_kkt, e_kkt))


# ---- 12. the examples ----
def run_example(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, json.loads(r.stdout.strip().splitlines()[-1])


def all_finite(x):
    if isinstance(x, dict):
        return all(all_finite(v) for v in x.values())
    if isinstance(x, list):
        return all(all_finite(v) for v in x)
    return not isinstance(x, float) or np.isfinite(x)


@pytest.mark.parametrize("double", [False, True])
def test_examples_take_gravity(double):
    """sqp_batched_iiwa(_f64) --gravity 9.81 and mpc_closed_loop(_f64) --gravity 9.81 at their smallest sizes: exit 0, finite numbers, the key in the line;
    --gravity 0 prints what a run without the flag prints, character for character; and --sim-gravity alone changes the batched run only."""
    from mpcgpu_amd import build
    exe = build.build_sqp_batched_f64() if double else build.build_sqp_batched()
    small = ("--batch", "3", "--knots", "8", "--iters", "2")
    plain, zero, heavy = run_example(exe, *small), run_example(exe, *small, "--gravity", "0"), run_example(exe, *small, "--gravity", "9.81")
    assert plain[0] == zero[0] and "gravity" not in plain[1]
    assert heavy[1]["gravity"] == 9.81 and heavy[1]["ok"] is True and all_finite(heavy[1]) and heavy[1]["merit"] != plain[1]["merit"]
    exe = build.build_mpc_closed_loop_f64() if double else build.build_mpc_closed_loop()
    small = ("--batch", "3", "--knots", "8", "--updates", "9", "--mpc-steps", "12")
    plain, zero, heavy = run_example(exe, *small), run_example(exe, *small, "--gravity", "0"), run_example(exe, *small, "--gravity", "9.81")
    assert plain[0] == zero[0] and "gravity" not in plain[1]
    assert heavy[1]["gravity"] == 9.81 and heavy[1]["sim_gravity"] == 9.81 and heavy[1]["ok"] is True and all_finite(heavy[1])
    assert heavy[1]["shifts"] == plain[1]["shifts"] and len(heavy[1]["simulate_mpc"]["tracking_errors"]) == 12
    sim_only = run_example(exe, *small, "--sim-gravity", "9.81")[1]
    assert sim_only["gravity"] == 0 and sim_only["sim_gravity"] == 9.81 and all_finite(sim_only)
    assert sim_only["tracking_errors"] != plain[1]["tracking_errors"] and sim_only["simulate_mpc"] == plain[1]["simulate_mpc"]
