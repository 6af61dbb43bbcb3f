"""GPU: mpcg_generate_kkt_f64 (mpcgpu_amd/csrc/kkt_plant.hip.h: generate_kkt_kernel with IO = double) — the KKT block assembly with double arrays in and out, the producer of
mpcg_form_schur(_rhov)_f64.  The arithmetic is the float entry's (float64 inside): on float-representable inputs the outputs rounded to float ARE the
float entry's bits; on genuinely double inputs nothing passes through float; against the float64 restatement oracle/iiwa_ref.py the arrays without a
dynamics derivative agree far below the float entry's output rounding.  Bit-stability over the batch, inside a hipGraph, guard bands, errors, and the
Python dispatch on dtype."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import iiwa_ref
from mpcgpu_amd import _lib, iiwa

pytestmark = pytest.mark.gpu
n, m = 14, 7
QD32 = float(np.float32(iiwa.QD_COST))                         # the cost as the float entry sees it


def r32(N):
    return float(np.float32(iiwa.r_cost(N)))


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def env():
    from mpcgpu_amd import PcgSolver, Plant
    return PcgSolver, Plant()


@functools.lru_cache(maxsize=None)
def big_batch():
    """Just over the grid cap of 32 x num_cus workgroups of four items at N = 128: a workgroup runs more than one trip (259 on a 256-CU part)."""
    from mpcgpu_amd import PcgSolver
    cus = PcgSolver(2, max_batch=1).get_option("num_cus")
    B = (128 * cus) // 127 + 1
    assert B * 127 > 128 * cus
    return B


def shapes():
    return [(2, 1), (3, 5), (9, 3), (128, big_batch())]


@functools.lru_cache(maxsize=None)
def windows32(N, B):
    """(xu, goals, xs) rounded to float32 — what both entries can be given — computed once per shape; nobody writes to them."""
    if B > 16:                                                 # the large batch: sixteen windows repeated (a knot's blocks do not depend on the batch)
        xu, goals, xs = windows32(N, 16)
        rep = lambda a: np.concatenate([a] * ((B + 15) // 16))[:B]
        return rep(xu), rep(goals), rep(xs)
    xu, goals, xs = iiwa.random_windows(N, B, 300 + N)
    return tuple(np.ascontiguousarray(a, np.float32) for a in (xu, goals.reshape(B, -1), xs))


@functools.lru_cache(maxsize=None)
def windows64(N, B):
    """Genuinely double inputs: the float32 values times (1 + 1e-12 r), r uniform in [-1, 1] — none of them is a float."""
    rng = np.random.default_rng(7 + N)
    out = tuple(a.astype(np.float64) * (1.0 + 1e-12 * rng.uniform(-1, 1, a.shape)) for a in windows32(N, B))
    assert all((a != a.astype(np.float32)).mean() > 0.9 for a in (out[0], out[2]))
    return out


def kkt(sol, plant, N, arrs, dtype, qd=None, r=None):
    xu, goals, xs = (dev(a, dtype) for a in arrs)
    out = sol.generate_kkt(plant, goals, xs, xu, iiwa.TIMESTEP, QD32 if qd is None else qd, r32(N) if r is None else r)
    torch.cuda.synchronize()
    return out


# ---- 1. the float entry's arithmetic, bit for bit ----
@pytest.mark.parametrize("analytic", [1, 0])
@pytest.mark.parametrize("case", range(4))
def test_outputs_rounded_to_float_are_the_float_entry(env, case, analytic):
    """Inputs that are floats widened, timestep 1/64 and costs that are floats: out64.astype(float32) equals mpcg_generate_kkt's G, C, g, c bitwise, on
    both gradient routes.  (2, 1): one item that is first and last block at once; (3, 5), (9, 3): B (N - 1) no multiple of a wavefront's four items;
    (128, 259 on 256 CUs): a workgroup runs more than one trip."""
    PcgSolver, plant = env
    N, B = shapes()[case]
    sol = PcgSolver(N, max_batch=B)
    sol.set_option("kkt_analytic", analytic)
    arrs = windows32(N, B)
    o32 = kkt(sol, plant, N, arrs, np.float32)
    o64 = kkt(sol, plant, N, arrs, np.float64)
    for a32, a64, name in zip(o32, o64, "GCgc"):
        assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and a64.shape == a32.shape
        assert torch.isfinite(a64).all(), name
        assert torch.equal(a64.to(torch.float32).view(torch.int32), a32.view(torch.int32)), (N, B, name)
    # and the doubles are not floats widened: the stores did not go through float
    assert (o64[1].to(torch.float32).to(torch.float64) != o64[1]).float().mean() > 0.3


# ---- 2. the inputs are not squeezed through float ----
@pytest.mark.parametrize("N,B", [(2, 1), (3, 5), (9, 3)])
def test_double_inputs_are_used_as_they_are(env, N, B):
    """c_0 = x_0 - x_s is one correctly rounded subtraction on both sides: on double inputs it equals numpy's float64 difference bit for bit (through
    float it would be the difference of the rounded values)."""
    PcgSolver, plant = env
    xu, goals, xs = windows64(N, B)
    sol = PcgSolver(N, max_batch=B)
    c = kkt(sol, plant, N, (xu, goals, xs), np.float64)[3].cpu().numpy()
    want = xu[:, :n] - xs
    assert np.array_equal(bits(c[:, :n]), bits(want))
    squeezed = xu[:, :n].astype(np.float32).astype(np.float64) - xs.astype(np.float32).astype(np.float64)
    assert not np.array_equal(bits(want), bits(squeezed))


# ---- 3. accuracy against the float64 restatement, on double inputs ----
# Limits: ten times the measured worst of the first measured run (below and DESIGN.md §3.10); the margin covers other seeds.  The limit of C is the
# restatement's: its central differences (h = 1e-6) carry ~1e-9 |dID| / h of rounding noise, which the analytic recursion on the device does not.
LIMIT_Ggc = 8.8e-11
LIMIT_C = 8.9e-7


@functools.lru_cache(maxsize=None)
def restated(N, B, b):
    """oracle/iiwa_ref.py on trajectory b of the double windows of shape (N, B), once."""
    xu, goals, xs = windows64(N, B)
    return iiwa_ref.generate_kkt(iiwa_ref.Model(), xu[b], goals[b].reshape(N, 6), xs[b], N)


def test_accuracy_against_the_host_restatement(env):
    """Worst |got - want| / max(1, max |want block array|) per group over the shapes of test 1 (every trajectory of the three small ones; the last
    trajectory of the large one, whose knots belong to a workgroup's second trip — the restatement is a Python loop over knots).  G, g, c carry no dynamics derivative; C = (-A, -B) is limited by
    the restatement's central differences (h = 1e-6, ~1e-9 |dID| / h).  Costs are the exact doubles 1e-4 here, as the restatement's.
    Measured worst: G, g, c 8.77e-12 (8.71e-12 already at N = 2), C 8.88e-8 (2.1e-8 / 2.9e-8 / 3.4e-8 / 8.9e-8 with the four shapes added one by one) — the
    float entry's figure for all four arrays is 2e-7, the rounding of its float stores."""
    PcgSolver, plant = env
    worst = {"Ggc": 0.0, "C": 0.0}
    for N, B in shapes():
        sol = PcgSolver(N, max_batch=B)
        got = [t.cpu().numpy() for t in kkt(sol, plant, N, windows64(N, B), np.float64, qd=iiwa.QD_COST, r=iiwa.r_cost(N))]
        for b in (range(B) if B <= 16 else (B - 1,)):
            want = restated(N, B, b)
            for a, w, name in zip(got, want, "GCgc"):
                err = np.abs(a[b] - w).max() / max(1.0, np.abs(w).max())
                key = "C" if name == "C" else "Ggc"
                worst[key] = max(worst[key], err)
        print(f"N={N} B={B}: worst so far G,g,c {worst['Ggc']:.3e}  C {worst['C']:.3e}")
    assert worst["Ggc"] < 2e-7, worst                          # the rounding this entry removes
    assert worst["Ggc"] <= LIMIT_Ggc and worst["C"] <= LIMIT_C, worst


# ---- 4. a trajectory's bits do not depend on the batch ----
def test_bits_do_not_depend_on_the_batch(env):
    PcgSolver, plant = env
    N, B = 3, 5
    arrs = windows64(N, B)
    sol = PcgSolver(N, max_batch=B)
    full = [bits(t) for t in kkt(sol, plant, N, arrs, np.float64)]
    for b in range(B):
        one = [bits(t) for t in kkt(sol, plant, N, tuple(a[b:b + 1] for a in arrs), np.float64)]
        for f, o, name in zip(full, one, "GCgc"):
            assert np.array_equal(f[b], o[0]), (b, name)


# ---- 5. a captured call replays the eager bits ----
def test_replay_from_a_hipgraph(env):
    """Pure stream work from the FIRST call: a fresh handle is captured without an eager call before."""
    PcgSolver, plant = env
    N, B = 9, 3
    arrs = windows64(N, B)
    eager = [bits(t) for t in kkt(PcgSolver(N, max_batch=B), plant, N, arrs, np.float64)]
    xu, goals, xs = (dev(a, np.float64) for a in arrs)
    sol = PcgSolver(N, max_batch=B)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        outs = sol.generate_kkt(plant, goals, xs, xu, iiwa.TIMESTEP, QD32, r32(N))
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want, name in zip(outs, eager, "GCgc"):
            assert np.array_equal(bits(got), want), name


# ---- 6. / 8. raw calls: guard bands and errors ----
def raw_call(lib, sol, plant, N, B, xu, goals, xs, outs, h=True, pl=True, cs=7, batch=None):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    return lib.mpcg_generate_kkt_f64(sol._h if h else None, plant._p if pl else None, cs, iiwa.TIMESTEP, p(goals), p(xs), p(xu), QD32, r32(N),
                                     p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), B if batch is None else batch, None)


def out_lens(N, B):
    return [B * ((n * n + m * m) * N - m * m), B * (n * n + n * m) * (N - 1), B * ((n + m) * N - m), B * n * N]


@pytest.mark.parametrize("N,B", [(2, 1), (3, 5)])
def test_nothing_outside_the_four_arrays_is_written(env, N, B):
    """Each output lies between two bands of 512 NaNs: every element inside is written (finite), every band element is still a NaN."""
    PcgSolver, plant = env
    lib = _lib.load()
    sol = PcgSolver(N, max_batch=B)
    xu, goals, xs = (dev(a, np.float64) for a in windows64(N, B))
    W = 512
    bufs = [torch.full((ln + 2 * W,), float("nan"), dtype=torch.float64, device="cuda") for ln in out_lens(N, B)]
    views = [b[W:-W] for b in bufs]
    assert raw_call(lib, sol, plant, N, B, xu, goals, xs, views) == _lib.MPCG_OK
    torch.cuda.synchronize()
    for b, name in zip(bufs, "GCgc"):
        assert torch.isnan(b[:W]).all() and torch.isnan(b[-W:]).all(), name
        assert torch.isfinite(b[W:-W]).all(), name


def test_float_entry_is_untouched_by_double_calls(env):
    """A float mpcg_generate_kkt on the same handle before and after a double call gives identical bits; float64 tensors reach the _f64 entry (result
    dtype), and mixed float32 / float64 arguments raise TypeError."""
    PcgSolver, plant = env
    N, B = 9, 3
    sol = PcgSolver(N, max_batch=B)
    arrs = windows32(N, B)
    before = [bits(t) for t in kkt(sol, plant, N, arrs, np.float32)]
    o64 = kkt(sol, plant, N, windows64(N, B), np.float64)
    assert all(t.dtype == torch.float64 for t in o64)
    after = kkt(sol, plant, N, arrs, np.float32)
    assert all(t.dtype == torch.float32 for t in after)
    for a, b, name in zip(before, after, "GCgc"):
        assert np.array_equal(a, bits(b)), name
    xu, goals, xs = arrs
    for mixed in ((np.float64, np.float32, np.float32), (np.float32, np.float64, np.float32), (np.float32, np.float32, np.float64)):
        with pytest.raises(TypeError):
            sol.generate_kkt(plant, dev(goals, mixed[0]), dev(xs, mixed[1]), dev(xu, mixed[2]), iiwa.TIMESTEP, QD32, r32(N))
    with pytest.raises(TypeError):
        sol.generate_kkt(plant, dev(goals, np.float16), dev(xs, np.float16), dev(xu, np.float16), iiwa.TIMESTEP, QD32, r32(N))


def test_argument_errors(env):
    """The float twin's table: a null pointer, state_size != 14 or control_size != 7 (UNSUPPORTED), batch > max_batch, a plant on another device, and
    batch == 0 = MPCG_OK with nothing written."""
    PcgSolver, plant = env
    lib = _lib.load()
    N, B = 3, 2
    sol = PcgSolver(N, max_batch=B)
    xu, goals, xs = (dev(a[:B], np.float64) for a in windows64(N, 5))
    outs = [torch.full((ln,), float("nan"), dtype=torch.float64, device="cuda") for ln in out_lens(N, B)]
    INV, UNS, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_ERR_UNSUPPORTED, _lib.MPCG_OK
    call = lambda **kw: raw_call(lib, sol, plant, N, B, kw.pop("xu", xu), kw.pop("goals", goals), kw.pop("xs", xs), kw.pop("outs", outs), **kw)
    assert call(h=False) == INV and call(pl=False) == INV
    for kw in ("xu", "goals", "xs"):
        assert call(**{kw: None}) == INV, kw
    assert b"mpcg_generate_kkt_f64: null device pointer" in lib.mpcg_last_error(sol._h)
    for i in range(4):
        assert call(outs=[None if j == i else o for j, o in enumerate(outs)]) == INV, i
    assert call(cs=6) == UNS
    small = PcgSolver(N, max_batch=B, state_size=6, control_size=3)
    assert raw_call(lib, small, plant, N, B, xu, goals, xs, outs, cs=3) == UNS and raw_call(lib, small, plant, N, B, xu, goals, xs, outs) == UNS
    assert call(batch=B + 1) == INV
    assert b"max_batch" in lib.mpcg_last_error(sol._h)
    # a plant on another device (the first member of the opaque mpcg_plant is its device index: tests/test_gpu_merit.py::test_argument_errors)
    dev_field = C.cast(plant._p, C.POINTER(C.c_int))
    own = dev_field[0]
    dev_field[0] = own + 1
    try:
        assert call() == INV
        assert b"different devices" in lib.mpcg_last_error(sol._h)
    finally:
        dev_field[0] = own
    assert call(batch=0) == OK
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)             # nothing was launched by any of them
    assert call() == OK
    torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() for o in outs)
