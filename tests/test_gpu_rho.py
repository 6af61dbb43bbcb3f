"""GPU: rho per trajectory in device memory — mpcg_form_schur_rhov(_f64) (the three formation kernel families reading a rho VECTOR) and
mpcg_line_search_step_rho (the line-search step followed by the reference's rho adaptation, include/pcg/sqp.cuh:304-320, with rho, drho and a
"finished" flag as device state).  Formation: the oracle called once per trajectory with that trajectory's scalar rho, BIT FOR BIT.  The step: the
float32 restatement tests/rho_ref.py (pinned in tests/test_rho_ref_cpu.py), bit for bit.  The closed loop: a batched adaptive SQP loop against
independent single-trajectory loops over the scalar entry points, bit for bit, eagerly and as ONE captured iteration replayed."""
import ctypes as C
import functools
import json
import subprocess

import numpy as np
import pytest
import torch

import rho_ref
from mpcgpu_amd import _lib, iiwa, synth
from test_generic_producers_cpu import make_kkt_nm

pytestmark = pytest.mark.gpu
n, m = 14, 7
TORCH = {np.float32: torch.float32, np.float64: torch.float64}
RHOS = [1e-3, 0.5, 10.0, 3e-2, 1.7]
B5 = 5                                                         # a wavefront of four 16-lane rows: one full, one with three dead rows
STEPS8 = [-1.0 / (1 << p) for p in range(8)]
MU = 10.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def nans(*shape, dtype):
    return torch.full(shape, float("nan"), device="cuda", dtype=TORCH[dtype])


@functools.lru_cache(maxsize=None)
def inputs(nn, mm, N, dtype):
    """(G, C, g, c) of five trajectories, computed once per shape and shared; nobody writes to them."""
    k = synth.make_kkt(N, B5, 700 + N) if (nn, mm) == (n, m) else make_kkt_nm(N, B5, 9, nn, mm)
    return synth.pack_kkt_dense(k, dtype)


@functools.lru_cache(maxsize=None)
def oracle_rows(nn, mm, N, dtype, ss):
    """The oracle once per trajectory with that trajectory's SCALAR rho: [(S, Pinv, gamma, Ginv)]."""
    import oracle as orc
    G, Cd, g, c = inputs(nn, mm, N, dtype)
    return [orc.form_schur(G[b], Cd[b], g[b], c[b], N, dtype(RHOS[b]), ss=ss, n=nn, m=mm) for b in range(B5)]


def gpu_form(sol, packed, nn, mm, N, precond, dtype, rho):
    G, Cd, g, c = packed
    B = G.shape[0]
    dG = dev(G)
    S, P, gam = nans(B, 3 * nn * nn * N, dtype=dtype), nans(B, 3 * nn * nn * N, dtype=dtype), nans(B, nn * N, dtype=dtype)
    sol.form_schur(dG, dev(Cd), dev(g), dev(c), rho, precond, S=S, Pinv=P, gamma=gam, control_size=mm)
    torch.cuda.synchronize()
    return S, P, gam, dG


def check_form(orc, sol, nn, mm, N, precond, dtype):
    """S, Pinv, gamma, G^-1 and which slots stay NaN, as tests/test_gpu_generic_producers.py::check_form."""
    rho = torch.tensor(RHOS, dtype=TORCH[dtype], device="cuda")
    S, P, gam, Ginv = (t.cpu().numpy() for t in gpu_form(sol, inputs(nn, mm, N, dtype), nn, mm, N, precond, dtype, rho))
    want = oracle_rows(nn, mm, N, dtype, precond == "ss")
    for b in range(B5):
        So, Po, go, Go = want[b]
        np.testing.assert_array_equal(S[b], So, err_msg=f"S of trajectory {b}")              # NaN == NaN positions included
        np.testing.assert_array_equal(gam[b], go, err_msg=f"gamma of trajectory {b}")
        np.testing.assert_array_equal(Ginv[b], Go, err_msg=f"G^-1 of trajectory {b}")
        if precond == "none":
            assert np.isnan(P[b]).all()
        else:
            np.testing.assert_array_equal(P[b], Po, err_msg=f"Pinv of trajectory {b}")


# ---- 1. formation, bit for bit against the oracle with each trajectory's own scalar rho ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("chunk", [1, 5, 16, 0])
@pytest.mark.parametrize("N", [2, 3, 9, 33])
def test_form_schur_rhov_walking_kernels_vs_oracle(orc, N, chunk, dtype):
    """The register-resident walking kernel + seam kernel at 14 x 7, float and double; N = 33 with chunk 5 has a ragged last chunk and seams;
    chunk 0: the automatic length (1 at this size)."""
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=B5)
    sol.set_option("schur_chunk", chunk)
    check_form(orc, sol, n, m, N, "ss", dtype)
    assert sol.get_option("last_schur_chunk") == (chunk or 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("precond", ["ss", "jacobi", "none"])
def test_form_schur_rhov_every_preconditioner(orc, precond, dtype):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(9, max_batch=B5)
    sol.set_option("schur_chunk", 5)
    check_form(orc, sol, n, m, 9, precond, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [2, 9])
@pytest.mark.parametrize("nn,mm", [(6, 3), (13, 5), (17, 17)])
def test_form_schur_rhov_runtime_dimension_kernels_vs_oracle(orc, nn, mm, N, dtype):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=B5, state_size=nn, control_size=mm)
    check_form(orc, sol, nn, mm, N, "ss", dtype)
    assert sol.get_option("last_schur_chunk") == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_form_schur_rhov_tuned_shape_through_the_runtime_dimension_kernels(orc, dtype):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(9, max_batch=B5)
    sol.set_option("producers_generic", 1)
    check_form(orc, sol, n, m, 9, "ss", dtype)
    assert sol.get_option("last_schur_chunk") == 0


def test_form_schur_rhov_grid_stride_wrap_of_the_walking_kernel(orc):
    """14 x 7 float, N = 33, one block row per chunk: B x 32 items, more than four times the launch cap of num_cus x 64 workgroups of four items,
    so every wavefront walks the item list more than once and meets other trajectories (and rho values) on the way.  The data repeat with period 4,
    rho with period 5: the outputs repeat with period 20 — checked for every trajectory on the device — and the oracle gives trajectories 0, 1,
    B / 2, B - 2, B - 1."""
    from mpcgpu_amd import PcgSolver
    N = 33
    probe = PcgSolver(2, max_batch=1)
    cap = probe.get_option("num_cus") * 64
    B = (4 * cap) // (N - 1) + 1
    assert B * (N - 1) > 4 * cap
    base = tuple(a[:4] for a in inputs(n, m, N, np.float32))
    packed = tuple(np.tile(a, ((B + 3) // 4, 1))[:B] for a in base)
    rho = np.array([RHOS[b % 5] for b in range(B)], np.float32)
    sol = PcgSolver(N, max_batch=B)
    sol.set_option("schur_chunk", 1)
    outs = gpu_form(sol, packed, n, m, N, "ss", np.float32, dev(rho))
    assert sol.get_option("last_schur_chunk") == 1
    full = (B // 20) * 20
    for t in outs:
        v = t.view(torch.int32)
        assert torch.equal(v[:full].view(B // 20, 20, -1), v[:20].unsqueeze(0).expand(B // 20, -1, -1))
        assert torch.equal(v[full:], v[:B - full])
    for b in (0, 1, B // 2, B - 2, B - 1):
        want = orc.form_schur(*(a[b % 4] for a in base), N, np.float32(rho[b]), ss=True)
        for got, w in zip(outs, want):
            np.testing.assert_array_equal(got[b].cpu().numpy(), w, err_msg=f"trajectory {b}")


# ---- 2. equal entries give the scalar call's bits ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_form_schur_rhov_with_equal_entries_is_the_scalar_call(dtype):
    from mpcgpu_amd import PcgSolver
    N = 9
    sol = PcgSolver(N, max_batch=B5)
    packed = inputs(n, m, N, dtype)
    vec = torch.full((B5,), 1e-3, dtype=TORCH[dtype], device="cuda")
    for generic, chunk in ((0, 1), (1, 0)):                     # both routes on ONE handle
        sol.set_option("producers_generic", generic)
        scalar = gpu_form(sol, packed, n, m, N, "ss", dtype, 1e-3)
        assert sol.get_option("last_schur_chunk") == chunk
        vector = gpu_form(sol, packed, n, m, N, "ss", dtype, vec)
        assert sol.get_option("last_schur_chunk") == chunk
        for a0, a1 in zip(scalar, vector):
            np.testing.assert_array_equal(a0.cpu().numpy(), a1.cpu().numpy())


# ---- 3. the step on synthetic merits ----
@pytest.mark.parametrize("nn,mm", [(14, 7), (6, 3)])
def test_line_search_step_rho_on_synthetic_merits(nn, mm):
    """14 consecutive calls, compared with tests/rho_ref.py after every one: rho, drho, merit_ref and xu as integer views, done and step exact.
    Trajectory 0 always fails from rho = 1e-3 and gives up at call 10; 1 starts at rho = 5 and gives up at call 3; 2 always succeeds; 3 alternates;
    4 sees NaN rows only (a failure each); 5 comes with `done` set by the caller.  A frozen trajectory's arrays keep the bits of the call that froze them."""
    from mpcgpu_amd import PcgSolver
    N, B, calls = 4, 6, 14
    L = (nn + mm) * N - mm
    rng = np.random.default_rng(12)
    steps = [-1.0, -0.5, -0.25, -0.125]
    reset = 0.25
    h = dict(xu=rng.standard_normal((B, L)).astype(np.float32), ref=np.full(B, 100.0, np.float32),
             rho=np.array([1e-3, 5.0, 1e-3, 1e-3, 5e-3, 0.7], np.float32), drho=np.array([1, 1, 1, 1, 1, 3], np.float32),
             done=np.array([0, 0, 0, 0, 0, 3], np.uint8))
    sol = PcgSolver(N, max_batch=B, state_size=nn, control_size=mm)
    d = {k: dev(v.copy()) for k, v in h.items()}
    d_step = torch.zeros(B, dtype=torch.int32, device="cuda")
    frozen_at = {}
    for t in range(calls):
        dz = rng.standard_normal((B, L)).astype(np.float32)
        merit = np.full((B, 4), 200.0, np.float32)               # above every merit_ref: a failure
        merit[2] = [150, 99 - t, 99 - t, 160] if t % 2 else [99 - t, 120, 99.5 - t, 98.5 - t]
        if t % 2:
            merit[3, t % 4] = 99.0 - t
        merit[4] = np.nan
        merit[5] = 1.0                                           # would be a success, were the trajectory not frozen
        sol.line_search_step_rho(dev(merit), steps, d["ref"], dev(dz), d["xu"], d["rho"], d["drho"], d["done"], rho_reset=reset, step=d_step)
        torch.cuda.synchronize()
        want = rho_ref.step(merit, steps, h["ref"], dz, h["xu"], h["rho"], h["drho"], h["done"], rho_reset=reset)
        got = d_step.cpu().numpy()
        assert np.array_equal(got, want), (t, got, want)
        for k in h:
            assert np.array_equal(bits(d[k]), bits(h[k])), (t, k, d[k].cpu().numpy(), h[k])
        for b in range(B):
            if h["done"][b] and b not in frozen_at:
                frozen_at[b] = (t, {k: bits(d[k])[b].copy() for k in h})
            elif b in frozen_at:
                assert got[b] == _lib.MPCG_STEP_FROZEN
                for k in h:
                    assert np.array_equal(bits(d[k])[b], frozen_at[b][1][k]), (t, b, k)
    assert {b: t for b, (t, _) in frozen_at.items()} == {0: 9, 1: 2, 5: 0, 4: 8}          # (call numbers from 0; from rho = 5e-3 the ninth product, 18.3, is already beyond rho_max)
    assert h["rho"][0] == np.float32(reset) and h["done"].tolist() == [1, 1, 0, 0, 1, 3] and h["rho"][5] == np.float32(0.7)
    assert h["rho"][2] == np.float32(1e-3) and h["drho"][2] < 0.1              # clamped, drho still shrinking


# ---- 4. / 5. the closed loop ----
ITERS = 5
RHO0 = [1e-3, 5.0, 0.1]
WINDOWS = (8, 3, 19)                                                            # N, B, seed of iiwa.random_windows


def sqp_env():
    from mpcgpu_amd import PcgSolver, Plant, pcg_config
    N, B, seed = WINDOWS
    xu, goals, xs = iiwa.random_windows(N, B, seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return PcgSolver, Plant(), pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=3000), N, B, f(xu), f(goals.reshape(B, -1)), f(xs)


class Loop:
    """The state of a batched adaptive loop on one handle and its six calls (stage settings: tests/test_gpu_merit.py::test_closed_loop_sqp_on_the_device)."""

    def __init__(self, PcgSolver, plant, cfg, N, xu, goals, xs, rho0, zero_ref=()):
        B = len(xu)
        self.sol, self.plant, self.cfg, self.N, self.B = PcgSolver(N, max_batch=B), plant, cfg, N, B
        self.goals, self.xs, self.xu = dev(goals), dev(xs), dev(xu)
        self.lam = torch.zeros(B, n * N, device="cuda")
        self.tail = (iiwa.TIMESTEP, MU, iiwa.QD_COST, iiwa.r_cost(N))
        self.ref = self.sol.compute_merit(plant, self.goals, self.xs, self.xu, None, [0.0], *self.tail).reshape(B).clone()
        for b in zero_ref:
            self.ref[b] = 0.0                                   # merits are non-negative and the comparison is strict: every search of b fails
        self.rho = torch.tensor(rho0, dtype=torch.float32, device="cuda")
        self.drho = torch.ones(B, device="cuda")
        self.done = torch.zeros(B, dtype=torch.uint8, device="cuda")
        self.step = torch.zeros(B, dtype=torch.int32, device="cuda")

    def front(self, rho):
        """generate_kkt -> form_schur -> solve -> compute_dz -> compute_merit"""
        s = self.sol
        G, Cd, g, c = s.generate_kkt(self.plant, self.goals, self.xs, self.xu, iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(self.N))
        S, Pinv, gam = s.form_schur(G, Cd, g, c, rho, "ss")
        s.solve(S, Pinv, gam, self.lam, self.cfg, "ss")
        dz = s.compute_dz(G, Cd, g, self.lam)
        return dz, s.compute_merit(self.plant, self.goals, self.xs, self.xu, dz, STEPS8, *self.tail)

    def adaptive_iteration(self, reset):
        dz, merit = self.front(self.rho)
        self.sol.line_search_step_rho(merit, STEPS8, self.ref, dz, self.xu, self.rho, self.drho, self.done, rho_reset=reset, step=self.step)

    def state(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("xu", "ref", "rho", "drho", "done", "step")}


RESET = 2e-3


@functools.lru_cache(maxsize=None)
def eager_batched():
    """The batched adaptive loop run eagerly: its state after every iteration, computed once and shared by tests 4 and 5."""
    PcgSolver, plant, cfg, N, B, xu, goals, xs = sqp_env()
    loop = Loop(PcgSolver, plant, cfg, N, xu, goals, xs, RHO0, zero_ref=(1,))
    states = []
    for _ in range(ITERS):
        loop.adaptive_iteration(RESET)
        states.append(loop.state())
    return states


def test_closed_loop_batched_adaptive_vs_single_trajectory_loops():
    """Batched: rho tensor + line_search_step_rho, nothing read back inside the loop.  Reference side, per trajectory alone (max_batch = 1): the
    scalar form_schur(float(rho)) and line_search_step, the rule of tests/rho_ref.py on the host, stopping at give-up.  Trajectory 1 starts at
    rho = 5 with merit_ref = 0: it fails three times (6, 8.64, 14.93 > 10), gives up and is frozen for the last two iterations with its initial xu.
    No tolerance and no pair left out: every stage is batch-independent by its own tests."""
    PcgSolver, plant, cfg, N, B, xu, goals, xs = sqp_env()
    got = eager_batched()
    final = got[-1]
    for b in range(B):
        one = Loop(PcgSolver, plant, cfg, N, xu[b:b + 1], goals[b:b + 1], xs[b:b + 1], RHO0[b:b + 1], zero_ref=(0,) if b == 1 else ())
        rho, drho, done = np.float32(RHO0[b]), np.float32(1.0), False
        hist = []
        for it in range(ITERS):
            if done:
                hist.append(_lib.MPCG_STEP_FROZEN)
                continue
            dz, merit = one.front(float(rho))
            p = int(one.sol.line_search_step(merit, STEPS8, one.ref, dz, one.xu).cpu()[0])
            hist.append(p)
            rho, drho, done = rho_ref.update(rho, drho, p, rho_reset=RESET)
        torch.cuda.synchronize()
        assert [int(s["step"][b]) for s in got] == hist, (b, hist)
        assert np.array_equal(bits(final["xu"][b]), bits(one.xu)[0]), b
        assert bits(final["ref"])[b] == bits(one.ref)[0], b
        assert bits(final["rho"])[b] == bits(np.array([rho], np.float32))[0] and bits(final["drho"])[b] == bits(np.array([drho], np.float32))[0], b
        assert int(final["done"][b]) == int(done), b
    assert [int(s["step"][1]) for s in got] == [-1, -1, -1, -2, -2] and final["done"].tolist() == [0, 1, 0]
    assert np.array_equal(bits(final["xu"][1]), bits(xu[1])) and final["ref"][1] == 0.0 and final["rho"][1] == np.float32(RESET)
    # rho moved between iterations: from 0.1 every outcome changes it (x 1.2 or more, or / 1.2 or more; the floor is five successes away).
    # (Trajectory 0 starts AT the floor 1e-3: as long as its searches succeed it stays there.)
    assert len({float(s["rho"][2]) for s in got}) > 1


def test_one_captured_adaptive_iteration_replays_for_the_whole_solve():
    """After one eager iteration on the handle the six calls are captured ONCE (a linear chain) and replayed four times: the state after each
    replay is the eager loop's after that iteration, bit for bit — with a rho that differs from replay to replay, which a captured scalar could not."""
    PcgSolver, plant, cfg, N, B, xu, goals, xs = sqp_env()
    want = eager_batched()
    loop = Loop(PcgSolver, plant, cfg, N, xu, goals, xs, RHO0, zero_ref=(1,))
    loop.adaptive_iteration(RESET)
    first = loop.state()
    for k in first:
        assert np.array_equal(bits(first[k]), bits(want[0][k])), k
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        loop.adaptive_iteration(RESET)
    rhos = [first["rho"].copy()]
    for it in range(1, ITERS):
        graph.replay()
        got = loop.state()
        for k in got:
            assert np.array_equal(bits(got[k]), bits(want[it][k])), (it, k)
        rhos.append(got["rho"].copy())
    assert all(not np.array_equal(a, b) for a, b in zip(rhos, rhos[1:]))


# ---- 6. argument errors ----
def test_argument_errors():
    """Every row of include/mpcg.h's table for mpcg_line_search_step_rho; for the formation entries a null d_rho, batch > max_batch and batch 0; a
    first mpcg_form_schur_rhov on a capturing stream of a fresh handle is refused like mpcg_form_schur's and leaves the capture usable."""
    from mpcgpu_amd import PcgSolver
    lib = _lib.load()
    N, B = 4, 2
    sol = PcgSolver(N, max_batch=B)
    L = (n + m) * N - m
    xu, dz = (torch.zeros(B, L, device="cuda") for _ in range(2))
    merit, ref = torch.zeros(B, 16, device="cuda"), torch.zeros(B, device="cuda")
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    rho, drho = torch.full((B,), 1e-3, device="cuda"), torch.ones(B, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    arr = lambda v: (C.c_float * len(v))(*v)

    def ls(h=sol._h, cs=7, merit=merit, steps=arr([-1.0, -0.5]), A=2, ref=ref, dz=dz, xu=xu, step=step, rho=rho, drho=drho, done=done,
           factor=1.2, lo=1e-3, hi=10.0, reset=1e-3, batch=B):
        return lib.mpcg_line_search_step_rho(h, cs, p(merit), steps, A, p(ref), p(dz), p(xu), p(step), p(rho), p(drho), p(done), factor, lo, hi, reset, batch, None)

    INV, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_OK
    assert ls() == OK
    assert ls(h=None) == INV
    for kw in ("merit", "steps", "ref", "dz", "xu", "step", "rho", "drho", "done"):
        assert ls(**{kw: None}) == INV, kw
    big = arr([-1.0] * 17)
    assert ls(A=0) == INV and ls(steps=big, A=17) == INV and ls(steps=arr([-1.0] * 16), A=16) == OK
    assert ls(batch=B + 1) == INV
    assert b"max_batch" in lib.mpcg_last_error(sol._h)
    assert ls(batch=0) == OK
    assert ls(cs=0) == INV and ls(cs=15) == INV
    for kw in ("factor", "lo", "hi", "reset"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert ls(**{kw: bad}) == INV, (kw, bad)
    assert ls(factor=1.0) == INV and ls(factor=0.5) == INV and ls(factor=1.0000001) == OK
    assert ls(lo=0.0) == INV and ls(lo=-1.0) == INV
    assert ls(lo=2.0, hi=1.0) == INV and ls(lo=2.0, hi=2.0) == OK
    assert ls(reset=0.0) == OK and ls(reset=100.0) == OK                  # rho_reset is the caller's: any finite value
    torch.cuda.synchronize()

    for dtype, fn in ((np.float32, lib.mpcg_form_schur_rhov), (np.float64, lib.mpcg_form_schur_rhov_f64)):
        G, Cd, g, c = (dev(a[:B]) for a in inputs(n, m, N, dtype))
        S, P, gam = (nans(B, k, dtype=dtype) for k in (3 * n * n * N, 3 * n * n * N, n * N))
        r = torch.full((B,), 1e-3, dtype=TORCH[dtype], device="cuda")
        fs = lambda rho=r, batch=B: fn(sol._h, m, p(G), p(Cd), p(g), p(c), p(S), p(P), p(gam), p(rho), batch, _lib.MPCG_PRECOND_SS, None)
        assert fs(rho=None) == INV
        assert b"null device pointer" in lib.mpcg_last_error(sol._h)
        assert fs(batch=B + 1) == INV
        assert fs(batch=0) == OK
        torch.cuda.synchronize()
        assert np.isnan(S.cpu().numpy()).all()                               # nothing was launched by any of them
        assert fs() == OK
        torch.cuda.synchronize()
        assert not np.isnan(gam.cpu().numpy()).any()

    # a FIRST call inside a stream capture: refused (the handle-owned buffers are not stream work), the capture stays usable
    G, Cd, g, c = (dev(a[:B]) for a in inputs(n, m, N, np.float32))
    S, P, gam = (nans(B, k, dtype=np.float32) for k in (3 * n * n * N, 3 * n * n * N, n * N))
    r = torch.full((B,), 1e-3, device="cuda")
    fresh = PcgSolver(N, max_batch=B)
    marker = torch.zeros(4, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="outside the stream capture") as ei:
            fresh.form_schur(G, Cd, g, c, r, "ss", S=S, Pinv=P, gamma=gam)
        assert ei.value.code == INV
        marker.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert marker.tolist() == [1.0] * 4 and np.isnan(S.cpu().numpy()).all()


# ---- 7. the example ----
def test_batched_sqp_example_with_adaptive_rho():
    from mpcgpu_amd import build
    exe = build.build_sqp_batched()
    r = subprocess.run([exe, "--adapt-rho"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["batch"] == 8 and out["iters"] == 4
    for key in ("rho_final", "drho_final", "done"):
        assert len(out[key]) == 8, key
    assert out["done"] == [0] * 8
    assert all(1e-3 <= v <= 10.0 for v in out["rho_final"]) and all(v > 0 for v in out["drho_final"])
