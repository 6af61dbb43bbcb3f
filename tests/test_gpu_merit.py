"""GPU: mpcg_compute_merit and mpcg_line_search_step (mpcgpu_amd/csrc/merit_plant.hip.h) — the merit function of the SQP line search batched over
trajectories and step sizes, and the reference's step selection + update (include/common/merit.cuh:16-143, include/pcg/sqp.cuh:264-353) — against
the float64 restatement tests/plant_ref.py (pinned on the reference's own trajectory: tests/test_merit_ref_cpu.py), directly against that trajectory,
for bit-stability, inside a hipGraph, and closing the loop of a device-side SQP iteration: KKT -> Schur -> PCG -> dz -> merit -> step."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest
import torch

import iiwa_ref
import plant_ref as P
from mpcgpu_amd import _lib, iiwa

pytestmark = pytest.mark.gpu
n, m = 14, 7
STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]          # 0, -1, -1/2, ..., -1/128
STEPS8 = STEPS9[1:]
MU = 10.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def env():
    from mpcgpu_amd import PcgSolver, Plant, pcg_config
    return PcgSolver, Plant(), pcg_config, iiwa_ref.Model()


_cases = {}


def case(N, B):
    """Inputs of the restatement tests and the host's merits for them, computed once per shape."""
    if (N, B) not in _cases:
        xu, goals, xs = iiwa.random_windows(N, B, 11 + N)
        dz = 0.05 * np.random.default_rng(1000 + N).standard_normal(xu.shape)
        M = iiwa_ref.Model()
        r = iiwa.r_cost(N)
        want = {with_xs: P.merits(M, xu, dz, STEPS9, P.f32(goals), P.f32(xs if with_xs else None), N, MU, cost=P.Cost.plain(iiwa.QD_COST, r)) for with_xs in (True, False)}
        _cases[(N, B)] = (xu, goals, xs, dz, want)
    return _cases[(N, B)]


def call(sol, plant, N, goals, xs, xu, dz, steps, mu=MU):
    B = len(xu)
    return sol.compute_merit(plant, dev(goals.reshape(B, -1)), None if xs is None else dev(xs), dev(xu), None if dz is None else dev(dz), steps,
                             iiwa.TIMESTEP, mu, iiwa.QD_COST, iiwa.r_cost(N))


@pytest.mark.parametrize("with_xs", [True, False])
@pytest.mark.parametrize("N,B", [(2, 1), (3, 2), (8, 3), (9, 1), (32, 2)])
def test_merit_vs_host_restatement(env, N, B, with_xs):
    """|got - want| <= 1e-6 max(1, |want|): the float rounding of ONE output number (6e-8 relative) with the margin the KKT tests give the float64-inside
    build.  N = 2 is one dynamics item + the pose-only last item; (3, 2) x 9 = 54 items leaves the last wavefront partly idle.  with_xs = False:
    d_xs = NULL, the reference's compute_merit without the initial-state term.  Merits here: 1 .. 300.
    Measured worst |got - want| / max(1, |want|): 5.4e-8 (N = 8, B = 3, with d_xs); every case 3.2e-8 .. 5.4e-8."""
    PcgSolver, plant, _, _ = env
    xu, goals, xs, dz, want = case(N, B)
    sol = PcgSolver(N, max_batch=B)
    got = call(sol, plant, N, goals, xs if with_xs else None, xu, dz, STEPS9).cpu().numpy().astype(np.float64)
    assert got.shape == (B, 9) and np.isfinite(got).all()
    w = want[with_xs]
    err = np.abs(got - w) / np.maximum(1.0, np.abs(w))
    print(f"N={N} B={B} xs={with_xs}: merits {w.min():.3g} .. {w.max():.3g}, worst error {err.max():.2e}")
    assert err.max() <= 1e-6, (err.max(), got, w)
    if with_xs:
        assert (want[True][:, 1:] > want[False][:, 1:]).all()      # every step moves x_0 off x_s (the windows start AT x_s): the term is there


def test_merit_vanishes_on_the_reference_trajectory(env):
    """The device pin on reference-held data: the windows and the bound of tests/test_merit_ref_cpu.py through mpcg_compute_merit with step size 0 and
    d_dz = NULL.  Measured 1.4e-5 .. 5.0e-5 against 4.3e-4 / 8.8e-4 (the host restatement's figures to three digits)."""
    PcgSolver, plant, _, _ = env
    for t0, N in P.WINDOWS:
        xu, goals, xs = P.reference_window(t0, N)
        sol = PcgSolver(N, max_batch=1)
        got = float(sol.compute_merit(plant, dev(goals.reshape(1, -1)), dev(xs.reshape(1, -1)), dev(xu.reshape(1, -1)), None, [0.0],
                                      iiwa.TIMESTEP, 1.0, 0.0, 0.0).cpu()[0, 0])
        print(f"rows {t0}..{t0 + N - 1}: merit {got:.3e}, bound {14 * (N - 1) * 1e-6:.3e}")
        assert 0.0 <= got <= 14 * (N - 1) * 1e-6, (t0, got)


def test_merit_bits(env):
    """The same call twice; a trajectory inside a batch of 7 and alone; num_steps = 1, 9 and 16 for the step sizes they share: the same bits."""
    PcgSolver, plant, _, _ = env
    N, B = 8, 7
    xu, goals, xs = iiwa.random_windows(N, B, 77)
    dz = 0.05 * np.random.default_rng(78).standard_normal(xu.shape)
    sol = PcgSolver(N, max_batch=B)
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    full = bits(call(sol, plant, N, goals, xs, xu, dz, STEPS9))
    assert np.array_equal(full, bits(call(sol, plant, N, goals, xs, xu, dz, STEPS9)))
    for b in (0, 3, 6):
        alone = bits(call(sol, plant, N, goals[b:b + 1], xs[b:b + 1], xu[b:b + 1], dz[b:b + 1], STEPS9))
        assert np.array_equal(alone[0], full[b]), b
    one = bits(call(sol, plant, N, goals, xs, xu, dz, [-0.25]))
    assert np.array_equal(one[:, 0], full[:, STEPS9.index(-0.25)])
    steps16 = STEPS9 + [-0.75, 0.5, -0.3, 1e-3, -1.0, 0.0, -2.0]
    sixteen = bits(call(sol, plant, N, goals, xs, xu, dz, steps16))
    assert np.array_equal(sixteen[:, :9], full)
    assert np.array_equal(sixteen[:, 13], full[:, 1]) and np.array_equal(sixteen[:, 14], full[:, 0])      # the same step size in another slot


@pytest.mark.parametrize("nn,mm", [(14, 7), (6, 3)])
def test_line_search_step_on_synthetic_merits(nn, mm):
    """include/pcg/sqp.cuh:292-301, 317, 332-338, 352 per trajectory, on a 14 x 7 and on a 6 x 3 handle (no dynamics in this call)."""
    from mpcgpu_amd import PcgSolver
    N, B = 4, 6
    L = (nn + mm) * N - mm
    rng = np.random.default_rng(5)
    xu0 = rng.standard_normal((B, L)).astype(np.float32)
    dz = rng.standard_normal((B, L)).astype(np.float32)
    steps = [-1.0, -0.5, -0.25, -0.125]
    nan = float("nan")
    merit = np.array([[5, 6, 7, 8],              # nothing better than merit_ref = 4
                      [3, 2, 2, 9],              # a tie: the first
                      [4, 4, 4, 4],              # equal to merit_ref: not accepted
                      [nan, 3, nan, 1],          # a NaN is never chosen
                      [nan, nan, nan, nan],
                      [9, 9, 9, 3.5]], np.float32)
    ref0 = np.full(B, 4.0, np.float32)
    want_p = np.array([-1, 1, -1, 3, -1, 3], np.int32)
    sol = PcgSolver(N, max_batch=B, state_size=nn, control_size=mm)
    d_xu, d_ref = torch.from_numpy(xu0.copy()).cuda(), torch.from_numpy(ref0.copy()).cuda()
    step = sol.line_search_step(torch.from_numpy(merit).cuda(), steps, d_ref, torch.from_numpy(dz).cuda(), d_xu)
    torch.cuda.synchronize()
    assert step.dtype == torch.int32 and np.array_equal(step.cpu().numpy(), want_p)
    got_xu, got_ref = d_xu.cpu().numpy(), d_ref.cpu().numpy()
    for b, p in enumerate(want_p):
        if p < 0:
            assert np.array_equal(got_xu[b].view(np.uint32), xu0[b].view(np.uint32)) and got_ref[b].view(np.uint32) == ref0[b].view(np.uint32)
        else:
            want = (xu0[b] + np.float32(steps[p]) * dz[b]).astype(np.float32)          # power-of-two step: the product is exact, one rounding
            assert np.array_equal(got_xu[b].view(np.uint32), want.view(np.uint32)), b
            assert got_ref[b].view(np.uint32) == merit[b, p].view(np.uint32)


def test_accepted_merit_is_the_merit_of_the_new_iterate(env):
    """After an accepted step, compute_merit with step size 0 on the new xu equals d_merit_ref bit for bit: the step kernel stores the float the merit
    kernel evaluated."""
    PcgSolver, plant, _, _ = env
    N, B = 8, 3
    xu, goals, xs, dz, _ = case(N, B)
    sol = PcgSolver(N, max_batch=B)
    d_xu, d_dz = dev(xu), dev(dz)
    args = (plant, dev(goals.reshape(B, -1)), dev(xs))
    tail = (iiwa.TIMESTEP, MU, iiwa.QD_COST, iiwa.r_cost(N))
    merit = sol.compute_merit(*args, d_xu, d_dz, STEPS8, *tail)
    ref = torch.full((B,), float("inf"), device="cuda")                   # anything is better: every trajectory steps
    step = sol.line_search_step(merit, STEPS8, ref, d_dz, d_xu)
    again = sol.compute_merit(*args, d_xu, None, [0.0], *tail)
    torch.cuda.synchronize()
    assert (step.cpu().numpy() >= 0).all()
    assert np.array_equal(again.cpu().numpy()[:, 0].view(np.uint32), ref.cpu().numpy().view(np.uint32))
    assert np.array_equal(ref.cpu().numpy(), merit.cpu().numpy().min(axis=1))


@pytest.mark.parametrize("N,B,seed", [(8, 3, 19), (32, 2, 43)])
def test_closed_loop_sqp_on_the_device(env, N, B, seed):
    """Four SQP iterations on the device: KKT -> Schur (SS) -> PCG -> dz -> merit at eight steps -> step, rho = 1e-3, mu = 10; merit_ref evaluated at the
    first iterate and carried.  After each iteration the host restates the eight merits on the downloaded xu, dz and makes its own choice; a
    (trajectory, iteration) pair is compared unless the host's best and second-best merits, or its best and merit_ref, are closer than
    1e-5 max(1, |merit|) — ten times the limit of the restatement test — and at most 20 % of the pairs may be left out.  Every trajectory's final
    merit_ref is below its first.  Measured: all 12 + 8 pairs compared, none left out; merit 20.5 / 3.29 / 1.12 -> 0.30 / 0.67 / 0.63 and 3.98 / 8.42 -> 2.32 / 1.79."""
    PcgSolver, plant, pcg_config, M = env
    xu, goals, xs = iiwa.random_windows(N, B, seed)
    r = iiwa.r_cost(N)
    sol = PcgSolver(N, max_batch=B)
    d_goals, d_xs, d_xu = dev(goals.reshape(B, -1)), dev(xs), dev(xu)
    lam = torch.zeros(B, n * N, device="cuda")
    tail = (iiwa.TIMESTEP, MU, iiwa.QD_COST, r)
    d_ref = sol.compute_merit(plant, d_goals, d_xs, d_xu, None, [0.0], *tail).reshape(B).clone()
    first = d_ref.cpu().numpy().copy()
    host_ref = P.merits(M, d_xu.cpu().numpy(), None, [0.0], P.f32(goals), P.f32(xs), N, MU, cost=P.Cost.plain(iiwa.QD_COST, r))[:, 0]
    assert (np.abs(first - host_ref) <= 1e-6 * np.maximum(1.0, np.abs(host_ref))).all()
    compared = skipped = 0
    for it in range(4):
        G, Cd, g, c = sol.generate_kkt(plant, d_goals, d_xs, d_xu, iiwa.TIMESTEP, iiwa.QD_COST, r)
        S, Pinv, gam = sol.form_schur(G, Cd, g, c, 1e-3, "ss")
        sol.solve(S, Pinv, gam, lam, pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=3000), "ss")
        dz = sol.compute_dz(G, Cd, g, lam)
        merit = sol.compute_merit(plant, d_goals, d_xs, d_xu, dz, STEPS8, *tail)
        xu_before = d_xu.cpu().numpy()
        step = sol.line_search_step(merit, STEPS8, d_ref, dz, d_xu)
        torch.cuda.synchronize()
        step = step.cpu().numpy()
        host = P.merits(M, xu_before, dz.cpu().numpy(), STEPS8, P.f32(goals), P.f32(xs), N, MU, cost=P.Cost.plain(iiwa.QD_COST, r))
        assert (np.abs(merit.cpu().numpy() - host) <= 1e-6 * np.maximum(1.0, np.abs(host))).all()
        for b in range(B):
            p, best = P.select(host[b], host_ref[b])
            order = np.sort(np.append(host[b], host_ref[b]))
            gap = order[1] - order[0]                          # best against the runner-up, merit_ref among them
            if gap < 1e-5 * max(1.0, abs(order[0])):
                skipped += 1
            else:
                compared += 1
                assert step[b] == p, (it, b, step[b], p, host[b], host_ref[b])
            if step[b] >= 0:
                host_ref[b] = host[b, step[b]]                 # (follow the device's iterate: the next restatement starts from its xu)
    print(f"N={N} B={B}: compared {compared}, left out {skipped}, merit {first} -> {d_ref.cpu().numpy()}")
    assert skipped <= 0.2 * (compared + skipped)
    assert (d_ref.cpu().numpy() < first).all()


def test_merit_and_step_replay_from_a_hipgraph(env):
    """Both calls are pure stream work after the first compute_merit has allocated the handle's scratch: captured with torch.cuda.graph after one eager
    call, a replay gives the eager results bit for bit.  A FIRST compute_merit on a capturing stream of a fresh handle is refused with a message and
    leaves the capture usable."""
    PcgSolver, plant, _, _ = env
    N, B = 8, 3
    xu, goals, xs, dz, _ = case(N, B)
    d_goals, d_xs, d_dz = dev(goals.reshape(B, -1)), dev(xs), dev(dz)
    tail = (iiwa.TIMESTEP, MU, iiwa.QD_COST, iiwa.r_cost(N))
    xu_in = dev(xu)
    ref_in = torch.tensor([1e9, 0.0, 1e9], device="cuda")             # trajectory 1 takes no step
    sol = PcgSolver(N, max_batch=B)
    e_xu, e_ref = xu_in.clone(), ref_in.clone()
    e_merit = sol.compute_merit(plant, d_goals, d_xs, e_xu, d_dz, STEPS8, *tail)
    e_step = sol.line_search_step(e_merit, STEPS8, e_ref, d_dz, e_xu)
    torch.cuda.synchronize()
    assert e_step.cpu().numpy()[1] == -1 and (e_step.cpu().numpy()[[0, 2]] >= 0).all()

    g_xu, g_ref = torch.empty_like(xu_in), torch.empty_like(ref_in)
    g_merit = torch.zeros(B, 8, device="cuda")
    g_step = torch.zeros(B, dtype=torch.int32, device="cuda")
    fresh = PcgSolver(N, max_batch=B)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="outside the stream capture") as ei:
            fresh.compute_merit(plant, d_goals, d_xs, xu_in, d_dz, STEPS8, *tail, merit=g_merit)
        assert ei.value.code == _lib.MPCG_ERR_INVALID
        g_xu.copy_(xu_in)
        g_ref.copy_(ref_in)
        sol.compute_merit(plant, d_goals, d_xs, g_xu, d_dz, STEPS8, *tail, merit=g_merit)
        sol.line_search_step(g_merit, STEPS8, g_ref, d_dz, g_xu, step=g_step)
    for _ in range(2):
        g_merit.zero_(); g_step.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in ((g_merit, e_merit), (g_xu, e_xu), (g_ref, e_ref)):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
        assert torch.equal(g_step, e_step)


def test_argument_errors(env):
    """Every row of the table in include/mpcg.h's description of the two calls."""
    PcgSolver, plant, _, _ = env
    lib = _lib.load()
    N, B = 4, 2
    sol = PcgSolver(N, max_batch=B)
    L = (n + m) * N - m
    goals, xs, xu, dz = (torch.zeros(B, k, device="cuda") for k in (6 * N, n, L, L))
    merit, ref = torch.zeros(B, 16, device="cuda"), torch.zeros(B, device="cuda")
    step = torch.zeros(B, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    arr = lambda v: (C.c_float * len(v))(*v)

    def cm(h=sol._h, pl=plant._p, cs=7, goals=goals, xs=xs, xu=xu, dz=dz, steps=arr([0.0, -1.0]), A=2, merit=merit, batch=B):
        return lib.mpcg_compute_merit(h, pl, cs, 1 / 64, p(goals), p(xs), p(xu), p(dz), steps, A, 10.0, 1e-4, 1e-4, p(merit), batch, None)

    def ls(h=sol._h, cs=7, merit=merit, steps=arr([-1.0, -0.5]), A=2, ref=ref, dz=dz, xu=xu, step=step, batch=B):
        return lib.mpcg_line_search_step(h, cs, p(merit), steps, A, p(ref), p(dz), p(xu), p(step), batch, None)

    INV, UNS, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_ERR_UNSUPPORTED, _lib.MPCG_OK
    assert cm() == OK and ls() == OK
    assert cm(xs=None) == OK                                                 # d_xs may be NULL
    assert cm(dz=None, steps=arr([0.0, -0.0])) == OK                         # d_dz may be NULL if every step size is 0
    # null required pointers
    assert cm(h=None) == INV and cm(pl=None) == INV
    for kw in ("goals", "xu", "merit", "steps"):
        assert cm(**{kw: None}) == INV, kw
    assert ls(h=None) == INV
    for kw in ("merit", "steps", "ref", "dz", "xu", "step"):
        assert ls(**{kw: None}) == INV, kw
    # num_steps 0 or > 16
    big = arr([-1.0] * 17)
    assert cm(A=0) == INV and cm(steps=big, A=17) == INV and ls(A=0) == INV and ls(steps=big, A=17) == INV
    assert cm(steps=arr([-1.0] * 16), A=16) == OK
    # batch
    assert cm(batch=B + 1) == INV and ls(batch=B + 1) == INV
    assert b"max_batch" in lib.mpcg_last_error(sol._h)
    assert cm(batch=0) == OK and ls(batch=0) == OK
    # d_dz == NULL with a non-zero step size
    assert cm(dz=None) == INV
    # control_size of the step: 1 .. state_size
    assert ls(cs=0) == INV and ls(cs=15) == INV
    # compute_merit on anything but 14 x 7
    assert cm(cs=6) == UNS
    small = PcgSolver(N, max_batch=B, state_size=6, control_size=3)
    assert cm(h=small._h, cs=3) == UNS and cm(h=small._h) == UNS
    # a plant on another device: the handle compares the plant's device with its own before anything touches either (the first member of the
    # opaque mpcg_plant is its device index; a machine with one GPU cannot make a real plant elsewhere)
    dev_field = C.cast(plant._p, C.POINTER(C.c_int))
    own = dev_field[0]
    assert own == sol.device
    dev_field[0] = own + 1
    try:
        assert cm() == INV
        assert b"different devices" in lib.mpcg_last_error(sol._h)
    finally:
        dev_field[0] = own
    assert cm() == OK
    torch.cuda.synchronize()


def test_batched_sqp_example():
    """examples/sqp_batched_iiwa: B windows of the reference trajectory, K SQP iterations entirely on the device; exits 0 only if every trajectory's
    merit went down."""
    from mpcgpu_amd import build
    exe = build.build_sqp_batched()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["batch"] == 8 and out["knots"] == 32 and out["iters"] == 4
    merit = np.array(out["merit"])                         # [batch][iters + 1]
    assert merit.shape == (8, 5) and (merit[:, -1] < merit[:, 0]).all() and (np.diff(merit, axis=1) <= 0).all()
    assert np.array(out["exponents"]).shape == (8, 4)


def test_line_search_stage_of_the_shim():
    """mpcgpu_compat::use_mpcg_line_search<float> (include/mpcgpu_compat/sqp_stages.cuh): sqpSolvePcg over the shim headers with the library's KKT and
    line-search stages, four SQP iterations on a perturbed window of the reference trajectory; the merit of the iterate goes down."""
    from mpcgpu_amd import build
    exe = build.build_line_search_stage()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"] is True and out["sqp_iterations"] == 4 and out["merit_after"] < out["merit_before"]
