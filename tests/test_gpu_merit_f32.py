"""GPU: mpcg_compute_merit with option "merit_f32" = 1 — the point merits in packed float, two work items per 16-lane group
(mpcgpu_amd/csrc/merit_plant_f32.hip.h) — against the float64 restatement tests/plant_ref.py within the limit tests/test_merit_ref_f32_cpu.py pins for
plain float arithmetic, on the reference's own trajectory, for the bit properties of the pairing, for the decisions the line search takes from it, inside
a closed device-side SQP iteration and a hipGraph; and the default build untouched by the option."""
import ctypes as C

import numpy as np
import pytest
import torch

import iiwa_ref
import plant_ref as P
import merit_ref_f32 as mf
from mpcgpu_amd import _lib, iiwa

pytestmark = pytest.mark.gpu
n, m = 14, 7
STEPS9, STEPS8, MU = mf.STEPS9, mf.STEPS8, mf.MU
TOL = 1e-5                                                    # relative to max(1, |merit|): the limit of "kkt_f32" (tests/test_gpu_kkt.py)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def env():
    from mpcgpu_amd import PcgSolver, Plant, pcg_config
    return PcgSolver, Plant(), pcg_config, iiwa_ref.Model()


def solver(PcgSolver, N, B, f32=1):
    sol = PcgSolver(N, max_batch=B)
    if f32 is not None:
        sol.set_option("merit_f32", f32)
    return sol


_want = {}


def want64(N, B, with_xs):
    """The float64 restatement's merits of mf.case_inputs(N, B) at the nine step sizes, computed once per shape."""
    if (N, B, with_xs) not in _want:
        xu, goals, xs, dz = mf.case_inputs(N, B)
        _want[(N, B, with_xs)] = P.merits(iiwa_ref.Model(), xu, dz, STEPS9, P.f32(goals), P.f32(xs if with_xs else None), N, MU, cost=P.Cost.plain(iiwa.QD_COST, iiwa.r_cost(N)))
    return _want[(N, B, with_xs)]


def call(sol, plant, N, goals, xs, xu, dz, steps, mu=MU):
    B = len(xu)
    return sol.compute_merit(plant, dev(goals.reshape(B, -1)), None if xs is None else dev(xs), dev(xu), None if dz is None else dev(dz), steps,
                             iiwa.TIMESTEP, mu, iiwa.QD_COST, iiwa.r_cost(N))


# ---- 1. against the float64 restatement ----
@pytest.mark.parametrize("with_xs", [True, False])
@pytest.mark.parametrize("N,B", mf.SHAPES)
def test_float_merit_vs_host_restatement(env, N, B, with_xs):
    """|got - want| <= 1e-5 max(1, |want|) against the FLOAT64 restatement: the five shapes and seeds of tests/test_gpu_merit.py, with and without d_xs.
    (3, 2) x 9 = 54 items leaves the last wavefront partly idle; (2, 1) x 9 pairs a dynamics item with a cost-only one in every lane group.
    The numpy float32 restatement of the same inputs is within 2.5e-6 (tests/test_merit_ref_f32_cpu.py).
    Measured worst |got - want| / max(1, |want|) on the device: NOT MEASURED yet; the test prints it per case."""
    PcgSolver, plant, _, _ = env
    xu, goals, xs, dz = mf.case_inputs(N, B)
    sol = solver(PcgSolver, N, B)
    got = call(sol, plant, N, goals, xs if with_xs else None, xu, dz, STEPS9).cpu().numpy().astype(np.float64)
    assert got.shape == (B, 9) and np.isfinite(got).all()
    w = want64(N, B, with_xs)
    err = np.abs(got - w) / np.maximum(1.0, np.abs(w))
    print(f"merit_f32 N={N} B={B} xs={with_xs}: merits {w.min():.3g} .. {w.max():.3g}, worst error {err.max():.2e}")
    assert err.max() <= TOL, (err.max(), got, w)


@pytest.mark.parametrize("N,B,A", [(2, 1, 1), (3, 1, 1), (3, 1, 9)])
def test_float_merit_smallest_and_odd_totals(env, N, B, A):
    """(2, 1) with ONE step size: two items, one lane pair, one half a dynamics item and the other cost-only — the smallest shape that can go wrong.
    (3, 1) with one step size: three items, the last half has no item; with nine: 27 items, odd again, pairs straddling step sizes.  The same limit."""
    PcgSolver, plant, _, M = env
    xu, goals, xs, dz = (a[:B] for a in mf.case_inputs(N, 1 if N == 2 else 2))
    steps = STEPS9[:A] if A > 1 else [-0.5]
    sol = solver(PcgSolver, N, B)
    got = call(sol, plant, N, goals, xs, xu, dz, steps).cpu().numpy().astype(np.float64)
    w = P.merits(M, xu, dz, steps, P.f32(goals), P.f32(xs), N, MU, cost=P.Cost.plain(iiwa.QD_COST, iiwa.r_cost(N)))
    err = np.abs(got - w) / np.maximum(1.0, np.abs(w))
    print(f"merit_f32 N={N} B={B} A={A}: worst error {err.max():.2e}")
    assert got.shape == (B, A) and err.max() <= TOL, (err.max(), got, w)


# ---- 2. the reference-trajectory pin ----
def test_float_merit_vanishes_on_the_reference_trajectory(env):
    """The windows and the bound of tests/test_merit_ref_cpu.py through the option, step size 0 and d_dz = NULL.  The numpy float32 restatement:
    9.6e-6 .. 5.0e-5 against 4.3e-4 / 8.8e-4."""
    PcgSolver, plant, _, _ = env
    for t0, N in P.WINDOWS:
        xu, goals, xs = P.reference_window(t0, N)
        sol = solver(PcgSolver, N, 1)
        got = float(sol.compute_merit(plant, dev(goals.reshape(1, -1)), dev(xs.reshape(1, -1)), dev(xu.reshape(1, -1)), None, [0.0],
                                      iiwa.TIMESTEP, 1.0, 0.0, 0.0).cpu()[0, 0])
        print(f"merit_f32 rows {t0}..{t0 + N - 1}: merit {got:.3e}, bound {14 * (N - 1) * 1e-6:.3e}")
        assert 0.0 <= got <= 14 * (N - 1) * 1e-6, (t0, got)


# ---- 3. the default is untouched ----
def test_default_build_is_untouched_by_the_option(env):
    """With the option at 0 a call's bits are those of a handle that never had it set — and those of the same handle after 1 and back to 0."""
    PcgSolver, plant, _, _ = env
    N, B = 8, 3
    xu, goals, xs, dz = mf.case_inputs(N, B)
    never = bits(call(solver(PcgSolver, N, B, None), plant, N, goals, xs, xu, dz, STEPS9))
    sol = solver(PcgSolver, N, B, 0)
    assert sol.get_option("merit_f32") == 0
    assert np.array_equal(bits(call(sol, plant, N, goals, xs, xu, dz, STEPS9)), never)
    sol.set_option("merit_f32", 1)
    on = bits(call(sol, plant, N, goals, xs, xu, dz, STEPS9))
    sol.set_option("merit_f32", 0)
    assert np.array_equal(bits(call(sol, plant, N, goals, xs, xu, dz, STEPS9)), never)
    assert not np.array_equal(on, never)                       # (the option does select another arithmetic)


# ---- 4. bit properties of the float build ----
def test_float_merit_bits(env):
    """The same call twice; a trajectory inside a batch of 7 and alone at N = 3 (27 items per trajectory: the pairing parity of every second trajectory
    differs between the two); num_steps = 1, 9 and 16 for the step sizes they share (an item moves from one half to the other and gets another
    partner): the same bits.  NaN in ONE trajectory's dz leaves every other trajectory's bits unchanged."""
    PcgSolver, plant, _, _ = env
    N, B = 3, 7
    xu, goals, xs = iiwa.random_windows(N, B, 77)
    dz = 0.05 * np.random.default_rng(78).standard_normal(xu.shape)
    sol = solver(PcgSolver, N, B)
    full = bits(call(sol, plant, N, goals, xs, xu, dz, STEPS9))
    assert np.array_equal(full, bits(call(sol, plant, N, goals, xs, xu, dz, STEPS9)))
    for b in range(B):
        alone = bits(call(sol, plant, N, goals[b:b + 1], xs[b:b + 1], xu[b:b + 1], dz[b:b + 1], STEPS9))
        assert np.array_equal(alone[0], full[b]), b
    one = bits(call(sol, plant, N, goals, xs, xu, dz, [-0.25]))
    assert np.array_equal(one[:, 0], full[:, STEPS9.index(-0.25)])
    steps16 = STEPS9 + [-0.75, 0.5, -0.3, 1e-3, -1.0, 0.0, -2.0]
    sixteen = bits(call(sol, plant, N, goals, xs, xu, dz, steps16))
    assert np.array_equal(sixteen[:, :9], full)
    assert np.array_equal(sixteen[:, 13], full[:, 1]) and np.array_equal(sixteen[:, 14], full[:, 0])      # the same step size in another slot
    bad = dz.copy()
    bad[3, 5] = np.nan                                         # q_5 of knot 0 of trajectory 3
    got = call(sol, plant, N, goals, xs, xu, bad, STEPS9).cpu().numpy()
    others = [b for b in range(B) if b != 3]
    assert np.array_equal(bits(got)[others], full[others])
    assert np.isnan(got[3, 1:]).all() and bits(got)[3, 0] == full[3, 0]          # (its own step size 0 reads no dz)


# ---- 5. the accepted merit is the merit of the new iterate ----
def test_accepted_float_merit_is_the_merit_of_the_new_iterate(env):
    """tests/test_gpu_merit.py::test_accepted_merit_is_the_merit_of_the_new_iterate with "merit_f32" = 1 for every call: the float the step kernel stores
    is the float the packed kernel evaluated, so step size 0 on the new xu gives d_merit_ref bit for bit."""
    PcgSolver, plant, _, _ = env
    N, B = 8, 3
    xu, goals, xs, dz = mf.case_inputs(N, B)
    sol = solver(PcgSolver, N, B)
    d_xu, d_dz = dev(xu), dev(dz)
    args = (plant, dev(goals.reshape(B, -1)), dev(xs))
    tail = (iiwa.TIMESTEP, MU, iiwa.QD_COST, iiwa.r_cost(N))
    merit = sol.compute_merit(*args, d_xu, d_dz, STEPS8, *tail)
    ref = torch.full((B,), float("inf"), device="cuda")
    step = sol.line_search_step(merit, STEPS8, ref, d_dz, d_xu)
    again = sol.compute_merit(*args, d_xu, None, [0.0], *tail)
    torch.cuda.synchronize()
    assert (step.cpu().numpy() >= 0).all()
    assert np.array_equal(bits(again)[:, 0], bits(ref))
    assert np.array_equal(ref.cpu().numpy(), merit.cpu().numpy().min(axis=1))


# ---- 6. decisions ----
@pytest.mark.parametrize("N,B,seed", [(8, 3, 19), (32, 2, 43)])
def test_decisions(env, N, B, seed):
    """The step mpcg_line_search_step chooses from the FLOAT merits (merit_ref = the float merit at step size 0) is plant_ref.select's on the FLOAT64
    merits, for every trajectory whose float64 candidates (merit_ref among them) are separated from the winner by more than 2e-5 max(1, |merit|) —
    twice the limit of test 1.  At most one trajectory per case may be left out; tests/test_merit_ref_f32_cpu.py checks that these seeds leave none."""
    PcgSolver, plant, _, M = env
    xu, goals, xs, dz = mf.decision_inputs(N, B, seed)
    host = P.merits(M, xu, dz, [0.0] + STEPS8, P.f32(goals), P.f32(xs), N, MU, cost=P.Cost.plain(iiwa.QD_COST, iiwa.r_cost(N)))
    sol = solver(PcgSolver, N, B)
    d_xu, d_dz = dev(xu), dev(dz)
    d_ref = call(sol, plant, N, goals, xs, xu, None, [0.0]).reshape(B).clone()
    merit = call(sol, plant, N, goals, xs, xu, dz, STEPS8)
    step = sol.line_search_step(merit, STEPS8, d_ref, d_dz, d_xu).cpu().numpy()
    left_out, chosen = 0, []
    for b in range(B):
        p, _ = P.select(host[b, 1:], host[b, 0])
        chosen.append(p)
        if mf.close_tie(host[b, 1:], host[b, 0]):
            left_out += 1
        else:
            assert step[b] == p, (b, step[b], p, host[b], merit.cpu().numpy()[b])
    print(f"merit_f32 decisions N={N} B={B}: host {chosen}, device {step.tolist()}, left out {left_out}")
    assert left_out <= 1


# ---- 7. a closed device-side SQP iteration, and the merit + step pair in a hipGraph ----
def test_closed_loop_and_graph_with_the_float_merit(env):
    """KKT -> Schur (SS, rho per trajectory) -> PCG -> dz -> merit ("merit_f32" = 1) -> step_rho, N = 8, B = 3, three iterations: everything finite, merit_ref
    non-increasing per trajectory.  Then the merit + step pair of a fourth iteration captured into a hipGraph: a replay on the same inputs gives the
    eager bits (the option is read when the call is made: the capture keeps the packed build)."""
    PcgSolver, plant, pcg_config, _ = env
    N, B = 8, 3
    xu, goals, xs = iiwa.random_windows(N, B, 19)
    r = iiwa.r_cost(N)
    sol = solver(PcgSolver, N, B)
    cfg = pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=3000)
    d_goals, d_xs, d_xu = dev(goals.reshape(B, -1)), dev(xs), dev(xu)
    lam = torch.zeros(B, n * N, device="cuda")
    tail = (iiwa.TIMESTEP, MU, iiwa.QD_COST, r)
    rho, drho = torch.full((B,), 1e-3, device="cuda"), torch.ones(B, device="cuda")
    done = torch.zeros(B, dtype=torch.uint8, device="cuda")
    d_ref = sol.compute_merit(plant, d_goals, d_xs, d_xu, None, [0.0], *tail).reshape(B).clone()
    hist = [d_ref.cpu().numpy().copy()]

    def front():
        G, Cd, g, c = sol.generate_kkt(plant, d_goals, d_xs, d_xu, iiwa.TIMESTEP, iiwa.QD_COST, r)
        S, Pinv, gam = sol.form_schur(G, Cd, g, c, rho, "ss")
        sol.solve(S, Pinv, gam, lam, cfg, "ss")
        return sol.compute_dz(G, Cd, g, lam)

    for it in range(3):
        dz = front()
        merit = sol.compute_merit(plant, d_goals, d_xs, d_xu, dz, STEPS8, *tail)
        step = sol.line_search_step_rho(merit, STEPS8, d_ref, dz, d_xu, rho, drho, done)
        torch.cuda.synchronize()
        for t in (dz, merit, d_xu, d_ref, rho, drho):
            assert torch.isfinite(t).all(), it
        hist.append(d_ref.cpu().numpy().copy())
    hist = np.array(hist)
    print(f"merit_f32 closed loop: merit_ref per iteration {hist.T.tolist()}, last steps {step.cpu().numpy().tolist()}")
    assert (np.diff(hist, axis=0) <= 0).all() and (hist[-1] < hist[0]).all()

    dz = front().clone()
    xu_in, ref_in, rho_in, drho_in = d_xu.clone(), d_ref.clone(), rho.clone(), drho.clone()
    e_xu, e_ref, e_rho, e_drho, e_done = xu_in.clone(), ref_in.clone(), rho_in.clone(), drho_in.clone(), torch.zeros_like(done)
    e_merit = sol.compute_merit(plant, d_goals, d_xs, e_xu, dz, STEPS8, *tail)
    e_step = sol.line_search_step_rho(e_merit, STEPS8, e_ref, dz, e_xu, e_rho, e_drho, e_done)
    torch.cuda.synchronize()
    g_xu, g_ref, g_rho, g_drho, g_done = (torch.empty_like(t) for t in (xu_in, ref_in, rho_in, drho_in, done))
    g_merit = torch.zeros(B, 8, device="cuda")
    g_step = torch.zeros(B, dtype=torch.int32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_xu.copy_(xu_in); g_ref.copy_(ref_in); g_rho.copy_(rho_in); g_drho.copy_(drho_in); g_done.zero_()
        sol.compute_merit(plant, d_goals, d_xs, g_xu, dz, STEPS8, *tail, merit=g_merit)
        sol.line_search_step_rho(g_merit, STEPS8, g_ref, dz, g_xu, g_rho, g_drho, g_done, step=g_step)
    sol.set_option("merit_f32", 0)                             # (the graph keeps the build it was captured with)
    for _ in range(2):
        g_merit.zero_(); g_step.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in ((g_merit, e_merit), (g_xu, e_xu), (g_ref, e_ref), (g_rho, e_rho), (g_drho, e_drho)):
            assert np.array_equal(bits(got), bits(want))
        assert torch.equal(g_step, e_step) and torch.equal(g_done, e_done)


# ---- 8. the option table ----
def test_option_table_and_argument_errors(env):
    """"merit_f32" takes 0 and 1, anything else is MPCG_ERR_INVALID and leaves the value; mpcg_get_option returns it.  The argument errors of
    mpcg_compute_merit are the same with the option on: a null d_merit, num_steps = 17, a handle that is not 14 x 7."""
    PcgSolver, plant, _, _ = env
    lib = _lib.load()
    N, B = 4, 2
    sol = PcgSolver(N, max_batch=B)
    INV, UNS, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_ERR_UNSUPPORTED, _lib.MPCG_OK
    assert sol.get_option("merit_f32") == 0
    assert lib.mpcg_set_option(sol._h, b"merit_f32", 1) == OK and sol.get_option("merit_f32") == 1
    for bad in (2, -1):
        assert lib.mpcg_set_option(sol._h, b"merit_f32", bad) == INV
        assert b"merit_f32" in lib.mpcg_last_error(sol._h) and sol.get_option("merit_f32") == 1
    assert lib.mpcg_set_option(sol._h, b"merit_f32", 0) == OK and sol.get_option("merit_f32") == 0
    sol.set_option("merit_f32", 1)
    sol.set_option("kkt_f32", 1)                               # independent of each other
    assert sol.get_option("merit_f32") == 1 and sol.get_option("kkt_f32") == 1
    sol.set_option("kkt_f32", 0)
    assert sol.get_option("merit_f32") == 1

    L = (n + m) * N - m
    goals, xs, xu, dz = (torch.zeros(B, k, device="cuda") for k in (6 * N, n, L, L))
    merit = torch.zeros(B, 16, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    arr = lambda v: (C.c_float * len(v))(*v)

    def cm(h=sol._h, cs=7, steps=arr([0.0, -1.0]), A=2, merit=merit, dz=dz, batch=B):
        return lib.mpcg_compute_merit(h, plant._p, cs, 1 / 64, p(goals), p(xs), p(xu), p(dz), steps, A, 10.0, 1e-4, 1e-4, p(merit), batch, None)

    assert cm() == OK
    assert cm(merit=None) == INV
    assert cm(steps=arr([-1.0] * 17), A=17) == INV and cm(A=0) == INV
    assert cm(steps=arr([-1.0] * 16), A=16) == OK
    assert cm(dz=None) == INV and cm(dz=None, steps=arr([0.0, -0.0])) == OK
    assert cm(batch=B + 1) == INV and cm(batch=0) == OK
    assert cm(cs=6) == UNS
    small = PcgSolver(N, max_batch=B, state_size=6, control_size=3)
    small.set_option("merit_f32", 1)
    assert cm(h=small._h, cs=3) == UNS and cm(h=small._h) == UNS
    torch.cuda.synchronize()
