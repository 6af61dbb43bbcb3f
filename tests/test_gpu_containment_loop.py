"""GPU: non-finite containment of the chain a user actually runs.  (1) Three rho-adaptive SQP iterations, float and double — the six calls of
tests/test_gpu_rho.py's loop (generate_kkt, form_schur with the rho tensor, solve, compute_dz, compute_merit, line_search_step_rho) on four
trajectories of eight knots, trajectory 2's iterate holding one NaN from the start: trajectories 0, 1 and 3 end with the bits of the clean batch,
trajectory 2 gets step -1 every iteration ("a NaN never wins") and its rho follows the no-step rule of include/mpcg.h until the solve is given
up.  (2) Two control updates of the closed loop of examples/mpc_closed_loop (one SQP iteration, simulate under the previous plan,
advance_horizon), float, one trajectory's plant state NaN.  Bit patterns only (tests/containment.py)."""
import numpy as np
import pytest
import torch

import containment as ct
import rho_ref
from mpcgpu_amd import _lib, iiwa
from test_gpu_rho import MU, STEPS8

pytestmark = pytest.mark.gpu
n, m, N, B = 14, 7, 8, 4
L = (n + m) * N - m
BAD = 2
RHO0 = [1e-3, 5.0, 4.0, 0.1]
RESET = 2e-3
MAX_ITER = 12
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()


def windows(dtype):
    xu, goals, xs = iiwa.random_windows(N, B, 19)
    return tuple(np.ascontiguousarray(a, dtype) for a in (xu, goals.reshape(B, -1), xs))


class Loop:
    """A batched adaptive SQP loop on one handle: the state and the six calls of tests/test_gpu_rho.py::Loop, in the dtype of its arrays."""

    def __init__(self, dtype, xu, goals, xs):
        from mpcgpu_amd import PcgSolver, Plant, pcg_config
        dt = TORCH[dtype]
        self.sol, self.plant = PcgSolver(N, max_batch=B), Plant()
        self.cfg = pcg_config(pcg_exit_tol=1e-7, pcg_max_iter=MAX_ITER)
        self.solve = self.sol.solve if dtype == np.float32 else self.sol.solve_f64
        self.goals, self.xs, self.xu = dev(goals), dev(xs), dev(xu)
        self.lam = torch.zeros(B, n * N, device="cuda", dtype=dt)
        self.tail = (iiwa.TIMESTEP, MU, iiwa.QD_COST, iiwa.r_cost(N))
        self.rho = torch.tensor(RHO0, dtype=dt, device="cuda")
        self.drho = torch.ones(B, device="cuda", dtype=dt)
        self.done = torch.zeros(B, dtype=torch.uint8, device="cuda")
        self.step = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.start_merit()

    def start_merit(self):
        self.ref = self.sol.compute_merit(self.plant, self.goals, self.xs, self.xu, None, [0.0], *self.tail).reshape(B).clone()

    def iteration(self):
        s = self.sol
        G, Cd, g, c = s.generate_kkt(self.plant, self.goals, self.xs, self.xu, iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(N))
        S, Pinv, gam = s.form_schur(G, Cd, g, c, self.rho, "ss")
        self.its, self.exits = self.solve(S, Pinv, gam, self.lam, self.cfg, "ss")
        dz = s.compute_dz(G, Cd, g, self.lam)
        merit = s.compute_merit(self.plant, self.goals, self.xs, self.xu, dz, STEPS8, *self.tail)
        s.line_search_step_rho(merit, STEPS8, self.ref, dz, self.xu, self.rho, self.drho, self.done, rho_reset=RESET, step=self.step)

    def state(self, names=("xu", "rho", "drho", "done", "ref", "step")):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy().copy() for k in names}


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_three_adaptive_sqp_iterations_with_a_nan_in_one_iterate(dtype):
    xu, goals, xs = windows(dtype)
    bad = ct.poison(xu, (BAD,), lambda a: ct.nan_one(a, (n + m) * 3 + 2))            # q_2 of knot 3
    clean, poisoned = Loop(dtype, xu, goals, xs), Loop(dtype, bad, goals, xs)
    rho, drho, done = dtype(RHO0[BAD]), dtype(1.0), False
    for it in range(3):
        clean.iteration()
        poisoned.iteration()
        want, got = clean.state(), poisoned.state()
        ct.check(want, got, (BAD,), entry=f"adaptive SQP iteration {it} {np.dtype(dtype).name}")
        # the poisoned trajectory: no step ever — its merits are NaN and so is its reference merit —, rho by the no-step rule until the solve is given up
        if done:
            assert got["step"][BAD] == _lib.MPCG_STEP_FROZEN
        else:
            assert got["step"][BAD] == -1, (it, got["step"])
            rho, drho, done = rho_ref.update(rho, drho, -1, rho_reset=RESET, dtype=dtype)
        assert got["rho"][BAD].tobytes() == dtype(rho).tobytes() and got["drho"][BAD].tobytes() == dtype(drho).tobytes(), (it, got["rho"], rho, got["drho"], drho)
        assert int(got["done"][BAD]) == int(done), (it, got["done"])
        assert np.array_equal(got["xu"][BAD].view(np.uint8), bad[BAD].view(np.uint8)) and np.isnan(got["ref"][BAD])
        it_, ex_ = poisoned.its.cpu().numpy(), poisoned.exits.cpu().numpy()
        assert 0 <= it_[BAD] <= MAX_ITER and ex_[BAD] in (0, 1)
    assert done and rho == dtype(RESET)                      # 4 x 1.2, x 1.44, x 1.728 = 11.9 > 10: given up in the third iteration
    assert (want["step"][[0, 1, 3]] >= -1).all() and want["done"][[0, 1, 3]].tolist() == [0, 0, 0]


def test_two_control_updates_of_the_closed_loop_with_a_nan_plant_state():
    """Per update: the merit of the start iterate and one SQP iteration, the plant simulated for one knot's time under the PREVIOUS plan, the
    horizon shifted (a plan per trajectory).  Trajectory 2's measured state is NaN from the start; the others' xs, xu, lambda, goals, offsets,
    done flags and tracking errors are the clean run's after each update."""
    dtype = np.float32
    xu, goals, xs = windows(dtype)
    rng = np.random.default_rng(23)
    T = N + 6
    plan, plan_goals = (0.3 * rng.standard_normal((B, T, n + m))).astype(dtype), (0.3 * rng.standard_normal((B, T, 6))).astype(dtype)
    period_us = iiwa.TIMESTEP * 1e6
    runs = []
    for xs0 in (xs, ct.poison(xs, (BAD,), ct.nan_all)):
        loop = Loop(dtype, xu, goals, xs0)
        loop.xu_old = loop.xu.clone()
        loop.eePos = torch.full((B, 3), float("nan"), device="cuda")
        loop.err = torch.full((B,), float("nan"), device="cuda")
        loop.offset = dev(np.array([0, 1, 2, 3], np.int32))
        loop.mpc_done = torch.zeros(B, dtype=torch.int32, device="cuda")
        d_plan, d_plan_goals = dev(plan), dev(plan_goals)
        states, prev_us = [], 0.0
        for u in range(2):
            loop.drho.fill_(1.0)
            loop.done.zero_()
            loop.start_merit()
            loop.iteration()
            loop.sol.simulate(loop.plant, loop.xs, loop.xu_old, iiwa.TIMESTEP, prev_us, period_us, float(np.float32(2e-4)), eePos=loop.eePos)
            loop.xu_old.copy_(loop.xu)
            loop.sol.advance_horizon(True, loop.xu, loop.xs, loop.lam, loop.goals, loop.eePos, d_plan, d_plan_goals, loop.offset, loop.mpc_done, loop.err)
            prev_us = period_us
            states.append(loop.state(("xs", "xu", "lam", "goals", "offset", "mpc_done", "err", "eePos", "rho", "drho", "ref", "step")))
        runs.append(states)
    for u, (want, got) in enumerate(zip(*runs)):
        ct.check(want, got, (BAD,), entry=f"control update {u}")
        assert want["offset"].tolist() == [u + 1, u + 2, u + 3, u + 4] and np.isfinite(want["err"]).all() and np.isfinite(want["xs"]).all()
        assert np.isnan(got["xs"][BAD]).all() and got["offset"][BAD] == u + 3          # (the integer bookkeeping of the poisoned trajectory goes on)
