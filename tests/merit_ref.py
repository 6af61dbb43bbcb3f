"""Float64 restatement of the merit function of the SQP line search (ls_gato_compute_merit / compute_merit, reference
include/common/merit.cuh:16-143) and of its step selection (include/pcg/sqp.cuh:292-301) — TEST INFRASTRUCTURE, the checker of
mpcg_compute_merit / mpcg_line_search_step (mpcgpu_amd/csrc/merit_plant.hip.h).  Built from the pinned pieces of oracle/iiwa_ref.py:

    merit = sum_{k<N} J_k + mu ( sum_{k<N-1} |x_{k+1} - (x_k + dt [qd_k; qdd_k])|_1 + [xs given] |x_0 - xs|_1 )
    J_k = 1/2 |ee(q_k) - goal_k[0:3]|^2 + 1/2 qd_cost |qd_k|^2 + [k < N-1] 1/2 r_cost |u_k|^2

The last knot's cost is evaluated at its own state x_{N-1} (merit.cuh:62).  Everything is restated on the float32-rounded inputs the device sees,
and the trial iterate xu + alpha dz is formed in np.float32 first (one rounding; exact agreement with a fused multiply-add for power-of-two alpha)."""
import os

import numpy as np

import iiwa_ref

n, m = 14, 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# windows (first row, knots) of the reference's own trajectory that lie inside one segment: rows 2..65, 150..213, 300..331, 544..607
WINDOWS = ((2, 64), (150, 64), (300, 32), (544, 64))


def reference_window(t0, N):
    """(xu, goals, xs) of rows t0 .. t0 + N - 1 of the reference's 0_0 trajectory pair: goals = its own end-effector rows, xs = x_0."""
    d = np.load(os.path.join(GOLDEN, "iiwa_traj_0_0_full.npz"))
    xu = d["xu"][t0:t0 + N].reshape(-1)[:(n + m) * N - m]
    return xu, d["eepos"][t0:t0 + N], xu[:n].copy()


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def trial(xu, dz, alpha):
    """The float32 trial iterate, widened to float64."""
    xu = f32(xu)
    if alpha == 0.0 or dz is None:
        return xu.astype(np.float64)
    return (xu + np.float32(alpha) * f32(dz)).astype(np.float32).astype(np.float64)


def merit_at(model, z, goals, xs, N, mu, qd_cost, r_cost, dt=iiwa_ref.TIMESTEP):
    """Merit of ONE trajectory at the float64 iterate z [(n+m)N - m]; goals [N][6], xs [n] or None."""
    goals = f32(goals).astype(np.float64).reshape(N, 6)
    total = 0.0
    viol = 0.0
    for k in range(N):
        x = z[k * (n + m):k * (n + m) + n]
        e = model.ee_pos(x[:7]) - goals[k, :3]
        total += 0.5 * e @ e + 0.5 * qd_cost * x[7:] @ x[7:]
        if k < N - 1:
            u = z[k * (n + m) + n:(k + 1) * (n + m)]
            total += 0.5 * r_cost * u @ u
            viol += np.abs(iiwa_ref.euler_defect(model, x, u, z[(k + 1) * (n + m):(k + 1) * (n + m) + n], dt)).sum()
    if xs is not None:
        viol += np.abs(z[:n] - f32(xs).astype(np.float64)).sum()
    return total + mu * viol


def merits(model, xu, dz, step_sizes, goals, xs, N, mu, qd_cost, r_cost, dt=iiwa_ref.TIMESTEP):
    """[B, A] float64 merits of a batch: xu, dz [B, (n+m)N - m], goals [B, N, 6], xs [B, n] or None."""
    B = len(xu)
    out = np.zeros((B, len(step_sizes)))
    for b in range(B):
        for a, alpha in enumerate(step_sizes):
            out[b, a] = merit_at(model, trial(xu[b], None if dz is None else dz[b], alpha), goals[b], None if xs is None else xs[b],
                                 N, mu, qd_cost, r_cost, dt)
    return out


def select(merit_row, merit_ref):
    """include/pcg/sqp.cuh:292-301: the first strictly smallest merit below merit_ref; (-1, merit_ref) if none."""
    best, p = merit_ref, -1
    for i, v in enumerate(merit_row):
        if v < best:
            best, p = v, i
    return p, best
