"""Float64 restatement of the generalised running cost of mpcg_generate_kkt_xuref / mpcg_compute_merit_xuref (include/mpcg.h; the joint-space plant of
the reference, include/dynamics/iiwa/iiwa_plant.cuh:300-323, next to the end-effector one) — TEST INFRASTRUCTURE, written from the formulas:

    J_k = 1/2 ee_cost |ee(q_k) - goal_k[0:3]|^2 + 1/2 q_cost |q_k - q_ref|^2 + 1/2 qd_cost |qd_k - [QD_REL] qd_ref|^2 + [k < N-1] 1/2 r_cost |u_k - [U_REL] u_ref|^2
    [q_ref, qd_ref, u_ref] = plan_b[row(b, k)],   row(b, k) = clamp(off_b + k, 0, traj_steps - 1),   plan_b = plan rows from b * traj_batch_stride

The dynamics (C, c) and the end-effector parts gq = J^T (ee - goal) are those of oracle/iiwa_ref.py (tests/integrator_ref.py for the semi-implicit
integrator); G and g are recomposed here.  The merit is tests/merit_ref.py's with J_k above, every knot at its own state against its own row."""
from dataclasses import dataclass

import numpy as np

import iiwa_ref
import integrator_ref
import merit_ref
import merit_ref_f64

NJ = 7
n, m = 14, 7
ROW = n + m
QD_RELATIVE, U_RELATIVE = 1, 2


@dataclass(frozen=True)
class Cost:
    ee_cost: float = 1.0
    q_cost: float = 0.0
    qd_cost: float = iiwa_ref.QD_COST
    r_cost: float = 1e-4
    flags: int = 0

    @property
    def qd_rel(self):
        return 1.0 if self.flags & QD_RELATIVE else 0.0

    @property
    def u_rel(self):
        return 1.0 if self.flags & U_RELATIVE else 0.0


def row_index(off, k, traj_steps):
    """row(b, k) in Python integers (no 32-bit wrap)."""
    return min(max(int(off) + int(k), 0), int(traj_steps) - 1)


def plan_rows(plan, b, off, N, traj_steps, stride=0):
    """[N, 21]: the reference rows of trajectory b's knots.  plan: [rows, 21] (flattened plans); stride 0: one plan shared by the batch."""
    plan = np.asarray(plan, np.float64).reshape(-1, ROW)
    base = int(b) * int(stride)
    return np.stack([plan[base + row_index(off, k, traj_steps)] for k in range(N)])


def split(z, N):
    """(x [N, 14], u [N-1, 7]) of one trajectory's xu."""
    z = np.asarray(z, np.float64)
    x = np.stack([z[k * ROW:k * ROW + n] for k in range(N)])
    u = np.stack([z[k * ROW + n:(k + 1) * ROW] for k in range(N - 1)]) if N > 1 else np.zeros((0, m))
    return x, u


def joint_cost(z, rows, N, cost):
    """sum_k of the joint-space terms of J_k (everything but the end-effector term) at the iterate z."""
    x, u = split(z, N)
    total = 0.0
    for k in range(N):
        dq = x[k, :NJ] - rows[k, :NJ]
        dqd = x[k, NJ:] - cost.qd_rel * rows[k, NJ:n]
        total += 0.5 * cost.q_cost * dq @ dq + 0.5 * cost.qd_cost * dqd @ dqd
        if k < N - 1:
            du = u[k] - cost.u_rel * rows[k, n:]
            total += 0.5 * cost.r_cost * du @ du
    return total


def ee_cost_sum(model, z, goals, N):
    """sum_k 1/2 |ee(q_k) - goal_k[0:3]|^2, every knot at its own state (the merit's view)."""
    x, _ = split(z, N)
    goals = np.asarray(goals, np.float64).reshape(N, 6)
    total = 0.0
    for k in range(N):
        e = model.ee_pos(x[k, :NJ]) - goals[k, :3]
        total += 0.5 * e @ e
    return total


def dynamics(model, xu, goals, xs, N, dt=iiwa_ref.TIMESTEP, integrator=0):
    """What does not depend on the cost's weights or on the plan: (C, g0, c) of iiwa_ref.generate_kkt — the slow part, shared by a test's cost settings."""
    _, C, g0, c = integrator_ref.generate_kkt(model, np.asarray(xu, np.float64), np.asarray(goals, np.float64).reshape(N, 6), np.asarray(xs, np.float64), N, dt, integrator)
    return C, g0, c


def generate_kkt(model, xu, goals, xs, N, rows, cost, dt=iiwa_ref.TIMESTEP, integrator=0, base=None):
    """(G, C, g, c) of ONE trajectory in iiwa_ref.generate_kkt's layouts.  goals None: ee_cost must be 0.  rows: plan_rows(...).  base: dynamics(...) of the
    same xu, xs, dt and integrator (and of the same goals unless ee_cost is 0), if the caller has it."""
    xu = np.asarray(xu, np.float64)
    if goals is None:
        assert cost.ee_cost == 0.0
        goals = np.zeros((N, 6))
    C, g0, c = base if base is not None else dynamics(model, xu, goals, xs, N, dt, integrator)
    x, u = split(xu, N)
    G = np.zeros((n * n + m * m) * N - m * m)
    g = np.zeros(ROW * N - m)

    def block(gq, xk, ref):
        Q = np.zeros((n, n))
        Q[:NJ, :NJ] = cost.ee_cost * np.outer(gq, gq) + cost.q_cost * np.eye(NJ)
        Q[NJ:, NJ:] = cost.qd_cost * np.eye(NJ)
        q = np.concatenate([cost.ee_cost * gq + cost.q_cost * (xk[:NJ] - ref[:NJ]), cost.qd_cost * (xk[NJ:] - cost.qd_rel * ref[NJ:n])])
        return Q, q

    for k in range(N - 1):
        Q, q = block(g0[ROW * k:ROW * k + NJ], x[k], rows[k])          # the q part of iiwa_ref's q_k is gq itself
        o = (n * n + m * m) * k
        G[o:o + n * n] = Q.T.reshape(-1)
        G[o + n * n:o + n * n + m * m] = (cost.r_cost * np.eye(m)).reshape(-1)
        g[ROW * k:ROW * k + n] = q
        g[ROW * k + n:ROW * (k + 1)] = cost.r_cost * (u[k] - cost.u_rel * rows[k, n:])
    # last block: the end-effector part is iiwa_ref's (the pose of x_{N-2} against goal_{N-1}); the joint-space terms at x_{N-1} against row(b, N-1)
    Q, q = block(g0[ROW * (N - 1):ROW * (N - 1) + NJ], x[N - 1], rows[N - 1])
    G[(n * n + m * m) * (N - 1):] = Q.T.reshape(-1)
    g[ROW * (N - 1):] = q
    return G, C, g, c


def merit_at(model, z, goals, xs, N, mu, rows, cost, dt=iiwa_ref.TIMESTEP, integrator=0):
    """Merit of ONE trajectory at the float64 iterate z: merit_ref.merit_at's violation terms, J_k above."""
    z = np.asarray(z, np.float64)
    total = joint_cost(z, rows, N, cost)
    if goals is not None:
        total += cost.ee_cost * ee_cost_sum(model, z, goals, N)
    else:
        assert cost.ee_cost == 0.0
    viol = 0.0
    for k in range(N - 1):
        viol += np.abs(integrator_ref.defect(model, z[k * ROW:k * ROW + n], z[k * ROW + n:(k + 1) * ROW], z[(k + 1) * ROW:(k + 1) * ROW + n], dt, integrator)).sum()
    if xs is not None:
        viol += np.abs(z[:n] - np.asarray(xs, np.float64)).sum()
    return total + mu * viol


def merits(model, xu, dz, step_sizes, goals, xs, N, mu, rows_of, cost, dt=iiwa_ref.TIMESTEP, integrator=0, double=False):
    """[B, A] float64 merits: the float trial iterate of merit_ref.trial, or (double) merit_ref_f64.trial's.  rows_of(b) -> [N, 21].  Inputs are
    used as the numbers they are (a float test passes float32-rounded arrays)."""
    trial = merit_ref_f64.trial if double else merit_ref.trial
    out = np.zeros((len(xu), len(step_sizes)))
    for b in range(len(xu)):
        for a, alpha in enumerate(step_sizes):
            out[b, a] = merit_at(model, trial(xu[b], None if dz is None else dz[b], alpha), None if goals is None else np.asarray(goals[b], np.float64),
                                 None if xs is None else xs[b], N, mu, rows_of(b), cost, dt, integrator)
    return out
