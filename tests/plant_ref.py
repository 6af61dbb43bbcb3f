"""Float64 restatement of the plant stages of one MPC step — TEST INFRASTRUCTURE, the checker of the KKT, merit and simulate kernels
(mpcgpu_amd/csrc/kkt_plant.hip.h, merit_plant.hip.h, merit_plant_f32.hip.h, sim_plant.hip.h).  One function per stage; precision, integrator, cost
and limits are arguments.  Built on the pinned pieces of oracle/iiwa_ref.py::Model (ee_pos, rnea, mass_matrix, forward_dynamics_and_gradient), so it
serves tests/chain_models.py::Chain and tests/gravity_ref.py's models too.

    trial      the trial iterate xu + alpha dz of the line search: the float32 sum rounded once and widened, or (double) the exactly rounded fma
    step       integrator 0, explicit Euler:       q' = q + dt qd;   qd' = qd + dt qdd            qdd = FD(q, qd, u) (include/common/integrator.cuh)
               integrator 1, semi-implicit Euler:  qd' = qd + dt qdd;  q' = q + dt qd'
    defect     x_{k+1} - step(x_k, u_k)
    AB         the Jacobians of step: I + dt [[0, I], [dqdd/dq, dqdd/dqd]], [0; dt Minv] for integrator 0;
               I + dt [[dt dqdd/dq, I + dt dqdd/dqd], [dqdd/dq, dqdd/dqd]], [dt^2 Minv; dt Minv] for integrator 1
    J_k        1/2 ee_cost |ee(q_k) - goal_k[0:3]|^2 + 1/2 q_cost |q_k - q_ref|^2 + 1/2 qd_cost |qd_k - [QD_REL] qd_ref|^2
               + [k < N-1] 1/2 r_cost |u_k - [U_REL] u_ref|^2                                      [q_ref, qd_ref, u_ref] = plan_b[row(b, k)]
               + 1/2 q_weight sum_i viol(q_i)^2 + 1/2 qd_weight sum_i viol(qd_i)^2 + [k < N-1] 1/2 u_weight sum_i viol(u_i)^2        (Limits)
               row(b, k) = clamp(off_b + k, 0, traj_steps - 1);  viol(x; lo, hi) = x > hi ? x - hi : (x < lo ? x - lo : 0), strict comparisons
    KKT        cost = None is the plain entry, mpcg_generate_kkt: iiwa_ref.generate_kkt's arrays, whose last block is the cost of knot N-1
               evaluated at x_{N-2} (the reference's quirk, include/common/kkt.cuh).  A Cost is the _xuref entry: the end-effector part of the last
               block is still the pose of x_{N-2} against goal_{N-1}, the joint-space terms are at x_{N-1} against row(b, N-1) — so
               Cost.plain(...) differs from cost = None in the seven qd entries of q_{N-1}: qd_cost qd_{N-1}, not qd_cost qd_{N-2}.
    merit      sum_{k<N} J_k + mu ( sum_{k<N-1} |defect_k|_1 + [xs given] |x_0 - xs|_1 ), every knot at its own state (include/common/merit.cuh)
    schedule, simulate   the substeps of simple_simulate (integrator.cuh:301-324), the state carried in float64
    tracking_error, advance   the horizon shift of simulateMPC (include/mpcsim.cuh:300-348): copies only

Inputs are used as the numbers they are: a test of a float entry rounds what the device sees in float with f32(...) where it calls."""
import math
import os
from dataclasses import dataclass

import numpy as np

import iiwa_ref
from rho_ref import fma

NJ = 7
n, m = 14, 7
ROW = n + m
QD_RELATIVE, U_RELATIVE = 1, 2
SIM_STEP = 2e-4                          # integrator.cuh:304; the float entries round it to float
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# windows (first row, knots) of the reference's own trajectory that lie inside one segment: rows 2..65, 150..213, 300..331, 544..607
WINDOWS = ((2, 64), (150, 64), (300, 32), (544, 64))


def reference_window(t0, N):
    """(xu, goals, xs) of rows t0 .. t0 + N - 1 of the reference's 0_0 trajectory pair: goals = its own end-effector rows, xs = x_0."""
    d = np.load(os.path.join(GOLDEN, "iiwa_traj_0_0_full.npz"))
    xu = d["xu"][t0:t0 + N].reshape(-1)[:ROW * N - m]
    return xu, d["eepos"][t0:t0 + N], xu[:n].copy()


def f32(a):
    """What a float entry sees of a (None stays None)."""
    return None if a is None else np.ascontiguousarray(a, np.float32)


# ---- cost, plan rows, limits ----
@dataclass(frozen=True)
class Cost:
    ee_cost: float = 1.0
    q_cost: float = 0.0
    qd_cost: float = iiwa_ref.QD_COST
    r_cost: float = 1e-4
    flags: int = 0

    @classmethod
    def plain(cls, qd_cost, r_cost):
        """The end-effector cost of the entries without xu_ref; it needs no plan rows."""
        return cls(1.0, 0.0, qd_cost, r_cost, 0)

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


def _seven(v, default):
    a = np.full(NJ, default, np.float64) if v is None else np.broadcast_to(np.asarray(v, np.float64), (NJ,)).copy()
    a.setflags(write=False)
    return a


@dataclass(frozen=True)
class Limits:
    """Bounds per joint ([7] each; None: no bound on that side) and one weight per kind."""
    q_lo: np.ndarray = None
    q_hi: np.ndarray = None
    qd_lo: np.ndarray = None
    qd_hi: np.ndarray = None
    u_lo: np.ndarray = None
    u_hi: np.ndarray = None
    q_weight: float = 0.0
    qd_weight: float = 0.0
    u_weight: float = 0.0

    def __post_init__(self):
        for name in ("q", "qd", "u"):
            object.__setattr__(self, name + "_lo", _seven(getattr(self, name + "_lo"), -np.inf))
            object.__setattr__(self, name + "_hi", _seven(getattr(self, name + "_hi"), np.inf))

    @property
    def x_lo(self):
        return np.concatenate([self.q_lo, self.qd_lo])

    @property
    def x_hi(self):
        return np.concatenate([self.q_hi, self.qd_hi])

    @property
    def x_weight(self):
        return np.concatenate([np.full(NJ, self.q_weight), np.full(NJ, self.qd_weight)])

    def rounded_to_float(self):
        """The limits the float builds ("kkt_f32", "merit_f32") use: bounds and weights rounded to float."""
        f = lambda a: np.asarray(a, np.float32).astype(np.float64)
        return Limits(f(self.q_lo), f(self.q_hi), f(self.qd_lo), f(self.qd_hi), f(self.u_lo), f(self.u_hi), float(np.float32(self.q_weight)),
                      float(np.float32(self.qd_weight)), float(np.float32(self.u_weight)))


def viol(x, lo, hi):
    """viol(x; lo, hi), elementwise; strict comparisons (NaN -> 0)."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x > hi, x - hi, np.where(x < lo, x - lo, 0.0))


def side(x, lo, hi):
    """-1 below, 0 inside (or on a bound), +1 above."""
    x = np.asarray(x, np.float64)
    return np.where(x > hi, 1, np.where(x < lo, -1, 0))


# ---- the three parts of sum_k J_k ----
def joint_cost(z, rows, N, cost):
    """sum_k of the joint-space terms of J_k (everything but the end-effector term and the limits) at the iterate z.  rows None: no plan (zeros)."""
    x, u = split(z, N)
    rows = np.zeros((N, ROW)) if rows is None else rows
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


def penalty(z, N, lim):
    """sum_k of the limits terms of J_k at the iterate z of one trajectory."""
    x, u = split(z, N)
    vx = viol(x, lim.x_lo, lim.x_hi)
    total = 0.5 * (lim.x_weight * vx * vx).sum()
    if N > 1:
        vu = viol(u, lim.u_lo, lim.u_hi)
        total += 0.5 * lim.u_weight * (vu * vu).sum()
    return total


# ---- the trial iterate ----
def trial(xu, dz, alpha, double=False):
    """xu + alpha dz as float64: the float32 sum rounded once (exact agreement with a fused multiply-add for power-of-two alpha) and widened, or
    (double) the correctly rounded fma(alpha, dz, xu) of rho_ref.fma.  alpha == 0 reads no dz."""
    xu = np.ascontiguousarray(xu, np.float64) if double else f32(xu)
    if alpha == 0.0 or dz is None:
        return xu.astype(np.float64)
    if double:
        return fma(alpha, dz, xu)
    return (xu + np.float32(alpha) * f32(dz)).astype(np.float32).astype(np.float64)


# ---- the integrators ----
def step(model, x, u, dt, integrator=0):
    """The next state.  Integrator 0 is iiwa_ref.euler_defect with x_next = 0, negated."""
    if not integrator:
        return -iiwa_ref.euler_defect(model, x, u, np.zeros(n), dt)
    q, qd = x[:NJ], x[NJ:]
    qdn = qd + dt * (np.linalg.inv(model.mass_matrix(q)) @ (u - model.rnea(q, qd, np.zeros(NJ))))        # forward dynamics as iiwa_ref.euler_defect states them
    return np.concatenate([q + dt * qdn, qdn])


def defect(model, x, u, x_next, dt=iiwa_ref.TIMESTEP, integrator=0):
    return x_next - step(model, x, u, dt, integrator) if integrator else iiwa_ref.euler_defect(model, x, u, x_next, dt)


def AB(model, x, u, dt=iiwa_ref.TIMESTEP, integrator=0):
    """(A [n, n], B [n, m]) of the step map at (x, u); integrator 0 as iiwa_ref.generate_kkt composes them."""
    _, dq, dqd, Minv = model.forward_dynamics_and_gradient(x[:NJ], x[NJ:], u)
    A = np.eye(n)
    A[NJ:, :NJ] += dt * dq
    A[NJ:, NJ:] += dt * dqd
    if not integrator:
        A[:NJ, NJ:] += dt * np.eye(NJ)
        return A, np.vstack([np.zeros((NJ, m)), dt * Minv])
    A[:NJ, :NJ] += dt * dt * dq
    A[:NJ, NJ:] += dt * np.eye(NJ) + dt * dt * dqd
    return A, np.vstack([dt * dt * Minv, dt * Minv])


# ---- KKT ----
def _plain_kkt(model, xu, goals, xs, N, dt, integrator):
    """iiwa_ref.generate_kkt (dense layouts: column-major blocks, C = -A, -B) with C and c of integrator 1 laid over it; G, g and c_0 do not depend on it."""
    G, C, g, c = iiwa_ref.generate_kkt(model, xu, goals, xs, N, dt)
    if integrator:
        C, c = C.copy(), c.copy()
        for k in range(N - 1):
            x, u, xn = xu[k * ROW:k * ROW + n], xu[k * ROW + n:(k + 1) * ROW], xu[(k + 1) * ROW:(k + 1) * ROW + n]
            A, B = AB(model, x, u, dt, integrator)
            oc = (n * n + n * m) * k
            C[oc:oc + n * n] = (-A).T.reshape(-1)
            C[oc + n * n:oc + n * n + n * m] = (-B).T.reshape(-1)
            c[(k + 1) * n:(k + 2) * n] = defect(model, x, u, xn, dt, integrator)
    return G, C, g, c


def dynamics(model, xu, goals, xs, N, dt=iiwa_ref.TIMESTEP, integrator=0):
    """What does not depend on the cost's weights or on the plan: (C, g0, c) of the plain entry — the slow part, shared by a test's cost settings."""
    return _plain_kkt(model, np.asarray(xu, np.float64), np.asarray(goals, np.float64).reshape(N, 6), np.asarray(xs, np.float64), N, dt, integrator)[1:]


def generate_kkt(model, xu, goals, xs, N, *, cost=None, rows=None, limits=None, dt=iiwa_ref.TIMESTEP, integrator=0, base=None):
    """(G, C, g, c) of ONE trajectory in iiwa_ref.generate_kkt's layouts.  cost None: the plain entry (no rows, no limits).  Otherwise rows:
    plan_rows(...) or None (zeros); goals None: ee_cost must be 0; base: dynamics(...) of the same xu, xs, dt and integrator (and of the same goals
    unless ee_cost is 0), if the caller has it; limits add their Gauss-Newton terms: w [viol != 0] on the diagonals of Q_k and R_k, w viol in q_k and
    r_k, the last block at x_{N-1}."""
    if cost is None:
        assert rows is None and limits is None and base is None
        return _plain_kkt(model, xu, goals, xs, N, dt, integrator)
    xu = np.asarray(xu, np.float64)
    if goals is None:
        assert cost.ee_cost == 0.0
        goals = np.zeros((N, 6))
    C, g0, c = base if base is not None else dynamics(model, xu, goals, xs, N, dt, integrator)
    x, u = split(xu, N)
    rows = np.zeros((N, ROW)) if rows is None else rows
    gq, G = n * n + m * m, np.zeros((n * n + m * m) * N - m * m)
    g = np.zeros(ROW * N - m)
    for k in range(N):
        # the q part of iiwa_ref's q_k is J^T (ee - goal) itself; in the last block it is iiwa_ref's too: the pose of x_{N-2} against goal_{N-1}
        ge = g0[ROW * k:ROW * k + NJ]
        Q = np.zeros((n, n))
        Q[:NJ, :NJ] = cost.ee_cost * np.outer(ge, ge) + cost.q_cost * np.eye(NJ)
        Q[NJ:, NJ:] = cost.qd_cost * np.eye(NJ)
        G[gq * k:gq * k + n * n] = Q.T.reshape(-1)
        g[ROW * k:ROW * k + n] = np.concatenate([cost.ee_cost * ge + cost.q_cost * (x[k, :NJ] - rows[k, :NJ]), cost.qd_cost * (x[k, NJ:] - cost.qd_rel * rows[k, NJ:n])])
        if k < N - 1:
            G[gq * k + n * n:gq * (k + 1)] = (cost.r_cost * np.eye(m)).reshape(-1)
            g[ROW * k + n:ROW * (k + 1)] = cost.r_cost * (u[k] - cost.u_rel * rows[k, n:])
    if limits is not None:
        for k in range(N):
            vx = viol(x[k], limits.x_lo, limits.x_hi)
            G[gq * k + np.arange(n) * (n + 1)] += limits.x_weight * (vx != 0)
            g[ROW * k:ROW * k + n] += limits.x_weight * vx
            if k < N - 1:
                vu = viol(u[k], limits.u_lo, limits.u_hi)
                G[gq * k + n * n + np.arange(m) * (m + 1)] += limits.u_weight * (vu != 0)
                g[ROW * k + n:ROW * (k + 1)] += limits.u_weight * vu
    return G, C, g, c


def blocks(C, c, N):
    """(A [N-1, n, n], B [N-1, n, m], c [N, n]) out of the dense arrays."""
    Cb = C.reshape(N - 1, n * n + n * m)
    return -Cb[:, :n * n].reshape(N - 1, n, n).transpose(0, 2, 1), -Cb[:, n * n:].reshape(N - 1, m, n).transpose(0, 2, 1), c.reshape(N, n)


# ---- merit ----
def merit_at(model, z, goals, xs, N, mu, *, cost, rows=None, limits=None, dt=iiwa_ref.TIMESTEP, integrator=0):
    """Merit of ONE trajectory at the float64 iterate z [(n+m)N - m]; goals [N][6] or None (ee_cost must be 0), xs [n] or None.  The sum runs joint-space
    terms, then the end-effector sum, then the violations, then the limits.  The plain-cost callers used to sum knot by knot (end-effector and qd term,
    then the u term); over the inputs of every plain-cost merit case of test_gpu_merit*.py, test_gpu_integrator.py, test_gpu_gravity.py and
    test_gpu_chain_plants.py that the CPU can compute (all but the closed loops, whose iterates come from the device), 2342 merits, 22 moved, by
    one unit in the last place: the largest |new - old| / max(1, |old|) is 2.2e-16, against the 1.2e-15 that one hundredth of the tightest limit on a
    merit (1.2e-13, tests/test_gpu_merit_f64.py) allows."""
    z = np.asarray(z, np.float64)
    total = joint_cost(z, rows, N, cost)
    if goals is not None:
        total += cost.ee_cost * ee_cost_sum(model, z, goals, N)
    else:
        assert cost.ee_cost == 0.0
    v = 0.0
    for k in range(N - 1):
        v += np.abs(defect(model, z[k * ROW:k * ROW + n], z[k * ROW + n:(k + 1) * ROW], z[(k + 1) * ROW:(k + 1) * ROW + n], dt, integrator)).sum()
    if xs is not None:
        v += np.abs(z[:n] - np.asarray(xs, np.float64)).sum()
    return total + mu * v if limits is None else total + mu * v + penalty(z, N, limits)


def merits(model, xu, dz, step_sizes, goals, xs, N, mu, *, cost, rows_of=None, limits=None, dt=iiwa_ref.TIMESTEP, integrator=0, double=False, base=None):
    """[B, A] float64 merits of a batch at trial(xu[b], dz[b], alpha, double): xu, dz [B, (n+m)N - m], goals [B, N, 6] or None, xs [B, n] or None,
    rows_of(b) -> [N, 21].  base: the merits of the same arguments without limits, if the caller has them (the penalty is added to them)."""
    out = np.zeros((len(xu), len(step_sizes)))
    for b in range(len(xu)):
        for a, alpha in enumerate(step_sizes):
            z = trial(xu[b], None if dz is None else dz[b], alpha, double)
            if base is not None:
                out[b, a] = base[b, a] + penalty(z, N, limits)
            else:
                out[b, a] = merit_at(model, z, None if goals is None else goals[b], None if xs is None else xs[b], N, mu, cost=cost,
                                     rows=None if rows_of is None else rows_of(b), limits=limits, dt=dt, integrator=integrator)
    return out


def select(merit_row, merit_ref):
    """include/pcg/sqp.cuh:292-301: the first strictly smallest merit below merit_ref; (-1, merit_ref) if none."""
    best, p = merit_ref, -1
    for i, v in enumerate(merit_row):
        if v < best:
            best, p = v, i
    return p, best


# ---- simulate ----
def schedule(toff_us, sim_us, timestep, sim_step=SIM_STEP, double=False):
    """(S, [control index of every full substep], remainder, control index of the remainder substep) — indices NOT clamped.  S = (uint32)(sim / ss),
    idx_s = (uint32)((toff + s ss) / timestep) in IEEE double; ss = sim_step rounded to float and the remainder fmod(sim, ss) an np.float32, or (double)
    sim_step as the double it is and the remainder a double: at 2e-4 and 2,000 us that is S = 10 AND a remainder of 0.00019999999999999996 (ten times
    the double 0.0002 exceeds the double 0.002), reproduced literally.  The remainder keeps the index of the last full substep (the reference does not
    recompute it, :322-324), or (uint32)(toff / timestep) if S = 0."""
    ss = float(sim_step) if double else float(np.float32(sim_step))
    toff, sim = toff_us * 1e-6, sim_us * 1e-6
    S = int(sim / ss)
    idx = [int((toff + s * ss) / timestep) for s in range(S)]
    rem = math.fmod(sim, ss)
    return S, idx, (rem if double else np.float32(rem)), (idx[-1] if S else int(toff / timestep))


def simulate(model, xs, xu, N, timestep, toff_us, sim_us, sim_step=SIM_STEP, integrator=0, double=False, recompute_remainder_index=False,
             ignore_crossing=False):
    """The new float64 state of ONE trajectory: xs [n], xu [(n+m)N - m], float32 values widened or (double) float64 used as they are.  S substeps of
    dt = ss and a remainder substep, the state carried in float64 (the library's stated departure from the reference, which rounds to float after
    every substep), control indices beyond the last control clamped to N - 2.  The two flags give the WRONG alternatives a test must be able to tell
    from the right one: a remainder substep whose index is recomputed at its own time, and a schedule that keeps the first index throughout."""
    S, idx, rem, rem_idx = schedule(toff_us, sim_us, timestep, sim_step, double)
    ss = float(sim_step) if double else float(np.float32(sim_step))
    if recompute_remainder_index:
        rem_idx = int((toff_us * 1e-6 + S * ss) / timestep)
    if ignore_crossing:
        first = int(toff_us * 1e-6 / timestep)
        idx, rem_idx = [first] * S, first
    wide = (lambda a: np.array(a, np.float64)) if double else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    x, xu = wide(xs), wide(xu)
    control = lambda i: xu[min(i, N - 2) * ROW + n:min(i, N - 2) * ROW + ROW]
    for i in idx:
        x = step(model, x, control(i), ss, integrator)
    if rem != 0:
        x = step(model, x, control(rem_idx), float(rem), integrator)
    return x


# ---- the horizon shift ----
def tracking_error(ee, goal0, dtype=np.float32):
    """(|ee0 - g0| + |ee1 - g1|) + |ee2 - g2| in dtype, in that order (mpcsim.cuh:303-306)."""
    t = np.dtype(dtype).type
    d = np.abs(np.asarray(ee, t)[:3] - np.asarray(goal0, t)[:3])
    return t(t(d[0] + d[1]) + d[2])


def advance(shift, N, xu, lam, goal, xs, ee, xu_traj, ee_traj, traj_steps, traj_offset, done, lead=0, dtype=np.float32):
    """mpcg_advance_horizon(_f64) on ONE trajectory: tracking error, traj_offset, just_shift of xu / goals / lambda with their tail fills, and the
    start-state copy, as array operations in dtype (copies only: nothing is rounded).  xu [(n+m)N - m], lam [n N], goal [6 N], xs [n], ee [3], xu_traj
    [traj_steps, n+m], ee_traj [traj_steps, 6].  Returns new (xu, lam, goal, traj_offset, done, tracking error or None); the inputs are not modified."""
    xu, lam, goal = (np.array(a, dtype, copy=True).reshape(-1) for a in (xu, lam, goal))
    if done:
        return xu, lam, goal, traj_offset, done, None
    if not shift:
        xu[:n] = xs
        return xu, lam, goal, traj_offset, done, None
    plan, goals = np.asarray(xu_traj, dtype).reshape(-1), np.asarray(ee_traj, dtype).reshape(-1)
    err = tracking_error(ee, goal[:3], dtype)
    off = traj_offset + 1
    inside = off + N < traj_steps
    new_xu = xu.copy()
    new_xu[:len(xu) - ROW] = xu[ROW:]                         # knots 1..N-2 whole, then x_{N-1} alone: the last moved knot carries no control
    if inside:
        new_xu[len(xu) - ROW:] = plan[ROW * (off + lead) - m:ROW * (off + lead) - m + ROW]
    else:
        new_xu[len(xu) - ROW:] = 0.0
        new_xu[len(xu) - n:len(xu) - n + n // 2] = plan[(traj_steps - 1) * ROW:(traj_steps - 1) * ROW + n // 2]
    new_goal = np.concatenate([goal[6:], goals[6 * ((off + N - 1) if inside else (traj_steps - 1)):][:6]])
    new_lam = np.concatenate([lam[n:], lam[-n:]])             # the last knot keeps its value
    new_xu[:n] = xs
    return new_xu, new_lam, new_goal, off, (1 if off >= traj_steps else 0), err
