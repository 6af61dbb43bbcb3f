"""Float64 restatement of the SECOND integrator of the reference, semi-implicit (symplectic) Euler — INTEGRATOR_TYPE == 1 of include/common/integrator.cuh
(:22-57 defect, :59-100 A and B, :103-130 step) — TEST INFRASTRUCTURE, the checker of options "integrator" and "sim_integrator" = 1
(mpcgpu_amd/csrc/kkt_plant.hip.h, merit_plant.hip.h, merit_plant_f32.hip.h, sim_plant.hip.h).  With qdd = FD(q, qd, u) as everywhere else (no gravity):

    step     qd' = qd + dt qdd;  q' = q + dt qd'
    defect   c_{k+1} = x_{k+1} - [q + dt (qd + dt qdd); qd + dt qdd]          (c_0 = x_0 - x_s as before)
    A        I + dt [[dt dqdd/dq, I + dt dqdd/dqd], [dqdd/dq, dqdd/dqd]]      (the lower half is explicit Euler's)
    B        [dt^2 Minv; dt Minv]

Built on the pieces of oracle/iiwa_ref.py::Model (forward_dynamics_and_gradient, rnea, mass_matrix), so it serves tests/chain_models.py::Chain too.
integrator = 0 is explicit Euler and delegates to the existing restatements: the arrays are theirs exactly."""
import numpy as np

import iiwa_ref
import merit_ref
import merit_ref_f64
import sim_ref
import sim_ref_f64

NJ = 7
n, m = 14, 7


def qdd_of(model, x, u):
    """Forward dynamics as iiwa_ref.euler_defect states them."""
    q, qd = x[:NJ], x[NJ:]
    return np.linalg.inv(model.mass_matrix(q)) @ (u - model.rnea(q, qd, np.zeros(NJ)))


def semi_implicit_step(model, x, u, dt):
    q, qd = x[:NJ], x[NJ:]
    qdn = qd + dt * qdd_of(model, x, u)
    return np.concatenate([q + dt * qdn, qdn])


def semi_implicit_defect(model, x, u, x_next, dt=iiwa_ref.TIMESTEP):
    return x_next - semi_implicit_step(model, x, u, dt)


def step(model, x, u, dt, integrator):
    return semi_implicit_step(model, x, u, dt) if integrator else sim_ref.euler_step(model, x, u, dt)


def defect(model, x, u, x_next, dt, integrator):
    return semi_implicit_defect(model, x, u, x_next, dt) if integrator else iiwa_ref.euler_defect(model, x, u, x_next, dt)


def semi_implicit_AB(model, x, u, dt=iiwa_ref.TIMESTEP):
    """(A [n, n], B [n, m]) of the semi-implicit step map at (x, u)."""
    _, dq, dqd, Minv = model.forward_dynamics_and_gradient(x[:NJ], x[NJ:], u)
    A = np.eye(n)
    A[NJ:, :NJ] += dt * dq
    A[NJ:, NJ:] += dt * dqd
    A[:NJ, :NJ] += dt * dt * dq
    A[:NJ, NJ:] += dt * np.eye(NJ) + dt * dt * dqd
    B = np.vstack([dt * dt * Minv, dt * Minv])
    return A, B


def generate_kkt(model, xu, ee_goals, xs, knot_points, dt=iiwa_ref.TIMESTEP, integrator=0):
    """iiwa_ref.generate_kkt (same dense layouts: column-major blocks, C = -A, -B) under either integrator.  The costs G, g and c_0 do not depend on it."""
    G, C, g, c = iiwa_ref.generate_kkt(model, xu, ee_goals, xs, knot_points, dt)
    if not integrator:
        return G, C, g, c
    N = knot_points
    C, c = C.copy(), c.copy()
    for k in range(N - 1):
        x = xu[k * (n + m):k * (n + m) + n]
        u = xu[k * (n + m) + n:(k + 1) * (n + m)]
        xn = xu[(k + 1) * (n + m):(k + 1) * (n + m) + n]
        A, B = semi_implicit_AB(model, x, u, dt)
        oc = (n * n + n * m) * k
        C[oc:oc + n * n] = (-A).T.reshape(-1)
        C[oc + n * n:oc + n * n + n * m] = (-B).T.reshape(-1)
        c[(k + 1) * n:(k + 2) * n] = semi_implicit_defect(model, x, u, xn, dt)
    return G, C, g, c


def blocks(C, c, N):
    """(A [N-1, n, n], B [N-1, n, m], c [N, n]) out of the dense arrays."""
    Cb = C.reshape(N - 1, n * n + n * m)
    return -Cb[:, :n * n].reshape(N - 1, n, n).transpose(0, 2, 1), -Cb[:, n * n:].reshape(N - 1, m, n).transpose(0, 2, 1), c.reshape(N, n)


# ---- merit ----
def merit_at(model, z, goals, xs, N, mu, qd_cost, r_cost, dt=iiwa_ref.TIMESTEP, integrator=0):
    """merit_ref.merit_at with the violation |x_{k+1} - step(x_k, u_k)|_1 of either integrator."""
    if not integrator:
        return merit_ref.merit_at(model, z, goals, xs, N, mu, qd_cost, r_cost, dt)
    goals = merit_ref.f32(goals).astype(np.float64).reshape(N, 6)
    total = viol = 0.0
    for k in range(N):
        x = z[k * (n + m):k * (n + m) + n]
        e = model.ee_pos(x[:7]) - goals[k, :3]
        total += 0.5 * e @ e + 0.5 * qd_cost * x[7:] @ x[7:]
        if k < N - 1:
            u = z[k * (n + m) + n:(k + 1) * (n + m)]
            total += 0.5 * r_cost * u @ u
            viol += np.abs(semi_implicit_defect(model, x, u, z[(k + 1) * (n + m):(k + 1) * (n + m) + n], dt)).sum()
    if xs is not None:
        viol += np.abs(z[:n] - merit_ref.f32(xs).astype(np.float64)).sum()
    return total + mu * viol


def merits(model, xu, dz, step_sizes, goals, xs, N, mu, qd_cost, r_cost, dt=iiwa_ref.TIMESTEP, integrator=0, double=False):
    """[B, A] float64 merits of a batch: the float trial iterate of merit_ref.trial, or (double) the double one of merit_ref_f64.trial."""
    trial = merit_ref_f64.trial if double else merit_ref.trial
    out = np.zeros((len(xu), len(step_sizes)))
    for b in range(len(xu)):
        for a, alpha in enumerate(step_sizes):
            out[b, a] = merit_at(model, trial(xu[b], None if dz is None else dz[b], alpha), goals[b], None if xs is None else xs[b], N, mu, qd_cost, r_cost,
                                 dt, integrator)
    return out


# ---- simulate ----
def simulate(model, xs, xu, N, timestep, toff_us, sim_us, sim_step, integrator=0, double=False):
    """sim_ref.simulate / sim_ref_f64.simulate (their schedule: sim_ref.schedule, or its double twin) with the substep of either integrator."""
    ref = sim_ref_f64 if double else sim_ref
    if not integrator:
        return ref.simulate(model, xs, xu, N, timestep, toff_us, sim_us, sim_step)
    S, idx, rem, rem_idx = ref.schedule(toff_us, sim_us, timestep, sim_step)
    ss = float(sim_step) if double else float(np.float32(sim_step))
    wide = (lambda a: np.asarray(a, np.float64)) if double else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    x, xu = np.array(wide(xs)), wide(xu)
    control = lambda i: xu[min(i, N - 2) * (n + m) + n:min(i, N - 2) * (n + m) + n + m]
    for i in idx:
        x = semi_implicit_step(model, x, control(i), ss)
    if rem != 0:
        x = semi_implicit_step(model, x, control(rem_idx), float(rem))
    return x
