"""Float32 restatement of tests/plant_ref.py's merit — TEST INFRASTRUCTURE, the yardstick of the tolerance the tests of `"merit_f32"` = 1
(mpcgpu_amd/csrc/merit_plant_f32.hip.h) use: what plain float arithmetic — the reference's own, include/common/merit.cuh with T = float — makes of the
same formula on the same inputs.

    merit = sum_{k<N} [ J_k + mu ( [k < N-1] |x_{k+1} - (x_k + dt [qd_k; qdd_k])|_1 + [k = 0, xs given] |x_0 - xs|_1 ) ]

Model tables rounded to float32; sine and cosine in float64, rounded (as the device build does); the recursive Newton-Euler passes, the mass matrix, its
Cholesky solve, the cost and the L1 defect all in np.float32 with one rounding per operation (numpy does not fuse); the per-knot values are widened and
summed in float64 (as merit_sum_kernel does).  The trial iterate is plant_ref.trial's float32, used as is.  tests/test_merit_ref_f32_cpu.py pins it
against the float64 restatement."""
import numpy as np

import iiwa_ref
import plant_ref
from mpcgpu_amd import iiwa

F = np.float32
NJ = iiwa_ref.NJ
n, m = plant_ref.n, plant_ref.m
STEPS9 = [0.0] + [-1.0 / (1 << p) for p in range(8)]          # tests/test_gpu_merit.py
STEPS8 = STEPS9[1:]
MU = 10.0
SHAPES = ((2, 1), (3, 2), (8, 3), (9, 1), (32, 2))            # (N, B) of tests/test_gpu_merit.py::test_merit_vs_host_restatement
_inputs = {}


def case_inputs(N, B):
    """(xu, goals, xs, dz) of tests/test_gpu_merit.py::case — the same seeds —, made once per shape and never written to."""
    if (N, B) not in _inputs:
        xu, goals, xs = iiwa.random_windows(N, B, 11 + N)
        dz = 0.05 * np.random.default_rng(1000 + N).standard_normal(xu.shape)
        for arr in (xu, goals, xs, dz):
            arr.setflags(write=False)
        _inputs[(N, B)] = (xu, goals, xs, dz)
    return _inputs[(N, B)]


class Model32:
    """oracle/iiwa_ref.Model with float32 tables and float32 arithmetic."""

    def __init__(self, model=None):
        M = model if model is not None else iiwa_ref.Model()
        self.X_const = M.X_const.astype(F)
        self.X_trig = [(i, F(c), j) for i, c, j in M.X_trig]
        self.I = M.I.astype(F)
        self.Xhom_const = M.Xhom_const.astype(F)
        self.Xhom_trig = [(i, F(c), j) for i, c, j in M.Xhom_trig]

    @staticmethod
    def trig(q):
        q64 = np.asarray(q, F).astype(np.float64)
        return np.concatenate([np.sin(q64), np.cos(q64)]).astype(F)

    def X(self, q):
        t = self.trig(q)
        x = self.X_const.copy()
        for i, c, j in self.X_trig:
            x[np.unravel_index(i, x.shape)] = c * t[j]
        X = x.reshape(NJ, 6, 6).transpose(0, 2, 1).copy()
        X[:, 3:, 3:] = X[:, :3, :3]
        return X

    def Xhom(self, q):
        t = self.trig(q)
        x = self.Xhom_const.copy()
        for i, c, j in self.Xhom_trig:
            x[np.unravel_index(i, x.shape)] = c * t[j]
        return x.reshape(NJ, 4, 4).transpose(0, 2, 1)

    def ee_pos(self, q):
        T = np.eye(4, dtype=F)
        for Xh in self.Xhom(q):
            T = T @ Xh
        return T[:3, 3].copy()

    @staticmethod
    def _crm(v):
        w, u = v[:3], v[3:]
        z = F(0)
        sk = lambda a: np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], F)
        M = np.zeros((6, 6), F)
        M[:3, :3] = sk(w)
        M[3:, :3] = sk(u)
        M[3:, 3:] = sk(w)
        return M

    def rnea(self, q, qd, qdd, X=None):
        X = self.X(q) if X is None else X
        S = np.zeros(6, F)
        S[2] = 1.0
        f = np.zeros((NJ, 6), F)
        vp, ap = np.zeros(6, F), np.zeros(6, F)
        for k in range(NJ):
            v = X[k] @ vp + S * qd[k]
            a = X[k] @ ap + S * qdd[k] + self._crm(v) @ (S * qd[k])
            f[k] = self.I[k] @ a - self._crm(v).T @ (self.I[k] @ v)
            vp, ap = v, a
        tau = np.zeros(NJ, F)
        for k in range(NJ - 1, -1, -1):
            tau[k] = f[k][2]
            if k > 0:
                f[k - 1] += X[k].T @ f[k]
        return tau

    def mass_matrix(self, q, X=None):
        X = self.X(q) if X is None else X
        z = np.zeros(NJ, F)
        M = np.zeros((NJ, NJ), F)
        for j in range(NJ):
            e = np.zeros(NJ, F)
            e[j] = 1.0
            M[:, j] = self.rnea(q, z, e, X)
        return F(0.5) * (M + M.T)

    def forward_dynamics(self, q, qd, u):
        """qdd = M^-1 (u - c(q, qd)) through a float32 Cholesky factorisation and two substitutions."""
        X = self.X(q)
        M = self.mass_matrix(q, X)
        rhs = u - self.rnea(q, qd, np.zeros(NJ, F), X)
        L = np.zeros((NJ, NJ), F)
        for i in range(NJ):
            for j in range(i + 1):
                s = M[i, j]
                for t in range(j):
                    s = s - L[i, t] * L[j, t]
                L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
        y = np.zeros(NJ, F)
        for i in range(NJ):
            s = rhs[i]
            for t in range(i):
                s = s - L[i, t] * y[t]
            y[i] = s / L[i, i]
        for i in range(NJ - 1, -1, -1):
            s = y[i]
            for t in range(i + 1, NJ):
                s = s - L[t, i] * y[t]
            y[i] = s / L[i, i]
        return y


def merit_at(model32, z, goals, xs, N, mu, qd_cost, r_cost, dt=iiwa_ref.TIMESTEP):
    """Merit of ONE trajectory at the float32 iterate z: every knot's value in float32, the knots added in float64."""
    z = np.asarray(z, F)
    goals = plant_ref.f32(goals).reshape(N, 6)
    mu, qd_cost, r_cost, dt, half = F(mu), F(qd_cost), F(r_cost), F(dt), F(0.5)
    total = 0.0
    for k in range(N):
        x = z[k * (n + m):k * (n + m) + n]
        q, qd = x[:NJ], x[NJ:]
        e = model32.ee_pos(q) - goals[k, :3]
        pm = half * (e @ e) + half * qd_cost * (qd @ qd)
        viol = F(0)
        if k < N - 1:
            u = z[k * (n + m) + n:(k + 1) * (n + m)]
            xn = z[(k + 1) * (n + m):(k + 1) * (n + m) + n]
            pm = pm + half * r_cost * (u @ u)
            qdd = model32.forward_dynamics(q, qd, u)
            viol = np.abs(xn - np.concatenate([q + dt * qd, qd + dt * qdd])).sum(dtype=F)
        if k == 0 and xs is not None:
            viol = viol + np.abs(x - plant_ref.f32(xs)).sum(dtype=F)
        point = pm + mu * viol
        assert point.dtype == F
        total += float(point)
    return total


def merits(model32, xu, dz, step_sizes, goals, xs, N, mu, qd_cost, r_cost, dt=iiwa_ref.TIMESTEP):
    """[B, A] merits of a batch, as plant_ref.merits."""
    B = len(xu)
    out = np.zeros((B, len(step_sizes)))
    for b in range(B):
        for a, alpha in enumerate(step_sizes):
            z = plant_ref.trial(xu[b], None if dz is None else dz[b], alpha).astype(F)      # (the widening of trial() undone: exact)
            out[b, a] = merit_at(model32, z, goals[b], None if xs is None else xs[b], N, mu, qd_cost, r_cost, dt)
    return out


def decision_inputs(N, B, seed):
    """Inputs of the decision tests: windows of iiwa.random_windows moved off by a seeded error e, and dz = s_b e + a smaller independent error with
    s_b = 1, 2, 4, ... per trajectory — the best of the step sizes -1, -1/2, ... lies near -1 / s_b, another one for every trajectory."""
    xu, goals, xs = iiwa.random_windows(N, B, seed)
    rng = np.random.default_rng(seed + 1)
    e = 0.03 * rng.standard_normal(xu.shape)
    scale = np.array([float(1 << (b % 6)) for b in range(B)])[:, None]
    dz = scale * (e + 0.004 * rng.standard_normal(xu.shape))
    return xu + e, goals, xs, dz


def close_tie(candidates, ref):
    """True if the runner-up among the candidates and merit_ref lies within 2e-5 max(1, |winner|) of the winner: a decision float arithmetic may make
    differently."""
    order = np.sort(np.append(np.asarray(candidates, np.float64), ref))
    return order[1] - order[0] <= 2e-5 * max(1.0, abs(order[0]))
