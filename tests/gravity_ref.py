"""Gravity in the float64 restatements — TEST INFRASTRUCTURE (a helper module, not a conftest): the checker of the plants mpcg_plant_clone_gravity makes
(include/mpcg.h, GRAVITY; mpcgpu_amd/csrc/kkt_plant.hip.h::rnea) and of mpcg_inverse_dynamics(_f64) (csrc/invdyn_plant.hip.h).

The reference hands gato_plant::GRAVITY<T>() to every GRiD call and GRiD uses it as the acceleration the chain's root starts from, a_1 = X_1[:, 5] * gravity: a
base spatial acceleration [0 0 0 0 0 g].  Here: `base_accel`, the linear part, three numbers in the base frame; the physical gravitational acceleration is
its negative.

    GravityChain    chain_models.Chain whose rnea starts from ap[3:] = base_accel, and whose mass_matrix evaluates its columns WITHOUT it (the inherited
                    one calls self.rnea(q, 0, e_j) and would add the gravity torques to every column).  Every other restatement takes the model as an
                    argument — iiwa_ref.generate_kkt and every stage of tests/plant_ref.py — and follows with no further code.
    Gravity32       merit_ref_f32.Model32, the separate float model, with the same two changes
    potential       V(q) = sum_i m_i base_accel . c_i(q), the link centres of mass taken through Xhom: independent of the recursion, so
                    dV/dq = ID(q, 0, 0) pins the sign and the axes (tests/test_gravity_ref_cpu.py)
"""
import numpy as np

import chain_models as cm
import iiwa_ref
import merit_ref_f32

NJ = iiwa_ref.NJ
F = np.float32
G_CHAIN = (1.7, -2.9, 9.2)               # the vector the random chains of chain_models.SEEDS are cloned with: no component zero, none equal
G_IIWA = (0.0, 0.0, 9.81)                # the built-in iiwa standing on the ground, z up
Q_PRINTED = (0.3, -0.7, 1.1, 0.5, -1.3, 0.9, 0.2)
TAU_PRINTED = (0.0, 52.87, 7.121, -15.039, 0.932, 0.038, 0.0)      # iiwa gravity torques at Q_PRINTED under G_IIWA [Nm], to the three decimals printed


class GravityChain(cm.Chain):
    def __init__(self, ET, p, I, base_accel=(0.0, 0.0, 0.0)):
        super().__init__(ET, p, I)
        self.base_accel = np.array(base_accel, np.float64).reshape(3)

    @classmethod
    def of(cls, chain, base_accel):
        return cls(chain.ET, chain.p, chain.I, base_accel)

    def rnea(self, q, qd, qdd, X=None):
        """iiwa_ref.Model.rnea, statement for statement, with the root's linear acceleration started at base_accel."""
        X = self.X(q) if X is None else X
        S = np.zeros(6)
        S[2] = 1.0
        v = np.zeros((NJ, 6))
        a = np.zeros((NJ, 6))
        f = np.zeros((NJ, 6))
        vp, ap = np.zeros(6), np.zeros(6)
        ap[3:] = self.base_accel
        for k in range(NJ):
            v[k] = X[k] @ vp + S * qd[k]
            a[k] = X[k] @ ap + S * qdd[k] + self._crm(v[k]) @ (S * qd[k])
            f[k] = self.I[k] @ a[k] - self._crm(v[k]).T @ (self.I[k] @ v[k])
            vp, ap = v[k], a[k]
        tau = np.zeros(NJ)
        for k in range(NJ - 1, -1, -1):
            tau[k] = f[k][2]
            if k > 0:
                f[k - 1] += X[k].T @ f[k]
        return tau

    def mass_matrix(self, q):
        """iiwa_ref.Model.mass_matrix with the columns ID(q, 0, e_j) evaluated without gravity."""
        X = self.X(q)
        z = np.zeros(NJ)
        M = np.zeros((NJ, NJ))
        for j in range(NJ):
            e = np.zeros(NJ)
            e[j] = 1.0
            M[:, j] = iiwa_ref.Model.rnea(self, q, z, e, X)
        return 0.5 * (M + M.T)

    def gravity_torques(self, q):
        z = np.zeros(NJ)
        return self.rnea(q, z, z)

    def potential(self, q):
        """sum_i m_i base_accel . c_i: link i's centre of mass c = h / m (skew(h) is the upper-right block of its spatial inertia) carried to the base
        frame by the homogeneous transforms."""
        T = np.eye(4)
        V = 0.0
        for k, Xh in enumerate(self.Xhom(q)):
            T = T @ Xh
            mass = self.I[k][3, 3]
            h = np.array([self.I[k][2, 4], self.I[k][0, 5], self.I[k][1, 3]])
            V += mass * self.base_accel @ (T @ np.append(h / mass, 1.0))[:3]
        return V


class Gravity32(merit_ref_f32.Model32):
    """merit_ref_f32.Model32 (float32 tables, float32 arithmetic) with a float32 base_accel; `model`: iiwa_ref.Model() (Model32 evaluates one trig
    term per table entry: the iiwa's tables, not a general chain's)."""

    def __init__(self, model=None, base_accel=(0.0, 0.0, 0.0)):
        super().__init__(model)
        self.base_accel = np.array(base_accel, np.float64).astype(F).reshape(3)

    def rnea(self, q, qd, qdd, X=None):
        X = self.X(q) if X is None else X
        S = np.zeros(6, F)
        S[2] = 1.0
        f = np.zeros((NJ, 6), F)
        vp, ap = np.zeros(6, F), np.zeros(6, F)
        ap[3:] = self.base_accel
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
            M[:, j] = merit_ref_f32.Model32.rnea(self, q, z, e, X)
        return F(0.5) * (M + M.T)


def chain(which, base_accel=None):
    """The plants of the tests: the random chain of seed `which` with G_CHAIN, or ("iiwa") the iiwa from its geometry with G_IIWA."""
    if which == "iiwa":
        return GravityChain.of(cm.Chain.from_iiwa(), G_IIWA if base_accel is None else base_accel)
    return GravityChain.of(cm.random_chain(which), G_CHAIN if base_accel is None else base_accel)


def perturbed(model, rng):
    """The model with every table entry multiplied by 1 + delta, delta uniform in +-2^-52 (the convention of tests/util.py's bands, in double)."""
    d = lambda a: a * (1.0 + rng.uniform(-1, 1, np.shape(a)) * 2.0 ** -52)
    return GravityChain(d(model.ET), d(model.p), d(model.I), d(model.base_accel))
