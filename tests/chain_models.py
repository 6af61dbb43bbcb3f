"""Robots other than the KUKA iiwa 14 for the plant kernels — TEST INFRASTRUCTURE (a helper module, not a conftest).

mpcg_plant_create takes any fixed-base serial chain of seven revolute-z joints (include/mpcg.h: "the robot as DATA"); the kernels behind it
(mpcgpu_amd/csrc/kkt_plant.hip.h, merit_plant*.hip.h, sim_plant.hip.h) run generic recursions over ET[7][9], BT[7][9], Ib[7][10].  The iiwa is a
degenerate point of that table space: every ET_k is a signed permutation, BT_k has two non-zero entries, no link offset has an x component, and
the inertia products and h_x lie below the tests' tolerances — about half of the 28 numbers per joint are invisible to a test on the iiwa.

    Chain           a model given by GEOMETRY (rotations ET_k, link offsets p_k, spatial inertias I_k) with X(q), Xhom(q) evaluated from it;
                    the rigid-body algorithms are oracle/iiwa_ref.py's, inherited unchanged
    random_chain    a general chain in which no table entry sits below the tolerances (seeds: SEEDS)
    tables          the chain in the table format mpcg_plant_create reads (what solver.Plant takes)
    eval_tables     X(q), Xhom(q) from such tables, as place() of mpcg_plant_create reads them
    hard_inputs     states over more than one turn of every joint, with large or modest velocities and torques
    CORRUPTIONS     single wrong table entries a test on a random chain must see (tests/test_chain_models_cpu.py)
"""
import types

import numpy as np

import iiwa_ref

NJ = iiwa_ref.NJ
n, m = 2 * NJ, NJ
SEEDS = (1, 2, 3)                      # the random chains every test uses
SHAPES = ((2, 1), (3, 5), (9, 3))      # (knot points, batch) of the GPU tests
# mpcg_generate_kkt_f64 against the restatement, arrays G and g, on these chains and inputs (tests/test_gpu_chain_plants.py): ten times the restatement's
# OWN noise in those two arrays — its central-difference ee_jac at h = 1e-6 against h = 2e-6, measured on the CPU by
# tests/test_chain_models_cpu.py::test_restatement_noise_of_the_cost_arrays (G 6.84e-10 at worst, g 3.81e-10; on the iiwa's windows, centimetres from their goals, the noise is 1e-11)
KKT_F64_LIMIT_Gg = 6.9e-9


def skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


class Chain(iiwa_ref.Model):
    """E_k(q) = Rz(q_k) ET_k with Rz = [[c, s, 0], [-s, c, 0], [0, 0, 1]];  X_k = [[E, 0], [-E skew(p_k), E]];  Xhom_k = [[E^T, p_k], [0, 1]].
    iiwa_ref.Model evaluates its tables as x[i] = coef * t[j], one term per entry; in a general chain every entry of rows 0 and 1 carries a sine AND
    a cosine term, so the geometry is the reference here."""

    def __init__(self, ET, p, I):
        self.ET = np.array(ET, np.float64).reshape(NJ, 3, 3)
        self.p = np.array(p, np.float64).reshape(NJ, 3)
        self.I = np.array(I, np.float64).reshape(NJ, 6, 6)

    @classmethod
    def from_iiwa(cls):
        M = iiwa_ref.Model()
        z = np.zeros(NJ)
        return cls(M.X(z)[:, :3, :3], M.Xhom(z)[:, :3, 3], M.I)

    def E(self, q):
        E = np.empty((NJ, 3, 3))
        for k in range(NJ):
            c, s = np.cos(q[k]), np.sin(q[k])
            E[k, 0] = c * self.ET[k, 0] + s * self.ET[k, 1]
            E[k, 1] = c * self.ET[k, 1] - s * self.ET[k, 0]
            E[k, 2] = self.ET[k, 2]
        return E

    def X(self, q):
        E = self.E(q)
        X = np.zeros((NJ, 6, 6))
        for k in range(NJ):
            X[k, :3, :3] = X[k, 3:, 3:] = E[k]
            X[k, 3:, :3] = -E[k] @ skew(self.p[k])
        return X

    def Xhom(self, q):
        E = self.E(q)
        H = np.zeros((NJ, 4, 4))
        for k in range(NJ):
            H[k, :3, :3] = E[k].T
            H[k, :3, 3] = self.p[k]
            H[k, 3, 3] = 1.0
        return H

    def BT(self):
        """-ET_k skew(p_k): the lower-left block of X_k(0)."""
        return np.array([-self.ET[k] @ skew(self.p[k]) for k in range(NJ)])


def _rotation(rng):
    Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def _signed(rng, lo, hi, size):
    return rng.choice([-1.0, 1.0], size) * rng.uniform(lo, hi, size)


def random_chain(seed):
    """ET_k a random proper rotation; p_k with each component in +-[0.08, 0.25] m; mass in [1, 6] kg, centre of mass c with each component in +-0.1 m,
    Ibar = U diag(pr) U^T + m (|c|^2 1 - c c^T) with principal moments pr in [0.005, 0.05] that respect the triangle inequality.  A joint is redrawn
    until every entry of ET_k and BT_k exceeds 0.02, every inertia product 1e-3 and every component of h = m c 1e-2 in magnitude."""
    rng = np.random.default_rng(seed)
    ET, P, I = [], [], []
    for _ in range(NJ):
        while True:
            E = _rotation(rng)
            p = _signed(rng, 0.08, 0.25, 3)
            mass = rng.uniform(1.0, 6.0)
            c = rng.uniform(-0.1, 0.1, 3)
            pr = rng.uniform(0.005, 0.05, 3)
            U = _rotation(rng)
            Ibar = U @ np.diag(pr) @ U.T + mass * (c @ c * np.eye(3) - np.outer(c, c))
            Ibar = 0.5 * (Ibar + Ibar.T)
            h = mass * c
            if (2 * pr.max() < pr.sum() and np.abs(E).min() > 0.02 and np.abs(E @ skew(p)).min() > 0.02
                    and min(abs(Ibar[0, 1]), abs(Ibar[0, 2]), abs(Ibar[1, 2])) > 1e-3 and np.abs(h).min() > 1e-2):
                break
        S = np.zeros((6, 6))
        S[:3, :3] = Ibar
        S[:3, 3:] = skew(h)
        S[3:, :3] = skew(h).T
        S[3:, 3:] = mass * np.eye(3)
        ET.append(E)
        P.append(p)
        I.append(S)
    return Chain(ET, P, I)


def tables(chain):
    """The attributes solver.Plant reads, in the format include/mpcg.h documents (GRiD's): column-major 6x6 / 4x4 constants; a trig entry
    (index, coef, j) = coef * sin(q_j) for j < 7, coef * cos(q_{j-7}) otherwise, REPLACING the constant at its index.  Rows 0 and 1 of E and B
    (columns 0 and 1 of the rotation of Xhom) carry one sine and one cosine entry per index; row 2 is constant.  As in the committed iiwa tables the
    lower-right block of X carries its constant row only: it repeats E."""
    ET, BT = chain.ET, chain.BT()
    Xc = np.zeros((NJ, 36))
    Hc = np.zeros((NJ, 16))
    Xt, Ht = [], []
    for k in range(NJ):
        for c in range(3):
            for T, r0 in ((ET[k], 0), (BT[k], 3)):
                Xc[k, 6 * c + r0 + 2] = T[2, c]
                i0, i1 = 36 * k + 6 * c + r0, 36 * k + 6 * c + r0 + 1
                Xt += [(i0, T[1, c], k), (i0, T[0, c], NJ + k), (i1, -T[0, c], k), (i1, T[1, c], NJ + k)]
            Xc[k, 6 * (3 + c) + 5] = ET[k][2, c]
        for r in range(3):                                         # Xhom rotation = E^T: [r][0] = E[0][r], [r][1] = E[1][r], [r][2] = ET[2][r]
            i0, i1 = 16 * k + r, 16 * k + 4 + r
            Ht += [(i0, ET[k][1, r], k), (i0, ET[k][0, r], NJ + k), (i1, -ET[k][0, r], k), (i1, ET[k][1, r], NJ + k)]
            Hc[k, 8 + r] = ET[k][2, r]
            Hc[k, 12 + r] = chain.p[k, r]
        Hc[k, 15] = 1.0
    clean = lambda t: [(int(i), float(c), int(j)) for i, c, j in t]
    return types.SimpleNamespace(X_const=Xc, X_trig=clean(Xt), I=chain.I.copy(), Xhom_const=Hc, Xhom_trig=clean(Ht))


def eval_tables(X_const, X_trig, Xhom_const, Xhom_trig, q):
    """(X(q) [7, 6, 6], Xhom(q) [7, 4, 4]) from the tables: the constant, replaced at an index by the SUM of that index's trig terms — how place() of
    mpcg_plant_create reads them.  The lower-right block of X repeats the upper-left one (the library ignores what the tables hold there)."""
    t = np.concatenate([np.sin(q), np.cos(q)])

    def ev(const, trig):
        x = np.array(const, np.float64).reshape(-1).copy()
        for i in {i for i, _, _ in trig}:
            x[i] = 0.0
        for i, c, j in trig:
            x[i] += c * t[j]
        return x

    X = ev(X_const, X_trig).reshape(NJ, 6, 6).transpose(0, 2, 1).copy()
    X[:, 3:, 3:] = X[:, :3, :3]
    return X, ev(Xhom_const, Xhom_trig).reshape(NJ, 4, 4).transpose(0, 2, 1).copy()


# ---- inputs ----
SETS = {"large": (2.0, 20.0), "modest": (0.5, 2.0)}              # (|qd| <=, |u| <=)


def hard_inputs(N, B, seed, size="large"):
    """float64 (xu [B, (n+m)N - m], goals [B, N, 6], xs [B, n]): every q uniform in [-2 pi, 2 pi] — all four quadrants of the kernels' own sine / cosine
    reduction, both signs, more than one turn —, |qd| <= 2 and |u| <= 20 ("large") or 0.5 and 2 ("modest"), goals in +-1, xs = x_0 + 0.01."""
    vq, vu = SETS[size]
    rng = np.random.default_rng([seed, N, B, 0 if size == "large" else 1])
    z = np.zeros((B, N, n + m))
    z[:, :, :NJ] = rng.uniform(-2 * np.pi, 2 * np.pi, (B, N, NJ))
    z[:, :, NJ:n] = rng.uniform(-vq, vq, (B, N, NJ))
    z[:, :, n:] = rng.uniform(-vu, vu, (B, N, m))
    xu = z.reshape(B, -1)[:, :(n + m) * N - m].copy()
    goals = rng.uniform(-1.0, 1.0, (B, N, 6))
    return xu, goals, xu[:, :n] + 0.01


def input_seed(seed):
    """The seed of the inputs the GPU tests give chain `seed`."""
    return 1000 + seed


def states(count, seed, size="large"):
    """`count` single states (q, qd, u) of a set."""
    xu, _, _ = hard_inputs(2, count, seed, size)
    return [(w[:NJ], w[NJ:n], w[n:n + m]) for w in xu]


# ---- single wrong table entries ----
def _with(chain, ET=None, p=None, I=None):
    return Chain(chain.ET if ET is None else ET, chain.p if p is None else p, chain.I if I is None else I)


def _offset_x_dropped(ch):
    p = ch.p.copy()
    p[:, 0] = 0.0
    return _with(ch, p=p)


def _ixy_ixz_swapped(ch):
    I = ch.I.copy()
    I[:, 0, 1], I[:, 0, 2] = ch.I[:, 0, 2], ch.I[:, 0, 1]
    I[:, 1, 0], I[:, 2, 0] = ch.I[:, 2, 0], ch.I[:, 1, 0]
    return _with(ch, I=I)


def _products_dropped(ch):
    I = ch.I.copy()
    for a, b in ((0, 1), (0, 2), (1, 2)):
        I[:, a, b] = I[:, b, a] = 0.0
    return _with(ch, I=I)


def _hx_dropped(ch):
    I = ch.I.copy()                                                # skew(h): h_x sits at [1][5], [2][4] and their mirror images
    I[:, 1, 5] = I[:, 5, 1] = I[:, 2, 4] = I[:, 4, 2] = 0.0
    return _with(ch, I=I)


def _one_et_transposed(ch):
    ET = ch.ET.copy()
    ET[3] = ch.ET[3].T
    return _with(ch, ET=ET)


CORRUPTIONS = {"link-offset x dropped": _offset_x_dropped, "Ixy <-> Ixz": _ixy_ixz_swapped, "inertia products dropped": _products_dropped,
               "h_x dropped": _hx_dropped, "one ET_k transposed": _one_et_transposed}
