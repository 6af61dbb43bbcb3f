"""CPU: the Cost argument of tests/plant_ref.py, the float64 restatement of the generalised running cost (mpcg_generate_kkt_xuref / mpcg_compute_merit_xuref), against
itself — its two reductions, the gradient and Hessian of its own cost sum, the row rule — and the four new symbols in the built library and in
include/mpcg.h."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import iiwa_ref
import plant_ref as X
from mpcgpu_amd import iiwa

n, m, NJ, ROW = 14, 7, 7, 21


@pytest.fixture(scope="module")
def model():
    return iiwa_ref.Model()


def window(N, seed):
    xu, goals, xs = iiwa.random_windows(N, 1, seed)
    return xu[0], goals[0], xs[0]


def plan(T, seed):
    return np.random.default_rng(seed).standard_normal((T, ROW))


@pytest.mark.parametrize("N", [2, 5])
def test_reduces_to_the_end_effector_plant(model, N):
    """ee_cost = 1, q_cost = 0, no flags: iiwa_ref.generate_kkt's numbers, except the seven qd entries of q_{N-1}: qd_cost qd_{N-1}, not qd_cost qd_{N-2}."""
    xu, goals, xs = window(N, 5 + N)
    rows = X.plan_rows(plan(9, N), 0, 3, N, 9)
    cost = X.Cost(1.0, 0.0, iiwa_ref.QD_COST, iiwa_ref.r_cost(N), 0)
    got = X.generate_kkt(model, xu, goals, xs, N, rows=rows, cost=cost)
    want = [a.copy() for a in iiwa_ref.generate_kkt(model, xu, goals, xs, N)]
    last = slice(ROW * (N - 1) + NJ, ROW * (N - 1) + n)
    assert not np.array_equal(got[2][last], want[2][last])
    assert np.array_equal(want[2][last], iiwa_ref.QD_COST * xu[ROW * (N - 2) + NJ:ROW * (N - 2) + n])
    want[2][last] = iiwa_ref.QD_COST * xu[ROW * (N - 1) + NJ:ROW * (N - 1) + n]
    for a, w, name in zip(got, want, "GCgc"):
        assert np.array_equal(a, w), name


@pytest.mark.parametrize("N", [2, 4])
def test_reduces_to_the_joint_space_plant(model, N):
    """ee_cost = 0, q_cost > 0, QD_RELATIVE: include/dynamics/iiwa/iiwa_plant.cuh — Q = blkdiag(Q_cost I, QD_cost I), q = [Q_cost (q - q_ref); QD_cost (qd - qd_ref)],
    R = R_cost I, r = R_cost u, the last block at x_{N-1} against its own row; written out here knot by knot."""
    xu, goals, xs = window(N, 17 + N)
    T, off = 6, 3                                              # N = 4: knot 3 clamps to the plan's last row
    P = plan(T, 40 + N)
    rows = X.plan_rows(P, 0, off, N, T)
    cost = X.Cost(0.0, 0.37, 2e-3, 5e-4, X.QD_RELATIVE)
    G, C, g, c = X.generate_kkt(model, xu, None, xs, N, rows=rows, cost=cost)
    _, C0, _, c0 = iiwa_ref.generate_kkt(model, xu, goals, xs, N)
    assert np.array_equal(C, C0) and np.array_equal(c, c0)
    Q = np.diag([0.37] * NJ + [2e-3] * NJ)
    for k in range(N):
        x = xu[ROW * k:ROW * k + n]
        ref = P[min(off + k, T - 1)]
        o = (n * n + m * m) * k
        assert np.array_equal(G[o:o + n * n], Q.reshape(-1))
        assert np.array_equal(g[ROW * k:ROW * k + n], np.concatenate([0.37 * (x[:NJ] - ref[:NJ]), 2e-3 * (x[NJ:] - ref[NJ:n])]))
        if k < N - 1:
            assert np.array_equal(G[o + n * n:o + n * n + m * m], (5e-4 * np.eye(m)).reshape(-1))
            assert np.array_equal(g[ROW * k + n:ROW * (k + 1)], 5e-4 * xu[ROW * k + n:ROW * (k + 1)])


@pytest.mark.parametrize("flags", [0, X.QD_RELATIVE, X.U_RELATIVE, X.QD_RELATIVE | X.U_RELATIVE])
def test_g_is_the_gradient_and_G_the_hessian_of_the_cost_sum(model, flags):
    """ee_cost = 0: the cost sum is quadratic in xu, so central differences with h = 1e-3 are exact to rounding — they equal the restated g to 1e-9, and
    the second differences the stated diagonal (G has no off-diagonal entry and no cross-knot block)."""
    N, T = 4, 5
    xu, _, xs = window(N, 23)
    rows = X.plan_rows(plan(T, 7), 0, -1, N, T)
    cost = X.Cost(0.0, 0.8, 0.05, 0.02, flags)
    G, _, g, _ = X.generate_kkt(model, xu, None, xs, N, rows=rows, cost=cost)
    J = lambda z: X.joint_cost(z, rows, N, cost)
    h = 1e-3
    num = np.zeros_like(g)
    hess = np.zeros_like(g)
    for i in range(len(xu)):
        e = np.zeros_like(xu)
        e[i] = h
        num[i] = (J(xu + e) - J(xu - e)) / (2 * h)
        hess[i] = (J(xu + e) - 2 * J(xu) + J(xu - e)) / (h * h)
    assert np.abs(num - g).max() <= 1e-9 * max(1.0, np.abs(g).max()), np.abs(num - g).max()
    diag = np.concatenate([np.concatenate([[0.8] * NJ, [0.05] * NJ, [0.02] * m]) for _ in range(N)])[:len(xu)]
    assert np.abs(hess - diag).max() <= 1e-6
    for k in range(N):
        o = (n * n + m * m) * k
        assert np.array_equal(G[o:o + n * n].reshape(n, n), np.diag(diag[ROW * k:ROW * k + n]))
        if k < N - 1:
            assert np.array_equal(G[o + n * n:o + n * n + m * m].reshape(m, m), 0.02 * np.eye(m))


def test_row_rule():
    """row(b, k) = clamp(off_b + k, 0, traj_steps - 1) in 64-bit, plan_b = plan + b * traj_batch_stride rows."""
    T, N = 5, 4
    assert [X.row_index(-2, k, T) for k in range(N)] == [0, 0, 0, 1]                     # a negative offset clamps at the first row
    assert [X.row_index(3, k, T) for k in range(N)] == [3, 4, 4, 4]                      # off + k >= traj_steps clamps mid-horizon
    assert [X.row_index(2 ** 31 - 1, k, T) for k in range(N)] == [4] * N                 # no 32-bit wrap at the largest offset
    assert [X.row_index(-2 ** 31, k, T) for k in range(N)] == [0] * N
    assert X.row_index(7, 0, 1) == 0 and X.row_index(-7, 3, 1) == 0                      # a plan of one row
    stride = 7                                                                           # two trajectories' plans, two unused rows behind each
    P = np.arange(2 * stride * ROW, dtype=np.float64).reshape(2 * stride, ROW)
    assert np.array_equal(X.plan_rows(P, 1, 3, N, T, stride), P[[stride + 3, stride + 4, stride + 4, stride + 4]])
    assert np.array_equal(X.plan_rows(P, 0, -1, N, T, stride), P[[0, 0, 1, 2]])
    assert np.array_equal(X.plan_rows(P, 1, 3, N, T, 0), P[[3, 4, 4, 4]])                # stride 0: trajectory 1 reads the shared plan


def test_merit_is_the_cost_sum_plus_the_violations(model):
    """mu = 0 leaves sum_k J_k: the joint-space sum plus ee_cost times the end-effector sum; and the violation terms are the plain cost's."""
    N, T = 3, 4
    xu, goals, xs = window(N, 31)
    rows = X.plan_rows(plan(T, 3), 0, 1, N, T)
    cost = X.Cost(0.6, 0.3, 0.01, 0.02, X.QD_RELATIVE | X.U_RELATIVE)
    got = X.merit_at(model, xu, goals, xs, N, 0.0, rows=rows, cost=cost)
    assert got == X.joint_cost(xu, rows, N, cost) + 0.6 * X.ee_cost_sum(model, xu, goals, N)
    plain = X.Cost(1.0, 0.0, iiwa_ref.QD_COST, iiwa_ref.r_cost(N), 0)
    a = X.merit_at(model, xu, X.f32(goals).astype(np.float64), X.f32(xs).astype(np.float64), N, 10.0, rows=rows, cost=plain)
    b = X.merit_at(model, xu, X.f32(goals), X.f32(xs), N, 10.0, cost=X.Cost.plain(iiwa_ref.QD_COST, iiwa_ref.r_cost(N)))
    assert abs(a - b) <= 1e-13 * max(1.0, abs(b))


NEW = ("mpcg_generate_kkt_xuref", "mpcg_generate_kkt_xuref_f64", "mpcg_compute_merit_xuref", "mpcg_compute_merit_xuref_f64")


def test_new_symbols_are_exported_and_declared(hiplib):
    from mpcgpu_amd import _lib
    header = open(os.path.join(ROOT, "include", "mpcg.h")).read()
    for name in NEW:
        assert hasattr(hiplib, name), f"{name} is not exported by the built library"
        assert name in _lib.SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/mpcg.h"
    assert "typedef struct mpcg_xuref" in header and "MPCG_XUREF_QD_RELATIVE" in header and "MPCG_XUREF_U_RELATIVE" in header
    assert _lib.MPCG_XUREF_QD_RELATIVE == 1 and _lib.MPCG_XUREF_U_RELATIVE == 2
    import ctypes as C
    assert C.sizeof(_lib.mpcg_xuref) == 48                    # pointer, 2 x uint32, pointer, 2 x double, uint32 + padding (LP64)
