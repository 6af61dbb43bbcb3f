"""CPU: tests/gravity_ref.py — the restatements with gravity that tests/test_gpu_gravity.py holds the kernels to — pinned without the device:
the gravity torques against the gradient of a potential energy that does not come out of the recursion (sign and axes), the zero vector against the
plain chain bit for bit, the compensation identity FD_g(q, qd, u + tau_g) = FD_0(q, qd, u), the visibility of a wrong convention at the GPU tests'
tolerances, and the restatement's own noise in C."""
import functools

import numpy as np
import pytest

import chain_models as cm
import gravity_ref as gr
import iiwa_ref
import merit_ref_f32

PLANTS = list(cm.SEEDS) + ["iiwa"]
LIMIT_C = 8.9e-7                         # tests/test_gpu_kkt_f64.py::LIMIT_C
NJ = cm.NJ
Z = np.zeros(NJ)


@functools.lru_cache(maxsize=None)
def plain(which):
    return cm.Chain.from_iiwa() if which == "iiwa" else cm.random_chain(which)


def seed_of(which):
    return 70 if which == "iiwa" else 70 + which


def fd(model, q, qd, u):
    return np.linalg.inv(model.mass_matrix(q)) @ (u - model.rnea(q, qd, Z))


# ---- 1. the sign and the axes ----
@pytest.mark.parametrize("which", PLANTS)
def test_gravity_torques_are_the_gradient_of_the_potential_energy(which):
    """ID(q, 0, 0) = dV/dq with V = sum_i m_i base_accel . c_i(q), the centres of mass taken through Xhom: central differences at h = 1e-6 of a potential
    of order 100, noise 1e-14 / 1e-6 x a few.  Limit 1e-6 (absolute, Nm).  Measured 1.7e-8 on the random chains."""
    ch = gr.chain(which)
    worst = biggest = 0.0
    for q, _, _ in cm.states(6, seed_of(which)):
        tau = ch.gravity_torques(q)
        grad = np.zeros(NJ)
        for j in range(NJ):
            e = np.zeros(NJ)
            e[j] = 1e-6
            grad[j] = (ch.potential(q + e) - ch.potential(q - e)) / 2e-6
        worst, biggest = max(worst, np.abs(tau - grad).max()), max(biggest, np.abs(tau).max())
    print(f"{which}: |tau_g - dV/dq| {worst:.1e}, |tau_g| up to {biggest:.1f} Nm")
    assert biggest > 5.0
    assert worst <= 1e-6


def test_the_iiwa_gravity_torques_at_the_printed_state():
    tau = gr.chain("iiwa").gravity_torques(np.array(gr.Q_PRINTED))
    print("iiwa tau_g", np.round(tau, 3).tolist())
    assert np.abs(tau - np.array(gr.TAU_PRINTED)).max() <= 5.1e-4           # (three decimals printed)


# ---- 2. the zero vector is the plain chain ----
@pytest.mark.parametrize("which", PLANTS)
def test_the_zero_vector_is_the_plain_chain_bit_for_bit(which):
    ch, zero = plain(which), gr.chain(which, (0.0, 0.0, 0.0))
    for q, qd, u in cm.states(3, seed_of(which)):
        assert np.array_equal(zero.rnea(q, qd, u), ch.rnea(q, qd, u))
        assert np.array_equal(zero.mass_matrix(q), ch.mass_matrix(q))
        x, xn = np.concatenate([q, qd]), np.concatenate([qd, q])
        assert np.array_equal(iiwa_ref.euler_defect(zero, x, u, xn), iiwa_ref.euler_defect(ch, x, u, xn))
    xu, goals, xs = cm.hard_inputs(3, 1, 5, "large")
    for a, b in zip(iiwa_ref.generate_kkt(zero, xu[0], goals[0], xs[0], 3), iiwa_ref.generate_kkt(ch, xu[0], goals[0], xs[0], 3)):
        assert np.array_equal(a, b)


# ---- 3. compensation ----
@pytest.mark.parametrize("which", PLANTS)
def test_compensated_forward_dynamics_are_the_plain_ones(which):
    """FD_g(q, qd, u + tau_g(q)) = FD_0(q, qd, u) to 1e-13 of max(1, |qdd|).  Measured 2.5e-16."""
    ch, g = plain(which), gr.chain(which)
    worst = 0.0
    for q, qd, u in cm.states(6, seed_of(which)):
        a, b = fd(g, q, qd, u + g.gravity_torques(q)), fd(ch, q, qd, u)
        assert np.array_equal(g.mass_matrix(q), ch.mass_matrix(q))            # the inertia matrix does not see gravity
        assert np.abs(fd(g, q, qd, u) - b).max() > 1e-2                        # (and uncompensated it matters)
        worst = max(worst, float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max()))
    print(f"{which}: compensation {worst:.1e}")
    assert worst <= 1e-13


# ---- 4. a wrong convention is visible at the GPU tests' tolerances ----
def moves(right, wrong, xu, goals, xs, N):
    """Worst relative move of C and of c over the batch, each of max(1, |block|)."""
    out = [0.0, 0.0]
    for b in range(len(xu)):
        x, y = (iiwa_ref.generate_kkt(mdl, xu[b], goals[b], xs[b], N) for mdl in (right, wrong))
        out = [max(o, np.abs(x[i] - y[i]).max() / max(1.0, np.abs(x[i]).max())) for o, i in zip(out, (1, 3))]
    return out


@pytest.mark.parametrize("size", list(cm.SETS))
@pytest.mark.parametrize("which", PLANTS)
def test_a_wrong_convention_is_visible(which, size):
    """On the inputs tests/test_gpu_gravity.py uses (shape (3, 5)): the restatement with the vector negated, and the one with x and y swapped, each move C
    and c by more than 1e-3 of max(1, |block|) — a thousand times the float entries' 1e-6.  The iiwa's vector (0, 0, g) has no x or y to swap: its case
    is the negation alone."""
    N, B = 3, 5
    xu, goals, xs = cm.hard_inputs(N, B, 0 if which == "iiwa" else cm.input_seed(which), size)
    right = gr.chain(which)
    g = right.base_accel
    wrong = {"negated": -g} if which == "iiwa" else {"negated": -g, "x <-> y": np.array([g[1], g[0], g[2]])}
    for name, vec in wrong.items():
        mv = moves(right, gr.chain(which, vec), xu, goals, xs, N)
        print(f"{which} {size} {name}: C {mv[0]:.1e} c {mv[1]:.1e}")
        assert min(mv) > 1e-3, (name, mv)


# ---- 5. the restatement's own noise in C, with gravity ----
@pytest.mark.parametrize("which", PLANTS)
def test_restatement_noise_of_C_with_gravity(which):
    """dt dqdd/d(q, qd) by central differences at h = 1e-6 against h = 2e-6, of max(1, |block|), on the large set: below a tenth of LIMIT_C.
    Measured 3.5e-9 with gravity (1.7e-9 without)."""
    ch = gr.chain(which)
    worst = 0.0
    for q, qd, u in cm.states(6, seed_of(which)):
        a, b = ch.forward_dynamics_and_gradient(q, qd, u, h=1e-6), ch.forward_dynamics_and_gradient(q, qd, u, h=2e-6)
        for x, y in zip(a[1:3], b[1:3]):
            worst = max(worst, iiwa_ref.TIMESTEP * np.abs(x - y).max() / max(1.0, iiwa_ref.TIMESTEP * np.abs(x).max()))
    print(f"{which}: noise of C with gravity {worst:.1e}")
    assert worst <= LIMIT_C / 10


# ---- 6. the float model ----
def test_the_float_model_follows():
    """gravity_ref.Gravity32 on the iiwa (Model32 evaluates one trig term per table entry, as iiwa_ref.Model does: the iiwa's tables, not a general
    chain's): with the zero vector it is merit_ref_f32.Model32 bit for bit; with gravity its forward dynamics are the float64 model's to float accuracy
    (1e-4 of max(1, |qdd|): cond(M) of a few hundred times 6e-8 times torques of tens of Nm), and its inertia matrix is Model32's."""
    which = "iiwa"
    tab = iiwa_ref.Model()
    g64 = gr.chain(which)
    m32, z32, g32 = merit_ref_f32.Model32(tab), gr.Gravity32(tab), gr.Gravity32(tab, g64.base_accel)
    F = np.float32
    for q, qd, u in cm.states(3, seed_of(which), "modest"):
        q, qd, u = F(q), F(qd), F(u)
        assert np.array_equal(z32.rnea(q, qd, u), m32.rnea(q, qd, u)) and np.array_equal(z32.forward_dynamics(q, qd, u), m32.forward_dynamics(q, qd, u))
        assert np.array_equal(g32.mass_matrix(q), m32.mass_matrix(q))
        want = fd(g64, q.astype(np.float64), qd.astype(np.float64), u.astype(np.float64))
        err = float((np.abs(g32.forward_dynamics(q, qd, u) - want) / np.maximum(1.0, np.abs(want))).max())
        assert err <= 1e-4, err
