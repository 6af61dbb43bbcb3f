"""CPU: tests/plant_ref.py and tests/rho_ref.py pinned on a record of what the nine restatement modules they replace computed.

tests/golden/plant_ref_parent.npz holds outputs only, each under its call's parameters as the key, and names the commit it was made from.  It was
written at that commit by a script that fed the inputs built below (inputs(), limits_of(), advance_inputs(), the rho sequences) to the modules of that
commit — merit_ref, merit_ref_f64, integrator_ref, xuref_ref, limits_ref, sim_ref, sim_ref_f64, rho_ref, rho_ref_f64 — call for call as record() feeds
them to the two modules here; those modules are gone, so the script is not kept.  Everything is held bit for bit (np.array_equal), except the merits
of the plain cost, which moved from the knot-by-knot sum of merit_ref.merit_at to the order of xuref_ref.merit_at: those are held within 1.2e-15
relative to max(1, |merit|), one hundredth of the tightest limit a GPU test applies to a merit (1.2e-13, tests/test_gpu_merit_f64.py)."""
import os

import numpy as np
import pytest

import iiwa_ref
import plant_ref as P
import rho_ref
from mpcgpu_amd import iiwa

RECORD = os.path.join(P.GOLDEN, "plant_ref_parent.npz")
PARENT = "8817aa5144c57996b766933530e86e607467b0a6"
DT = iiwa_ref.TIMESTEP
MU = 10.0
STEPS = [0.0, -1.0, -0.25]
B = 2
SCHEDULES = [(0, 2000), (15000, 2100), (15000, 100), (46000, 2000), (15500, 300)]          # tests/test_gpu_simulate.py::CASES
MERIT_MOVE = 1.2e-15
COSTS = {"plain": lambda N: P.Cost.plain(iiwa_ref.QD_COST, iiwa_ref.r_cost(N)),
         "joint": lambda N: P.Cost(0.0, 0.37, 2e-3, 5e-4, P.QD_RELATIVE),
         "both": lambda N: P.Cost(0.6, 0.3, 0.01, 0.02, P.QD_RELATIVE | P.U_RELATIVE)}


def widened(a):
    return np.asarray(a, np.float32).astype(np.float64)


def inputs(N):
    """B windows: xu and dz genuinely double, goals and xs float-representable (merit_ref.merit_at rounded those two itself), and per-trajectory plans."""
    xu, goals, xs = iiwa.random_windows(N, B, 100 + N)
    rng = np.random.default_rng(200 + N)
    dz = 0.01 * rng.standard_normal(xu.shape)
    T, stride = 6, 7
    plan = rng.standard_normal((B * stride, P.ROW))
    rows_of = lambda b: P.plan_rows(plan, b, (1, 3)[b], N, T, stride)                      # N = 5: both clamp to the plan's last row
    return xu, dz, widened(goals), widened(xs), rows_of


def thirds(vals):
    """Bounds at the lower and upper third of each column of vals [rows, 7] (tests/test_limits_ref_cpu.py); one row: it lies below."""
    s = np.sort(vals, axis=0)
    if len(s) < 2:
        return s[0] + 0.5, s[0] + 1.0
    k = max(1, len(s) // 3)
    return 0.5 * (s[k - 1] + s[k]), 0.5 * (s[-k - 1] + s[-k])


def limits_of(xu, N):
    x, u = P.split(xu[0], N)
    return P.Limits(*thirds(x[:, :P.NJ]), *thirds(x[:, P.NJ:]), *thirds(u), 3.0, 0.25, 0.125)


def advance_inputs(N, inside):
    T = N + 6 if inside else N + 1
    rng = np.random.default_rng(300 + 10 * N + inside)
    f = lambda *s: rng.standard_normal(s)
    return (f(P.ROW * N - P.m), f(P.n * N), f(6 * N), f(P.n), f(3), f(T, P.ROW), f(T, 6)), T


RHO_OUTCOMES = [-1] * 14 + [0, 2, -1, 1, 1, 1, -1]              # rho passes rho_max and resets in the failures, then recovers


def rho_step_inputs(dtype):
    rng = np.random.default_rng(7)
    Bn, A, L = 5, 3, 11
    merit = rng.standard_normal((Bn, A)).astype(dtype)
    merit[3] = 9.0                                              # no step
    ref = np.full(Bn, 0.5, dtype)
    dz, xu = rng.standard_normal((Bn, L)).astype(dtype), rng.standard_normal((Bn, L)).astype(dtype)
    rho, drho = np.array([1e-3, 0.3, 9.5, 9.9, 1.0], dtype), np.array([1.0, 1.2, 1.5, 2.0, 0.9], dtype)
    return merit, ref, dz, xu, rho, drho, np.array([0, 0, 0, 0, 1], np.uint8)


def record():
    """{key: array} of the two modules here."""
    M, out = iiwa_ref.Model(), {}
    for N in (2, 5):
        xu, dz, goals, xs, rows_of = inputs(N)
        lim = limits_of(xu, N)
        for double in (False, True):
            for alpha in STEPS + [0.3]:
                out[f"trial N={N} double={double} alpha={alpha}"] = P.trial(xu[0], dz[0], alpha, double)
        for integ in (0, 1):
            x, u, xn = xu[0][:P.n], xu[0][P.n:P.ROW], xu[0][P.ROW:P.ROW + P.n]
            out[f"step N={N} integrator={integ}"] = P.step(M, x, u, DT, integ)
            out[f"defect N={N} integrator={integ}"] = P.defect(M, x, u, xn, DT, integ)
            if integ:
                A, Bm = P.AB(M, x, u, DT, integ)
                out[f"A N={N} integrator={integ}"], out[f"B N={N} integrator={integ}"] = A, Bm
            for b in range(B):
                base = P.dynamics(M, xu[b], goals[b], xs[b], N, DT, integ)
                kkts = {"none": P.generate_kkt(M, xu[b], goals[b], xs[b], N, dt=DT, integrator=integ)}
                for name, cost in COSTS.items():
                    g = None if cost(N).ee_cost == 0.0 else goals[b]
                    kkts[name] = P.generate_kkt(M, xu[b], g, xs[b], N, cost=cost(N), rows=rows_of(b), dt=DT, integrator=integ, base=base if b else None)
                kkts["both+limits"] = P.generate_kkt(M, xu[b], goals[b], xs[b], N, cost=COSTS["both"](N), rows=rows_of(b), limits=lim, dt=DT, integrator=integ, base=base)
                for name, arrays in kkts.items():
                    for a, letter in zip(arrays, "GCgc"):
                        if letter in "Cc" and name not in ("none", "both+limits"):      # (C and c pass through the cost: recorded at both ends)
                            continue
                        out[f"kkt {letter} N={N} integrator={integ} cost={name} b={b}"] = a
            for double in (False, True):
                for name, cost in COSTS.items():
                    g = None if cost(N).ee_cost == 0.0 else goals
                    kw = dict(cost=cost(N), dt=DT, integrator=integ, double=double)
                    if name != "plain":
                        kw["rows_of"] = rows_of
                    out[f"merits N={N} integrator={integ} double={double} cost={name}"] = P.merits(M, xu, dz, STEPS, g, xs, N, MU, **kw)
                out[f"merits N={N} integrator={integ} double={double} cost=plain no xs"] = P.merits(M, xu, dz, STEPS, goals, None, N, MU, cost=COSTS["plain"](N), dt=DT,
                                                                                                      integrator=integ, double=double)
                out[f"merits N={N} integrator={integ} double={double} cost=both+limits"] = P.merits(M, xu, dz, STEPS, goals, xs, N, MU, cost=COSTS["both"](N), rows_of=rows_of,
                                                                                                     limits=lim, dt=DT, integrator=integ, double=double)
    xu, _, _, xs, _ = inputs(4)
    for toff, sim in SCHEDULES:
        for double in (False, True):
            S, idx, rem, ridx = P.schedule(toff, sim, DT, 2e-4, double)
            out[f"schedule toff={toff} sim={sim} double={double}"] = np.array([S, ridx] + idx, np.float64)
            out[f"schedule remainder toff={toff} sim={sim} double={double}"] = np.array(rem)
            for integ in (0, 1):
                for flags in ({}, {"recompute_remainder_index": True}, {"ignore_crossing": True})[:1 if integ else 3]:      # (the flags: integrator 0 only)
                    out[f"simulate toff={toff} sim={sim} double={double} integrator={integ} {sorted(flags)}"] = P.simulate(M, xs[0], xu[0], 4, DT, toff, sim, 2e-4, integ, double, **flags)
    for N in (2, 4):
        for inside in (True, False):
            args, T = advance_inputs(N, inside)
            for lead in (0, N - 1):
                for dtype in (np.float32, np.float64):
                    got = P.advance(True, N, *[a.astype(dtype) for a in args], T, 0, 0, lead, dtype)
                    for a, name in zip(got, ("xu", "lam", "goal", "off", "done", "err")):
                        out[f"advance {name} N={N} inside={inside} lead={lead} {np.dtype(dtype).name}"] = np.asarray(a)
    for dtype in (np.float32, np.float64):
        name = np.dtype(dtype).name
        rho, drho, seq = 1e-3, 1.0, []
        for p in RHO_OUTCOMES:
            rho, drho, done = rho_ref.update(rho, drho, p, dtype=dtype)
            seq.append([rho, drho, done])
        out[f"rho update {name}"] = np.array(seq, dtype)
        merit, ref, dz, xu, rho, drho, done = rho_step_inputs(dtype)
        steps = [-1.0, -0.5, -0.25] if dtype == np.float32 else [-1.0, -0.3, -0.25]
        codes = rho_ref.step(merit, steps, ref, dz, xu, rho, drho, done, rho_reset=0.01, dtype=dtype)
        for a, key in zip((codes, ref, xu, rho, drho, done), ("codes", "ref", "xu", "rho", "drho", "done")):
            out[f"rho step {key} {name}"] = a
        if dtype == np.float64:
            merit, ref, dz, xu = rho_step_inputs(dtype)[:4]
            out[f"plain step codes {name}"] = rho_ref.step(merit, steps, ref, dz, xu, dtype=dtype)
            out[f"plain step xu {name}"] = xu
    return out


@pytest.fixture(scope="module")
def parent():
    return np.load(RECORD)


@pytest.fixture(scope="module")
def here():
    return record()


def test_record_is_small_and_names_its_commit(parent):
    assert os.path.getsize(RECORD) < 256 * 1024
    assert str(parent["commit"]) == PARENT


def test_every_recorded_call_is_made_here(parent, here):
    assert set(parent.files) - {"commit"} == set(here)


def test_the_recorded_cases_reach_every_branch():
    """A limits case pins the penalty only where bounds are active: q, qd and u on both sides (u at N = 2, one row: below).  The rho sequence reaches
    rho_max and resets.  The schedules hold ten substeps, a crossing, a remainder and S = 0."""
    for N in (2, 5):
        xu = inputs(N)[0]
        lim = limits_of(xu, N)
        x, u = P.split(xu[0], N)
        for s in (P.side(x[:, :P.NJ], lim.q_lo, lim.q_hi), P.side(x[:, P.NJ:], lim.qd_lo, lim.qd_hi), P.side(u, lim.u_lo, lim.u_hi)):
            assert (s != 0).any() and (N == 2 or ((s > 0).any() and (s < 0).any()))
    rho, drho, resets = 1e-3, 1.0, 0
    for p in RHO_OUTCOMES:
        rho, drho, done = rho_ref.update(rho, drho, p)
        resets += done
    assert resets >= 1
    S = {c: P.schedule(*c, DT, 2e-4) for c in SCHEDULES}
    assert S[(0, 2000)][0] == 10 and S[(15000, 100)][0] == 0 and S[(15000, 2100)][2] != 0 and len(set(S[(15000, 2100)][1])) == 2


def test_bit_for_bit_except_the_plain_merit(parent, here):
    for key, got in here.items():
        want = parent[key]
        if key.startswith("merits") and "cost=plain" in key:
            move = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            assert move.max() <= MERIT_MOVE, (key, move.max())
        else:
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True), key
