"""GPU: the PCG entry points inside a guard-banded arena (tests/arena.py) — no entry reads or writes past its arrays, writes an input, or
depends on where its arrays lie.  Every case in both layouts ("aligned": 256-byte starts; "minimal": every array at exactly the smallest
alignment the entry accepts).  Next to the arena's four checks the outputs are, bit for bit, those of the same call on the same handle with
separately allocated tensors — the calls tests/test_gpu_first_steps.py and tests/test_gpu_invariants.py pin to the float64 model on these
very inputs (tests/pcg_step_cases.py), so the equality carries that comparison over.

Two calls from lambda0 per case: max_iter = 2 with exit_tol = 0, and max_iter = 0 (lambda keeps every bit)."""
import numpy as np
import pytest
import torch

import arena
import arena_specs as A
import pcg_step_cases as cases
from test_gpu_first_steps import launched, solver

pytestmark = pytest.mark.gpu
B = cases.B


def batched_call(sol, entry, Bt, K, pc):
    from mpcgpu_amd import pcg_config

    def call(a):
        getattr(sol, entry)(a["S"].view(Bt, -1), a["Pinv"].view(Bt, -1), a["gamma"].view(Bt, -1), a["lambda"].view(Bt, -1),
                            pcg_config(pcg_exit_tol=0.0, pcg_max_iter=K), pc, iters=a["iters"], exits=a["exits"])
    return call


def ref_call(sol, prec, K):
    fn = sol.solve_ref if prec == "f32" else sol.solve_ref_f64

    def call(a):
        fn(a["S"], a["Pinv"], a["gamma"], a["lambda"], a["r"], a["p"], a["v_temp"], a["eta_new_temp"], a["iters"], a["exits"], K, 0.0)
    return call


def counts_and_flags(out, K, lam0, tag):
    assert (out["iters"] == K).all() and (out["exits"] == 1).all(), (tag, K, out["iters"], out["exits"])
    if K == 0:
        assert out["lambda"].tobytes() == np.ascontiguousarray(lam0).tobytes(), (tag, "max_iter = 0 must hand lambda0 back bit for bit")


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("r", cases.ROWS, ids=cases.row_id)
def test_batched_entries(r, mode):
    """mpcg_pcg_solve / mpcg_pcg_solve_f64, every row: five systems per launch (three at state sizes other than 14)."""
    Bt = A.batch_of(r)
    S, P, g, lam0 = (a[:Bt] for a in cases.device_matrices(r))
    sol = solver(r, Bt)
    tag = cases.row_id(r)
    for K in (2, 0):
        out = arena.both_ways(A.pcg(r.prec, r.n, r.N, Bt, K > 0), mode, {"S": S, "Pinv": P, "gamma": g, "lambda": lam0},
                              batched_call(sol, "solve" if r.prec == "f32" else "solve_f64", Bt, K, r.pc), tag)
        launched(sol, r.family, r.waves, tag)
        counts_and_flags(out, K, lam0, tag)


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("pc", ["ss", "jacobi"])
@pytest.mark.parametrize("N,opts,family,waves", cases.F16_CASES, ids=[f"N{c[0]}-family{c[2]}" for c in cases.F16_CASES])
def test_fp16_storage(N, opts, family, waves, pc, mode):
    """mpcg_pcg_solve_f16: S and Pinv in half precision at 4-byte alignment (the 0xFF fill is a half NaN too)."""
    S, P, g, lam0 = cases.f16_system(N, pc)
    r = cases.Row("f32", 14, 7, N, pc, family, opts, waves)
    sol = solver(r, B)
    S16, P16 = (sol.to_f16(torch.from_numpy(M.copy()).cuda()).cpu().numpy() for M in (S, P))
    tag = f"fp16 storage N={N} {pc} family {family}"
    for K in (2, 0):
        out = arena.both_ways(A.pcg("f32", 14, N, B, K > 0, "f16"), mode, {"S": S16, "Pinv": P16, "gamma": g, "lambda": lam0},
                              batched_call(sol, "solve_f16", B, K, pc), tag)
        launched(sol, family, waves, tag)
        counts_and_flags(out, K, lam0, tag)


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("r", cases.ROWS, ids=cases.row_id)
def test_twelve_argument_entries(r, mode):
    """mpcg_pcg_solve_ref / _ref_f64 on trajectory 0 of every row: d_r and d_p written whole, d_v_temp and d_eta_new_temp (knot_points
    elements each, as the reference sizes them) untouched, one 32-bit count and ONE byte of flag with bands around both.  The handle as
    tests/test_gpu_invariants.py makes it: nobody vouches for block symmetry, the first launch of a lower-triangle row is guarded."""
    from mpcgpu_amd import PcgSolver
    S, P, g, lam0 = (np.array(a[0]) for a in cases.three_column_matrices(r))
    sol = PcgSolver(r.N, max_batch=1, state_size=r.n)
    for key, value in r.opts:
        sol.set_option(key, value)
    tag = "12 arguments " + cases.row_id(r)
    for K in (2, 0):
        out = arena.both_ways(A.pcg_ref(r.prec, r.n, r.N, K > 0), mode, {"S": S, "Pinv": P, "gamma": g, "lambda": lam0},
                              ref_call(sol, r.prec, K), tag)
        launched(sol, r.family, r.waves, tag)
        counts_and_flags(out, K, lam0, tag)


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("r", A.LATCH, ids=cases.row_id)
def test_guarded_launch_and_symmetry_check_on_a_fresh_handle(r, mode):
    """One row per lower-triangle family WITHOUT "assume_symmetric": the symmetry check kernel and the guarded launch run against NaN bands and
    NaN never-read blocks.  The matrices are block-symmetric, so after three more calls the latch must say 1; a check kernel that compares one
    block too far compares a NaN and would latch 2.  Four calls in the arena, the same bits each time and from separately allocated tensors."""
    from mpcgpu_amd import PcgSolver
    S, P, g, lam0 = cases.device_matrices(r)
    sol = PcgSolver(r.N, max_batch=B, state_size=r.n)
    for key, value in r.opts:
        sol.set_option(key, value)
    tag = "fresh handle " + cases.row_id(r)
    ar = arena.Arena(A.pcg(r.prec, r.n, r.N, B, True), mode, "torch")
    for name, values in (("S", S), ("Pinv", P), ("gamma", g)):
        ar.put(name, values)
    call = batched_call(sol, "solve" if r.prec == "f32" else "solve_f64", B, 2, r.pc)
    outs = []
    for _ in range(4):
        ar.put("lambda", lam0)
        ar.refill("iters", "exits")
        outs.append(ar.run(call))
        counts_and_flags(outs[-1], 2, lam0, tag)
    assert sol.get_option("symmetry_state") == 1, (tag, sol.get_option("symmetry_state"), sol.last_error())
    launched(sol, r.family, r.waves, tag)
    ar.put("lambda", lam0)
    plain = ar.plain()
    call(plain)
    torch.cuda.synchronize()
    want = plain["lambda"].cpu().numpy().tobytes()
    for i, out in enumerate(outs):
        assert out["lambda"].tobytes() == want, (tag, mode, i)


@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("r", A.TILED, ids=cases.row_id)
def test_more_workgroups_than_cus_and_the_stored_dispatch_order(r, mode):
    """2 x num_cus + 3 trajectories tiled from the row's five, called twice: the second call runs under the dispatch order the first one stored
    (sched_order_kernel reads d_iters behind the solve).  Every copy carries the bits of its original, both times, and the bands stay intact."""
    S, P, g, lam0 = cases.device_matrices(r)
    total = A.tiled_total(solver(r, 1).get_option("num_cus"))
    tile = lambda a: np.tile(a, (-(-total // B), 1))[:total]
    sol = solver(r, total)
    tag = "tiled " + cases.row_id(r)
    ar = arena.Arena(A.pcg("f32", 14, r.N, total, True), mode, "torch")
    for name, values in (("S", S), ("Pinv", P), ("gamma", g)):
        ar.put(name, tile(values))
    call = batched_call(sol, "solve", total, 2, r.pc)
    lam = []
    for _ in range(2):
        ar.put("lambda", tile(lam0))
        ar.refill("iters", "exits")
        out = ar.run(call)
        launched(sol, r.family, r.waves, tag)
        assert (out["iters"] == 2).all() and (out["exits"] == 1).all(), tag
        lam.append(out["lambda"].reshape(total, -1))
    ar.put("lambda", tile(lam0))
    plain = ar.plain()
    call(plain)
    torch.cuda.synchronize()
    want = plain["lambda"].cpu().numpy().reshape(total, -1)
    for b in range(total):
        assert lam[0][b].tobytes() == lam[0][b % B].tobytes() == lam[1][b].tobytes() == want[b].tobytes(), (tag, mode, b)
