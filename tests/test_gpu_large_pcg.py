"""GPU: the PCG entry points with S and Pinv each past 2^32 bytes, one test per kernel family the plan table (tests/golden/pcg_plan_table.json)
can select — float families 0, 5, 6, 7 and 11, the generic family 3 at n = 13, fp16 storage, double families 8, 9 and 10 — each at the smallest
horizon of tests/pcg_step_cases.py that selects it, pinned by the row's options; "last_kernel_family" is asserted after the call on D
trajectories and after the large one.  tests/large_extents.py: five distinct systems tiled over the batch on the device, one of them cold
(lambda0 = 0), four warm; exit_tol = 0 and max_iter = 2, so every count is 2 and every flag 1, exactly, and "cluster_fixups" stays 0 (two
iterations suffice: the addressing is the same in every iteration).  lambda, counts and flags of every tile carry the bits of the call on the
five, and that call is held to tests/pcg_step_model.py's prediction of the first two iterations at tests/test_gpu_first_steps.py's limit.
The 12-argument entries run once per precision on the LAST trajectory of the large arrays (its matrices straddle 2^32 bytes) against the
same call on that trajectory's original: lambda, d_r, d_p, count and flag bit for bit, d_v_temp and d_eta_new_temp untouched."""
import numpy as np
import pytest
import torch

import large_extents as le
import pcg_step_cases as cases
from pcg_step_model import EPS32, HP
from test_gpu_first_steps import U64, check, dev, solve, solver

pytestmark = pytest.mark.gpu
COLD = 1                                   # the tile that starts from lambda0 = 0


def family_is(sol, r, tag):
    assert sol.get_option("last_kernel_family") == r.family, (tag, sol.get_option("last_kernel_family"))
    if r.family in cases.CLUSTERED:
        assert sol.get_option("cluster_fixups") == 0, tag


def filled(count, dt):
    """count elements of dt holding 0xFF bytes."""
    return torch.full((count * torch.empty((), dtype=dt).element_size(),), le.FILL, dtype=torch.uint8, device="cuda").view(dt)


def with_a_cold_tile(lam0):
    lam0 = lam0.copy()
    lam0[COLD] = 0
    return lam0


def large_solve(r, spec, entry, S, P, g, lam0, Sh, Ph, after_big=None):
    """K = 1 on the five (for the model), then le.run with K = 2; S, P as the device gets them, Sh, Ph as the row's kernel applies them."""
    from mpcgpu_amd import pcg_config
    if r.prec == "f64" and np.finfo(np.longdouble).eps > 2.0 ** -60:
        pytest.skip("no extended-precision long double on this host")
    sol = solver(r, spec.B)
    tag = spec.label
    lam1 = solve(sol, entry, dev(S), dev(P), dev(g), dev(lam0), 1, r.pc)
    family_is(sol, r, tag)
    cfg = pcg_config(pcg_exit_tol=0.0, pcg_max_iter=2)
    families = []

    def call(a, Bt):
        getattr(sol, entry)(a["S"], a["Pinv"], a["gamma"], a["lambda"], cfg, r.pc, iters=a["iters"].view(-1), exits=a["exits"].view(-1))
        families.append(sol.get_option("last_kernel_family"))
    out = le.run(spec, {"S": S, "Pinv": P, "gamma": g, "lambda": lam0}, call, (lambda *a: after_big(sol, *a)) if after_big else None)
    assert families == [r.family, r.family], (tag, families)
    if r.family in cases.CLUSTERED:
        assert sol.get_option("cluster_fixups") == 0, tag
    sol.close()
    assert (out["iters"] == 2).all() and (out["exits"] == 1).all(), (tag, out["iters"].ravel(), out["exits"].ravel())
    HP[0] = np.float64 if r.prec == "f32" else np.longdouble
    try:
        check(tag, Sh, Ph, g, lam0, lam1, out["lambda"], r.N, r.n, r.pc, EPS32 if r.prec == "f32" else U64)
    finally:
        HP[0] = np.float64


def row_solve(r, spec, after_big=None):
    S, P, g, lam0 = cases.device_matrices(r)
    Sh, Ph = cases.host_matrices(r)[:2]
    large_solve(r, spec, "solve" if r.prec == "f32" else "solve_f64", S, P, g, with_a_cold_tile(lam0), Sh, Ph, after_big)


@pytest.mark.parametrize("r", le.PCG_ROWS, ids=cases.row_id)
def test_pcg_solve_with_matrices_past_2_32(r):
    row_solve(r, le.pcg_spec(r))


def test_pcg_solve_f16_with_matrices_past_2_32():
    """Half storage: S16 and Pinv16 of 2^32 bytes hold twice the elements.  The five are rounded by mpcg_convert_f32_to_f16, the prediction is
    made from the rounded matrices (tests/test_gpu_first_steps.py)."""
    r = le.f16_row()
    spec = le.pcg_spec(r, "f16")
    S, P, g, lam0 = cases.f16_system(r.N, r.pc)
    sol = solver(r, cases.B)
    S16, P16 = (sol.to_f16(dev(M)).cpu() for M in (S, P))
    sol.close()
    Sh, Ph = (np.stack([cases.applied(M[b], 14, r.N, cases.reads_lower(r)) for b in range(cases.B)]) for M in (S16.float().numpy(), P16.float().numpy()))
    large_solve(r, spec, "solve_f16", S16.numpy(), P16.numpy(), g, with_a_cold_tile(lam0), Sh, Ph)


@pytest.mark.parametrize("r", le.PCG_REF_ROWS, ids=cases.row_id)
def test_pcg_solve_ref_on_the_last_trajectory_of_the_large_arrays(r):
    spec = le.pcg_spec(r, ref=True)
    tdt = torch.float32 if r.prec == "f32" else torch.float64

    def ref_at_the_top(sol, big, before, small):
        b = spec.B - 1
        d = b % spec.D
        assert b * big["S"].shape[1] * big["S"].element_size() < 2 ** 32 < (b + 1) * big["S"].shape[1] * big["S"].element_size()       # (it straddles the line)
        outs = []
        for src, row in ((big, b), (before, d)):
            lam = before["lambda"][d].clone()
            rr, pp, vt, et = filled(r.N * r.n, tdt), filled(r.N * r.n, tdt), filled(r.N, tdt), filled(r.N, tdt)
            it, ex = filled(1, torch.int32), filled(1, torch.uint8)
            keep = src["S"][row].clone(), src["Pinv"][row].clone(), src["gamma"][row].clone()
            getattr(sol, "solve_ref" if r.prec == "f32" else "solve_ref_f64")(src["S"][row], src["Pinv"][row], src["gamma"][row], lam, rr, pp, vt, et, it, ex, 2, 0.0)
            torch.cuda.synchronize()
            for k, name in zip(keep, ("S", "Pinv", "gamma")):
                assert torch.equal(le._bits(k.view(1, -1)), le._bits(src[name][row].view(1, -1))), f"12-argument entry: '{name}' modified"
            outs.append([le._bits(t.view(1, -1)).cpu().numpy() for t in (lam, rr, pp, it, ex, vt, et)])
        for name, top, orig in zip(("lambda", "r", "p", "iters", "exit", "v_temp", "eta_new_temp"), *outs):
            assert np.array_equal(top, orig), f"{spec.label}: 12-argument entry on trajectory {b}: '{name}' differs from the call on its original"
        lam, rr, pp, it, ex, vt, et = outs[0]
        assert int(it[0, 0]) == 2 and int(ex[0, 0]) == 1
        assert (vt == -1).all() and (et == -1).all()                 # left untouched
        assert not (rr == -1).any() and not (pp == -1).any()         # written whole
        assert not np.array_equal(lam, le._bits(before["lambda"][d].view(1, -1)).cpu().numpy())
    row_solve(r, spec, ref_at_the_top)
