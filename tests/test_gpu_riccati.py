"""GPU: mpcg_riccati_gains(_f64) — the Riccati feedback gains of include/mpcg_riccati.h — against the numpy restatement tests/riccati_ref.py on the
smallest shapes at which each thing can break (riccati_ref.CASES), on blocks mpcg_generate_kkt made for the iiwa, and for what the contract
promises bit for bit: rho per trajectory, graph replay, batch position, reproducibility, containment, extents, the refusals; and against the
library's own QP solve (Schur formation, block solve, dz in double), whose solution's sensitivity to x_k the gains are.

TOLERANCE.  Per knot ||K_gpu - K64||_max / max(1, ||K64||_max) <= 16 max(e_ref, 2.2e-16), e_ref being float64 against 80-bit arithmetic of the
restatement ON THE SAME INPUTS, computed here: the kernel sums in another order and fuses multiply-adds, both a multiple of the same amplification
through the recursion; one decimal digit of room covers order effects and nothing more.  With e_ref < 6e-11 (asserted) no case passes above 1e-9.
The float entry adds the single rounding of the store, 2^-24 |K64|, element-wise.
Measured (MI355X): DESIGN.md §3.19."""
import ctypes as C

import numpy as np
import pytest
import torch

import arena
import containment
import riccati_ref as rr
from mpcgpu_amd import _lib, gain_blocks, iiwa

pytestmark = pytest.mark.gpu
NPDT = {torch.float64: np.float64, torch.float32: np.float32}
DTYPES = [torch.float64, torch.float32]
ids = lambda c: "x".join(map(str, c))


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, NPDT[dt])).cuda()


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)


_solvers = {}


def solver(n, m, N, B):
    """One handle per shape for the whole module (the entry keeps nothing on it)."""
    from mpcgpu_amd import PcgSolver
    key = (n, m, N, B)
    if key not in _solvers:
        _solvers[key] = PcgSolver(N, max_batch=B, state_size=n, control_size=m)
    return _solvers[key]


_refs = {}


def reference(key, G, Cd, n, m, N, rho):
    """(e_ref, K64 [B, N-1, m, n]) of host arrays G, Cd [B, ...] with rho a float or one per trajectory; computed once per key, never changed."""
    if key not in _refs:
        B = G.shape[0]
        rhos = np.broadcast_to(np.asarray(rho, np.float64), (B,))
        out = [rr.e_ref(G[b], Cd[b], n, m, N, rhos[b]) for b in range(B)]
        K64 = np.stack([k for _, k in out])
        K64.setflags(write=False)
        _refs[key] = (max(e for e, _ in out), K64)
    return _refs[key]


def check_against_reference(K, e_ref, K64, dt, tag):
    """K: flat [B, (N-1) m n] from the device (tensor or host copy).  The bound of the module docstring; prints the figures before it asserts."""
    B, N1, m, n = K64.shape
    K = K.cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)
    got = np.swapaxes(K.astype(np.float64).reshape(B, N1, n, m), -1, -2)
    assert e_ref < rr.E_REF_MAX, (tag, e_ref)
    rel = 16 * max(e_ref, rr.EPS64)
    scale = np.maximum(1, np.abs(K64).reshape(B, N1, -1).max(axis=2))[..., None, None]
    err = np.abs(got - K64)
    store = 2.0 ** -24 * np.abs(K64) if dt == torch.float32 else 0.0
    worst = float((err / scale).max())
    print(f"{tag} {str(dt)[6:]}: e_ref {e_ref:.3g}, bound {rel:.3g}, observed {worst:.3g}" + (" (before the store rounding allowance)" if dt == torch.float32 else ""))
    assert np.isfinite(got).all(), tag
    assert (err <= rel * scale + store).all(), (tag, worst, rel)


def as_entry_sees(rho, dt):
    """The scalar rho as the entry of dtype dt receives it: the float entry takes a float (an input rounded to float like the arrays)."""
    return float(NPDT[dt](rho))


def case_arrays(n, m, N, B, dt):
    G, Cd = rr.make_case(n, m, N, B, NPDT[dt])
    return G, Cd, dev(G, dt), dev(Cd, dt)


# ---- 1. against the reference: every shape, both entries ----
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", rr.ALL_CASES, ids=ids)
def test_against_reference(case, dt):
    n, m, N, B = case
    G, Cd, dG, dC = case_arrays(n, m, N, B, dt)
    e_ref, K64 = reference((case, dt), G, Cd, n, m, N, as_entry_sees(rr.RHO, dt))
    sol = solver(14 if case == (14, 3, 4, 3) else n, 7 if case == (14, 3, 4, 3) else m, N, B)       # (the foreign m on a handle tuned for 14 x 7)
    G0, C0 = dG.clone(), dC.clone()
    K = sol.riccati_gains(dG, dC, rr.RHO, control_size=m)
    torch.cuda.synchronize()
    assert K.shape == (B, (N - 1) * m * n) and K.dtype == dt
    assert torch.equal(dG, G0) and torch.equal(dC, C0)
    check_against_reference(K, e_ref, K64, dt, f"{case}")


@pytest.fixture(scope="module")
def iiwa_blocks():
    """G, C of three iiwa tracking windows at 32 knots as mpcg_generate_kkt(_f64) leaves them on the device, and their host copies."""
    from mpcgpu_amd import Plant
    N, B = 32, 3
    xu, goals, xs = iiwa.random_windows(N, B, 41)
    sol, plant, out = solver(14, 7, N, B), Plant(), {}
    for dt in DTYPES:
        G, Cd, _, _ = sol.generate_kkt(plant, dev(goals.reshape(B, -1), dt), dev(xs, dt), dev(xu, dt), iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(N))
        torch.cuda.synchronize()
        out[dt] = (G, Cd, G.cpu().numpy(), Cd.cpu().numpy())
    return sol, out


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_iiwa_blocks_against_reference(iiwa_blocks, dt):
    """Realistic conditioning: the very numbers the device generated go to the restatement; e_ref < 6e-11 is asserted on them."""
    sol, blocks = iiwa_blocks
    dG, dC, G, Cd = blocks[dt]
    e_ref, K64 = reference(("iiwa", dt), G, Cd, 14, 7, 32, as_entry_sees(rr.RHO, dt))
    K = sol.riccati_gains(dG, dC, rr.RHO)
    torch.cuda.synchronize()
    check_against_reference(K, e_ref, K64, dt, "iiwa (14, 7, 32, 3)")


# ---- 2. rho per trajectory, and a captured graph that follows it ----
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", [(14, 7, 3, 5), (6, 3, 5, 5)], ids=ids)
def test_rho_vector_is_the_scalar_call_bit_for_bit(case, dt):
    n, m, N, B = case
    _, _, dG, dC = case_arrays(n, m, N, B, dt)
    sol = solver(n, m, N, B)
    rhos = [1e-3, 1e-1, 1.0, 0.0, 37.5]
    d_rho = torch.tensor(rhos, dtype=dt, device="cuda")
    K = sol.riccati_gains(dG, dC, d_rho)
    for b, r in enumerate(d_rho.cpu().numpy().tolist()):               # (the float entry's scalar: the float the vector holds)
        Ks = sol.riccati_gains(dG, dC, r)
        assert np.array_equal(bits(K[b]), bits(Ks[b])), (b, r)
    assert len({bits(K[b]).tobytes() for b in range(B)}) == B          # (and rho reaches the result)

    # a graph captured with the vector follows what the vector holds when it replays
    Kg = torch.zeros_like(K)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        sol.riccati_gains(dG, dC, d_rho, K=Kg)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(Kg), bits(K))
    d_rho.copy_(torch.tensor(rhos[::-1], dtype=dt, device="cuda"))
    want = sol.riccati_gains(dG, dC, d_rho.clone())
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(Kg), bits(want)) and not np.array_equal(bits(Kg), bits(K))


# ---- 3. independence of the batch position, reproducibility ----
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", [(14, 7, 33, 5), (13, 5, 4, 5), (14, 3, 4, 3), (18, 18, 3, 2)], ids=ids)
def test_batch_position_and_reproducibility(case, dt):
    """((18, 18): the 16-lane tail behind the run-time build's prefetch.)"""
    n, m, N, B = case
    _, _, dG, dC = case_arrays(n, m, N, B, dt)
    sol = solver(n, m, N, B)
    K = sol.riccati_gains(dG, dC, rr.RHO)
    assert np.array_equal(bits(sol.riccati_gains(dG, dC, rr.RHO)), bits(K))
    for b in range(B):
        alone = sol.riccati_gains(dG[b:b + 1].clone(), dC[b:b + 1].clone(), rr.RHO)
        assert np.array_equal(bits(alone), bits(K[b])), b
    perm = torch.tensor(list(range(B))[::-1], device="cuda")
    assert np.array_equal(bits(sol.riccati_gains(dG[perm].contiguous(), dC[perm].contiguous(), rr.RHO)), bits(K[perm]))


# ---- 4. containment ----
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", [(14, 7, 5, 3), (6, 3, 5, 3)], ids=ids)
def test_a_bad_trajectory_harms_no_neighbour(case, dt):
    """Trajectory 1 of 3 all NaN, all Inf, all zero (a singular H_uu at rho = 0), in G, in C and in both: 0 and 2 keep the bits of the healthy
    call, and the call returns."""
    n, m, N, B = case
    G, Cd, _, _ = case_arrays(n, m, N, B, dt)
    sol = solver(n, m, N, B)

    def run(Gh, Ch, rho):
        K = sol.riccati_gains(dev(Gh, dt), dev(Ch, dt), rho)
        torch.cuda.synchronize()
        return {"K": K.cpu().numpy()}
    fills = {"nan": np.nan, "inf": np.inf, "zero": 0.0}
    for rho in (rr.RHO, 0.0):
        clean = run(G, Cd, rho)
        assert np.isfinite(clean["K"]).all()
        for label, v in fills.items():
            fill = lambda a, v=v: np.full_like(a, v)
            for which in ("G", "C", "GC"):
                Gb = containment.poison(G, (1,), fill) if "G" in which else G
                Cb = containment.poison(Cd, (1,), fill) if "C" in which else Cd
                out = run(Gb, Cb, rho)
                containment.check(clean, out, (1,), entry=f"riccati_gains {case} [{which} <- {label}, rho {rho}]")
                if which == "GC" and (label != "zero" or rho == 0.0):
                    assert not np.isfinite(out["K"][1]).all(), (label, rho)        # (the poison arrived: 0 / 0 at rho = 0)


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", [(14, 7, 4, 6), (13, 5, 4, 6)], ids=ids)
def test_containment_sweep(case, dt):
    """tests/containment.py's sweep, as every other entry's: six trajectories, the sets {1}, {5}, {0, 3}; G and C with a
    NaN and an Inf at the first, the last and a middle element, the whole trajectory NaN, a block of +-3e38 / +-1e308 that overflows inside
    the kernel, all zeros; one rho[b] NaN.  K of every healthy trajectory carries the bits of the clean call.  Both builds of the kernel."""
    from test_gpu_containment_linsys import runner
    n, m, N, B = case
    assert B == containment.B
    G, Cd, _, _ = case_arrays(n, m, N, B, dt)
    sol = solver(n, m, N, B)
    inputs = {"G": G, "C": Cd, "rho": np.array([1e-3, 0.5, 10.0, 3e-2, 1.7, 1e-3], NPDT[dt])}
    run = runner(lambda d: sol.riccati_gains(d["G"], d["C"], d["rho"], K=d["K"]), {"K": ((B, (N - 1) * m * n), NPDT[dt])})
    tag = f"riccati_gains {case} {str(dt)[6:]}"
    assert np.isfinite(run(inputs)["K"]).all()
    containment.sweep(tag, inputs, ["G", "C"], run, matrices=("G", "C"), blocks={"G": n * n, "C": n * n})
    containment.sweep(tag, inputs, ["rho"], run, only=("nan_one@first",))


# ---- 5. arena: extents, alignment, const inputs, every element of K written ----
@pytest.mark.parametrize("mode", arena.MODES)
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("case", [(14, 7, 4, 3), (13, 5, 4, 3), (17, 17, 3, 2), (34, 32, 3, 2)], ids=ids)
def test_arena(case, dt, mode):
    """((34, 32): the first shape above 64 KiB of LDS, through both layouts.)"""
    n, m, N, B = case
    G, Cd, _, _ = case_arrays(n, m, N, B, dt)
    sol = solver(n, m, N, B)
    npdt = NPDT[dt]
    specs = [arena.spec("G", npdt, G.size, "in", knot=n * n + m * m, traj=G.shape[1]),
             arena.spec("rho", npdt, B, "in"),
             arena.spec("K", npdt, B * (N - 1) * m * n, "out", knot=m * n, traj=(N - 1) * m * n),
             arena.spec("C", npdt, Cd.size, "in", knot=n * n + n * m, traj=Cd.shape[1])]
    rho = np.array([1e-3, 1e-1, 1.0][:B], npdt)

    def call(a):
        sol.riccati_gains(a["G"].view(B, -1), a["C"].view(B, -1), a["rho"], K=a["K"].view(B, -1))
    got = arena.both_ways(specs, mode, {"G": G, "C": Cd, "rho": rho}, call, tag=f"riccati_gains {case}")
    e_ref, K64 = reference((case, dt, "arena"), G, Cd, n, m, N, rho.astype(np.float64))
    check_against_reference(got["K"], e_ref, K64, dt, f"arena {case}")


# ---- 6. the refusals: every MPCG_ERR_* row, nothing written ----
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_error_table(dt):
    n, m, N, B = 14, 7, 4, 3
    _, _, dG, dC = case_arrays(n, m, N, B, dt)
    sol = solver(n, m, N, B)
    lib, h = sol.lib, sol._h
    entry = "mpcg_riccati_gains" + ("_f64" if dt == torch.float64 else "")
    fn = getattr(lib, entry)
    K = torch.full((B, (N - 1) * m * n), float("nan"), dtype=dt, device="cuda")
    d_rho = torch.full((B,), 1e-3, dtype=dt, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    INV, UNS, OK = _lib.MPCG_ERR_INVALID, _lib.MPCG_ERR_UNSUPPORTED, _lib.MPCG_OK

    def refused(rc, code, handle=h):
        assert rc == code
        msg = lib.mpcg_last_error(handle).decode()
        assert msg.startswith(entry + ":"), msg
        torch.cuda.synchronize()
        assert torch.isnan(K).all(), msg                                  # nothing written
    refused(fn(None, m, p(dG), p(dC), 1e-3, None, p(K), B, st), INV, handle=None)
    refused(fn(h, m, None, p(dC), 1e-3, None, p(K), B, st), INV)
    refused(fn(h, m, p(dG), None, 1e-3, None, p(K), B, st), INV)
    refused(fn(h, m, p(dG), p(dC), 1e-3, None, None, B, st), INV)
    refused(fn(h, 0, p(dG), p(dC), 1e-3, None, p(K), B, st), INV)
    refused(fn(h, n + 1, p(dG), p(dC), 1e-3, None, p(K), B, st), INV)
    refused(fn(h, m, p(dG), p(dC), 1e-3, None, p(K), B + 1, st), INV)
    for bad in (float("nan"), float("inf"), -1e-3):
        refused(fn(h, m, p(dG), p(dC), bad, None, p(K), B, st), INV)
    # with d_rho the scalar is not read
    assert fn(h, m, p(dG), p(dC), float("nan"), p(d_rho), p(K), B, st) == OK
    torch.cuda.synchronize()
    assert torch.isfinite(K).all()
    K.fill_(float("nan"))
    # batch 0: MPCG_OK, nothing launched.  (The knot_points == 1 row cannot be reached: mpcg_create refuses a handle of fewer than two knots.)
    assert fn(h, m, p(dG), p(dC), 1e-3, None, p(K), 0, st) == OK
    torch.cuda.synchronize()
    assert torch.isnan(K).all()
    # LDS: 8 (LD^2 + 2 LD (n + m) + LM (m + 2 n)) bytes against 160 KiB — (64, 28) is the last that fits at 64 states, (64, 29) the first that does not
    big = solver(64, 29, 2, 1)
    for mm, code in ((28, OK), (29, UNS), (64, UNS)):
        eye = lambda k: torch.eye(k, dtype=dt, device="cuda").reshape(-1)
        Gb = torch.cat([eye(64), eye(mm), eye(64)])                         # Q_0, R_0, Q_1
        Cb = torch.zeros((64 * 64 + 64 * mm), dtype=dt, device="cuda")
        Kb = torch.full((mm * 64,), float("nan"), dtype=dt, device="cuda")
        rc = getattr(big.lib, entry)(big._h, mm, p(Gb), p(Cb), 1e-3, None, p(Kb), 1, st)
        torch.cuda.synchronize()
        assert rc == code, (mm, rc, big.last_error())
        if code == UNS:
            msg = big.last_error()
            assert msg.startswith(entry + ":") and "160 KiB" in msg and torch.isnan(Kb).all()
        else:
            assert (Kb == 0).all()                                           # A = B = 0: K = -H_uu^-1 0
    with pytest.raises(_lib.MpcgError) as e:
        sol.riccati_gains(dG, dC, float("nan"))
    assert e.value.code == INV and entry + ":" in str(e.value)


# ---- 7. the Python wrapper ----
def test_python_wrapper():
    n, m, N, B = 6, 3, 5, 5
    G, Cd, dG, dC = case_arrays(n, m, N, B, torch.float64)
    sol = solver(n, m, N, B)
    K64 = sol.riccati_gains(dG, dC, rr.RHO)
    K32 = sol.riccati_gains(dG.float(), dC.float(), rr.RHO)
    assert K64.dtype == torch.float64 and K32.dtype == torch.float32 and K64.shape == K32.shape == (B, (N - 1) * m * n)
    assert not torch.equal(K32.double(), K64) and torch.allclose(K32.double(), K64, rtol=1e-4, atol=1e-4)       # two entries, one answer
    for args in ((dG.float(), dC), (dG, dC.float()), (dG, dC, torch.full((B,), 1e-3, device="cuda")), (dG.half(), dC.half())):
        with pytest.raises(TypeError):
            sol.riccati_gains(*(args if len(args) == 3 else args + (rr.RHO,)))
    with pytest.raises(TypeError):
        sol.riccati_gains(dG, dC, rr.RHO, K=torch.empty(B, (N - 1) * m * n, device="cuda"))
    with pytest.raises(ValueError):
        sol.riccati_gains(dG[:, :-1].contiguous(), dC, rr.RHO)
    out = torch.empty_like(K64)
    assert sol.riccati_gains(dG, dC, rr.RHO, K=out) is out and torch.equal(out, K64)
    # gain_blocks: a view [B, N-1, m, n], K_view[b, k] @ dx the reference product
    V = gain_blocks(K64, n, m)
    assert V.shape == (B, N - 1, m, n) and V.data_ptr() == K64.data_ptr()
    _, Kref = reference(((n, m, N, B), torch.float64), G, Cd, n, m, N, rr.RHO)
    dx = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
    for b in (0, B - 1):
        for k in (0, N - 2):
            np.testing.assert_allclose((V[b, k] @ dx).cpu().numpy(), Kref[b, k] @ dx.cpu().numpy(), rtol=0, atol=1e-12)


# ---- 8. the gains are the sensitivity of the library's own QP solve ----
def sensitivity_check(tag, k0, n, m, N, rho, max_bound=None):
    """k0: a synth.KKT of one trajectory in float64.  K from mpcg_riccati_gains_f64 on its packed blocks; dz for c and for c perturbed at knot 1 by
    mpcg_form_schur_f64 -> mpcg_block_solve_f64 -> mpcg_compute_dz_f64 on clones of G.  Both residuals of riccati_ref.feedback_residuals within
    64 cond(KKT) 2.2e-16, cond computed here; first for a dense float64 solve on the host, which must be inside the bound by itself.
    max_bound: the bound must lie below it, else None is returned before anything is asserted (the caller raises rho)."""
    from mpcgpu_amd import synth
    from test_generic_producers_cpu import dense_kkt_solve
    k1 = rr.perturbed(k0, 901)
    G, Cd, g, c0 = synth.pack_kkt_dense(k0, np.float64)
    c1 = synth.pack_kkt_dense(k1, np.float64)[3]
    dz0, _, Cm = dense_kkt_solve(k0, 0, rho)
    dz1, _, _ = dense_kkt_solve(k1, 0, rho)
    cond = rr.kkt_cond(k0, rho, Cm)
    tol = 64 * cond * rr.EPS64
    print(f"{tag} rho {rho:g}: cond(KKT) {cond:.3g}, bound {tol:.3g}")
    if max_bound is not None and not tol < max_bound:
        return None
    sol = solver(n, m, N, 1)
    dG, dC, dg = (dev(a, torch.float64) for a in (G, Cd, g))
    K = sol.riccati_gains(dG, dC, rho, control_size=m)                  # (before the formation overwrites G with its block inverses)
    torch.cuda.synchronize()
    K = np.swapaxes(K.cpu().numpy().reshape(N - 1, n, m), -1, -2)
    res = rr.feedback_residuals(dz0, dz1, K, k0)
    print(f"{tag} rho {rho:g}: host dense solve, feedback {res[0]:.3g} dynamics {res[1]:.3g}")
    assert max(res) <= tol, (tag, "the host dense solve", res, tol)

    def device_solve(c):
        Gc = dG.clone()
        S, _, gamma = sol.form_schur(Gc, dC, dg, dev(c, torch.float64), rho, "ss", control_size=m)
        lam = sol.block_solve(S, gamma)
        dz = sol.compute_dz(Gc, dC, dg, lam, control_size=m)
        torch.cuda.synchronize()
        return dz.cpu().numpy()[0]
    assert torch.equal(dG, dev(G, torch.float64))
    res = rr.feedback_residuals(device_solve(c0), device_solve(c1), K, k0)
    print(f"{tag} rho {rho:g}: device solve, feedback {res[0]:.3g} dynamics {res[1]:.3g}")
    assert max(res) <= tol, (tag, "the device solve", res, tol)
    return cond, tol, res


@pytest.mark.parametrize("n,m,N", [(14, 7, 9), (13, 5, 6), (3, 2, 5), (17, 17, 4)], ids=lambda v: str(v))
def test_gains_are_the_sensitivity_of_the_device_solve(n, m, N):
    """K from the device against what the library's own direct path (Schur formation, block solve, dz; all double) does to a perturbation of c
    in knot 1: du_k = K_k dx_k and the dynamics for every k >= 1.  The two code paths read rho and the packed G and C independently."""
    from test_generic_producers_cpu import make_kkt_nm
    assert sensitivity_check(f"({n}, {m}, {N})", make_kkt_nm(N, 1, 900 + N, n, m), n, m, N, rr.RHO) is not None


def test_gains_are_the_sensitivity_of_the_device_solve_on_iiwa_blocks():
    """The same on the blocks mpcg_generate_kkt_f64 makes of one iiwa tracking window at 8 knots.  cond(KKT) comes from those blocks and is not
    known in advance: rho is raised from 1e-3 by decades, to 1e-1 at most, until 64 cond 2.2e-16 < 1e-6 (DESIGN.md section 3.19 records the
    value this takes)."""
    from mpcgpu_amd import Plant
    N = 8
    xu, goals, xs = iiwa.random_windows(N, 1, 41)
    dt = torch.float64
    G, Cd, g, c = solver(14, 7, N, 1).generate_kkt(Plant(), dev(goals.reshape(1, -1), dt), dev(xs, dt), dev(xu, dt), iiwa.TIMESTEP, iiwa.QD_COST, iiwa.r_cost(N))
    torch.cuda.synchronize()
    k0 = rr.kkt_of_packed(*(t.cpu().numpy()[0] for t in (G, Cd, g, c)), 14, 7, N)
    for rho in (1e-3, 1e-2, 1e-1):
        out = sensitivity_check("iiwa (14, 7, 8)", k0, 14, 7, N, rho, max_bound=1e-6)
        if out is not None:
            return
    raise AssertionError("no rho up to 1e-1 brings 64 cond(KKT) 2.2e-16 below 1e-6 on the iiwa blocks")
