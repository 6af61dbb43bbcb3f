"""GPU: non-finite containment of the linear-system stage — mpcg_form_schur(_rhov)(_f64), mpcg_compute_dz(_f64), mpcg_block_solve(_f64),
mpcg_bt_spmv, mpcg_bd_to_csr_lowertri and the batched PCG entries in every kernel family of the launch plan — and the one handle-wide effect
a non-finite matrix has, the symmetry latch, pinned as it is.

Six trajectories; one input array of trajectories {1}, {5} or {0, 3} is poisoned (tests/containment.py: a NaN or an Inf at the first, the last
or a middle element, the whole trajectory NaN, a block of finite values that overflow inside the kernel, all-zero matrices), and every output
of every other trajectory must carry the bits of the same call on healthy data.  No tolerance anywhere: the clean call is what the suites of
each entry pin to the float64 oracle.  Every spin and loop of these kernels is bounded by a host argument (containment table)."""
import functools

import numpy as np
import pytest
import torch

import containment as ct
import generic_pcg_cases as gc
from mpcgpu_amd import synth
from test_generic_producers_cpu import make_kkt_nm

pytestmark = pytest.mark.gpu
n, m, B = 14, 7, ct.B
DTYPES = [np.float32, np.float64]
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}
SENTINEL = -7                                                  # integer outputs start from it: "never written" stays visible


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()                  # (a copy: the shared inputs are read-only)


def solver(N, opts=(), nn=n, mm=None):
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(N, max_batch=B, state_size=nn, control_size=mm)
    for key, value in opts:
        sol.set_option(key, value)
    return sol


def runner(call, outputs, after=None):
    """run(inputs) for containment.sweep: every input on the device, every pure output — outputs = {name: (shape, numpy dtype)} — filled with
    NaN (floats) or SENTINEL (integers), call(d), and the arrays named in `outputs` back on the host (a name that is also an input: in/out)."""
    def run(inputs):
        d = {k: dev(v) for k, v in inputs.items()}
        for name, spec in outputs.items():
            if spec is not None:
                shape, dt = spec
                dt = np.dtype(dt)
                d[name] = torch.full(shape, float("nan") if dt.kind == "f" else SENTINEL, dtype=TORCH[dt], device="cuda")
        call(d)
        torch.cuda.synchronize()
        if after is not None:
            after()
        return {name: d[name].cpu().numpy() for name in outputs}
    return run


def ids(opts):
    return "-".join(f"{k}{v}" for k, v in opts) or "default"


def frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def kkt(nn, mm, N, dtype):
    """(G, C, g, c) of six trajectories, read-only and shared."""
    k = synth.make_kkt(N, B, 4100 + N) if (nn, mm) == (n, m) else make_kkt_nm(N, B, 9, nn, mm)
    return frozen(*synth.pack_kkt_dense(k, dtype))


@functools.lru_cache(maxsize=None)
def schur(N, dtype, pc="ss", unused_nan=False):
    """(S, Pinv, gamma, lambda0) of six 14-state trajectories; under block-Jacobi the off-diagonal blocks of Pinv are NaN (never read)."""
    S, P, g = synth.form_schur(synth.make_kkt(N, B, 4200 + N), precond=pc, dtype=dtype, poison_unused=unused_nan)
    if pc == "jacobi":
        Pb = P.reshape(B, N, 3, n * n)
        Pb[:, :, 0] = np.nan
        Pb[:, :, 2] = np.nan
    lam0 = (0.1 * np.random.default_rng([n, N]).standard_normal((B, n * N))).astype(dtype)
    return frozen(S, P, g, lam0)


# ---- formation ----
# (N, state, control, options): the walking kernel at its automatic chunk and at forced chunks whose wavefronts of four chunks straddle
# trajectories (N = 9: 8 block rows, so 8, 2 and 2 chunks per trajectory), the LDS kernels by both switches, and a generic shape
ROUTES = [(3, n, m, ()), (9, n, m, ()), (9, n, m, (("schur_chunk", 1),)), (9, n, m, (("schur_chunk", 4),)), (9, n, m, (("schur_chunk", 5),)),
          (9, n, m, (("schur_dpp", 0),)), (9, n, m, (("producers_generic", 1),)), (9, 6, 3, ())]


@pytest.mark.parametrize("rhov", [False, True], ids=["rho", "rhov"])
@pytest.mark.parametrize("precond", ["ss", "jacobi", "none"])
@pytest.mark.parametrize("N,nn,mm,opts", ROUTES, ids=[f"N{r[0]}-{r[1]}x{r[2]}-{ids(r[3])}" for r in ROUTES])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_form_schur(dtype, N, nn, mm, opts, precond, rhov):
    """S, Pinv, gamma and the overwritten G of the healthy trajectories, with G, C, g, c poisoned in turn and — the tensor form — one rho[b] NaN.
    Under MPCG_PRECOND_NONE Pinv is never written, under block-Jacobi its off-diagonal blocks are not: the NaN fill equals itself."""
    G, Cd, g, c = kkt(nn, mm, N, dtype)
    sol = solver(N, opts, nn, mm)
    inputs = {"G": G, "C": Cd, "g": g, "c": c}
    if rhov:
        inputs["rho"] = np.array([1e-3, 0.5, 10.0, 3e-2, 1.7, 1e-3], dtype)

    def call(d):
        sol.form_schur(d["G"], d["C"], d["g"], d["c"], d["rho"] if rhov else 1e-3, precond, S=d["S"], Pinv=d["Pinv"], gamma=d["gamma"], control_size=mm)
    M = (B, 3 * nn * nn * N)
    run = runner(call, {"S": (M, dtype), "Pinv": (M, dtype), "gamma": ((B, nn * N), dtype), "G": None})
    tag = f"form_schur{'_rhov' if rhov else ''} {np.dtype(dtype).name} {nn}x{mm} N={N} {ids(opts)} {precond}"
    ct.sweep(tag, inputs, ["G", "C", "g", "c"], run, matrices=("G", "C"), blocks={"G": nn * nn, "C": nn * nn, "g": nn, "c": nn})
    if rhov:
        ct.sweep(tag, inputs, ["rho"], run, only=("nan_one@first",))


# ---- dz ----
@pytest.mark.parametrize("dpp", [1, 0])
@pytest.mark.parametrize("N", [3, 9])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_compute_dz(dtype, N, dpp):
    """Four knots per wavefront ("dz_dpp" = 1) and the LDS kernel; G^-1, C, g and lambda poisoned in turn."""
    G, Cd, g, _ = kkt(n, m, N, dtype)
    lam = (0.1 * np.random.default_rng(N).standard_normal((B, n * N))).astype(dtype)
    sol = solver(N, (("dz_dpp", dpp),))
    run = runner(lambda d: sol.compute_dz(d["Ginv"], d["C"], d["g"], d["lambda"], dz=d["dz"]), {"dz": ((B, (n + m) * N - m), dtype)})
    ct.sweep(f"compute_dz {np.dtype(dtype).name} N={N} dz_dpp={dpp}", {"Ginv": G, "C": Cd, "g": g, "lambda": lam}, ["Ginv", "C", "g", "lambda"], run,
             matrices=("Ginv", "C"), blocks={"Ginv": n * n, "C": n * n})


# ---- block solve ----
SWEEPS = [(np.float32, (("block_solve_wide", 0),)), (np.float32, (("block_solve_wide", 1),)), (np.float32, (("block_solve_f64", 1),)), (np.float64, ())]


@pytest.mark.parametrize("N", [3, 9, 33])
@pytest.mark.parametrize("dtype,opts", SWEEPS, ids=["f32-four-per-wavefront", "f32-wide", "f32-f64-inside", "f64"])
def test_block_solve(dtype, opts, N):
    """Four trajectories per wavefront, one per 16-lane DPP row (dead rows redo trajectory 5), the wide kernel and the double sweeps; S and gamma
    poisoned, zero_all included: a singular pivot block, 0 / 0 in the Gauss-Jordan scheme of one row."""
    S, _, gam, _ = schur(N, dtype)
    sol = solver(N, opts)
    run = runner(lambda d: sol.block_solve(d["S"], d["gamma"], lam=d["lambda"]), {"lambda": ((B, n * N), dtype)})
    ct.sweep(f"block_solve {np.dtype(dtype).name} N={N} {ids(opts)}", {"S": S, "gamma": gam}, ["S", "gamma"], run, matrices=("S",), blocks={"S": n * n})


# ---- the building blocks ----
@pytest.mark.parametrize("cols", [3, 1])
def test_bt_spmv(cols):
    """y = M x over the rows of the whole batch; M and x of one trajectory poisoned."""
    N = 9
    S, _, _, x = schur(N, np.float32)
    sol = solver(N)
    run = runner(lambda d: sol.bt_spmv(d["M"], d["x"], y=d["y"], cols=cols), {"y": ((B, n * N), np.float32)})
    ct.sweep(f"bt_spmv cols={cols}", {"M": S, "x": x}, ["M", "x"], run, matrices=("M",), blocks={"M": n * n})


def test_bd_to_csr_lowertri():
    N = 9
    S = schur(N, np.float32)[0]
    sol = solver(N)
    def call(d):
        d["val"] = sol.bd_to_csr_lowertri(d["S"], 1.0)
    run = runner(call, {"val": None})
    ct.sweep("bd_to_csr_lowertri", {"S": S}, ["S"], run, matrices=("S",), blocks={"S": n * n})


# ---- PCG: every family of the launch plan, at a horizon and with the pinning options of its rows in tests/pcg_step_cases.py ----
MAX_ITER, EXIT_TOL = 12, 1e-6
# (precision, state, control, N, family, options); the clustered families (7, 8, 10) at the shortest horizon that table forces them at
PCG_ROWS = [("f32", 13, 5, 9, 3, ()), ("f32", n, m, 17, 5, (("pcg_rpl", 1), ("rpl_waves", 4))), ("f32", n, m, 33, 6, (("pcg_lpk", 1), ("pcg_lqb", 0))),
            ("f32", n, m, 129, 7, ()), ("f32", n, m, 17, 11, (("pcg_lpk", 1), ("pcg_lqb", 1))),
            ("f64", n, m, 100, 3, (("cluster", 0),)), ("f64", n, m, 17, 5, ()), ("f64", n, m, 33, 8, (("pcg_lqk", 0),)), ("f64", n, m, 17, 9, (("pcg_lqk", 1),)),
            ("f64", n, m, 65, 10, ())]


@functools.lru_cache(maxsize=None)
def pcg_system(prec, nn, mm, N, pc):
    dt = {"f32": np.float32, "f64": np.float64}[prec]
    if nn == n:
        return schur(N, dt, pc, True)
    S, P, g = gc.system(nn, mm, N, B, gc.SEED, dt, 1e-3, pc)
    return S, P, g, frozen((0.1 * np.random.default_rng([nn, N]).standard_normal((B, nn * N))).astype(dt))[0]


@pytest.mark.parametrize("pc", ["ss", "jacobi"])
@pytest.mark.parametrize("prec,nn,mm,N,family,opts", PCG_ROWS, ids=[f"{r[0]}-n{r[1]}-N{r[3]}-family{r[4]}" for r in PCG_ROWS])
def test_pcg(prec, nn, mm, N, family, opts, pc):
    """mpcg_pcg_solve / _f64, 12 iterations at most, exit_tol 1e-6, "assume_symmetric" = 1 so that both runs are the same kernel family: lambda,
    the iteration counts and the flags of the healthy trajectories; the family after every run; no cluster ever gives a trajectory up (members
    that disagreed about an exit on non-finite partials would time out at a hand-off); the poisoned trajectories themselves come back with
    iters <= max_iter and a flag of 0 or 1."""
    from mpcgpu_amd import pcg_config
    S, P, g, lam0 = pcg_system(prec, nn, mm, N, pc)
    sol = solver(N, opts + (("assume_symmetric", 1),), nn, mm)
    cfg = pcg_config(pcg_exit_tol=EXIT_TOL, pcg_max_iter=MAX_ITER)
    entry = sol.solve if prec == "f32" else sol.solve_f64
    tag = f"pcg {prec} n={nn} N={N} {pc} family {family}"

    def after():
        assert sol.get_option("last_kernel_family") == family, (tag, sol.get_option("last_kernel_family"))
        assert sol.get_option("cluster_fixups") == 0, tag

    def own(out, pset, case):
        it, ex = out["iters"], out["exits"]
        assert ((0 <= it) & (it <= MAX_ITER)).all() and np.isin(ex, (0, 1)).all(), (case, pset, it, ex)
    run = runner(lambda d: entry(d["S"], d["Pinv"], d["gamma"], d["lambda"], cfg, pc, iters=d["iters"], exits=d["exits"]),
                 {"lambda": None, "iters": ((B,), np.int32), "exits": ((B,), np.uint8)}, after)
    ct.sweep(tag, {"S": S, "Pinv": P, "gamma": g, "lambda": lam0}, ["S", "Pinv", "gamma", "lambda"], run, matrices=("S", "Pinv"),
             blocks={"S": nn * nn, "Pinv": nn * nn, "gamma": nn, "lambda": nn}, own=own)


# ---- the latch, pinned as it is ----
LATCH_N = 33                                                   # a default float handle serves it with a lower-triangle kernel, guarded until the latch resolves


def latch_solver():
    from mpcgpu_amd import PcgSolver
    return PcgSolver(LATCH_N, max_batch=B)


def latch_call(sol, S, P, g, lam0, pc="ss"):
    from mpcgpu_amd import pcg_config
    lam = dev(lam0)
    it, ex = sol.solve(dev(S), dev(P), dev(g), lam, pcg_config(pcg_exit_tol=EXIT_TOL, pcg_max_iter=MAX_ITER), pc)
    torch.cuda.synchronize()
    return {"lambda": lam.cpu().numpy(), "iters": it.cpu().numpy(), "exits": ex.cpu().numpy()}


def with_nan(a, b, N, k, col, e=5):
    """A copy of a bd-layout matrix [B, 3 n n N] with one NaN in block (k, col) of trajectory b."""
    out = np.array(a, copy=True)
    out.reshape(B, N, 3, n * n)[b, k, col, e] = np.nan
    return out


@pytest.mark.parametrize("which,col", [("S", 2), ("S", 0), ("Pinv", 2), ("Pinv", 0)], ids=["S-right", "S-left", "Pinv-right", "Pinv-left"])
def test_a_nan_in_an_off_diagonal_block_closes_the_symmetry_latch_for_the_handle(which, col):
    """include/mpcg.h, NON-FINITE DATA: the ONE handle-wide effect.  A fresh handle with default options whose first call carries a NaN in an
    off-diagonal block of S (or, symmetric stair, of Pinv) of trajectory 1: the check counts it as a violation, "symmetry_state" becomes 2, and
    the healthy trajectories of that call and every trajectory of a second, clean call carry the bits of the same calls on a handle that ran the
    three-column kernels from the start (one whose first call showed it a structurally asymmetric Pinv)."""
    N = LATCH_N
    S, P, g, lam0 = schur(N, np.float32)
    k = 4 if col == 2 else 5
    Sb, Pb = (with_nan(S, 1, N, k, col), P) if which == "S" else (S, with_nan(P, 1, N, k, col))
    fresh = latch_solver()
    first = latch_call(fresh, Sb, Pb, g, lam0)
    assert fresh.get_option("symmetry_state") == 2 and "block-symmetric" in fresh.last_error()
    second = latch_call(fresh, S, P, g, lam0)
    assert fresh.get_option("symmetry_state") == 2 and fresh.get_option("last_kernel_family") in (0, 5)
    three = latch_solver()
    Pa = np.array(P, copy=True).reshape(B, N, 3, n * n)
    Pa[:, :, 2] *= 0.9
    latch_call(three, S, Pa.reshape(B, -1), g, lam0)
    assert three.get_option("symmetry_state") == 2
    want_first, want_second = latch_call(three, Sb, Pb, g, lam0), latch_call(three, S, P, g, lam0)
    assert three.get_option("last_kernel_family") == fresh.get_option("last_kernel_family")
    ct.check(want_first, first, (1,), entry=f"first call of a fresh handle, NaN in block ({k}, {col}) of {which}")
    ct.check(want_second, second, (), entry="second, clean call of the latched handle")


@pytest.mark.parametrize("which", ["gamma", "lambda", "S-diagonal", "Pinv-diagonal"])
def test_a_nan_elsewhere_leaves_the_latch_at_block_symmetric(which):
    """A NaN only in gamma, lambda0 or a diagonal block is no symmetry violation: the handle latches "block-symmetric" (1) and stays on its
    lower-triangle kernel."""
    N = LATCH_N
    S, P, g, lam0 = schur(N, np.float32)
    if which == "gamma":
        g = ct.poison(g, (1,), lambda a: ct.nan_one(a, 70))
    elif which == "lambda":
        lam0 = ct.poison(lam0, (1,), lambda a: ct.nan_one(a, 70))
    elif which == "S-diagonal":
        S = with_nan(S, 1, N, 5, 1)
    else:
        P = with_nan(P, 1, N, 5, 1)
    clean = schur(N, np.float32)
    sol, ref = latch_solver(), latch_solver()
    out = latch_call(sol, S, P, g, lam0)
    assert sol.get_option("symmetry_state") == 1 and sol.get_option("last_kernel_family") == 11
    ct.check(latch_call(ref, *clean), out, (1,), entry=f"fresh handle, NaN in {which}")


# ---- the plumbing of these files held to account on the device (tests/test_containment_cpu.py does the same for the helper in numpy) ----
@pytest.mark.parametrize("defect", [None, "select_by_multiplication", "reduction_over_the_batch"])
def test_a_planted_leak_on_the_device_is_caught(defect):
    """An "entry" made of torch kernels through the same runner and sweep: y[b] = x[b] / max |x[b]|, correct as written; with a halo term of the
    next trajectory selected by a factor 0, or the maximum taken over the whole batch, the sweep must fail and name a healthy trajectory."""
    x = np.random.default_rng(17).standard_normal((B, 16)).astype(np.float32)

    def call(d):
        v = d["x"]
        halo = 0.0 * torch.roll(v, -1, 0)[:, :1] if defect == "select_by_multiplication" else torch.zeros_like(v[:, :1])
        scale = v.abs().max() if defect == "reduction_over_the_batch" else v.abs().amax(1, keepdim=True)
        d["y"].copy_(v / scale + halo)
    run = runner(call, {"y": ((B, 16), np.float32)})
    if defect is None:
        assert ct.sweep("torch model", {"x": x}, ["x"], run, matrices=("x",)) == 9 * len(ct.SETS)
    else:
        with pytest.raises(AssertionError, match=r"torch model \[x <- .*array 'y' of healthy trajectory \d .*poisoned trajectory"):
            ct.sweep("torch model", {"x": x}, ["x"], run, matrices=("x",))
