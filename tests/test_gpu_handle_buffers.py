"""GPU: the device buffers a handle makes AFTER mpcg_create — at the first call that needs one, or when a call needs a larger one — through
every stage of their life: made eagerly, refused inside a stream capture (MPCG_ERR_INVALID, "outside the stream capture", nothing launched,
the capture replays), grown eagerly, growth refused inside a capture, and freed by mpcg_destroy whichever of them exist.

Inventory: which test covers (a) the first use, eager; (b) the first use inside a capture; (c) a growth, eager; (d) a growth inside a capture.
"here" = this module; Buffers by their BufId (mpcgpu_amd/csrc/mpcg_handle.hpp).  "-" = the buffer has one size for the handle's life (sized from max_batch), there is no growth.

  BUF_SEAM            (a) every 14 x 7 formation, e.g. test_gpu_schur.py      (b) test_gpu_graph.py::test_first_call_allocations_are_refused_...
                      (c) here: test_seam_buffer_growth                      (d) here: test_seam_buffer_growth
  BUF_STAGING(64)     (a) test_gpu_generic_producers.py::test_form_schur_bit_exact_vs_oracle_at_any_shape
                      (b) test_gpu_generic_producers.py::test_generic_chain_replays_..., test_gpu_rho.py (the _rhov entry),
                          test_gpu_large_producers.py (a 14 x 7 handle's first call past the 31-bit offsets)
                      (c) test_gpu_generic_producers.py::test_a_larger_control_size_regrows_the_staging_buffer
                      (d) here: test_staging_growth_is_refused_inside_a_capture
  BUF_BLOCK           (a) test_gpu_schur.py, test_gpu_graph.py                (b) test_gpu_graph.py::test_first_call_allocations_are_refused_...   (c), (d) -
  BUF_BLOCK64         (a) test_gpu_block_solve_f64.py                         (b) test_gpu_block_solve_f64.py::test_first_f64_call_is_refused_...  (c), (d) -
                      neither licenses the other's captured first call: here, test_the_block_solve_buffers_are_independent
  BUF_MERIT           (a) test_gpu_merit.py, test_gpu_merit_f64.py, test_gpu_xuref.py      (b) test_gpu_merit.py::test_merit_and_step_replay_from_a_hipgraph
                      (c), (d) -        one buffer for the four entries: here, test_merit_scratch_is_shared_by_the_four_entries
  BUF_LAM_BACKUP      (a) test_gpu_cluster.py::test_a_forced_cluster_sizes_its_copy_of_lambda_...   (b) test_gpu_cluster.py::test_a_forced_clusters_first_launch_is_refused_...
                      (c) test_gpu_cluster.py::test_a_forced_cluster_sizes_its_copy_of_lambda_... (float-sized to double-sized)
                      (d) here: test_lambda_copy_growth_is_refused_inside_a_capture (a larger batch of a forced float cluster)
  BUF_CLUSTER64       (a) test_gpu_cluster.py (the first double cluster solve; "reserve_f64")  (b) test_gpu_graph.py::test_a_large_handles_first_double_solve_needs_reserve_f64_...
                      (c), (d) -
  mpcg_destroy        a plain handle is destroyed by every test; with each lazy buffer made, all of them, and during another handle's capture: here,
                      test_destroy_at_every_stage

No test here replays a graph captured before a growth of a buffer it uses, and none forces a double cluster on a horizon of 32 knots or fewer."""
import functools

import numpy as np
import pytest
import torch

from mpcgpu_amd import XuRef, _lib, iiwa, synth

pytestmark = pytest.mark.gpu
n, m = 14, 7
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ff(rows, cols, dtype):
    """[rows, cols] of `dtype` with every byte 0xFF."""
    return torch.full((rows, cols * np.dtype(dtype).itemsize), 0xFF, dtype=torch.uint8, device="cuda").view(TORCH[dtype])


def same_bytes(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def refused(e):
    return e.value.code == _lib.MPCG_ERR_INVALID and "outside the stream capture" in str(e.value)


# ---- 1. the seam buffer grows under a forced short "schur_chunk", outside a capture only ----
def seam_grows(N, B, esz, cus):
    """A one-row-per-chunk call of B trajectories needs more seams than the handle's automatic sizing holds (mpcg_producers.hip, ensure_seam_buffer)."""
    return B * (N - 1) * esz > 8 * max(2 * 24 * cus + B + 4, B * -(-(N - 1) // 16))


@pytest.mark.parametrize("dtype,N", [(np.float32, 128), (np.float64, 65)])
def test_seam_buffer_growth(dtype, N):
    """One handle, max_batch = B: an automatic formation sizes the seam buffer; "schur_chunk" = 1 then asks for B (N - 1) seams, more than that.
    Inside a capture the call is refused and writes nothing; eagerly it grows the buffer and gives the bits of a fresh handle whose first call
    it is; the automatic call after it gives the bits of the one before.  B: the smallest multiple of four that outgrows the automatic sizing
    on this device (200 in float, 196 in double on 256 CUs), from four trajectories repeated."""
    from mpcgpu_amd import PcgSolver
    esz = np.dtype(dtype).itemsize
    probe = PcgSolver(2, max_batch=1)
    cus = probe.get_option("num_cus")
    probe.close()
    B = next(b for b in range(4, 8192, 4) if seam_grows(N, b, esz, cus))
    assert B * N * 3 * n * n * esz < 2 ** 31                 # (the register-resident route)
    G, C, g, c = (dev(a).repeat(B // 4, 1) for a in synth.pack_kkt_dense(synth.make_kkt(N, 4, 4600 + N), dtype))

    def form(sol):
        S, P, gam, dG = ff(B, 3 * n * n * N, dtype), ff(B, 3 * n * n * N, dtype), ff(B, n * N, dtype), G.clone()
        sol.form_schur(dG, C, g, c, 1e-3, "ss", S=S, Pinv=P, gamma=gam)
        torch.cuda.synchronize()
        return S, P, gam, dG

    sol = PcgSolver(N, max_batch=B)
    auto = form(sol)
    assert sol.get_option("last_schur_chunk") == auto_chunk(sol, B, N) > 1
    sol.set_option("schur_chunk", 1)
    assert seam_grows(N, B, esz, sol.get_option("num_cus")), (N, B, sol.get_option("num_cus"))

    S, P, gam, dG = ff(B, 3 * n * n * N, dtype), ff(B, 3 * n * n * N, dtype), ff(B, n * N, dtype), G.clone()
    marker = torch.zeros(4, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        with pytest.raises(_lib.MpcgError) as e:
            sol.form_schur(dG, C, g, c, 1e-3, "ss", S=S, Pinv=P, gamma=gam)
        assert refused(e)
        marker.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert marker.tolist() == [1.0] * 4
    for t in (S, P, gam):
        assert bool((t.view(torch.uint8) == 0xFF).all())
    assert same_bytes(dG, G)

    grown = form(sol)                                        # eager: the buffer grows
    assert sol.get_option("last_schur_chunk") == 1
    fresh = PcgSolver(N, max_batch=B)
    fresh.set_option("schur_chunk", 1)
    first = form(fresh)                                      # a buffer of that size from the start
    assert fresh.get_option("last_schur_chunk") == 1
    for got, want, name in zip(grown, first, ("S", "Pinv", "gamma", "G^-1")):
        assert same_bytes(got, want), name
    assert not same_bytes(grown[3], G) and not bool((grown[0].view(torch.uint8) == 0xFF).all())
    sol.set_option("schur_chunk", 0)
    again = form(sol)
    assert sol.get_option("last_schur_chunk") == auto_chunk(sol, B, N)
    for got, want, name in zip(again, auto, ("S", "Pinv", "gamma", "G^-1")):
        assert same_bytes(got, want), name


def auto_chunk(sol, B, N):
    """The automatic chunk length of a B x N call (mpcg_producers.hip, form_schur_walk)."""
    rows, want, L = B * (N - 1), sol.get_option("num_cus") * 24, 1
    while L < 16 and rows // (2 * L) >= want:
        L *= 2
    return L


# ---- the staging buffer of the LDS formation: a larger control_size inside a capture ----
def test_staging_growth_is_refused_inside_a_capture(orc):
    from mpcgpu_amd import PcgSolver
    from test_gpu_generic_producers import case, check_form
    nn, N, B = 6, 3, 5
    sol = PcgSolver(N, max_batch=B, state_size=nn)
    check_form(sol, nn, 1, N, B, "ss", np.float32)           # sized for control_size 1
    G, C, g, c = (dev(a) for a in case(nn, 6, N, B, 7, np.float32)[1])
    S, P, gam = ff(B, 3 * nn * nn * N, np.float32), ff(B, 3 * nn * nn * N, np.float32), ff(B, nn * N, np.float32)
    dG = G.clone()
    marker = torch.zeros(4, device="cuda")
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        with pytest.raises(_lib.MpcgError, match="mpcg_form_schur") as e:
            sol.form_schur(dG, C, g, c, 1e-3, "ss", S=S, Pinv=P, gamma=gam, control_size=6)
        assert refused(e)
        marker.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert marker.tolist() == [1.0] * 4 and same_bytes(dG, G)
    for t in (S, P, gam):
        assert bool((t.view(torch.uint8) == 0xFF).all())
    check_form(sol, nn, 6, N, B, "ss", np.float32)           # eagerly it grows
    check_form(sol, nn, 1, N, B, "ss", np.float32)


# ---- the copy of lambda of a forced float cluster is sized for the call's batch: a larger batch inside a capture ----
def test_lambda_copy_growth_is_refused_inside_a_capture(orc):
    from mpcgpu_amd import PcgSolver, pcg_config
    from test_gpu_cluster import LAMCOPY_K, LAMCOPY_MAX_BATCH, LAMCOPY_N, lamcopy_solve, lamcopy_system
    sysd = lamcopy_system(orc)
    S, P, g, l0, _, _ = sysd[np.float32]
    dS, dP, dg = dev(S), dev(P), dev(g)
    cfg = pcg_config(pcg_exit_tol=0.0, pcg_max_iter=LAMCOPY_K)
    sol = PcgSolver(LAMCOPY_N, max_batch=LAMCOPY_MAX_BATCH)
    sol.set_option("cluster", 2)
    for _ in range(2):                                       # one trajectory: the copy is made for a batch of one; the second call runs latched
        one = dev(l0[:1].copy())
        sol.solve(dS[:1], dP[:1], dg[:1], one, cfg, "ss")
        torch.cuda.synchronize()
    assert sol.get_option("last_kernel_family") == 7 and sol.get_option("symmetry_state") == 1
    lam = dev(l0.copy())
    marker = torch.zeros(4, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(_lib.MpcgError, match="a cluster launch whose copy of lambda mpcg_create did not size") as e:
            sol.solve(dS, dP, dg, lam, cfg, "ss")
        assert refused(e)
        marker.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert marker.tolist() == [1.0] * 4 and torch.equal(lam, dev(l0))
    lamcopy_solve(sol, sysd, False, 7)                       # eagerly it grows; the answer is checked against the oracle


# ---- 2. BUF_BLOCK and BUF_BLOCK64 are two buffers ----
@pytest.mark.parametrize("eager,captured", [("f32", "f64"), ("f32", "option"), ("f64", "f32"), ("option", "f32")])
def test_the_block_solve_buffers_are_independent(orc, eager, captured):
    """An eager float sweep does not license a captured first double sweep — mpcg_block_solve_f64 or "block_solve_f64" = 1 — nor the other way round."""
    from mpcgpu_amd import PcgSolver
    from test_gpu_block_solve_f64 import system14, want14_f64
    N = 9
    S, g = system14(N)
    B = S.shape[0]
    data = {"f32": (dev(S), dev(g)), "f64": (dev(S.astype(np.float64)), dev(g.astype(np.float64)))}
    want = {"f64": want14_f64(N), "option": want14_f64(N).astype(np.float32), "f32": np.stack([orc.block_solve(S[b], g[b], N) for b in range(B)])}
    sol = PcgSolver(N, max_batch=B)

    def run(kind, lam=None):
        sol.set_option("block_solve_f64", 1 if kind == "option" else 0)
        dS, dg = data["f64" if kind == "f64" else "f32"]
        return sol.block_solve(dS, dg, lam)

    lam = run(eager)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(lam.cpu().numpy(), want[eager])
    out = ff(B, n * N, np.float64 if captured == "f64" else np.float32)
    marker = torch.zeros(4, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(_lib.MpcgError) as e:
            run(captured, out)
        assert refused(e)
        marker.add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert marker.tolist() == [1.0] * 4 and bool((out.view(torch.uint8) == 0xFF).all())
    run(captured, out)                                       # eagerly: made now, and the other sweep's bits are what they were
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want[captured])
    np.testing.assert_array_equal(run(eager).cpu().numpy(), want[eager])


# ---- 3. BUF_MERIT is one buffer for the four merit entries ----
MERIT_ENTRIES = ("f32", "f64", "xuref_f32", "xuref_f64")
MERIT_N, MERIT_B, MERIT_STEPS = 4, 2, [-1.0, -0.25]


@functools.lru_cache(maxsize=None)
def merit_plant():
    from mpcgpu_amd import Plant
    return Plant()


@functools.lru_cache(maxsize=None)
def merit_inputs():
    """Device inputs per dtype (never written) and the plan of the _xuref entries."""
    N, B = MERIT_N, MERIT_B
    xu, goals, xs = iiwa.random_windows(N, B, 4100)
    rng = np.random.default_rng(4101)
    dz = 0.05 * rng.standard_normal(xu.shape)
    plan = 0.5 * rng.standard_normal((N + 1, n + m))
    return {dt: tuple(dev(np.asarray(a, dt)) for a in (goals.reshape(B, -1), xs, xu, dz, plan)) for dt in (np.float32, np.float64)}


def merit_call(sol, entry, out=None):
    dt = np.float64 if entry.endswith("f64") else np.float32
    goals, xs, xu, dz, plan = merit_inputs()[dt]
    args = (merit_plant(), goals, xs, xu, dz, MERIT_STEPS, iiwa.TIMESTEP, 10.0, iiwa.QD_COST, iiwa.r_cost(MERIT_N))
    if entry.startswith("xuref"):
        return sol.compute_merit_xuref(*args, XuRef(plan, ee_cost=0.75, q_cost=0.5), merit=out)
    return sol.compute_merit(*args, merit=out)


@functools.lru_cache(maxsize=None)
def merit_eager():
    """The four entries' merits from eager calls on one handle."""
    from mpcgpu_amd import PcgSolver
    sol = PcgSolver(MERIT_N, max_batch=MERIT_B)
    out = {e: merit_call(sol, e).cpu().numpy() for e in MERIT_ENTRIES}
    assert all(np.isfinite(v).all() for v in out.values())
    assert not np.array_equal(out["f32"], out["xuref_f32"])
    return out


@pytest.mark.parametrize("first", MERIT_ENTRIES)
def test_merit_scratch_is_shared_by_the_four_entries(first):
    """After one eager call of any one of mpcg_compute_merit, _f64, _xuref and _xuref_f64 a first call of each of the other three captures, and
    replays the eager bits."""
    from mpcgpu_amd import PcgSolver
    want = merit_eager()
    sol = PcgSolver(MERIT_N, max_batch=MERIT_B)
    np.testing.assert_array_equal(merit_call(sol, first).cpu().numpy(), want[first])
    others = [e for e in MERIT_ENTRIES if e != first]
    outs = {e: torch.zeros(MERIT_B, len(MERIT_STEPS), device="cuda", dtype=torch.float64 if e.endswith("f64") else torch.float32) for e in others}
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        for e in others:
            merit_call(sol, e, outs[e])
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in outs.values())     # (captured, not run)
    graph.replay()
    torch.cuda.synchronize()
    for e in others:
        np.testing.assert_array_equal(outs[e].cpu().numpy(), want[e], err_msg=e)


# ---- 4. mpcg_destroy with any subset of the lazy buffers ----
DESTROY_N, DESTROY_B = 8, 2


@functools.lru_cache(maxsize=None)
def destroy_inputs():
    """What the makers below read (never written): the KKT blocks per dtype and a float system S, Pinv, gamma."""
    from mpcgpu_amd import PcgSolver
    N, B = DESTROY_N, DESTROY_B
    k = synth.make_kkt(N, B, 4800)
    kkt = {dt: tuple(dev(a) for a in synth.pack_kkt_dense(k, dt)) for dt in (np.float32, np.float64)}
    prep = PcgSolver(N, max_batch=B)
    G, C, g, c = kkt[np.float32]
    S, P, gam = prep.form_schur(G.clone(), C, g, c, 1e-3, "ss", S=torch.zeros(B, 3 * n * n * N, device="cuda"), Pinv=torch.zeros(B, 3 * n * n * N, device="cuda"))
    torch.cuda.synchronize()
    prep.close()
    return kkt, (S, P, gam)


def _form(sol, dt, lds):
    G, C, g, c = destroy_inputs()[0][dt]
    sol.set_option("schur_dpp", 0 if lds else 1)
    S, _, _ = sol.form_schur(G.clone(), C, g, c, 1e-3, "ss")
    sol.set_option("schur_dpp", 1)
    assert sol.get_option("last_schur_chunk") == (0 if lds else 1) and bool(torch.isfinite(S[:, n * n:-n * n]).all())


def _block(sol, dbl):
    S, _, gam = destroy_inputs()[1]
    lam = sol.block_solve(S.double(), gam.double()) if dbl else sol.block_solve(S, gam)
    assert bool(torch.isfinite(lam).all())


def _merit(sol):
    N, B = DESTROY_N, DESTROY_B
    xu8, goals8, xs8 = (dev(np.asarray(a, np.float32)) for a in iiwa.random_windows(N, B, 4900))
    out = sol.compute_merit(merit_plant(), goals8.reshape(B, -1), xs8, xu8, None, [0.0], iiwa.TIMESTEP, 10.0, iiwa.QD_COST, iiwa.r_cost(N))
    assert bool(torch.isfinite(out).all())


def _lambda_copy(sol):
    from mpcgpu_amd import pcg_config
    S, P, gam = destroy_inputs()[1]
    sol.set_option("cluster", 2)                             # float, two members of four knots: the copy of lambda is made at this launch
    lam = torch.zeros(DESTROY_B, n * DESTROY_N, device="cuda")
    sol.solve(S, P, gam, lam, pcg_config(pcg_exit_tol=0.0, pcg_max_iter=4), "ss")
    sol.set_option("cluster", -1)
    assert sol.get_option("last_kernel_family") == 7 and bool(torch.isfinite(lam).all())


MAKERS = {"seam": lambda s: _form(s, np.float32, False), "staging": lambda s: _form(s, np.float32, True), "staging64": lambda s: _form(s, np.float64, True),
          "block": lambda s: _block(s, False), "block64": lambda s: _block(s, True), "merit": _merit, "lambda": _lambda_copy}


def test_destroy_at_every_stage():
    """A handle is destroyed with no lazy buffer, with each single one, and with all of them (8 knots, max_batch 2; and, on 64 knots, with the double
    clusters' buffers of "reserve_f64" = 1, which a handle of 8 knots never has).  The handle that has them all is destroyed while another handle's
    stream is capturing: the capture replays."""
    from mpcgpu_amd import PcgSolver
    N, B = DESTROY_N, DESTROY_B
    PcgSolver(N, max_batch=B).close()
    for name, make in MAKERS.items():
        sol = PcgSolver(N, max_batch=B)
        make(sol)
        torch.cuda.synchronize()
        sol.close()
    big = PcgSolver(64, max_batch=1200)                      # (mpcg_create makes no double buffers for it: more than 8 MB of double iterates)
    big.set_option("reserve_f64", 1)
    big.close()
    full = PcgSolver(N, max_batch=B)
    for make in MAKERS.values():
        make(full)
    S, _, gam = destroy_inputs()[1]
    other = PcgSolver(N, max_batch=B)
    want = other.block_solve(S, gam)
    lam = torch.zeros_like(want)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        other.block_solve(S, gam, lam)
        full.close()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lam, want) and bool(torch.isfinite(want).all())
