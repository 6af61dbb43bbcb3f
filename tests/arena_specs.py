"""The arrays of every device entry point of include/mpcg.h as arena specs (tests/arena.py), and the case lists of the three GPU arena files
(tests/test_gpu_arena_pcg.py, _producers.py, _plant.py).  CPU only: tests/test_arena_cpu.py checks the layout properties over every list
(all_spec_lists) without a GPU.

Alignments are the smallest the entry accepts (include/mpcg.h, ALIGNMENT): the element's own, except where the entry refuses less.
knot / traj are the extents the bands are sized from: one knot's (for S and Pinv one block row's) and one trajectory's elements."""
import numpy as np

import generic_pcg_cases as gc
import pcg_step_cases as cases
from arena import spec

DT = {"f32": np.float32, "f64": np.float64}
I32, U8, F16 = np.int32, np.uint8, np.float16
n14, m7 = 14, 7
B = cases.B


def glen(n, m, N):
    return (n * n + m * m) * N - m * m


def clen(n, m, N):
    return (n * n + n * m) * (N - 1)


def zlen(n, m, N):
    return (n + m) * N - m


def nnz(n, N):
    return (N - 1) * n * n + N * (n * (n + 1)) // 2


def bd_mask(Bt, N, n, offdiag=False):
    """True where mpcg_form_schur never writes a bd-layout output: blocks (0, left) and (N-1, right); under block-Jacobi every off-diagonal
    block of Pinv as well."""
    mk = np.zeros((Bt, N, 3, n * n), bool)
    mk[:, 0, 0] = True
    mk[:, -1, 2] = True
    if offdiag:
        mk[:, :, 0] = True
        mk[:, :, 2] = True
    return mk


def rows_mask(Bt, per, rows):
    """[Bt, per] bool, True for the trajectories in rows."""
    mk = np.zeros((Bt, per), bool)
    mk[list(rows)] = True
    return mk


# ---- PCG ----
def pcg(prec, n, N, Bt, written, storage=None):
    """mpcg_pcg_solve / _f64 / _f16.  written: max_iter > 0 (at max_iter = 0 lambda keeps every bit)."""
    dt = DT[prec]
    mdt, malign = (F16, 4) if storage == "f16" else (dt, 16 if prec == "f32" else 8)
    bs = 3 * n * n
    return [spec("S", mdt, Bt * N * bs, "in", malign, bs, N * bs), spec("Pinv", mdt, Bt * N * bs, "in", malign, bs, N * bs),
            spec("gamma", dt, Bt * N * n, "in", None, n, N * n),
            spec("lambda", dt, Bt * N * n, "inout", None, n, N * n, None if written else np.ones(Bt * N * n, bool)),
            spec("iters", I32, Bt, "out", None, 1, 1), spec("exits", U8, Bt, "out", None, 1, 1)]


def pcg_ref(prec, n, N, written):
    """The 12-argument entries: d_r, d_p outputs; d_v_temp and d_eta_new_temp sized as the reference sizes them (knot_points elements,
    include/pcg/sqp.cuh:124-125) and untouched; one uint32 and one byte."""
    dt = DT[prec]
    head = pcg(prec, n, N, 1, written)
    return head[:4] + [spec("r", dt, N * n, "out", None, n), spec("p", dt, N * n, "out", None, n),
                       spec("v_temp", dt, N, "untouched"), spec("eta_new_temp", dt, N, "untouched")] + head[4:]


def tiled_total(num_cus):
    return 2 * num_cus + 3


TILED = [r for r in cases.ROWS32 if r.n == 14 and r.family in (5, 6, 11) and r.N == 17]
LATCH = [next(r for r in cases.ROWS if r.prec == prec and r.family == fam and r.pc == "ss" and r.N > 32)
         for prec, fam in (("f32", 6), ("f32", 7), ("f32", 11), ("f64", 9), ("f64", 10))]
GENERIC_B = 3            # (tests/test_gpu_first_steps.py: three systems per launch at state sizes other than 14)


def batch_of(r):
    return B if r.n == 14 else GENERIC_B


# ---- producers and linear algebra ----
SCHUR_ROUTINGS = ("auto", "chunk1", "chunk3", "lds", "generic")
SCHUR_N = (2, 3, 9)
GENERIC_SHAPES = [(1, 1), (4, 1), (6, 3), (13, 5), (14, 3), (17, 17), (32, 8)]      # tests/test_gpu_generic_producers.py FORM_SHAPES, at N = 2
PRECONDS = ("ss", "jacobi", "none")


def form_schur(prec, n, m, N, Bt, pc, rhov):
    dt = DT[prec]
    bs = 3 * n * n
    out = [spec("G", dt, Bt * glen(n, m, N), "inout", None, n * n + m * m, glen(n, m, N)),
           spec("C", dt, Bt * clen(n, m, N), "in", None, n * n + n * m, clen(n, m, N)),
           spec("g", dt, Bt * zlen(n, m, N), "in", None, n + m, zlen(n, m, N)),
           spec("c", dt, Bt * n * N, "in", None, n, n * N),
           spec("S", dt, Bt * N * bs, "out", None, bs, N * bs, bd_mask(Bt, N, n))]
    if pc == "none":
        out.append(spec("Pinv", dt, Bt * N * bs, "untouched", None, bs, N * bs))
    else:
        out.append(spec("Pinv", dt, Bt * N * bs, "out", None, bs, N * bs, bd_mask(Bt, N, n, pc == "jacobi")))
    out.append(spec("gamma", dt, Bt * N * n, "out", None, n, N * n))
    if rhov:
        out.append(spec("rho", dt, Bt, "in", None, 1, 1))
    return out


def compute_dz(prec, n, m, N, Bt):
    dt = DT[prec]
    return [spec("Ginv", dt, Bt * glen(n, m, N), "in", None, n * n + m * m, glen(n, m, N)),
            spec("C", dt, Bt * clen(n, m, N), "in", None, n * n + n * m, clen(n, m, N)),
            spec("g", dt, Bt * zlen(n, m, N), "in", None, n + m, zlen(n, m, N)),
            spec("lambda", dt, Bt * n * N, "in", None, n, n * N),
            spec("dz", dt, Bt * zlen(n, m, N), "out", None, n + m, zlen(n, m, N))]


def block_solve(prec, n, N, Bt):
    dt = DT[prec]
    bs = 3 * n * n
    return [spec("S", dt, Bt * N * bs, "in", None, bs, N * bs), spec("gamma", dt, Bt * N * n, "in", None, n, N * n),
            spec("lambda", dt, Bt * N * n, "out", None, n, N * n)]


def prep_csr(n, N):
    return [spec("col_ptr", I32, n * N + 1, "out", None, n), spec("row_ind", I32, nnz(n, N), "out", None, n * n + n * (n + 1) // 2)]


def bd_to_csr(n, N, Bt):
    bs = 3 * n * n
    return [spec("S", np.float32, Bt * N * bs, "in", None, bs, N * bs),
            spec("val", np.float32, Bt * nnz(n, N), "out", None, n * n + n * (n + 1) // 2, nnz(n, N))]


def qdldl(n, N):
    return [spec("val", np.float32, nnz(n, N), "in", None, n * n + n * (n + 1) // 2), spec("gamma", np.float32, n * N, "in", None, n),
            spec("lambda", np.float32, n * N, "out", None, n)]


CONVERT_COUNTS = (8 * 5, 8 * 5 + 3, 2048 * 2 + 5)        # 8 k, 8 k + 3 (the scalar tail), 2048 k + 5 (a tail in a block of its own)


def convert(count):
    return [spec("src", np.float32, count, "in", 16), spec("dst", F16, count, "out", 16)]


PROBE_FLOATS = 4096 + 4 * 37        # 16,976 bytes: a multiple of 16 and of nothing the probe's 256 x 16-byte sweep likes


def probe():
    """mpcg_probe_hbm_read: d_src read whole in 16-byte pieces, d_sink (one float) written only for one particular sum — never here."""
    return [spec("src", np.float32, PROBE_FLOATS, "in", 16), spec("sink", np.float32, 1, "inout", None, 1, 1, np.ones(1, bool))]


def refusals(N):
    """One arena for every alignment refusal (tests/test_gpu_parity.py::test_error_behaviour): nothing in it may change."""
    bs = 3 * n14 * n14
    f = np.float32
    return [spec("S", f, N * bs, "in", 16, bs), spec("Pinv", f, N * bs, "in", 16, bs), spec("gamma", f, N * n14, "in", 8, n14),
            spec("lambda", f, N * n14, "untouched", 8, n14), spec("r", f, N * n14, "untouched"), spec("p", f, N * n14, "untouched"),
            spec("S16", F16, N * bs, "untouched", 16, bs), spec("P16", F16, N * bs, "untouched", 16, bs),
            spec("iters", I32, 1, "untouched"), spec("exits", U8, 1, "untouched"), spec("sink", f, 1, "untouched")]


# ---- plant and MPC-loop kernels (14 x 7) ----
PLANT_NB = ((2, 1), (3, 5))
KKT_BUILDS = ((("kkt_analytic", 1), ("kkt_f32", 0)), (("kkt_analytic", 0), ("kkt_f32", 0)), (("kkt_analytic", 1), ("kkt_f32", 1)),
              (("kkt_analytic", 1), ("kkt_f32", 2)))


def generate_kkt(prec, N, Bt):
    dt = DT[prec]
    n, m = n14, m7
    return [spec("goals", dt, Bt * 6 * N, "in", None, 6, 6 * N), spec("xs", dt, Bt * n, "in", None, n, n),
            spec("xu", dt, Bt * zlen(n, m, N), "in", None, n + m, zlen(n, m, N)),
            spec("G", dt, Bt * glen(n, m, N), "out", None, n * n + m * m, glen(n, m, N)),
            spec("C", dt, Bt * clen(n, m, N), "out", None, n * n + n * m, clen(n, m, N)),
            spec("g", dt, Bt * zlen(n, m, N), "out", None, n + m, zlen(n, m, N)), spec("c", dt, Bt * n * N, "out", None, n, n * N)]


def compute_merit(prec, N, Bt, A, with_xs, with_dz):
    dt = DT[prec]
    n, m = n14, m7
    out = [spec("goals", dt, Bt * 6 * N, "in", None, 6, 6 * N)]
    if with_xs:
        out.append(spec("xs", dt, Bt * n, "in", None, n, n))
    out.append(spec("xu", dt, Bt * zlen(n, m, N), "in", None, n + m, zlen(n, m, N)))
    if with_dz:
        out.append(spec("dz", dt, Bt * zlen(n, m, N), "in", None, n + m, zlen(n, m, N)))
    out.append(spec("merit", dt, Bt * A, "out", None, 1, A))
    return out


# line search: which trajectory does what (the merits are made to fit: tests/test_gpu_arena_plant.py)
LS_B, LS_A = 5, 3
LS_STEPS, LS_NONE, LS_FROZEN = (0, 3), (1, 4), (2,)


def line_search(prec, n, m, N, rho):
    """mpcg_line_search_step(_f64) / _rho(_f64) on five trajectories: 0 and 3 take a step, 1 and 4 take none (d_xu and d_merit_ref not written),
    2 is frozen under _rho (nothing but d_step written; without rho it takes no step)."""
    dt = DT[prec]
    L = zlen(n, m, N)
    still = LS_NONE + LS_FROZEN
    out = [spec("merit", dt, LS_B * LS_A, "in", None, 1, LS_A),
           spec("merit_ref", dt, LS_B, "inout", None, 1, 1, rows_mask(LS_B, 1, still)),
           spec("dz", dt, LS_B * L, "in", None, n + m, L), spec("xu", dt, LS_B * L, "inout", None, n + m, L, rows_mask(LS_B, L, still)),
           spec("step", I32, LS_B, "out", None, 1, 1)]
    if rho:
        out += [spec("rho", dt, LS_B, "inout", None, 1, 1, rows_mask(LS_B, 1, LS_FROZEN)),
                spec("drho", dt, LS_B, "inout", None, 1, 1, rows_mask(LS_B, 1, LS_FROZEN)),
                spec("done", U8, LS_B, "inout", None, 1, 1, rows_mask(LS_B, 1, LS_FROZEN))]
    return out


def simulate(prec, N, Bt, with_ee):
    dt = DT[prec]
    n, m = n14, m7
    out = [spec("xs", dt, Bt * n, "inout", None, n, n), spec("xu", dt, Bt * zlen(n, m, N), "in", None, n + m, zlen(n, m, N))]
    if with_ee:
        out.append(spec("eePos", dt, Bt * 3, "out", None, 3, 3))
    return out


ADV_B = 4
ADV_FROZEN = 3


def advance_shift(prec, N, T, per_traj):
    """shift = 1 on four trajectories: inside the plan; the else branch (offset beyond the plan); the plan used up (done becomes 1); frozen on
    entry (nothing of it is written).  The last knot of lambda keeps its value: never written."""
    dt = DT[prec]
    n, m = n14, m7
    L = zlen(n, m, N)
    rows = ADV_B if per_traj else 1
    lam_mask = rows_mask(ADV_B, n * N, (ADV_FROZEN,))
    lam_mask[:, n * (N - 1):] = True
    fz = lambda per: rows_mask(ADV_B, per, (ADV_FROZEN,))
    return [spec("xu", dt, ADV_B * L, "inout", None, n + m, L, fz(L)), spec("lambda", dt, ADV_B * n * N, "inout", None, n, n * N, lam_mask),
            spec("goal", dt, ADV_B * 6 * N, "inout", None, 6, 6 * N, fz(6 * N)), spec("xs", dt, ADV_B * n, "in", None, n, n),
            spec("eePos", dt, ADV_B * 3, "in", None, 3, 3),
            spec("xu_traj", dt, rows * T * (n + m), "in", None, n + m, T * (n + m)), spec("goal_traj", dt, rows * T * 6, "in", None, 6, T * 6),
            spec("traj_offset", I32, ADV_B, "inout", None, 1, 1, fz(1)), spec("done", I32, ADV_B, "inout", None, 1, 1, fz(1)),
            spec("tracking_error", dt, ADV_B, "out", None, 1, 1, fz(1))]


def advance_noshift(prec, N):
    """shift = 0: x_0 of every live trajectory from d_xs and nothing else."""
    dt = DT[prec]
    n, m = n14, m7
    L = zlen(n, m, N)
    mk = np.ones((ADV_B, L), bool)
    mk[:ADV_FROZEN, :n] = False
    return [spec("xu", dt, ADV_B * L, "inout", None, n + m, L, mk), spec("xs", dt, ADV_B * n, "in", None, n, n),
            spec("done", I32, ADV_B, "in", None, 1, 1)]


INVDYN_COUNT = 5


def invdyn(prec, with_qd, with_qdd):
    dt = DT[prec]
    out = [spec("q", dt, INVDYN_COUNT * 7, "in", None, 7, 7)]
    if with_qd:
        out.append(spec("qd", dt, INVDYN_COUNT * 7, "in", None, 7, 7))
    if with_qdd:
        out.append(spec("qdd", dt, INVDYN_COUNT * 7, "in", None, 7, 7))
    out.append(spec("tau", dt, INVDYN_COUNT * 7, "out", None, 7, 7))
    return out


def all_spec_lists(num_cus=256):
    """(label, specs) of every arena the GPU files build (the tiled PCG case at the MI355X's 256 CUs)."""
    out = []
    for r in cases.ROWS:
        for written in (True, False):
            out.append((f"pcg {cases.row_id(r)} {written}", pcg(r.prec, r.n, r.N, batch_of(r), written)))
            out.append((f"pcg_ref {cases.row_id(r)} {written}", pcg_ref(r.prec, r.n, r.N, written)))
    for N, _, family, _ in cases.F16_CASES:
        for written in (True, False):
            out.append((f"pcg f16 N{N} family{family} {written}", pcg("f32", 14, N, B, written, "f16")))
    for r in TILED:
        out.append((f"pcg tiled {cases.row_id(r)}", pcg("f32", 14, r.N, tiled_total(num_cus), True)))
    for prec in DT:
        for pc in PRECONDS:
            for rhov in (False, True):
                for N in SCHUR_N:
                    out.append((f"form_schur {prec} 14x7 N{N} {pc} rhov{rhov}", form_schur(prec, 14, 7, N, B, pc, rhov)))
                for n, m in GENERIC_SHAPES:
                    out.append((f"form_schur {prec} {n}x{m} {pc} rhov{rhov}", form_schur(prec, n, m, 2, B, pc, rhov)))
        for n, m, N, Bt in [(14, 7, 5, 1), (14, 7, 3, B)] + [(n, m, 2, B) for n, m in GENERIC_SHAPES]:
            out.append((f"compute_dz {prec} {n}x{m} N{N} B{Bt}", compute_dz(prec, n, m, N, Bt)))
        for n, N in [(14, 9), (14, 2), (13, 2)]:
            out.append((f"block_solve {prec} n{n} N{N}", block_solve(prec, n, N, B)))
        for N, Bt in PLANT_NB:
            out.append((f"generate_kkt {prec} N{N} B{Bt}", generate_kkt(prec, N, Bt)))
            for A in (1, 3):
                for with_xs in (True, False):
                    out.append((f"compute_merit {prec} N{N} B{Bt} A{A} xs{with_xs}", compute_merit(prec, N, Bt, A, with_xs, True)))
            out.append((f"compute_merit {prec} N{N} B{Bt} no dz", compute_merit(prec, N, Bt, 1, True, False)))
            for with_ee in (True, False):
                out.append((f"simulate {prec} N{N} B{Bt} ee{with_ee}", simulate(prec, N, Bt, with_ee)))
        for n, m, N in ((14, 7, 3), (6, 3, 3)):
            for rho in (False, True):
                out.append((f"line_search {prec} {n}x{m} rho{rho}", line_search(prec, n, m, N, rho)))
        for N in (2, 3):
            for per_traj in (False, True):
                out.append((f"advance shift {prec} N{N} per_traj{per_traj}", advance_shift(prec, N, N + 6, per_traj)))
            out.append((f"advance noshift {prec} N{N}", advance_noshift(prec, N)))
        for with_qd in (True, False):
            for with_qdd in (True, False):
                out.append((f"invdyn {prec} qd{with_qd} qdd{with_qdd}", invdyn(prec, with_qd, with_qdd)))
    for n, N in ((14, 9), (13, 2)):
        out += [(f"prep_csr n{n} N{N}", prep_csr(n, N)), (f"bd_to_csr n{n} N{N}", bd_to_csr(n, N, B)), (f"qdldl n{n} N{N}", qdldl(n, N))]
    for count in CONVERT_COUNTS:
        out.append((f"convert {count}", convert(count)))
    out.append(("probe", probe()))
    out.append(("refusals", refusals(8)))
    return out
