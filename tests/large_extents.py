"""Large extents: every array of a call past 2^31 and 2^32 bytes.  The checker of tests/test_gpu_large_*.py, pinned
without a GPU by tests/test_large_extents_cpu.py.

A wrapped offset does not fault: it lands inside the same allocation, or inside the same buffer resource, and reads another trajectory's data
or overwrites another trajectory's results.  So a call is made twice on one handle with the same options: on D distinct trajectories (the call
the older suites pin to the float64 oracle) and on B trajectories tiled from them ON THE DEVICE, trajectory b a copy of trajectory b mod D,
every output prefilled with 0xFF bytes.  Then
  (a) position independence: every output of trajectory b carries the bits of trajectory b mod D of the small call;
  (b) every owed element is written: no must-write element of an output of the small call holds the prefill, elements the header
      says are never written still hold it — and by (a) the same is true of every tile of the large call;
  (c) inputs are untouched: every input tile still carries its bits.
Large arrays never leave the device: they are filled and compared in slices of at most 256 MB (torch.equal on integer views).

A wrap is VISIBLE only if it lands on other bits.  check_conditions() asserts, before any call:
  D condition           D odd and >= 3, B no multiple of D.  With D = 4 a per-trajectory scalar (rho_v, a count, a byte flag) that wraps at 2^32
                        bytes lands on the same tile index: 2^32 mod (4 x 4) = 0.
  B mod 4 != 0          the "dead rows redo the last item" lanes of the four-per-wavefront kernels run at the top of the range.
  wrap-shift condition  for every array and every W in {2^31, 2^32}, in bytes and in elements: W mod (D x per-trajectory extent) != 0, so a
                        wrapped access never lands on the same element of a trajectory with the same tile index.
and check_small() that the D base trajectories differ pairwise in every input and every output array (arrays marked const — the exact
iteration counts and flags of a solve with exit_tol = 0 — are the same for every trajectory by construction: for them (b) is the check).

Specs are pure data (no torch): Arr per array of ONE trajectory, Spec = arrays + D + B + the handle-owned bytes of the call; need_bytes() is
the peak device memory a test computes up front and the CPU test holds below CAP_BYTES."""
import collections
import time

import numpy as np

import arena_specs as A
import pcg_step_cases as cases

FILL = 0xFF
SLICE_BYTES = 256 << 20
CAP_BYTES = 24 << 30
MODULI = (2 ** 31, 2 ** 32)
ROLES = ("in", "out", "inout", "untouched")

Arr = collections.namedtuple("Arr", "name dtype traj role mask const")
Spec = collections.namedtuple("Spec", "label arrays D B scratch")


def arr(name, dtype, traj, role, mask=None, const=False):
    """One trajectory's extent of an array.  mask: bool [traj], True = never written by the call.  const: every trajectory gets the same value."""
    assert role in ROLES, role
    if mask is not None:
        mask = np.ascontiguousarray(mask, bool).reshape(-1)
        assert mask.size == traj and role in ("out", "inout"), name
    return Arr(name, np.dtype(dtype), int(traj), role, mask, bool(const))


def from_arena(specs, const=()):
    """tests/arena_specs.py's description of a call on ONE trajectory (Bt = 1) as Arr's: the same roles and never-written masks."""
    out = []
    for s in specs:
        assert s.count == s.traj, (s.name, "build the arena specs with one trajectory")
        out.append(arr(s.name, s.dtype, s.count, s.role, s.mask, s.name in const))
    return out


def nbytes(a, rows):
    return rows * a.traj * a.dtype.itemsize


def need_bytes(spec):
    """Peak device memory of run(): every array at B and at D (the small call's arrays and its kept results), the handle's own buffers, and the
    slices of the fill and of the compare (one tile, one comparison result)."""
    big = sum(nbytes(a, spec.B) for a in spec.arrays)
    small = 3 * sum(nbytes(a, spec.D) for a in spec.arrays)
    return big + small + spec.scratch + 3 * SLICE_BYTES


def check_conditions(spec, moduli=MODULI):
    D, B = spec.D, spec.B
    assert D >= 3 and D % 2 == 1 and B % D != 0, \
        f"{spec.label}: D condition: D = {D} must be odd and >= 3 and B = {B} no multiple of it (a wrapped per-trajectory scalar would land on its own tile index)"
    assert B % 4 != 0, f"{spec.label}: B = {B} is a multiple of 4: no dead rows in the last wavefront of a four-per-wavefront kernel"
    assert len({a.name for a in spec.arrays}) == len(spec.arrays)
    for a in spec.arrays:
        for W in moduli:
            for unit, what in ((a.dtype.itemsize, "bytes"), (1, "elements")):
                assert W % (D * a.traj * unit) != 0, \
                    f"{spec.label}: wrap-shift condition: array '{a.name}': {W} mod (D x {a.traj * unit} {what}) = 0, a wrapped access would land on its own copy"


# ---- backends: numpy (the CPU model) and torch (the device) ----
_INT = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def _bits(x):
    """[rows, traj] as integers of the element's width (float NaN payloads compare as bits)."""
    name = _INT[x.dtype.itemsize if isinstance(x, np.ndarray) else x.element_size()]
    if isinstance(x, np.ndarray):
        return x.view(getattr(np, name))
    import torch
    return x.view(getattr(torch, name))


def _tile(x, k):
    return np.tile(x, (k, 1)) if isinstance(x, np.ndarray) else x.repeat(k, 1)


def _equal(x, y):
    if isinstance(x, np.ndarray):
        return np.array_equal(x, y)
    import torch
    return torch.equal(x, y)


def _first_diff(x, y):
    ne = (x != y).reshape(-1)
    if isinstance(x, np.ndarray):
        return int(np.flatnonzero(ne)[0])
    return int(ne.nonzero()[0, 0].item())


def _slices(a, D, B):
    """(r0, r1) row ranges of at most SLICE_BYTES, each a whole number of tiles (but the last)."""
    rows = min(max(1, SLICE_BYTES // max(1, nbytes(a, D))), -(-B // D)) * D
    return [(r0, min(B, r0 + rows)) for r0 in range(0, B, rows)], rows // D


def fill_tiled(a, big, small, D, B):
    """big[b] = small[b mod D], slice by slice."""
    ranges, k = _slices(a, D, B)
    tile = _tile(small, k)
    for r0, r1 in ranges:
        big[r0:r1] = tile[:r1 - r0]


def compare_tiled(a, big, small, D, B, what, moduli=MODULI, label=""):
    """(a) / (c): big[b] carries the bits of small[b mod D].  The failure names the array, the first differing trajectory, its byte offset and
    that offset modulo 2^31 and 2^32."""
    ranges, k = _slices(a, D, B)
    want = _tile(_bits(small), k)
    got = _bits(big)
    for r0, r1 in ranges:
        if _equal(got[r0:r1], want[:r1 - r0]):
            continue
        i = _first_diff(got[r0:r1], want[:r1 - r0])
        b, e = r0 + i // a.traj, i % a.traj
        off = (b * a.traj + e) * a.dtype.itemsize
        v = int(got[b, e])
        fill = -1 if a.dtype.itemsize > 1 else FILL
        held = [d for d in range(D) if int(_bits(small)[d, e]) == v and d != b % D]
        note = "still holds the 0xFF prefill: never written" if (v == fill and a.role != "in") else \
            (f"holds the value of tile {held[0]}" if held else "holds none of the tiles' values")
        raise AssertionError(f"{label}: array '{a.name}' ({what}): first difference at trajectory {b} (tile {b % D}), element {e}, byte offset {off} ("
                             + ", ".join(f"mod {W}: {off % W}" for W in moduli) + f"); it {note}")


def check_small(spec, before, after):
    """The call on D trajectories: (b), (c) and pairwise distinct trajectories.  before / after: name -> numpy [D, traj] (before: what every
    array held when the call was made — outputs the prefill)."""
    D = spec.D
    for a in spec.arrays:
        b, x = _bits(before[a.name]), _bits(after[a.name])
        if a.role in ("in", "untouched"):
            assert np.array_equal(b, x), f"{spec.label}: {'input ' if a.role == 'in' else 'untouched '}array '{a.name}' was modified by the call on {D} trajectories"
        else:
            masked = np.broadcast_to(a.mask if a.mask is not None else np.zeros(a.traj, bool), x.shape)
            kept = (b == x)
            if a.role == "out" and (kept & ~masked).any():           # (inout: an element may keep its bits — a zero of Q is a zero of its inverse)
                d, e = np.argwhere(kept & ~masked)[0]
                raise AssertionError(f"{spec.label}: output array '{a.name}': element {e} of trajectory {d} still holds the 0xFF prefill: never written")
            assert not (~kept & masked).any(), f"{spec.label}: array '{a.name}': an element the call must not write was written"
        if a.role != "untouched" and not a.const:
            for i in range(D):
                for j in range(i + 1, D):
                    assert not np.array_equal(x[i], x[j]), f"{spec.label}: array '{a.name}': trajectories {i} and {j} carry the same bits — a wrap between their tiles would be invisible"


def torch_dtype(dt):
    import torch
    return {"float16": torch.float16, "float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8}[dt.name]


def run(spec, inputs, call, after_big=None, report=print):
    """The GPU tests' one move.  inputs: name -> numpy [D, traj] of every in / inout array.  call(arrays, Bt): the library call on a dict of
    [Bt, traj] device tensors.  Returns the small call's out / inout arrays (numpy, [D, traj]) for the caller to hold against the oracle.
    after_big(big, small_before, small_after): further calls on the large arrays while they live."""
    import pytest
    import torch
    check_conditions(spec)
    need = need_bytes(spec)
    assert need <= CAP_BYTES, (spec.label, need)
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0]
    if free < 1.5 * need:
        pytest.skip(f"{spec.label}: needs {need} bytes of device memory (x 1.5 = {int(1.5 * need)}), {free} are free")
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    D, B = spec.D, spec.B
    dev = torch.device("cuda")
    small = {}
    for a in spec.arrays:
        if a.role in ("in", "inout"):
            v = np.ascontiguousarray(inputs[a.name], a.dtype).reshape(D, a.traj)
            small[a.name] = torch.from_numpy(v.copy()).to(dev)
        else:
            small[a.name] = torch.full((D, nbytes(a, 1)), FILL, dtype=torch.uint8, device=dev).view(torch_dtype(a.dtype))
    before = {k: v.clone() for k, v in small.items()}
    call(small, D)
    torch.cuda.synchronize()
    before_h, after_h = ({k: v.cpu().numpy() for k, v in d.items()} for d in (before, small))
    check_small(spec, before_h, after_h)
    t1 = time.perf_counter()
    big = {}
    for a in spec.arrays:
        big[a.name] = torch.empty((B, a.traj), dtype=torch_dtype(a.dtype), device=dev)
        fill_tiled(a, big[a.name], before[a.name], D, B)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    call(big, B)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    for a in spec.arrays:
        if a.role in ("in", "untouched"):
            compare_tiled(a, big[a.name], before[a.name], D, B, "an input of the large call, must come back intact" if a.role == "in" else "must keep the prefill", label=spec.label)
        else:
            compare_tiled(a, big[a.name], small[a.name], D, B, "an output of the large call against the call on D trajectories", label=spec.label)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    if after_big is not None:
        after_big(big, before, small)
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() + spec.scratch
    report(f"large extents {spec.label}: D {D} B {B} need {need / 2 ** 30:.2f} GiB, peak {peak / 2 ** 30:.2f} GiB (handle buffers {spec.scratch / 2 ** 30:.2f}); "
           f"small call {t1 - t0:.2f} s, fill {t2 - t1:.2f} s, call {t3 - t2:.3f} s, compare {t4 - t3:.2f} s, all {time.perf_counter() - t0:.2f} s")
    assert peak <= CAP_BYTES, (spec.label, peak)
    big.clear()
    small.clear()
    before.clear()
    torch.cuda.empty_cache()
    return {a.name: after_h[a.name] for a in spec.arrays if a.role in ("out", "inout")}


def run_numpy(spec, inputs, call, moduli=MODULI):
    """run() on host arrays: the same conditions, fill and checks (tests/test_large_extents_cpu.py: a numpy model of a batched kernel)."""
    check_conditions(spec, moduli)
    D, B = spec.D, spec.B

    def fresh(rows, src):
        out = {}
        for a in spec.arrays:
            out[a.name] = np.empty((rows, a.traj), a.dtype)
            fill_tiled(a, out[a.name], src[a.name], D, rows)
        return out
    before = {}
    for a in spec.arrays:
        if a.role in ("in", "inout"):
            before[a.name] = np.ascontiguousarray(inputs[a.name], a.dtype).reshape(D, a.traj).copy()
        else:
            before[a.name] = np.full((D, nbytes(a, 1)), FILL, np.uint8).view(a.dtype)
    small = fresh(D, before)
    call(small, D)
    check_small(spec, before, small)
    big = fresh(B, before)
    call(big, B)
    for a in spec.arrays:
        if a.role in ("in", "untouched"):
            compare_tiled(a, big[a.name], before[a.name], D, B, "an input of the large call, must come back intact", moduli, spec.label)
        else:
            compare_tiled(a, big[a.name], small[a.name], D, B, "an output of the large call against the call on D trajectories", moduli, spec.label)
    return small


# ---- sizes ----
def schur_bytes_per_knot(n, elem):
    """mpcg_producers.hip's: S, the largest array of the formation per knot."""
    return 3 * n * n * elem


def dz_bytes_per_knot(n, m, elem):
    """mpcg_producers.hip's: C, the largest array of dz per knot."""
    return (n * n + n * m) * elem


def pick_batch(W, traj_bytes, Ds=(5, 3)):
    """(B, D): the first batch whose array of traj_bytes per trajectory is LARGER than W bytes, moved up to the first B that is no multiple of
    4 and of D = 5 (else 3)."""
    B = W // traj_bytes + 1
    while True:
        if B % 4:
            for D in Ds:
                if B % D:
                    return B, D
        B += 1


E = {"f32": 4, "f64": 8}
MB = 1 << 20
n14, m7 = 14, 7

# Formation: (N, last batch on the register-resident route, D).  N chosen so that B and B + 1 are both no multiple of 4 and of D, and the horizon
# has two 16-row chunks (the seam kernel runs).  Distance of S to 2^31 bytes: f32 4,160 below / 47,584 past; f64 13,568 below / 80,512 past.
FORM = {"f32": (22, 41502, 5), "f64": (20, 22826, 5)}
# The first batch whose S passes 2^32 bytes at the same horizons: f32 43,424 bytes past, f64 66,944 past.
FORM_4G = {"f32": (22, 83005, 3), "f64": (20, 45653, 3)}
# dz: C is what the host tests (knots x 1,176 / 2,352 bytes).  f32 632 bytes below / 31,120 past; f64 4,160 below / 47,584 past.
DZ = {"f32": (27, 67633, 3), "f64": (22, 41502, 5)}
FORM_CASES = [("f32", "ss", True), ("f32", "jacobi", False), ("f64", "ss", False), ("f64", "jacobi", True)]      # (precision, preconditioner, _rhov)
FORM_4G_CASES = [("f32", "ss", True), ("f64", "jacobi", True)]


def seam_bytes(N, B, num_cus=256):
    """ensure_seam_buffer (mpcg_producers.hip) for a handle of max_batch B."""
    want = num_cus * 24
    return 196 * 8 * max(2 * want + B + 4, B * ((N - 1 + 15) // 16))


def form_spec(prec, pc, rhov, N, B, D, side):
    arrays = from_arena(A.form_schur(prec, n14, m7, N, 1, pc, rhov))
    scratch = seam_bytes(N, B) + B * A.glen(n14, m7, N) * E[prec]          # the seam buffer and the LDS route's staging copy of G
    return Spec(f"form_schur {prec} {pc} {'rhov' if rhov else 'rho'} N{N} B{B} {side}", arrays, D, B, scratch)


def form_specs():
    out = []
    for prec, pc, rhov in FORM_CASES:
        N, B, D = FORM[prec]
        out += [form_spec(prec, pc, rhov, N, B, D, "below 2^31"), form_spec(prec, pc, rhov, N, B + 1, D, "past 2^31")]
    for prec, pc, rhov in FORM_4G_CASES:
        out.append(form_spec(prec, pc, rhov, *FORM_4G[prec], "past 2^32"))
    return out


def dz_spec(prec, N, B, D, side):
    return Spec(f"compute_dz {prec} N{N} B{B} {side}", from_arena(A.compute_dz(prec, n14, m7, N, 1)), D, B, 0)


def dz_specs():
    out = []
    for prec in ("f32", "f64"):
        N, B, D = DZ[prec]
        out += [dz_spec(prec, N, B, D, "below 2^31"), dz_spec(prec, N, B + 1, D, "past 2^31")]
    return out


# PCG: one row of tests/pcg_step_cases.py per kernel family the plan table can select, the smallest horizon that selects it; S and Pinv each
# past 2^32 bytes.
def _row(prec, family, N, pc, n=14):
    return next(r for r in cases.ROWS if (r.prec, r.family, r.N, r.pc, r.n) == (prec, family, N, pc, n))


PCG_ROWS = [_row("f32", 0, 3, "ss"), _row("f32", 5, 3, "jacobi"), _row("f32", 6, 3, "ss"), _row("f32", 7, 129, "ss"), _row("f32", 11, 3, "jacobi"),
            _row("f32", 3, 9, "ss", 13), _row("f64", 8, 33, "ss"), _row("f64", 9, 17, "jacobi"), _row("f64", 10, 65, "ss")]
PCG_REF_ROWS = [_row("f32", 11, 3, "ss"), _row("f64", 9, 17, "ss")]
PCG_F16 = cases.F16_CASES[0]               # (N = 17, no options, family 0, 8 wavefronts)
PCG_D = 5


def pcg_scratch(n, N, B):
    """What a handle of max_batch B owns for its solves, bounded from above: copies of lambda (the clusters' warm start, in double for the
    double kernels), queue, flags, hand-off cells and the dispatch order."""
    return 4 * B * N * n * 8 + 64 * MB


def pcg_spec(r, storage=None, ref=False):
    bs = 3 * r.n * r.n * r.N * (2 if storage == "f16" else E[r.prec])
    B, D = pick_batch(2 ** 32, bs)
    while B % PCG_D == 0 or B % 4 == 0:
        B += 1
    arrays = from_arena(A.pcg(r.prec, r.n, r.N, 1, True, storage), const=("iters", "exits"))
    tag = "pcg f16" if storage else "pcg_ref + pcg" if ref else "pcg"
    return Spec(f"{tag} {cases.row_id(r)} B{B}", arrays, PCG_D, B, pcg_scratch(r.n, r.N, B))


def f16_row():
    N, opts, family, waves = PCG_F16
    return cases.Row("f32", 14, 7, N, "ss", family, opts, waves)


def pcg_specs():
    return [pcg_spec(r) for r in PCG_ROWS] + [pcg_spec(r, ref=True) for r in PCG_REF_ROWS] + [pcg_spec(f16_row(), "f16")]


# mpcg_bt_spmv, mpcg_block_solve(_f64), mpcg_bd_to_csr_lowertri: the first batch whose S passes 2^32 bytes, three knots per trajectory
LINALG_N = 3
BLOCK_SOLVES = [("f32", {"block_solve_wide": 0}), ("f32", {"block_solve_wide": 1}), ("f32", {"block_solve_wide": 0, "block_solve_f64": 1}), ("f64", {})]


def spmv_spec(cols):
    N = LINALG_N
    B, D = pick_batch(2 ** 32, 3 * 196 * N * 4)
    arrays = [arr("M", np.float32, 3 * 196 * N, "in"), arr("x", np.float32, 14 * N, "in"), arr("y", np.float32, 14 * N, "out")]
    return Spec(f"bt_spmv cols{cols} N{N} B{B}", arrays, D, B, 0)


def block_solve_spec(prec, opts):
    N = LINALG_N
    B, D = pick_batch(2 ** 32, 3 * 196 * N * E[prec])
    sweep = 8 if (prec == "f64" or opts.get("block_solve_f64")) else 4
    tag = "-".join(f"{k}{v}" for k, v in opts.items()) or "default"
    return Spec(f"block_solve {prec} {tag} N{N} B{B}", from_arena(A.block_solve(prec, n14, N, 1)), D, B, B * N * (196 + 14) * sweep)


def csr_spec():
    N = LINALG_N
    B, D = pick_batch(2 ** 32, 3 * 196 * N * 4)
    return Spec(f"bd_to_csr N{N} B{B}", from_arena(A.bd_to_csr(n14, N, 1)), D, B, 0)


def linalg_specs():
    return [spmv_spec(3), spmv_spec(1)] + [block_solve_spec(p, o) for p, o in BLOCK_SOLVES] + [csr_spec()]


# mpcg_generate_kkt(_f64): the first batch whose C passes 2^32 bytes.  (precision, N, options, _xuref with a limits plant)
KKT_CASES = [("f32", 5, (("kkt_f32", 0), ("integrator", 1)), False), ("f32", 5, (("kkt_f32", 1), ("integrator", 0)), False),
             ("f64", 3, (("integrator", 0),), False), ("f64", 5, (("integrator", 1),), True)]


def kkt_spec(prec, N, opts, xuref):
    B, D = pick_batch(2 ** 32, A.clen(n14, m7, N) * E[prec], (3,) if xuref else (5, 3))
    arrays = from_arena(A.generate_kkt(prec, N, 1))
    if xuref:
        # (tests/test_gpu_xuref.py's case (5, 3): a plan of N + 1 rows per trajectory at a stride of N + 3 rows, one offset per trajectory)
        arrays[3:3] = [arr("xu_traj", A.DT[prec], (N + 3) * 21, "in"), arr("traj_offset", np.int32, 1, "in")]
    tag = "-".join(f"{k}{v}" for k, v in opts)
    return Spec(f"generate_kkt{'_xuref limits' if xuref else ''} {prec} {tag} N{N} B{B}", arrays, D, B, 0)


def kkt_specs():
    return [kkt_spec(*c) for c in KKT_CASES]


# mpcg_riccati_gains(_f64): 14 x 7 at three knots, the first admissible batch whose G passes 2^32 bytes (686 elements per trajectory: 1,565,222
# trajectories in float, 782,611 in double; G, C, K and rho together 9.2 GB either way); one rho per trajectory, so rho_v[b] is indexed there too.
RICCATI_N = 3


def riccati_spec(prec):
    N, dt = RICCATI_N, A.DT[prec]
    B, D = pick_batch(2 ** 32, A.glen(n14, m7, N) * E[prec])
    arrays = [arr("G", dt, A.glen(n14, m7, N), "in"), arr("C", dt, A.clen(n14, m7, N), "in"), arr("rho", dt, 1, "in"),
              arr("K", dt, (N - 1) * m7 * n14, "out")]
    return Spec(f"riccati_gains {prec} N{N} B{B}", arrays, D, B, 0)                # (pure stream work: the handle owns nothing for it)


def riccati_specs():
    return [riccati_spec(p) for p in ("f32", "f64")]


# mpcg_convert_f32_to_f16: the element index passes int, the source 2^33 bytes, the destination 2^32 bytes, the ragged tail at the top.
CONVERT_COUNT = 2 ** 31 + 13


def convert_need():
    return CONVERT_COUNT * 6 + 3 * SLICE_BYTES


def all_specs():
    return form_specs() + dz_specs() + pcg_specs() + linalg_specs() + kkt_specs() + riccati_specs()
