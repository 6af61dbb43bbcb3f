"""GPU: the kernels behind mpcg_plant_create on robots OTHER than the KUKA iiwa 14 — mpcg_generate_kkt (double analytic, double difference checker,
one-knot float, packed two-knot float, the _f64 entry), mpcg_compute_merit (double, packed "merit_f32", the _f64 entry) and mpcg_simulate — against
the float64 restatements (oracle/iiwa_ref.py, tests/plant_ref.py) run on the same chain.

Every other GPU test uses Plant() = the iiwa, where about half of the 28 numbers per joint the recursions multiply are zero or below the tolerances
(tests/chain_models.py).  The chains here (tests/chain_models.py::random_chain, seeds chain_models.SEEDS) have no such entry: a kernel
that indexes ET transposed, picks the wrong packed half for a constant or mishandles an inertia product moves some output by more than 1e-2 of
max(1, |block|) (tests/test_chain_models_cpu.py), thousands of times the limits below.  Each limit is the one the project already holds the same
kernel to against the same restatement on the iiwa; all are relative to max(1, |block|) or max(1, |value|).  The iiwa rebuilt from its geometry
through the same export is the control: bit for bit Plant().

States: every q uniform in [-2 pi, 2 pi] (all quadrants of the kernels' sine / cosine reduction, more than one turn), "large" |qd| <= 2, |u| <= 20 and
"modest" |qd| <= 0.5, |u| <= 2.  Shapes: (2, 1) one item that is first and last block at once; (3, 5) B (N - 1) no multiple of four items and, with
three step sizes, an odd item total for the packed halves; (9, 3) an odd knot count, one idle half in the packed builds."""
import functools

import numpy as np
import pytest
import torch

import chain_models as cm
import iiwa_ref
import plant_ref as P
from mpcgpu_amd import iiwa
from test_gpu_kkt_f64 import LIMIT_C, LIMIT_Ggc
from test_gpu_merit_f64 import LIMIT as LIMIT_MERIT_F64

pytestmark = pytest.mark.gpu
n, m = cm.n, cm.m
SHAPES = list(cm.SHAPES)
SIZES = ("large", "modest")
STEPS3 = [0.0, -1.0, -0.5]
MU = 10.0
QD32 = float(np.float32(iiwa.QD_COST))
f32, f64 = np.float32, np.float64
NAN = float("nan")


def r32(N):
    return float(np.float32(iiwa.r_cost(N)))


def dev(a, dtype=f32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def rel(got, want):
    return float(np.abs(np.asarray(got, f64) - want).max() / max(1.0, np.abs(want).max()))


def widen(*arrs):
    return tuple(np.asarray(a, f32).astype(f64) for a in arrs)


# ---- chains, plants, inputs and restatements: built once, never written to ----
@functools.lru_cache(maxsize=None)
def chain(which):
    return cm.Chain.from_iiwa() if which == "iiwa" else cm.random_chain(which)


@functools.lru_cache(maxsize=None)
def plant(which):
    from mpcgpu_amd import Plant
    return Plant() if which == "default" else Plant(cm.tables(chain(which)))


def input_seed(which):
    return 0 if which in ("iiwa", "default") else cm.input_seed(which)


@functools.lru_cache(maxsize=None)
def inputs32(which, N, B, size):
    """(xu, goals [B, 6N], xs) rounded to float32: what both the float and the _f64 entries can be given."""
    xu, goals, xs = cm.hard_inputs(N, B, input_seed(which), size)
    return tuple(np.ascontiguousarray(a, f32) for a in (xu, goals.reshape(B, -1), xs))


@functools.lru_cache(maxsize=None)
def inputs64(which, N, B, size):
    """Genuinely double inputs, built as tests/test_gpu_kkt_f64.py::windows64: the float32 values times (1 + 1e-12 r), r uniform in [-1, 1]."""
    rng = np.random.default_rng([7, N, input_seed(which)])
    out = tuple(a.astype(f64) * (1.0 + 1e-12 * rng.uniform(-1, 1, a.shape)) for a in inputs32(which, N, B, size))
    assert all((a != a.astype(f32)).mean() > 0.9 for a in out)
    return out


def restate(which, N, arrs):
    xu, goals, xs = arrs
    return [iiwa_ref.generate_kkt(chain(which), xu[b], goals[b].reshape(N, 6), xs[b], N) for b in range(len(xu))]


@functools.lru_cache(maxsize=None)
def restated32(which, N, B, size):
    """oracle/iiwa_ref.py on exactly the float32-rounded inputs the float entries see."""
    return restate(which, N, widen(*inputs32(which, N, B, size)))


@functools.lru_cache(maxsize=None)
def restated64(which, N, B, size):
    return restate(which, N, inputs64(which, N, B, size))


def poison(shapes, dtype):
    """NaN-filled blocks of the sizes the next call allocates for its outputs, handed back to the caching allocator: an entry the kernel leaves
    unwritten must not look right."""
    for t in [torch.full(s, NAN, dtype=dtype, device="cuda") for s in shapes]:
        del t
    torch.cuda.synchronize()


def kkt(which, N, arrs, dtype=f32, qd=None, r=None, **options):
    """One generate_kkt call on a fresh handle -> [G, C, g, c] as numpy [B, ...]; the device outputs are left NaN-filled for the next call."""
    from mpcgpu_amd import PcgSolver
    B = len(arrs[0])
    sol = PcgSolver(N, max_batch=B)
    for key, v in options.items():
        sol.set_option(key, v)
        assert sol.get_option(key) == v
    tdt = torch.float32 if dtype == f32 else torch.float64
    poison([(B, (n * n + m * m) * N - m * m), (B, (n * n + n * m) * (N - 1)), (B, (n + m) * N - m), (B, n * N)], tdt)
    xu, goals, xs = (dev(a, dtype) for a in arrs)
    out = sol.generate_kkt(plant(which), goals, xs, xu, iiwa.TIMESTEP, QD32 if qd is None else qd, r32(N) if r is None else r)
    torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in out]
    for t in out:
        t.fill_(NAN)
    torch.cuda.synchronize()
    assert all(a.dtype == dtype and np.isfinite(a).all() for a in res), (which, N, options)
    return res


def worst_per_array(got, want):
    """[G, C, g, c] worst error over the batch, each relative to max(1, |that trajectory's array|)."""
    return [max(rel(got[i][b], want[b][i]) for b in range(len(want))) for i in range(4)]


def fig(*a):
    print("CHAIN-FIG", *a)


# ---- 0. the control: the iiwa through the export path is Plant(), bit for bit, on every entry ----
@functools.lru_cache(maxsize=None)
def merit_inputs(which, N, B, size):
    """(xu, goals, xs, dz) float32 and the genuinely double (xu, dz) for the _f64 entry (goals and xs stay float-representable)."""
    xu, goals, xs = inputs32(which, N, B, size)
    rng = np.random.default_rng([9, N, input_seed(which)])
    dz = (0.05 * rng.standard_normal(xu.shape)).astype(f32)
    xu64 = xu.astype(f64) * (1.0 + 1e-12 * rng.uniform(-1, 1, xu.shape))
    dz64 = dz.astype(f64) * (1.0 + 1e-12 * rng.uniform(-1, 1, dz.shape))
    return xu, goals, xs, dz, xu64, dz64


def merit(which, N, goals, xs, xu, dz, dtype=f32, steps=STEPS3, **options):
    from mpcgpu_amd import PcgSolver
    B = len(xu)
    sol = PcgSolver(N, max_batch=B)
    for key, v in options.items():
        sol.set_option(key, v)
    out = torch.full((B, len(steps)), NAN, dtype=torch.float32 if dtype == f32 else torch.float64, device="cuda")
    sol.compute_merit(plant(which), dev(goals, dtype), None if xs is None else dev(xs, dtype), dev(xu, dtype), None if dz is None else dev(dz, dtype),
                      steps, iiwa.TIMESTEP, MU, iiwa.QD_COST, iiwa.r_cost(N), merit=out)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert np.isfinite(res).all(), (which, N, options)
    return res


@pytest.mark.parametrize("N,B", SHAPES)
def test_the_iiwa_from_geometry_is_the_built_in_plant_bit_for_bit(N, B):
    """Chain.from_iiwa() -> tables() -> Plant(...) against Plant(): the same bits out of every KKT and merit entry.  This pins the export path the random
    chains go through."""
    a32, a64 = inputs32("iiwa", N, B, "large"), inputs64("iiwa", N, B, "large")
    calls = [("kkt", a32, f32, {}), ("kkt difference", a32, f32, {"kkt_analytic": 0}), ("kkt_f32 = 1", a32, f32, {"kkt_f32": 1}),
             ("kkt_f32 = 2", a32, f32, {"kkt_f32": 2}), ("kkt_f64", a64, f64, {}), ("kkt_f64 difference", a64, f64, {"kkt_analytic": 0})]
    for name, arrs, dtype, opts in calls:
        mine, theirs = kkt("iiwa", N, arrs, dtype, **opts), kkt("default", N, arrs, dtype, **opts)
        for x, y, arr in zip(mine, theirs, "GCgc"):
            assert np.array_equal(bits(x), bits(y)), (name, arr)
    xu, goals, xs, dz, xu64, dz64 = merit_inputs("iiwa", N, B, "large")
    for with_xs in (True, False):
        for name, args, dtype, opts in (("merit", (xu, dz), f32, {}), ("merit_f32", (xu, dz), f32, {"merit_f32": 1}), ("merit_f64", (xu64, dz64), f64, {})):
            mine, theirs = (merit(w, N, goals, xs if with_xs else None, *args, dtype=dtype, **opts) for w in ("iiwa", "default"))
            assert np.array_equal(bits(mine), bits(theirs)), (name, with_xs)


# ---- 1. mpcg_generate_kkt, float arrays ----
@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("seed", cm.SEEDS)
def test_generate_kkt_double_builds_vs_host_restatement(seed, N, B):
    """The default (float64 inside, analytic gradient recursion): 1e-6 on G, C, g, c on both sets — tests/test_gpu_kkt.py's limit.  The difference checker
    ("kkt_analytic" = 0): 3e-6 on the modest set; on the large set its quotient amplifies ID(FD(u)) - u with |u|, and the assertion is the one of
    test_analytic_gradient_does_not_depend_on_the_size_of_the_torques, over the whole large set: the next test.
    Measured worst over the nine cases per chain: analytic C 2.4e-7 / 2.8e-7 / 1.5e-7 (G, g, c below 5.5e-8), difference C on the modest set 2.4e-7."""
    for size in SIZES:
        arrs, want = inputs32(seed, N, B, size), restated32(seed, N, B, size)
        ana = worst_per_array(kkt(seed, N, arrs), want)
        dif = worst_per_array(kkt(seed, N, arrs, kkt_analytic=0), want)
        fig(f"kkt seed {seed} N {N} B {B} {size}: analytic G C g c", " ".join(f"{e:.2e}" for e in ana), "difference", " ".join(f"{e:.2e}" for e in dif))
        assert max(ana) <= 1e-6, (size, ana)
        if size == "modest":
            assert max(dif) <= 3e-6, (size, dif)


def test_analytic_gradient_is_never_worse_than_the_difference_quotient_on_the_large_set():
    """worst[analytic] <= worst[difference] + 1e-9 on C, each worst taken over the large set — every chain, shape and trajectory, 105 knots — as
    tests/test_gpu_kkt.py::test_analytic_gradient_does_not_depend_on_the_size_of_the_torques takes it over all of its trajectories.
    Why over the set and not per case: at |u| <= 20 and cond(M) of a few hundred the quotient's amplified term stays at the level of the analytic route's own floor,
    the float the link forces wait as in LDS (kkt_plant.hip.h, KktR::rec), so per knot the smaller error is the luck of two roundings — (2, 1) is ONE knot —
    and only the tails over many knots say which route is worse.  Measured per (chain, shape), analytic / difference:
      seed 1  1.36e-7 / 9.14e-8   2.36e-7 / 3.69e-7   2.12e-7 / 1.91e-7
      seed 2  2.38e-7 / 5.23e-7   7.56e-8 / 2.14e-7   2.81e-7 / 1.56e-7
      seed 3  7.74e-8 / 3.74e-8   1.08e-7 / 1.02e-7   1.46e-7 / 9.74e-8        over the set: 2.81e-7 against 5.23e-7.
    Per case the analytic route is the worse one in six of nine, per chain for seed 3: held per case this assertion fails."""
    worst = {1: 0.0, 0: 0.0}
    for seed in cm.SEEDS:
        for N, B in SHAPES:
            arrs, want = inputs32(seed, N, B, "large"), restated32(seed, N, B, "large")
            for analytic in (1, 0):
                worst[analytic] = max(worst[analytic], worst_per_array(kkt(seed, N, arrs, kkt_analytic=analytic), want)[1])
    fig(f"kkt large set, C: analytic {worst[1]:.2e} difference {worst[0]:.2e}")
    assert worst[1] <= 1e-6, worst
    assert worst[1] <= worst[0] + 1e-9, worst


@pytest.mark.parametrize("name", list(cm.CORRUPTIONS))
def test_a_wrong_table_entry_is_seen_on_the_device(name):
    """The teeth of this file, on the device: the kernel given a chain with ONE kind of table entry wrong (tests/chain_models.py::CORRUPTIONS — each still
    a valid chain, so mpcg_plant_create accepts it) against the restatement of the right chain: some array is off by more than 1e-3 of max(1, |block|),
    a thousand times the limit above.  On the iiwa three of the five would move nothing, or less than the limits."""
    from mpcgpu_amd import PcgSolver, Plant
    seed, (N, B) = cm.SEEDS[0], SHAPES[1]
    wrong = Plant(cm.tables(cm.CORRUPTIONS[name](chain(seed))))
    xu, goals, xs = (dev(a) for a in inputs32(seed, N, B, "large"))
    out = PcgSolver(N, max_batch=B).generate_kkt(wrong, goals, xs, xu, iiwa.TIMESTEP, QD32, r32(N))
    torch.cuda.synchronize()
    off = worst_per_array([t.cpu().numpy() for t in out], restated32(seed, N, B, "large"))
    fig(f"wrong table ({name}): G C g c", " ".join(f"{e:.2e}" for e in off))
    assert max(off) > 1e-3, off


@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("seed", cm.SEEDS)
def test_generate_kkt_float_builds_vs_host_restatement(seed, N, B):
    """"kkt_f32" = 1 (two knots per lane in packed float: the table constants come out of halves of scalar register pairs) and = 2 (one knot per lane):
    1e-5 against the restatement and against the default build, both sets — the limits of test_generate_kkt_in_float_arithmetic.
    Measured worst (C on the large set; G, g, c below 1e-6): packed 4.9e-6 / 5.0e-6 / 2.4e-6 for seeds 1 / 2 / 3, one knot per lane 4.9e-6 / 2.5e-6 / 1.7e-6;
    modest set 2.1e-6 at worst."""
    for size in SIZES:
        arrs, want = inputs32(seed, N, B, size), restated32(seed, N, B, size)
        dflt = kkt(seed, N, arrs)
        for build in (1, 2):
            got = kkt(seed, N, arrs, kkt_f32=build)
            err = worst_per_array(got, want)
            gap = [max(rel(got[i][b], dflt[i][b].astype(f64)) for b in range(B)) for i in range(4)]
            fig(f"kkt_f32={build} seed {seed} N {N} B {B} {size}: G C g c", " ".join(f"{e:.2e}" for e in err), "to default", " ".join(f"{e:.2e}" for e in gap))
            assert max(err) <= 1e-5, (size, build, err)
            assert max(gap) <= 1e-5, (size, build, gap)


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_packed_float_bits_do_not_depend_on_the_batch(seed):
    """"kkt_f32" = 1: which knot shares a lane with which depends on the batch, the arithmetic of a half does not — each trajectory alone against
    inside the batch of five."""
    N, B = 3, 5
    arrs = inputs32(seed, N, B, "large")
    full = kkt(seed, N, arrs, kkt_f32=1)
    for b in range(B):
        one = kkt(seed, N, tuple(a[b:b + 1] for a in arrs), kkt_f32=1)
        for x, y, arr in zip(full, one, "GCgc"):
            assert np.array_equal(bits(x[b]), bits(y[0])), (b, arr)


# ---- 2. mpcg_generate_kkt_f64 ----
# G and g on these chains: tests/test_gpu_kkt_f64.py's LIMIT_Ggc (8.8e-11) was measured on iiwa windows whose end effector is centimetres from its goal.
# Here |ee - goal| is of order 1 and the restatement's central-difference Jacobian (ee_jac, h = 1e-6) carries its rounding noise 1e-16 |ee| / h ~ 1e-10
# into g = J^T (ee - goal) and twice into G = g g^T: measured ON THE CPU as the restatement at h = 1e-6 against h = 2e-6 on these very inputs,
# 6.84e-10 at worst (tests/test_chain_models_cpu.py::test_restatement_noise_of_the_cost_arrays).  Ten times that, still 29 times below the 2e-7
# float-store rounding the entry exists to remove; c carries no derivative and keeps LIMIT_Ggc, C keeps LIMIT_C.
LIMIT_Gg_CHAIN = cm.KKT_F64_LIMIT_Gg


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("seed", cm.SEEDS)
def test_generate_kkt_f64_vs_host_restatement(seed, size):
    """Double inputs, the exact double costs of the restatement; worst error per array over the three shapes.
    Measured worst over both sets, seeds 1 / 2 / 3: G 4.6e-10 / 3.9e-10 / 6.6e-10, g 2.5e-10 / 3.3e-10 / 3.7e-10 (the restatement's ee_jac noise: above),
    c 1.4e-15 / 2.2e-15 / 8.3e-16, C 2.5e-7 / 2.5e-7 / 1.5e-7.  C is NOT the restatement's noise here (1.7e-9 at h against 2h on these inputs,
    tests/test_chain_models_cpu.py): it is the float the link forces of the analytic route wait as in LDS (kkt_plant.hip.h, KktR::rec), which this entry
    shares with the float entry so that its outputs round to that entry's bits."""
    worst = [0.0] * 4
    for N, B in SHAPES:
        got = kkt(seed, N, inputs64(seed, N, B, size), f64, qd=iiwa.QD_COST, r=iiwa.r_cost(N))
        worst = [max(w, e) for w, e in zip(worst, worst_per_array(got, restated64(seed, N, B, size)))]
    fig(f"kkt_f64 seed {seed} {size}: G C g c", " ".join(f"{e:.2e}" for e in worst))
    assert worst[3] <= LIMIT_Ggc, worst
    assert worst[1] <= LIMIT_C, worst
    assert LIMIT_Gg_CHAIN < 2e-7 and worst[0] <= LIMIT_Gg_CHAIN and worst[2] <= LIMIT_Gg_CHAIN, worst


@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("seed", cm.SEEDS)
def test_generate_kkt_f64_rounded_to_float_is_the_float_entry(seed, N, B):
    """The existing identity (tests/test_gpu_kkt_f64.py) on a non-iiwa chain: float-representable inputs and costs, both gradient routes."""
    arrs = inputs32(seed, N, B, "large")
    for analytic in (1, 0):
        o32 = kkt(seed, N, arrs, f32, kkt_analytic=analytic)
        o64 = kkt(seed, N, arrs, f64, kkt_analytic=analytic)
        for a32, a64, arr in zip(o32, o64, "GCgc"):
            assert np.array_equal(bits(a64.astype(f32)), bits(a32)), (analytic, arr)
        assert (o64[1].astype(f32).astype(f64) != o64[1]).mean() > 0.3


# ---- 3. mpcg_compute_merit ----
@functools.lru_cache(maxsize=None)
def merits_restated(seed, N, B, size, double):
    """{with_xs: [B, 3]} of the host restatement, float trial iterate or double."""
    xu, goals, xs, dz, xu64, dz64 = merit_inputs(seed, N, B, size)
    a, d = (xu64, dz64) if double else (xu, dz)
    g3 = goals.reshape(B, N, 6)
    return {w: P.merits(chain(seed), a, d, STEPS3, g3, xs if w else None, N, MU, cost=P.Cost.plain(iiwa.QD_COST, iiwa.r_cost(N)), double=double) for w in (True, False)}


@pytest.mark.parametrize("N,B", SHAPES)
@pytest.mark.parametrize("seed", cm.SEEDS)
def test_merit_vs_host_restatement(seed, N, B):
    """Step sizes 0, -1, -1/2, d_xs given and NULL, both sets.  Default build 1e-6 (test_merit_vs_host_restatement), packed "merit_f32" = 1 1e-5 (the
    documented limit of include/mpcg.h), the _f64 entry against the double trial iterate at tests/test_gpu_merit_f64.py's limit (1.2e-13).
    Merits here: 120 .. 3700.  Measured worst over the nine cases: default 5.7e-8, "merit_f32" 3.4e-7, _f64 6.8e-16."""
    worst = {"default": 0.0, "merit_f32": 0.0, "f64": 0.0}
    for size in SIZES:
        xu, goals, xs, dz, xu64, dz64 = merit_inputs(seed, N, B, size)
        for with_xs in (True, False):
            sx = xs if with_xs else None
            w32, w64 = merits_restated(seed, N, B, size, False)[with_xs], merits_restated(seed, N, B, size, True)[with_xs]
            err = lambda got, want: float((np.abs(got.astype(f64) - want) / np.maximum(1.0, np.abs(want))).max())
            worst["default"] = max(worst["default"], err(merit(seed, N, goals, sx, xu, dz), w32))
            worst["merit_f32"] = max(worst["merit_f32"], err(merit(seed, N, goals, sx, xu, dz, merit_f32=1), w32))
            worst["f64"] = max(worst["f64"], err(merit(seed, N, goals, sx, xu64, dz64, dtype=f64), w64))
        if size == "large":
            both = merits_restated(seed, N, B, size, False)
            assert (both[True][:, 1:] > both[False][:, 1:]).all()          # the initial-state term is there
    fig(f"merit seed {seed} N {N} B {B}:", " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["default"] <= 1e-6, worst
    assert worst["merit_f32"] <= 1e-5, worst
    assert worst["f64"] <= LIMIT_MERIT_F64, worst


@pytest.mark.parametrize("seed", cm.SEEDS[:1])
def test_accepted_merit_is_the_merit_of_the_new_iterate(seed):
    """compute_merit -> line_search_step -> compute_merit with step 0 on the new xu equals the new d_merit_ref bit for bit, on a random chain."""
    from mpcgpu_amd import PcgSolver
    N, B = 9, 3
    xu, goals, xs, dz, _, _ = merit_inputs(seed, N, B, "modest")
    sol = PcgSolver(N, max_batch=B)
    d_xu, d_dz = dev(xu), dev(dz)
    args, tail = (plant(seed), dev(goals), dev(xs)), (iiwa.TIMESTEP, MU, iiwa.QD_COST, iiwa.r_cost(N))
    steps = STEPS3[1:]
    mer = sol.compute_merit(*args, d_xu, d_dz, steps, *tail)
    ref = torch.full((B,), float("inf"), device="cuda")                       # anything is better: every trajectory steps
    step = sol.line_search_step(mer, steps, ref, d_dz, d_xu)
    again = sol.compute_merit(*args, d_xu, None, [0.0], *tail)
    torch.cuda.synchronize()
    assert (step.cpu().numpy() >= 0).all() and np.isfinite(again.cpu().numpy()).all()
    assert np.array_equal(bits(again)[:, 0], bits(ref))
    assert np.array_equal(ref.cpu().numpy(), mer.cpu().numpy().min(axis=1))


# ---- 4. mpcg_simulate ----
N4 = 4
SS = np.float32(2e-4)


@functools.lru_cache(maxsize=None)
def plan4(seed):
    """One trajectory at N = 4 with three clearly different controls (the large set), and its start state."""
    xu, _, xs = inputs32(seed, N4, 1, "large")
    return xu[0], xs[0]


@pytest.mark.parametrize("toff,sim", [(0, 2000), (15000, 2100)])
@pytest.mark.parametrize("seed", cm.SEEDS)
def test_simulate_vs_host_restatement(seed, toff, sim):
    """Ten substeps under one control; a knot crossing and a non-zero remainder.  1e-6 of max(1, |x|): test_simulate_vs_host_restatement's limit.  d_eePos
    against the chain's kinematics of the restated state within the 2e-5 of the reference-trajectory pin, and of the state the kernel returned within
    1e-6: there only the rounding of the float state (6e-8 x 2 pi, times a lever below 2 m) and of the float output separate the two.
    Measured worst: state 5.0e-8, eePos 5.5e-8 against the restated state and 1.6e-7 against the returned one."""
    from mpcgpu_amd import PcgSolver
    xu, xs = plan4(seed)
    d_xs, ee = dev(xs.copy()), torch.full((3,), NAN, device="cuda")
    PcgSolver(N4, max_batch=1).simulate(plant(seed), d_xs, dev(xu), iiwa.TIMESTEP, toff, sim, float(SS), eePos=ee)
    torch.cuda.synchronize()
    got, ee = d_xs.cpu().numpy().astype(f64), ee.cpu().numpy().astype(f64)
    want = P.simulate(chain(seed), xs, xu, N4, iiwa.TIMESTEP, toff, sim, SS)
    assert np.isfinite(got).all() and np.isfinite(ee).all()
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
    ee_want, ee_got = np.abs(ee - chain(seed).ee_pos(want[:7])).max(), np.abs(ee - chain(seed).ee_pos(got[:7])).max()
    fig(f"simulate seed {seed} toff {toff} sim {sim}: state {err:.2e} eePos vs restated state {ee_want:.2e} vs returned state {ee_got:.2e}")
    assert np.abs(got - xs).max() > 1e-4                                       # it moved
    assert err <= 1e-6, err
    assert ee_want <= 2e-5 and ee_got <= 1e-6, (ee_want, ee_got)


def test_simulate_of_the_iiwa_from_geometry_is_the_built_in_plant_bit_for_bit():
    from mpcgpu_amd import PcgSolver
    xu, xs = plan4("iiwa")
    out = {}
    for which in ("iiwa", "default"):
        d_xs, ee = dev(xs.copy()), torch.full((3,), NAN, device="cuda")
        PcgSolver(N4, max_batch=1).simulate(plant(which), d_xs, dev(xu), iiwa.TIMESTEP, 15000, 2100, float(SS), eePos=ee)
        torch.cuda.synchronize()
        out[which] = (d_xs.cpu().numpy(), ee.cpu().numpy())
        assert all(np.isfinite(a).all() for a in out[which])
    assert np.array_equal(bits(out["iiwa"][0]), bits(out["default"][0])) and np.array_equal(bits(out["iiwa"][1]), bits(out["default"][1]))


# ---- 5. across kernels ----
@pytest.mark.parametrize("seed", cm.SEEDS)
def test_the_defect_of_a_simulated_step_vanishes(seed):
    """xu = [x, u, x'] with x' = mpcg_simulate's one step of dt = 1/64 from (x, u): the integrator defect c_1 mpcg_generate_kkt stores vanishes to float
    rounding — 5e-6, the limit of the reference-trajectory pin (tests/test_gpu_kkt.py).  The modest set: |x'| < 16, so the rounding of x' to float is
    below 1e-6.  Measured: 2.3e-7 on each chain."""
    from mpcgpu_amd import PcgSolver
    N, B = 2, 5
    xu, goals, _ = (a.copy() for a in inputs32(seed, N, B, "modest"))
    xs = np.ascontiguousarray(xu[:, :n])
    sol = PcgSolver(N, max_batch=B)
    d_x = dev(xs.copy())
    sol.simulate(plant(seed), d_x, dev(xu), iiwa.TIMESTEP, 0, 15625, 1 / 64)
    torch.cuda.synchronize()
    xn = d_x.cpu().numpy()
    assert np.isfinite(xn).all() and np.abs(xn).max() < 16 and np.abs(xn - xs).max() > 1e-3
    xu[:, n + m:] = xn
    c = kkt(seed, N, (xu, goals, xs))[3].reshape(B, N, n)
    fig(f"defect seed {seed}: |c_1| {np.abs(c[:, 1]).max():.2e}")
    assert np.abs(c[:, 0]).max() == 0.0
    assert np.abs(c[:, 1]).max() <= 5e-6, np.abs(c[:, 1]).max()
