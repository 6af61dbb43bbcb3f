"""Cases of the COST = 1 / COST = 2 plant kernels and of the saturating and clocked simulate on robots OTHER than the iiwa — TEST INFRASTRUCTURE (a
helper module, not a conftest; no torch, no GPU).  Shared by tests/test_gpu_chain_costs.py (the device side) and tests/test_chain_costs_cpu.py (the
conditions under which those cases mean anything), and read-only: every array is made once per case and never written to.

    COSTS, WEIGHTS          the two cost settings and the limit weights of tests/test_gpu_xuref.py and tests/test_gpu_limits.py (imported back there)
    bounds_of, limits_of    soft limits from a case's own values: per kind and joint the lower and upper third, nudged off every value
    far_bounds              bounds further than 2 h from every value, for the central differences of the merit
    ChainCase               inputs (chain_models.hard_inputs), dz, plan, offsets of one (seed, N, B, size, precision) and its cached restatements
    SimCase                 the plan, start states, torque limits and per-trajectory times of the simulate tests
"""
import functools

import numpy as np

import chain_models as cm
import iiwa_ref
import plant_ref as P

n, m, NJ, ROW = 14, 7, 7, 21
DT = iiwa_ref.TIMESTEP
MU = 10.0
STEPS3 = [0.0, -1.0, -0.5]
WEIGHTS = (3.0, 0.25, 0.125)                                  # q, qd, u: floats
# weights that are floats (the float entries take qd_cost and r_cost as floats; the packed build rounds ee_cost and q_cost)
COSTS = {"all": P.Cost(0.75, 0.5, 2.0 ** -6, 2.0 ** -7, P.QD_RELATIVE | P.U_RELATIVE),          # every weight positive, both flags
         "joint": P.Cost(0.0, 0.5, 2.0 ** -6, 2.0 ** -7, P.QD_RELATIVE)}                        # ee_cost = 0 with a NULL goal pointer: iiwa_plant.cuh
# (seed, N, B): every seed at (3, 5); seed 1 at the other two shapes of chain_models.SHAPES — (2, 1) one item that is first and last block at once, (9, 3)
# an odd knot count and an idle half in the packed builds
CASES = tuple((s, 3, 5) for s in cm.SEEDS) + ((1, 2, 1), (1, 9, 3))
G_LIMITS = (0.5, 0.0, 9.81)                                   # the base acceleration of the gravity-with-limits plant
H = 1e-3                                                      # the step of the merit's central differences
f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)


def bounds_of(vals):
    """(lo, hi) [7] each, float32-representable, for vals [rows, 7]: per joint the lower and upper third of its values, each bound halfway between two
    neighbours of the sorted values; a joint with fewer than three values lies below (joint % 3 == 0), inside (1) or above (2) its bounds as a whole."""
    vals = np.asarray(vals, np.float64)
    lo, hi = np.zeros(NJ), np.zeros(NJ)
    for i in range(NJ):
        s = np.sort(vals[:, i])
        if len(s) >= 3:
            k = len(s) // 3
            lo[i], hi[i] = 0.5 * (s[k - 1] + s[k]), 0.5 * (s[-k - 1] + s[-k])
        else:
            d = 0.25
            lo[i], hi[i] = ((s[-1] + d, s[-1] + 2 * d), (s[0] - d, s[-1] + d), (s[0] - 2 * d, s[0] - d))[i % 3]
    lo, hi = f32(lo), f32(hi)
    assert (lo <= hi).all() and not (vals == lo).any() and not (vals == hi).any()          # no value ON a bound
    return lo, hi


def limits_of(xs_list, us_list, weights=WEIGHTS):
    """Limits from all the states [*, 14] and controls [*, 7] given; joint 1's lower bound of every kind is -inf (one-sided).  Valid only if below, inside and
    above each occur for q, qd and u."""
    x, u = np.concatenate(xs_list), np.concatenate(us_list)
    (q_lo, q_hi), (qd_lo, qd_hi), (u_lo, u_hi) = bounds_of(x[:, :NJ]), bounds_of(x[:, NJ:]), bounds_of(u)
    for lo in (q_lo, qd_lo, u_lo):
        lo[1] = -np.inf
    lim = P.Limits(q_lo, q_hi, qd_lo, qd_hi, u_lo, u_hi, *weights)
    for name, vals, lo, hi in (("q", x[:, :NJ], q_lo, q_hi), ("qd", x[:, NJ:], qd_lo, qd_hi), ("u", u, u_lo, u_hi)):
        s = P.side(vals, lo, hi)
        assert all((s == v).any() for v in (-1, 0, 1)), name
    return lim


def far_bounds(vals, h=H):
    """(lo, hi) [7] each, float32-representable: per joint its smallest value below, its largest above, the rest inside — or, where those lie within 5 h
    of their neighbours, one bound 1/4 below all of them (tests/test_gpu_limits.py::test_merit_differences_are_the_kkt_gradient)."""
    lo, hi = np.zeros(NJ), np.zeros(NJ)
    for i in range(NJ):
        s = np.sort(vals[:, i])
        lo[i], hi[i] = 0.5 * (s[0] + s[1]), 0.5 * (s[-2] + s[-1])
        if min(s[1] - s[0], s[-1] - s[-2]) <= 5 * h:
            lo[i], hi[i] = -np.inf, s[0] - 0.25
    return f32(lo), f32(hi)


@functools.lru_cache(maxsize=None)
def chain(seed):
    return cm.random_chain(seed)


@functools.lru_cache(maxsize=None)
def model(seed, gravity=None):
    """The restatement's model: the chain, or the chain whose recursion starts from the base acceleration `gravity` (tests/gravity_ref.py)."""
    if gravity is None:
        return chain(seed)
    import gravity_ref                                         # (here: it brings the package, and torch with it, which the other cases do without)
    return gravity_ref.chain(seed, gravity)


class ChainCase:
    """Inputs of one chain and shape: chain_models.hard_inputs rounded to float32 and widened — or (double) those times 1 + 1e-12 r, none of them a
    float —, dz = 0.05 standard_normal, a plan of T = N + 1 rows of 0.5 standard_normal — shared by the batch, or ((3, 5)) one per trajectory at a stride of
    T + 2 rows with NaN in the two rows between the plans — and offsets that cycle through -1 (clamps at the first row), T - 2 (clamps at the last row from
    knot 1 on) and 1 (inside)."""

    def __init__(self, seed, N, B, size="large", double=False):
        self.seed, self.N, self.B, self.size, self.double = seed, N, B, size, double
        xu, goals, xs = cm.hard_inputs(N, B, cm.input_seed(seed), size)
        rng = np.random.default_rng([13, seed, N, B, 0 if size == "large" else 1])
        dz = 0.05 * rng.standard_normal(xu.shape)
        self.T = T = N + 1
        self.stride = T + 2 if (N, B) == (3, 5) else 0
        plan = 0.5 * rng.standard_normal((B * self.stride if self.stride else T, ROW))
        arrs = [f32(a) for a in (xu, goals.reshape(B, -1), xs, dz, plan)]
        if double:
            arrs = [a * (1.0 + 1e-12 * rng.uniform(-1, 1, a.shape)) for a in arrs]
            assert all((a != a.astype(np.float32)).mean() > 0.9 for a in arrs)
        self.xu, self.goals, self.xs, self.dz, self.plan = arrs
        if self.stride:
            for b in range(B):
                self.plan[b * self.stride + T:(b + 1) * self.stride] = np.nan
        self.offsets = np.array([(-1, T - 2, 1)[b % 3] for b in range(B)], np.int32)
        for a in arrs + [self.offsets]:
            a.setflags(write=False)
        self._dyn, self._merits = {}, {}

    def rows(self, b):
        return P.plan_rows(self.plan, b, self.offsets[b], self.N, self.T, self.stride)

    def own_plan(self, b):
        """Trajectory b's plan alone [T, 21]: what a call on that trajectory by itself is given (stride 0)."""
        return self.plan[b * self.stride:b * self.stride + self.T] if self.stride else self.plan

    def states_controls(self, steps):
        """The states and controls of every trajectory at the trial iterates of `steps` (step size 0: the iterate itself)."""
        xs, us = [], []
        for b in range(self.B):
            for a in steps:
                x, u = P.split(P.trial(self.xu[b], self.dz[b], a, self.double), self.N)
                xs.append(x)
                us.append(u)
        return xs, us

    @functools.cached_property
    def kkt_limits(self):
        return limits_of(*self.states_controls([0.0]))

    @functools.cached_property
    def merit_limits(self):
        return limits_of(*self.states_controls(STEPS3))

    def dynamics(self, b, integrator, gravity=None):
        """The cost-independent part of the restatement (the slow part), once per trajectory, integrator and base acceleration."""
        key = (b, integrator, gravity)
        if key not in self._dyn:
            self._dyn[key] = P.dynamics(model(self.seed, gravity), self.xu[b], self.goals[b], self.xs[b], self.N, DT, integrator)
        return self._dyn[key]

    def want_kkt(self, b, cost, integrator=0, limits=False, gravity=None):
        """(G, C, g, c) of trajectory b: cost "all" / "joint" (COST = 1), with the case's kkt_limits (COST = 2)."""
        co = COSTS[cost]
        return P.generate_kkt(model(self.seed, gravity), self.xu[b], None if co.ee_cost == 0 else self.goals[b], self.xs[b], self.N, rows=self.rows(b), cost=co,
                              limits=self.kkt_limits if limits else None, dt=DT, integrator=integrator, base=self.dynamics(b, integrator, gravity))

    def want_merits(self, cost, with_xs, integrator=0, limits=False, gravity=None):
        """[B, 3] at STEPS3; with limits the penalty of merit_limits is added to the cached plain merits."""
        key = (cost, with_xs, integrator, gravity)
        co = COSTS[cost]
        if key not in self._merits:
            w = P.merits(model(self.seed, gravity), self.xu, self.dz, STEPS3, None if co.ee_cost == 0 else self.goals, self.xs if with_xs else None, self.N, MU,
                         rows_of=self.rows, cost=co, dt=DT, integrator=integrator, double=self.double)
            w.setflags(write=False)
            self._merits[key] = w
        base = self._merits[key]
        if not limits:
            return base
        return P.merits(None, self.xu, self.dz, STEPS3, None, None, self.N, MU, cost=co, limits=self.merit_limits, double=self.double, base=base)


@functools.lru_cache(maxsize=None)
def case(seed, N, B, size="large", double=False):
    return ChainCase(seed, N, B, size, double)


# ---- the device-against-device case: seed 1, N = 3, cost "joint", bounds further than 2 h from every value ----
@functools.lru_cache(maxsize=None)
def far_limits():
    """Limits for the five trajectories of case(1, 3, 5, "large", True) from all their values at once (one trajectory has two controls per joint: too
    few for three sides)."""
    xs, us = case(1, 3, 5, "large", True).states_controls([0.0])
    x, u = np.concatenate(xs), np.concatenate(us)
    return P.Limits(*far_bounds(x[:, :NJ]), *far_bounds(x[:, NJ:]), *far_bounds(u), *WEIGHTS)


# ---- simulate ----
N4 = 4
TIMES = ((0.0, 0.0), (15000.0, 2100.0), (0.0, 2000.0), (4000.0, 650.0), (15000.0, 2100.0))          # zero time; knot crossing and remainder; ten substeps; S = 3 and a remainder; (frozen)
FROZEN = 4
CROSSING = (15000.0, 2100.0)


class SimCase:
    """Chain seed 1 at N = 4: B trajectories of the large set (float32-representable, or genuinely double), and torque limits at the thirds of the controls
    a schedule can apply (knots 0 .. N - 2)."""

    def __init__(self, B, double=False):
        self.B, self.double = B, double
        xu, _, xs = cm.hard_inputs(N4, B, cm.input_seed(1), "large")
        xu, xs = f32(xu), f32(xs)
        if double:
            rng = np.random.default_rng([17, B])
            xu, xs = (a * (1.0 + 1e-12 * rng.uniform(-1, 1, a.shape)) for a in (xu, xs))
        self.xu, self.xs = xu, xs
        u = np.concatenate([P.split(z, N4)[1] for z in xu])
        lo, hi = bounds_of(u)
        self.limits = P.Limits(u_lo=lo, u_hi=hi, u_weight=WEIGHTS[2])
        clamped = xu.copy()
        for k in range(N4 - 1):
            c = clamped[:, ROW * k + n:ROW * (k + 1)]
            c[:] = np.minimum(np.maximum(c, lo), hi)
        self.clamped = clamped
        for a in (self.xu, self.xs, self.clamped):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def sim_case(B, double=False):
    return SimCase(B, double)
