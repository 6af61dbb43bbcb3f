// sim_plant.hip.h — the step between two SQP solves of the MPC loop, batched: the HIP twin of simple_simulate (reference
// include/common/integrator.cuh:295-325: sim_time / 2e-4 launches of one 32-thread block and a remainder launch) as ONE launch for the whole batch and
// all substeps, and of the tracking error, just_shift, the tail fills and the start-state copy of simulateMPC (include/mpcsim.cuh:300-348: one
// cudaMemcpy per knot) as a second, dynamics-free kernel.
//
// simulate_kernel<IO, INTEGRATOR>.  A substep is the explicit Euler step of the KKT kernel's integrator, q += dt qd, qd += dt qdd (both from the old values;
// INTEGRATOR = 1, option "sim_integrator": semi-implicit Euler, qd' = qd + dt qdd, q' = q + dt qd' — a compile-time parameter, `if constexpr` in the kernel), qdd =
// Minv (u - bias) (the bias with the gravity vector of the plant given: rnea, kkt_plant.hip.h), so the mapping is merit_points_kernel's: a 16-lane group per trajectory, four trajectories per wavefront; lanes
// 0..6 the inertia-matrix columns and lane 7 the bias through rnea<double>, then lanes 0..6 the Cholesky solve (plant_qdd_lane: the merit kernel's
// arithmetic).  The substeps are a loop INSIDE the kernel: q, qd and sin / cos wait in the item record in LDS between them.  The schedule is the reference's,
// evaluated in IEEE double with one rounding per operation (no contraction: __dmul_rn / __dadd_rn / __ddiv_rn):
//     S = (uint32)(sim / ss) full substeps of dt = ss (host);  substep s applies u of knot idx_s = (uint32)((toff + s ss) / timestep);
//     then one substep of dt = (float)fmod(sim, ss) with the control of the LAST full substep — the reference does not recompute the index there
//     (integrator.cuh:322-324) — or of (uint32)(toff / timestep) if S = 0.  A substep is gated on its NUMBER, never on accumulated time.
// Two deliberate departures from the reference:
//   * the state is carried in float64 across the substeps of a call and rounded to float ONCE, on store (the reference rounds after every substep:
//     its T is float); the inputs are read as float and widened, as in the merit kernel;
//   * a control index beyond the last control, idx > N - 2, is clamped to N - 2 (the reference reads past its buffer there).
// A remainder of exactly 0 is not run (x + 0 f = x): sim_time 0 leaves the state as it is, bit for bit.
// The pose sweeps (lanes 8..10) run ONCE, on the final state, and only when an end-effector output is asked for.  A group without a trajectory
// recomputes the last one and writes nothing; no atomics; a trajectory's arithmetic depends on nothing but that trajectory.
// LDS per wavefront: merit_points_kernel's (4 x 840 B item records + 4 x 11 recursion records of 296 B) = 16,384 B.
//
// advance_horizon_kernel<IO>.  One workgroup per trajectory; every value that moves is LOADED, then a barrier, then stored (the source and destination
// regions of a shift overlap by one knot).  See include/mpcg.h for the order of operations.
//
// CLOCK = 1 (mpcg_simulate_clk, mpcg_simulate_clk_f64): the time offset and the simulated time are device arrays, one pair per trajectory, and the host's
// part of the schedule — toff = t 1e-6, sim = t 1e-6, S = (uint32)(sim / ss), rem = (double)(IO)fmod(sim, ss) — is evaluated by every group for its own
// trajectory, one rounding per operation (fmod is exact: the host's bits).  The substep loop has barriers and a wavefront holds four trajectories, so its
// trip count is the largest of its four groups' round counts (a wave-level maximum; no LDS): A WAVEFRONT TAKES AS LONG AS ITS LONGEST TRAJECTORY.  Each group
// predicates its own work on its own S, rem, idx and dt: it steps while k < steps, runs the pose sweeps in round k == steps and idles after that, writing
// nothing to its LDS records, so the pose records survive to the final read.  A trajectory whose done flag is set on entry, or whose times are no schedule
// (non-finite, negative, sim / ss >= 65537), has no rounds and stores nothing but — the latter — done = MPCG_DONE_BAD_CLOCK.  Read in `if constexpr` only.
// advance_horizon_clk_kernel<IO> is advance_horizon_kernel with the shift decided per trajectory from clock state in device memory (mpcsim.cuh:294-352).
//
// The double twins (mpcg_simulate_f64, mpcg_advance_horizon_f64; linsys_t = double) are the same two templates with IO = double.  simulate_kernel<double> uses
// d_xs and the controls as they are and stores the float64 state and end-effector position without a rounding; its remainder is fmod(sim, ss) as a double (the host's part of
// the schedule: mpcg_plant.hip).  advance_horizon_kernel<double> sweeps chunks of the same number of ELEMENTS and forms the tracking error in double.
#pragma once
#include "merit_plant.hip.h"
#pragma clang fp contract(fast)

namespace mpcg {

constexpr unsigned SIM_MAX_SUBSTEPS = 65536;     // MPCG_SIM_MAX_SUBSTEPS

// Lane l < PJ of a group, after round 0 (records of lanes 0..6 hold the inertia-matrix columns, lane 7's the bias): qdd_l = Minv_l . (u - bias) through the
// Cholesky solve of the symmetrised M, redundantly factorised per lane.  This is merit_points_kernel's block (merit_plant.hip.h), statement for
// statement.  It is restated here and not shared: with the block lifted into this function merit_points_kernel compiled to different instructions
// (1,729 -> 1,697, tools/_prof/diff_kernels.py), and no existing kernel may change.
__device__ __forceinline__ double plant_qdd_lane(KktLds<double>::vr* recs, KktLds<double>::item* I, const int l) {
    typedef double R;
    auto rec = [&](int j) -> KktLds<double>::vr* { return recs + j * RN_ROWS; };
    R qdd = 0.0;
    R Lm[PJ][PJ], rd[PJ];
#pragma unroll
    for (int i = 0; i < PJ; ++i)
#pragma unroll
        for (int jj = 0; jj <= i; ++jj) {
            R sv = 0.5 * (rec(jj)[RN_TAU(i)] + rec(i)[RN_TAU(jj)]);
#pragma unroll
            for (int t = 0; t < jj; ++t) sv -= Lm[i][t] * Lm[jj][t];
            if (i == jj) {
                R y = __builtin_amdgcn_rsq(sv);
                y = __builtin_elementwise_fma(y * 0.5, __builtin_elementwise_fma(-sv * y, y, 1.0), y);
                y = __builtin_elementwise_fma(y * 0.5, __builtin_elementwise_fma(-sv * y, y, 1.0), y);
                rd[i] = y;
                Lm[i][i] = sv * y;
            }
            else Lm[i][jj] = sv * rd[jj];
        }
    R y[PJ];
#pragma unroll
    for (int i = 0; i < PJ; ++i) {
        R sv = (i == l) ? 1.0 : 0.0;
#pragma unroll
        for (int t = 0; t < i; ++t) sv -= Lm[i][t] * y[t];
        y[i] = sv * rd[i];
    }
#pragma unroll
    for (int i = PJ - 1; i >= 0; --i) {
        R sv = y[i];
#pragma unroll
        for (int t = i + 1; t < PJ; ++t) sv -= Lm[t][i] * y[t];
        y[i] = sv * rd[i];
    }
#pragma unroll
    for (int i = 0; i < PJ; ++i) qdd += y[i] * (I->U[i] - rec(PJ)[RN_TAU(i)]);      // bias_i = tau_i of lane 7
    return qdd;
}

// End-effector position from the three pose sweeps of lanes 8..10 (kkt_plant.hip.h: [W_i ; V_i] = [R e_i ; R (e_i x p)])
__device__ __forceinline__ void plant_ee_pos(KktLds<double>::vr* recs, double& ee0, double& ee1, double& ee2) {
    typedef double R;
    auto rec = [&](int j) -> KktLds<double>::vr* { return recs + j * RN_ROWS; };
    R W1[3], W2[3], V0[3], V1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        W1[r] = rec(PJ + 2)[RN_AW + r]; W2[r] = rec(PJ + 3)[RN_AW + r];
        V0[r] = rec(PJ + 1)[RN_AU + r]; V1[r] = rec(PJ + 2)[RN_AU + r];
    }
    ee0 = -(W2[0] * V1[0] + W2[1] * V1[1] + W2[2] * V1[2]);
    ee1 = W2[0] * V0[0] + W2[1] * V0[1] + W2[2] * V0[2];
    ee2 = -(W1[0] * V0[0] + W1[1] * V0[1] + W1[2] * V0[2]);
}

// IO = float: mpcg_simulate; IO = double (mpcg_simulate_f64, linsys_t = double): d_xs and the controls are used as they are, the state and the end-effector
// position are stored without a rounding.
template <typename IO> struct SimArgsT {
    const PlantDev* plant;
    IO* xs;                              // [batch][n] in/out
    const IO* xu;                        // [batch][(n+m)N - m]
    IO* eePos;                           // [batch][3] or NULL
    int N, batch;
    unsigned S;                          // full substeps
    double ss, toff, timestep;           // substep, time offset, knot spacing [s]
    double rem;                          // the remainder substep, (double)(IO)fmod(sim, ss): rounded to float, or fmod's value as a double; 0: none
};
// CLOCK = 1: S, toff and rem above are not read; every trajectory forms its own from these
template <typename IO> struct SimClkArgsT : SimArgsT<IO> {
    const double* toff_us; const double* sim_us;     // [batch]
    int32_t* done;                       // [batch] in/out or NULL
};
template <typename IO, int CLOCK> struct SimArgsOf { typedef SimArgsT<IO> type; };
template <typename IO> struct SimArgsOf<IO, 1> { typedef SimClkArgsT<IO> type; };
constexpr int SIM_DONE_BAD_CLOCK = 2;            // MPCG_DONE_BAD_CLOCK

// The arithmetic between load and store is float64 for either IO: only the loads (widened, or used as they are) and the stores (rounded once, or not at all)
// depend on it.  INTEGRATOR: 0 explicit, 1 semi-implicit Euler ("sim_integrator").  (As for the KKT and merit kernels, a shared __device__ body was tried and changed the code.)
// SATURATE = 1 (a plant whose limits carry MPCG_LIMITS_SIM_SATURATE): every control applied is clamped to the plant's [u_lo, u_hi] where it is loaded and widened
// — the actuator saturates; a NaN passes.  Read in `if constexpr` only: SATURATE = 0 is the kernel it was.
// CLOCK = 1: per-trajectory times (the head of this file).  Read in `if constexpr` only: CLOCK = 0 is the kernel it was.
template <typename IO, int INTEGRATOR = 0, int SATURATE = 0, int CLOCK = 0>
__global__ __launch_bounds__(KKT_THREADS, 2) void simulate_kernel(typename SimArgsOf<IO, CLOCK>::type a) {
    typedef double R;
    typedef KktLds<R>::vr kkt_lds_vd;
    typedef KktLds<R>::item kkt_lds_item;
    typedef PlantC<R>::creal creal;
    constexpr int n = 2 * PJ, m = PJ;
    __shared__ KktItemLds<R> sI[KKT_ITEMS];
    __shared__ R sF[KKT_ITEMS][KKT_R0 * RN_ROWS];
    static_assert(sizeof(KktItemLds<R>) * KKT_ITEMS + sizeof(R) * KKT_ITEMS * KKT_R0 * RN_ROWS <= 16384, "the merit kernel's LDS budget");
    const int lane = threadIdx.x, gi = lane / KKT_GL, l = lane - gi * KKT_GL;
    kkt_lds_item* I = (kkt_lds_item*)&sI[gi];
    kkt_lds_vd* recs = (kkt_lds_vd*)&sF[gi][0];
    kkt_lds_vd* fl = recs + (l < KKT_R0 ? l : 0) * RN_ROWS;
    const PlantC<R> P{reinterpret_cast<creal*>(reinterpret_cast<unsigned long long>(a.plant))};
    const long b0 = (long)blockIdx.x * KKT_ITEMS + gi;
    const bool live = b0 < a.batch;                          // (a group without a trajectory recomputes the last one — it shares this wavefront — and writes nothing)
    const size_t b = live ? (size_t)b0 : (size_t)a.batch - 1;
    const IO* xu = a.xu + b * ((size_t)(n + m) * a.N - m);
    IO* xs = a.xs + b * n;
    const unsigned last = (unsigned)a.N - 2;                 // the last knot that has a control
    auto knot_of = [&](double t) -> unsigned {               // (uint32)(t / timestep), clamped to the last control; one rounding per operation
        const double v = __ddiv_rn(t, a.timestep);
        return v >= (double)last ? last : (unsigned)v;
    };
    if (l < n) I->Xq[l] = (double)xs[l];
    double toff = a.toff, rem = a.rem;                       // CLOCK = 1: this group's own schedule, and `own` rounds of the wavefront's `rounds`
    unsigned S = a.S, own = 0;
    bool active = live;                                      // CLOCK = 1: ... and not frozen, and with times that are a schedule
    if constexpr (CLOCK == 1) {
#pragma clang fp contract(off)                               // the host's part of the schedule: products the substep loop's sums must not fuse with
        static_assert(KKT_THREADS == 64 && KKT_GL == 16, "the wave-level maximum below: four groups of 16 lanes");
        const double tu = a.toff_us[b], su = a.sim_us[b];
        toff = tu * 1e-6;                                    // (plain operators: the __d*_rn wrappers carry their header's contraction)
        const double sim = su * 1e-6, full = sim / a.ss;
        const bool valid = tu >= 0.0 && su >= 0.0 && tu < INFINITY && su < INFINITY && full < (double)SIM_MAX_SUBSTEPS + 1.0;      // (a NaN fails every comparison)
        const bool frozen = a.done && a.done[b] != 0;
        active = live && !frozen && valid;
        S = active ? (unsigned)full : 0u;
        rem = active ? (double)(IO)fmod(sim, a.ss) : 0.0;
        if (live && !frozen && !valid && a.done && l == 0) a.done[b] = SIM_DONE_BAD_CLOCK;
    }
    unsigned idx = knot_of(toff);
    const unsigned steps = S + (rem != 0.0 ? 1u : 0u);
    unsigned rounds = steps + (a.eePos ? 1u : 0u);
    if constexpr (CLOCK == 1) {
        own = active ? rounds : 0u;
        rounds = own;
        const unsigned r16 = (unsigned)__shfl_xor((int)rounds, 16);
        rounds = r16 > rounds ? r16 : rounds;
        const unsigned r32 = (unsigned)__shfl_xor((int)rounds, 32);
        rounds = r32 > rounds ? r32 : rounds;
        rounds = (unsigned)__builtin_amdgcn_readfirstlane((int)rounds);
    }
    for (unsigned k = 0; k < rounds; ++k) {
        const bool step = k < steps;                         // the last round of a call with an end-effector output: the pose sweeps on the final state
        bool busy = true;                                    // CLOCK = 1: a group behind its own last round idles and writes nothing to its records
        if constexpr (CLOCK == 1) busy = k < own;
        double dt = rem;
        if (k < S) { idx = knot_of(__dadd_rn(toff, __dmul_rn((double)k, a.ss))); dt = a.ss; }
        if (l < m && busy) {
            if constexpr (SATURATE == 1) {
                if (step) {
                    const double u = (double)xu[(size_t)idx * (n + m) + n + l], lo = P.ulo()[l], hi = P.uhi()[l];
                    I->U[l] = u > hi ? hi : (u < lo ? lo : u);
                }
            } else
            if (step) I->U[l] = (double)xu[(size_t)idx * (n + m) + n + l];
            double sn, cs;
            kkt_sincos(I->Xq[l], sn, cs);
            I->Sc[0][l] = sn;
            I->Sc[1][l] = cs;
        }
        __syncthreads();
        // ---- round 0 of the KKT kernel: lanes 0..6 ID(q, 0, e_l), lane 7 ID(q, qd, 0); in the pose round lanes 8..10 instead ----
        if (l < KKT_R0 && busy && (step ? l <= PJ : l > PJ)) {
            R a6w[3], a6u[3];
            RneaTask<R> t;
            t.sj = -1; t.pj = -1; t.qdscale = (l == PJ) ? 1.0 : 0.0; t.knot_qdd = false; t.unit = l < PJ ? l : -1; t.base = l > PJ ? l - PJ - 1 : -1;
            rnea<R>(P, fl, I, t, a6w, a6u);
#pragma unroll
            for (int r = 0; r < 3; ++r) { fl[RN_AW + r] = a6w[r]; fl[RN_AU + r] = a6u[r]; }
        }
        __syncthreads();
        if (step && l < PJ) {                                // lanes 0..6: qdd_l, then joint l's Euler step from the old values
            const R qdd = plant_qdd_lane(recs, I, l);
            const R q = I->Xq[l], qd = I->Xq[PJ + l];
            if constexpr (INTEGRATOR == 1) {                 // semi-implicit Euler: the position moves with the NEW velocity
                const R qdn = qd + dt * qdd;
                I->Xq[l] = q + dt * qdn;
                I->Xq[PJ + l] = qdn;
            } else {
            I->Xq[l] = q + dt * qd;
            I->Xq[PJ + l] = qd + dt * qdd;
            }
        }
        __syncthreads();
    }
    if (a.eePos && active && l < 3) {
        R ee0, ee1, ee2;
        plant_ee_pos(recs, ee0, ee1, ee2);
        a.eePos[b * 3 + l] = (IO)(l == 0 ? ee0 : (l == 1 ? ee1 : ee2));
    }
    if (active && l < n) xs[l] = (IO)I->Xq[l];              // IO = float: the one rounding of the call; IO = double: the state as it is
}

template <typename IO> struct AdvanceArgsT {                // IO = float: mpcg_advance_horizon; IO = double: mpcg_advance_horizon_f64
    IO* xu; IO* lambda; IO* goal;                           // [batch][(n+m)N - m], [batch][n N], [batch][6 N] in/out
    const IO* xs;                                           // [batch][n]
    const IO* eePos;                                        // [batch][3] (shift = 1)
    const IO* xu_traj; const IO* goal_traj;                 // the plan: traj_steps rows of (n + m) / 6
    int32_t* traj_offset; int32_t* done;                    // [batch] in/out
    IO* tracking_error;                                     // [batch] out
    uint32_t n, m, N, traj_steps, traj_stride, lead, shift;
};

// (|ee0 - g0| + |ee1 - g1|) + |ee2 - g2| in the arrays' type, in that order, one rounding per operation (mpcsim.cuh:303-306)
__device__ __forceinline__ float tracking_error_of(const float* ee, const float* goal) {
    return __fadd_rn(__fadd_rn(fabsf(__fsub_rn(ee[0], goal[0])), fabsf(__fsub_rn(ee[1], goal[1]))), fabsf(__fsub_rn(ee[2], goal[2])));
}
__device__ __forceinline__ double tracking_error_of(const double* ee, const double* goal) {
    return __dadd_rn(__dadd_rn(fabs(__dsub_rn(ee[0], goal[0])), fabs(__dsub_rn(ee[1], goal[1]))), fabs(__dsub_rn(ee[2], goal[2])));
}

// Every element of the three iterates gets its new value from ONE source element (new_xu, new_goal, lambda[e + n]).  A shift moves values DOWN, so
// a sweep in ascending chunks of ADV_THREADS x ADV_KEEP elements (floats or doubles) — load the chunk's sources into registers, barrier, store, barrier — never reads
// an element that was already overwritten: what a store destroys is the source of an element of the same or an earlier chunk.
constexpr int ADV_THREADS = 256, ADV_KEEP = 8;
template <class V, class F>
__device__ __forceinline__ void advance_sweep(V* dst, const size_t count, F&& value) {
    V v[ADV_KEEP];
    for (size_t c0 = 0; c0 < count; c0 += (size_t)ADV_THREADS * ADV_KEEP) {
#pragma unroll
        for (int i = 0; i < ADV_KEEP; ++i) { const size_t e = c0 + (size_t)i * ADV_THREADS + threadIdx.x; v[i] = e < count ? value(e) : V(0); }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ADV_KEEP; ++i) { const size_t e = c0 + (size_t)i * ADV_THREADS + threadIdx.x; if (e < count) dst[e] = v[i]; }
        __syncthreads();
    }
}

// Copies only, and the tracking error in IO (tracking_error_of: one rounding per operation).
template <typename IO>
__global__ __launch_bounds__(ADV_THREADS) void advance_horizon_kernel(AdvanceArgsT<IO> a) {
    const size_t b = blockIdx.x;
    const uint32_t n = a.n, m = a.m, N = a.N, nm = n + m, t = threadIdx.x;
    const size_t len = (size_t)nm * N - m;
    IO* xu = a.xu + b * len;
    const IO* xs = a.xs + b * n;
    if (a.done && a.done[b] != 0) return;                    // frozen (uniform; done is written behind the barriers below)
    if (!a.shift) {                                          // mpcsim.cuh:348 alone
        for (uint32_t e = t; e < n; e += ADV_THREADS) xu[e] = xs[e];
        return;
    }
    IO* lam = a.lambda + b * (size_t)n * N;
    IO* goal = a.goal + b * (size_t)6 * N;
    const IO* xut = a.xu_traj + b * (size_t)a.traj_stride * nm;
    const IO* gt = a.goal_traj + b * (size_t)a.traj_stride * 6;
    const uint32_t off = (uint32_t)a.traj_offset[b] + 1;     // (:310; a value that is no row of the plan takes the else branch and reads the plan's last row)
    const bool inside = off >= 1 && (uint64_t)off + N < a.traj_steps;    // (:314, :327)
    IO err = 0;
    if (t == 0) err = tracking_error_of(a.eePos + b * 3, goal);          // (:303-306) against knot 0 of the unshifted goals
    // xu: x_0 from xs (:348, the last write of the reference); everything else below the last n + m elements from one knot up (just_shift: knots
    // 0..N-3 whole, x_{N-2} <- x_{N-1} without a control, integrator.cuh:258-263); the last n + m elements u_{N-2}, x_{N-1} from the plan (:316) or
    // the final plan position with zero velocity and zero control (:320-322).
    advance_sweep(xu, len, [&](size_t e) -> IO {
        if (e < n) return xs[e];
        if (e + nm < len) return xu[e + nm];
        const uint32_t r = (uint32_t)(e + nm - len);         // 0..m-1: u_{N-2}; m..m+n-1: x_{N-1}
        if (inside) return xut[(size_t)nm * (off + a.lead) - m + r];
        return r >= m && r - m < n / 2 ? xut[(size_t)(a.traj_steps - 1) * nm + (r - m)] : IO(0);
    });
    advance_sweep(goal, (size_t)6 * N, [&](size_t e) -> IO {         // (:326-334)
        if (e + 6 < (size_t)6 * N) return goal[e + 6];
        return gt[(size_t)(inside ? off + N - 1 : a.traj_steps - 1) * 6 + (e + 6 - (size_t)6 * N)];
    });
    advance_sweep(lam, (size_t)n * (N - 1), [&](size_t e) -> IO { return lam[e + n]; });         // the last knot of lambda keeps its value (:337-338)
    if (t == 0) {
        a.tracking_error[b] = err;
        a.traj_offset[b] = (int32_t)off;
        if (off >= a.traj_steps) a.done[b] = 1;              // (:252)
    }
}

// mpcg_advance_horizon_clk(_f64): the clock bookkeeping of mpcsim.cuh:294-352 per trajectory, in double with one rounding per operation, around what
// advance_horizon_kernel does to the trajectory with the shift it decides.  a.shift is not read; a.done is required.  The copies are that kernel's,
// restated: with the shift lifted into a function of both, advance_horizon_kernel kept its 1,171 / 1,210 instructions but not their order
// (tools/_prof/diff_kernels.py), and no existing kernel may change.
template <typename IO> struct AdvanceClkArgsT : AdvanceArgsT<IO> {
    double timestep, threshold;                             // knot spacing and SHIFT_THRESHOLD [s]
    const double* sim_us;                                   // [batch]
    double* prev_us; double* since; int32_t* shifted;       // [batch] in/out: prev_simulation_time [us], time_since_timestep [s], shifted
    int32_t* did_shift;                                     // [batch] out or NULL
};
constexpr int ADV_DONE_BAD_CLOCK = 2;                       // MPCG_DONE_BAD_CLOCK

template <typename IO>
__global__ __launch_bounds__(ADV_THREADS) void advance_horizon_clk_kernel(AdvanceClkArgsT<IO> a) {
#pragma clang fp contract(off)                              // since + t 1e-6 is a product rounded, then a sum rounded: under this file's contract(fast) it became one fma
    const size_t b = blockIdx.x;
    const uint32_t t = threadIdx.x;
    // every thread reads the flags and the clock, then a barrier: thread 0 writes them at the end, and no thread may decide on the new values
    const int32_t done = a.done[b];
    const double su = a.sim_us[b];
    const bool bad = !(su >= 0.0 && su < INFINITY);         // negative, infinite or NaN
    const double su_s = su * 1e-6;
    double since = a.since[b] + su_s;                       // (:294; plain operators: the __d*_rn wrappers carry their header's contraction)
    int32_t shifted = a.shifted[b];
    __syncthreads();
    if (done != 0) {                                        // frozen: the clock too
        if (t == 0 && a.did_shift) a.did_shift[b] = 0;
        return;
    }
    if (bad) {
        if (t == 0) a.done[b] = ADV_DONE_BAD_CLOCK;
        return;
    }
    const bool shift = shifted == 0 && since > a.threshold;             // (:296)
    const uint32_t n = a.n, m = a.m, N = a.N, nm = n + m;
    const size_t len = (size_t)nm * N - m;
    IO* xu = a.xu + b * len;
    const IO* xs = a.xs + b * n;
    if (!shift) {                                           // (:348 alone)
        for (uint32_t e = t; e < n; e += ADV_THREADS) xu[e] = xs[e];
    } else {                                                // advance_horizon_kernel's shift, restated: shared as a function, that kernel compiled to other code
        IO* lam = a.lambda + b * (size_t)n * N;
        IO* goal = a.goal + b * (size_t)6 * N;
        const IO* xut = a.xu_traj + b * (size_t)a.traj_stride * nm;
        const IO* gt = a.goal_traj + b * (size_t)a.traj_stride * 6;
        const uint32_t off = (uint32_t)a.traj_offset[b] + 1;     // (:310; a value that is no row of the plan takes the else branch and reads the plan's last row)
        const bool inside = off >= 1 && (uint64_t)off + N < a.traj_steps;    // (:314, :327)
        IO err = 0;
        if (t == 0) err = tracking_error_of(a.eePos + b * 3, goal);          // (:303-306) against knot 0 of the unshifted goals
        // xu: x_0 from xs (:348, the last write of the reference); everything else below the last n + m elements from one knot up (just_shift: knots
        // 0..N-3 whole, x_{N-2} <- x_{N-1} without a control, integrator.cuh:258-263); the last n + m elements u_{N-2}, x_{N-1} from the plan (:316) or
        // the final plan position with zero velocity and zero control (:320-322).
        advance_sweep(xu, len, [&](size_t e) -> IO {
            if (e < n) return xs[e];
            if (e + nm < len) return xu[e + nm];
            const uint32_t r = (uint32_t)(e + nm - len);         // 0..m-1: u_{N-2}; m..m+n-1: x_{N-1}
            if (inside) return xut[(size_t)nm * (off + a.lead) - m + r];
            return r >= m && r - m < n / 2 ? xut[(size_t)(a.traj_steps - 1) * nm + (r - m)] : IO(0);
        });
        advance_sweep(goal, (size_t)6 * N, [&](size_t e) -> IO {         // (:326-334)
            if (e + 6 < (size_t)6 * N) return goal[e + 6];
            return gt[(size_t)(inside ? off + N - 1 : a.traj_steps - 1) * 6 + (e + 6 - (size_t)6 * N)];
        });
        advance_sweep(lam, (size_t)n * (N - 1), [&](size_t e) -> IO { return lam[e + n]; });         // the last knot of lambda keeps its value (:337-338)
        if (t == 0) {
            a.tracking_error[b] = err;
            a.traj_offset[b] = (int32_t)off;
            if (off >= a.traj_steps) a.done[b] = 1;              // (:252)
        }
    }
    if (t == 0) {
        if (shift) shifted = 1;                             // (:340)
        if (since > a.timestep) { shifted = 0; since = fmod(since, a.timestep); }      // (:343-347; fmod is exact)
        a.since[b] = since;
        a.shifted[b] = shifted;
        a.prev_us[b] = su;                                  // (:352)
        if (a.did_shift) a.did_shift[b] = shift ? 1 : 0;
    }
}

}  // namespace mpcg
