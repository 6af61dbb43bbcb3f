// sim_plant.hip.h — the step between two SQP solves of the MPC loop, batched: the HIP twin of simple_simulate (reference
// include/common/integrator.cuh:295-325: sim_time / 2e-4 launches of one 32-thread block and a remainder launch) as ONE launch for the whole batch and
// all substeps, and of the tracking error, just_shift, the tail fills and the start-state copy of simulateMPC (include/mpcsim.cuh:300-348: one
// cudaMemcpy per knot) as a second, dynamics-free kernel.
//
// simulate_kernel<INTEGRATOR>.  A substep is the explicit Euler step of the KKT kernel's integrator, q += dt qd, qd += dt qdd (both from the old values;
// INTEGRATOR = 1, option "sim_integrator": semi-implicit Euler, qd' = qd + dt qdd, q' = q + dt qd' — a compile-time parameter, `if constexpr` in sim_steps.inc), qdd =
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
// advance_horizon_kernel.  One workgroup per trajectory; every value that moves is LOADED, then a barrier, then stored (the source and destination
// regions of a shift overlap by one knot).  See include/mpcg.h for the order of operations.
//
// The double twins (mpcg_simulate_f64, mpcg_advance_horizon_f64; linsys_t = double): simulate_f64_kernel and advance_horizon_f64_kernel over the SAME body
// texts (sim_steps.inc, sim_advance.inc, included by both kernels of a pair with IO = float / double).  simulate_f64_kernel uses d_xs and the controls as
// they are and stores the float64 state and end-effector position without a rounding; its remainder is fmod(sim, ss) as a double (the host's part of
// the schedule: mpcg_plant.hip).  advance_horizon_f64_kernel sweeps chunks of the same number of ELEMENTS and forms the tracking error in double.
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

struct SimArgs {
    const PlantDev* plant;
    float* xs;                           // [batch][n] in/out
    const float* xu;                     // [batch][(n+m)N - m]
    float* eePos;                        // [batch][3] or NULL
    int N, batch;
    unsigned S;                          // full substeps
    double ss, toff, timestep;           // substep, time offset, knot spacing [s]
    double rem;                          // the remainder substep, (double)(float)fmod(sim, ss); 0: none
};

// mpcg_simulate_f64 (linsys_t = double): the same fields with the arrays in double.  d_xs and the controls are used as they are, the state and the end-effector
// position are stored without a rounding; rem is fmod(sim, ss) as a double.
struct SimArgsF64 {
    const PlantDev* plant;
    double* xs;
    const double* xu;
    double* eePos;
    int N, batch;
    unsigned S;
    double ss, toff, timestep;
    double rem;
};

// One body text for both (sim_steps.inc, as kkt_knots.inc and merit_points.inc): the arithmetic between load and store is float64 in either.
template <int INTEGRATOR = 0>
__global__ __launch_bounds__(KKT_THREADS, 2) void simulate_kernel(SimArgs a) {
    typedef float IO;
#include "sim_steps.inc"
}
template <int INTEGRATOR = 0>
__global__ __launch_bounds__(KKT_THREADS, 2) void simulate_f64_kernel(SimArgsF64 a) {
    typedef double IO;
#include "sim_steps.inc"
}

struct AdvanceArgs {
    float* xu; float* lambda; float* goal;                  // [batch][(n+m)N - m], [batch][n N], [batch][6 N] in/out
    const float* xs;                                        // [batch][n]
    const float* eePos;                                     // [batch][3] (shift = 1)
    const float* xu_traj; const float* goal_traj;           // the plan: traj_steps rows of (n + m) / 6
    int32_t* traj_offset; int32_t* done;                    // [batch] in/out
    float* tracking_error;                                  // [batch] out
    uint32_t n, m, N, traj_steps, traj_stride, lead, shift;
};

struct AdvanceArgsF64 {                                     // mpcg_advance_horizon_f64: the same fields with the arrays in double
    double* xu; double* lambda; double* goal;
    const double* xs;
    const double* eePos;
    const double* xu_traj; const double* goal_traj;
    int32_t* traj_offset; int32_t* done;
    double* tracking_error;
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

__global__ __launch_bounds__(ADV_THREADS) void advance_horizon_kernel(AdvanceArgs a) {
    typedef float IO;
#include "sim_advance.inc"
}
__global__ __launch_bounds__(ADV_THREADS) void advance_horizon_f64_kernel(AdvanceArgsF64 a) {
    typedef double IO;
#include "sim_advance.inc"
}

}  // namespace mpcg
