// merit_plant.hip.h — the merit function of the SQP line search, batched over trajectories AND step sizes: the HIP twin of ls_gato_compute_merit /
// compute_merit (reference include/common/merit.cuh:16-143) with the plant functions they call (gato_plant::trackingcost,
// include/dynamics/iiwa/iiwa_eepos_plant.cuh:242-290; integratorError, include/common/integrator.cuh) — and the step selection + update of
// include/pcg/sqp.cuh:292-301, 317, 332-338, 352 as a second, dynamics-free kernel.
//
//     merit(b, a) = sum_{k<N} J_k + mu ( sum_{k<N-1} | x_{k+1} - (x_k + dt [qd_k; qdd_k]) |_1  +  [xs given] | x_0 - xs_b |_1 )      at z = xu_b + alpha_a dz_b
//     J_k = 1/2 |ee(q_k) - goal_k|^2 + 1/2 qd_cost |qd_k|^2 + [k < N-1] 1/2 r_cost |u_k|^2
//
// The integrator is a compile-time parameter of the three point-merit kernels (INTEGRATOR, option "integrator": the one mpcg_generate_kkt reads, merit.cuh:99):
// 0 the explicit Euler step above, 1 semi-implicit Euler, | x_{k+1} - [q_k + dt (qd_k + dt qdd_k); qd_k + dt qdd_k] |_1 (integrator.cuh:22-57).
//
// What a point merit needs is what round 0 of generate_kkt_kernel (kkt_plant.hip.h) computes — qdd = M^-1 (u - bias) and the end-effector position —
// so the mapping is that kernel's: a 16-lane group per work item (trajectory, step size, knot), four items per wavefront; lanes 0..6 the
// inertia-matrix columns, lane 7 the bias, lanes 8..10 the pose sweeps through the same rnea<double>, then lanes 0..6 the Cholesky solve.  There is no
// gradient round and no matrix output: an item writes ONE double.  The last knot of a trajectory is an item too (N per trajectory and step, not N-1):
// its cost is evaluated at its own state x_{N-1} against goal_{N-1} (merit.cuh:62 — not the _lastblock quirk of the KKT kernel) and needs the pose
// sweeps only.
// The trial iterate is formed in FLOAT with one rounding, fmaf(alpha, dz, xu), and widened: the float line_search_step_kernel stores for the accepted
// step size is the float this kernel evaluated, so the merit of the new iterate (step size 0) is the accepted merit bit for bit.  A step size of 0
// reads no dz at all.
// Sums have a fixed order and use no atomics (the reference's compute_merit adds its point merits with atomicAdd): lanes 0..6 of a group each hold one
// joint's share of the point merit and lane 0 adds them in lane order; the point merits wait as doubles in a handle-owned scratch [batch][16][N], and
// merit_sum_kernel adds a row knot by knot and rounds ONCE to float.  An item's arithmetic depends on nothing but its own (trajectory, step size,
// knot): results are bitwise reproducible and independent of the rest of the batch and of the other step sizes of the call.
// The double twins (mpcg_compute_merit_f64, mpcg_line_search_step(_rho)_f64; linsys_t = double): merit_points_f64_kernel over the SAME body text
// (merit_points.inc, included by both kernels) with double loads and the trial iterate fma(alpha, dz, xu) in double; merit_sum_f64_kernel stores the double
// sum itself; line_search_step_kernel over StepArgsF64 / StepRhoArgsF64.
// LDS per wavefront: the KKT kernel's item records (4 x 840 B) + 11 recursion records per item (4 x 3,256 B) = 16,384 B — its budget exactly.
#pragma once
#include <type_traits>
#include "kkt_plant.hip.h"
#pragma clang fp contract(fast)

namespace mpcg {

constexpr int MERIT_MAX_STEPS = 16;      // MPCG_MAX_STEP_SIZES; also the row stride of the point-merit scratch

// One rounding per operation in the arrays' type (nothing contracts: these are the intrinsics), correctly rounded divisions
__device__ __forceinline__ float step_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
__device__ __forceinline__ double step_fma(double a, double b, double c) { return __fma_rn(a, b, c); }
__device__ __forceinline__ float step_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double step_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float step_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double step_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ float step_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double step_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ float step_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double step_min(double a, double b) { return fmin(a, b); }

struct MeritArgs {
    const PlantDev* plant;
    const float* eePos_traj;             // [batch][N][6]
    const float* xs;                     // [batch][n] or NULL: no initial-state term (the reference's compute_merit, merit.cuh:133-135)
    const float* xu;                     // [batch][(n+m)N - m]
    const float* dz;                     // same shape; NULL allowed when every step size is 0
    double* point;                       // [batch][MERIT_MAX_STEPS][N] point merits
    int N, batch, A;
    double dt, mu, qd_cost, r_cost;
    float alpha[MERIT_MAX_STEPS];
};
// mpcg_compute_merit_f64 (linsys_t = double): the same fields with every array in double.  The trial iterate is fma(alpha, dz, xu) in DOUBLE with one
// rounding — the double line_search_step_kernel stores; float64 inside only: "merit_f32" does not apply to this entry.
struct MeritArgsF64 {
    const PlantDev* plant;
    const double* eePos_traj;
    const double* xs;
    const double* xu;
    const double* dz;
    double* point;
    int N, batch, A;
    double dt, mu, qd_cost, r_cost;
    double alpha[MERIT_MAX_STEPS];
};

template <int INTEGRATOR = 0>
__global__ __launch_bounds__(KKT_THREADS, 2) void merit_points_kernel(MeritArgs a) {
    typedef float IO;
#include "merit_points.inc"
}
template <int INTEGRATOR = 0>
__global__ __launch_bounds__(KKT_THREADS, 2) void merit_points_f64_kernel(MeritArgsF64 a) {
    typedef double IO;
#include "merit_points.inc"
}

// One thread per (trajectory, step size): the point merits of its row added knot by knot, rounded once (T = double: the sum itself).
template <typename T>
__device__ __forceinline__ void merit_sum(const double* point, T* merit, int N, int A, int rows) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    const int b = r / A, ai = r - b * A;
    const double* p = point + ((size_t)b * MERIT_MAX_STEPS + ai) * N;
    double s = p[0];
#pragma unroll 8
    for (int k = 1; k < N; ++k) s += p[k];
    merit[r] = (T)s;
}
__global__ __launch_bounds__(64) void merit_sum_kernel(const double* point, float* merit, int N, int A, int rows) { merit_sum(point, merit, N, A, rows); }
__global__ __launch_bounds__(64) void merit_sum_f64_kernel(const double* point, double* merit, int N, int A, int rows) { merit_sum(point, merit, N, A, rows); }

// The step selection of include/pcg/sqp.cuh:292-301 and the update :317, 332-338, 352, per trajectory (one workgroup each): strict comparison, the
// first of equals wins, a NaN never wins; p >= 0: xu = fmaf(alpha_p, dz, xu) — the float merit_points_kernel evaluated — and merit_ref = merit[p];
// p = -1: xu and merit_ref are not written.
struct StepArgs {
    const float* merit;                  // [batch][A]
    float* merit_ref;                    // [batch] in/out
    const float* dz;
    float* xu;
    int32_t* step;                       // [batch] out
    int A;
    size_t len;                          // (n + m) N - m
    float alpha[MERIT_MAX_STEPS];
    typedef float real;
};
struct StepArgsF64 {                     // mpcg_line_search_step_f64: the same fields in double
    const double* merit;
    double* merit_ref;
    const double* dz;
    double* xu;
    int32_t* step;
    int A;
    size_t len;
    double alpha[MERIT_MAX_STEPS];
    typedef double real;
};

// mpcg_line_search_step_rho: the same selection and update, then the rho adaptation of sqp.cuh:304-320 per trajectory, in float with one rounding
// per operation (nothing here can contract: no product feeds an addition) and correctly rounded divisions:
//   p < 0 :  drho = max(drho * f, f);      rho = max(rho * drho, rho_min);  rho > rho_max: rho = rho_reset, done = 1
//   p >= 0:  drho = min(drho / f, 1 / f);  rho = max(rho * drho, rho_min)
// A trajectory with done != 0 on entry is frozen: step = STEP_FROZEN and nothing else is written.
struct StepRhoArgs : StepArgs {
    float* rho;                          // [batch] in/out
    float* drho;                         // [batch] in/out
    uint8_t* done;                       // [batch] in/out
    float factor, rho_min, rho_max, rho_reset;
};
struct StepRhoArgsF64 : StepArgsF64 {    // mpcg_line_search_step_rho_f64: the rule above in double (__dmul_rn, __ddiv_rn, fmax, fmin)
    double* rho;
    double* drho;
    uint8_t* done;
    double factor, rho_min, rho_max, rho_reset;
};
constexpr int32_t STEP_FROZEN = -2;      // MPCG_STEP_FROZEN
template <typename T> struct StepTypes { typedef StepArgs plain; typedef StepRhoArgs with_rho; };
template <> struct StepTypes<double> { typedef StepArgsF64 plain; typedef StepRhoArgsF64 with_rho; };

// SA = StepArgs(F64): mpcg_line_search_step(_f64); SA = StepRhoArgs(F64): mpcg_line_search_step_rho(_f64) — one selection, one update
template <class SA = StepArgs>
__global__ __launch_bounds__(256) void line_search_step_kernel(SA a) {
    typedef typename SA::real T;
    constexpr bool RHO = std::is_same<SA, typename StepTypes<T>::with_rho>::value;
    const size_t b = blockIdx.x;
    if constexpr (RHO) {
        if (a.done[b] != 0) {                                // (uniform; nobody in this workgroup writes done before the barrier below)
            if (threadIdx.x == 0) a.step[b] = STEP_FROZEN;
            return;
        }
    }
    T best = a.merit_ref[b], al = 0;
    int p = -1;
#pragma unroll
    for (int i = 0; i < MERIT_MAX_STEPS; ++i)
        if (i < a.A) {
            const T v = a.merit[b * a.A + i];
            if (v < best) { best = v; p = i; al = a.alpha[i]; }
        }
    __syncthreads();                                         // every thread has read merit_ref
    if (threadIdx.x == 0) {
        a.step[b] = p;
        if (p >= 0) a.merit_ref[b] = best;
        if constexpr (RHO) {
            T rho = a.rho[b], drho = a.drho[b];
            if (p < 0) {
                drho = step_max(step_mul(drho, a.factor), a.factor);
                rho = step_max(step_mul(rho, drho), a.rho_min);
                if (rho > a.rho_max) { rho = a.rho_reset; a.done[b] = 1; }
            } else {
                drho = step_min(step_div(drho, a.factor), step_div(T(1), a.factor));
                rho = step_max(step_mul(rho, drho), a.rho_min);
            }
            a.rho[b] = rho; a.drho[b] = drho;
        }
    }
    if (p < 0) return;
    const T* dz = a.dz + b * a.len;
    T* xu = a.xu + b * a.len;
    for (size_t e = threadIdx.x; e < a.len; e += 256) xu[e] = step_fma(al, dz[e], xu[e]);
}

}  // namespace mpcg
