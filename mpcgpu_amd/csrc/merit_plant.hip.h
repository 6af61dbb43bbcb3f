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
// The double twins (mpcg_compute_merit_f64, mpcg_line_search_step(_rho)_f64; linsys_t = double) are the same templates: merit_points_kernel<double, INTEGRATOR>
// with double loads and the trial iterate fma(alpha, dz, xu) in double; merit_sum_kernel<double> stores the double sum itself; line_search_step_kernel over
// StepArgsT<double> / StepRhoArgsT<double>.
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

// IO: the type of the arrays and of the step sizes; S: the type of the model tables and of the scalars (float: merit_points_f32_kernel, merit_plant_f32.hip.h).
// IO = double (mpcg_compute_merit_f64, linsys_t = double): the trial iterate is fma(alpha, dz, xu) in DOUBLE with one rounding — the double
// line_search_step_kernel stores; float64 inside only: "merit_f32" does not apply to that entry.
template <typename IO, typename S = double> struct MeritArgsT {
    const PlantDevT<S>* plant;
    const IO* eePos_traj;                // [batch][N][6]
    const IO* xs;                        // [batch][n] or NULL: no initial-state term (the reference's compute_merit, merit.cuh:133-135)
    const IO* xu;                        // [batch][(n+m)N - m]
    const IO* dz;                        // same shape; NULL allowed when every step size is 0
    double* point;                       // [batch][MERIT_MAX_STEPS][N] point merits
    int N, batch, A;
    S dt, mu, qd_cost, r_cost;
    IO alpha[MERIT_MAX_STEPS];
};

// COST = 1 (mpcg_compute_merit_xuref): J_k of the generalised cost (kkt_plant.hip.h, XuRefT) — every knot, the last one included, at its own state against its own plan row
template <typename IO, typename S = double> struct MeritXuArgsT : MeritArgsT<IO, S> { XuRefT<S, IO> ref; };
template <int COST, typename IO, typename S> struct MeritArgsSel { typedef MeritArgsT<IO, S> type; };
template <typename IO, typename S> struct MeritArgsSel<1, IO, S> { typedef MeritXuArgsT<IO, S> type; };
// COST = 2 (the plant given has limits): COST = 1 plus the limits penalty of kkt_plant.hip.h (KktArgsSel<2>), every knot at its own state; the arguments are COST = 1's
template <typename IO, typename S> struct MeritArgsSel<2, IO, S> { typedef MeritXuArgsT<IO, S> type; };

// IO = float: mpcg_compute_merit; IO = double: mpcg_compute_merit_f64.  Only the loads and the trial iterate depend on IO; INTEGRATOR: 0 explicit, 1 semi-implicit
// Euler; COST: 0 the end-effector plant's cost, 1 the generalised cost, 2 that plus the plant's soft limits (`if constexpr` only).  (A shared __device__ body was tried and changed the float kernel's code.)
template <typename IO, int INTEGRATOR = 0, int COST = 0>
__global__ __launch_bounds__(KKT_THREADS, 2) void merit_points_kernel(typename MeritArgsSel<COST, IO, double>::type a) {
    typedef double R;
    typedef KktLds<R>::vr kkt_lds_vd;
    typedef KktLds<R>::item kkt_lds_item;
    typedef PlantC<R>::creal creal;
    constexpr int n = 2 * PJ, m = PJ;
    __shared__ KktItemLds<R> sI[KKT_ITEMS];
    __shared__ R sF[KKT_ITEMS][KKT_R0 * RN_ROWS];
    static_assert(sizeof(KktItemLds<R>) * KKT_ITEMS + sizeof(R) * KKT_ITEMS * KKT_R0 * RN_ROWS <= 16384, "the KKT kernel's LDS budget: ten wavefronts per CU");
    const int lane = threadIdx.x, gi = lane / KKT_GL, l = lane - gi * KKT_GL;
    kkt_lds_item* I = (kkt_lds_item*)&sI[gi];
    kkt_lds_vd* recs = (kkt_lds_vd*)&sF[gi][0];
    auto rec = [&](int j) -> kkt_lds_vd* { return recs + j * RN_ROWS; };
    kkt_lds_vd* fl = rec(l < KKT_R0 ? l : 0);
    const PlantC<R> P{reinterpret_cast<creal*>(reinterpret_cast<unsigned long long>(a.plant))};
    const int N = a.N;
    const long per_traj = (long)a.A * N, total = (long)a.batch * per_traj;
    const size_t xu_len = (size_t)(n + m) * N - m;
    // consecutive items per wavefront, as the KKT kernel: the four point merits of a trip are neighbours in the scratch
    const long groups = (total + KKT_ITEMS - 1) / KKT_ITEMS, per = (groups + gridDim.x - 1) / gridDim.x;
    const long g_begin = (long)blockIdx.x * per, g_end = g_begin + per < groups ? g_begin + per : groups;
    for (long grp = g_begin; grp < g_end; ++grp) {
        const long item0 = grp * KKT_ITEMS + gi;
        const bool live = item0 < total;                     // (a group without an item recomputes the last one and writes nothing)
        const long item = live ? item0 : total - 1;
        const int b = (int)(item / per_traj);
        const int rem = (int)(item - (long)b * per_traj);
        const int ai = rem / N, k = rem - ai * N;
        const bool dyn = k < N - 1;                          // the last knot has no control and no successor: cost only
        IO alpha = 0;
#pragma unroll
        for (int i = 0; i < MERIT_MAX_STEPS; ++i) alpha = i == ai ? a.alpha[i] : alpha;
        const bool moved = alpha != 0;
        const IO* xu = a.xu + (size_t)b * xu_len;
        const IO* dz = moved ? a.dz + (size_t)b * xu_len : nullptr;
        auto trial = [&](size_t e) -> double {               // one rounding in the arrays' type (float: then widened)
            IO x = xu[e];
            if (moved) x = step_fma(alpha, dz[e], x);
            return (double)x;
        };
        const size_t xk = (size_t)k * (n + m);
        double ul = 0.0, xn_q = 0.0, xn_qd = 0.0;
        [[maybe_unused]] int roff = 0;                       // COST = 1: the plan offset is asked for here, the row that depends on it behind the sines and cosines
        if constexpr (COST >= 1) roff = a.ref.offset(b);
        if (l < n) I->Xq[l] = trial(xk + l);
        if (l < m) {
            if (dyn) { ul = trial(xk + n + l); xn_q = trial(xk + (n + m) + l); xn_qd = trial(xk + (n + m) + PJ + l); }
            I->U[l] = ul;
            double sn, cs;
            kkt_sincos(trial(xk + l), sn, cs);
            I->Sc[0][l] = sn;
            I->Sc[1][l] = cs;
        }
        // COST = 1: joint l's entries of the knot's plan row, read ONCE per item, here, kept as the arrays' type (every lane reads: lanes 7..15 an entry they drop;
        // a row has its 21 entries at the last knot too)
        [[maybe_unused]] IO rvq = 0, rvqd = 0, rvu = 0;
        if constexpr (COST >= 1) {
            const IO* ref = a.ref.row(b, roff, k) + (l < m ? l : m - 1);
            rvq = ref[0]; rvqd = ref[PJ]; rvu = ref[n];
        }
        __syncthreads();
        // ---- round 0 of the KKT kernel: lanes 0..6 ID(q, 0, e_l), lane 7 ID(q, qd, 0), lanes 8..10 the pose sweeps (the last knot: those only) ----
        if (l < KKT_R0 && (dyn || l > PJ)) {
            R a6w[3], a6u[3];
            RneaTask<R> t;
            t.sj = -1; t.pj = -1; t.qdscale = (l == PJ) ? 1.0 : 0.0; t.knot_qdd = false; t.unit = l < PJ ? l : -1; t.base = l > PJ ? l - PJ - 1 : -1;
            rnea<R>(P, fl, I, t, a6w, a6u);
#pragma unroll
            for (int r = 0; r < 3; ++r) { fl[RN_AW + r] = a6w[r]; fl[RN_AU + r] = a6u[r]; }
        }
        __syncthreads();
        // ---- lanes 0..6: qdd_l = Minv_l . (u - bias) through the Cholesky solve of the symmetrised M (as the KKT kernel), then joint l's share of the point merit ----
        if (l < PJ) {
            R qdd = 0.0;
            if (dyn) {
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
            }
            // end-effector position from the three pose sweeps (kkt_plant.hip.h: [W_i ; V_i] = [R e_i ; R (e_i x p)])
            R W1[3], W2[3], V0[3], V1[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                W1[r] = rec(PJ + 2)[RN_AW + r]; W2[r] = rec(PJ + 3)[RN_AW + r];
                V0[r] = rec(PJ + 1)[RN_AU + r]; V1[r] = rec(PJ + 2)[RN_AU + r];
            }
            const R ee0 = -(W2[0] * V1[0] + W2[1] * V1[1] + W2[2] * V1[2]);
            const R ee1 = W2[0] * V0[0] + W2[1] * V0[1] + W2[2] * V0[2];
            const R ee2 = -(W1[0] * V0[0] + W1[1] * V0[1] + W1[2] * V0[2]);
            const R q = I->Xq[l], qd = I->Xq[PJ + l];
            R pm;
            if constexpr (COST >= 1) { const R dqd = qd - ((a.ref.flags & XUREF_QD_RELATIVE) != 0 ? (R)rvqd : 0.0); pm = 0.5 * a.qd_cost * dqd * dqd; }
            else pm = 0.5 * a.qd_cost * qd * qd;
            if (l < 3) {                                     // lanes 0..2: one coordinate of the tracking error each
                if constexpr (COST >= 1) {
                    if (a.eePos_traj) {                      // (NULL with ee_cost = 0: no goal is read)
                        const IO* goal = a.eePos_traj + ((size_t)b * N + k) * 6;
                        const R d = (l == 0 ? ee0 : (l == 1 ? ee1 : ee2)) - (R)goal[l];
                        pm += 0.5 * a.ref.ee_cost * d * d;
                    }
                } else {
                const IO* goal = a.eePos_traj + ((size_t)b * N + k) * 6;
                const R d = (l == 0 ? ee0 : (l == 1 ? ee1 : ee2)) - (R)goal[l];
                pm += 0.5 * d * d;
                }
            }
            R viol = 0.0;
            if (dyn) {
                if constexpr (COST >= 1) { const R du = ul - ((a.ref.flags & XUREF_U_RELATIVE) != 0 ? (R)rvu : 0.0); pm += 0.5 * a.r_cost * du * du; }
                else
                pm += 0.5 * a.r_cost * ul * ul;
                if constexpr (INTEGRATOR == 1) {                  // semi-implicit Euler: q' = q + dt qd', qd' = qd + dt qdd (the map the KKT kernel linearised)
                    const R qdn = qd + a.dt * qdd;
                    viol = fabs(xn_q - (q + a.dt * qdn)) + fabs(xn_qd - qdn);
                } else
                viol = fabs(xn_q - (q + a.dt * qd)) + fabs(xn_qd - (qd + a.dt * qdd));
            }
            if (k == 0 && a.xs) viol += fabs(q - (R)a.xs[(size_t)b * n + l]) + fabs(qd - (R)a.xs[(size_t)b * n + PJ + l]);
            if constexpr (COST >= 1) { const R dq = q - (R)rvq; pm += 0.5 * a.ref.q_cost * dq * dq; }      // the joint-space term: behind the existing ones
            if constexpr (COST == 2) {                       // the limits penalty of joint l: behind that (this lane's own bounds, read here)
                const R vq = lim_viol(q, (R)P.xlo()[l], (R)P.xhi()[l]), vqd = lim_viol(qd, (R)P.xlo()[PJ + l], (R)P.xhi()[PJ + l]);
                pm += 0.5 * P.limw()[0] * vq * vq;
                pm += 0.5 * P.limw()[1] * vqd * vqd;
                if (dyn) { const R vu = lim_viol(ul, (R)P.ulo()[l], (R)P.uhi()[l]); pm += 0.5 * P.limw()[2] * vu * vu; }
            }
            I->Gq[l] = pm + a.mu * viol;
        }
        __syncthreads();
        if (l == 0 && live) {                                // the group's sum, in lane order
            R s = I->Gq[0];
#pragma unroll
            for (int i = 1; i < PJ; ++i) s += I->Gq[i];
            a.point[((size_t)b * MERIT_MAX_STEPS + ai) * N + k] = s;
        }
        __syncthreads();
    }
}

// One thread per (trajectory, step size): the point merits of its row added knot by knot, rounded once (T = double: the sum itself).
template <typename T>
__global__ __launch_bounds__(64) void merit_sum_kernel(const double* point, T* merit, int N, int A, int rows) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    const int b = r / A, ai = r - b * A;
    const double* p = point + ((size_t)b * MERIT_MAX_STEPS + ai) * N;
    double s = p[0];
#pragma unroll 8
    for (int k = 1; k < N; ++k) s += p[k];
    merit[r] = (T)s;
}

// The step selection of include/pcg/sqp.cuh:292-301 and the update :317, 332-338, 352, per trajectory (one workgroup each): strict comparison, the
// first of equals wins, a NaN never wins; p >= 0: xu = fma(alpha_p, dz, xu) in T — what merit_points_kernel<T> evaluated — and merit_ref = merit[p];
// p = -1: xu and merit_ref are not written.  T = float: mpcg_line_search_step; T = double: mpcg_line_search_step_f64.
template <typename T> struct StepArgsT {
    const T* merit;                      // [batch][A]
    T* merit_ref;                        // [batch] in/out
    const T* dz;
    T* xu;
    int32_t* step;                       // [batch] out
    int A;
    size_t len;                          // (n + m) N - m
    T alpha[MERIT_MAX_STEPS];
    typedef T real;
};

// mpcg_line_search_step_rho(_f64): the same selection and update, then the rho adaptation of sqp.cuh:304-320 per trajectory, in T with one rounding
// per operation (nothing here can contract: no product feeds an addition; step_mul, step_div, step_max, step_min) and correctly rounded divisions:
//   p < 0 :  drho = max(drho * f, f);      rho = max(rho * drho, rho_min);  rho > rho_max: rho = rho_reset, done = 1
//   p >= 0:  drho = min(drho / f, 1 / f);  rho = max(rho * drho, rho_min)
// A trajectory with done != 0 on entry is frozen: step = STEP_FROZEN and nothing else is written.
template <typename T> struct StepRhoArgsT : StepArgsT<T> {
    T* rho;                              // [batch] in/out
    T* drho;                             // [batch] in/out
    uint8_t* done;                       // [batch] in/out
    T factor, rho_min, rho_max, rho_reset;
};
constexpr int32_t STEP_FROZEN = -2;      // MPCG_STEP_FROZEN

// SA = StepArgsT<T>: mpcg_line_search_step(_f64); SA = StepRhoArgsT<T>: mpcg_line_search_step_rho(_f64) — one selection, one update
template <class SA = StepArgsT<float>>
__global__ __launch_bounds__(256) void line_search_step_kernel(SA a) {
    typedef typename SA::real T;
    constexpr bool RHO = std::is_same<SA, StepRhoArgsT<T>>::value;
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
