// merit_plant_f32.hip.h — the merit function of merit_plant.hip.h in PACKED FLOAT (option "merit_f32" = 1): merit_points_kernel re-derived for the
// arithmetic type kkt_f2, as "kkt_f32" = 1 re-derived round 0 of generate_kkt_kernel.  It is the reference's own arithmetic (include/common/merit.cuh,
// T = float); the float64 kernel stays the default and is not touched by this header (a kernel of its own, not a template over the existing one).
//
// Mapping: a 16-lane group carries TWO work items, a wavefront eight.  Items are consecutive in the flattening (trajectory, step size, knot) of the
// double kernel: half .x of every value is item 2p, half .y item 2p + 1 of the wavefront's trip — a pair may straddle knots, step sizes and
// trajectories, and a half without an item (odd total) recomputes the last item and writes nothing.  Per half the trial iterate is the float
// fmaf(alpha, dz, xu) line_search_step_kernel stores, used as is; sine and cosine in double through kkt_sincos, rounded (as the packed KKT build); the
// model tables are the float ones (PlantDevT<float>) through PlantC<float>.  Lanes 0..6 inertia columns, lane 7 bias, lanes 8..10 pose sweeps through
// rnea<kkt_f2>; lanes 0..6 the Cholesky solve (hardware rsq + two Newton steps) and joint l's share of cost and violation, statement for statement
// what the double kernel does, every multiply-add a v_pk_fma_f32.
// The halves of a lane may differ in `dyn` (a last knot is cost-only), in `moved` and in k == 0: BOTH halves run the whole instruction stream and
// the result is SELECTED per half — no branch on one half, no multiplication by zero.  A cost-only half feeds finite numbers (u = 0, x_next = x, its
// own q and qd) into the shared stream; what it computes there is dropped by the select.  Addresses are selected the same way (a half that is not
// moved reads xu where the other reads dz: a step size of 0 still reads no dz), and every address read lies inside the call's arrays.
// A half's arithmetic depends on nothing but its own item: the bits do not depend on the partner, on the side, on the batch or on the other step sizes.
// Sums: lane 0 adds the seven lane shares in lane order in float (both halves in one packed add), widens, and stores each live half's point merit as
// a double into the SAME scratch [batch][16][N]; merit_sum_kernel adds the row in double and rounds once.  No atomics, no new scratch.
// LDS per wavefront: 4 x 840 B item records + 4 x 11 x 37 x 8 B recursion records = 16,384 B — the double kernel's figure (a float pair is as wide
// as a double; 37 rows of 8 bytes at lane stride: conflict-free, kkt_plant.hip.h), within the packed KKT build's 20,480 B: eight wavefronts per CU.
#pragma once
#include "merit_plant.hip.h"
#pragma clang fp contract(fast)

namespace mpcg {

__device__ __forceinline__ kkt_f2 merit_sel(const bool (&c)[2], kkt_f2 x, kkt_f2 y) { return kkt_f2{c[0] ? x.x : y.x, c[1] ? x.y : y.y}; }

// MeritArgsT<float, float>: the float model tables and float scalars; `point` is the double kernel's scratch.  COST = 1 (mpcg_compute_merit_xuref with "merit_f32"):
// the generalised cost of MeritXuArgsT, each half against its own knot's plan row.
template <int INTEGRATOR = 0, int COST = 0>
__global__ __launch_bounds__(KKT_THREADS, 2) void merit_points_f32_kernel(typename MeritArgsSel<COST, float, float>::type a) {
    typedef kkt_f2 R;
    typedef KktR<R> T;
    typedef KktLds<R>::vr kkt_lds_vd;
    typedef KktLds<R>::item kkt_lds_item;
    typedef PlantC<float>::creal creal;
    constexpr int n = 2 * PJ, m = PJ, KP = 2, PER_TRIP = KKT_ITEMS * KP;
    __shared__ KktItemLds<R> sI[KKT_ITEMS];
    __shared__ R sF[KKT_ITEMS][KKT_R0 * RN_ROWS];
    static_assert(sizeof(KktItemLds<R>) * KKT_ITEMS + sizeof(R) * KKT_ITEMS * KKT_R0 * RN_ROWS <= 20480, "the packed KKT build's LDS budget: eight wavefronts per CU");
    auto sp = [](float v) -> R { return R{v, v}; };
    const int lane = threadIdx.x, gi = lane / KKT_GL, l = lane - gi * KKT_GL;
    kkt_lds_item* I = (kkt_lds_item*)&sI[gi];
    kkt_lds_vd* recs = (kkt_lds_vd*)&sF[gi][0];
    auto rec = [&](int j) -> kkt_lds_vd* { return recs + j * RN_ROWS; };
    kkt_lds_vd* fl = rec(l < KKT_R0 ? l : 0);
    const PlantC<float> P{reinterpret_cast<creal*>(reinterpret_cast<unsigned long long>(a.plant))};
    const int N = a.N;
    const long per_traj = (long)a.A * N, total = (long)a.batch * per_traj;
    const size_t xu_len = (size_t)(n + m) * N - m;
    // ONE trip per wavefront (the grid is the number of trips): inside a trip loop the compiler parks the loop-invariant constants of the whole body — the
    // sine / cosine coefficients, the step sizes, the unit vectors of the solve — in ~70 registers across the recursion, which a float pair per value has
    // no room for (28 registers spilled); without the loop they are formed where they are used.  Trips are consecutive in the flattening, as the double
    // kernel's: the eight point merits of a trip are neighbours in the scratch.
    {
        const long grp = blockIdx.x;
        const long base = grp * PER_TRIP + (long)gi * KP;
        bool live[KP], dyn[KP], moved[KP];
        int bb[KP], aa[KP], kk[KP];                         // (all that stays in registers across the recursion: the addresses below are formed where they are used)
        float alpha[KP];
        const float* xu[KP];
        const float* dz[KP];                                // (a half that is not moved: its own xu — read, never used)
        size_t xk[KP];
#pragma unroll
        for (int hf = 0; hf < KP; ++hf) {
            live[hf] = base + hf < total;                    // (a half without an item recomputes the last one and writes nothing)
            if (hf == 0 || !live[hf]) {
                const long item = live[hf] ? base + hf : total - 1;
                bb[hf] = (int)(item / per_traj);
                const int rem = (int)(item - (long)bb[hf] * per_traj);
                aa[hf] = rem / N;
                kk[hf] = rem - aa[hf] * N;
            } else {                                        // the item behind the first half's
                const bool wk = kk[0] + 1 == N, wa = wk && aa[0] + 1 == a.A;
                kk[hf] = wk ? 0 : kk[0] + 1;
                aa[hf] = wa ? 0 : aa[0] + (wk ? 1 : 0);
                bb[hf] = bb[0] + (wa ? 1 : 0);
            }
            dyn[hf] = kk[hf] < N - 1;                        // the last knot has no control and no successor: cost only
            float al = 0.f;
#pragma unroll
            for (int i = 0; i < MERIT_MAX_STEPS; ++i) al = i == aa[hf] ? a.alpha[i] : al;
            alpha[hf] = al;
            moved[hf] = al != 0.f;
            xu[hf] = a.xu + (size_t)bb[hf] * xu_len;
            dz[hf] = moved[hf] ? a.dz + (size_t)bb[hf] * xu_len : xu[hf];
            xk[hf] = (size_t)kk[hf] * (n + m);
        }
        auto trial = [&](int hf, size_t e) -> float {        // one float rounding: the float line_search_step_kernel stores
            const float x = xu[hf][e], t = __fmaf_rn(alpha[hf], dz[hf][e], x);
            return moved[hf] ? t : x;
        };
        [[maybe_unused]] int roff[KP] = {0, 0};             // COST = 1: the plan offsets are asked for here, the rows that depend on them behind the sines and cosines
        if constexpr (COST >= 1) { roff[0] = a.ref.offset(bb[0]); roff[1] = a.ref.offset(bb[1]); }
        if (l < n) I->Xq[l] = T::mk(trial(0, xk[0] + l), trial(1, xk[1] + l));
        if (l < m) {
            float u_[KP], nq_[KP], nqd_[KP], sn_[KP], cs_[KP];
#pragma unroll
            for (int hf = 0; hf < KP; ++hf) {
                // a cost-only half: u = 0, x_next = x (its own q_l, qd_l: inside the trajectory, finite where the item is)
                const float tu = trial(hf, xk[hf] + (dyn[hf] ? n : 0) + l);
                u_[hf] = dyn[hf] ? tu : 0.f;
                nq_[hf] = trial(hf, xk[hf] + (dyn[hf] ? n + m : 0) + l);
                nqd_[hf] = trial(hf, xk[hf] + (dyn[hf] ? n + m : 0) + PJ + l);
                double sn, cs;                               // (in double in every build, rounded)
                kkt_sincos((double)trial(hf, xk[hf] + l), sn, cs);
                sn_[hf] = (float)sn;
                cs_[hf] = (float)cs;
            }
            I->U[l] = T::mk(u_[0], u_[1]);
            I->Qdd[l] = T::mk(nq_[0], nq_[1]);               // x_{k+1} waits in two fields of the item record the merit has no other use for
            I->Gq1[l] = T::mk(nqd_[0], nqd_[1]);
            I->Sc[0][l] = T::mk(sn_[0], sn_[1]);
            I->Sc[1][l] = T::mk(cs_[0], cs_[1]);
        }
        // COST = 1: joint l's entries of each half's plan row, read ONCE per item, here (every lane reads: lanes 7..15 an entry they drop; a cost-only half: a row
        // has its 21 entries, and what it computes from u_ref is dropped by the select)
        [[maybe_unused]] R rq = sp(0.f), rqd = sp(0.f), ru = sp(0.f);
        if constexpr (COST >= 1) {
            const float* ref0 = a.ref.row(bb[0], roff[0], kk[0]) + (l < m ? l : m - 1);
            const float* ref1 = a.ref.row(bb[1], roff[1], kk[1]) + (l < m ? l : m - 1);
            rq = T::mk(ref0[0], ref1[0]); rqd = T::mk(ref0[PJ], ref1[PJ]); ru = T::mk(ref0[n], ref1[n]);
        }
        __syncthreads();
        // ---- round 0 of the packed KKT kernel: lanes 0..6 ID(q, 0, e_l), lane 7 ID(q, qd, 0), lanes 8..10 the pose sweeps — for both halves, whatever they are ----
        if (l < KKT_R0) {
            R a6w[3], a6u[3];
            RneaTask<R> t;
            t.sj = -1; t.pj = -1; t.qdscale = (l == PJ) ? sp(1.f) : sp(0.f); t.knot_qdd = false; t.unit = l < PJ ? l : -1; t.base = l > PJ ? l - PJ - 1 : -1;
            rnea<R>(P, fl, I, t, a6w, a6u);
#pragma unroll
            for (int r = 0; r < 3; ++r) { fl[RN_AW + r] = a6w[r]; fl[RN_AU + r] = a6u[r]; }
        }
        __syncthreads();
        // ---- lanes 0..6: qdd_l = Minv_l . (u - bias) through the Cholesky solve of the symmetrised M, then joint l's share of the point merit ----
        if (l < PJ) {
            R Lm[PJ][PJ], rd[PJ];
#pragma unroll
            for (int i = 0; i < PJ; ++i)
#pragma unroll
                for (int jj = 0; jj <= i; ++jj) {
                    R sv = sp(0.5f) * (rec(jj)[RN_TAU(i)] + rec(i)[RN_TAU(jj)]);
#pragma unroll
                    for (int t = 0; t < jj; ++t) sv -= Lm[i][t] * Lm[jj][t];
                    if (i == jj) {
                        R y = T::rsq(sv);
                        y = __builtin_elementwise_fma(y * sp(0.5f), __builtin_elementwise_fma(-sv * y, y, sp(1.f)), y);
                        y = __builtin_elementwise_fma(y * sp(0.5f), __builtin_elementwise_fma(-sv * y, y, sp(1.f)), y);
                        rd[i] = y;
                        Lm[i][i] = sv * y;
                    }
                    else Lm[i][jj] = sv * rd[jj];
                }
            R y[PJ];
#pragma unroll
            for (int i = 0; i < PJ; ++i) {
                R sv = (i == l) ? sp(1.f) : sp(0.f);
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
            R qdd = sp(0.f);
#pragma unroll
            for (int i = 0; i < PJ; ++i) qdd += y[i] * (I->U[i] - rec(PJ)[RN_TAU(i)]);      // bias_i = tau_i of lane 7
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
            const R q = I->Xq[l], qd = I->Xq[PJ + l], ul = I->U[l], xn_q = I->Qdd[l], xn_qd = I->Gq1[l];
            R pm;
            if constexpr (COST >= 1) { const R dqd = (a.ref.flags & XUREF_QD_RELATIVE) != 0 ? qd - rqd : qd; pm = sp(0.5f * a.qd_cost) * dqd * dqd; }
            else pm = sp(0.5f * a.qd_cost) * qd * qd;
            if (l < 3) {                                     // lanes 0..2: one coordinate of the tracking error each
                if constexpr (COST >= 1) {
                    if (a.eePos_traj) {                      // (NULL with ee_cost = 0: no goal is read)
                        const R goal = T::mk(a.eePos_traj[((size_t)bb[0] * N + kk[0]) * 6 + l], a.eePos_traj[((size_t)bb[1] * N + kk[1]) * 6 + l]);
                        const R d = (l == 0 ? ee0 : (l == 1 ? ee1 : ee2)) - goal;
                        pm += sp(0.5f * a.ref.ee_cost) * d * d;
                    }
                } else {
                const R goal = T::mk(a.eePos_traj[((size_t)bb[0] * N + kk[0]) * 6 + l], a.eePos_traj[((size_t)bb[1] * N + kk[1]) * 6 + l]);
                const R d = (l == 0 ? ee0 : (l == 1 ? ee1 : ee2)) - goal;
                pm += sp(0.5f) * d * d;
                }
            }
            // the dynamics half's control cost and integrator defect: computed for both halves, kept where the half is a dynamics item
            R pm_dyn;
            if constexpr (COST >= 1) { const R du = (a.ref.flags & XUREF_U_RELATIVE) != 0 ? ul - ru : ul; pm_dyn = pm + sp(0.5f * a.r_cost) * du * du; }
            else pm_dyn = pm + sp(0.5f * a.r_cost) * ul * ul;
            R viol_dyn;
            if constexpr (INTEGRATOR == 1) {                 // semi-implicit Euler: q' = q + dt qd', qd' = qd + dt qdd
                const R qdn = qd + sp(a.dt) * qdd;
                viol_dyn = __builtin_elementwise_abs(xn_q - (q + sp(a.dt) * qdn)) + __builtin_elementwise_abs(xn_qd - qdn);
            } else
            viol_dyn = __builtin_elementwise_abs(xn_q - (q + sp(a.dt) * qd)) + __builtin_elementwise_abs(xn_qd - (qd + sp(a.dt) * qdd));
            pm = merit_sel(dyn, pm_dyn, pm);
            R viol = merit_sel(dyn, viol_dyn, sp(0.f));
            // the initial-state term, likewise (a half that has none reads its trajectory's x_s all the same; no x_s at all: x_0 of the first trajectory — finite or not, dropped)
            const bool first[KP] = {kk[0] == 0 && a.xs != nullptr, kk[1] == 0 && a.xs != nullptr};
            const float* xs0 = a.xs ? a.xs + (size_t)bb[0] * n : a.xu;
            const float* xs1 = a.xs ? a.xs + (size_t)bb[1] * n : a.xu;
            const R xs_q = T::mk(xs0[l], xs1[l]), xs_qd = T::mk(xs0[PJ + l], xs1[PJ + l]);
            const R viol_first = viol + (__builtin_elementwise_abs(q - xs_q) + __builtin_elementwise_abs(qd - xs_qd));
            viol = merit_sel(first, viol_first, viol);
            if constexpr (COST >= 1) { const R dq = q - rq; pm += sp(0.5f * a.ref.q_cost) * dq * dq; }      // the joint-space term: behind the existing ones
            if constexpr (COST == 2) {                       // the limits penalty of joint l: behind that; the control's for both halves, kept where the half is a dynamics item
                const float qlo = P.xlo()[l], qhi = P.xhi()[l], dlo = P.xlo()[PJ + l], dhi = P.xhi()[PJ + l], clo = P.ulo()[l], chi = P.uhi()[l];
                const R vq = T::mk(lim_viol(q.x, qlo, qhi), lim_viol(q.y, qlo, qhi)), vqd = T::mk(lim_viol(qd.x, dlo, dhi), lim_viol(qd.y, dlo, dhi));
                const R vu = T::mk(lim_viol(ul.x, clo, chi), lim_viol(ul.y, clo, chi));
                pm += sp(0.5f * P.limw()[0]) * vq * vq;
                pm += sp(0.5f * P.limw()[1]) * vqd * vqd;
                pm = merit_sel(dyn, pm + sp(0.5f * P.limw()[2]) * vu * vu, pm);
            }
            I->Gq[l] = pm + sp(a.mu) * viol;
        }
        __syncthreads();
        if (l == 0) {                                        // the two items' sums, in lane order, in float; widened on the way out
            R s = I->Gq[0];
#pragma unroll
            for (int i = 1; i < PJ; ++i) s += I->Gq[i];
#pragma unroll
            for (int hf = 0; hf < KP; ++hf)
                if (live[hf]) a.point[((size_t)bb[hf] * MERIT_MAX_STEPS + aa[hf]) * N + kk[hf]] = (double)T::get(s, hf);
        }
    }
}

}  // namespace mpcg
