// merit_points.inc — the body of merit_points_kernel (IO = float) and of merit_points_f64_kernel (IO = double), included INSIDE each kernel
// (merit_plant.hip.h) with IO, INTEGRATOR (0 explicit, 1 semi-implicit Euler) and the argument struct `a` in scope.  One text for both: a shared __device__ function in its place changed the code of
// the float kernel.  Only the loads and the trial iterate depend on IO.
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
        if (l < n) I->Xq[l] = trial(xk + l);
        if (l < m) {
            if (dyn) { ul = trial(xk + n + l); xn_q = trial(xk + (n + m) + l); xn_qd = trial(xk + (n + m) + PJ + l); }
            I->U[l] = ul;
            double sn, cs;
            kkt_sincos(trial(xk + l), sn, cs);
            I->Sc[0][l] = sn;
            I->Sc[1][l] = cs;
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
            R pm = 0.5 * a.qd_cost * qd * qd;
            if (l < 3) {                                     // lanes 0..2: one coordinate of the tracking error each
                const IO* goal = a.eePos_traj + ((size_t)b * N + k) * 6;
                const R d = (l == 0 ? ee0 : (l == 1 ? ee1 : ee2)) - (R)goal[l];
                pm += 0.5 * d * d;
            }
            R viol = 0.0;
            if (dyn) {
                pm += 0.5 * a.r_cost * ul * ul;
                if constexpr (INTEGRATOR == 1) {                  // semi-implicit Euler: q' = q + dt qd', qd' = qd + dt qdd (the map the KKT kernel linearised)
                    const R qdn = qd + a.dt * qdd;
                    viol = fabs(xn_q - (q + a.dt * qdn)) + fabs(xn_qd - qdn);
                } else
                viol = fabs(xn_q - (q + a.dt * qd)) + fabs(xn_qd - (qd + a.dt * qdd));
            }
            if (k == 0 && a.xs) viol += fabs(q - (R)a.xs[(size_t)b * n + l]) + fabs(qd - (R)a.xs[(size_t)b * n + PJ + l]);
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
