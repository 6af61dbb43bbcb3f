// kkt_knots.inc — the body of generate_kkt_kernel<ANALYTIC, R, INTEGRATOR> (IO = float: float arrays) and of generate_kkt_f64_kernel<ANALYTIC, INTEGRATOR> (R = IO = double: double
// arrays), included INSIDE each kernel (kkt_plant.hip.h) with ANALYTIC, R, IO, INTEGRATOR (0 explicit, 1 semi-implicit Euler: `if constexpr` only) and the argument struct `a` in scope.  One text for both: a shared
// __device__ function in its place changed the code of the float kernels.  Only the loads and the output staging depend on IO.
    typedef KktR<R> T;
    typedef typename T::scalar S;
    constexpr int KP = T::KP;
    static_assert(ANALYTIC || T::is_double, "the difference quotients need float64");
    static_assert(sizeof(IO) == 4 || (T::is_double && KP == 1), "double arrays: the float64 build only");
    typedef typename KktLds<R>::vr kkt_lds_vd;
    typedef typename KktLds<R>::item kkt_lds_item;
    typedef typename PlantC<S>::creal creal;
    constexpr int n = 2 * PJ, m = PJ, nn = n * n, mm = m * m, nm = n * m;
    __shared__ KktItemLds<R> sI[KKT_ITEMS];
    constexpr int RL = kkt_rec_lanes(ANALYTIC);             // round-0 records per group: 11 (analytic: 13.0 KB per wavefront in double) or 14 (16.6 KB)
    constexpr int RE = kkt_rec_elems<R>(ANALYTIC);          // elements of a group's record region (float: the staging area decides, 14.4 KB per wavefront; packed: 20.6 KB)
    __shared__ R sF[KKT_ITEMS][RE];                         // the recursion records
    static_assert(sizeof(KktItemLds<R>) * KKT_ITEMS + sizeof(R) * KKT_ITEMS * RE <= (ANALYTIC && KP == 1 ? 16384 : 20480), "ten / eight wavefronts per CU");
    // The model tables are read with RUNTIME joint indices.  With compile-time indices (unrolled sweeps) all table entries are
    // loop-invariant loads that the compiler hoists into registers: 512 VGPR + AGPR and scratch.
    const int lane = threadIdx.x, gi = lane / KKT_GL, l = lane - gi * KKT_GL;
    kkt_lds_item* I = (kkt_lds_item*)&sI[gi];
    kkt_lds_vd* recs = (kkt_lds_vd*)&sF[gi][0];
    auto rec = [&](int j) -> kkt_lds_vd* { return recs + j * RN_ROWS; };                // record of lane j of this group
    kkt_lds_vd* fl = rec(l < RL ? l : 0);                    // (lanes beyond the records never touch theirs)
    kkt_lds_f* st = (kkt_lds_f*)&sF[gi][0];                  // (float arrays only)
    const PlantC<S> P{reinterpret_cast<creal*>(reinterpret_cast<unsigned long long>(a.plant))};
    const int N = a.N;
    const long total = (long)a.batch * (N - 1);
    // A wavefront's trips cover CONSECUTIVE groups of four (packed: eight) knots (not a grid stride): the knots' pieces of g (84 B), c (56 B), G (980 B) and
    // C (1176 B) are then neighbours in memory and most 128-byte lines are completed inside one L2 instead of leaving two XCDs as partial writes.
    constexpr int PER_TRIP = KKT_ITEMS * KP;
    const long groups = (total + PER_TRIP - 1) / PER_TRIP, per = (groups + gridDim.x - 1) / gridDim.x;
    const long g_begin = (long)blockIdx.x * per, g_end = g_begin + per < groups ? g_begin + per : groups;
    for (long grp = g_begin; grp < g_end; ++grp) {
        const long base = grp * PER_TRIP + (long)gi * KP;
        bool live[KP];                                      // (a half without a knot recomputes the last one and writes nothing)
        int bb[KP], kk[KP];
        const IO* xu[KP];
#pragma unroll
        for (int hf = 0; hf < KP; ++hf) {
            live[hf] = base + hf < total;
            const long item = live[hf] ? base + hf : total - 1;
            if (hf == 0 || !live[hf]) {
                bb[hf] = (int)(item / (N - 1));              // (a 32-bit division where the knot count allows, behind a wave-uniform test, measured SLOWER: 0.336 against 0.330 ms in double)
                kk[hf] = (int)(item - (long)bb[hf] * (N - 1));
            } else {                                        // the knot behind the first half's
                const bool wrap = kk[0] + 1 == N - 1;
                bb[hf] = bb[0] + (wrap ? 1 : 0);
                kk[hf] = wrap ? 0 : kk[0] + 1;
            }
            xu[hf] = a.xu + (size_t)bb[hf] * ((size_t)(n + m) * N - m) + (size_t)kk[hf] * (n + m);      // x_k, u_k, x_{k+1}
        }
        if (l < n) I->Xq[l] = T::mk((S)xu[0][l], (S)xu[KP - 1][l]);
        if (l < m) {
            I->U[l] = T::mk((S)xu[0][n + l], (S)xu[KP - 1][n + l]);
            double sn_[KP], cs_[KP];                          // (seven sine / cosine pairs per knot: in double in every build, rounded to R)
#pragma unroll
            for (int hf = 0; hf < KP; ++hf) {
                if (KKT_ABLATE & 4) { sn_[hf] = (double)xu[hf][l]; cs_[hf] = 1.0 - sn_[hf]; } else
                kkt_sincos((double)xu[hf][l], sn_[hf], cs_[hf]);
            }
            I->Sc[0][l] = T::mk((S)sn_[0], (S)sn_[KP - 1]);
            I->Sc[1][l] = T::mk((S)cs_[0], (S)cs_[KP - 1]);
        }
        __syncthreads();
        // ---- round 0: lanes 0..6 inertia-matrix columns ID(q, 0, e_l), lane 7 bias ID(q, qd, 0), lanes 8..10 the pose sweeps ----
        R a6w[3], a6u[3];
        if (l < PJ + 4) {
            RneaTask<R> t;
            t.sj = -1; t.pj = -1; t.qdscale = (l == PJ) ? KR(1.0) : KR(0.0); t.knot_qdd = false; t.unit = l < PJ ? l : -1; t.base = l > PJ ? l - PJ - 1 : -1;
            if (!(KKT_ABLATE & 16)) rnea(P, fl, I, t, a6w, a6u);
#pragma unroll
            for (int r = 0; r < 3; ++r) { fl[RN_AW + r] = a6w[r]; fl[RN_AU + r] = a6u[r]; }
        }
        __syncthreads();
        // ---- Minv (column l through a Cholesky solve of the symmetrised M), qdd_l = Minv_l . (u - bias)  (Minv is symmetric: row l = column l),
        //      end-effector position, Jacobian column l, cost gradient entries ----
        if (l < PJ && !(KKT_ABLATE & 2)) {
            R Lm[PJ][PJ], rd[PJ];
#pragma unroll
            for (int i = 0; i < PJ; ++i)
#pragma unroll
                for (int jj = 0; jj <= i; ++jj) {
                    R sv = KR(0.5) * (rec(jj)[RN_TAU(i)] + rec(i)[RN_TAU(jj)]);      // M[i][jj] = tau_i of lane jj
#pragma unroll
                    for (int t = 0; t < jj; ++t) sv -= Lm[i][t] * Lm[jj][t];
                    if (i == jj) {
                        // 1 / sqrt(pivot) from the hardware estimate + two Newton steps (full double precision for these O(1) pivots): the
                        // correctly rounded sqrt and division of the textbook form are ~30 instructions per pivot
                        R y = T::rsq(sv);
                        y = __builtin_elementwise_fma(y * KR(0.5), __builtin_elementwise_fma(-sv * y, y, KR(1.0)), y);
                        if constexpr (T::is_double) y = __builtin_elementwise_fma(y * KR(0.5), __builtin_elementwise_fma(-sv * y, y, KR(1.0)), y);      // (float: 1 ulp estimate + one Newton step)
                        rd[i] = y;
                        Lm[i][i] = sv * y;
                    }
                    else Lm[i][jj] = sv * rd[jj];
                }
            R y[PJ];
#pragma unroll
            for (int i = 0; i < PJ; ++i) {
                R sv = (i == l) ? KR(1.0) : KR(0.0);
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
            R qdd = KR(0.0);
#pragma unroll
            for (int i = 0; i < PJ; ++i) {
                I->Minv[i][l] = y[i];
                qdd += y[i] * (I->U[i] - rec(PJ)[RN_TAU(i)]);          // bias_i = tau_i of lane 7
            }
            I->Qdd[l] = qdd;
            // pose of the last link from the three base-acceleration sweeps (lanes 8..10): their final acceleration is [W_i ; V_i] =
            // [R e_i ; R (e_i x p)], R = rotation world -> link.  Row i of R^T is W_i, so R^T x = (W_0.x, W_1.x, W_2.x);
            // e_x x p = (0, -pz, py), e_y x p = (pz, 0, -px).
            R W[3][3], V0[3], V1[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int r = 0; r < 3; ++r) W[i][r] = rec(PJ + 1 + i)[RN_AW + r];
#pragma unroll
            for (int r = 0; r < 3; ++r) { V0[r] = rec(PJ + 1)[RN_AU + r]; V1[r] = rec(PJ + 2)[RN_AU + r]; }
            R ee[3], J[3];
            ee[0] = -(W[2][0] * V1[0] + W[2][1] * V1[1] + W[2][2] * V1[2]);
            ee[1] = W[2][0] * V0[0] + W[2][1] * V0[1] + W[2][2] * V0[2];
            ee[2] = -(W[1][0] * V0[0] + W[1][1] * V0[1] + W[1][2] * V0[2]);
            // Jacobian column l = R^T (linear velocity of the last link's origin for qd = e_l) = R^T au of this lane's own sweep
#pragma unroll
            for (int r = 0; r < 3; ++r) J[r] = W[r][0] * a6u[0] + W[r][1] * a6u[1] + W[r][2] * a6u[2];
            const IO* goal[KP];
#pragma unroll
            for (int hf = 0; hf < KP; ++hf) goal[hf] = a.eePos_traj + ((size_t)bb[hf] * N + kk[hf]) * 6;
            R s0 = KR(0.0), s1 = KR(0.0);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                s0 += J[r] * (ee[r] - T::mk((S)goal[0][r], (S)goal[KP - 1][r]));
                s1 += J[r] * (ee[r] - T::mk((S)goal[0][6 + r], (S)goal[KP - 1][6 + r]));       // goal of knot k+1: used by the last block only
            }
            I->Gq[l] = s0;
            I->Gq1[l] = s1;
        }
        __syncthreads();
        // ---- round 1: lanes 0..6 ID(q + h e_l, qd, qdd), 7..13 ID(q, qd + h e_(l-7), qdd); each lane then owns column l of
        //      [dqdd/dq, dqdd/dqd] = -Minv (ID(. + h e) - u) / h  and writes column l of A and Q (lanes 0..6: of B and R too) ----
        // analytic gradient (default): 15 lanes — 14 columns + the nominal recursion in lane 14; records re-used as 15 x RN_ROWS floats (packed: float pairs)
        typename KktRecLds<R>::vf* flf = (typename KktRecLds<R>::vf*)recs + (l <= KKT_NOM ? KktGrad<R>::rec(l) : 0) * RN_ROWS;
        if (ANALYTIC && l <= KKT_NOM && !(KKT_ABLATE & 1)) rnea_grad<R>(P, flf, I, l);
        R colv[PJ];
        if (l < n) {
            R d[PJ];
            if constexpr (ANALYTIC) {
#pragma unroll
                for (int i = 0; i < PJ; ++i) d[i] = -T::from_rec(flf[KktGrad<R>::tau(l, i)]);
            } else {
                RneaTask<R> t;
                t.sj = l < PJ ? l : -1; t.pj = l < PJ ? -1 : l - PJ; t.qdscale = KR(1.0); t.knot_qdd = true; t.unit = -1; t.base = -1;
                if (!(KKT_ABLATE & 1)) rnea(P, fl, I, t, a6w, a6u);
#pragma unroll
                for (int i = 0; i < PJ; ++i) d[i] = (fl[RN_TAU(i)] - I->U[i]) * (-KR(1.0) / KR(KKT_FD_H));
            }
            asm volatile("" ::: "memory");                // (the float staging stores below reuse the records: keep them behind these loads)
#pragma unroll
            for (int i = 0; i < PJ; ++i) {
                R sv = KR(0.0);
#pragma unroll
                for (int tt = 0; tt < PJ; ++tt) sv += I->Minv[i][tt] * d[tt];
                colv[i] = sv;
            }
        }
        // The knot's outputs are STAGED in the group's (now free) records as float, in the order they have in memory, and
        // copied out by all 16 lanes in 64-byte runs below.  Written straight from here — a lane per column, 14 lanes 56 bytes
        // apart per store — the ~60 stores per lane were a fifth of the kernel's time (one cache line per lane and store).
        // Packed build: one knot of the pair at a time through the same staging area.
        if constexpr (sizeof(IO) == 4) {
#pragma unroll
        for (int hf = 0; hf < KP; ++hf) {
            const int k = kk[hf], b = bb[hf];
            if (l < n && !(KKT_ABLATE & 8)) {
                const S dt = a.dt;
                const S gql = l < PJ ? T::get(I->Gq[l], hf) : S(0.0), gq1l = l < PJ ? T::get(I->Gq1[l], hf) : S(0.0);
                // column l (column-major):  A = I + dt [[0, I], [dqdd/dq, dqdd/dqd]] (semi-implicit: [[dt dqdd/dq, I + dt dqdd/dqd], [dqdd/dq, dqdd/dqd]]),  Q = blkdiag(g g^T, QD I)
#pragma unroll
                for (int r = 0; r < n; ++r) {
                    S av = (r == l) ? S(1.0) : S(0.0);
                    if (r < PJ) {
                        av += (l == r + PJ) ? dt : S(0.0);
                        if constexpr (INTEGRATOR == 1) av += dt * (dt * T::get(colv[r], hf));      // semi-implicit: q' = q + dt qd', the upper half gains dt x the lower half's
                    }
                    else av += dt * T::get(colv[r - PJ], hf);
                    st[ST_C + l * n + r] = (float)(-av);
                    S qv, q1;
                    if (r < PJ) { qv = T::get(I->Gq[r], hf) * gql; q1 = T::get(I->Gq1[r], hf) * gq1l; }
                    else qv = q1 = (r == l) ? a.qd_cost : S(0.0);
                    st[ST_G + l * n + r] = (float)qv;
                    st[ST_Q1 + l * n + r] = (float)q1;
                }
                if (l < m) {
#pragma unroll
                    for (int r = 0; r < n; ++r) {
                        if constexpr (INTEGRATOR == 1) st[ST_C + nn + l * n + r] = (float)(-(r < PJ ? dt * (dt * T::get(I->Minv[r][l], hf)) : dt * T::get(I->Minv[r - PJ][l], hf)));      // B = [dt^2 Minv; dt Minv]
                        else st[ST_C + nn + l * n + r] = (float)(-(r < PJ ? S(0.0) : dt * T::get(I->Minv[r - PJ][l], hf)));      // B = dt [0; Minv]
                    }
#pragma unroll
                    for (int r = 0; r < m; ++r) st[ST_G + nn + l * m + r] = (float)(r == l ? a.r_cost : S(0.0));
                    st[ST_g + n + l] = (float)(a.r_cost * T::get(I->U[l], hf));
                }
                const S qdl = T::get(I->Xq[l < PJ ? l + PJ : l], hf);              // qd_{l mod 7}
                st[ST_g + l] = (float)(l < PJ ? gql : a.qd_cost * qdl);
                st[ST_g1 + l] = (float)(l < PJ ? gq1l : a.qd_cost * qdl);  // last block only (evaluated at x_{N-2}: iiwa_eepos_plant.cuh:407)
                // integrator defect c_{k+1} = x_{k+1} - (x_k + dt [qd; qdd]) (semi-implicit: x_{k+1} - [q + dt qd'; qd'], qd' = qd + dt qdd);  c_0 = x_0 - x_s
                S pred;
                if constexpr (INTEGRATOR == 1) {
                    const S qdn = qdl + dt * T::get(I->Qdd[l < PJ ? l : l - PJ], hf);
                    pred = l < PJ ? T::get(I->Xq[l], hf) + dt * qdn : qdn;
                } else pred = l < PJ ? T::get(I->Xq[l], hf) + dt * qdl : qdl + dt * T::get(I->Qdd[l - PJ], hf);
                st[ST_c1 + l] = (float)((S)xu[hf][(n + m) + l] - pred);
                if (k == 0) st[ST_c0 + l] = (float)((S)xu[hf][l] - (S)a.xs[(size_t)b * n + l]);
            }
            __syncthreads();
            if (live[hf] && !(KKT_ABLATE & 8)) {
                IO* G = a.G + (size_t)b * ((size_t)(nn + mm) * N - mm) + (size_t)(nn + mm) * k;
                IO* Cm = a.C + (size_t)b * (size_t)(nn + nm) * (N - 1) + (size_t)(nn + nm) * k;
                IO* g = a.g + (size_t)b * ((size_t)(n + m) * N - m) + (size_t)(n + m) * k;
                IO* c = a.c + (size_t)b * (size_t)n * N + (size_t)n * (k + 1);
                kkt_copy_out<nn + mm>(G, st + ST_G, l);
                kkt_copy_out<nn + nm>(Cm, st + ST_C, l);
                kkt_copy_out<n + m>(g, st + ST_g, l);
                kkt_copy_out<n>(c, st + ST_c1, l);
                if (k == N - 2) {                                 // the last block: Q_{N-1}, q_{N-1} follow R_{N-2}, r_{N-2} in memory
                    kkt_copy_out<nn>(G + nn + mm, st + ST_Q1, l);
                    kkt_copy_out<n>(g + n + m, st + ST_g1, l);
                }
                if (k == 0) kkt_copy_out<n>(c - n, st + ST_c0, l);
            }
            __syncthreads();
        }
        } else {
            // Double arrays: the same values, not rounded, through the same region in three pieces (SD_*; [-A -B] first: it is the only one that reads colv).
            // What a later piece needs is in the item record and in registers; a piece is copied out by all 16 lanes in 128-byte runs.
            kkt_lds_d* sd = (kkt_lds_d*)&sF[gi][0];
            const int k = kk[0], b = bb[0];
            const bool on = !(KKT_ABLATE & 8), lastblk = k == N - 2;
            const S dt = a.dt;
            const S gql = l < PJ ? I->Gq[l] : S(0.0), gq1l = l < PJ ? I->Gq1[l] : S(0.0);
            IO* G = a.G + (size_t)b * ((size_t)(nn + mm) * N - mm) + (size_t)(nn + mm) * k;
            IO* Cm = a.C + (size_t)b * (size_t)(nn + nm) * (N - 1) + (size_t)(nn + nm) * k;
            IO* g = a.g + (size_t)b * ((size_t)(n + m) * N - m) + (size_t)(n + m) * k;
            IO* c = a.c + (size_t)b * (size_t)n * N + (size_t)n * (k + 1);
            if (l < n && on) {
#pragma unroll
                for (int r = 0; r < n; ++r) {
                    S av = (r == l) ? S(1.0) : S(0.0);
                    if (r < PJ) {
                        av += (l == r + PJ) ? dt : S(0.0);
                        if constexpr (INTEGRATOR == 1) av += dt * (dt * colv[r]);
                    }
                    else av += dt * colv[r - PJ];
                    sd[l * n + r] = -av;
                }
                if (l < m) {
#pragma unroll
                    for (int r = 0; r < n; ++r) {
                        if constexpr (INTEGRATOR == 1) sd[nn + l * n + r] = -(r < PJ ? dt * (dt * I->Minv[r][l]) : dt * I->Minv[r - PJ][l]);
                        else sd[nn + l * n + r] = -(r < PJ ? S(0.0) : dt * I->Minv[r - PJ][l]);
                    }
                }
            }
            __syncthreads();
            if (live[0] && on) kkt_copy_out<nn + nm>(Cm, sd, l);
            __syncthreads();
            if (l < n && on) {
#pragma unroll
                for (int r = 0; r < n; ++r) sd[SD_G + l * n + r] = r < PJ ? I->Gq[r] * gql : ((r == l) ? a.qd_cost : S(0.0));
                if (l < m) {
#pragma unroll
                    for (int r = 0; r < m; ++r) sd[SD_G + nn + l * m + r] = r == l ? a.r_cost : S(0.0);
                    sd[SD_g + n + l] = a.r_cost * I->U[l];
                }
                const S qdl = I->Xq[l < PJ ? l + PJ : l];
                sd[SD_g + l] = l < PJ ? gql : a.qd_cost * qdl;
                sd[SD_g1 + l] = l < PJ ? gq1l : a.qd_cost * qdl;
                S pred;
                if constexpr (INTEGRATOR == 1) {
                    const S qdn = qdl + dt * I->Qdd[l < PJ ? l : l - PJ];
                    pred = l < PJ ? I->Xq[l] + dt * qdn : qdn;
                } else pred = l < PJ ? I->Xq[l] + dt * qdl : qdl + dt * I->Qdd[l - PJ];
                sd[SD_c1 + l] = xu[0][(n + m) + l] - pred;
                if (k == 0) sd[SD_c0 + l] = xu[0][l] - a.xs[(size_t)b * n + l];
            }
            __syncthreads();
            if (live[0] && on) {
                kkt_copy_out<nn + mm>(G, sd + SD_G, l);
                kkt_copy_out<n + m>(g, sd + SD_g, l);
                kkt_copy_out<n>(c, sd + SD_c1, l);
                if (lastblk) kkt_copy_out<n>(g + n + m, sd + SD_g1, l);
                if (k == 0) kkt_copy_out<n>(c - n, sd + SD_c0, l);
            }
            __syncthreads();
            // the last block's Q_{N-1} (evaluated at x_{N-2}); the barriers are taken by every group of the wavefront, whichever knot it holds
            if (l < n && on && lastblk) {
#pragma unroll
                for (int r = 0; r < n; ++r) sd[l * n + r] = r < PJ ? I->Gq1[r] * gq1l : ((r == l) ? a.qd_cost : S(0.0));
            }
            __syncthreads();
            if (live[0] && on && lastblk) kkt_copy_out<nn>(G + nn + mm, sd, l);
            __syncthreads();
        }
    }
