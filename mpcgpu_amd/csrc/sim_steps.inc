// sim_steps.inc — the body of simulate_kernel (IO = float) and of simulate_f64_kernel (IO = double), included INSIDE each kernel (sim_plant.hip.h)
// with IO, INTEGRATOR (0 explicit, 1 semi-implicit Euler: "sim_integrator") and the argument struct `a` in scope.  One text for both, as kkt_knots.inc and merit_points.inc: only the loads (widened, or used as they
// are) and the stores (rounded once, or not at all) depend on IO.
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
    unsigned idx = knot_of(a.toff);
    const unsigned steps = a.S + (a.rem != 0.0 ? 1u : 0u), rounds = steps + (a.eePos ? 1u : 0u);
    for (unsigned k = 0; k < rounds; ++k) {
        const bool step = k < steps;                         // the last round of a call with an end-effector output: the pose sweeps on the final state
        double dt = a.rem;
        if (k < a.S) { idx = knot_of(__dadd_rn(a.toff, __dmul_rn((double)k, a.ss))); dt = a.ss; }
        if (l < m) {
            if (step) I->U[l] = (double)xu[(size_t)idx * (n + m) + n + l];
            double sn, cs;
            kkt_sincos(I->Xq[l], sn, cs);
            I->Sc[0][l] = sn;
            I->Sc[1][l] = cs;
        }
        __syncthreads();
        // ---- round 0 of the KKT kernel: lanes 0..6 ID(q, 0, e_l), lane 7 ID(q, qd, 0); in the pose round lanes 8..10 instead ----
        if (l < KKT_R0 && (step ? l <= PJ : l > PJ)) {
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
    if (a.eePos && live && l < 3) {
        R ee0, ee1, ee2;
        plant_ee_pos(recs, ee0, ee1, ee2);
        a.eePos[b * 3 + l] = (IO)(l == 0 ? ee0 : (l == 1 ? ee1 : ee2));
    }
    if (live && l < n) xs[l] = (IO)I->Xq[l];                // IO = float: the one rounding of the call; IO = double: the state as it is
