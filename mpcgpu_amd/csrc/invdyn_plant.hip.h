// invdyn_plant.hip.h — batched inverse dynamics of the mpcg_plant for a caller: tau = ID(q, qd, qdd), the plant's gravity (PlantDevT::grav) included, for
// `count` independent states — mpcg_inverse_dynamics (IO = float: float64 inside, rounded once on store) and mpcg_inverse_dynamics_f64 (IO = double: inputs
// used as they are, torques stored as they are).  With qd = qdd = NULL it returns the gravity torques ID(q, 0, 0): what a plan made for zero gravity must
// gain in its controls before a loop over a gravity clone starts from it.
//
// The sweep is rnea<double> of kkt_plant.hip.h with the task of the bias lane plus the knot's qdd (qdscale = 1, knot_qdd): the same instruction text as
// lane 7 of the KKT, merit and simulate kernels, so this entry and their bias agree by construction.
//
// Mapping: a 16-lane group per state, four states per wavefront, ONE working lane per group — the scaffolding of simulate_kernel (an item record per
// group for q, qd, qdd and the sines / cosines, which lanes 0..6 fill and lanes 0..6 read the torques back from) with a single recursion record.  Chosen
// over one state per lane because rnea reads its joint values through the group's item record and is left untouched that way, and because LDS stays at
// 4 x 840 B + 4 x 296 B = 4,544 B per wavefront (a lane per state: 1.1 KB per lane, 71 KB per wavefront).  A sweep is one ninth of a merit point's work
// (one of its eight round-0 sweeps plus no solve); 15 of 16 lanes idle through it, which an entry called once per plan can afford.
// A group without a state recomputes the last one and writes nothing; no atomics; a state's arithmetic depends on nothing but that state.
#pragma once
#include "kkt_plant.hip.h"
#pragma clang fp contract(fast)

namespace mpcg {

template <typename IO> struct InvDynArgsT {
    const PlantDev* plant;
    const IO* q;                         // [count][PJ]
    const IO* qd;                        // [count][PJ] or NULL: 0
    const IO* qdd;                       // [count][PJ] or NULL: 0
    IO* tau;                             // [count][PJ]
    unsigned count;
};

template <typename IO>
__global__ __launch_bounds__(KKT_THREADS) void inverse_dynamics_kernel(InvDynArgsT<IO> a) {
    typedef double R;
    typedef KktLds<R>::vr kkt_lds_vd;
    typedef KktLds<R>::item kkt_lds_item;
    typedef PlantC<R>::creal creal;
    __shared__ KktItemLds<R> sI[KKT_ITEMS];
    __shared__ R sF[KKT_ITEMS][RN_ROWS];                     // one recursion record per group
    const int lane = threadIdx.x, gi = lane / KKT_GL, l = lane - gi * KKT_GL;
    kkt_lds_item* I = (kkt_lds_item*)&sI[gi];
    kkt_lds_vd* fl = (kkt_lds_vd*)&sF[gi][0];
    const PlantC<R> P{reinterpret_cast<creal*>(reinterpret_cast<unsigned long long>(a.plant))};
    const size_t s0 = (size_t)blockIdx.x * KKT_ITEMS + gi;
    const bool live = s0 < a.count;
    const size_t s = live ? s0 : (size_t)a.count - 1;
    if (l < PJ) {
        const double q = (double)a.q[s * PJ + l];
        I->Xq[l] = q;
        I->Xq[PJ + l] = a.qd ? (double)a.qd[s * PJ + l] : 0.0;
        I->Qdd[l] = a.qdd ? (double)a.qdd[s * PJ + l] : 0.0;
        double sn, cs;
        kkt_sincos(q, sn, cs);
        I->Sc[0][l] = sn;
        I->Sc[1][l] = cs;
    }
    __syncthreads();
    if (l == 0) {
        R a6w[3], a6u[3];
        RneaTask<R> t;
        t.sj = -1; t.pj = -1; t.qdscale = 1.0; t.knot_qdd = true; t.unit = -1; t.base = -1;
        rnea<R>(P, fl, I, t, a6w, a6u);
    }
    __syncthreads();
    if (live && l < PJ) a.tau[s * PJ + l] = (IO)fl[RN_TAU(l)];
}

}  // namespace mpcg
