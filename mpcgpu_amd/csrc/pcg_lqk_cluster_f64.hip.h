// pcg_lqk_cluster_f64.hip.h — the lane-quad-per-knot kernel in double (pcg_lqk_f64.hip.h) for horizons one CU cannot hold: G = ceil(N / 64)
// workgroups on G CUs of one XCD solve ONE trajectory, each with up to 64 consecutive knots of the lower block triangle of S and Pinv in its
// register file.  The double twin of pcg_lpkc_kernel (pcg_lpk_cluster.hip.h), whose decomposition it takes over, on the same cluster runtime
// (pcg_cluster.hip.h):
//   * member g owns knots [k0, k1); LDS knot slot 0 = the replica knot k0 - 1 (its operand entries are rebuilt by the lanes of knot k0), slots
//     1..KL = own knots, slot KL + 1 = the right halo knot k1;
//   * a half-iteration needs from outside T[k0 - 1] (the LEFT member's merged rows of its last knot), Z[k1] (the RIGHT member's z = L_k1^T x_k1
//     of its first knot) and the cluster-wide inner product: ONE hand-off per pass carries them as epoch-tagged 16-byte granules
//     {value lo, value hi, tag, 0} published straight from the registers of the lanes that hold them (z mid-pass), polled by a wavefront of
//     the matrix that sits the pass out; it drops the neighbours' entries into the halo slots, folds the partials, ONE barrier ends the exchange;
//   * members pinned to one XCD (verified at start-up; write-through hand-offs otherwise), persistent clusters drawing trajectories from a
//     queue, bounded spins + completion counts + a fix-up launch that warm-starts from the handle's copy of lambda0.
// N = 128: two CUs per trajectory (the clustered row-per-lane kernel needs four, with twice the hand-off partners).  Reads only the left +
// diagonal block columns: launched when the handle's latch says block-symmetric.
// The recurrence between the passes (run_role) is the single-CU kernels' lxk_role (pcg_lxk_driver.hip.h) with a hand-off where that has a barrier,
// plus the failure exits; it is this kernel's own copy (profiles/lxk_driver_same_code.txt §3: under the driver, same opcode counts, other text).
#pragma once
#include "pcg_lqk_f64.hip.h"
#include "pcg_cluster.hip.h"

namespace mpcg {

// Cells of one member, u64 words: two exchange slots of 64 words — [0, 8) four wave partials, [8, 36) T of the last own knot (14 granules, for
// the right neighbour), [36, 64) Z of the first own knot (for the left one) — then {trajectory, sequence number} (leader) and {XCC id, 1}.
constexpr int LQKC_WG_WORDS = 144;
constexpr int LQKC_SLOT_V = 0, LQKC_SLOT_E = 64, LQKC_W_T = 8, LQKC_W_Z = 36;
constexpr int LQKC_SLOT_T = 128, LQKC_SLOT_X = 130;
constexpr int LQKC_MAX_G = 8;                       // G x 4 wave partials polled by lanes 0..31 of one wavefront

#ifndef LQKC_NPARK
#define LQKC_NPARK 10     // (the hand-off state — epoch, cell addresses, tables — takes the registers the single-CU kernel still had: more of D_k waits in LDS)
#endif
// LDS (doubles): the lane-quad kernel's seven pair-major vectors | broadcast cell (4) | hand-off tables (3 x 64 ints) | parked matrix values
template <int NWR> struct LqkcLds : LqkLds<NWR, LQKC_NPARK> {
    typedef LqkLds<NWR, LQKC_NPARK> B;                 // (its parking rule, parked / pidx, with this kernel's NPARK)
    static constexpr int NW = B::NW, VS = B::VS, NPARK = B::NPARK;
    static constexpr int BC = 7 * VS, TAB = BC + 4, MX = TAB + 3 * 32, TOTAL = MX + NPARK * NW * 64;
    // double index of entry i of knot slot s inside a vector
    __host__ __device__ static constexpr int at(int s, int i) { return 2 * ((i >> 1) * B::KN + s) + (i & 1); }
};
__host__ __device__ constexpr size_t pcg_lqkc_lds_doubles() { return (size_t)LqkcLds<2>::TOTAL; }

template <int NWR>
__global__ __launch_bounds__(NWR * 256, 2) void pcg_lqkc_f64_kernel(ClusterArgs64 ca) {
    typedef LqkcLds<NWR> L;
    typedef double real;
    constexpr int NW = 4 * NWR, NTHR = NW * 64, NWM = NW / 2;
    static_assert(NWM == 4, "the partial cells hold four wavefronts per matrix");
    const PcgArgs64& a = ca.p;
    typedef const __attribute__((address_space(4))) ClusterArgs64* kargp_t;
    const kargp_t kp = (kargp_t)__builtin_amdgcn_kernarg_segment_ptr();
    extern __shared__ __attribute__((aligned(16))) double lds_d[];
    real* lds = lds_d;
    const int N = a.N;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = ca.G;
    const unsigned nclusters = (unsigned)ca.clusters;
    const ClusterPlace pl = cluster_place(G, nclusters);
    if (!pl.member) return;
    const int gm = pl.g, cl = pl.cl;
    const int k0 = cluster_first_knot(gm, N, G), k1 = cluster_first_knot(gm + 1, N, G);
    const int KL = k1 - k0;                             // own knots (launcher: 1 <= KL <= NMAX)
    real* bc = lds + L::BC;                             // [0] / [3] cluster-wide sum of even / odd hand-offs, [1] sticky timeout flag, [2] trajectory index / same-XCD (int)

    const size_t mstride = (size_t)N * ROWF, vstride = (size_t)N * NS;
    gu64* my_words = (gu64*)ca.scratch + ((size_t)cl * G + gm) * LQKC_WG_WORDS;
    gu64* cl_words = (gu64*)ca.scratch + (size_t)cl * G * LQKC_WG_WORDS;

    // ---- role of this wave; knot (i = knot inside the member, slot i + 1), column half and row of this lane (pcg_lqk_f64_kernel's mapping) ----
    const bool isP = w >= NWM;
    const int wl = w - (isP ? NWM : 0);
    const int li = 64 * wl + lane;
    const int i = li >> 2, h = (li >> 1) & 1, g = li & 1;
    const bool p3 = a.pcols == 3;
    const bool hasL = !isP || p3;
    const bool valid = i < KL;
    constexpr int KN = L::KN, K2 = 2 * KN;
    const int b0 = 2 * (i + 1) + g;
    const int bA = b0 + (h ? 4 * K2 : 0);

    real Md[7][7], Ml[7][7];
    real* const park = lds + L::MX + tid;
    bool same_xcd = false;
    unsigned epoch = 0, seq = 0;
    bool failed = false;

    typedef LqkOwn Own;
    typedef LqkFetch Fetch;
    typedef LqkVec Vec;
    auto load_own = [&](int X, int dk) -> Own { return lqk_load_own<K2>(lds, bA, b0, X, dk); };
    auto store_own = [&](int X, const Own& o) {
        if (valid) lqk_store_own<K2>(lds, bA, b0, X, o);      // (slot KL + 1 is the right halo: lanes beyond the member's knots must not write)
    };
    auto fetch = [&](int T, int Z) -> Fetch { return lqk_fetch<K2>(lds, bA, b0, T, Z); };
    // 14 entries of a knot held by its quad -> the 14 granules of the group at word WORD: this lane's v0..v2 are entries 8h + 2s + g, `v3` is
    // entry e3 of the lanes for which pub3 holds (T: own slot 3 = entry 6 + g, lanes h = 0; Z: column 6 = entry 6 + h, lanes g = h)
    auto publish_quad = [&](auto word_tag, auto isz_tag, unsigned ep, real v0, real v1, real v2, real v3) {
        constexpr int WORD = decltype(word_tag)::value;
        constexpr bool ISZ = decltype(isz_tag)::value;
        // (h, g re-read from the hardware lane count: as lane constants living across the pass they were registers this kernel does not have —
        //  spilled, and reloaded from scratch right in front of the hand-off, pcg_lpkc_kernel)
        int ln;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const int hh = (ln >> 1) & 1, gg = ln & 1;
        const int e3 = ISZ ? 6 + hh : 6 + gg;
        const bool pub3 = ISZ ? gg == hh : hh == 0;
        const int h = hh, g = gg;
        const unsigned o0 = 16u * (unsigned)(8 * h + g);
        if (same_xcd) {
            granule_store16<WORD, true>(my_words, o0, granule_of(v0, ep));
            granule_store16<WORD + 4, true>(my_words, o0, granule_of(v1, ep));
            granule_store16<WORD + 8, true>(my_words, o0, granule_of(v2, ep));
            if (pub3) granule_store16<WORD, true>(my_words, 16u * (unsigned)e3, granule_of(v3, ep));
        } else {
            granule_store16<WORD, false>(my_words, o0, granule_of(v0, ep));
            granule_store16<WORD + 4, false>(my_words, o0, granule_of(v1, ep));
            granule_store16<WORD + 8, false>(my_words, o0, granule_of(v2, ep));
            if (pub3) granule_store16<WORD, false>(my_words, 16u * (unsigned)e3, granule_of(v3, ep));
        }
    };

    // One half-iteration of this wave's matrix (lqk_half) + the publishing of what the neighbours and the reduction need.
    auto half = [&](auto mode_tag, auto slot, const Fetch& f, const Vec& old, real c, int TOUT, int ZOUT) -> Vec {
        constexpr int base = decltype(slot)::value;
        const unsigned ep = epoch + 1;                      // tag of the hand-off that follows this pass
        return lqk_half<decltype(mode_tag)::value, L, NTHR>(Md, Ml, park, h, g, hasL, f, old, c,
            [&](const real (&z)[7]) {
                const real zg0 = g ? z[1] : z[0], zg1 = g ? z[3] : z[2], zg2 = g ? z[5] : z[4];     // this lane's columns of parity g
                if (valid) {
                    real* zo = lds + ZOUT;
                    zo[bA] = zg0; zo[bA + K2] = zg1; zo[bA + 2 * K2] = zg2;
                    if (g == h) zo[b0 + 3 * K2] = z[6];
                }
                // z of the first own knot is the LEFT member's missing part: published now, half a pass before the hand-off
                if (valid && i == 0 && gm > 0) publish_quad(std::integral_constant<int, base + LQKC_W_Z>{}, std::true_type{}, ep, zg0, zg1, zg2, z[6]);
            },
            [&](const Own& o) {
                store_own(TOUT, o);
                // the merged rows of the last own knot are the RIGHT member's T[k0 - 1]
                if (valid && i == KL - 1 && gm < G - 1) publish_quad(std::integral_constant<int, base + LQKC_W_T>{}, std::false_type{}, ep, o.v[0], o.v[1], o.v[2], o.v[3]);
            },
            [&](real part) {
                if (lane == 0) {
                    const f4 gr = granule_of(part, ep);
                    if (same_xcd) granule_store16<base, true>(my_words, 16u * (unsigned)wl, gr);
                    else granule_store16<base, false>(my_words, 16u * (unsigned)wl, gr);
                }
            });
    };

    using SlotV = std::integral_constant<int, LQKC_SLOT_V>;
    using SlotE = std::integral_constant<int, LQKC_SLOT_E>;
    // The one hand-off of a half.  `poller`: this wave polls (a wave of the matrix that sits the half out — it starts while the pass still runs).
    // TV / ZV: the local vectors whose halo slots receive the neighbours' T and Z.  withZ: the pass produced z (false: block-Jacobi Pinv pass).
    auto exchange = [&](auto slot, bool poller, int TV, int ZV, bool withZ) -> real {
        constexpr int base = decltype(slot)::value;
        ++epoch;
        if (poller) {
            // lane l < G NWM: wave partial l (member l / NWM, wave l % NWM); lanes 32..45: entry l - 32 of the left member's T; lanes 48..61: entry
            // l - 48 of the right member's Z.  Byte offsets and LDS destinations: three 64-entry tables filled once per launch.
            int ln;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
            const int* tab = reinterpret_cast<const int*>(lds + L::TAB) + ln;
            const unsigned pbyte = (unsigned)tab[0];
            const unsigned vbyte = (unsigned)tab[64];
            const int dst = tab[128];
            const bool isZ = ln >= 48;
            const bool wantp = pbyte != 0xFFFFFFFFu;
            const bool wantv = vbyte != 0xFFFFFFFFu && (withZ || !isZ);
            u4 xp = {0u, 0u, 0u, 0u}, xv = {0u, 0u, 0u, 0u};
            unsigned spins = 0;
            bool ok;
            const unsigned pb_ = wantp ? pbyte : 0u, vb_ = wantv ? vbyte : 0u;
            do {
                asm volatile("s_nop 4\n\t"
                             "global_load_dwordx4 %0, %2, %4 offset:%5 sc1\n\t"
                             "global_load_dwordx4 %1, %3, %4 offset:%5 sc1\n\t"
                             "s_waitcnt vmcnt(0)"
                             : "=&v"(xp), "=&v"(xv) : "v"(pb_), "v"(vb_), "s"(cl_words), "n"(8 * base) : "memory");
                ok = (!wantp || xp.z == epoch) && (!wantv || xv.z == epoch);
                if (__all(ok)) break;
                __builtin_amdgcn_s_sleep(1);
            } while (++spins < CL_SPIN_LIMIT);
            if (wantv) (lds + (isZ ? ZV : TV))[dst] = granule_value(xv);
            const real partial = granule_value(xp);
            const real tot = rpl_wave_fold(wantp ? partial : real(0));
            if (ln == 0) { bc[(epoch & 1u) ? 3 : 0] = tot; if (spins >= CL_SPIN_LIMIT) bc[1] = 1.0; }
        }
        lds_barrier();
        if (bc[1] != 0.0) failed = true;
        // (two cells by epoch parity: the next hand-off's poller — another wavefront of this workgroup — may finish before a wavefront that takes no
        //  part in the next pass has read this value; with one cell that would be a race, however unlikely a wavefront lags a whole pass)
        return bc[(epoch & 1u) ? 3 : 0];
    };

    if (tid == 0) { bc[0] = 0.0; bc[1] = 0.0; bc[2] = 0.0; bc[3] = 0.0; }
    if (tid < 64) {
        const int l = tid;
        int* tab = reinterpret_cast<int*>(lds + L::TAB) + l;
        tab[0] = l < G * NWM ? 8 * ((l / NWM) * LQKC_WG_WORDS + 2 * (l % NWM)) : -1;
        const bool isT = l >= 32 && l < 46, isZ = l >= 48 && l < 62;
        const int e = isT ? l - 32 : l - 48;
        const bool have = isT ? gm > 0 : (isZ && gm < G - 1);
        const int src_m = isT ? gm - 1 : gm + 1;
        tab[64] = have ? 8 * (src_m * LQKC_WG_WORDS + (isT ? LQKC_W_T : LQKC_W_Z) + 2 * e) : -1;
        tab[128] = have ? L::at(isT ? 0 : KL + 1, e) : 0;
    }
    // ---- are all members of this cluster on one XCD? ----
    if (w == 0) {
        const bool all_same = cluster_on_one_xcd<LQKC_SLOT_X, LQKC_WG_WORDS>(my_words, cl_words, lane, G);
        if (lane == 0) reinterpret_cast<int*>(bc + 2)[0] = all_same ? 1 : 0;
    }
    lds_barrier();
    same_xcd = reinterpret_cast<const int*>(bc + 2)[0] != 0 && ca.l2_handoff != 0;
    lds_barrier();
    for (;;) {
        // ---- next trajectory of this cluster: own index first, then the leader draws from the queue ----
        ++seq;
        if (seq > 1) {
            if ((unsigned)ca.batch <= nclusters) break;
            if (w == 0) {
                int bn = 0;
                if (gm == 0) {
                    if (lane == 0) {
                        bn = cluster_hand_out<LQKC_SLOT_T>(kp, my_words, seq, nclusters, same_xcd);
                    }
                } else {
                    const ClusterDraw d = cluster_await_trajectory<LQKC_SLOT_T>(cl_words, seq);
                    bn = d.index;
                    if (d.timed_out && lane == 0) bc[1] = 1.0;
                }
                if (lane == 0) reinterpret_cast<int*>(bc + 2)[0] = bn;
            }
        } else if (tid == 0) {
            reinterpret_cast<int*>(bc + 2)[0] = cl;
        }
        lds_barrier();
        const int b = reinterpret_cast<const int*>(bc + 2)[0];
        if (bc[1] != 0.0 || b >= ca.batch) break;
        const real* gam = kp->p.gamma + (size_t)b * vstride;
        const real* lam_in = kp->p.lambda + (size_t)b * vstride;
        {
            const rsrc_t M = make_rsrc(static_cast<const char*>(static_cast<const void*>(isP ? kp->p.Pinv : kp->p.S)) + (size_t)b * mstride * 8, (uint32_t)(mstride * 8));
            // (lane constants made opaque per trajectory: hoisted out of the trajectory loop, the load addresses are 40 registers this kernel
            //  does not have — spilled once, reloaded between the loads of every trajectory, each reload waiting for all loads in flight)
            int i_st = i, h_st = h, g_st = g;
            asm volatile("" : "+v"(i_st), "+v"(h_st), "+v"(g_st));
            lqk_load_blocks(M, k0 + i_st, h_st, g_st, valid, valid && k0 + i_st > 0 && hasL, Md, Ml);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0)
        lqk_park<L, NTHR>(park, Md);
        // ---- stage: everything <- 0, then P0 <- lambda0, lambda <- lambda0, R0 <- gamma for the own knots AND the replica knot k0 - 1 ----
        for (int e = tid; e < L::BC; e += NTHR) lds[e] = real(0);
        lds_barrier();
        for (int e = tid + (gm == 0 ? NS : 0); e < (KL + 1) * NS; e += NTHR) {
            const int sl = e / NS, ii = e - sl * NS;            // slot 0 = knot k0 - 1
            const int ge = (k0 - 1) * NS + e;
            const real l0 = lam_in[ge];
            lds[L::P0 + L::at(sl, ii)] = l0;
            lds[L::LAM + L::at(sl, ii)] = l0;
            lds[L::R0 + L::at(sl, ii)] = gam[ge];
        }
        lds_barrier();

        uint32_t iters = 0;
        uint32_t max_iter_exit = 1;
        real beta = real(0);
        bool p_pending = true;
        auto run_role = [&](auto role_tag) {
            constexpr bool P = decltype(role_tag)::value;
            const bool poll_s = P && w == NWM, poll_p = !P && w == 0;      // poller of the S half: first Pinv wave; of the Pinv half: wave 0
            Fetch f;
            Vec x;
            x.k = load_own(P ? L::R0 : L::P0, 0);
            x.m = load_own(P ? L::R0 : L::P0, -1);
            // ---- setup: r = gamma - S lambda0 ; r~ = Pinv r ; eta = r . r~   (p = r~ is formed by the first S half: beta = 0) ----
            if constexpr (!P) (void)half(std::integral_constant<int, 0>{}, SlotV{}, f, x, real(0), L::US, L::ZS);
            (void)exchange(SlotV{}, poll_s, L::US, L::ZS, true);
            if constexpr (P) {
                f = fetch(L::US, L::ZS);
                x = half(std::integral_constant<int, 1>{}, SlotE{}, f, x, real(1), L::RT, L::ZP);
            }
            real eta = lqk_uniform(exchange(SlotE{}, poll_p, L::RT, L::ZP, p3));
            if constexpr (!P) f = fetch(L::RT, L::ZP);
            if (failed) { iters = 0xFFFFFFFFu; max_iter_exit = 2; return; }
            // (a setup exit skips the loop, not the store behind it: the Pinv waves hold r_0 = gamma - S lambda0 in x.k, R0 still holds gamma)
            if (fabs(eta) < a.exit_tol) max_iter_exit = 0;
            else for (int it = 0; it < a.max_iter; ++it) {
                real v;
                if constexpr (!P) {
                    x = half(std::integral_constant<int, 2>{}, SlotV{}, f, x, beta, L::US, L::ZS);
                    v = exchange(SlotV{}, false, L::US, L::ZS, true);
                    // alpha ; lambda += alpha p (own entries) — while the Pinv half runs
                    const Own cur = load_own(L::LAM, 0);
                    const real alpha = lqk_uniform(eta / v);
                    Own nw;
#pragma unroll
                    for (int s = 0; s < 4; ++s) nw.v[s] = cur.v[s] + alpha * x.k.v[s];
                    store_own(L::LAM, nw);
                } else {
                    v = exchange(SlotV{}, poll_s, L::US, L::ZS, true);
                    f = fetch(L::US, L::ZS);
                    const real alpha = lqk_uniform(eta / v);
                    x = half(std::integral_constant<int, 1>{}, SlotE{}, f, x, alpha, L::RT, L::ZP);
                }
                const real eta_new = lqk_uniform(exchange(SlotE{}, poll_p, L::RT, L::ZP, p3));
                if constexpr (!P) f = fetch(L::RT, L::ZP);
                if (failed) { iters = 0xFFFFFFFFu; max_iter_exit = 2; break; }
                iters = (uint32_t)(it + 1);
                if (fabs(eta_new) < a.exit_tol) { max_iter_exit = 0; p_pending = false; break; }
                beta = lqk_uniform(eta_new / eta);
                eta = eta_new;
            }
            store_own(P ? L::R0 : L::P0, x.k);
        };
        if (isP) run_role(std::true_type{}); else run_role(std::false_type{});
        lds_barrier();

        // ---- write back own knots (a member that gave up leaves lambda alone: its trajectory's count stays short of G, the fix-up launch re-solves it
        //      from the handle's copy of lambda0) ----
        if (ca.test_fail && cl == 0 && gm == G - 1 && seq == 1) failed = true;
        if (failed) {
            cluster_report_abandoned(kp, b, tid);
            break;
        }
        for (int e = tid; e < KL * NS; e += NTHR) {
            const int sl = e / NS + 1, ii = e % NS;
            const size_t ge = (size_t)b * vstride + (size_t)k0 * NS + e;
            kp->p.lambda[ge] = lds[L::LAM + L::at(sl, ii)];
            if (kp->p.r_out) kp->p.r_out[ge] = lds[L::R0 + L::at(sl, ii)];
            if (kp->p.p_out) {
                real pv = lds[L::P0 + L::at(sl, ii)];
                if (p_pending) pv = (lds[L::RT + L::at(sl, ii)] + (p3 ? lds[L::ZP + L::at(sl + 1, ii)] : real(0))) + beta * pv;
                kp->p.p_out[ge] = pv;
            }
        }
        cluster_finish(kp, b, gm == 0, tid, iters, max_iter_exit);
        lds_barrier();                                      // LDS is restaged for the next trajectory
    }
}

}  // namespace mpcg
