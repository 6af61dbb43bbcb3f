// block_solve_f64.hip.h — the block-tridiagonal DIRECT solve of block_solve.hip.h with the sweep in DOUBLE (linsys_t = double, USE_DOUBLES = 1 of
// include/common/settings.cuh:41-49; and "float64 inside, float outputs" for float callers).  State size 14, gfx950.
//
// Same recurrence, same operation order, contraction off (the bits of the C oracle's double instantiation of the sweep):
//   Delta_0 = D_0, y_0 = gamma_0;  k >= 1:  Delta_k = D_k - L_k W_{k-1},  y_k = gamma_k - L_k z_{k-1};
//   [Delta_k | U_k y_k] -> [I | W_k z_k] by one pivot-free Gauss-Jordan elimination;  lambda_{N-1} = z_{N-1},  lambda_k = z_k - W_k lambda_{k+1}
// in the layout of bt_block_solve_wide_kernel: ONE trajectory per wavefront, the 29 columns of [Delta | U y] dealt round-robin to the four
// 16-lane DPP rows (lane = 16 g + r holds row r of columns c = 4 j + g, j = 0..3, of Delta and of U; g = 3 also carries y / z), the pivot column
// moved from its owner row to the other three by ds_bpermute (two 32-bit halves), the next knot's operands requested before the current
// elimination.  The live set is ~45 doubles per lane (D, U, W: 4 each, L: 14, the prefetch: 23 in the storage type), which fits the register
// file with no scratch; the four-trajectories-per-wavefront layout of bt_block_solve_kernel would hold ~100 doubles per lane (200 VGPRs before
// temporaries) and is NOT built: this layout serves every batch, "block_solve_wide" is not read.
//
// 64-bit operands are broadcast inside a row by v_mov_b64_dpp row_newbcast (sw64::mulbc, schur_walk_f64.hip.h); the two wait states between the
// VALU write of an operand and its DPP read are kept by SW64_SETTLE() (tools/check_dpp_hazards.py verifies the built code).
//
// ST is the STORAGE type of S, gamma and lambda: double, or float widened on load (exact) and rounded once on the store of lambda — the
// "block_solve_f64" = 1 route of mpcg_block_solve.  W_k, z_k go through a scratch of N x 210 DOUBLES per trajectory either way.
#pragma once
#include "schur_walk_f64.hip.h"

namespace mpcg {
namespace bs64 {

#pragma clang fp contract(off)

using sw64::mulbc;
using sw64::SFor;

template <typename ST>
struct BlockSolve64Args {
    const ST* S; const ST* gamma; ST* lambda; double* work;    // work: [batch][N][14*14 + 14]
    int N; int batch;
};

// the double held by lane L of this lane's 16-lane row
template <int L>
__device__ __forceinline__ double bc(double b) {
    double r;
    asm("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(b), "n"(L));
    return r;
}
// the double held by lane `src_lane` of the wavefront (byte address src_lane * 4), as two 32-bit halves
__device__ __forceinline__ double bperm(int addr, double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}

template <typename ST>
__global__ __launch_bounds__(64, 2) void bt_block_solve_f64_kernel(BlockSolve64Args<ST> a) {
    constexpr int n = 14, nn = n * n, WS = nn + n, NSL = 4;
    const int N = a.N;
    const int lane = threadIdx.x, lr = lane & 15, g = lane >> 4;
    const bool r14 = lr < n;
    const int lc = r14 ? lr : n - 1;                       // lanes 14, 15 repeat row 13 and store nothing
    const size_t b = blockIdx.x;
    const ST* S = a.S + b * 3 * nn * N;
    const ST* gamma = a.gamma + b * n * N;
    ST* lambda = a.lambda + b * n * N;
    double* work = a.work + b * (size_t)N * WS;
    // this lane's columns: c_j = 4 j + g (clamped for addressing; slots with c_j >= 14 compute on duplicates, store nothing)
    int cj[NSL];
    bool cv[NSL];
#pragma unroll
    for (int j = 0; j < NSL; ++j) { cv[j] = 4 * j + g < n; cj[j] = cv[j] ? 4 * j + g : n - 1; }

    double W[NSL];                                         // this lane's columns of W_{k-1}
    double zp = 0.0;                                       // z_{k-1}[lr] (meaningful in row g = 3)
#pragma unroll
    for (int j = 0; j < NSL; ++j) W[j] = 0.0;
    ST Dn[NSL], Un[NSL], Ln[n], yn;                        // the next knot's operands, as stored (widened when the knot starts)
    auto fetch = [&](int k) {
        const ST* blk = S + (size_t)k * 3 * nn;
#pragma unroll
        for (int j = 0; j < NSL; ++j) {
            Dn[j] = blk[nn + lc + cj[j] * n];
            Un[j] = blk[2 * nn + lc + cj[j] * n];         // (k = N-1: the never-written block, never used)
        }
#pragma unroll
        for (int c = 0; c < n; ++c) Ln[c] = blk[lc + c * n];   // (k = 0: likewise)
        yn = gamma[(size_t)k * n + lc];
    };
    fetch(0);
    for (int k = 0; k < N; ++k) {
        double D[NSL], U[NSL], L[n];
#pragma unroll
        for (int j = 0; j < NSL; ++j) { D[j] = (double)Dn[j]; U[j] = (k < N - 1) ? (double)Un[j] : 0.0; }
#pragma unroll
        for (int c = 0; c < n; ++c) L[c] = (double)Ln[c];
        double y = (double)yn;
        if (k + 1 < N) fetch(k + 1);
        if (k > 0) {
            // Delta = D - L W_{k-1} (own columns), y -= L z_{k-1}: sums over t = 0..13 in order, W / z from lane t of the row
            double t[NSL];
#pragma unroll
            for (int j = 0; j < NSL; ++j) t[j] = 0.0;
            double v = 0.0;
            SW64_SETTLE();
            SFor<0, n>::run([&](auto tc) {
                constexpr int T = decltype(tc)::value;
                if constexpr (T > 0) SW64_FENCE();         // term T's products start after term T-1's sums: five broadcasts in flight, not 70
#pragma unroll
                for (int j = 0; j < NSL; ++j) t[j] = t[j] + mulbc<T>(L[T], W[j]);
                v = v + mulbc<T>(L[T], zp);
            });
#pragma unroll
            for (int j = 0; j < NSL; ++j) D[j] = D[j] - t[j];
            y = y - v;
        }
        // Gauss-Jordan on [Delta | U y], columns dealt over the four rows
        SFor<0, n>::run([&](auto pc_) {
            constexpr int P = decltype(pc_)::value;
            constexpr int GP = P % 4, JP = P / 4;
            // column P of Delta, from its owner row to every row (same lr)
            const double pcol = bperm((GP * 16 + lr) * 4, D[JP]);
            SW64_SETTLE();
            const double pinv = 1.0 / bc<P>(pcol);
            const bool is_p = lr == P;
            double pa[NSL], pu[NSL];
            // columns right of the pivot (slot JP: only in rows g > GP; the others recompute dead columns, which nobody reads again)
#pragma unroll
            for (int j = JP; j < NSL; ++j) pa[j] = D[j] * pinv;
#pragma unroll
            for (int j = 0; j < NSL; ++j) pu[j] = U[j] * pinv;
            double py = y * pinv;
            // pinned in front of the settle (the launder idiom of schur_walk_f64.hip.h): a scaled entry whose only other reader is the pivot
            // lane's select would otherwise be sunk behind the s_nop, next to its DPP reader
#pragma unroll
            for (int j = JP; j < NSL; ++j) asm volatile("" : "+v"(pa[j]));
#pragma unroll
            for (int j = 0; j < NSL; ++j) asm volatile("" : "+v"(pu[j]));
            asm volatile("" : "+v"(py));
            SW64_SETTLE();
#pragma unroll
            for (int j = JP; j < NSL; ++j) {
                const double ta = mulbc<P>(pcol, pa[j]);
                const double na = D[j] - ta;
                D[j] = is_p ? pa[j] : na;
            }
#pragma unroll
            for (int j = 0; j < NSL; ++j) {
                const double tu = mulbc<P>(pcol, pu[j]);
                const double nu = U[j] - tu;
                U[j] = is_p ? pu[j] : nu;
            }
            const double ty = mulbc<P>(pcol, py);
            const double ny = y - ty;
            y = is_p ? py : ny;
            SW64_FENCE();
        });
        // U now holds W_k (own columns), y holds z_k (row g = 3)
#pragma unroll
        for (int j = 0; j < NSL; ++j) W[j] = U[j];
        if (g == 3 && r14) work[(size_t)k * WS + nn + lr] = y;
        if (k < N - 1 && r14) {
#pragma unroll
            for (int j = 0; j < NSL; ++j)
                if (cv[j]) work[(size_t)k * WS + lr + cj[j] * n] = W[j];
        }
        zp = y;
    }
    // make the rows' stores visible to each other's loads (same wave, different lanes: order through the memory system)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // the back substitution sums over all 14 columns in order: rows in lanes, redundantly in the four DPP rows
    double lam = work[(size_t)(N - 1) * WS + nn + lc];     // lambda_{N-1} = z_{N-1}
    if (g == 0 && r14) lambda[(size_t)(N - 1) * n + lr] = (ST)lam;
    double Wn[n], zn = 0.0;
    auto fetch_b = [&](int k) {
#pragma unroll
        for (int c = 0; c < n; ++c) Wn[c] = work[(size_t)k * WS + lc + c * n];
        zn = work[(size_t)k * WS + nn + lc];
    };
    if (N >= 2) fetch_b(N - 2);
    for (int k = N - 2; k >= 0; --k) {
        double Wk[n];
#pragma unroll
        for (int c = 0; c < n; ++c) Wk[c] = Wn[c];
        const double zk = zn;
        if (k > 0) fetch_b(k - 1);
        const double v = sw64::matvec<n>(Wk, lam);
        lam = zk - v;
        if (g == 0 && r14) lambda[(size_t)k * n + lr] = (ST)lam;
    }
}

#pragma clang fp contract(fast)     // (hipcc's default for device code: what the headers included after this one are written for)

}  // namespace bs64
}  // namespace mpcg
