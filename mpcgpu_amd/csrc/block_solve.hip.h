// block_solve.hip.h — batched block-tridiagonal DIRECT solve of S lambda = gamma on the GPU.
//
// The reference's second linear-system path (LINSYS_SOLVE == 0) ships the Schur matrix to the host and calls QDLDL
// (qdldl_solve_schur, include/qdldl/sqp.cuh:22-49: sparse LDL^T factor + solve per SQP iteration, one trajectory,
// one CPU thread).  The GPU-native counterpart keeps the system where mpcg_form_schur left it (bd layout, stored
// negated) and runs a block LU sweep per trajectory on the register/DPP primitives of dpp_rows.hip.h:
//   Delta_0 = D_0, y_0 = gamma_0;  k >= 1:  Delta_k = D_k - L_k W_{k-1},  y_k = gamma_k - L_k z_{k-1};
//   z_k = Delta_k^-1 y_k,  W_k = Delta_k^-1 U_k;   lambda_{N-1} = z_{N-1},  lambda_k = z_k - W_k lambda_{k+1}
// (D_k = S[k,1], L_k = S[k,0], U_k = S[k,2]; W_k and z_k come out of ONE pivot-free Gauss-Jordan elimination of
// [Delta_k | U_k y_k], the reference's elimination scheme — include/utils/matrix.cuh:120-238 — with the right-hand
// sides in place of the identity and the already-eliminated columns skipped).
// FOUR trajectories per wavefront — one per 16-lane DPP row, lane r < 14 holds row r of every 14x14 operand — all
// four sweeping k = 0..N-1 in lock-step; W_k and z_k go through a global scratch of N x 210 floats per trajectory
// for the back substitution.  ~1.7 k instructions per knot and wave, no LDS, no barriers; the sweep is serial in k
// (that is what PCG avoids for ONE trajectory), so this is the throughput solver for batches: 1/50 of the flops of
// 167 PCG iterations.  The test oracle restates the same operation order on the CPU: results are bit-identical (tested).
//
// bt_block_solve_wide_kernel<CT, ST> is the same sweep with ONE trajectory per wavefront, in float or with the sweep in
// DOUBLE (linsys_t = double, USE_DOUBLES = 1 of include/common/settings.cuh:41-49; and "float64 inside, float outputs"
// for float callers).  CT is the sweep type — the scratch holds N x 210 CTs per trajectory — and ST the STORAGE type of
// S, gamma and lambda: widened on load (exact) and rounded once on the store of lambda.  One body serves both
// precisions, so the operation order the oracle pins bit for bit is written once; what float and double differ in is
// the "float and double rows" section of dpp_rows.hip.h.
#pragma once
#include "dpp_rows.hip.h"

namespace mpcg {

#pragma clang fp contract(off)

template <typename CT, typename ST = CT>
struct BlockSolveArgsT {
    const ST* S; const ST* gamma; ST* lambda; CT* work;    // work: [batch][N][14*14 + 14]
    int N; int batch;
};
typedef BlockSolveArgsT<float> BlockSolveArgs;

// lambda_k = z_k - W_k lambda_{k+1} for k = N-2..0, from lam = lambda_{N-1} (stored by the caller): rows in lanes, the sum over all 14
// columns in order, W_k and z_k prefetched one knot ahead from the scratch.  Lanes with `st` store.
template <typename CT, typename ST>
__device__ __forceinline__ void back_substitute(const CT* work, ST* lambda, int N, int lr, int lc, CT lam, bool st) {
    using namespace sdpp;
    constexpr int n = 14, nn = n * n, WS = nn + n;
    CT Wn[n], zn = 0;
    auto fetch_b = [&](int k) {
#pragma unroll
        for (int c = 0; c < n; ++c) Wn[c] = work[(size_t)k * WS + lc + c * n];
        zn = work[(size_t)k * WS + nn + lc];
    };
    if (N >= 2) fetch_b(N - 2);
    for (int k = N - 2; k >= 0; --k) {
        CT Wk[n];
#pragma unroll
        for (int c = 0; c < n; ++c) Wk[c] = Wn[c];
        const CT zk = zn;
        if (k > 0) fetch_b(k - 1);
        const CT v = matvec<n>(Wk, lam);
        lam = zk - v;
        if (st) lambda[(size_t)k * n + lr] = (ST)lam;
    }
}

__global__ __launch_bounds__(64, 2) void bt_block_solve_kernel(BlockSolveArgs a) {
    using namespace sdpp;
    constexpr int n = 14, nn = n * n, WS = nn + n;
    const int N = a.N;
    const int lane = threadIdx.x, lr = lane & 15;
    const bool r14 = lr < n;
    const int lc = r14 ? lr : n - 1;                       // lanes 14, 15 repeat row 13 and store nothing
    const unsigned traj = blockIdx.x * 4u + (unsigned)(lane >> 4);
    const bool live = traj < (unsigned)a.batch;
    const size_t b = live ? traj : (unsigned)a.batch - 1;  // dead rows redo the last trajectory and store nothing
    const float* S = a.S + b * 3 * nn * N;
    const float* gamma = a.gamma + b * n * N;
    float* lambda = a.lambda + b * n * N;
    float* work = a.work + b * (size_t)N * WS;
    const bool st = live && r14;

    float W[n];                                            // W_{k-1}, rows in lanes
    float zp = 0.f;                                        // z_{k-1}, element lr
#pragma unroll
    for (int c = 0; c < n; ++c) W[c] = 0.f;
    // operands of the NEXT knot are requested before the current knot is eliminated: the sweep is one dependent
    // chain per trajectory, an un-prefetched HBM round trip per knot would double its length
    float Dn[n], Ln[n], Un[n], yn;
    auto fetch = [&](int k) {
        load_rows(Dn, S + (size_t)k * 3 * nn + nn, n, lr, true);
        load_rows(Ln, S + (size_t)k * 3 * nn, n, lr, true);            // (k = 0: the never-written block, never used)
        load_rows(Un, S + (size_t)k * 3 * nn + 2 * nn, n, lr, true);   // (k = N-1: likewise)
        yn = gamma[(size_t)k * n + lc];
    };
    fetch(0);
    for (int k = 0; k < N; ++k) {
        float D[n], L[n], R[n + 1];
#pragma unroll
        for (int c = 0; c < n; ++c) { D[c] = Dn[c]; L[c] = Ln[c]; R[c] = (k < N - 1) ? Un[c] : 0.f; }
        float y = yn;
        if (k + 1 < N) fetch(k + 1);
        if (k > 0) {
            float t[n];
            gemm_nn<n, n>(L, W, t);                        // L_k W_{k-1}
#pragma unroll
            for (int c = 0; c < n; ++c) D[c] = D[c] - t[c];
            const float v = matvec<n>(L, zp);              // L_k z_{k-1}
            y = y - v;
        }
        // [Delta_k | U_k y_k] -> [I | W_k z_k] in one elimination (the last block row carries y only)
        R[n] = y;
        solve_aug<n, n + 1>(D, R, lr);
#pragma unroll
        for (int c = 0; c < n; ++c) W[c] = R[c];
        const float z = R[n];
        if (st) work[(size_t)k * WS + nn + lr] = z;
        if (k < N - 1) store_rows(W, work + (size_t)k * WS, n, lr, st, 1.f);
        zp = z;
    }
    if (st) lambda[(size_t)(N - 1) * n + lr] = zp;         // lambda_{N-1} = z_{N-1}
    back_substitute(work, lambda, N, lr, lc, zp, st);
}

// ---- the same sweep for FEW trajectories, and the only layout built in double: one trajectory per wavefront, the 29 columns of
// [Delta | U y] dealt round-robin to the four 16-lane DPP rows (lane = 16 g + r holds row r of columns c = 4 j + g, j = 0..3, of Delta and
// of U; g = 3 also carries y / z).  Per pivot one bperm moves the pivot column from its owner row to the other three; everything else stays
// inside a row (row_newbcast).  Every entry goes through exactly the operations of the narrow kernel above, so the results are
// bit-identical; ~0.9 k instead of ~2.3 k instructions per knot on the critical path in float.  In double the live set is ~45 doubles per
// lane (D, U, W: 4 each, L: 14, the prefetch: 23 in the storage type), which fits the register file with no scratch.  The back substitution
// sums over all 14 columns in order, so it runs in the narrow layout (redundantly in the four rows). ----
template <typename CT, typename ST>
__global__ __launch_bounds__(64, 2) void bt_block_solve_wide_kernel(BlockSolveArgsT<CT, ST> a) {
    using namespace sdpp;
    constexpr int n = 14, nn = n * n, WS = nn + n, NSL = 4;
    const int N = a.N;
    const int lane = threadIdx.x, lr = lane & 15, g = lane >> 4;
    const bool r14 = lr < n;
    const int lc = r14 ? lr : n - 1;                       // lanes 14, 15 repeat row 13 and store nothing
    const size_t b = blockIdx.x;
    const ST* S = a.S + b * 3 * nn * N;
    const ST* gamma = a.gamma + b * n * N;
    ST* lambda = a.lambda + b * n * N;
    CT* work = a.work + b * (size_t)N * WS;
    // this lane's columns: c_j = 4 j + g (clamped for addressing; slots with c_j >= 14 compute on duplicates, store nothing)
    int cj[NSL];
    bool cv[NSL];
#pragma unroll
    for (int j = 0; j < NSL; ++j) { cv[j] = 4 * j + g < n; cj[j] = cv[j] ? 4 * j + g : n - 1; }

    CT W[NSL];                                             // this lane's columns of W_{k-1}
    CT zp = 0;                                             // z_{k-1}[lr] (meaningful in row g = 3)
#pragma unroll
    for (int j = 0; j < NSL; ++j) W[j] = 0;
    // operands of the NEXT knot are requested before the current knot is eliminated (as in the narrow kernel), as stored: widened when the knot starts
    ST Dn[NSL], Un[NSL], Ln[n], yn;
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
        CT D[NSL], U[NSL], L[n];
#pragma unroll
        for (int j = 0; j < NSL; ++j) { D[j] = (CT)Dn[j]; U[j] = (k < N - 1) ? (CT)Un[j] : CT(0); }
#pragma unroll
        for (int c = 0; c < n; ++c) L[c] = (CT)Ln[c];
        CT y = (CT)yn;
        if (k + 1 < N) fetch(k + 1);
        if (k > 0) {
            // Delta = D - L W_{k-1} (own columns), y -= L z_{k-1}: sums over t = 0..13 in order, W / z from lane t of the row
            CT t[NSL];
#pragma unroll
            for (int j = 0; j < NSL; ++j) t[j] = 0;
            CT v = 0;
            settle<CT>();
            SFor<0, n>::run([&](auto tc) {
                constexpr int T = decltype(tc)::value;
                if constexpr (T > 0) sched_fence<CT>();    // (double) term T's products start after term T-1's sums: five broadcasts in flight, not 70
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
            const CT pcol = bperm((GP * 16 + lr) * 4, D[JP]);
            settle<CT>();
            const CT pinv = CT(1) / rbc<P>(pcol);
            const bool is_p = lr == P;
            CT pa[NSL], pu[NSL];
            // columns right of the pivot (slot JP: only in rows g > GP; the others recompute dead columns, which nobody reads again)
#pragma unroll
            for (int j = JP; j < NSL; ++j) pa[j] = D[j] * pinv;
#pragma unroll
            for (int j = 0; j < NSL; ++j) pu[j] = U[j] * pinv;
            CT py = y * pinv;
            // (double) pinned in front of the settle: a scaled entry whose only other reader is the pivot lane's select would otherwise be
            // sunk behind the s_nop, next to its DPP reader
#pragma unroll
            for (int j = JP; j < NSL; ++j) pin(pa[j]);
#pragma unroll
            for (int j = 0; j < NSL; ++j) pin(pu[j]);
            pin(py);
            settle<CT>();
#pragma unroll
            for (int j = JP; j < NSL; ++j) {
                const CT ta = mulbc<P>(pcol, pa[j]);
                const CT na = D[j] - ta;
                D[j] = is_p ? pa[j] : na;
            }
#pragma unroll
            for (int j = 0; j < NSL; ++j) {
                const CT tu = mulbc<P>(pcol, pu[j]);
                const CT nu = U[j] - tu;
                U[j] = is_p ? pu[j] : nu;
            }
            const CT ty = mulbc<P>(pcol, py);
            const CT ny = y - ty;
            y = is_p ? py : ny;
            sched_fence<CT>();
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
    const CT lam = work[(size_t)(N - 1) * WS + nn + lc];   // lambda_{N-1} = z_{N-1}
    if (g == 0 && r14) lambda[(size_t)(N - 1) * n + lr] = (ST)lam;
    back_substitute(work, lambda, N, lr, lc, lam, g == 0 && r14);
}
// Built as <float, float> (mpcg_block_solve), <double, double> (mpcg_block_solve_f64) and <double, float> ("block_solve_f64" = 1).  The
// four-per-wavefront layout of bt_block_solve_kernel would hold ~100 doubles per lane (200 VGPRs before temporaries) and is NOT built in
// double: there the wide layout serves every batch, and "block_solve_wide" is not read.

}  // namespace mpcg

#pragma clang fp contract(fast)     // (hipcc's default for device code: what the headers included after this one are written for)
