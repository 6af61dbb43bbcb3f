// riccati.hip.h — the time-varying LQR gains K_k = du_k/dx_k of the regularised LQ subproblem, by a backward Riccati sweep over the KKT
// blocks mpcg_generate_kkt leaves in device memory (include/mpcg_riccati.h: the contract and the recursion):
//   P_{N-1} = Q_{N-1} + rho I;   k = N-2 .. 0:   H_uu = R_k + rho I + B_k^T P_{k+1} B_k,   H_ux = B_k^T P_{k+1} A_k,   K_k = -H_uu^-1 H_ux,
//   P_k = Q_k + rho I + A_k^T P_{k+1} A_k + H_ux^T K_k   (lower triangle computed, then mirrored: exactly symmetric)
// with A_k = -C[k][0 : n^2], B_k = -C[k][n^2 : n^2 + n m] (d_C_dense stores -A, -B).
//
// ONE WAVEFRONT PER TRAJECTORY, one workgroup of 64 lanes each, sweeping k = N-2 .. 0 as block_solve.hip.h sweeps its knots: a dependent chain
// per trajectory, so the blocks Q, R, A, B of knot k-1 are requested from HBM into registers before knot k is eliminated.  Everything else lives in
// the wavefront's own LDS as doubles, column-major with leading dimensions LD = n rounded up to 4 and LM = m rounded up to 4 (every column starts
// 32-byte aligned, the pads hold zeros from the start of the kernel and are never written, so the inner loops run over pairs of rows with
// 16-byte reads and need no tail):
//   P   LD x LD        P_{k+1}; Q_k + rho I once P A and P B are formed; P_k at the end of the knot
//   X   LD x (n + m)   [A_k | B_k]
//   Y   LD x (n + m)   [P A_k | P B_k]
//   W   LM x (m + n)   [H_uu | H_ux], eliminated in place to [. | H_uu^-1 H_ux] = [. | -K_k]
//   Hk  LM x n         H_ux kept for H_ux^T K_k
// riccati_lds_doubles(n, m) = LD^2 + 2 LD (n + m) + LM (m + 2 n) doubles: 9,664 bytes at 14 x 7 (16 wavefronts per CU by LDS), 65,536 at 32 x 32.
// The phases of a knot, each closed by a wavefront-level fence (a single wavefront owns the region: no s_barrier, nothing crosses trajectories):
//   1  X <- -C_k (widened), H_uu <- R_k + rho I                                      from the prefetched registers
//   2  Y = P X                    4 x 2 outputs per lane and pass, rows in pairs: six 16-byte reads per 16 FMAs
//   2' P <- Q_k + rho I           (P_{k+1} has been consumed)
//   3  X^T Y                      2 x 2 outputs per lane and pass, both operands are columns: four 16-byte reads per 8 FMAs.  Of the
//                                 (n + m)^2 outputs only the lower triangle of A^T (P A) (added to P), B^T (P A) = H_ux (to W and Hk) and
//                                 B^T (P B) (added to H_uu) are enumerated; A^T (P B) = H_ux^T is not.
//   4  pivot-free Gauss-Jordan on W, one column per lane, columns left of the pivot skipped (the elimination scheme of the path: pivot inverse,
//      scaled pivot row, rank-one update); H_uu is symmetric positive definite for rho > 0.  One fence per pivot.
//   5  K_k = -W[:, m:] stored (rounded once to the storage type), P -= Hk^T W[:, m:] on the lower triangle, then the mirror.
// Float64 inside for both entries, as the plant kernels: IO = float widens on load (exact) and rounds K once.  <IO, 14, 7> has the loop bounds at
// compile time; <IO, 0, 0> reads (n, m) from the arguments and serves every other shape (its prefetch holds RIC_PF_RT elements per lane, what lies
// beyond — a knot of tot = 2 n^2 + m^2 + n m > 64 RIC_PF_RT = 1280 elements, first at 18 x 18 with 1296 — is loaded where it is used).  Loop bounds are host arguments only: a trajectory of NaN, Inf or zeros ends
// like any other and, a workgroup of its own, touches nobody else's data.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpcg {
namespace ric {

template <typename IO>
struct RiccatiArgsT {
    const IO* G; const IO* C; const IO* rho_v; IO* K;      // rho_v: one rho per trajectory, or null: `rho`
    double rho;
    int n, m, N;
};

__host__ __device__ constexpr int r4(int x) { return (x + 3) & ~3; }
__host__ __device__ constexpr size_t riccati_lds_doubles(int n, int m) {
    return (size_t)r4(n) * r4(n) + 2 * (size_t)r4(n) * (n + m) + (size_t)r4(m) * (m + 2 * n);
}

#ifndef RIC_PF_RT
#define RIC_PF_RT 20          // elements per lane the run-time-dimension build prefetches: all of a knot up to (n^2 + m^2) + (n^2 + n m) = 1280
#endif

// the wavefront's LDS writes before, its LDS reads after (LDS operations of one wavefront complete in order; the fences keep the compiler's order)
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// t-th pair (ti, tj), tj <= ti, of the lower triangle in row order
__device__ __forceinline__ void tri_decode(int t, int& ti, int& tj) {
    int r = (int)((__fsqrt_rn(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    if (r * (r + 1) / 2 > t) --r;
    if ((r + 1) * (r + 2) / 2 <= t) ++r;
    ti = r;
    tj = t - r * (r + 1) / 2;
}

__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }

template <typename IO, int NC, int MC>
__global__ __launch_bounds__(64) void riccati_gains_kernel(RiccatiArgsT<IO> a) {
    extern __shared__ __attribute__((aligned(16))) double ric_lds[];
    constexpr bool CT = NC > 0;
    constexpr int U8 = CT ? 8 : 2, U4 = CT ? 4 : 2, U1 = CT ? 8 : 1;      // unroll factors of the inner loops
    const int n = CT ? NC : a.n, m = CT ? MC : a.m, N = a.N;
    const int w = n + m, LD = r4(n), LM = r4(m), nn = n * n, mm = m * m, nm = n * m;
    const int n2 = (n + 1) & ~1, m2 = (m + 1) & ~1;
    const int Gset = nn + mm, Cset = nn + nm, tot = Gset + Cset;
    constexpr int PF = CT ? (2 * NC * NC + MC * MC + NC * MC + 63) / 64 : RIC_PF_RT;
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    double* const P = ric_lds;
    double* const X = P + LD * LD;
    double* const Y = X + LD * w;
    double* const W = Y + LD * w;
    double* const Hk = W + LM * w;
    const int lds_total = LD * LD + 2 * LD * w + LM * (w + n);
    const IO* const G = a.G + b * ((size_t)Gset * N - mm);
    const IO* const C = a.C + b * ((size_t)Cset * (N - 1));
    IO* const K = a.K + b * ((size_t)nm * (N - 1));
    const double rho = a.rho_v ? (double)a.rho_v[b] : a.rho;

    for (int e = lane; e < lds_total; e += 64) ric_lds[e] = 0.0;
    wave_fence();
    // P_{N-1} = Q_{N-1} + rho I
    for (int e = lane; e < nn; e += 64) {
        const int i = e % n, j = e / n;
        const double v = (double)G[(size_t)(N - 1) * Gset + e];
        P[i + j * LD] = i == j ? v + rho : v;
    }

    // element e of knot k's blocks as they lie in memory: [Q | R] of d_G_dense, then [-A | -B] of d_C_dense
    auto load = [&](int k, int e) -> IO { return e < Gset ? G[(size_t)k * Gset + e] : C[(size_t)k * Cset + (e - Gset)]; };
    // ... to its place in LDS: Q in the pass after P has been consumed (qpass), R, A, B in the pass before
    auto place = [&](int e, double v, bool qpass) {
        if (e < nn) {
            if (qpass) { const int i = e % n, j = e / n; P[i + j * LD] = i == j ? v + rho : v; }
        } else if (!qpass) {
            if (e < Gset) { const int f = e - nn, i = f % m, j = f / m; W[i + j * LM] = i == j ? v + rho : v; }
            else { const int f = e - Gset, i = f % n, j = f / n; X[i + j * LD] = -v; }
        }
    };
    IO pf[PF];
    auto fetch = [&](int k) {
#pragma unroll
        for (int c = 0; c < PF; ++c) {
            const int e = lane + 64 * c;
            pf[c] = e < tot ? load(k, e) : IO(0);
        }
    };
    auto place_all = [&](int k, const IO (&cur)[PF], bool qpass) {
#pragma unroll
        for (int c = 0; c < PF; ++c) {
            const int e = lane + 64 * c;
            if (e < tot) place(e, (double)cur[c], qpass);
        }
        if constexpr (!CT)
            for (int e = lane + 64 * PF; e < tot; e += 64) place(e, (double)load(k, e), qpass);
    };

    fetch(N - 2);
    for (int k = N - 2; k >= 0; --k) {
        IO cur[PF];
#pragma unroll
        for (int c = 0; c < PF; ++c) cur[c] = pf[c];
        if (k > 0) fetch(k - 1);

        // ---- 1: X = [A | B], H_uu = R + rho I ----
        place_all(k, cur, false);
        wave_fence();

        // ---- 2: Y = P X ----
        {
            const int rb = LD / 4, cp = (w + 1) / 2;
            for (int t = lane; t < rb * cp; t += 64) {
                const int i0 = 4 * (t % rb), j0 = 2 * (t / rb);
                const bool two = j0 + 1 < w;
                const double* Pp = P + i0;
                const double* x0 = X + j0 * LD;
                const double* x1 = X + (two ? j0 + 1 : j0) * LD;
                double a00 = 0, a10 = 0, a20 = 0, a30 = 0, a01 = 0, a11 = 0, a21 = 0, a31 = 0;
#pragma unroll U8
                for (int l = 0; l < n2; l += 2) {
                    const double2 pa = ld2(Pp + l * LD), pb = ld2(Pp + l * LD + 2);
                    const double2 qa = ld2(Pp + (l + 1) * LD), qb = ld2(Pp + (l + 1) * LD + 2);
                    const double2 u = ld2(x0 + l), v = ld2(x1 + l);
                    a00 = fma(pa.x, u.x, a00); a10 = fma(pa.y, u.x, a10); a20 = fma(pb.x, u.x, a20); a30 = fma(pb.y, u.x, a30);
                    a01 = fma(pa.x, v.x, a01); a11 = fma(pa.y, v.x, a11); a21 = fma(pb.x, v.x, a21); a31 = fma(pb.y, v.x, a31);
                    a00 = fma(qa.x, u.y, a00); a10 = fma(qa.y, u.y, a10); a20 = fma(qb.x, u.y, a20); a30 = fma(qb.y, u.y, a30);
                    a01 = fma(qa.x, v.y, a01); a11 = fma(qa.y, v.y, a11); a21 = fma(qb.x, v.y, a21); a31 = fma(qb.y, v.y, a31);
                }
                // (rows of P beyond n are zero pads: so are those of Y)
                double* y0 = Y + i0 + j0 * LD;
                *reinterpret_cast<double2*>(y0) = make_double2(a00, a10);
                *reinterpret_cast<double2*>(y0 + 2) = make_double2(a20, a30);
                if (two) {
                    *reinterpret_cast<double2*>(y0 + LD) = make_double2(a01, a11);
                    *reinterpret_cast<double2*>(y0 + LD + 2) = make_double2(a21, a31);
                }
            }
        }
        wave_fence();

        // ---- 2': P = Q + rho I ----
        place_all(k, cur, true);
        wave_fence();

        // ---- 3: the needed blocks of X^T Y ----
        {
            const int ntile = (w + 1) / 2, tA = n / 2, triA = tA * (tA + 1) / 2;
            const int tasks = triA + (ntile - tA) * ntile;      // tile rows inside A: up to the diagonal; the rest (B, and a row straddling both): all
            auto emit = [&](int i, int j, double g) {
                if (i < n) {
                    if (j <= i) P[i + j * LD] += g;
                } else if (j < n) {
                    W[(i - n) + (m + j) * LM] = g;
                    Hk[(i - n) + j * LM] = g;
                } else {
                    W[(i - n) + (j - n) * LM] += g;
                }
            };
            for (int t = lane; t < tasks; t += 64) {
                int ti, tj;
                if (t < triA) tri_decode(t, ti, tj);
                else { const int r = t - triA; ti = tA + r / ntile; tj = r % ntile; }
                const int i0 = 2 * ti, j0 = 2 * tj;
                const bool ri = i0 + 1 < w, rj = j0 + 1 < w;
                const double* xi0 = X + i0 * LD;
                const double* xi1 = X + (ri ? i0 + 1 : i0) * LD;
                const double* yj0 = Y + j0 * LD;
                const double* yj1 = Y + (rj ? j0 + 1 : j0) * LD;
                double g00 = 0, g10 = 0, g01 = 0, g11 = 0;
#pragma unroll U8
                for (int l = 0; l < n2; l += 2) {
                    const double2 u0 = ld2(xi0 + l), u1 = ld2(xi1 + l), v0 = ld2(yj0 + l), v1 = ld2(yj1 + l);
                    g00 = fma(u0.x, v0.x, g00); g10 = fma(u1.x, v0.x, g10); g01 = fma(u0.x, v1.x, g01); g11 = fma(u1.x, v1.x, g11);
                    g00 = fma(u0.y, v0.y, g00); g10 = fma(u1.y, v0.y, g10); g01 = fma(u0.y, v1.y, g01); g11 = fma(u1.y, v1.y, g11);
                }
                emit(i0, j0, g00);
                if (ri) emit(i0 + 1, j0, g10);
                if (rj) emit(i0, j0 + 1, g01);
                if (ri && rj) emit(i0 + 1, j0 + 1, g11);
            }
        }
        wave_fence();

        // ---- 4: [H_uu | H_ux] -> [. | H_uu^-1 H_ux], a column per lane ----
        for (int p = 0; p < m; ++p) {
            const double* pc = W + p * LM;
            const double pinv = 1.0 / pc[p];
            for (int j = p + 1 + lane; j < w; j += 64) {
                double* col = W + j * LM;
                const double s = col[p] * pinv;
#pragma unroll U1
                for (int i = 0; i < m; ++i)
                    if (i != p) col[i] = fma(-pc[i], s, col[i]);
                col[p] = s;
            }
            wave_fence();
        }

        // ---- 5: K_k out, P -= H_ux^T (H_uu^-1 H_ux) on the lower triangle ----
        const double* Z = W + m * LM;                           // H_uu^-1 H_ux = -K_k, LM x n
        for (int e = lane; e < nm; e += 64) {
            const int i = e % m, j = e / m;
            K[(size_t)k * nm + e] = (IO)(-Z[i + j * LM]);
        }
        {
            const int nt = (n + 1) / 2;
            for (int t = lane; t < nt * (nt + 1) / 2; t += 64) {
                int ti, tj;
                tri_decode(t, ti, tj);
                const int i0 = 2 * ti, j0 = 2 * tj;
                const bool ri = i0 + 1 < n, rj = j0 + 1 < n;
                const double* hi0 = Hk + i0 * LM;
                const double* hi1 = Hk + (ri ? i0 + 1 : i0) * LM;
                const double* zj0 = Z + j0 * LM;
                const double* zj1 = Z + (rj ? j0 + 1 : j0) * LM;
                double g00 = 0, g10 = 0, g01 = 0, g11 = 0;
#pragma unroll U4
                for (int l = 0; l < m2; l += 2) {
                    const double2 u0 = ld2(hi0 + l), u1 = ld2(hi1 + l), v0 = ld2(zj0 + l), v1 = ld2(zj1 + l);
                    g00 = fma(u0.x, v0.x, g00); g10 = fma(u1.x, v0.x, g10); g01 = fma(u0.x, v1.x, g01); g11 = fma(u1.x, v1.x, g11);
                    g00 = fma(u0.y, v0.y, g00); g10 = fma(u1.y, v0.y, g10); g01 = fma(u0.y, v1.y, g01); g11 = fma(u1.y, v1.y, g11);
                }
                P[i0 + j0 * LD] -= g00;
                if (ri) P[i0 + 1 + j0 * LD] -= g10;
                if (rj && j0 + 1 <= i0) P[i0 + (j0 + 1) * LD] -= g01;
                if (ri && rj) P[i0 + 1 + (j0 + 1) * LD] -= g11;
            }
        }
        wave_fence();
        // the upper triangle is the mirror of the lower: P_k exactly symmetric
        for (int e = lane; e < nn; e += 64) {
            const int i = e % n, j = e / n;
            if (i < j) P[i + j * LD] = P[j + i * LD];
        }
        wave_fence();
    }
}

}  // namespace ric
}  // namespace mpcg
