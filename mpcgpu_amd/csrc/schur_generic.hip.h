// schur_generic.hip.h — the steps either side of the PCG for ANY state and control size (1 <= m <= n <= 64), gfx950 HIP:
//   gen::form_schur_kernel + gen::complete_ss_kernel   (G, C, g, c, rho) -> (S, Pinv, gamma), G <- G^-1
//        replaces form_S_gamma_Pinv_kernel / form_schur_system (include/pcg/linsys_setup.cuh:565-656)
//   gen::compute_dz_kernel                             dz = G^-1 (g - C^T lambda)      replaces compute_dz (include/common/dz.cuh:3-136)
//   gen::bt_block_solve_kernel                         block-tridiagonal direct solve of S lambda = gamma (float, double, float storage / double sweep)
// and, ahead of them, what every producer kernel of the library shares: the argument structs of formation and dz (the register-resident
// kernels of schur_walk.hip.h take the same ones) and the two CSR kernels of the QDLDL path.
//
// Arithmetic follows the reference operation for operation and is written with contraction OFF, sequential inner products and pivot-free
// Gauss-Jordan (pivot row scaled by 1 / pivot, then eliminated from every other row), so that it is BIT-IDENTICAL to the C oracle
// (oracle/mpcg_oracle_impl.inc, built with -ffp-contract=off) — the parity tests compare bits, not tolerances.  The dimensions are run-time
// values and the operands live in DYNAMIC LDS sized from (n, m).  These are the library's only LDS producers: every shape other than 14 x 7
// runs them, and 14 x 7 — whose default is the register-resident kernels — runs them under "schur_dpp" / "dz_dpp" = 0, under
// "producers_generic" = 1 and for calls beyond the register-resident kernels' 31-bit byte offsets.
//
// The reference runs both halves of the Schur formation in one cooperative kernel with a grid sync between them (:600); a kernel boundary
// (~1.5 us on this chip) is cheaper than any grid barrier, so they are two launches here.  The reference also overwrites G with its block
// inverses while other blocks may still be reading the raw blocks (row k writes slot k-1 which row k-1 reads, :321 vs :372 — a benign race
// there); here the first kernel writes the inverses to a staging buffer and the second copies them into G.
//
// Mapping.  A workgroup of blockDim.x = 64 (n <= 16) or 256 threads owns one block row (formation, completion), a few knots (dz) or one
// trajectory (block solve).  Over an operand with `rows` rows a thread keeps ONE row r = tid % rows and walks the columns c0, c0 + cs, ...
// (cs = blockDim.x / rows; the blockDim.x % rows lanes left over idle): the integer division by a run-time dimension happens once per
// kernel, not once per element, and every bulk LDS access is unit-stride over the lanes — A[r + t * rows] is consecutive (lanes of another
// column repeat the address: a broadcast), B[t + c * n] is one address per column group, the transposed operand B[c + t * k] of the
// transB products is consecutive in c.  So power-of-two n (power-of-two column strides) costs nothing there and the leading dimensions
// are NOT padded; padding them would put 2-way conflicts into exactly these bulk accesses (r + c * (n + 1) wraps the 32 banks inside a
// half-wave).  The two strided accesses that remain: the pivot row of the Gauss-Jordan step (n elements per pivot, against 2 n^2 in the
// update) and the transposition of phi, which walks the columns skewed by the row ((q + r) mod n) so that read and write both spread
// over the banks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mpcg {

constexpr int SCH_THREADS = 64;      // workgroup of the CSR kernels

template <typename T>
struct SchurArgsT {
    const T* G; const T* C; const T* g; const T* c;
    T* S; T* Pinv; T* gamma; T* Ginv_scratch; T* Ginv_out;
    T rho; int n; int m; int N; int batch; int ss;
    int pinv;                 // 0: S and gamma only (no Pinv block is computed or written)
    int k0_only;              // reserved, always 0 (no kernel reads it; it stays so that the kernel arguments keep their offsets)
};
typedef SchurArgsT<float> SchurArgs;
// The per-trajectory form (mpcg_form_schur_rhov): trajectory b is formed with rho_v[b]; `rho` of the base is not read.  The scalar kernels take
// the base, so their arguments keep their offsets.
template <typename T>
struct SchurArgsVT : SchurArgsT<T> { const T* rho_v; };
template <typename T> __device__ __forceinline__ T rho_of(const SchurArgsT<T>& a, int) { return a.rho; }
template <typename T> __device__ __forceinline__ T rho_of(const SchurArgsVT<T>& a, int b) { return a.rho_v[b]; }

template <typename T>
struct DzArgsT { const T* Ginv; const T* C; const T* g; const T* lambda; T* dz; int n; int m; int N; int batch; };
typedef DzArgsT<float> DzArgs;

#pragma clang fp contract(off)

// ---- CSR side of the QDLDL twin ----
// prep_csr_kernel: pattern of the lower triangle of a symmetric block-tridiagonal matrix, exactly
// include/utils/csr.cuh:40-73 (row (k,i) holds (k>0)*n + i+1 entries, first column (k>0)*(k-1)*n).
__global__ __launch_bounds__(SCH_THREADS) void prep_csr_kernel(int n, int N, int* col_ptr, int* row_ind) {
    const int brow = n * n + (n * (n + 1)) / 2;
    for (int k = blockIdx.x; k < N; k += gridDim.x)
        for (int row = threadIdx.x; row < n; row += SCH_THREADS) {
            if (k == 0 && row == 0) col_ptr[0] = 0;
            const int tri = ((row + 1) * row) / 2;
            const int off = (k > 0) * ((n + 1) * n) / 2 + (k > 0) * (k - 1) * brow + (k > 0) * row * n + tri;
            const int len = (k > 0) * n + row + 1;
            col_ptr[k * n + row + 1] = off + len;
            for (int c = 0; c < len; ++c) row_ind[off + c] = (k > 0) * (k - 1) * n + c;
        }
}
// values: what form_schur_qdl_kernel leaves in d_val (include/qdldl/linsys_setup.cuh:12-336 via
// store_block_csr_lowertri, include/utils/csr.cuh:9-36), gathered from the bd-layout S that
// mpcg_form_schur produced: left block S[k,0] then the lower triangle of S[k,1], scaled by mult.
struct CsrArgs { const float* S; float* val; float mult; int n; int N; int batch; };
__global__ __launch_bounds__(SCH_THREADS) void bd_to_csr_kernel(CsrArgs a) {
    const int n = a.n, N = a.N, nn = n * n;
    const int brow = nn + (n * (n + 1)) / 2;
    const size_t nnz = (size_t)(N - 1) * nn + (size_t)N * ((n * (n + 1)) / 2);
    for (long item = blockIdx.x; item < (long)a.batch * N; item += gridDim.x) {
        const int b = (int)(item / N), k = (int)(item % N);
        const float* Sk = a.S + ((size_t)b * N + k) * 3 * nn;
        float* val = a.val + (size_t)b * nnz;
        const int per_row_max = n + n;
        for (int e = threadIdx.x; e < n * per_row_max; e += SCH_THREADS) {
            const int row = e / per_row_max, c = e % per_row_max;
            const int tri = ((row + 1) * row) / 2;
            const int off = (k > 0) * ((n + 1) * n) / 2 + (k > 0) * (k - 1) * brow + (k > 0) * row * n + tri;
            if (k > 0 && c < n) val[off + c] = a.mult * Sk[row + c * n];                               // left block
            else if (c >= n && c - n <= row) val[off + (k > 0) * n + (c - n)] = a.mult * Sk[nn + row + (c - n) * n];   // diagonal block
        }
    }
}

namespace gen {

struct Lane { int r, c0, cs; };      // this thread's row, first column and column step over an operand with `rows` rows (idle: c0 beyond any column)
__device__ __forceinline__ Lane lane_of(int rows) {
    Lane l;
    l.cs = (int)blockDim.x / rows;
    l.r = (int)threadIdx.x % rows;
    l.c0 = (int)threadIdx.x / rows;
    if (l.c0 >= l.cs) l.c0 = 1 << 20;
    return l;
}

template <typename T>
__device__ __forceinline__ void g_copy(int cnt, const T* src, T* dst, T mult = (T)1) {
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) dst[e] = src[e] * mult;
}
// C[m x k] = mult * (A[m x n] * B[n x k]) (column-major); TB: B stored k x n.  Sequential over n.  l = lane_of(m).
template <bool TB, typename T>
__device__ __forceinline__ void g_gemm(const Lane l, int m, int n, int k, const T* A, const T* B, T* C, T mult = (T)1) {
    for (int c = l.c0; c < k; c += l.cs) {
        T acc = 0;
#pragma unroll 4
        for (int t = 0; t < n; ++t) acc += A[l.r + t * m] * (TB ? B[c + t * k] : B[t + c * n]);
        C[l.r + c * m] = acc * mult;
    }
}
template <typename T>
__device__ __forceinline__ void g_matvec(int rows, int cols, const T* M, const T* v, T* out) {
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        T acc = 0;
        for (int c = 0; c < cols; ++c) acc += M[r + c * rows] * v[c];
        out[r] = acc;
    }
}
// one Gauss-Jordan step on [A | I] (pivot piv < n): scratch sc = {scaled pivot row of A, of I, pivot column}, filled by g_gj_pivot
template <typename T>
__device__ __forceinline__ void g_gj_pivot(int n, int piv, int c, const T* A, const T* I, T* sc) {
    const T pinv = (T)1 / A[piv + piv * n];
    sc[c] = A[piv + c * n] * pinv;
    sc[n + c] = I[piv + c * n] * pinv;
    sc[2 * n + c] = A[c + piv * n];
}
template <typename T>
__device__ __forceinline__ void g_gj_update(const Lane l, int n, int piv, T* A, T* I, const T* sc) {
    const T f = sc[2 * n + l.r];
    for (int c = l.c0; c < n; c += l.cs) {
        const int e = l.r + c * n;
        if (l.r == piv) { A[e] = sc[c]; I[e] = sc[n + c]; }
        else { A[e] -= f * sc[c]; I[e] -= f * sc[n + c]; }
    }
}
// Gauss-Jordan on [A | I] without pivoting: A destroyed, Ainv out.  scr: 3 n.  Ends on a barrier.
template <typename T>
__device__ __forceinline__ void g_invert(const Lane l, int n, T* A, T* Ainv, T* scr) {
    for (int e = threadIdx.x; e < n * n; e += blockDim.x) Ainv[e] = (T)0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) Ainv[i + i * n] = (T)1;
    __syncthreads();
    for (int piv = 0; piv < n; ++piv) {
        for (int c = threadIdx.x; c < n; c += blockDim.x) g_gj_pivot(n, piv, c, A, Ainv, scr);
        __syncthreads();
        g_gj_update(l, n, piv, A, Ainv, scr);
        __syncthreads();
    }
}
// The three inversions of a block row (Q_k, Q_{k+1}: n x n; R_k: m x m, m <= n) advanced in lock-step (the reference inverts them together too:
// invertMatrix<T>(dimA, dimB, dimC, ...), include/utils/matrix.cuh): the arithmetic of three g_invert calls per element, a third of the barriers.  m = n is the boundary case (every pivot step touches all three).
// scr: 3 (2 n + m).  Ends on a barrier.
template <typename T>
__device__ __forceinline__ void g_invert3(const Lane ln, const Lane lm, int n, T* A1, T* I1, T* A2, T* I2, int m, T* A3, T* I3, T* scr) {
    const int nn = n * n, mm = m * m;
    for (int e = threadIdx.x; e < 2 * nn + mm; e += blockDim.x) {
        if (e < nn) I1[e] = (T)0;
        else if (e < 2 * nn) I2[e - nn] = (T)0;
        else I3[e - 2 * nn] = (T)0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * n + m; i += blockDim.x) {
        if (i < n) I1[i + i * n] = (T)1;
        else if (i < 2 * n) I2[(i - n) + (i - n) * n] = (T)1;
        else I3[(i - 2 * n) + (i - 2 * n) * m] = (T)1;
    }
    __syncthreads();
    T* s1 = scr;
    T* s2 = s1 + 3 * n;
    T* s3 = s2 + 3 * n;
    for (int piv = 0; piv < n; ++piv) {
        for (int c = threadIdx.x; c < 2 * n + m; c += blockDim.x) {
            if (c < n) g_gj_pivot(n, piv, c, A1, I1, s1);
            else if (c < 2 * n) g_gj_pivot(n, piv, c - n, A2, I2, s2);
            else if (piv < m) g_gj_pivot(m, piv, c - 2 * n, A3, I3, s3);
        }
        __syncthreads();
        g_gj_update(ln, n, piv, A1, I1, s1);
        g_gj_update(ln, n, piv, A2, I2, s2);
        if (piv < m) g_gj_update(lm, m, piv, A3, I3, s3);
        __syncthreads();
    }
}

// LDS working set of the formation kernel in elements: Qk Qki Qp Qpi Ak phi (n x n), Bk BR (n x m), Rk Rki (m x m), six n-vectors
// (gam v1 v2 qk qp + one spare), rk, the Gauss-Jordan scratch 3 (2 n + m).  theta, theta^-1 and phi^T reuse the blocks the inversions destroyed.
__host__ __device__ constexpr size_t form_lds_elems(int n, int m) {
    return (size_t)6 * n * n + (size_t)2 * n * m + (size_t)2 * m * m + (size_t)6 * n + m + (size_t)3 * (2 * n + m);
}
__host__ __device__ constexpr size_t complete_lds_elems(int n) { return (size_t)6 * n * n; }

// block row k of trajectory b: S[k,0], S[k,1], S[k-1,2], Pinv[k,1], gamma[k]; inverses -> staging buffer (linsys_setup.cuh:139-562)
// A: SchurArgsT<T> (one rho per call) or SchurArgsVT<T> (one per trajectory) — the same body, rho read through rho_of
template <typename T, typename A = SchurArgsT<T>>
__global__ __launch_bounds__(256) void form_schur_kernel(A a) {
    extern __shared__ __align__(16) unsigned char gen_smem[];
    T* sm = reinterpret_cast<T*>(gen_smem);
    const int n = a.n, m = a.m, N = a.N;
    const int nn = n * n, mm = m * m, nm = n * m;
    const int Gset = nn + mm, Cset = nn + nm, gset = n + m;
    const size_t Gsz = (size_t)Gset * N - mm, Csz = (size_t)Cset * (N - 1), gsz = (size_t)gset * N - m;
    T *Qk = sm, *Qki = Qk + nn, *Qp = Qki + nn, *Qpi = Qp + nn, *Ak = Qpi + nn, *phi = Ak + nn, *Bk = phi + nn, *BR = Bk + nm,
      *Rk = BR + nm, *Rki = Rk + mm, *gam = Rki + mm, *v1 = gam + n, *v2 = v1 + n, *qk = v2 + n, *qp = qk + n, *rk = qp + 2 * n, *scr = rk + m;
    T *theta = Qk, *thetaInv = Qp, *phiT = Ak;               // (free once the inversions / the theta products are through)
    const int nt = blockDim.x, tid = threadIdx.x;
    const Lane ln = lane_of(n), lm = lane_of(m);

    for (long item = blockIdx.x; item < (long)a.batch * N; item += gridDim.x) {
        const int b = (int)(item / N), k = (int)(item % N);
        const T* G = a.G + (size_t)b * Gsz;
        const T* C = a.C + (size_t)b * Csz;
        const T* g = a.g + (size_t)b * gsz;
        const T* c = a.c + (size_t)b * n * N;
        T* S = a.S + (size_t)b * 3 * nn * N;
        T* P = a.Pinv + (size_t)b * 3 * nn * N;
        T* gamma = a.gamma + (size_t)b * n * N;
        T* Gs = a.Ginv_scratch + (size_t)b * Gsz;
        const T rho = rho_of(a, b);
        __syncthreads();
        if (k == 0) {
            g_copy(nn, G, Qk);
            g_copy(n, g, qk);
            __syncthreads();
            for (int i = tid; i < n; i += nt) Qk[i + i * n] += rho;
            __syncthreads();
            if (a.pinv) g_copy(nn, Qk, P + nn, (T)-1);                   // Pinv[0,1] = -(Q0 + rho I)
            __syncthreads();
            g_invert(ln, n, Qk, Qki, scr);
            g_copy(nn, Qki, S + nn, (T)-1);                              // S[0,1] = -Q0^-1
            g_matvec(n, n, Qki, qk, v1);
            __syncthreads();
            for (int i = tid; i < n; i += nt) gamma[i] = -v1[i];
            continue;
        }
        g_copy(nn, C + (size_t)(k - 1) * Cset, Ak);
        g_copy(nm, C + (size_t)(k - 1) * Cset + nn, Bk);
        g_copy(nn, G + (size_t)(k - 1) * Gset, Qk);
        g_copy(mm, G + (size_t)(k - 1) * Gset + nn, Rk);
        g_copy(nn, G + (size_t)k * Gset, Qp);
        g_copy(n, g + (size_t)(k - 1) * gset, qk);
        g_copy(m, g + (size_t)(k - 1) * gset + n, rk);
        g_copy(n, g + (size_t)k * gset, qp);
        __syncthreads();
        for (int i = tid; i < n; i += nt) { Qk[i + i * n] += rho; Qp[i + i * n] += rho; }
        for (int i = tid; i < m; i += nt) Rk[i + i * m] += rho;
        __syncthreads();
        g_invert3(ln, lm, n, Qk, Qki, Qp, Qpi, m, Rk, Rki, scr);
        g_gemm<false>(ln, n, n, n, Ak, Qki, phi);                        // phi = Abar Qi
        g_gemm<false>(ln, n, m, m, Bk, Rki, BR);                         // Bbar Ri
        g_matvec(n, n, Qpi, qp, gam);
        __syncthreads();
        for (int i = tid; i < n; i += nt) gam[i] -= c[(size_t)k * n + i];
        g_matvec(n, n, phi, qk, v1);
        g_matvec(n, m, BR, rk, v2);
        __syncthreads();
        for (int i = tid; i < n; i += nt) gam[i] += v2[i] + v1[i];
        // theta = phi Abar^T, += Qpi, += (Bbar Ri) Bbar^T: one thread owns element (r, c) of all three terms, so the two products stay in
        // registers; S[k,0] = -phi and S[k,1] = -theta leave from here (theta itself lands in the block the inversion of Q_k destroyed)
        {
            T* S0 = S + (size_t)k * 3 * nn;
            for (int cc = ln.c0; cc < n; cc += ln.cs) {
                T acc = 0, acc2 = 0;
#pragma unroll 4
                for (int t = 0; t < n; ++t) acc += phi[ln.r + t * n] * Ak[cc + t * n];
#pragma unroll 4
                for (int t = 0; t < m; ++t) acc2 += BR[ln.r + t * n] * Bk[cc + t * n];
                const int e = ln.r + cc * n;
                T th = acc;
                th += Qpi[e];
                th += acc2;
                theta[e] = th;
                S0[e] = phi[e] * (T)-1;
                S0[nn + e] = th * (T)-1;
            }
        }
        __syncthreads();
        for (int q = ln.c0; q < n; q += ln.cs) {                           // phi^T, columns skewed by the row
            int j = q + ln.r;
            if (j >= n) j -= n;
            phiT[ln.r + j * n] = phi[j + ln.r * n];
        }
        for (int i = tid; i < n; i += nt) gamma[(size_t)k * n + i] = -gam[i];
        g_copy(nn, Qki, Gs + (size_t)(k - 1) * Gset);                    // G <- G^-1 (via the staging buffer)
        g_copy(mm, Rki, Gs + (size_t)(k - 1) * Gset + nn);
        if (k == N - 1) g_copy(nn, Qpi, Gs + (size_t)k * Gset);
        __syncthreads();
        g_copy(nn, phiT, S + (size_t)(k - 1) * 3 * nn + 2 * nn, (T)-1);   // S[k-1,2] = -phi^T
        if (a.pinv) {
            g_invert(ln, n, theta, thetaInv, scr);
            g_copy(nn, thetaInv, P + (size_t)k * 3 * nn + nn, (T)-1);     // Pinv[k,1]
        }
    }
}

// symmetric-stair completion + publication of G^-1 (linsys_setup.cuh:9-137).  phi_{k+1}^T enters its product as the
// transposed operand (B stored k x n): the same sums in the same order as a transposed load followed by a plain product.
template <typename T>
__global__ __launch_bounds__(256) void complete_ss_kernel(SchurArgsT<T> a) {
    extern __shared__ __align__(16) unsigned char gen_smem[];
    T* sm = reinterpret_cast<T*>(gen_smem);
    const int n = a.n, m = a.m, N = a.N, nn = n * n, mm = m * m;
    const int Gset = nn + mm;
    const size_t Gsz = (size_t)Gset * N - mm;
    T *Dk = sm, *Dm = Dk + nn, *Dp = Dm + nn, *L = Dp + nn, *Rn = L + nn, *t1 = Rn + nn;
    const Lane ln = lane_of(n);
    for (long item = blockIdx.x; item < (long)a.batch * N; item += gridDim.x) {
        const int b = (int)(item / N), k = (int)(item % N);
        const T* S = a.S + (size_t)b * 3 * nn * N;
        T* P = a.Pinv + (size_t)b * 3 * nn * N;
        const int cnt = (k < N - 1) ? Gset : nn;
        g_copy(cnt, a.Ginv_scratch + (size_t)b * Gsz + (size_t)k * Gset, a.Ginv_out + (size_t)b * Gsz + (size_t)k * Gset);
        if (!a.ss) continue;
        __syncthreads();
        g_copy(nn, P + (size_t)k * 3 * nn + nn, Dk);
        if (k > 0) {
            g_copy(nn, S + (size_t)k * 3 * nn, L);
            g_copy(nn, P + (size_t)(k - 1) * 3 * nn + nn, Dm);
        }
        if (k < N - 1) {
            g_copy(nn, S + (size_t)(k + 1) * 3 * nn, Rn);                // phi_{k+1} as stored
            g_copy(nn, P + (size_t)(k + 1) * 3 * nn + nn, Dp);
        }
        __syncthreads();
        if (k > 0) {
            g_gemm<false>(ln, n, n, n, Dk, L, t1);
            __syncthreads();
            g_gemm<false>(ln, n, n, n, t1, Dm, P + (size_t)k * 3 * nn, (T)-1);              // Pinv[k,0]
            __syncthreads();
        }
        if (k < N - 1) {
            g_gemm<true>(ln, n, n, n, Dk, Rn, t1);
            __syncthreads();
            g_gemm<false>(ln, n, n, n, t1, Dp, P + (size_t)k * 3 * nn + 2 * nn, (T)-1);     // Pinv[k,2]
        }
    }
}

// dz recovery (include/common/dz.cuh:3-121: dz_x = Qi (q - lambda_k - Abar^T lambda_{k+1}), dz_u = Ri (r - Bbar^T lambda_{k+1})): one lane per element of dz_k, blockDim.x / (n + m) knots per workgroup
// (every output is one sequential inner product, so a knot cannot use more than n + m lanes).  blockDim.x >= n + m.
template <typename T>
__global__ __launch_bounds__(128) void compute_dz_kernel(DzArgsT<T> a) {
    __shared__ T sm[128];
    const int n = a.n, m = a.m, N = a.N, nn = n * n, mm = m * m, nm = n * m, w = n + m;
    const size_t Gsz = (size_t)(nn + mm) * N - mm, Csz = (size_t)(nn + nm) * (N - 1), gsz = (size_t)w * N - m;
    const int kpw = (int)blockDim.x / w;                                  // knots per workgroup
    const int slot = (int)threadIdx.x / w, i = (int)threadIdx.x % w;
    T* tv = sm + slot * w;                                                // [0, n): state part, [n, n + m): control part
    const long total = (long)a.batch * N, groups = (total + kpw - 1) / kpw;
    for (long grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const long item = grp * kpw + slot;
        const bool live = slot < kpw && item < total;
        const int b = live ? (int)(item / N) : 0, k = live ? (int)(item % N) : 0;
        const T* Qi = a.Ginv + (size_t)b * Gsz + (size_t)k * (nn + mm);
        const T* Ck = a.C + (size_t)b * Csz + (size_t)k * (nn + nm);
        const T* gk = a.g + (size_t)b * gsz + (size_t)k * w;
        const T* lam = a.lambda + (size_t)b * n * N;
        T* dz = a.dz + (size_t)b * gsz + (size_t)k * w;
        const bool ctl = i >= n;                                          // control rows exist for k < N - 1 only
        const bool on = live && (!ctl || k != N - 1);
        __syncthreads();
        if (on) {
            T acc = 0;
            if (k != N - 1) {
                const T* col = Ck + (size_t)i * n;                        // column i of [Abar | Bbar]
                const T* ln = lam + (size_t)(k + 1) * n;
                for (int t = 0; t < n; ++t) acc += col[t] * ln[t];
            }
            tv[i] = ctl ? gk[i] - acc : gk[i] - (lam[(size_t)k * n + i] + acc);
        }
        __syncthreads();
        if (on) {
            T acc = 0;
            if (!ctl) for (int c = 0; c < n; ++c) acc += Qi[i + c * n] * tv[c];
            else for (int c = 0; c < m; ++c) acc += Qi[nn + (i - n) + c * m] * tv[n + c];
            dz[i] = acc;
        }
    }
}

// Block-tridiagonal direct solve for any n (bt_block_solve_kernel of block_solve.hip.h): one workgroup per trajectory, serial in the
// knot index.  Delta_k, [U_k | y_k] (double-buffered: the eliminated block is W_k, the next knot's operand), L_k in LDS; the L W product
// stays in registers (thread (r, c) owns Delta(r, c)).  W_k, z_k -> work for the back substitution.
//   Delta_0 = D_0, y_0 = gamma_0;  k >= 1: Delta_k = D_k - L_k W_{k-1}, y_k = gamma_k - L_k z_{k-1};  [Delta_k | U_k y_k] -> [I | W_k z_k] by one
//   Gauss-Jordan elimination (columns at or left of the pivot untouched);  lambda_{N-1} = z_{N-1}, lambda_k = z_k - W_k lambda_{k+1}.
// T: the type of the sweep (operands in LDS, work); ST: the storage type of S, gamma and lambda — T itself, or float under T = double: widened
// on load (exact), lambda rounded once on store ("block_solve_f64" = 1).  LDS: block_solve_lds_elems(n) x sizeof(T).
template <typename T, typename ST = T>
struct BlockSolveGenArgsT {
    const ST* S; const ST* gamma; ST* lambda; T* work;                    // work: [batch][N][n * n + n]
    int n; int N; int batch;
};
typedef BlockSolveGenArgsT<float> BlockSolveGenArgs;
__host__ __device__ constexpr size_t block_solve_lds_elems(int n) { return (size_t)4 * n * n + (size_t)5 * n + 4; }

template <typename T, typename ST>
__device__ __forceinline__ void g_widen(int cnt, const ST* src, T* dst) {
    for (int e = threadIdx.x; e < cnt; e += blockDim.x) dst[e] = (T)src[e];
}

template <typename T, typename ST = T>
__global__ __launch_bounds__(256) void bt_block_solve_kernel(BlockSolveGenArgsT<T, ST> a) {
    extern __shared__ __align__(16) unsigned char gen_smem[];
    T* sm = reinterpret_cast<T*>(gen_smem);
    const int n = a.n, N = a.N, nn = n * n, WS = nn + n;
    T *Delta = sm, *Lb = Delta + nn, *cur = Lb + nn, *prev = cur + nn, *y = prev + nn, *zp = y + n, *prowD = zp + n, *prowB = prowD + n,
      *pcol = prowB + n, *py = pcol + n;
    const int nt = blockDim.x, tid = threadIdx.x;
    const Lane ln = lane_of(n);
    for (long b = blockIdx.x; b < a.batch; b += gridDim.x) {
        const ST* S = a.S + (size_t)b * 3 * nn * N;
        const ST* gamma = a.gamma + (size_t)b * n * N;
        ST* lambda = a.lambda + (size_t)b * n * N;
        T* work = a.work + (size_t)b * N * WS;
        for (int k = 0; k < N; ++k) {
            const ST* blk = S + (size_t)k * 3 * nn;
            __syncthreads();
            g_widen(nn, blk + nn, Delta);
            if (k < N - 1) g_widen(nn, blk + 2 * nn, cur);
            else for (int e = tid; e < nn; e += nt) cur[e] = (T)0;          // the last block row carries y only
            if (k > 0) g_widen(nn, blk, Lb);
            for (int i = tid; i < n; i += nt) y[i] = (T)gamma[(size_t)k * n + i];
            __syncthreads();
            if (k > 0) {
                for (int c = ln.c0; c < n; c += ln.cs) {                   // Delta = D - L W_{k-1}
                    T acc = 0;
#pragma unroll 4
                    for (int t = 0; t < n; ++t) acc += Lb[ln.r + t * n] * prev[t + c * n];
                    const int e = ln.r + c * n;
                    Delta[e] = Delta[e] - acc;
                }
                for (int r = tid; r < n; r += nt) {                        // y -= L z_{k-1}
                    T acc = 0;
                    for (int c = 0; c < n; ++c) acc += Lb[r + c * n] * zp[c];
                    y[r] = y[r] - acc;
                }
                __syncthreads();
            }
            for (int piv = 0; piv < n; ++piv) {
                const int right = n - piv - 1;                             // columns of Delta still alive
                for (int c = tid; c < n; c += nt) {
                    const T pinv = (T)1 / Delta[piv + piv * n];
                    if (c > piv) prowD[c] = Delta[piv + c * n] * pinv;
                    prowB[c] = cur[piv + c * n] * pinv;
                    pcol[c] = Delta[c + piv * n];
                    if (c == 0) py[0] = y[piv] * pinv;
                }
                __syncthreads();
                const T f = pcol[ln.r];
                const bool isp = ln.r == piv;
                for (int cc = ln.c0; cc < right + n + 1; cc += ln.cs) {
                    if (cc < right) {
                        const int c = piv + 1 + cc, e = ln.r + c * n;
                        Delta[e] = isp ? prowD[c] : Delta[e] - f * prowD[c];
                    } else if (cc < right + n) {
                        const int c = cc - right, e = ln.r + c * n;
                        cur[e] = isp ? prowB[c] : cur[e] - f * prowB[c];
                    } else {
                        y[ln.r] = isp ? py[0] : y[ln.r] - f * py[0];
                    }
                }
                __syncthreads();
            }
            for (int i = tid; i < n; i += nt) { const T z = y[i]; work[(size_t)k * WS + nn + i] = z; zp[i] = z; }
            if (k < N - 1) g_copy(nn, cur, work + (size_t)k * WS);
            T* sw = cur; cur = prev; prev = sw;
        }
        // back substitution: lambda_{N-1} = z_{N-1} (still in zp); W_k staged through LDS by the whole workgroup, one lane per row
        T *la = y, *lb = prowD;
        __syncthreads();
        for (int i = tid; i < n; i += nt) { la[i] = zp[i]; lambda[(size_t)(N - 1) * n + i] = (ST)zp[i]; }
        for (int k = N - 2; k >= 0; --k) {
            g_copy(nn, work + (size_t)k * WS, Lb);
            __syncthreads();
            for (int r = tid; r < n; r += nt) {
                T acc = 0;
                for (int c = 0; c < n; ++c) acc += Lb[r + c * n] * la[c];
                const T v = work[(size_t)k * WS + nn + r] - acc;
                lb[r] = v;
                lambda[(size_t)k * n + r] = (ST)v;
            }
            __syncthreads();
            T* sw = la; la = lb; lb = sw;
        }
    }
}

#pragma clang fp contract(fast)

}  // namespace gen
}  // namespace mpcg
