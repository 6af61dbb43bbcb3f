// dpp_rows.hip.h — rows-in-lanes primitives on 16-lane DPP rows (gfx950): four independent problems per wavefront, lane r < 14 of a
// row holds ROW r of every 14x14 operand in registers, and what another row needs from row t of an operand is a `row_newbcast:t` DPP source
// modifier on the multiply (verified on the chip: tools/_prof/dpp_probe.hip).  Used by the block-tridiagonal direct solver
// (block_solve.hip.h), in float and in double; what the two differ in is the section "float and double rows" below, which
// schur_walk.hip.h uses too.  (Rounds 2-3 ran the Schur formation on these as well; round 4's formation, schur_walk.hip.h, has its own
// column-pair versions in float.)
//
// Contraction is OFF: every a*b+c is a rounded multiply followed by a rounded add, sequential over the contracted index, accumulators
// starting at +0 — the C oracle's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace mpcg {

#pragma clang fp contract(off)

namespace sdpp {

// ---- float and double rows: the broadcast, a * bc(b), the wavefront-wide permute and the hazard idioms only double needs ----
// value held by lane L of this lane's 16-lane row.  float: a DPP source modifier once the compiler folds it into the reader.
template <int L>
__device__ __forceinline__ float rbc(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x150 + L, 0xf, 0xf, true));
}
// double: `v_mov_b64_dpp ... row_newbcast:L`, the only DPP control 64-bit operations have.  The compiler does not produce it (it splits a
// 64-bit broadcast into two v_mov_b32_dpp), so it is assembler text, and the DPP read-after-VALU-write hazard is ours to keep: SW64_SETTLE().
template <int L>
__device__ __forceinline__ double rbc(double v) {
    double r;
    asm("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(L));
    return r;
}
// a * (b held by lane L of this lane's 16-lane row), a rounded multiply.  (gfx950 has DPP forms of v_mov_b64 and v_fmac_f64 only —
// v_mul_f64 / v_add_f64 are VOP3 — and the fused multiply-add is not what the oracle computes.)
template <int L, typename T>
__device__ __forceinline__ T mulbc(T a, T b) {
    return a * rbc<L>(b);
}
// value held by lane `addr / 4` of the wavefront: one ds_bpermute in float, two 32-bit halves in double
__device__ __forceinline__ float bperm(int addr, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double bperm(int addr, double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}
// phase boundary: the scheduler may not move instructions across it
#define SW_FENCE() __builtin_amdgcn_sched_barrier(0)
// Two wait states between the last VALU write of an operand and its first DPP read: nothing is scheduled across this point, and the s_nop 1
// stands between whatever wrote the operands before it and the DPP multiplies behind it (verified on the built code: tools/check_dpp_hazards.py).
#define SW64_SETTLE() do { SW_FENCE(); asm volatile("s_nop 1"); SW_FENCE(); } while (0)
// The same three idioms for code written once for both types: nothing in float, where the compiler owns the DPP modifier and its hazard.
template <typename T>
__device__ __forceinline__ void sched_fence() {
    if constexpr (std::is_same<T, double>::value) SW_FENCE();
}
template <typename T>
__device__ __forceinline__ void settle() {
    if constexpr (std::is_same<T, double>::value) SW64_SETTLE();
}
// keeps the VALU write of v in front of this point (the launder idiom of schur_walk.hip.h)
template <typename T>
__device__ __forceinline__ void pin(T& v) {
    if constexpr (std::is_same<T, double>::value) asm volatile("" : "+v"(v));
}

// acc += a * (b held by lane L of this 16-lane row): rounded multiply through the DPP source modifier, rounded add
template <int L>
__device__ __forceinline__ void mac_bc(float& acc, float a, float b) {
    const float p = a * rbc<L>(b);
    acc = acc + p;
}

template <int I, int E>
struct SFor {
    template <class F>
    static __device__ __forceinline__ void run(F&& f) {
        f(std::integral_constant<int, I>{});
        SFor<I + 1, E>::run(f);
    }
};
template <int E>
struct SFor<E, E> {
    template <class F>
    static __device__ __forceinline__ void run(F&&) {}
};

// C[r][c] = sum_t A[r][t] * B[t][c]      A: NI columns per lane, B: rows in lanes 0..NI-1, NC columns
template <int NI, int NC>
__device__ __forceinline__ void gemm_nn(const float (&A)[NI], const float (&B)[NC], float (&Cm)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) Cm[c] = 0.f;
    SFor<0, NI>::run([&](auto tc) {
        constexpr int T = decltype(tc)::value;
#pragma unroll
        for (int c = 0; c < NC; ++c) mac_bc<T>(Cm[c], A[T], B[c]);
    });
}
// out[r] = sum_c M[r][c] * v[c]          v: element c in lane c
template <int NC, typename T>
__device__ __forceinline__ T matvec(const T (&M)[NC], T v) {
    settle<T>();
    T acc = 0;
    SFor<0, NC>::run([&](auto cc) {
        constexpr int Cc = decltype(cc)::value;
        acc = acc + mulbc<Cc>(M[Cc], v);
    });
    return acc;
}

// Gauss-Jordan elimination of [A | R] -> [I | A^-1 R] without pivoting, rows in lanes 0..NN-1, NR right-hand
// columns.  Columns of A at or left of the pivot are not touched (they are unit columns afterwards by construction
// and nobody reads them): 4 (NN - 1 - p + NR) instructions for pivot p.  A is destroyed.
template <int NN, int NR>
__device__ __forceinline__ void solve_aug(float (&A)[NN], float (&R)[NR], int lr) {
    SFor<0, NN>::run([&](auto pc) {
        constexpr int P = decltype(pc)::value;
        const float pinv = 1.0f / rbc<P>(A[P]);
        const float pcol = A[P];
        const bool is_p = lr == P;
#pragma unroll
        for (int c = P + 1; c < NN; ++c) {
            const float pa = A[c] * pinv;
            const float ta = pcol * rbc<P>(pa);
            const float na = A[c] - ta;
            A[c] = is_p ? pa : na;
        }
#pragma unroll
        for (int c = 0; c < NR; ++c) {
            const float pr = R[c] * pinv;
            const float tr = pcol * rbc<P>(pr);
            const float nr = R[c] - tr;
            R[c] = is_p ? pr : nr;
        }
    });
}

// row lr of a column-major rows x cols matrix
// (always loads — from a clamped, in-bounds row — and selects afterwards: a per-row condition around the loads
//  turns into divergent branches with the whole operand array parked in scratch)
template <int COLS>
__device__ __forceinline__ void load_rows(float (&M)[COLS], const float* base, int rows, int lr, bool on) {
    const int lrc = lr < rows ? lr : rows - 1;
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        const float v = base[lrc + c * rows];
        M[c] = on ? v : 0.f;
    }
}
template <int COLS>
__device__ __forceinline__ void store_rows(const float (&M)[COLS], float* base, int rows, int lr, bool on, float mult) {
    if (on) {
#pragma unroll
        for (int c = 0; c < COLS; ++c) base[lr + c * rows] = M[c] * mult;
    }
}

}  // namespace sdpp

#pragma clang fp contract(fast)

}  // namespace mpcg
