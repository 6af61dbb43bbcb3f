// schur_walk.hip.h — the Schur + preconditioner formation as ONE pass over the KKT blocks, and the dz recovery on
// the same rows-in-lanes primitives (row 3); float (round 4) and linsys_t = double (round 5: USE_DOUBLES = 1,
// include/common/settings.cuh:41-49) from one text.  gfx950.
//
// What it replaces, and why.  Round 3 ran the formation as three kernels (invert G in place | block rows from the inverses | symmetric-stair
// completion): 12.5 KB of HBM traffic per knot against 8.0 KB algorithmic (every inverse and every theta^-1 went out to memory and came
// back two or three times) and ~3,850 VALU instructions per four knots.  Here a 16-lane DPP row WALKS a chunk of consecutive block rows of
// one trajectory and carries what the next row needs in registers — (Q_{k-1} + rho I)^-1 and theta_{k-1}^-1 — so that
//   * every Q and every R is inverted once, every theta once; G^-1 is written once, in place (no staging copy);
//   * the symmetric-stair couplings Pinv[k,0] and Pinv[k-1,2] are formed from the registers that hold theta_k^-1, phi_k, theta_{k-1}^-1
//     (the round-3 completion kernel re-read three Pinv and two S blocks per knot);
//   * what is left for a second, small kernel (schur_seam_kernel) is the seam between two chunks: the two coupling blocks that need the
//     theta^-1 of both sides, and the one Q^-1 per chunk that cannot be stored in place because the neighbouring chunk still reads the raw Q.
// Same arithmetic, operation for operation, as linsys_setup.cuh:139-562 and :9-137 (every product a rounded multiply followed by a rounded
// add, sequential over the contracted index, accumulators starting at +0; Gauss-Jordan without pivoting, matrix.cuh:120-238) — the C
// oracle's bits in its float and in its double instantiation; tests/test_gpu_schur.py and tests/test_gpu_f64.py compare bits.
//
// The kernels are templates over the element type T; the primitives under them are overloads of one name set, selected by the operand
// type Rows<T, NC>.
//
// Float: instruction diet of the primitives (the kernels are VALU-issue bound, not HBM bound, once the traffic is down):
//   * operands live as PAIRS of neighbouring columns (float2 in an even-aligned register pair): the rounded add of a product term is one
//     v_pk_add_f32 for two columns (the multiply keeps its DPP row-broadcast source, which packed instructions do not have):
//     1.5 instead of 2 VALU instructions per multiply-add;
//   * Gauss-Jordan: the pivot row is scaled by a per-lane multiplier (1 / pivot in the pivot lane, 1.0 elsewhere), every other row then
//     adds (-pcol) x (pivot row entry); the pivot lane runs the same instruction with +0.0 as
//     its multiplier, and x + (+0 * x) has the bits of x for every finite x including both zeros — so there is no per-element select:
//     2 instead of 4 VALU instructions per element and pivot step.
// Double: what differs from float:
//   * a 64-bit operand is broadcast inside its row by `v_mov_b64_dpp ... row_newbcast:t` (the only DPP control 64-bit operations have; the
//     compiler does not produce it — it splits a 64-bit broadcast into two v_mov_b32_dpp — so it is written as assembler text, and the DPP read-after-VALU-write hazard, two wait states, is ours to keep: SW64_SETTLE() puts one s_nop 1
//     between the writers of a to-be-broadcast operand and its DPP readers; tools/check_dpp_hazards.py verifies the built code);
//   * no DPP source modifier on the 64-bit multiply and no packed 64-bit add: 3 VALU instructions per multiply-add (float: 1.5);
//   * operands take two registers each: one wavefront per SIMD (launch bound 1: up to 512 registers, the upper 256 as AGPR spill space).
//
// Round 4 chose the float build among A/B variants that were compile-time switches of this file: operands requested one row ahead
// (against: at the end of the row), Q and R inverted one after the other (against: advanced together, two dependency chains), the pivot
// scaled by recip_ieee (against: the compiler's division under an EXEC mask), stores through the LDS stage (against: 14 dword stores per
// block), plain cache policy on the stores (against: nt), launch bound 2; and timed builds with the stores, the loads, the Gauss-Jordan
// or the products compiled out.  What they measured is in profiles/r04_walk_store_side.txt, r04_ab_walk_io.txt and
// r04_ab_walk_compute.txt; the switch code is in the git history of this file.  Only the chosen arms are left.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "schur_generic.hip.h"
#include "dpp_rows.hip.h"

namespace mpcg {
namespace sw {

#pragma clang fp contract(off)

typedef float f2 __attribute__((ext_vector_type(2)));

// value held by lane L of this lane's 16-lane row; a * (b held by lane L), SW_FENCE() and SW64_SETTLE(): dpp_rows.hip.h, shared with the
// direct solve.  (SW_FENCE: a phase boundary the scheduler may not move instructions across — left alone it interleaves the independent
// inversions and products of a block row for latency, which needs more than 256 registers.)
using sdpp::rbc;
using sdpp::mulbc;
using sdpp::SFor;

constexpr int np(int nc) { return (nc + 1) / 2; }
// NC columns of an operand, one row per lane: column pairs in float, plain columns in double
template <typename T, int NC>
using Rows = std::conditional_t<std::is_same<T, float>::value, f2[np(NC)], double[NC]>;
// column i of an operand kept as column pairs
#define SW_EL(X, i) (((i) & 1) ? (X)[(i) >> 1].y : (X)[(i) >> 1].x)

// acc(pair) += (t0, t1); the empty asm keeps the two multiplies scalar (v_mul_f32_dpp): left alone, the vectoriser turns them into
// 2 x v_mov_b32_dpp + v_pk_mul_f32.
__device__ __forceinline__ void acc2(f2& acc, float t0, float t1) {
    asm("" : "+v"(t0), "+v"(t1));
    acc = acc + f2{t0, t1};
}

// A private copy of a broadcast operand that the optimiser cannot identify with the original.  Two products that broadcast the same
// entries of the same operand (Dk L and Dm L^T below) otherwise share ONE v_mov_b32_dpp per entry, kept alive from the first product to
// the second — 196 registers (double: one v_mov_b64_dpp per entry, 392); a broadcast with a single use folds into its multiply
// (v_mul_f32_dpp) and costs no register at all.
template <int NPAIR>
__device__ __forceinline__ void launder(f2 (&D)[NPAIR], const f2 (&Src)[NPAIR]) {
#pragma unroll
    for (int j = 0; j < NPAIR; ++j) { D[j] = Src[j]; asm volatile("" : "+v"(D[j])); }
}
template <int NC>
__device__ __forceinline__ void launder(double (&D)[NC], const double (&Src)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) { D[c] = Src[c]; asm volatile("" : "+v"(D[c])); }
}

// An ordering point for the scheduler: everything that produces `acc` is finished before anything that consumes `a` starts.  Left
// alone, the scheduler (which sees a 256-register budget) likes to issue ALL 196 multiplies of a product first and the adds afterwards —
// 196 live products, spilled — whenever the code around the product changes a little; which products it did that to changed from build to
// build.
template <int NPAIR>
__device__ __forceinline__ void pin(float& a, f2 (&acc)[NPAIR]) {
    if constexpr (NPAIR == 7) asm volatile("" : "+v"(a), "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]));
    else if constexpr (NPAIR == 4) asm volatile("" : "+v"(a), "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
    else static_assert(NPAIR == 7 || NPAIR == 4, "7 or 4 column pairs");
}

// C[r][c] = sum_t A[r][t] * B[t][c]      A: NI columns per lane; B: rows in lanes 0..NI-1, NC columns
template <int NI, int NC>
__device__ __forceinline__ void gemm_nn(const f2 (&A)[np(NI)], const f2 (&Bsrc)[np(NC)], f2 (&Cm)[np(NC)]) {
    f2 B[np(NC)];
    launder(B, Bsrc);
#pragma unroll
    for (int j = 0; j < np(NC); ++j) Cm[j] = f2{0.f, 0.f};
    SFor<0, NI>::run([&](auto tc) {
        constexpr int T = decltype(tc)::value;
        float a = SW_EL(A, T);
        pin(a, Cm);                  // the products of term T start after the sums of term T-1: at most NC products in flight
#pragma unroll
        for (int j = 0; j < np(NC); ++j) {
            const float t0 = a * rbc<T>(B[j].x);
            const float t1 = (2 * j + 1 < NC) ? a * rbc<T>(B[j].y) : 0.f;
            acc2(Cm[j], t0, t1);
        }
    });
}
template <int NI, int NC>
__device__ __forceinline__ void gemm_nn(const double (&A)[NI], const double (&Bsrc)[NC], double (&Cm)[NC]) {
    double B[NC];
    launder(B, Bsrc);
    SW64_SETTLE();
#pragma unroll
    for (int c = 0; c < NC; ++c) Cm[c] = 0.0;
    SFor<0, NI>::run([&](auto tc) {
        constexpr int T = decltype(tc)::value;
        if constexpr (T > 0) SW_FENCE();            // the products of term T start after the sums of term T-1: at most NC products in flight
#pragma unroll
        for (int c = 0; c < NC; ++c) Cm[c] = Cm[c] + mulbc<T>(A[T], B[c]);
    });
}
// C[r][c] = sum_t A[r][t] * Bt[c][t]     Bt: row c in lane c (NC rows), NI columns
template <int NI, int NC>
__device__ __forceinline__ void gemm_nt(const f2 (&A)[np(NI)], const f2 (&Btsrc)[np(NI)], f2 (&Cm)[np(NC)]) {
    f2 Bt[np(NI)];
    launder(Bt, Btsrc);
    SFor<0, np(NC)>::run([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        f2 acc{0.f, 0.f};
        if constexpr (J > 0) {       // column pair J starts after pair J-1 is finished: 2 NI products in flight at most
            float dummy = Cm[J - 1].x;
            pin(dummy, Bt);
            Cm[J - 1].x = dummy;
        }
#pragma unroll
        for (int t = 0; t < NI; ++t) {
            const float a = SW_EL(A, t), b = SW_EL(Bt, t);
            const float t0 = a * rbc<2 * J>(b);
            const float t1 = (2 * J + 1 < NC) ? a * rbc<(2 * J + 1 < 16 ? 2 * J + 1 : 0)>(b) : 0.f;
            acc2(acc, t0, t1);
        }
        Cm[J] = acc;
    });
}
template <int NI, int NC>
__device__ __forceinline__ void gemm_nt(const double (&A)[NI], const double (&Btsrc)[NI], double (&Cm)[NC]) {
    double Bt[NI];
    launder(Bt, Btsrc);
    SW64_SETTLE();
    SFor<0, NC>::run([&](auto cc) {
        constexpr int Cc = decltype(cc)::value;
        if constexpr (Cc > 0 && Cc % 2 == 0) SW_FENCE();        // two columns' chains interleave; the next pair starts after them
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < NI; ++t) acc = acc + mulbc<Cc>(A[t], Bt[t]);
        Cm[Cc] = acc;
    });
}
// out[r] = sum_c M[r][c] * v[c]          v: element c in lane c  (double: sdpp::matvec)
using sdpp::matvec;
template <int NC>
__device__ __forceinline__ float matvec(const f2 (&M)[np(NC)], float v) {
    float acc = 0.f;
    SFor<0, NC>::run([&](auto cc) {
        constexpr int Cc = decltype(cc)::value;
        const float p = SW_EL(M, Cc) * rbc<Cc>(v);
        acc = acc + p;
    });
    return acc;
}
// two of them at once: (M1 v1, M2 v2); float: one packed add per column, double: one after the other
template <int NC>
__device__ __forceinline__ f2 matvec2(const f2 (&M1)[np(NC)], float v1, const f2 (&M2)[np(NC)], float v2) {
    f2 acc{0.f, 0.f};
    SFor<0, NC>::run([&](auto cc) {
        constexpr int Cc = decltype(cc)::value;
        acc2(acc, SW_EL(M1, Cc) * rbc<Cc>(v1), SW_EL(M2, Cc) * rbc<Cc>(v2));
    });
    return acc;
}
struct d2 { double x, y; };
template <int NC>
__device__ __forceinline__ d2 matvec2(const double (&M1)[NC], double v1, const double (&M2)[NC], double v2) {
    const double x = matvec<NC>(M1, v1), y = matvec<NC>(M2, v2);
    return d2{x, y};
}

// 1 / x with the bits of the IEEE division (the oracle divides).  v_rcp_f32 + ONE Newton step reproduces the correctly rounded quotient
// for EVERY float with 2^-100 <= |x| <= 2^100 — checked exhaustively on the chip, all 2^32 bit patterns, tools/_prof/rcp_exhaustive.hip
// (profiles/r04_rcp_exhaustive.txt: 0 mismatches in that range; outside it — denormal quotients, overflow — the short form differs) — 3
// dependent instructions instead of the 11 of the compiler's division sequence, at the head of every pivot step's dependency chain.
// Pivots outside the range (a singular or wildly scaled block) take the division.
__device__ __forceinline__ float recip_ieee(float x, bool wanted) {
    const float r0 = __builtin_amdgcn_rcpf(x);
    const float e = __builtin_fmaf(-x, r0, 1.0f);
    float r = __builtin_fmaf(e, r0, r0);
    const float ax = __builtin_fabsf(x);
    if (__builtin_expect(wanted && !(ax >= 0x1p-100f && ax <= 0x1p100f), 0)) r = 1.0f / x;
    return r;
}

// One pivot step P of the Gauss-Jordan elimination of [A | I] (include/utils/matrix.cuh:120-238; rows in lanes 0..NN-1, lr = lane index
// inside the 16-lane row).  Half of the 2 NN columns are structurally inert at every pivot step and are skipped (columns of A at or left of
// the pivot: finished, never read again; columns of I right of the pivot: still unit columns, the reference's update leaves them as they
// are) — round 3, no bit changed.  Round 4: the pivot row is scaled by a per-lane multiplier (1 / pivot in the pivot lane, exactly 1.0 in
// every other lane: x * 1.0 is x), then every lane adds (-pcol) * (pivot row entry) with +0.0 as the pivot lane's multiplier.
template <int NN, int P>
__device__ __forceinline__ void gj_step(f2 (&A)[np(NN)], f2 (&I)[np(NN)], int lr) {
    constexpr int NP = np(NN);
    constexpr int JP = P / 2;                    // the pair that holds column P
    constexpr bool ODD = P & 1;
    const float app = SW_EL(A, P);               // pivot column entry of this row (the pivot itself in lane P)
    const bool is_p = lr == P;
    const float nmul = is_p ? 0.f : -app;        // x + (+0)(x) keeps the bits of x: the pivot lane needs no select
    const float pinv = recip_ieee(app, is_p);    // (matrix.cuh:146)
    const float mrow = is_p ? pinv : 1.0f;
    // pair JP of A: column P is finished; its neighbour P+1 (P even) is live.  Pair JP of I: column P is live, its neighbour P+1 (P even) is
    // still a unit column and must keep its +0 in the pivot lane.
    if (!ODD && 2 * JP + 1 < NN) A[JP].y = A[JP].y * mrow;
#pragma unroll
    for (int j = JP + 1; j < NP; ++j) A[j] = A[j] * f2{mrow, mrow};
#pragma unroll
    for (int j = 0; j < JP; ++j) I[j] = I[j] * f2{mrow, mrow};
    if (ODD) I[JP] = I[JP] * f2{mrow, mrow};
    else I[JP].x = I[JP].x * mrow;
    // every row: x += (-pcol) * (pivot row entry)
    if (!ODD && 2 * JP + 1 < NN) A[JP].y = A[JP].y + nmul * rbc<P>(A[JP].y);
#pragma unroll
    for (int j = JP + 1; j < NP; ++j) {
        const float t0 = nmul * rbc<P>(A[j].x);
        const float t1 = (2 * j + 1 < NN) ? nmul * rbc<P>(A[j].y) : 0.f;
        acc2(A[j], t0, t1);
    }
#pragma unroll
    for (int j = 0; j < JP; ++j) acc2(I[j], nmul * rbc<P>(I[j].x), nmul * rbc<P>(I[j].y));
    if (ODD) acc2(I[JP], nmul * rbc<P>(I[JP].x), nmul * rbc<P>(I[JP].y));
    else I[JP].x = I[JP].x + nmul * rbc<P>(I[JP].x);
}
// double: the same step on plain columns, the pivot's multiplier the IEEE quotient
template <int NN, int P>
__device__ __forceinline__ void gj_step(double (&A)[NN], double (&I)[NN], int lr) {
    const double app = A[P];
    const bool is_p = lr == P;
    const double nmul = is_p ? 0.0 : -app;
    const double mrow = is_p ? 1.0 / app : 1.0;            // (matrix.cuh:146: the IEEE quotient)
#pragma unroll
    for (int c = P + 1; c < NN; ++c) A[c] = A[c] * mrow;
#pragma unroll
    for (int c = 0; c <= P; ++c) I[c] = I[c] * mrow;
    SW64_SETTLE();
#pragma unroll
    for (int c = P + 1; c < NN; ++c) A[c] = A[c] + mulbc<P>(nmul, A[c]);
#pragma unroll
    for (int c = 0; c <= P; ++c) I[c] = I[c] + mulbc<P>(nmul, I[c]);
    SW_FENCE();
}
template <int NN>
__device__ __forceinline__ void unit_rows(f2 (&I)[np(NN)], int lr) {
#pragma unroll
    for (int j = 0; j < np(NN); ++j) I[j] = f2{lr == 2 * j ? 1.f : 0.f, lr == 2 * j + 1 ? 1.f : 0.f};
}
// A destroyed, I becomes A^-1
template <int NN>
__device__ __forceinline__ void invert(f2 (&A)[np(NN)], f2 (&I)[np(NN)], int lr) {
    unit_rows<NN>(I, lr);
    SFor<0, NN>::run([&](auto pc) { gj_step<NN, decltype(pc)::value>(A, I, lr); });
}
template <int NN>
__device__ __forceinline__ void invert(double (&A)[NN], double (&I)[NN], int lr) {
#pragma unroll
    for (int c = 0; c < NN; ++c) I[c] = lr == c ? 1.0 : 0.0;
    SFor<0, NN>::run([&](auto pc) { gj_step<NN, decltype(pc)::value>(A, I, lr); });
}

// ---- memory: every array goes through a buffer resource (base in SGPRs, ONE 32-bit byte offset per lane and block, column offsets as
// instruction immediates).  With per-lane 64-bit pointers the walking kernel kept ~20 register pairs of addresses alive across its loop and
// spilled.  A lane that must not store is sent to OOB_OFF (the hardware drops the access): no branches around the stores. ----
typedef __amdgpu_buffer_rsrc_t rsrc_t;
constexpr uint32_t SW_OOB = 0x80000000u;
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), /*stride*/ 0, (int)(uint32_t)bytes, 0x00020000);
}
template <typename T>
__device__ __forceinline__ T bld(rsrc_t r, uint32_t off) {
    if constexpr (std::is_same<T, float>::value) return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
    else return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0));
}
__device__ __forceinline__ void bst(rsrc_t r, uint32_t off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)off, 0, 0);
}
__device__ __forceinline__ void bst(rsrc_t r, uint32_t off, double v) {
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), r, (int)off, 0, 0);
}
// row lr of a column-major rows x COLS matrix that starts at byte `off`.  Rows beyond the matrix repeat its last row:
// what those lanes compute stays in those lanes (every broadcast reads a lane below `rows`) and is never stored.
template <int COLS>
__device__ __forceinline__ void load_rows(f2 (&M)[np(COLS)], rsrc_t r, uint32_t off, int rows, int lr) {
    const uint32_t v = off + 4u * (uint32_t)(lr < rows ? lr : rows - 1);
#pragma unroll
    for (int j = 0; j < np(COLS); ++j) {
        M[j].x = bld<float>(r, v + 4u * (uint32_t)(2 * j * rows));
        M[j].y = (2 * j + 1 < COLS) ? bld<float>(r, v + 4u * (uint32_t)((2 * j + 1) * rows)) : 0.f;
    }
}
template <int COLS>
__device__ __forceinline__ void load_rows(double (&M)[COLS], rsrc_t r, uint32_t off, int rows, int lr) {
    const uint32_t v = off + 8u * (uint32_t)(lr < rows ? lr : rows - 1);
#pragma unroll
    for (int c = 0; c < COLS; ++c) M[c] = bld<double>(r, v + 8u * (uint32_t)(c * rows));
}
// the TRANSPOSE of a column-major block with leading dimension NE: lane lr gets column lr of the block (NE contiguous elements)
template <int NE>
__device__ __forceinline__ void load_rows_t(f2 (&M)[np(NE)], rsrc_t r, uint32_t off, int ncols, int lr) {
    const uint32_t v = off + 4u * (uint32_t)NE * (uint32_t)(lr < ncols ? lr : ncols - 1);
#pragma unroll
    for (int j = 0; j < np(NE); ++j) {
        M[j].x = bld<float>(r, v + 8u * j);
        M[j].y = (2 * j + 1 < NE) ? bld<float>(r, v + 8u * j + 4u) : 0.f;
    }
}
template <int NE>
__device__ __forceinline__ void load_rows_t(double (&M)[NE], rsrc_t r, uint32_t off, int ncols, int lr) {
    const uint32_t v = off + 8u * (uint32_t)NE * (uint32_t)(lr < ncols ? lr : ncols - 1);
#pragma unroll
    for (int c = 0; c < NE; ++c) M[c] = bld<double>(r, v + 8u * c);
}
template <int COLS>
__device__ __forceinline__ void store_rows(const f2 (&M)[np(COLS)], rsrc_t r, uint32_t off, int rows, int lr, bool on, float mult) {
    const uint32_t v = on ? off + 4u * (uint32_t)lr : SW_OOB;
#pragma unroll
    for (int j = 0; j < np(COLS); ++j) {
        bst(r, v + 4u * (uint32_t)(2 * j * rows), M[j].x * mult);
        if (2 * j + 1 < COLS) bst(r, v + 4u * (uint32_t)((2 * j + 1) * rows), M[j].y * mult);
    }
}
template <int COLS>
__device__ __forceinline__ void store_rows(const double (&M)[COLS], rsrc_t r, uint32_t off, int rows, int lr, bool on, double mult) {
    const uint32_t v = on ? off + 8u * (uint32_t)lr : SW_OOB;
#pragma unroll
    for (int c = 0; c < COLS; ++c) bst(r, v + 8u * (uint32_t)(c * rows), M[c] * mult);
}
// row lr of M becomes COLUMN lr of the destination block (a transposed store: COLS contiguous elements per lane)
template <int COLS>
__device__ __forceinline__ void store_rows_t(const f2 (&M)[np(COLS)], rsrc_t r, uint32_t off, int lr, bool on, float mult) {
    const uint32_t v = on ? off + 4u * (uint32_t)COLS * (uint32_t)lr : SW_OOB;
#pragma unroll
    for (int j = 0; j < np(COLS); ++j) {
        bst(r, v + 8u * j, M[j].x * mult);
        if (2 * j + 1 < COLS) bst(r, v + 8u * j + 4u, M[j].y * mult);
    }
}
template <int COLS>
__device__ __forceinline__ void store_rows_t(const double (&M)[COLS], rsrc_t r, uint32_t off, int lr, bool on, double mult) {
    const uint32_t v = on ? off + 8u * (uint32_t)COLS * (uint32_t)lr : SW_OOB;
#pragma unroll
    for (int c = 0; c < COLS; ++c) bst(r, v + 8u * c, M[c] * mult);
}
// ---- float: stores through an LDS stage (round 4b).  A block held rows-in-lanes leaves the wavefront as 14 dword stores whose 64 lanes touch four
// 56-byte segments each — 150 store instructions per block row, and the walking kernel turned out to be bound by exactly that: the memory
// pipeline takes them one instruction at a time, later wavefronts queue behind earlier ones, and the next row's loads wait behind them all
// (profiles/r04_ab_walk_io.txt: with the stores compiled out 354 -> 269 us, with all I/O out 265).  So a group writes its block into its slot of
// the wavefront's LDS stage in memory order (14 ds_write_b32, conflict-free), and the WHOLE wavefront then copies each group's slot out in
// 16-byte pieces: 49 lanes x dwordx4 per 14x14 block — 4 store instructions per block (one per group) instead of 14, every one a run of
// 784 contiguous bytes.  The group's destination offset travels to the other lanes as an SGPR (v_readlane -> the store's soffset).
// No barrier: one wavefront per workgroup, LDS operations of a wavefront execute in
// order; the wavefront-scope fences only keep the COMPILER from reordering a lane's reads against the other lanes' writes. ----
typedef __attribute__((address_space(3))) float lds_f;
constexpr int SW_SLOT = 392;                 // floats per group in the stage: two 14x14 blocks
__device__ __forceinline__ void stage_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// rows-in-lanes block -> column-major ROWS x COLS at float offset o of this group's slot
template <int ROWS, int COLS>
__device__ __forceinline__ void stage_put(lds_f* slot, int o, const f2 (&M)[np(COLS)], int lr, float mult) {
    if (lr < ROWS) {
#pragma unroll
        for (int j = 0; j < np(COLS); ++j) {
            slot[o + 2 * j * ROWS + lr] = M[j].x * mult;
            if (2 * j + 1 < COLS) slot[o + (2 * j + 1) * ROWS + lr] = M[j].y * mult;
        }
    }
}
// the same block TRANSPOSED: row lr becomes column lr of the staged COLS x COLS block
template <int COLS>
__device__ __forceinline__ void stage_put_t(lds_f* slot, int o, const f2 (&M)[np(COLS)], int lr, float mult) {
    if (lr < COLS) {
#pragma unroll
        for (int j = 0; j < np(COLS); ++j) {
            slot[o + lr * COLS + 2 * j] = M[j].x * mult;
            if (2 * j + 1 < COLS) slot[o + lr * COLS + 2 * j + 1] = M[j].y * mult;
        }
    }
}
// copy the first NFL floats of every group's slot to that group's destination: dst = byte offset in r (uniform inside a 16-lane group),
// SW_OOB = this group stores nothing.  GB = bytes per lane and store: 16 (destination 16-byte aligned... or not: the hardware takes
// dword-aligned 16-byte stores), or 4.
template <int NFL, int GB>
__device__ __forceinline__ void stage_flush(lds_f* stage, rsrc_t r, uint32_t dst, int lane) {
    constexpr int NG = NFL * 4 / GB;                     // pieces per group
    constexpr int NR = (NG + 63) / 64;                   // store instructions per group
    static_assert(NFL * 4 % GB == 0, "whole pieces");
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) u4 lds_u4;
    stage_fence();
    // all LDS reads first (one round trip), then the stores.  The soffset operand is not bounds-checked (only voffset is): a disabled
    // group's lanes get the out-of-range voffset, like the lanes beyond the last piece.
    u4 v16[4][NR];
    float v4[4][NR];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            lds_f* src = stage + g * SW_SLOT + (q * 64 * GB) / 4;
            if constexpr (GB == 16) v16[g][q] = *(lds_u4*)(src + lane * 4);
            else v4[g][q] = src[lane];
        }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint32_t sd = (uint32_t)__builtin_amdgcn_readlane((int)dst, 16 * g);
        const bool en = sd != SW_OOB;                    // (uniform)
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const int idx = q * 64 + lane;
            const uint32_t vo = (en && (q * 64 + 64 <= NG || idx < NG)) ? (uint32_t)(idx * GB) : SW_OOB;
            if constexpr (GB == 16) __builtin_amdgcn_raw_buffer_store_b128(v16[g][q], r, (int)vo, (int)(en ? sd : 0u), 0);
            else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v4[g][q]), r, (int)vo, (int)(en ? sd : 0u), 0);
        }
    }
    stage_fence();
}

template <int NN>
__device__ __forceinline__ void add_rho(f2 (&M)[np(NN)], int lr, float rho) {
#pragma unroll
    for (int j = 0; j < np(NN); ++j)         // x + (-0.0) has the bits of x for every x: one packed add per pair, no branches
        M[j] = M[j] + f2{lr == 2 * j ? rho : -0.f, lr == 2 * j + 1 ? rho : -0.f};
}
template <int NN>
__device__ __forceinline__ void add_rho(double (&M)[NN], int lr, double rho) {
#pragma unroll
    for (int c = 0; c < NN; ++c) M[c] = M[c] + (lr == c ? rho : -0.0);      // x + (-0.0) has the bits of x
}

template <typename T>
struct WalkArgsT {
    SchurArgsT<T> s;
    T* seam_qinv;           // [batch][chunks][196]: (Q_{k0-1} + rho I)^-1 of chunks j >= 1 (schur_seam_kernel stores them into G)
    int L;                  // block rows per chunk
    int chunks;             // ceil((N - 1) / L) >= 1
};
// mpcg_form_schur_rhov(_f64): one rho per trajectory.  The scalar kernel takes the base, so its arguments keep their offsets.
template <typename T>
struct WalkArgsVT : WalkArgsT<T> { const T* rho_v; };     // [batch]

// wavefronts per SIMD the register allocation aims at: walk and seam 2 / 1, dz 4 / 2 for float / double
template <typename T>
constexpr int waves(int f32) { return std::is_same<T, float>::value ? f32 : f32 / 2; }

// One 16-lane row = one chunk: block rows k0 = 1 + j L ... k1 - 1 of trajectory b; chunk 0 also emits block row 0 (linsys_setup.cuh:152-277),
// which needs nothing but Q_0.  Four chunks per wavefront, in lock-step.  (Host: every array below 2^31 bytes.)
// WA = WalkArgsT<T>: s.rho for every trajectory.  WA = WalkArgsVT<T>: the item's trajectory b — one per 16-lane row — reads rho_v[b] once per
// item, through a buffer resource like every other operand (dead rows redo item `items - 1`: a valid index); the additions are the same.
// Float and double differ in six places: how blocks are stored (float: the LDS stage, double: rows — SW_STORE14 and two `if constexpr (F32)`
// blocks), the wait before the loop, the opaque lane number, matvec2 (an overload: two matvec in double), when the next row's A / B are
// requested, and the re-read of rho_v[b] — but for matvec2 an `if constexpr (F32)` each, at the place where the two builds always differed.
// SW_STORE14: one 14 x 14 block leaves the row loop — through the stage in float, as rows in double.  (A macro over the loop's locals, not a
// lambda: a function evaluates `on` and `off` BEFORE the block is staged, the code this replaces did so after, and with that order changed the
// float builds come out with other register numbers than the two-header version they are pinned to, profiles/schur_walk_templates_same_code.txt.)
#define SW_STORE14(M, r, off, on, mult)                                                             \
    do {                                                                                            \
        if constexpr (F32) {                                                                        \
            stage_put<n, n>(slot, 0, M, lr_s, mult);                                                \
            stage_flush<nn, 16>(stage, r, (on) ? (off) : SW_OOB, lane_s);                           \
        } else store_rows<n>(M, r, off, n, lr, on, mult);                                           \
    } while (0)
template <typename T, class WA = WalkArgsT<T>>
__global__ __launch_bounds__(64, waves<T>(2)) void schur_walk_kernel(WA w) {
    constexpr bool F32 = std::is_same<T, float>::value;
    constexpr bool RHOV = std::is_same<WA, WalkArgsVT<T>>::value;
    constexpr int n = 14, m = 7;
    constexpr uint32_t nn = n * n, mm = m * m, nm = n * m, E = sizeof(T);
    constexpr uint32_t Gset = nn + mm, Cset = nn + nm, gset = n + m;
    constexpr int W = F32 ? np(n) : n;                       // registers' worth of one 14-column operand: pairs or columns
    const SchurArgsT<T>& a = w.s;
    const int N = a.N, L = w.L, chunks = w.chunks;
    const uint32_t Gsz = Gset * (uint32_t)N - mm, Csz = Cset * (uint32_t)(N - 1), gsz = gset * (uint32_t)N - m;
    const uint32_t B = (uint32_t)a.batch;
    const rsrc_t rG = make_rsrc(a.Ginv_out, (size_t)B * Gsz * E), rC = make_rsrc(a.C, (size_t)B * Csz * E), rg = make_rsrc(a.g, (size_t)B * gsz * E),
                 rc = make_rsrc(a.c, (size_t)B * n * N * E), rS = make_rsrc(a.S, (size_t)B * 3 * nn * N * E),
                 rP = make_rsrc(a.Pinv, a.pinv ? (size_t)B * 3 * nn * N * E : 0), rgam = make_rsrc(a.gamma, (size_t)B * n * N * E),
                 rQ = make_rsrc(w.seam_qinv, (size_t)B * chunks * nn * E);
    const int lane = threadIdx.x;
    const int lr = lane & 15;
    const bool r14 = lr < n, r7 = lr < m;
    const uint32_t l14 = E * (r14 ? lr : n - 1), l7 = E * (r7 ? lr : m - 1);
    __shared__ float sStage[4 * SW_SLOT];                   // float: the store stage (6,272 B per wavefront); double: unused, not allocated
    lds_f* stage = (lds_f*)sStage;
    const unsigned items = B * (unsigned)chunks;
    for (unsigned base = blockIdx.x * 4u; base < items; base += gridDim.x * 4u) {
        const unsigned item = base + (unsigned)(lane >> 4);
        const bool live = item < items;
        const unsigned it = live ? item : items - 1;        // dead rows redo the last item and store nothing
        const uint32_t b = it / (unsigned)chunks, j = it % (unsigned)chunks;
        const int k0 = 1 + (int)j * L;
        const int k1 = (k0 + L < N) ? k0 + L : N;
        // byte offsets of trajectory b
        const uint32_t oG = b * Gsz * E, oC = b * Csz * E, og = b * gsz * E, oc = b * (uint32_t)(n * N) * E, oS = b * (3u * nn * (uint32_t)N) * E;
        const bool st14 = live && r14;
        T rho;
        if constexpr (RHOV) rho = bld<T>(make_rsrc(w.rho_v, (size_t)B * E), b * E);
        else rho = a.rho;

        // ---- prologue: (Q_{k0-1} + rho I)^-1; for chunk 0 that is block row 0 ----
        Rows<T, n> Qi;         // carried: (Q_{k-1} + rho I)^-1
        Rows<T, n> Tm;         // carried: theta_{k-1}^-1 (un-negated; for k-1 = 0: Q_0 + rho I, i.e. -Pinv[0,1])
        {
            Rows<T, n> Qa;
            load_rows<n>(Qa, rG, oG + (uint32_t)(k0 - 1) * Gset * E, n, lr);
            add_rho<n>(Qa, lr, rho);
#pragma unroll
            for (int q = 0; q < W; ++q) Tm[q] = Qa[q];
            const bool first = j == 0;
            store_rows<n>(Qa, rP, oS + nn * E, n, lr, st14 && first, T(-1));                      // Pinv[0,1] = -(Q0 + rho I)   :201-210  (no Pinv: zero-size resource)
            invert<n>(Qa, Qi, lr);                                                                // :356-368
            const T q0 = bld<T>(rg, og + l14);
            const T g0 = matvec<n>(Qi, q0);                                                       // :259-264
            store_rows<n>(Qi, rS, oS + nn * E, n, lr, st14 && first, T(-1));                      // S[0,1] = -Q0^-1             :248-255
            bst(rgam, (st14 && first) ? oc + E * lr : SW_OOB, -g0);                               // :272-276
            // G <- G^-1 (:371-380): Q_0 in place (nobody else reads it); the other chunks' first inverse belongs to the left neighbour's
            // last knot, which that neighbour still reads raw — it goes to the seam buffer
            store_rows<n>(Qi, rG, oG, n, lr, st14 && first, T(1));
            store_rows<n>(Qi, rQ, (b * (uint32_t)chunks + j) * nn * E, n, lr, st14 && !first, T(1));
        }
        bool have_tm = j == 0;
        // The operands of a block row are requested one row AHEAD, each set as soon as the registers of the previous set are dead (the raw
        // Q / R right after their inversion, A / B after the last product that reads them — double: see the end of the row): half a row of
        // arithmetic hides the HBM latency without a register of its own.  (Past the chunk's end the requests repeat its last row.)
        Rows<T, n> Ak;                                                                            // linsys_setup.cuh:318-325
        Rows<T, m> Bk, Rk;
        Rows<T, n> Qp;
        T qk, rk, qp, ck;
        auto row_of = [&](int s_) -> uint32_t { const int kk_ = k0 + s_; return (uint32_t)(kk_ < k1 ? kk_ : k1 - 1); };
        auto load_QR = [&](uint32_t k_) {
            const uint32_t oGk_ = oG + (k_ - 1) * Gset * E;
            load_rows<m>(Rk, rG, oGk_ + nn * E, m, lr);
            load_rows<n>(Qp, rG, oGk_ + Gset * E, n, lr);
        };
        auto load_AB = [&](uint32_t k_) {
            const uint32_t oCk_ = oC + (k_ - 1) * Cset * E;
            load_rows<n>(Ak, rC, oCk_, n, lr);
            load_rows<m>(Bk, rC, oCk_ + nn * E, n, lr);
        };
        auto load_vec = [&](uint32_t k_) {
            qk = bld<T>(rg, og + (k_ - 1) * gset * E + l14); rk = bld<T>(rg, og + (k_ - 1) * gset * E + n * E + l7);
            qp = bld<T>(rg, og + k_ * gset * E + l14); ck = bld<T>(rc, oc + k_ * n * E + l14);
        };
        load_QR(row_of(0)); load_AB(row_of(0)); load_vec(row_of(0));
        // Float: the first row's operands are waited for HERE, all of them.  Without this the compiler's wait-count bookkeeping merges two loop
        // entries — this one, where the requests above are the youngest memory operations, and the back edge, where the same registers were
        // requested BEFORE the previous row's 24 output stores — into the stricter of the two: vmcnt(5) ... vmcnt(0) at the top of every
        // row, i.e. every row also waited for the previous row's stores.  (With it: vmcnt(61) ... — loads only.  No measurable difference
        // in time, profiles/r04_walk_store_side.txt: the stores' cost is on the memory side.)
        if constexpr (F32) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        for (int s = 0; s < L; ++s) {
            const int kk = k0 + s;
            const bool rowl = kk < k1;
            const uint32_t k = row_of(s), kn = row_of(s + 1);    // rows past the chunk's end redo its last row and store nothing
            const bool on14 = st14 && rowl;
            [[maybe_unused]] const bool on7 = live && r7 && rowl;
            const uint32_t oGk = oG + (k - 1) * Gset * E, oSk = oS + k * 3u * nn * E;
            // Float: the stage's lane constants (piece offsets, slot addresses) are re-derived from an opaque copy of the lane number in
            // every trip: as loop invariants the compiler keeps two dozen of them in registers across the loop and spills
            int lane_s = lane;
            if constexpr (F32) asm volatile("" : "+v"(lane_s));
            [[maybe_unused]] const int lr_s = lane_s & 15;
            [[maybe_unused]] lds_f* slot = stage + (lane_s >> 4) * SW_SLOT;
            add_rho<n>(Qp, lr, rho);
            add_rho<m>(Rk, lr, rho);
            Rows<T, n> Qpi;
            Rows<T, m> Rki;
            SW_FENCE();
            invert<n>(Qp, Qpi, lr);                                                               // :356-368
            SW_FENCE();
            invert<m>(Rk, Rki, lr);
            SW_FENCE();
            // G <- G^-1 (:371-380): R_{k-1} and Q_k are this chunk's own — except the chunk's LAST Q when a right neighbour exists (that one
            // reads it raw in its prologue and hands its inverse to the seam kernel)
            [[maybe_unused]] const bool gl = live && rowl;       // (uniform inside the group)
            const bool bl14 = F32 ? gl : on14;                   // a block's store is enabled per group through the stage, per lane as rows
            if constexpr (F32) {
                stage_put<m, m>(slot, 0, Rki, lr_s, 1.f);
                stage_flush<mm, 4>(stage, rG, gl ? oGk + nn * E : SW_OOB, lane_s);
            } else store_rows<m>(Rki, rG, oGk + nn * E, m, lr, on7, 1.0);
            SW_STORE14(Qpi, rG, oGk + Gset * E, bl14 && (kk < k1 - 1 || k1 == N), T(1));
            load_QR(kn);                                                                          // (next row; after this row's in-place stores)
            Rows<T, n> phi;
            Rows<T, m> BR;
            gemm_nn<n, n>(Ak, Qi, phi);                                                           // phi = Abar Qi      :397-398
            SW_FENCE();
            gemm_nn<m, m>(Bk, Rki, BR);                                                           // Bbar Ri            :405-406
            SW_FENCE();
            const auto gv = matvec2<n>(Qpi, qp, phi, qk);                                         // :410-415, 421-426
            T gam = gv.x - ck;                                                                    // :416-418
            const T v2 = matvec<m>(BR, rk);                                                       // :431-436
            gam += v2 + gv.y;                                                                     // :441-443
            bst(rgam, on14 ? oc + k * n * E + E * lr : SW_OOB, -gam);                             // :528-532
            load_vec(kn);
            Rows<T, n> theta;
            {
                Rows<T, n> t1;
                gemm_nt<n, n>(phi, Ak, theta);                                                    // phi Abar^T         :446-455
                SW_FENCE();
                gemm_nt<m, n>(BR, Bk, t1);                                                        // (Bbar Ri) Bbar^T   :472-481
#pragma unroll
                for (int q = 0; q < W; ++q) { theta[q] = theta[q] + Qpi[q]; theta[q] = theta[q] + t1[q]; }   // :466-468, 485-487
            }
            SW_FENCE();
            if constexpr (F32) {
                load_AB(kn);
                stage_put<n, n>(slot, 0, phi, lr_s, -1.f);                                          // S[k,0]             :490-497
                stage_put<n, n>(slot, nn, theta, lr_s, -1.f);                                       // S[k,1]             :500-507
                stage_flush<2 * nn, 16>(stage, rS, gl ? oSk : SW_OOB, lane_s);
                stage_put_t<n>(slot, 0, phi, lr_s, -1.f);                                           // S[k-1,2] = -phi^T  :536-557
                stage_flush<nn, 16>(stage, rS, gl ? oSk - nn * E : SW_OOB, lane_s);
            } else {
                store_rows<n>(phi, rS, oSk, n, lr, on14, -1.0);                                   // S[k,0]             :490-497
                store_rows<n>(theta, rS, oSk + nn * E, n, lr, on14, -1.0);                        // S[k,1]             :500-507
                store_rows_t<n>(phi, rS, oSk - nn * E, lr, on14, -1.0);                           // S[k-1,2] = -phi^T  :536-557
            }
#pragma unroll
            for (int q = 0; q < W; ++q) Qi[q] = Qpi[q];
            if (a.pinv) {                                                                         // (uniform)
                Rows<T, n> Ti;
                SW_FENCE();
                invert<n>(theta, Ti, lr);                                                         // :510-514
                SW_FENCE();
                SW_STORE14(Ti, rP, oSk + nn * E, bl14, T(-1));                                       // Pinv[k,1] = -theta^-1   :517-524
                if (a.ss) {                                                                       // (uniform)  :9-137
                    // stored blocks are D = -theta^-1, L = -phi; the reference forms -(D_k L_k) D_{k-1} and -(D_{k-1} L_k^T) D_k from the stored
                    // (negated) blocks: the three sign flips cancel exactly, so the un-negated operands give the stored values directly
                    Rows<T, n> t1, t2;
                    gemm_nn<n, n>(Ti, phi, t1);                                                   // Dk L            :100
                    SW_FENCE();
                    gemm_nn<n, n>(t1, Tm, t2);                                                    // (Dk L) Dm       :102
                    SW_FENCE();
                    SW_STORE14(t2, rP, oSk, bl14 && have_tm, T(1));                                  // Pinv[k,0]       :106-113
                    gemm_nt<n, n>(Tm, phi, t1);                                                   // Dm phi^T        :121
                    SW_FENCE();
                    gemm_nn<n, n>(t1, Ti, t2);                                                    // (Dm phi^T) Dk   :123
                    SW_FENCE();
                    SW_STORE14(t2, rP, oSk - nn * E, bl14 && have_tm, T(1));                         // Pinv[k-1,2]     :127-134
                }
#pragma unroll
                for (int q = 0; q < W; ++q) Tm[q] = Ti[q];
            }
            have_tm = true;
            if constexpr (!F32) {
                // Double: next row's A / B only now: requested any earlier they would be live across the symmetric-stair products, the register
                // peak of a row (130 doubles); the two inversions at the head of the next row hide their latency.
                // rho_v[b] again for the next row (a cached 8-byte load) rather than a double carried across the row's register peak: with it
                // carried the kernel needs 4 registers more than its scalar twin, reloaded 22 fewer.  Requested AHEAD of A / B, so that the next
                // row's wait for it leaves their loads in flight.
                if constexpr (RHOV) rho = bld<T>(make_rsrc(w.rho_v, (size_t)B * E), b * E);
                load_AB(kn);
            }
        }
    }
}

#undef SW_STORE14

// The seams: for chunk j >= 1 of every trajectory, with k0 = 1 + j L — G[k0-1].Q <- the inverse the chunk's prologue computed, and (SS) the
// two coupling blocks across the seam, Pinv[k0,0] and Pinv[k0-1,2], from the stored blocks (linsys_setup.cuh:97-136).
template <typename T>
__global__ __launch_bounds__(64, waves<T>(2)) void schur_seam_kernel(WalkArgsT<T> w) {
    constexpr int n = 14, m = 7;
    constexpr uint32_t nn = n * n, mm = m * m, E = sizeof(T);
    constexpr uint32_t Gset = nn + mm;
    const SchurArgsT<T>& a = w.s;
    const int N = a.N, L = w.L, chunks = w.chunks;
    const uint32_t Gsz = Gset * (uint32_t)N - mm;
    const uint32_t B = (uint32_t)a.batch;
    const rsrc_t rG = make_rsrc(a.Ginv_out, (size_t)B * Gsz * E), rS = make_rsrc(a.S, (size_t)B * 3 * nn * N * E),
                 rP = make_rsrc(a.Pinv, a.pinv ? (size_t)B * 3 * nn * N * E : 0), rQ = make_rsrc(w.seam_qinv, (size_t)B * chunks * nn * E);
    const int lane = threadIdx.x;
    const int lr = lane & 15;
    const bool r14 = lr < n;
    const unsigned per = (unsigned)(chunks - 1);
    const unsigned items = B * per;
    for (unsigned base = blockIdx.x * 4u; base < items; base += gridDim.x * 4u) {
        const unsigned item = base + (unsigned)(lane >> 4);
        const bool live = item < items;
        const unsigned it = live ? item : items - 1;
        const uint32_t b = it / per, j = 1 + it % per;
        const uint32_t k0 = 1 + j * (uint32_t)L;
        const uint32_t oS = b * (3u * nn * (uint32_t)N) * E, oSk = oS + k0 * 3u * nn * E;
        {
            const uint32_t src = (b * (uint32_t)chunks + j) * nn * E, dst = b * Gsz * E + (k0 - 1) * Gset * E;
            for (uint32_t e = lr; e < nn; e += 16) bst(rG, live ? dst + E * e : SW_OOB, bld<T>(rQ, src + E * e));
        }
        if (!a.ss) continue;
        // stored blocks: Dk = Pinv[k0,1], Dm = Pinv[k0-1,1], Lk = S[k0,0].  Pinv[k0,0] = -((Dk Lk) Dm), Pinv[k0-1,2] = -((Dm Lk^T) Dk).
        // Second operands are loaded transposed and used through gemm_nt: the sums of A B in the same order.
        Rows<T, n> Dk, Dm, t1, t2;
        load_rows<n>(Dk, rP, oSk + nn * E, n, lr);
        load_rows<n>(Dm, rP, oSk - 2u * nn * E, n, lr);
        {
            Rows<T, n> LT, DmT;
            load_rows_t<n>(LT, rS, oSk, n, lr);
            load_rows_t<n>(DmT, rP, oSk - 2u * nn * E, n, lr);
            gemm_nt<n, n>(Dk, LT, t1);                                                            // Dk L            :100
            SW_FENCE();
            gemm_nt<n, n>(t1, DmT, t2);                                                           // (Dk L) Dm       :102
            store_rows<n>(t2, rP, oSk, n, lr, live && r14, T(-1));                                // Pinv[k0,0]      :106-113
        }
        SW_FENCE();
        {
            Rows<T, n> Lk, DkT;
            load_rows<n>(Lk, rS, oSk, n, lr);
            load_rows_t<n>(DkT, rP, oSk + nn * E, n, lr);
            gemm_nt<n, n>(Dm, Lk, t1);                                                            // Dm phi^T        :121
            SW_FENCE();
            gemm_nt<n, n>(t1, DkT, t2);                                                           // (Dm phi^T) Dk   :123
            store_rows<n>(t2, rP, oSk - nn * E, n, lr, live && r14, T(-1));                       // Pinv[k0-1,2]    :127-134
        }
    }
}

// dz = G^-1 (g - C^T lambda)  (include/common/dz.cuh:3-121), four knots per wavefront, a 16-lane row per knot:
//   dz_x = Qi (q - (lambda_k + Abar^T lambda_{k+1})), dz_u = Ri (r - Bbar^T lambda_{k+1});  the last knot has neither the A/B terms nor a dz_u.
// Abar^T lambda: lane t takes row t of Abar^T = column t of Abar (14 contiguous elements), gato_ATx's sum order (matrix.cuh:10-25).
// Round 3 ran one 64-thread workgroup per knot with two block barriers: 128 us per 1024 x 128 knots; this one is a plain HBM stream.
// (Host: N >= 2, every array below 2^31 bytes.)
template <typename T>
__global__ __launch_bounds__(64, waves<T>(4)) void compute_dz_dpp_kernel(DzArgsT<T> a) {
    constexpr int n = 14, m = 7;
    constexpr uint32_t nn = n * n, mm = m * m, nm = n * m, E = sizeof(T);
    constexpr uint32_t Gset = nn + mm, Cset = nn + nm, gset = n + m;
    const int N = a.N;
    const uint32_t Gsz = Gset * (uint32_t)N - mm, Csz = Cset * (uint32_t)(N - 1), gsz = gset * (uint32_t)N - m;
    const uint32_t B = (uint32_t)a.batch;
    const rsrc_t rG = make_rsrc(a.Ginv, (size_t)B * Gsz * E), rC = make_rsrc(a.C, (size_t)B * Csz * E), rg = make_rsrc(a.g, (size_t)B * gsz * E),
                 rl = make_rsrc(a.lambda, (size_t)B * n * N * E), rz = make_rsrc(a.dz, (size_t)B * gsz * E);
    const int lane = threadIdx.x;
    const int lr = lane & 15;
    const bool r14 = lr < n, r7 = lr < m;
    const uint32_t l14 = E * (r14 ? lr : n - 1), l7 = E * (r7 ? lr : m - 1);
    const unsigned items = B * (unsigned)N;
    // (one group of four knots per workgroup and trip.  Tried in round 4: spans of 4 / 8 / 16 consecutive groups per wavefront, so that its
    //  84-byte pieces of dz meet in one L2 as whole lines — what gained 25 % in bt_spmv_kernel: 60-63 us against 56.6 here, the serial
    //  trips cost more memory-level parallelism than the partial lines cost.)
    for (unsigned base = blockIdx.x * 4u; base < items; base += gridDim.x * 4u) {
        const unsigned item = base + (unsigned)(lane >> 4);
        const bool live = item < items;
        const unsigned it = live ? item : items - 1;
        const uint32_t b = it / (unsigned)N, k = it % (unsigned)N;
        const bool last = k == (uint32_t)(N - 1);
        const uint32_t kc = last ? k - 1 : k;                         // the last knot re-reads its neighbour's C / R (results dropped)
        const uint32_t oG = b * Gsz * E + k * Gset * E, oR = b * Gsz * E + kc * Gset * E + nn * E, oC = b * Csz * E + kc * Cset * E;
        const uint32_t og = b * gsz * E + k * gset * E, ol = b * (uint32_t)(n * N) * E + k * n * E;
        Rows<T, n> At, Bt, Qi;
        Rows<T, m> Ri;
        load_rows_t<n>(At, rC, oC, n, lr);                            // lane t: Abar[0..13][t] = Ck[t n + i]
        load_rows_t<n>(Bt, rC, oC + nn * E, m, lr);                   // lane j < 7: Bbar[0..13][j]
        load_rows<n>(Qi, rG, oG, n, lr);
        load_rows<m>(Ri, rG, oR, m, lr);
        const T lk = bld<T>(rl, ol + l14);
        const T ln = bld<T>(rl, ol + (last ? 0u : n * E) + l14);
        const T gx = bld<T>(rg, og + l14), gu = bld<T>(rg, og + (last ? l14 : n * E + l7));
        const auto acc = matvec2<n>(At, ln, Bt, ln);                  // Abar^T lambda_{k+1} | Bbar^T lambda_{k+1}
        const T ax = last ? T(0) : acc.x;
        const T tx = gx - (lk + ax);
        const T tu = gu - acc.y;
        const T dx = matvec<n>(Qi, tx);
        const T du = matvec<m>(Ri, tu);
        bst(rz, (live && r14) ? og + E * lr : SW_OOB, dx);
        bst(rz, (live && r7 && !last) ? og + n * E + E * lr : SW_OOB, du);
    }
}

#pragma clang fp contract(fast)

}  // namespace sw
}  // namespace mpcg
