// pcg_lxk_driver.hip.h — the conjugate-gradient recurrence of the register-resident single-CU kernels, written once: pcg_lpk_kernel (float, a
// lane pair per knot, pcg_lpk.hip.h) and pcg_lqk_f64_kernel (double, a lane quad per knot, pcg_lqk_f64.hip.h).  What a kernel does INSIDE a
// pass is its own (lpk_half / lqk_half); what happens between the passes is lxk_role.
//
// Half of a workgroup's wavefronts hold S, half hold Pinv.  The role is wave-uniform, and each role runs its own code path (lxk_role<P>)
// through the SAME two synchronisation points per iteration:
//     S waves  (P = false)                              Pinv waves  (P = true)
//     p = r~ + beta p ; upsilon = S p ; v = p.upsilon   .
//     ------------------------------------ arrive(V) : barrier ------------------------------------
//     alpha = eta / v ; lambda += alpha p               alpha = eta / v ; r -= alpha upsilon ; r~ = Pinv r ; eta' = r.r~
//     ------------------------------------ arrive(E) : barrier ------------------------------------
//     eta' ; exit test ; beta = eta' / eta              (the same, on the same values)
// p and r never exist in LDS inside the loop: a lane carries its entries in registers (Vec) and rebuilds the next operand from what the other
// matrix's pass published (Fetch) and the scalar.  The setup is the same sequence with r = gamma - S lambda0, r~ = Pinv r, eta = r.r~ (p = r~
// is formed by the first S half: beta = 0).  Results (LxkCg, references to the kernel's own variables): the iteration count; max_iter_exit (1:
// ran out of iterations, 0: tolerance reached); beta and p_pending for the write-back — after a max-iteration exit the last p = r~ + beta p
// has not been applied and d_p must hold it, after a tolerance exit the reference leaves p as it is.  At the end each role stores the vector
// it carries to R0 / P0, the staging buffers, free since the setup.
//
// What a kernel brings (callables; `phase` = LxkV / LxkE, `role` = std::integral_constant<bool, P>):
//     load_own(X, dk), store_own(X, own), fetch(T, Z)   thin wrappers over lpk_* / lqk_*
//     half(mode, phase, f, old, c, TOUT, ZOUT)          one pass of this wave's matrix; the wave's inner-product share goes to `phase`'s partials
//     arrive(role, phase)                               the synchronisation point behind a half (the -DMPCG_PROF build stamps around it)
//     value(phase)                                      the reduction: the sum of the partials for V, the wave-uniform sum for E.  Read AFTER what
//                                                       the role fetches first behind the barrier (operands: volatile LDS loads; lambda)
//     more(it)                                          another iteration?  (it < max_iter, read through the kernel's closure as the loop always
//                                                       did; the -DMPCG_PROF build arms its stamps here)
//
// Same device code as the two copies this replaces (profiles/lxk_driver_same_code.txt), which is why some of it looks arbitrary: the results
// are references held by value, the bound sits in a hook, the kernels call lxk_role<true> / <false> themselves.  Each of these was needed to
// keep the instruction text; the clustered kernels (pcg_lpkc_kernel, pcg_lqkc_f64_kernel) and the staging / write-back loops did not keep
// theirs under any shape tried and still carry their own copies.
#pragma once
#include "pcg_kernels.hip.h"

namespace mpcg {

using LxkV = std::integral_constant<int, 0>;      // the S half's inner product v = p . S p
using LxkE = std::integral_constant<int, 1>;      // the Pinv half's eta = r . Pinv r
template <class real> struct LxkCg {
    uint32_t& iters;
    uint32_t& max_iter_exit;
    real& beta;                                    // scalar of the NEXT p update (the S half applies it)
    bool& p_pending;                               // that update has not been applied to p (the write-back of d_p does it)
};

// L: the kernel's LDS layout; T: the precision's types and scalar helpers (LpkTypes / LqkTypes); a: PcgArgs / PcgArgs64 (exit_tol)
template <bool P, class L, class T, class A, class LoadOwn, class StoreOwn, class FetchF, class Half, class Arrive, class Value, class More>
__device__ __forceinline__ void lxk_role(const A& a, const LxkCg<typename T::real> cg, const LoadOwn& load_own, const StoreOwn& store_own, const FetchF& fetch,
                                         const Half& half, const Arrive& arrive, const Value& value, const More& more) {
    typedef typename T::real real;
    constexpr std::integral_constant<bool, P> role{};
    // ---- setup: r = gamma - S lambda0 ; r~ = Pinv r ; eta = r . r~ ----
    typename T::Fetch f;
    typename T::Vec x;                                       // S waves: p;  Pinv waves: r
    x.k = load_own(P ? L::R0 : L::P0, 0);
    x.m = load_own(P ? L::R0 : L::P0, -1);
    if constexpr (!P) (void)half(std::integral_constant<int, 0>{}, LxkV{}, f, x, real(0), L::US, L::ZS);
    arrive(role, LxkV{});
    if constexpr (P) {
        f = fetch(L::US, L::ZS);
        x = half(std::integral_constant<int, 1>{}, LxkE{}, f, x, real(1), L::RT, L::ZP);
    }
    arrive(role, LxkE{});
    if constexpr (!P) f = fetch(L::RT, L::ZP);
    real eta = value(LxkE{});
    // every matrix load has been consumed on the waves that ran a setup pass; say so, or the compiler keeps vmcnt waits inside the loop
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0)
    if (T::abs(eta) < a.exit_tol) {
        cg.max_iter_exit = 0;
    } else {
        for (int it = 0; more(it); ++it) {
            if constexpr (!P) {
                // p = r~ + beta p ; upsilon = S p ; v = p . upsilon
                x = half(std::integral_constant<int, 2>{}, LxkV{}, f, x, cg.beta, L::US, L::ZS);
                arrive(role, LxkV{});
                // alpha = eta / v ; lambda += alpha p (own entries) — while the Pinv half runs
                const typename T::Own cur = load_own(L::LAM, 0);
                const real alpha = T::uniform(eta / value(LxkV{}));
                typename T::Own nw;
#pragma unroll
                for (int s = 0; s < 4; ++s) nw.v[s] = cur.v[s] + alpha * x.k.v[s];
                store_own(L::LAM, nw);
            } else {
                arrive(role, LxkV{});
                // alpha = eta / v ; r -= alpha upsilon ; r~ = Pinv r ; eta' = r . r~
                f = fetch(L::US, L::ZS);
                const real alpha = T::uniform(eta / value(LxkV{}));
                x = half(std::integral_constant<int, 1>{}, LxkE{}, f, x, alpha, L::RT, L::ZP);
            }
            arrive(role, LxkE{});
            if constexpr (!P) f = fetch(L::RT, L::ZP);       // the next S half's operand loads fly during the scalar chain below
            // eta' ; exit test ; beta
            const real eta_new = value(LxkE{});
            cg.iters = (uint32_t)(it + 1);
            if (T::abs(eta_new) < a.exit_tol) { cg.max_iter_exit = 0; cg.p_pending = false; break; }     // (the reference leaves p as it is on this exit)
            cg.beta = T::uniform(eta_new / eta);
            eta = eta_new;
        }
    }
    // the vector this role carries, for d_p / d_r (the staging buffers are free since the setup)
    store_own(P ? L::R0 : L::P0, x.k);
}

}  // namespace mpcg
