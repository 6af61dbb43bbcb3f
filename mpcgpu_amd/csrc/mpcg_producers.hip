// mpcg_producers.hip — C ABI (include/mpcg.h) of the steps either side of the solve: Schur + preconditioner formation, dz
// recovery (float and linsys_t = double), the CSR emitter of the QDLDL path and the block-tridiagonal direct solve.  Two sets of gfx950
// kernels serve them: the register-resident ones of schur_walk.hip.h / block_solve.hip.h (the tuned 14 x 7 shape,
// the default there) and the run-time-dimension LDS kernels of schur_generic.hip.h (every other 1 <= control_size <= state_size <= 64; at
// 14 x 7 under "schur_dpp" / "dz_dpp" = 0 or "producers_generic" = 1, and for calls beyond the register-resident kernels' 31-bit offsets).
// Formation, dz and the direct solve have ONE host path each, form_schur_impl<T>, compute_dz_impl<T> and block_solve_impl<CT, ST>; ProducerTraits<T>
// holds what float and double differ in.
#include "mpcg_handle.hpp"
#ifndef MPCG_DZ64_CAPMUL
#define MPCG_DZ64_CAPMUL 4      // (grid cap of compute_dz_dpp_kernel<double> in units of 64 workgroups per CU; tools/_prof/dz64_ab.py)
#endif
#include "schur_generic.hip.h"
#include "schur_walk.hip.h"
#include "block_solve.hip.h"

using namespace mpcg;

// The walking Schur kernels' seam buffer (one 14 x 14 Q^-1 per chunk, float or double).  Sized ONCE, on first use, for whatever the automatic
// chunk length can ask of this handle: chunks shorter than 16 rows are chosen only while the call has fewer than 2 x `want` rows per chunk
// length, i.e. at most 2 x want + batch chunks; 16-row chunks beyond — so calls of different batch sizes never reallocate (a reallocation
// inside a stream capture would leave a dangling pointer in the captured graph: ADVICE r04).  Only a FORCED short "schur_chunk" can ask for
// more; that grows the buffer outside a capture and is refused inside one.
static int ensure_seam_buffer(mpcg_handle* h, size_t chunks_needed, size_t elem_bytes, hipStream_t st) {
    const size_t want = (size_t)h->num_cus * 6 * 4;
    const size_t auto_chunks = std::max<size_t>(2 * want + h->max_batch + 4, (size_t)h->max_batch * (size_t)(((size_t)h->N - 1 + 15) / 16));
    // (the automatic part in doubles whatever this call's type: a float call followed by a linsys_t = double call must not reallocate either)
    const size_t need = 196 * std::max(chunks_needed * elem_bytes, auto_chunks * sizeof(double));
    return buf_reserve(h, BUF_SEAM, need, &st, "mpcg_form_schur (the seam buffer; a forced short \"schur_chunk\" needs a larger one)");
}

// ---- the LDS route (schur_generic.hip.h): any 1 <= control_size <= state_size; at (14, 7) whatever does not run register-resident ----
static constexpr size_t kGenLdsMax = 160 * 1024;       // LDS of one CU: what one workgroup's operands may occupy

static inline bool gen_route(const mpcg_handle* h, uint32_t control_size) { return h->generic || control_size != 7 || h->producers_generic; }
static inline int gen_threads(int n) { return n <= 16 ? 64 : 256; }      // one wavefront up to n = 16; beyond, an n^2 update is >= 4 elements per lane of one
// workgroups of a grid-stride launch: 64 per CU, fewer when the LDS holds fewer per CU
static inline unsigned gen_grid(const mpcg_handle* h, long items, size_t lds_bytes) {
    const long per_cu = std::min<long>(64, std::max<long>(1, (long)(kGenLdsMax / std::max<size_t>(lds_bytes, 1))));
    return (unsigned)std::max<long>(1, std::min<long>(items, (long)h->num_cus * per_cu));
}
static int gen_check_control(mpcg_handle* h, const char* fn, uint32_t control_size) {
    if (control_size == 0 || control_size > h->n)
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": control_size must be between 1 and state_size (the n x m workspaces of the formation assume m <= n)");
    return MPCG_OK;
}
template <typename K>
static int gen_raise_lds(mpcg_handle* h, K kern, size_t lds_bytes) {      // (as the PCG launches: beyond 48 KiB of dynamic LDS the kernel's limit is raised first)
    if (lds_bytes > 48 * 1024) HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    return MPCG_OK;
}

// What the float and the double producers differ in: the handle's staging and block-solve buffers (one of each per type) and the grid cap of the dz kernel.
template <typename T> struct ProducerTraits;
template <> struct ProducerTraits<float> {
    static constexpr BufId staging = BUF_STAGING, block_scratch = BUF_BLOCK;
    static constexpr long dz_capmul = 4;
};
template <> struct ProducerTraits<double> {
    static constexpr BufId staging = BUF_STAGING64, block_scratch = BUF_BLOCK64;
    // (126 VGPRs, four wavefronts per SIMD against the float kernel's seven: capped at 1 the 1024 x 128 call ran two quads per workgroup,
    //  0.1165-0.1175 ms against 0.1126-0.1128 with the float kernel's cap, tools/_prof/dz64_ab.py)
    static constexpr long dz_capmul = MPCG_DZ64_CAPMUL;
};

// The register-resident kernels address every array through a buffer resource with 31-bit byte offsets; the largest array per knot is S
// for the formation (3 n^2 elements) and C for dz (n^2 + n m).  Calls beyond run the LDS kernels, which index with size_t.
static constexpr uint64_t schur_bytes_per_knot(int n, size_t elem) { return (uint64_t)3 * n * n * elem; }
static constexpr uint64_t dz_bytes_per_knot(int n, int m, size_t elem) { return (uint64_t)(n * n + n * m) * elem; }
static_assert(schur_bytes_per_knot(14, 4) == 2352 && schur_bytes_per_knot(14, 8) == 4704, "913 k knots per call in float, 456 k in double");
static_assert(dz_bytes_per_knot(14, 7, 4) == 1176 && dz_bytes_per_knot(14, 7, 8) == 2352, "");

// The LDS formation: one workgroup per block row, G^-1 through a handle-owned staging buffer (the second kernel publishes it).
// fn: the entry point's name, why: what sent a (14, 7) call here — both for the refusal of a first call inside a stream capture.
// a.rho_v set: the per-trajectory instantiation of the formation kernel; the completion kernel never sees rho.
template <typename T>
static int form_schur_lds(mpcg_handle* h, const char* fn, const char* why, SchurArgsVT<T> a, hipStream_t st) {
    typedef ProducerTraits<T> Tr;
    const int n = a.n, m = a.m, N = a.N;
    h->last_schur_chunk = 0;
    const size_t lds = gen::form_lds_elems(n, m) * sizeof(T), lds2 = gen::complete_lds_elems(n) * sizeof(T);
    if (lds > kGenLdsMax)
        return fail(h, MPCG_ERR_UNSUPPORTED, std::string(fn) + ": the operands of one block row (" + std::to_string(lds) + " bytes at state_size " + std::to_string(n) +
                    ", control_size " + std::to_string(m) + ") exceed the LDS limit of 160 KiB (6 n^2 + 2 n m + 2 m^2 + 12 n + 4 m elements)");
    // the G^-1 staging buffer, max_batch x ((n^2 + m^2) N - m^2) elements: grows with the largest control_size seen, outside a stream capture only
    const size_t Gsz = (size_t)(n * n + m * m) * N - (size_t)m * m;
    { const int rc = buf_reserve(h, Tr::staging, Gsz * h->max_batch * sizeof(T), &st, (std::string(fn) + why).c_str()); if (rc != MPCG_OK) return rc; }
    a.Ginv_scratch = h->ptr<T>(Tr::staging);
    const long items = (long)a.batch * N;
    const int nt = gen_threads(n);
    const SchurArgsT<T>& as = a;
    if (a.rho_v) {
        { const int rc = gen_raise_lds(h, gen::form_schur_kernel<T, SchurArgsVT<T>>, lds); if (rc != MPCG_OK) return rc; }
        hipLaunchKernelGGL((gen::form_schur_kernel<T, SchurArgsVT<T>>), dim3(gen_grid(h, items, lds)), dim3(nt), lds, st, a);
    } else {
        { const int rc = gen_raise_lds(h, gen::form_schur_kernel<T>, lds); if (rc != MPCG_OK) return rc; }
        hipLaunchKernelGGL(gen::form_schur_kernel<T>, dim3(gen_grid(h, items, lds)), dim3(nt), lds, st, as);
    }
    HIP_TRY(h, hipGetLastError());
    { const int rc = gen_raise_lds(h, gen::complete_ss_kernel<T>, lds2); if (rc != MPCG_OK) return rc; }
    hipLaunchKernelGGL(gen::complete_ss_kernel<T>, dim3(gen_grid(h, items, lds2)), dim3(nt), lds2, st, as);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

// Register-resident formation (schur_walk.hip.h; 14 x 7): a 16-lane row walks a chunk of L consecutive block rows, a
// second kernel closes the seams between chunks.  L trades parallelism against seam work: as long as a call has fewer than ~6 wavefronts of
// four chunks per CU the chunks are made shorter (L = 1: every row a seam — one trajectory of the MPC loop's own call; 16 at 1024 x 128 knots).
template <typename T>
static int form_schur_walk(mpcg_handle* h, const SchurArgsVT<T>& a, hipStream_t st) {
    int wL = h->schur_chunk;
    if (wL <= 0) {
        const long rows = (long)a.batch * (a.N - 1), want = (long)h->num_cus * 6 * 4;
        wL = 1;
        while (wL < 16 && rows / (2 * wL) >= want) wL *= 2;
    }
    const int wchunks = (a.N - 1 + wL - 1) / wL;
    // seam buffer: one Q^-1 per chunk (ensure_seam_buffer: sized once for every automatic chunk length of this handle)
    { const int rc = ensure_seam_buffer(h, (size_t)a.batch * wchunks, sizeof(T), st); if (rc != MPCG_OK) return rc; }
    sw::WalkArgsVT<T> wv;
    sw::WalkArgsT<T>& w = wv;                    // (what the scalar walking kernel and the seam kernel take)
    w.s = a;                                     // (Ginv_scratch stays null: G^-1 is written in place)
    w.seam_qinv = h->ptr<T>(BUF_SEAM); w.L = wL; w.chunks = wchunks;
    wv.rho_v = a.rho_v;
    h->last_schur_chunk = wL;
    const long capw = (long)h->num_cus * 64;
    long bw = ((long)a.batch * wchunks + 3) / 4;
    if (bw > capw) bw = capw;
    if (a.rho_v) hipLaunchKernelGGL((sw::schur_walk_kernel<T, sw::WalkArgsVT<T>>), dim3((unsigned)bw), dim3(64), 0, st, wv);
    else hipLaunchKernelGGL(sw::schur_walk_kernel<T>, dim3((unsigned)bw), dim3(64), 0, st, w);
    HIP_TRY(h, hipGetLastError());
    if (wchunks > 1) {
        long bs = ((long)a.batch * (wchunks - 1) + 3) / 4;
        if (bs > capw) bs = capw;
        hipLaunchKernelGGL(sw::schur_seam_kernel<T>, dim3((unsigned)bs), dim3(64), 0, st, w);
        HIP_TRY(h, hipGetLastError());
    }
    return MPCG_OK;
}

// One rho per call, or one per trajectory in device memory (the _rhov entry points; never validated: device data)
template <typename T>
struct RhoArg { T scalar; const T* vec; bool per_traj; };

// mpcg_form_schur(_rhov) and mpcg_form_schur(_rhov)_f64 (fn: the entry point's name, for its messages).  Same arithmetic order in float and
// double, on either route and for either form of rho: bit-identical to the oracle's instantiation for T.
template <typename T>
static int form_schur_impl(mpcg_handle* h, const char* fn, uint32_t control_size, T* d_G, const T* d_C, const T* d_g, const T* d_c, T* d_S, T* d_Pinv,
                           T* d_gamma, RhoArg<T> rho, uint32_t batch, mpcg_precond precond, void* stream) {
    if (!h) return MPCG_ERR_INVALID;
    if (!d_G || !d_C || !d_g || !d_c || !d_S || (!d_Pinv && precond != MPCG_PRECOND_NONE) || !d_gamma || (rho.per_traj && !rho.vec))
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    { const int rc = gen_check_control(h, fn, control_size); if (rc != MPCG_OK) return rc; }
    if (precond != MPCG_PRECOND_NONE && precond != MPCG_PRECOND_JACOBI && precond != MPCG_PRECOND_SS)
        return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": bad preconditioner");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    if ((uint64_t)batch * h->N >= (1ull << 31)) return fail(h, MPCG_ERR_UNSUPPORTED, std::string(fn) + ": batch * knot_points must stay below 2^31");    // (the kernels keep a knot's index in an int)
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    SchurArgsVT<T> a;
    a.G = d_G; a.C = d_C; a.g = d_g; a.c = d_c; a.S = d_S; a.Pinv = d_Pinv; a.gamma = d_gamma;
    a.Ginv_scratch = nullptr; a.Ginv_out = d_G;
    a.rho = rho.per_traj ? (T)0 : rho.scalar; a.rho_v = rho.per_traj ? rho.vec : nullptr; a.n = (int)h->n; a.m = (int)control_size; a.N = (int)h->N; a.batch = (int)batch;
    a.ss = precond == MPCG_PRECOND_SS; a.pinv = precond != MPCG_PRECOND_NONE;
    a.k0_only = 0;
    if (gen_route(h, control_size)) return form_schur_lds<T>(h, fn, "", a, st);
    if (!h->schur_dpp) return form_schur_lds<T>(h, fn, " (\"schur_dpp\" = 0)", a, st);
    if ((uint64_t)batch * h->N * schur_bytes_per_knot(a.n, sizeof(T)) >= (1ull << 31))
        return form_schur_lds<T>(h, fn, " (a call beyond the 31-bit offsets of the register-resident kernels)", a, st);
    return form_schur_walk<T>(h, a, st);
}

// The LDS dz recovery: one lane per element of dz_k, a few knots per workgroup.
template <typename T>
static int compute_dz_lds(mpcg_handle* h, const DzArgsT<T>& a, hipStream_t st) {
    const int w = a.n + a.m, nt = w <= 64 ? 64 : 128, kpw = nt / w;
    const long groups = ((long)a.batch * a.N + kpw - 1) / kpw;
    hipLaunchKernelGGL(gen::compute_dz_kernel<T>, dim3(gen_grid(h, groups, 0)), dim3(nt), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

// mpcg_compute_dz and mpcg_compute_dz_f64
template <typename T>
static int compute_dz_impl(mpcg_handle* h, const char* fn, uint32_t control_size, const T* d_Ginv, const T* d_C, const T* d_g, const T* d_lambda, T* d_dz,
                           uint32_t batch, void* stream) {
    typedef ProducerTraits<T> Tr;
    if (!h) return MPCG_ERR_INVALID;
    if (!d_Ginv || !d_C || !d_g || !d_lambda || !d_dz) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    { const int rc = gen_check_control(h, fn, control_size); if (rc != MPCG_OK) return rc; }
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DzArgsT<T> a{d_Ginv, d_C, d_g, d_lambda, d_dz, (int)h->n, (int)control_size, (int)h->N, (int)batch};
    const uint64_t knots = (uint64_t)batch * h->N;
    h->last_dz_route = 0;
    if (gen_route(h, control_size) || !h->dz_dpp || h->N < 2 || knots * dz_bytes_per_knot(a.n, a.m, sizeof(T)) >= (1ull << 31))
        return compute_dz_lds<T>(h, a, st);
    h->last_dz_route = 1;
    // four knots per wavefront (schur_walk.hip.h): grid-stride over quads of knots
    const long cap = (long)h->num_cus * 64 * Tr::dz_capmul;
    long bq = ((long)knots + 3) / 4;
    if (bq > cap) bq = cap;
    hipLaunchKernelGGL(sw::compute_dz_dpp_kernel<T>, dim3((unsigned)bq), dim3(64), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

// The direct solve, ONE host path: CT is the sweep type, ST the storage type of S, gamma and lambda (CT = double, ST = float: widened on load,
// lambda rounded once on store).  W_k, z_k go through BUF_BLOCK (CT = float) or BUF_BLOCK64 (CT = double), two buffers of their own,
// each allocated on its first use: neither is ever resized, freed or shared — a solve captured into a graph has its pointer baked in.
template <typename CT, typename ST>
static int block_solve_impl(mpcg_handle* h, const char* fn, const ST* d_S, const ST* d_gamma, ST* d_lambda, uint32_t batch, void* stream) {
    if (!h) return MPCG_ERR_INVALID;
    if (!d_S || !d_gamma || !d_lambda) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": null device pointer");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, std::string(fn) + ": batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // W_k (n x n) + z_k per knot: made at the first call of this sweep type (not stream-ordered: hipMalloc)
    { const int rc = buf_reserve(h, ProducerTraits<CT>::block_scratch, (size_t)h->max_batch * h->N * ((size_t)h->n * h->n + h->n) * sizeof(CT), &st, fn); if (rc != MPCG_OK) return rc; }
    CT* work = h->ptr<CT>(ProducerTraits<CT>::block_scratch);
    if (h->generic || h->producers_generic) {         // any state size: one workgroup per trajectory, operands in LDS (schur_generic.hip.h)
        gen::BlockSolveGenArgsT<CT, ST> ga{d_S, d_gamma, d_lambda, work, (int)h->n, (int)h->N, (int)batch};
        const size_t lds = gen::block_solve_lds_elems((int)h->n) * sizeof(CT);          // 133,664 bytes in double at n = 64
        { const int rc = gen_raise_lds(h, gen::bt_block_solve_kernel<CT, ST>, lds); if (rc != MPCG_OK) return rc; }
        hipLaunchKernelGGL((gen::bt_block_solve_kernel<CT, ST>), dim3(batch), dim3(gen_threads((int)h->n)), lds, st, ga);
        HIP_TRY(h, hipGetLastError());
        return MPCG_OK;
    }
    const BlockSolveArgsT<CT, ST> a{d_S, d_gamma, d_lambda, work, (int)h->N, (int)batch};
    if constexpr (std::is_same<CT, float>::value) {
        // few trajectories: one per wavefront (columns dealt over the four DPP rows, ~2.5x shorter critical path);
        // many: four per wavefront.  Same bits either way.  "block_solve_wide": -1 auto, 0 / 1 forced.
        // (N=128: one per wave 0.35 / 0.53 ms at batch 1024 / 2048 against 0.71 / 0.75; at 4096 four per wave wins, 0.88 vs 0.93)
        const bool wide = h->block_solve_wide < 0 ? batch <= 12u * (uint32_t)h->num_cus : h->block_solve_wide != 0;
        if (!wide) {
            hipLaunchKernelGGL(bt_block_solve_kernel, dim3((batch + 3) / 4), dim3(64), 0, st, a);
            HIP_TRY(h, hipGetLastError());
            return MPCG_OK;
        }
    }
    // (CT = double: one trajectory per wavefront at every batch, "block_solve_wide" is not read: block_solve.hip.h)
    hipLaunchKernelGGL((bt_block_solve_wide_kernel<CT, ST>), dim3(batch), dim3(64), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

extern "C" {

int mpcg_block_solve(mpcg_handle* h, const float* d_S, const float* d_gamma, float* d_lambda, uint32_t batch, void* stream) {
    if (!h) return MPCG_ERR_INVALID;
    if (h->block_solve_f64) return block_solve_impl<double, float>(h, "mpcg_block_solve", d_S, d_gamma, d_lambda, batch, stream);
    return block_solve_impl<float, float>(h, "mpcg_block_solve", d_S, d_gamma, d_lambda, batch, stream);
}

int mpcg_block_solve_f64(mpcg_handle* h, const double* d_S, const double* d_gamma, double* d_lambda, uint32_t batch, void* stream) {
    return block_solve_impl<double, double>(h, "mpcg_block_solve_f64", d_S, d_gamma, d_lambda, batch, stream);
}

int mpcg_form_schur(mpcg_handle* h, uint32_t control_size, float* d_G_dense, const float* d_C_dense, const float* d_g,
                    const float* d_c, float* d_S, float* d_Pinv, float* d_gamma, float rho, uint32_t batch,
                    mpcg_precond precond, void* stream) {
    return form_schur_impl<float>(h, "mpcg_form_schur", control_size, d_G_dense, d_C_dense, d_g, d_c, d_S, d_Pinv, d_gamma, {rho, nullptr, false}, batch, precond, stream);
}

int mpcg_form_schur_rhov(mpcg_handle* h, uint32_t control_size, float* d_G_dense, const float* d_C_dense, const float* d_g,
                         const float* d_c, float* d_S, float* d_Pinv, float* d_gamma, const float* d_rho, uint32_t batch,
                         mpcg_precond precond, void* stream) {
    return form_schur_impl<float>(h, "mpcg_form_schur_rhov", control_size, d_G_dense, d_C_dense, d_g, d_c, d_S, d_Pinv, d_gamma, {0.f, d_rho, true}, batch, precond, stream);
}

int mpcg_compute_dz(mpcg_handle* h, uint32_t control_size, const float* d_Ginv_dense, const float* d_C_dense,
                    const float* d_g, const float* d_lambda, float* d_dz, uint32_t batch, void* stream) {
    return compute_dz_impl<float>(h, "mpcg_compute_dz", control_size, d_Ginv_dense, d_C_dense, d_g, d_lambda, d_dz, batch, stream);
}

// linsys_t = double (USE_DOUBLES = 1, include/common/settings.cuh:41-49): the steps either side of the solve in double precision
int mpcg_form_schur_f64(mpcg_handle* h, uint32_t control_size, double* d_G_dense, const double* d_C_dense, const double* d_g,
                        const double* d_c, double* d_S, double* d_Pinv, double* d_gamma, double rho, uint32_t batch,
                        mpcg_precond precond, void* stream) {
    return form_schur_impl<double>(h, "mpcg_form_schur_f64", control_size, d_G_dense, d_C_dense, d_g, d_c, d_S, d_Pinv, d_gamma, {rho, nullptr, false}, batch, precond, stream);
}

int mpcg_form_schur_rhov_f64(mpcg_handle* h, uint32_t control_size, double* d_G_dense, const double* d_C_dense, const double* d_g,
                             const double* d_c, double* d_S, double* d_Pinv, double* d_gamma, const double* d_rho, uint32_t batch,
                             mpcg_precond precond, void* stream) {
    return form_schur_impl<double>(h, "mpcg_form_schur_rhov_f64", control_size, d_G_dense, d_C_dense, d_g, d_c, d_S, d_Pinv, d_gamma, {0.0, d_rho, true}, batch, precond, stream);
}

int mpcg_compute_dz_f64(mpcg_handle* h, uint32_t control_size, const double* d_Ginv_dense, const double* d_C_dense,
                        const double* d_g, const double* d_lambda, double* d_dz, uint32_t batch, void* stream) {
    return compute_dz_impl<double>(h, "mpcg_compute_dz_f64", control_size, d_Ginv_dense, d_C_dense, d_g, d_lambda, d_dz, batch, stream);
}

int mpcg_prep_csr(mpcg_handle* h, int32_t* d_col_ptr, int32_t* d_row_ind, void* stream) {
    if (!h) return MPCG_ERR_INVALID;
    if (!d_col_ptr || !d_row_ind) return fail(h, MPCG_ERR_INVALID, "mpcg_prep_csr: null device pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(prep_csr_kernel, dim3(h->N), dim3(SCH_THREADS), 0, static_cast<hipStream_t>(stream), (int)h->n, (int)h->N,
                       d_col_ptr, d_row_ind);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

int mpcg_bd_to_csr_lowertri(mpcg_handle* h, const float* d_S, float* d_val, float mult, uint32_t batch, void* stream) {
    if (!h) return MPCG_ERR_INVALID;
    if (!d_S || !d_val) return fail(h, MPCG_ERR_INVALID, "mpcg_bd_to_csr_lowertri: null device pointer");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, "mpcg_bd_to_csr_lowertri: batch exceeds max_batch");
    HIP_TRY(h, hipSetDevice(h->device));
    CsrArgs a{d_S, d_val, mult, (int)h->n, (int)h->N, (int)batch};
    long blocks = (long)batch * h->N;
    const long cap = (long)h->num_cus * 64;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(bd_to_csr_kernel, dim3((unsigned)blocks), dim3(SCH_THREADS), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

}  // extern "C"
