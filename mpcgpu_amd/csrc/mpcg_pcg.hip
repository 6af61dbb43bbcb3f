// mpcg_pcg.hip — C ABI (include/mpcg.h) of the hot path: handle and options, the PCG launch policy (which kernel family serves a call), the
// PCG / SpMV entry points, over the gfx950 kernels in pcg_*.hip.h.  Host side is plain C++/HIP: no torch types, no CPU fallback.
// Each thing is written once, in this order: the handle's device buffers (scratch layouts, counter line, reserve_f64) and mpcg_create /
// _destroy; the options (kOptions: one row per key, read by mpcg_set_option and mpcg_get_option); the launch plan (plan_f32 / plan_f64) and
// its launch (launch_plan); the symmetry latch (one check launch, one warning, one re-open rule under the asynchronous float latch and the
// blocking double one); the solve entries (solve_ends: their argument checks, solve_args: their kernel arguments).
#include "mpcg_handle.hpp"
#include "pcg_kernels.hip.h"
#include "pcg_lpk.hip.h"
#include "pcg_lqb.hip.h"
#include "pcg_lpk_cluster.hip.h"
#include "pcg_rpl.hip.h"
#include "pcg_rpl_cluster_f64.hip.h"
#include "pcg_lqk_f64.hip.h"
#include "pcg_lqk_cluster_f64.hip.h"
#include "pcg_f64.hip.h"

#include <type_traits>

using namespace mpcg;

thread_local std::string mpcg_create_err;

// n = 14 is the tuned specialisation (every entry point); any other 1 <= n <= 64 is served by the generic PCG kernel
// (mpcg_pcg_solve / _ref / _f64: pcg_generic_kernel, pcg_f64.hip.h), as long as its iterate vectors fit the LDS, and by the
// run-time-dimension producers of schur_generic.hip.h (mpcg_producers.hip).
static bool shape_supported(uint32_t n, uint32_t N) { return n == (uint32_t)NS && N >= 2 && N <= 2048; }
static bool generic_shape_supported(uint32_t n, uint32_t N) {
    return n >= 1 && n <= 64 && n != (uint32_t)NS && N >= 2 && N <= 2048 && pcg_generic_lds_elems((int)N, (int)n) * sizeof(float) <= 160 * 1024;
}

static constexpr size_t kLdsMax = 160 * 1024;
static constexpr uint32_t kRplMaxN = 64;          // row-per-lane kernel: full block rows of S and Pinv in registers
static constexpr uint32_t kLpbMaxN = 128;         // one block per lane: 8 waves x 64 lanes hold 2 (2N - 1) blocks
static constexpr uint32_t kLqkMaxN = 64;          // linsys_t = double: knots one CU holds as lane quads (pcg_lqk_f64.hip.h)
static constexpr uint32_t kCluster64MaxN = 64 * LQKC_MAX_G;      // linsys_t = double: the longest horizon a cluster kernel holds (eight members of 64 knots)
static constexpr size_t kEagerF64Bytes = (size_t)8 << 20;        // double iterates up to which mpcg_create makes the double clusters' buffers (reserve_f64)
static size_t lds_bytes_for(uint32_t N, int nw) { return pcg_lds_floats((int)N, nw) * sizeof(float); }

// (defined below, used by mpcg_create and the options)
static int stream_bufs_for(const mpcg_handle* h, const PcgKnobs& k, int nw, int esz);
static void choose_auto(const mpcg_handle* h, PcgKnobs& k, uint32_t batch, int esz);
static void sym_poll(mpcg_handle* h, hipStream_t st = nullptr, bool have_stream = false);

extern "C" {

int mpcg_abi_version(void) { return MPCG_ABI_VERSION; }

const char* mpcg_build_info(void) {
    return "libmpcg_hip gfx950 fp32 n=14 (row-per-lane DPP PCG for short horizons, lane-pair register-resident PCG to N = 128, clustered lane-pair PCG beyond, wave64 row-triple streaming PCG; linsys_t = double: row-per-lane to N = 32, lane-quad register-resident PCG to N = 64, clustered to 512; chunk-walking Schur formation in float and double; IIWA-14 KKT blocks with the analytic inverse-dynamics gradient)";
}

// Device scratch of the clustered kernels, one contiguous run per call so that one small fill precedes every launch —
//   float  (BUF_CLUSTER):       [queue line][flags: one 128-byte line per trajectory of the CALL, up to max_batch][cells: 1 KB per member of the
//                               launch, up to two members per CU][the handle's counter line, never re-zeroed by a launch: CounterSlot]
//   double (BUF_CLUSTER64):     [queue line][flags][cells: one member per CU][a spare line]
static size_t cluster_alloc_words(const mpcg_handle* h) {
    return (size_t)2 * h->num_cus * LPKC_WG_WORDS + CL_FLAG_STRIDE + (size_t)h->max_batch * CL_FLAG_STRIDE + 16;
}
static size_t cluster64_alloc_words(const mpcg_handle* h) {
    return CL_FLAG_STRIDE + (size_t)h->max_batch * CL_FLAG_STRIDE + (size_t)h->num_cus * RPLC_WG_WORDS + 16;
}
// words of the counter line: trajectories re-solved by fix-up launches ("cluster_fixups"), block pairs that failed the last "check_symmetry" run,
// the symmetry latch's sticky device flag
enum CounterSlot { CTR_FIXUPS = 0, CTR_SYM_VIOLATIONS = 8, CTR_SYM_FLAG = 9 };
static unsigned long long* counter(const mpcg_handle* h, CounterSlot slot) { return h->ptr<unsigned long long>(BUF_CLUSTER) + cluster_alloc_words(h) - 16 + slot; }

// queue + flags + cells zeroed and lambda copied, one launch (cluster_prologue_kernel).  The handle's copy of lambda0 (BUF_LAM_BACKUP): mpcg_create
// sizes it for every horizon the automatic policy gives to a cluster kernel, reserve_f64 for the double clusters; a forced "cluster" = G on a
// shorter horizon gets it here, for the call's batch — outside a stream capture.
static int launch_cluster_prologue(mpcg_handle* h, unsigned long long* words, size_t zw, const void* lambda, size_t lam_bytes, hipStream_t st) {
    const int rc = buf_reserve(h, BUF_LAM_BACKUP, lam_bytes, &st,
                               "a cluster launch whose copy of lambda mpcg_create did not size (a forced \"cluster\" on a horizon the automatic policy gives to one CU; a "
                               "first double solve on a handle created with more than 8 MB of double iterates: \"reserve_f64\")");
    if (rc != MPCG_OK) return rc;
    const size_t work = zw > lam_bytes / 16 ? zw : lam_bytes / 16;
    size_t blocks = (work + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks * 256 < zw) blocks = (zw + 255) / 256;
    hipLaunchKernelGGL(cluster_prologue_kernel, dim3((unsigned)blocks), dim3(256), 0, st, words, zw, static_cast<const uint32_t*>(lambda),
                       h->ptr<uint32_t>(BUF_LAM_BACKUP), lam_bytes / 4);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}
// no fix-up launch behind a cluster launch: report the trajectories whose completion count is short of G (cluster_report_kernel)
static int launch_cluster_report(mpcg_handle* h, const unsigned long long* flags, int G, uint32_t batch, uint32_t* iters, uint8_t* exits, hipStream_t st) {
    hipLaunchKernelGGL(cluster_report_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, flags, (int)CL_FLAG_STRIDE, (unsigned long long)G, (int)batch, iters, exits);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}
// the double cluster kernels' buffers: queue + flags + cells, and the double-sized copy of lambda0 their fix-up launch starts from.  Blocking
// (hipMalloc): mpcg_create for small handles, "reserve_f64" = 1, or the first double cluster solve outside a capture.
static int reserve_f64(mpcg_handle* h) {
    if (h->generic || h->N <= 32 || h->N > kCluster64MaxN) return MPCG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    { const int rc = buf_reserve(h, BUF_CLUSTER64, cluster64_alloc_words(h) * sizeof(unsigned long long), nullptr, "", true); if (rc != MPCG_OK) return rc; }
    return buf_reserve(h, BUF_LAM_BACKUP, (size_t)h->max_batch * h->N * h->n * sizeof(double));
}

int mpcg_create(mpcg_handle** out, int device, uint32_t state_size, uint32_t knot_points, uint32_t max_batch) {
    if (!out) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_create: out is null");
    *out = nullptr;
    const bool generic = generic_shape_supported(state_size, knot_points);
    if (!generic && (!shape_supported(state_size, knot_points) || lds_bytes_for(knot_points, 16) > kLdsMax))
        return fail(nullptr, MPCG_ERR_UNSUPPORTED,
                    "mpcg_create: state_size = 14 (tuned; every entry point) or 1..64 (run-time-dimension kernels), 2 <= knot_points, "
                    "and the iterate vectors must fit 160 KiB of LDS");
    if (max_batch == 0) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_create: max_batch is 0");
    int ndev = 0;
    HIP_TRY(nullptr, hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(nullptr, MPCG_ERR_HIP, "mpcg_create: no HIP device");
    if (device < 0) HIP_TRY(nullptr, hipGetDevice(&device));
    if (device >= ndev) return fail(nullptr, MPCG_ERR_INVALID, "mpcg_create: device out of range");
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MPCG_ERR_UNSUPPORTED, std::string("mpcg_create: built for gfx950, device is ") + prop.gcnArchName);
    mpcg_handle* h = new (std::nothrow) mpcg_handle();
    if (!h) return fail(nullptr, MPCG_ERR_NOMEM, "mpcg_create: out of host memory");
    h->device = device; h->n = state_size; h->N = knot_points; h->max_batch = max_batch;
    h->generic = generic;
    h->num_cus = prop.multiProcessorCount;
    h->nt_loads = 1;                    // SpMV kernel only: the matrix is read once — non-temporal loads, +4..9 % (profiles/r02_tune_spmv.txt, r04_spmv.txt)
    choose_auto(h, h->k, 1, 4);         // knobs of the single-workgroup kernels as a batch-1 call would pick them
    choose_auto(h, h->k, 1, 2);
    // every failure from here on leaves through mpcg_destroy (which tolerates the members not made yet)
    const auto give_up = [h](int rc, const std::string& msg) { (void)mpcg_destroy(h); return fail(nullptr, rc, msg); };
    // hand-off cells of the cluster kernel (512 B per member, up to two members per CU), allocated here so that every solve is pure stream work
    // and can be captured into a hipGraph
    if (hipSetDevice(device) != hipSuccess || buf_reserve(h, BUF_CLUSTER, cluster_alloc_words(h) * sizeof(unsigned long long)) != MPCG_OK)
        return give_up(MPCG_ERR_NOMEM, "mpcg_create: cannot allocate the cluster scratch");
    (void)hipMemset(h->buf[BUF_CLUSTER].p, 0, h->buf[BUF_CLUSTER].bytes);          // (the one fill whose result is not looked at)
    if (buf_reserve(h, BUF_SCHED_ORDER, ((size_t)max_batch + 1) * sizeof(uint32_t), nullptr, "", true) != MPCG_OK)      // tag 0 = no permutation yet (sched_pick)
        return give_up(MPCG_ERR_NOMEM, "mpcg_create: cannot allocate the dispatch-order buffer");
    // linsys_t = double beyond N = 32 runs cluster kernels with a queue + flags + cells buffer of their own and a DOUBLE-sized copy of lambda0.
    // A float caller never needs either (N = 128, max_batch 4096 = 59 MB per handle for nothing), so mpcg_create makes them only
    // while they are small (<= 8 MB of double iterates: every handle of the C++ shim, max_batch = 1) — then a fresh handle's first
    // mpcg_pcg_solve_f64 may still be a captured one; larger handles allocate at the first double solve, outside a capture, or when the caller
    // sets "reserve_f64" = 1 (mpcg.h, GRAPH CAPTURE).  Float clusters (N > 128) get their float-sized copy here as before.
    if (!generic && knot_points > 32) {
        const size_t bytes64 = (size_t)max_batch * knot_points * state_size * sizeof(double);
        if (knot_points <= kCluster64MaxN && bytes64 <= kEagerF64Bytes) {
            const int rc = reserve_f64(h);
            if (rc != MPCG_OK) return give_up(rc, "mpcg_create: " + h->err);
        } else if (knot_points > kLpbMaxN && buf_reserve(h, BUF_LAM_BACKUP, (size_t)max_batch * knot_points * state_size * sizeof(float)) != MPCG_OK) {
            return give_up(MPCG_ERR_NOMEM, "mpcg_create: cannot allocate the copy of lambda the cluster fix-up starts from");
        }
    }
    if (hipEventCreateWithFlags(&h->sym_event, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->sym_host), sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess)
        return give_up(MPCG_ERR_NOMEM, "mpcg_create: cannot allocate the symmetry latch");
    *h->sym_host = 0;
    *out = h;
    return MPCG_OK;
}

int mpcg_destroy(mpcg_handle* h) {
    if (h) {
        RelaxedCaptureScope relaxed;
        (void)hipSetDevice(h->device);
        for (const DevBuf& b : h->buf)
            if (b.p) (void)hipFree(b.p);
        if (h->sym_event) (void)hipEventDestroy(h->sym_event);
        if (h->sym_host) (void)hipHostFree(h->sym_host);
    }
    delete h;
    return MPCG_OK;
}

const char* mpcg_last_error(const mpcg_handle* h) { return h ? h->err.c_str() : mpcg_create_err.c_str(); }

// ---- options: one table (include/mpcg.h, Options, documents every row) ---------------------------------------------------------------
// A row: the key, where its value lives (an int of the handle, of its knobs or of `last`; none: the key's case in set / get does it all), the
// range a set accepts (lo > hi: any value) with the rest of "<key> ..." it is refused with, flags, and the key's special case if it has one.
enum : unsigned { OPT_R = 1, OPT_W = 2, OPT_RW = 3,
                  OPT_BOOL = 4,             // stored as value ? 1 : 0
                  OPT_CLEARS_AUTO = 8 };    // an explicit launch knob switches the automatic per-call configuration off — once the value has validated
enum OptCase { O_PLAIN, O_WAVES, O_PCG_RPL, O_PCG_LQK, O_PCG_LPK, O_KKT_F32, O_RESERVE_F64, O_ASSUME_SYMMETRIC, O_SYMMETRY_STATE, O_PCG_RESIDENT, O_AUTO_CFG,
               O_CLUSTER_FIXUPS };
struct Opt {
    const char* key;
    int mpcg_handle::* hm; int PcgKnobs::* km; int LastKernel::* lm;
    int lo, hi;
    unsigned flags;
    const char* refusal = nullptr;
    OptCase special = O_PLAIN;
};
#define OPT_H(m) &mpcg_handle::m, nullptr, nullptr
#define OPT_K(m) nullptr, &PcgKnobs::m, nullptr
#define OPT_L(m) nullptr, nullptr, &LastKernel::m
#define OPT_NONE nullptr, nullptr, nullptr
#define ANY 1, 0
static const Opt kOptions[] = {
    // launch knobs of the single-workgroup kernels (the plain ones: unchecked here, validated at launch)
    {"pcg_waves", OPT_K(waves), 4, 16, OPT_RW | OPT_CLEARS_AUTO, " must be 4, 8 or 16", O_WAVES},
    {"pcg_max_wg_per_cu", OPT_K(max_wg_per_cu), 0, 8, OPT_RW | OPT_CLEARS_AUTO, " out of range"},
    {"pcg_reg_rows", OPT_K(reg_rows), ANY, OPT_RW | OPT_CLEARS_AUTO},
    {"pcg_lds_rows", OPT_K(lds_rows), ANY, OPT_RW | OPT_CLEARS_AUTO},
    {"pcg_stream_bufs", OPT_K(stream_bufs), ANY, OPT_RW | OPT_CLEARS_AUTO},
    {"lds_extra", OPT_K(lds_extra), ANY, OPT_RW},
    {"pcg16_waves", OPT_K(waves16), ANY, OPT_RW},
    {"pcg16_reg_rows", OPT_K(reg_rows16), ANY, OPT_RW},
    {"pcg16_lds_rows", OPT_K(lds_rows16), ANY, OPT_RW},
    {"pcg_resident", OPT_NONE, ANY, OPT_R, nullptr, O_PCG_RESIDENT},         // 1: the single-workgroup configuration streams nothing
    {"auto_cfg", OPT_NONE, ANY, OPT_R, nullptr, O_AUTO_CFG},
    // kernel families (quirk: these pcg_* keys leave "auto_cfg" alone)
    {"pcg_rpl", OPT_H(rpl), -1, 1, OPT_RW, " must be -1 (auto), 0 or 1", O_PCG_RPL},
    {"rpl_waves", OPT_H(rpl_waves), 0, 16, OPT_RW, " must be 0 (auto), 4, 8 or 16", O_WAVES},
    {"pcg_lqk", OPT_H(lqk), -1, 1, OPT_RW, " must be -1 (auto), 0 (off) or 1 (forced)", O_PCG_LQK},
    {"pcg_lqb", OPT_H(lqb), -1, 1, OPT_RW, " must be -1 (auto), 0 (off) or 1 (in place of the lane-pair kernel)"},
    {"pcg_lpk", OPT_H(lpk), -1, 1, OPT_RW, " must be -1 (auto), 0 (off) or 1 (forced)", O_PCG_LPK},
    {"cluster", OPT_H(cluster), -1, 32, OPT_RW, " must be -1 (auto), 0 (off) or 1..32 workgroups per trajectory"},
    {"cluster_fixup", OPT_H(cluster_fixup), ANY, OPT_RW | OPT_BOOL},
    {"cluster_l2", OPT_H(cluster_l2), ANY, OPT_RW | OPT_BOOL},
    {"cluster_test_fail", OPT_H(cluster_test_fail), ANY, OPT_W | OPT_BOOL},
    {"cluster_fixups", OPT_NONE, ANY, OPT_R, nullptr, O_CLUSTER_FIXUPS},
    {"reserve_f64", OPT_NONE, ANY, OPT_W, nullptr, O_RESERVE_F64},
    {"sched_hint", OPT_H(sched_hint), ANY, OPT_RW | OPT_BOOL},
    {"num_cus", OPT_H(num_cus), ANY, OPT_R},
    // the symmetry latch
    {"check_symmetry", OPT_H(check_symmetry), ANY, OPT_RW | OPT_BOOL},
    {"last_symmetry_violations", OPT_H(last_sym_violations), ANY, OPT_R},
    {"assume_symmetric", OPT_NONE, ANY, OPT_W, nullptr, O_ASSUME_SYMMETRIC},
    {"symmetry_state", OPT_H(sym_state), ANY, OPT_R, nullptr, O_SYMMETRY_STATE},
    // SpMV, producers, plant
    {"nt_loads", OPT_H(nt_loads), ANY, OPT_RW | OPT_BOOL},
    {"spmv_mfma", OPT_H(spmv_mfma), ANY, OPT_RW | OPT_BOOL},
    {"spmv_blocks_per_cu", OPT_H(spmv_blocks_per_cu), 1, 64, OPT_RW, " out of range"},
    {"schur_dpp", OPT_H(schur_dpp), ANY, OPT_RW | OPT_BOOL},
    {"schur_chunk", OPT_H(schur_chunk), 0, 2048, OPT_RW, " must be 0 (auto) or 1..2048 block rows"},
    {"last_schur_chunk", OPT_H(last_schur_chunk), ANY, OPT_R},
    {"dz_dpp", OPT_H(dz_dpp), ANY, OPT_RW | OPT_BOOL},
    {"last_dz_route", OPT_H(last_dz_route), ANY, OPT_R},
    {"producers_generic", OPT_H(producers_generic), ANY, OPT_RW | OPT_BOOL},
    {"block_solve_wide", OPT_H(block_solve_wide), ANY, OPT_RW},
    {"block_solve_f64", OPT_H(block_solve_f64), 0, 1, OPT_RW, " must be 0 (the float sweep) or 1 (float64 inside)"},
    {"kkt_analytic", OPT_H(kkt_analytic), ANY, OPT_RW | OPT_BOOL},
    {"kkt_f32", OPT_H(kkt_f32), ANY, OPT_RW, nullptr, O_KKT_F32},
    {"merit_f32", OPT_H(merit_f32), 0, 1, OPT_RW, " must be 0 (float64 inside) or 1 (packed float)"},
    {"integrator", OPT_H(integrator), 0, 1, OPT_RW, " must be 0 (explicit Euler) or 1 (semi-implicit Euler)"},
    {"sim_integrator", OPT_H(sim_integrator), 0, 1, OPT_RW, " must be 0 (explicit Euler) or 1 (semi-implicit Euler)"},
    // what the last solve on this handle launched (family: 0 single-workgroup row-pair, 3 generic, 5 row-per-lane, 6 lane-pair, 7 clustered lane-pair,
    // 8 clustered row-per-lane (double), 9 / 10 lane-quad and clustered lane-quad (double), 11 lane-quad)
    {"last_kernel_family", OPT_L(family), ANY, OPT_R},
    {"last_kernel_waves", OPT_L(waves), ANY, OPT_R},
    {"last_kernel_reg_rows", OPT_L(reg_rows), ANY, OPT_R},
    {"last_kernel_lds_rows", OPT_L(lds_rows), ANY, OPT_R},
    {"last_kernel_lds_extra", OPT_L(lds_extra), ANY, OPT_R},
    {"last_kernel_stream_bufs", OPT_L(stream_bufs), ANY, OPT_R},
    {"last_kernel_cluster", OPT_L(cluster), ANY, OPT_R},
    {"last_kernel_lds_bytes", OPT_L(lds_bytes), ANY, OPT_R},
};
#undef OPT_H
#undef OPT_K
#undef OPT_L
#undef OPT_NONE
#undef ANY
static const Opt* find_option(const char* key, unsigned access) {
    for (const Opt& o : kOptions)
        if (!strcmp(key, o.key)) return o.flags & access ? &o : nullptr;
    return nullptr;
}
static int* option_slot(mpcg_handle* h, const Opt& o) { return o.hm ? &(h->*o.hm) : o.km ? &(h->k.*o.km) : &(h->last.*o.lm); }

int mpcg_set_option(mpcg_handle* h, const char* key, int value) {
    if (!h || !key) return MPCG_ERR_INVALID;
    const Opt* o = find_option(key, OPT_W);
    if (!o) return fail(h, MPCG_ERR_INVALID, std::string("unknown option ") + key);
    const auto refuse = [&](int rc, const char* why) { return fail(h, rc, std::string(key) + why); };
    const auto too_long = [&](uint32_t nmax, const char* kernel) {
        return refuse(MPCG_ERR_UNSUPPORTED, (": the " + std::string(kernel) + " kernel holds knot_points <= " + std::to_string(nmax)).c_str());
    };
    if (o->lo <= o->hi && (value < o->lo || value > o->hi)) return refuse(MPCG_ERR_INVALID, o->refusal);
    switch (o->special) {
    case O_WAVES: if (value != 0 && value != 4 && value != 8 && value != 16) return refuse(MPCG_ERR_INVALID, o->refusal); break;
    case O_PCG_RPL: if (value == 1 && h->N > kRplMaxN) return too_long(kRplMaxN, "row-per-lane"); break;
    case O_PCG_LQK: if (value == 1 && h->N > kLqkMaxN) return too_long(kLqkMaxN, "lane-quad"); break;
    case O_PCG_LPK: if (value == 1 && h->N > kLpbMaxN) return too_long(kLpbMaxN, "lane-pair"); break;
    case O_KKT_F32: value = value == 2 ? 2 : value ? 1 : 0; break;
    case O_RESERVE_F64: return value ? reserve_f64(h) : MPCG_OK;
    case O_ASSUME_SYMMETRIC:      // 1: the caller vouches (or fills only the lower block triangle): no check; 0: back to "unknown"
        // (1 vouches for Pinv too.  0 also forgets a violation: the sticky device flag is cleared by the next solve, on its stream)
        h->sym_state = value ? 1 : 0; h->sym_pending = false; h->sym_pinv_ok = value != 0;
        h->sym_pinv_guarded = h->sym_armed_pinv = false;
        if (!value) h->sym_flag_reset = true;
        return MPCG_OK;
    default: break;
    }
    *option_slot(h, *o) = o->flags & OPT_BOOL ? (value ? 1 : 0) : value;
    if (o->flags & OPT_CLEARS_AUTO) h->auto_cfg = false;
    return MPCG_OK;
}

int mpcg_get_option(const mpcg_handle* h, const char* key, int* value) {      // (an unknown key: MPCG_ERR_INVALID, the handle's error text stays)
    if (!h || !key || !value) return MPCG_ERR_INVALID;
    const Opt* o = find_option(key, OPT_R);
    if (!o) return MPCG_ERR_INVALID;
    mpcg_handle* hm = const_cast<mpcg_handle*>(h);
    switch (o->special) {
    case O_PCG_RESIDENT: *value = stream_bufs_for(h, h->k, h->k.waves, 4) == 0; return MPCG_OK;
    case O_AUTO_CFG: *value = h->auto_cfg ? 1 : 0; return MPCG_OK;
    case O_CLUSTER_FIXUPS: {
        // trajectories re-solved by fix-up launches since mpcg_create (their cluster gave up after the bounded spin): a blocking
        // 8-byte D2H copy — it waits for the device work queued before it
        unsigned long long v = 0;
        if (hipSetDevice(h->device) != hipSuccess || hipMemcpy(&v, counter(h, CTR_FIXUPS), sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return MPCG_ERR_HIP;
        *value = v > 0x7fffffffull ? 0x7fffffff : (int)v;
        return MPCG_OK;
    }
    case O_SYMMETRY_STATE: sym_poll(hm); break;
    default: break;
    }
    *value = *option_slot(hm, *o);
    return MPCG_OK;
}

}  // extern "C"

// ---- launch helpers -----------------------------------------------------------------------------
// Triples (3 block rows) per matrix per wave cached in LDS for this launch configuration.
static int lds_rows_for(const mpcg_handle* h, const PcgKnobs& k, int nw, int esz) {
    const size_t base = lds_bytes_for(h->N, nw);
    const int ntr = ((int)h->N + 2) / 3;
    const int TT = (ntr + nw - 1) / nw;                           // triples per matrix of wave 0
    const int rt = esz == 2 ? k.reg_rows16 : k.reg_rows;
    const int want_max = TT > rt ? TT - rt : 0;
    int lt = esz == 2 ? k.lds_rows16 : k.lds_rows;
    if (lt < 0) {
        if (rt <= 0) return 0;
        const size_t per_pair = pcg_lds_cache_floats(nw, 1, esz) * sizeof(float);
        lt = base < kLdsMax ? (int)((kLdsMax - base) / per_pair) : 0;
    }
    if (lt > want_max) lt = want_max;
    return lt;
}

// LDS bytes requested at launch: vectors + matrix cache, raised to floor(160 KiB / k) when the handle
// limits residency to k workgroups per CU.
static size_t lds_request(const mpcg_handle* h, const PcgKnobs& k, int nw, int esz) {
    size_t need = lds_bytes_for(h->N, nw) + pcg_lds_cache_floats(nw, lds_rows_for(h, k, nw, esz), esz) * sizeof(float);
    if (k.max_wg_per_cu > 0) {
        size_t pad = (kLdsMax / (size_t)k.max_wg_per_cu) & ~(size_t)15;
        if (pad > need) need = pad;
    }
    return need;
}

// <.,.,1> kernels: single-triple LDS slots that still fit after the uniform cache, at most two per wave that streams
static int lds_extra_for(const mpcg_handle* h, const PcgKnobs& k, int nw, int sb, int esz, int* streaming_waves_out) {
    *streaming_waves_out = 0;
    if (sb != 1 || k.lds_extra == 0) return 0;
    const int rt = esz == 2 ? k.reg_rows16 : k.reg_rows;
    const int lt = lds_rows_for(h, k, nw, esz);
    const int ntr = ((int)h->N + 2) / 3;
    int streaming_waves = 0;                                   // waves whose triples exceed registers + uniform cache
    for (int w = 0; w < nw; ++w) streaming_waves += (ntr - w + nw - 1) / nw > rt + lt;
    const size_t used = lds_bytes_for(h->N, nw) + pcg_lds_cache_floats(nw, lt, esz) * sizeof(float);
    const size_t slot = pcg_lds_cache_floats(1, 1, esz) * sizeof(float) / 2;      // one wave, one matrix, one triple
    int e = used < kLdsMax ? (int)((kLdsMax - used) / slot) : 0;
    // slot layout [S: nw][Pinv: nw]: a Pinv slot of wave w sits nw + w slots in, so Pinv slots only fit if ...
    if (e > streaming_waves) {
        const int room = e - nw;                    // slots available beyond the S bank
        e = streaming_waves + (room > 0 ? (room < streaming_waves ? room : streaming_waves) : 0);
    }
    if (k.lds_extra > 0 && e > k.lds_extra) e = k.lds_extra;
    *streaming_waves_out = streaming_waves;
    return e;
}

// LDS layout of one <NW,RT,SB> launch: (bytes, LT, extra S slots, extra Pinv slots)
struct TrajLds { size_t bytes; int lt, extra_s, extra_p; };
static TrajLds traj_lds(const mpcg_handle* h, const PcgKnobs& k, int nw, int sb, int esz) {
    TrajLds t;
    t.lt = lds_rows_for(h, k, nw, esz);
    int streaming_waves = 0;
    const int extra = lds_extra_for(h, k, nw, sb, esz, &streaming_waves);
    t.extra_s = extra < streaming_waves ? extra : streaming_waves;             // S first: one pass loses its longest stream
    t.extra_p = extra - t.extra_s;
    // (the kernel lays the extra slots out as [S: NW][Pinv: NW]; only the first extra_s / NW + extra_p are touched)
    const int extra_span = t.extra_p > 0 ? nw + t.extra_p : t.extra_s;
    t.bytes = lds_bytes_for(h->N, nw) + pcg_lds_cache_floats(nw, t.lt, esz) * sizeof(float)
            + (size_t)extra_span * (pcg_lds_cache_floats(1, 1, esz) * sizeof(float) / 2);
    const size_t padded = lds_request(h, k, nw, esz);
    if (t.bytes <= kLdsMax && padded > t.bytes && padded <= kLdsMax) t.bytes = padded;
    return t;
}

// Compiled (waves, register triples, stream buffers) variants.  X(NW, RT, SB)
#define MPCG_PCG_VARIANTS(X)                                                              \
    X(16, 0, 2) X(8, 0, 2) X(4, 0, 2)                                                     \
    X(16, 1, 0) X(16, 1, 1) X(16, 2, 1)                                                   \
    X(8, 2, 2) X(8, 2, 1) X(8, 2, 0) X(8, 3, 1) X(8, 3, 0) X(8, 4, 0)                                \
    X(4, 3, 0) X(4, 4, 2) X(4, 6, 1) X(4, 7, 1) X(4, 7, 0)
// fp16 matrix storage: a triple costs 14 registers instead of 28
#define MPCG_PCG_VARIANTS16(X)                                                            \
    X(16, 0, 2) X(8, 0, 2)                                                                \
    X(8, 4, 1) X(8, 5, 1) X(8, 6, 0)                                                      \
    X(4, 10, 1) X(4, 12, 1) X(4, 12, 0)

// stream buffers actually needed: 0 when every triple of every wave is resident
static int stream_bufs_for(const mpcg_handle* h, const PcgKnobs& k, int nw, int esz) {
    const int ntr = ((int)h->N + 2) / 3;
    const int TT = (ntr + nw - 1) / nw;
    const int rt = esz == 2 ? k.reg_rows16 : k.reg_rows;
    const bool all_resident = TT <= rt + lds_rows_for(h, k, nw, esz);
    if (k.stream_bufs >= 0) return (k.stream_bufs == 0 && !all_resident) ? 1 : k.stream_bufs;
    return all_resident ? 0 : -1;       // -1: any compiled SB > 0 (1 preferred)
}

// The compiled pcg_traj_kernel<waves, rt, SB> for the stream buffers `sb` asks (stream_bufs_for): the exact build, then a streaming one.
// nullptr: none compiled.
static const void* traj_variant(int waves, int rt, int sb, int esz, int* sb_out) {
    for (int want : {sb, sb == 0 ? 1 : -2, sb <= 0 ? 2 : -2}) {
        if (want == -2) continue;
#define X(NW_, RT_, SB_)                                                                                   \
        if (waves == NW_ && rt == RT_ && (want == SB_ || (want == -1 && SB_ > 0))) {                       \
            *sb_out = SB_;                                                                                 \
            return reinterpret_cast<const void*>(pcg_traj_kernel<NW_, RT_, SB_, MT>);                      \
        }
        if (esz == 4) { using MT = float; MPCG_PCG_VARIANTS(X) }
        else { using MT = _Float16; MPCG_PCG_VARIANTS16(X) }
#undef X
    }
    return nullptr;
}

// Automatic per-call configuration of the single-workgroup kernels (round-1 sweeps on MI355X: profiles/r01_tune11.txt,
// r01_tune12.txt, r01e_tune_nsweep.txt).  Writes into the caller's COPY of the knobs.
static void choose_auto(const mpcg_handle* h, PcgKnobs& k, uint32_t batch, int esz) {
    const uint32_t N = h->N;
    if (esz == 2) {     // fp16 storage: <= 48 triples all in registers
        if (N <= 144) { k.waves16 = 8; k.reg_rows16 = 6; } else { k.waves16 = 4; k.reg_rows16 = 12; }
        k.lds_rows16 = -1;
        return;
    }
    if (N <= 48) {
        // short horizons (<= 16 triples): with more trajectories than CUs, 4 waves x 3 register triples (+ 1 in LDS
        // beyond N=36) need < 256 registers, so TWO trajectories share a CU and fill each other's barrier and
        // reduction latencies (batch 2048: N=32 269 vs 171 M it/s, N=48 187 vs 166); up to one trajectory per CU
        // the 8-wave kernel with everything in registers is the faster solve
        if (batch > (uint32_t)h->num_cus) { k.waves = 4; k.reg_rows = 3; k.lds_rows = -1; }
        else { k.waves = 8; k.reg_rows = 2; k.lds_rows = 0; }
    } else if (N <= 96) {   // <= 32 triples: three in registers + one in LDS per wave and matrix
        k.waves = 8; k.reg_rows = 3; k.lds_rows = -1;
    } else {
        // long horizons: 8 waves (two per SIMD) with 3 register triples + 1 LDS triple per wave and matrix, the rest
        // streamed, beat 4 fat waves with 7 + 2 since <8,3,1> runs spill-free (N=128, batch 1024: 4.06 ms vs 5.23 ms,
        // profiles/r01e_phases_N128.txt); beyond N=256 (reached only with the cluster kernel switched off) the fat
        // waves' larger resident share wins again (profiles/r01_tune12.txt)
        if (N < 256 || batch < (uint32_t)h->num_cus) { k.waves = 8; k.reg_rows = 3; }
        else { k.waves = 4; k.reg_rows = 7; }
        k.lds_rows = -1;
    }
}

// The float lane-quad kernel takes the lane-pair kernel's launches (same contract: lower block triangle, gated / fix-up launches, dispatch order).
// Automatic use ("pcg_lqb" = 1 / 0 forces / forbids, an explicit "pcg_lpk" = 1 keeps the lane-pair kernel; steady clocks, tools/_prof/lqb_ab.py,
// lqb_n32.py, lqb_n32_forced.py; the first sweep: profiles/r06_lqb_policy.txt): WHEREVER the lane-pair kernel ran in fp32, both preconditioners
// (block-Jacobi is a build of its own, pcg_lqb_kernel<., false>: no off-diagonal Pinv blocks, no z) —
//   * 32 < knot_points <= 64, every batch: two independent workgroups per CU, all of their wavefronts working: one trajectory of 64 knots 1.03 against
//     1.44 us per iteration (block-Jacobi 0.94 / 1.22), batch 1024 3.02 / 3.71 (2.45 / 3.09); also ahead of the row-per-lane kernel's latency-sized calls;
//   * 64 < knot_points <= 128: 1.58 / 1.62 us per iteration of one trajectory, 6.31 / 6.54 per 1024 (block-Jacobi 1.32 / 1.34, 5.29 / 5.51);
//   * 16 < knot_points <= 32, throughput-sized calls (lpk_half): equal to the lane-pair kernel's half build at 2.5-4 trajectories per CU (+-1 %),
//     1.10x (SS) / 1.13-1.19x (block-Jacobi) beyond.
static bool lqb_auto(const mpcg_handle* h, int esz) { return esz == 4 && h->lqb == -1 && h->lpk == -1 && h->rpl != 1 && h->auto_cfg && h->cluster <= 0; }
static bool use_lqb(const mpcg_handle* h, int esz) {
    if (esz != 4 || h->lqb == 0) return false;
    return h->lqb == 1 || lqb_auto(h, esz);       // (quirk: "pcg_lqb" = 1 reaches only calls the lane-pair kernel takes without it: 36 < N, not 32 < N)
}
// Lane-pair kernel, automatic use: 36 < N <= 128 (where the row-per-lane kernel has not taken the call).  Its per-lane work does not shrink with the
// horizon (a lane pair per knot whatever N), so up to N = 36 — where the row-pair kernel <4,3,0> fits two trajectories per CU — that one stays
// ahead in throughput (N=36: 292 vs 222 M it/s at batch 2048); beyond it the order flips (HISTORY.md §3.1c).
// ... and, round 5, 16 < N <= 32 for calls of at least 2.5 trajectories per CU: the HALF build (one wavefront per matrix, 32 knots, four workgroups
// per CU) takes 1.45-1.55 us per iteration for up to four trajectories per CU, the row-per-lane kernel 1.26 us for two, 2.1 for three, 2.5-2.7 for
// four: N = 32, batch 1024 / 4096: 378 / 434 -> 661 / 629 M it/s (tools/_prof/lpk_half.py); at N <= 16 the row-per-lane kernel stays ahead (780-920 M).
static bool lpk_half(const mpcg_handle* h, int esz, uint32_t batch) {
    return esz == 4 && h->lpk != 0 && h->rpl != 1 && h->auto_cfg && h->cluster <= 0 && h->N > 16 && h->N <= 32 && 2ull * batch >= 5ull * (uint32_t)h->num_cus;
}
static bool use_lpk(const mpcg_handle* h, int esz, uint32_t batch) {
    if ((esz != 4 && esz != 2) || h->N > kLpbMaxN || h->lpk == 0) return false;     // (fp16 storage: converted once at the load)
    // (with the lane-quad kernel behind the lane-pair kernel's launches: from 33 knots, at every batch — it beats the row-pair kernel at 33..36 and
    //  the row-per-lane kernel's latency-sized calls up to 64, use_lqb)
    return h->lpk == 1 || (h->auto_cfg && h->cluster <= 0 && h->N > (lqb_auto(h, esz) ? 32u : 36u)) || lpk_half(h, esz, batch);
}
// Row-per-lane kernel (pcg_rpl.hip.h), automatic use (no explicit pcg_* knob): N <= 32 always (N=32: 0.150 vs 0.247 ms for one trajectory, 395 vs
// 277 M it/s at batch 2048; N=16: 875 vs 317 M); 32 < N <= 64 for latency-sized calls only (N=64 one trajectory 0.248 vs 0.341 ms, but 170 vs
// 211 M it/s at batch 2048, where the lane-pair / row-pair kernels stay ahead).
static bool use_rpl(const mpcg_handle* h, int esz, uint32_t batch) {
    if (esz != 4 || h->N > kRplMaxN || h->rpl == 0) return false;
    if (h->rpl == 1) return true;
    if (h->lpk == 1) return false;
    if (lpk_half(h, esz, batch)) return false;
    return h->auto_cfg && h->cluster <= 0 && (h->N <= 32 || (batch <= (uint32_t)h->num_cus && !lqb_auto(h, esz)));
}

// Members of a cluster: "cluster" = G forced, else ceil(N / nmax); 0 when the kernel cannot take the call (at most max_g members of at most
// nmax knots, no more members than CUs or knots).
static int cluster_members(const mpcg_handle* h, int nmax, int max_g) {
    const int G = h->cluster > 0 ? h->cluster : ((int)h->N + nmax - 1) / nmax;
    if (G < 2 || G > max_g || G > h->num_cus || G > (int)h->N) return 0;
    if (((int)h->N + G - 1) / G > nmax) return 0;        // the largest member: ceil(N / G) knots
    return G;
}
// clusters the chip holds: the kernel pins cluster cl to XCD cl % 8 (all its members on one XCD, 32 CUs each), so residency is a
// per-XCD count — 8 x floor(CUs of one XCD / G).  (Sized chip-wide, G = 3, 5, 6, 7 over-subscribed some XCDs by a member that could
// not start while the persistent clusters held the CUs: its peers spun to the limit and the trajectories fell to the fix-up launch.)
static uint32_t cluster_resident(const mpcg_handle* h, int G) {
    const int xcd_slots = h->num_cus / 8;
    return h->num_cus >= 8 && xcd_slots >= G ? (uint32_t)(8 * (xcd_slots / G)) : (uint32_t)(h->num_cus / G);
}

// ---- the launch plan ------------------------------------------------------------------------------
// Which kernel serves a call is decided here and nowhere else (include/mpcg.h, Options: one row of its kernel-selection table per branch of
// plan_f32 / plan_f64).  Pure host code — no HIP call, no change to the handle — so mpcg_pcg_lds_bytes(_f64) plan on a handle of the stack
// without a GPU.  The launch paths, mpcg_check_pcg_occupancy and the dispatch-order hint all read the plan.

// One kernel launch (grid 0: one workgroup per trajectory), or why there is none (rc != MPCG_OK: the call fails with err where it would launch)
struct Launch {
    const void* kern = nullptr;
    unsigned grid = 0, block = 0;
    size_t lds = 0;
    int lds_rows = 0, extra_s = 0, extra_p = 0;     // pcg_traj_kernel: its LDS layout (PcgArgs::lds_rows, lds_extra_s, lds_extra_p)
    int rc = MPCG_OK;
    const char* err = nullptr;
};
struct PcgPlan {
    Launch k;
    LastKernel last;            // what "last_kernel_*" reports after the call
    bool lower = false;         // reads only the lower block triangle: the latch (float: its own predicate, see plan_f32) / guard applies
    bool check = false;         // float: "check_symmetry" verifies this call first (its own predicate, see plan_f32)
    bool order = false;         // a call with more trajectories than CUs is followed by the dispatch-order kernel (sched_order_kernel)
    // clustered kernels (G > 0): the persistent launch holds min(batch, resident) clusters
    int G = 0;
    uint32_t resident = 0;
    int member_words = 0;       // hand-off cells per member (u64 words)
    int lam_esz = 0;            // element size of lambda (4: float, the float scratch; 8: double, the double kernels' scratch)
    bool fixup = false;         // trajectories whose cluster gave up are re-solved by `fix` (gated on the completion counts), else reported
    Launch fix;
    int fix_lower = 0;          // double: PcgArgs64::lower of the fix-up (the streaming kernel)
};
enum Cols { LOWER, GATED, FULL, FALLBACK };   // a lower-triangle kernel allowed / allowed but gated by the guard / three columns / the guard's fallback

static Launch unsupported(int rc, const char* err) { Launch L; L.rc = rc; L.err = err; return L; }
template <typename K>
static Launch make_launch(K* kern, unsigned block, size_t lds, unsigned grid = 0) {
    Launch L;
    L.kern = reinterpret_cast<const void*>(kern); L.grid = grid; L.block = block; L.lds = lds;
    return L;
}

static Launch plan_traj(const mpcg_handle* h, const PcgKnobs& k, int esz, LastKernel* last) {
    const int waves = esz == 2 ? k.waves16 : k.waves;
    const int rt = esz == 2 ? k.reg_rows16 : k.reg_rows;
    int sb = 0;
    const void* kern = traj_variant(waves, rt, stream_bufs_for(h, k, waves, esz), esz, &sb);
    if (!kern) return unsupported(MPCG_ERR_UNSUPPORTED, "no compiled kernel variant for this (pcg_waves, pcg_reg_rows, pcg_stream_bufs)");
    const TrajLds t = traj_lds(h, k, waves, sb, esz);
    Launch L;
    L.kern = kern; L.block = waves * 64; L.lds = t.bytes;
    L.lds_rows = t.lt; L.extra_s = t.extra_s; L.extra_p = t.extra_p;
    if (t.bytes > kLdsMax) { L.rc = MPCG_ERR_INVALID; L.err = "pcg_lds_rows does not fit 160 KiB of LDS"; }
    *last = LastKernel{FAM_TRAJ, waves, rt, t.lt, sb, 0, (int)t.bytes, t.extra_s + t.extra_p};
    return L;
}
// (NW, RHO) of a row-per-lane call: NW RHO slots of four knots must cover the horizon.  Automatic (profiles/r02_rpl_quick.txt): N <= 16 four
// wavefronts; N <= 32 eight wavefronts x one slot for a latency-sized call (at most one trajectory per CU), four x two slots for
// throughput (N=32 SS 395 vs 376 M it/s, block-Jacobi 623 vs 484 M); N <= 64 eight x two.
#define MPCG_RPL_VARIANTS(X) X(4, 1) X(4, 2) X(8, 1) X(8, 2) X(16, 1)
static Launch plan_rpl(const mpcg_handle* h, uint32_t batch, int pcols, LastKernel* last) {
    const int slots = ((int)h->N + 3) / 4;
    int nw = h->rpl_waves;
    if (nw == 0) nw = slots <= 4 ? 4 : slots <= 8 ? (batch > (uint32_t)h->num_cus ? 4 : 8) : 8;
    const int rho = (slots + nw - 1) / nw;
    const size_t lds = pcg_rpl_lds_floats((int)h->N, nw) * sizeof(float);
    *last = LastKernel{FAM_RPL, nw, rho, 0, 0, 0, (int)lds, 0};
#define X(NW_, RHO_) \
    if (nw == NW_ && rho == RHO_) return make_launch(pcols == 3 ? pcg_rpl_kernel<NW_, RHO_, true> : pcg_rpl_kernel<NW_, RHO_, false>, NW_ * 64, lds);
    MPCG_RPL_VARIANTS(X)
#undef X
    return unsupported(MPCG_ERR_UNSUPPORTED, "row-per-lane kernel: no compiled (waves, slots) variant covers this horizon with rpl_waves");
}
// lane-pair kernel (pcg_lpk.hip.h; N <= 32: the half build, one wavefront per matrix, four workgroups per CU), or the lane-quad kernel in its place
static Launch plan_lpk(const mpcg_handle* h, int esz, int pcols, LastKernel* last) {
    if (use_lqb(h, esz)) {
        const int nq = h->N <= 32 ? 32 : h->N <= 64 ? 64 : 128;
        const size_t lds = pcg_lqb_lds_floats(nq) * sizeof(float);
        *last = LastKernel{FAM_LQB, nq / 16, 0, 0, 0, 0, (int)lds, 0};
        const bool pc3 = pcols == 3;         // (SS / block-Jacobi builds)
        if (nq == 32) return make_launch(pc3 ? pcg_lqb_kernel<32, true> : pcg_lqb_kernel<32, false>, 128, lds);
        if (nq == 64) return make_launch(pc3 ? pcg_lqb_kernel<64, true> : pcg_lqb_kernel<64, false>, 256, lds);
        return make_launch(pc3 ? pcg_lqb_kernel<128, true> : pcg_lqb_kernel<128, false>, 512, lds);
    }
    const int nw = h->N <= 32 ? LpkLds<0>::NW : h->N <= 64 ? LpkLds<1>::NW : LpkLds<2>::NW;
    const size_t lds = pcg_lpk_lds_floats(nw) * sizeof(float);
    *last = LastKernel{FAM_LPK, nw, 0, 0, 0, 0, (int)lds, 0};
    return make_launch(h->N <= 32 ? pcg_lpk_kernel<0> : h->N <= 64 ? pcg_lpk_kernel<1> : pcg_lpk_kernel<2>, nw * 64, lds);
}
// the generic streaming kernel (pcg_f64.hip.h): state_size != 14 (NFIX = 0) in float and double; the double path's streaming kernel (NFIX = 14)
template <typename T, int NFIX>
static Launch plan_generic(const mpcg_handle* h, LastKernel* last) {
    const size_t lds = pcg_generic_lds_elems((int)h->N, (int)h->n) * sizeof(T);
    const int nthr = pcg_generic_threads((int)h->N, (int)h->n);
    *last = LastKernel{FAM_GENERIC, nthr / 64, 0, 0, 2, 0, (int)lds, 0};
    if (lds > kLdsMax) return unsupported(MPCG_ERR_UNSUPPORTED, "generic / double-precision kernel: the iterate vectors do not fit 160 KiB of LDS");
    return make_launch(nthr == F64_THREADS_WIDE ? pcg_generic_kernel<T, NFIX, F64_THREADS_WIDE> : pcg_generic_kernel<T, NFIX, F64_THREADS>, nthr, lds);
}

// float / fp16 storage.  In order: the generic kernel (state_size != 14); the row-per-lane kernel (use_rpl); the lane-pair / lane-quad kernel
// (use_lpk); the clustered lane-pair kernel ("cluster" = G forced, or automatic knobs and a horizon one CU cannot hold); pcg_traj_kernel with the
// handle's knobs, chosen per call (choose_auto) unless the caller set a pcg_* knob.  Three columns (a call whose matrices are not known to be
// block-symmetric): the row-per-lane kernel up to 64 knots, else pcg_traj_kernel.
static PcgPlan plan_f32(const mpcg_handle* h, uint32_t batch, int esz, int pcols, Cols cols) {
    PcgPlan p;
    const uint32_t N = h->N;
    if (h->generic) { p.k = plan_generic<float, 0>(h, &p.last); return p; }     // (fp16 storage: refused by mpcg_pcg_solve_f16)
    PcgKnobs k = h->k;
    if (cols == FULL || cols == FALLBACK) {
        if (esz == 4 && N <= kRplMaxN && h->rpl != 0) { p.k = plan_rpl(h, batch, pcols, &p.last); p.order = true; return p; }   // full block rows in registers
        if (h->auto_cfg || cols == FALLBACK) choose_auto(h, k, batch, esz);   // (quirk: the guard's fallback picks its knobs even under explicit pcg_* knobs)
        p.k = plan_traj(h, k, esz, &p.last);
        return p;
    }
    if (use_rpl(h, esz, batch)) { p.k = plan_rpl(h, batch, pcols, &p.last); p.order = true; return p; }      // (an explicit "pcg_lpk" = 1 wins over the automatic choice of this one)
    // the kernels below read only the left + diagonal block columns (mpcg.h "Block symmetry"): the predicates of the check and of the latch
    p.check = use_lpk(h, esz, batch) || (h->cluster != 0 && (h->cluster > 0 || N > kLpbMaxN));                // (quirk: without the auto_cfg test of `lower`)
    p.lower = use_lpk(h, esz, batch) || (h->cluster != 0 && (h->cluster > 0 || (h->auto_cfg && N > kLpbMaxN)));   // (quirk: also when cluster_members refuses G)
    if (use_lpk(h, esz, batch)) { p.k = plan_lpk(h, esz, pcols, &p.last); p.order = true; return p; }
    p.G = h->cluster == 0 || (h->cluster < 0 && (!h->auto_cfg || N <= kLpbMaxN)) ? 0 : cluster_members(h, 128, LPKC_MAX_G);
    if (p.G) {
        // G CUs per trajectory, 128 knots per member in registers (pcg_lpk_cluster.hip.h); the fix-up: the lane-pair kernel's launch up to
        // 128 knots — a GATED call's fix-up must read all three columns (every completion count is 0 after a gated exit: ADVICE r04) — else
        // pcg_traj_kernel with the knobs of a batch-1 call (quirk: whatever the call's batch and auto_cfg)
        p.resident = cluster_resident(h, p.G);
        p.member_words = LPKC_WG_WORDS; p.lam_esz = sizeof(float);
        p.k = make_launch(pcg_lpkc_kernel<2>, 512, pcg_lpkc_lds_floats(8) * sizeof(float));
        p.last = LastKernel{FAM_LPKC, 8, 0, 0, 0, p.G, (int)p.k.lds, 0};
        PcgKnobs kf = h->k;
        choose_auto(h, kf, 1, esz);
        p.fixup = h->cluster_fixup && (N <= kLpbMaxN || lds_bytes_for(N, kf.waves) <= kLdsMax);
        LastKernel unused;
        p.fix = N <= kLpbMaxN && cols != GATED ? plan_lpk(h, esz, pcols, &unused) : plan_traj(h, kf, esz, &unused);
        p.order = true;
        return p;
    }
    if (h->auto_cfg) choose_auto(h, k, batch, esz);
    p.k = plan_traj(h, k, esz, &p.last);
    return p;
}

// double (linsys_t = double).  lower_ok: the latch says the caller's matrices are block-symmetric (the lane-quad kernels need it).
static constexpr uint32_t kRplMaxN64 = 32;
static PcgPlan plan_f64(const mpcg_handle* h, uint32_t batch, int pcols, bool lower_ok) {
    PcgPlan p;
    const uint32_t N = h->N;
    // 32 < N <= 64 (or "pcg_lqk" = 1 at any N <= 64): the lane-quad kernel of one CU (pcg_lqk_f64.hip.h).  Also 16 < N <= 32 when the call brings at
    // least four trajectories per CU: two 32-knot workgroups per CU take 4.2 us per iteration of 1,024 trajectories at every such N and 30-39 us to
    // start, the row-per-lane kernel 4.4 us and 38-64 us — 40-iteration solves of 1,024 trajectories: 200-205 against 218-246 us
    // (tools/_prof/f64_fixed_cost.py); below that batch the row-per-lane kernel's 1.0-1.1 us per iteration of ONE trajectory wins (1.7).
    const bool lqk_short = N > 16 && batch >= 4u * (uint32_t)h->num_cus;
    if (lower_ok && !h->generic && N <= kLqkMaxN && h->lqk != 0 && (h->lqk == 1 || (h->auto_cfg && (N > kRplMaxN64 || lqk_short) && h->cluster < 0))) {
        const int nw = N <= 32 ? 4 : 8;
        const size_t lds = pcg_lqk_lds_doubles(nw) * sizeof(double);
        p.k = make_launch(nw == 4 ? pcg_lqk_f64_kernel<1> : pcg_lqk_f64_kernel<2>, nw * 64, lds);
        p.last = LastKernel{FAM_LQK64, nw, 0, 0, 0, 0, (int)lds, 0};
        p.lower = true;
        return p;
    }
    // N <= 32 (the real-time horizon): the row-per-lane kernel in double, one slot per wavefront
    if (!h->generic && N <= kRplMaxN64 && h->rpl != 0 && (h->rpl == 1 || h->auto_cfg)) {
        const int nw = N <= 16 ? 4 : 8;
        const size_t lds = pcg_rpl_lds_floats((int)N, nw) * sizeof(double);
        const bool pc3 = pcols == 3;
        p.k = nw == 4 ? make_launch(pc3 ? pcg_rpl_kernel_f64<4, 1, true> : pcg_rpl_kernel_f64<4, 1, false>, 256, lds)
                      : make_launch(pc3 ? pcg_rpl_kernel_f64<8, 1, true> : pcg_rpl_kernel_f64<8, 1, false>, 512, lds);
        p.last = LastKernel{FAM_RPL, nw, 1, 0, 0, 0, (int)lds, 0};
        return p;
    }
    if (h->generic) { p.k = plan_generic<double, 0>(h, &p.last); return p; }
    LastKernel unused;
    p.fix = plan_generic<double, 14>(h, &unused);          // the clusters' fix-up: the streaming kernel
    // 64 < N <= 512, block-symmetric matrices: the lane-quad kernel across G = ceil(N / 64) CUs of one XCD (pcg_lqk_cluster_f64.hip.h)
    p.G = lower_ok && N > kRplMaxN64 && h->cluster != 0 && h->lqk != 0 ? cluster_members(h, 64, LQKC_MAX_G) : 0;
    if (p.G) {
        p.k = make_launch(pcg_lqkc_f64_kernel<2>, 512, pcg_lqkc_lds_doubles() * sizeof(double));
        p.last = LastKernel{FAM_LQKC64, 8, 0, 0, 0, p.G, (int)p.k.lds, 0};
        p.member_words = LQKC_WG_WORDS;
        p.lower = true;
        // (the fix-up is the streaming kernel, two block columns (the latch says symmetric): beyond the horizon whose iterate vectors fit its LDS
        //  — N = 350 in double — an abandoned trajectory is reported, d_iters = 0xFFFFFFFF / d_max_iter_exit = 2, as with "cluster_fixup" = 0)
        p.fix_lower = 1;
    } else {
        // 32 < N <= 256: the row-per-lane kernel across G = ceil(N / 32) CUs of one XCD, full block rows of S and Pinv in registers
        // (pcg_rpl_cluster_f64.hip.h; "cluster" = 0: the streaming kernel below)
        p.G = h->cluster != 0 ? cluster_members(h, RPLC_KMAX, RPLC_MAX_G) : 0;
        if (!p.G) { p.k = plan_generic<double, 14>(h, &p.last); p.fix = Launch(); return p; }
        p.k = make_launch(pcols == 3 ? pcg_rplc_f64_kernel<true> : pcg_rplc_f64_kernel<false>, RPLC_NW * 64, pcg_rplc_lds_doubles() * sizeof(double));
        p.last = LastKernel{FAM_RPLC64, RPLC_NW, 0, 0, 0, p.G, (int)p.k.lds, 0};
        p.member_words = RPLC_WG_WORDS;
    }
    p.resident = cluster_resident(h, p.G);
    p.lam_esz = sizeof(double);
    p.fixup = h->cluster_fixup && p.fix.rc == MPCG_OK;
    return p;
}

// ---- launching a plan -------------------------------------------------------------------------------
// hipFuncSetAttribute when a launch needs more than 48 KiB of LDS
static int raise_lds(mpcg_handle* h, const Launch& L) {
    if (L.lds > 48 * 1024) HIP_TRY(h, hipFuncSetAttribute(L.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    return MPCG_OK;
}
// the LDS limit, the launch (grid 0: `batch` workgroups), the error check
static int launch(mpcg_handle* h, const Launch& L, void* arg, uint32_t batch, hipStream_t st) {
    if (L.rc != MPCG_OK) return fail(h, L.rc, L.err);
    { const int rc = raise_lds(h, L); if (rc != MPCG_OK) return rc; }
    void* args[] = {arg};
    (void)hipLaunchKernel(L.kern, dim3(L.grid ? L.grid : batch), dim3(L.block), args, L.lds, st);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}
static int launch_args(mpcg_handle* h, const Launch& L, PcgArgs a, uint32_t batch, hipStream_t st) {
    a.lds_rows = L.lds_rows; a.lds_extra_s = L.extra_s; a.lds_extra_p = L.extra_p;
    return launch(h, L, &a, batch, st);
}
template <typename T>
static int launch_args(mpcg_handle* h, const Launch& L, PcgArgsG<T> a, uint32_t batch, hipStream_t st) {
    a.n = (int)h->n;
    return launch(h, L, &a, batch, st);
}

// A clustered launch (pcg_lpkc_kernel, pcg_rplc_f64_kernel, pcg_lqkc_f64_kernel): one persistent launch for any batch, clusters draw trajectories
// from a queue.  Members must be co-resident, which a plain launch cannot guarantee when another stream holds CUs: a member that waits longer
// than the bounded spin gives up; every member that FINISHES a trajectory counts itself in that trajectory's flag, and the launch is followed by
// the fix-up launch, in which only the trajectories whose count is not G run — the caller always gets a solved system ("cluster_fixup" = 0, or
// no fix-up that fits: the report of those trajectories instead).
// Scratch: [queue: one 128-byte line][flags: one line per trajectory of the call][cells of the launch] — what a call uses is contiguous, so one
// small fill precedes every launch (with lambda0 copied for the fix-up when one follows).  count_fixups: the fix-up adds to "cluster_fixups"
// (not behind a gated launch, whose gated exits are no abandoned trajectories).
template <typename CA, typename A>
static int launch_cluster(mpcg_handle* h, const PcgPlan& p, const A& a, uint32_t batch, hipStream_t st, bool count_fixups) {
    unsigned long long* words = h->ptr<unsigned long long>(p.lam_esz == sizeof(double) ? BUF_CLUSTER64 : BUF_CLUSTER);
    const uint32_t clusters = batch < p.resident ? batch : p.resident;
    CA ca;
    if constexpr (std::is_same<CA, ClusterArgs>::value) ca.kl_max = 128;
    ca.p = a;
    ca.queue = words;
    ca.fail_flags = ca.queue + CL_FLAG_STRIDE;
    ca.scratch = ca.fail_flags + (size_t)batch * CL_FLAG_STRIDE;
    ca.G = p.G; ca.batch = (int)batch; ca.clusters = (int)clusters; ca.l2_handoff = h->cluster_l2;
    ca.test_fail = h->cluster_test_fail;
    const size_t zw = CL_FLAG_STRIDE + (size_t)batch * CL_FLAG_STRIDE + (size_t)clusters * p.G * p.member_words;
    if (p.fixup) {
        const int rc = launch_cluster_prologue(h, words, zw, a.lambda, (size_t)batch * h->N * NS * p.lam_esz, st);
        if (rc != MPCG_OK) return rc;
    } else {
        hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)((zw + 255) / 256)), dim3(256), 0, st, words, zw);
        HIP_TRY(h, hipGetLastError());
    }
    { const int rc = launch(h, p.k, &ca, ((clusters + 7) / 8) * 8 * (unsigned)p.G, st); if (rc != MPCG_OK) return rc; }
    if (!p.fixup) return launch_cluster_report(h, ca.fail_flags, p.G, batch, a.iters, a.max_iter_exit, st);
    A c = a;
    c.redo_flags = ca.fail_flags; c.redo_stride = CL_FLAG_STRIDE; c.redo_skip = (unsigned)p.G;
    c.redo_count = count_fixups ? counter(h, CTR_FIXUPS) : nullptr;
    c.lam0 = static_cast<decltype(c.lam0)>(h->buf[BUF_LAM_BACKUP].p);     // (members that finished a trajectory their cluster did not have written their knots of lambda)
    if constexpr (std::is_same<A, PcgArgs64>::value) c.lower = p.fix_lower;
    return launch_args(h, p.fix, c, batch, st);
}
// the planned launch(es); h->last on success.  (A cluster's launch size: its resident clusters, whatever `batch`.)
template <typename CA, typename A>
static int launch_plan(mpcg_handle* h, const PcgPlan& p, const A& a, uint32_t batch, hipStream_t st, bool count_fixups = true) {
    const int rc = p.G ? launch_cluster<CA>(h, p, a, batch, st, count_fixups) : launch_args(h, p.k, a, batch, st);
    if (rc == MPCG_OK) h->last = p.last;
    return rc;
}

// ---- the symmetry latch (mpcg.h, BLOCK SYMMETRY) ----------------------------------------------------------------------------------
// Tolerance of the block-symmetry checks: block pairs (k, right) / (k+1, left) that differ by more than 1 % of their largest entry.  The
// reference's construction gives 0 for S; its symmetric-stair Pinv[k,right] / Pinv[k+1,left] are the same triple product associated two ways
// in float — measured on the bench's systems: 2.5e-5 of the largest entry in the median, 6e-5 at worst, more on worse-conditioned blocks —
// so the check looks for STRUCTURAL asymmetry (a caller-made Pinv), not for rounding.
static constexpr float kSymRelTol = 1e-2f;
// (double: the two associations agree to ~1e-13; anything at the 1e-6 level is a different matrix, and a lower-triangle kernel would solve a
//  different system than the caller's without a word — ADVICE r05)
static constexpr double kSymRelTol64 = 1e-6;

// S (and Pinv when it has off-diagonal blocks: pcols = 3) of one call through bd_symmetry_check_kernel, in the call's storage type (esz 2, 4 or 8
// bytes) with that type's tolerance: failing block pairs are added to *cnt, OR-ed into *flag (either may be null)
static void launch_sym_check(mpcg_handle* h, int esz, const void* S, const void* Pinv, int pcols, uint32_t batch, hipStream_t st,
                             unsigned long long* cnt, unsigned long long* flag) {
    const long items = (long)batch * ((long)h->N - 1);
    const unsigned blocks = (unsigned)((items + 3) / 4);
    const auto go = [&](auto type, float tol) {
        using MT = decltype(type);
        for (const void* m : {S, pcols == 3 ? Pinv : nullptr})
            if (m) hipLaunchKernelGGL(bd_symmetry_check_kernel<MT>, dim3(blocks), dim3(256), 0, st, static_cast<const MT*>(m), (int)h->N, (int)batch, tol, cnt, flag);
    };
    if (esz == 2) go(_Float16(), kSymRelTol); else if (esz == 4) go(float(), kSymRelTol); else go(double(), (float)kSymRelTol64);
}
static void sym_mark_violated(mpcg_handle* h) {
    h->sym_state = 2;
    h->err = "warning: S / Pinv of a solve on this handle were not block-symmetric (block (k, right) != block (k+1, left)^T): the handle now "
             "runs kernels that read all three block columns (include/mpcg.h, BLOCK SYMMETRY)";
}
// A handle whose latch resolved on block-Jacobi calls knows S only: the first SS call (Pinv has off-diagonal blocks) re-opens it, so that its
// Pinv goes through a check before a lower-triangle kernel reads it.
static void sym_reopen_for_pinv(mpcg_handle* h, int pcols) {
    if (h->sym_state == 1 && pcols == 3 && !h->sym_pinv_ok) h->sym_state = 0;
}
// a pending reset of the sticky device flag ("assume_symmetric" = 0 after a violation) is issued by the next solve, on its stream
static int sym_reset_flag(mpcg_handle* h, hipStream_t st) {
    if (!h->sym_flag_reset) return MPCG_OK;
    hipLaunchKernelGGL(zero_words_kernel, dim3(1), dim3(256), 0, st, counter(h, CTR_SYM_FLAG), (size_t)1);
    HIP_TRY(h, hipGetLastError());
    h->sym_flag_reset = false;
    return MPCG_OK;
}
// has the asynchronous copy of the device flag landed?
// (never while `st` is being captured into a graph: an event query is not a capturable operation and would invalidate the capture —
//  a capturing caller stays on the guarded launches, which are plain kernel launches)
static void sym_poll(mpcg_handle* h, hipStream_t st, bool have_stream) {
    if (!h->sym_pending) return;
    if (have_stream) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return;
    }
    // (the query itself in relaxed capture mode: with ANOTHER stream of this thread being captured in global mode an event query is an
    //  "unsafe" call that would invalidate that unrelated capture — mpcg_get_option("symmetry_state") passes no stream at all)
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    const hipError_t q = hipEventQuery(h->sym_event);
    (void)hipThreadExchangeStreamCaptureMode(&mode);
    if (q != hipSuccess) return;
    h->sym_pending = false;
    if (*h->sym_host == 0 && h->sym_guard_seq != h->sym_armed_seq) {
        // guarded solves were issued AFTER this copy was armed: a clean flag says nothing about their matrices.  Stay unknown — the next
        // guarded call arms a new copy, which (the device flag is sticky) covers them all.
        return;
    }
    if (*h->sym_host) sym_mark_violated(h);
    else { h->sym_state = 1; h->sym_pinv_ok = h->sym_armed_pinv; }
}

// "check_symmetry": block pairs of S and (SS only) Pinv that fail the check.  Blocking: waits for `st`.
static int symmetry_violations(mpcg_handle* h, const PcgArgs& a, uint32_t batch, hipStream_t st, int* out) {
    unsigned long long* cnt = counter(h, CTR_SYM_VIOLATIONS);
    HIP_TRY(h, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st));
    launch_sym_check(h, a.esz, a.S, a.Pinv, a.pcols, batch, st, cnt, nullptr);
    HIP_TRY(h, hipGetLastError());
    unsigned long long v = 0;
    HIP_TRY(h, hipMemcpyAsync(&v, cnt, sizeof v, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    *out = v > 0x7fffffffull ? 0x7fffffff : (int)v;
    return MPCG_OK;
}

// The float latch: asynchronous.  A lower-triangle launch of a handle that does not know yet whether its caller's matrices are block-symmetric:
//   check kernel(s)  -> OR into the handle's device flag (never reset: the latch)
//   the lower-triangle kernel, gated: its workgroups leave at once if the flag is set
//   a three-column kernel, gated the other way: runs only if the flag is set
//   (clustered kernel: its own fix-up launch is that kernel — every completion count is 0 after a gated exit)
// and, outside graph capture, an asynchronous copy of the flag to pinned host memory + an event that sym_poll() queries on later calls.
// Returns 1 when the plan has no lower-triangle kernel after all (the check kernels have run: the caller falls through).
static int launch_guarded(mpcg_handle* h, const PcgArgs& a, uint32_t batch, hipStream_t st, bool* order) {
    const PcgPlan p = plan_f32(h, batch, a.esz, a.pcols, GATED);
    unsigned long long* flag = counter(h, CTR_SYM_FLAG);
    ++h->sym_guard_seq;
    if (a.pcols == 3) h->sym_pinv_guarded = true;
    launch_sym_check(h, a.esz, a.S, a.Pinv, a.pcols, batch, st, nullptr, flag);
    HIP_TRY(h, hipGetLastError());
    const int fam = p.last.family;
    if (fam != FAM_LPK && fam != FAM_LQB && fam != FAM_LPKC) return 1;
    PcgArgs g = a;
    g.redo_flags = flag; g.redo_stride = 0; g.redo_skip = 1; g.redo_count = nullptr;         // skip if the flag is 1
    { const int rc = launch_plan<ClusterArgs>(h, p, g, batch, st, /*count_fixups=*/false); if (rc != MPCG_OK) return rc; }
    *order = p.order;
    if (fam != FAM_LPKC || !h->cluster_fixup) {
        PcgArgs f = a;
        f.redo_flags = flag; f.redo_stride = 0; f.redo_skip = 0; f.redo_count = nullptr;     // skip if the flag is 0
        const int rc = launch_args(h, plan_f32(h, batch, a.esz, a.pcols, FALLBACK).k, f, batch, st);
        if (rc != MPCG_OK) return rc;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (!h->sym_pending && hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
        HIP_TRY(h, hipMemcpyAsync(h->sym_host, flag, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipEventRecord(h->sym_event, st));
        h->sym_pending = true;
        h->sym_armed_seq = h->sym_guard_seq;
        h->sym_armed_pinv = h->sym_pinv_guarded;
    }
    return MPCG_OK;
}
// The double latch: the double kernels that read only the left + diagonal block columns use the same per-handle state, but a handle that does not
// know yet checks THIS call's matrices once, with one blocking 8-byte copy (never during capture: a capturing call on such a handle runs a
// kernel that reads all three columns).
static int f64_symmetry_latch(mpcg_handle* h, const PcgArgs64& a, uint32_t batch, hipStream_t st) {
    sym_poll(h, st, true);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    sym_reopen_for_pinv(h, a.pcols);      // (a capturing call cannot check the Pinv it re-opens for: it runs a three-column kernel)
    if (h->sym_state != 0 || h->sym_pending || capturing) return MPCG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    { const int rc = sym_reset_flag(h, st); if (rc != MPCG_OK) return rc; }
    unsigned long long* flag = counter(h, CTR_SYM_FLAG);
    launch_sym_check(h, sizeof(double), a.S, a.Pinv, a.pcols, batch, st, nullptr, flag);
    HIP_TRY(h, hipGetLastError());
    unsigned long long v = 0;
    HIP_TRY(h, hipMemcpyAsync(&v, flag, sizeof v, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (v) sym_mark_violated(h); else h->sym_state = 1;
    h->sym_pinv_ok = !v && a.pcols == 3;
    return MPCG_OK;
}

// ---- the solve entries' shared host path -------------------------------------------------------------------------------------------
// The fields PcgArgs and PcgArgsG<T> have in common, from an entry's arguments (everything else: the structs' defaults, set by the launch paths)
template <typename A, typename MT, typename T>
static A solve_args(const mpcg_handle* h, const MT* S, const MT* Pinv, const T* gamma, T* lambda, T* r_out, T* p_out, uint32_t* iters, uint8_t* exits,
                    uint32_t max_iter, T exit_tol, int pcols) {
    A a{};
    a.S = S; a.Pinv = Pinv; a.gamma = gamma; a.lambda = lambda; a.r_out = r_out; a.p_out = p_out;
    a.iters = iters; a.max_iter_exit = exits;
    a.N = (int)h->N; a.max_iter = (int)max_iter; a.exit_tol = exit_tol; a.pcols = pcols;
    return a;
}
// What the five solve entries check before they launch, in the order they report it: null handle; null pointers; (the batched entries) batch 0 —
// nothing to do — batch above max_batch, the preconditioner; max_iter; the alignment of S / Pinv in their storage type MT (float 16 bytes,
// fp16 4, double none) — which the float `_ref` entry looks at BEFORE max_iter.  Returns true when the call ends here, with *rc.
template <typename MT>
static bool solve_ends(mpcg_handle* h, const char* entry, bool ref, const MT* S, const MT* Pinv, const void* gamma, const void* lambda, const void* iters,
                       const void* exits, uint32_t batch, int precond, uint32_t max_iter, int* rc) {
    constexpr uintptr_t align = std::is_same<MT, float>::value ? 16 : std::is_same<MT, uint16_t>::value ? 4 : 1;
    const auto refuse = [&](const char* why) { *rc = h ? fail(h, MPCG_ERR_INVALID, std::string(entry) + why) : MPCG_ERR_INVALID; return true; };
    const auto misaligned = [&] { return ((reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(Pinv)) & (align - 1)) != 0; };
    const char* align_text = align == 16 ? ": d_S / d_Pinv must be 16-byte aligned" : ": d_S16 / d_Pinv16 must be 4-byte aligned";
    if (!h) return refuse("");
    if (!S || !Pinv || !gamma || !lambda || !iters || !exits) return refuse(": null device pointer");
    if (!ref) {
        if (batch == 0) { *rc = MPCG_OK; return true; }
        if (batch > h->max_batch) return refuse(": batch exceeds max_batch");
        if (precond != MPCG_PRECOND_JACOBI && precond != MPCG_PRECOND_SS) return refuse(": bad preconditioner");
    } else if (misaligned()) return refuse(align_text);
    if (max_iter > 0x7fffffffu) return refuse(": max_iter too large");
    if (misaligned()) return refuse(align_text);
    return false;
}

// One float / fp16 solve.  *order: the launched plan asks for the dispatch-order kernel.
static int launch_pcg(mpcg_handle* h, const PcgArgs& a_in, uint32_t batch, hipStream_t st, int esz, bool* order) {
    HIP_TRY(h, hipSetDevice(h->device));
    PcgArgs a = a_in;
    a.esz = esz;
    PcgPlan p = plan_f32(h, batch, esz, a.pcols, LOWER);
    *order = false;
    if (h->generic) {      // state_size != 14: the PcgArgs of the tuned path re-packed for the generic kernel
        const auto g = solve_args<PcgArgsG<float>>(h, static_cast<const float*>(a.S), static_cast<const float*>(a.Pinv), a.gamma, a.lambda, a.r_out, a.p_out,
                                                   a.iters, a.max_iter_exit, (uint32_t)a.max_iter, a.exit_tol, a.pcols);
        const int rc = launch_args(h, p.k, g, batch, st);
        if (rc == MPCG_OK) h->last = p.last;
        return rc;
    }
    if (p.last.family != FAM_RPL) {
        // "check_symmetry" (debug, off by default): the kernels below read only the left + diagonal block columns (mpcg.h "Block symmetry").
        // Verify the precondition on this call's matrices; a call that violates it is solved by a kernel that reads all three columns.
        bool lower_ok = true;
        h->last_sym_violations = 0;
        if (h->check_symmetry && p.check) {
            int v = 0;
            const int rc = symmetry_violations(h, a, batch, st, &v);
            if (rc != MPCG_OK) return rc;
            h->last_sym_violations = v;
            lower_ok = v == 0;
        } else if (p.lower) {
            // the symmetry latch (see launch_guarded): no synchronisation, no per-solve D2H
            sym_poll(h, st, true);
            sym_reopen_for_pinv(h, a.pcols);
            { const int rc = sym_reset_flag(h, st); if (rc != MPCG_OK) return rc; }
            if (h->sym_state == 2) lower_ok = false;
            else if (h->sym_state == 0) {
                const int rc = launch_guarded(h, a, batch, st, order);
                if (rc != 1) return rc;
            }
        }
        if (!lower_ok) p = plan_f32(h, batch, esz, a.pcols, FULL);
    }
    const int rc = launch_plan<ClusterArgs>(h, p, a, batch, st);
    *order = rc == MPCG_OK && p.order;
    return rc;
}

// One double solve.
static int launch_f64(mpcg_handle* h, PcgArgs64 a, uint32_t batch, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(h, hipSetDevice(h->device));
    PcgPlan p = plan_f64(h, batch, a.pcols, true);
    if (p.lower) {         // the lane-quad kernels: once the latch says the matrices are block-symmetric
        const int rc = f64_symmetry_latch(h, a, batch, st);
        if (rc != MPCG_OK) return rc;
        if (h->sym_state != 1) p = plan_f64(h, batch, a.pcols, false);
    }
    if (p.last.family == FAM_GENERIC && !h->generic) {
        // the streaming kernel reads a third less when it may take block (k, right) from block (k+1, left) (mpcg.h, BLOCK SYMMETRY)
        const int rc = f64_symmetry_latch(h, a, batch, st);
        if (rc != MPCG_OK) return rc;
        a.lower = h->sym_state == 1 ? 1 : 0;
    }
    if (p.G && (!h->buf[BUF_CLUSTER64].p || (h->cluster_fixup && h->buf[BUF_LAM_BACKUP].bytes < (size_t)h->max_batch * h->N * NS * sizeof(double)))) {
        // (mpcg_create made them for handles with <= 8 MB of double iterates; "reserve_f64" = 1 makes them ahead of a capture)
        { const int rc = alloc_allowed(h, st, "mpcg_pcg_solve_f64 (or set \"reserve_f64\" = 1 first)"); if (rc != MPCG_OK) return rc; }
        { const int rc = reserve_f64(h); if (rc != MPCG_OK) return rc; }
    }
    return launch_plan<ClusterArgs64>(h, p, a, batch, st);
}

// The plan of a default-configured batch-1 call (256 CUs) on a handle of the stack: no GPU needed
static PcgPlan default_plan(uint32_t n, uint32_t N, bool f64) {
    mpcg_handle tmp;
    tmp.n = n; tmp.N = N; tmp.num_cus = 256; tmp.max_batch = 1;
    tmp.generic = generic_shape_supported(n, N);
    return f64 ? plan_f64(&tmp, 1, 3, true) : plan_f32(&tmp, 1, 4, 3, LOWER);
}


extern "C" {

// LDS bytes of the launch a default-configured batch-1 solve makes (what pcgSharedMemSize stands for)
size_t mpcg_pcg_lds_bytes(uint32_t state_size, uint32_t knot_points) {
    if (!generic_shape_supported(state_size, knot_points) &&
        (!shape_supported(state_size, knot_points) || (knot_points > kLpbMaxN && lds_bytes_for(knot_points, 16) > kLdsMax)))
        return 0;
    return default_plan(state_size, knot_points, false).k.lds;
}

size_t mpcg_pcg_lds_bytes_f64(uint32_t state_size, uint32_t knot_points) {     // (lane-quad kernels: block-symmetric matrices, the reference's)
    if (!shape_supported(state_size, knot_points) && !generic_shape_supported(state_size, knot_points)) return 0;
    const PcgPlan p = default_plan(state_size, knot_points, true);
    return p.k.rc == MPCG_OK ? p.k.lds : 0;
}

// Resident trajectories of the configuration a throughput-sized call (batch = max_batch) would launch.
int mpcg_check_pcg_occupancy(mpcg_handle* h, uint32_t* resident_trajectories) {
    if (!h || !resident_trajectories) return MPCG_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    const PcgPlan p = plan_f32(h, h->max_batch, 4, 3, LOWER);
    if (p.G) {      // clustered kernel: resident CLUSTERS = trajectories in flight, the count the launch itself uses
        *resident_trajectories = p.resident;
        return MPCG_OK;
    }
    if (p.k.rc != MPCG_OK) return fail(h, p.k.rc, p.k.err);
    { const int rc = raise_lds(h, p.k); if (rc != MPCG_OK) return rc; }
    int per_cu = 0;
    HIP_TRY(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, p.k.kern, (int)p.k.block, p.k.lds));
    if (per_cu < 1) return fail(h, MPCG_ERR_UNSUPPORTED, "PCG workgroup does not fit on a CU");
    *resident_trajectories = (uint32_t)per_cu * (uint32_t)h->num_cus;
    return MPCG_OK;
}

int mpcg_pcg_solve(mpcg_handle* h, const float* d_S, const float* d_Pinv, const float* d_gamma, float* d_lambda,
                   uint32_t batch, uint32_t max_iter, float exit_tol, mpcg_precond precond,
                   uint32_t* d_iters, uint8_t* d_max_iter_exit, void* stream) {
    int rc;
    if (solve_ends(h, "mpcg_pcg_solve", false, d_S, d_Pinv, d_gamma, d_lambda, d_iters, d_max_iter_exit, batch, precond, max_iter, &rc)) return rc;
    PcgArgs a = solve_args<PcgArgs>(h, d_S, d_Pinv, d_gamma, d_lambda, (float*)nullptr, (float*)nullptr, d_iters, d_max_iter_exit, max_iter, exit_tol, (int)precond);
    // Calls with more trajectories than CUs: dispatch longest-expected first, the expectation being the previous call's iteration
    // counts for the same batch (pcg_kernels.hip.h: sched_order_kernel).  A scheduling hint only: no result depends on it.
    const bool hinted = h->sched_hint && !h->generic && batch > (uint32_t)h->num_cus;
    if (hinted) { a.order = h->ptr<uint32_t>(BUF_SCHED_ORDER); a.order_tag = batch; }       // (used only if the stored permutation was made for this batch: sched_pick)
    bool order = false;
    rc = launch_pcg(h, a, batch, static_cast<hipStream_t>(stream), 4, &order);
    if (rc == MPCG_OK && hinted && order) {
        hipLaunchKernelGGL(sched_order_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), d_iters, (int)batch, h->ptr<uint32_t>(BUF_SCHED_ORDER));
        HIP_TRY(h, hipGetLastError());
    }
    return rc;
}

int mpcg_pcg_solve_ref(mpcg_handle* h, float* d_S, float* d_Pinv, float* d_gamma, float* d_lambda,
                       float* d_r, float* d_p, float* /*d_v_temp*/, float* /*d_eta_new_temp*/,      // (the reference's per-block partial-sum scratch: not needed)
                       uint32_t* d_pcg_iters, uint8_t* d_pcg_exit,
                       uint32_t pcg_max_iter, float pcg_exit_tol, void* stream) {
    int rc;
    if (solve_ends(h, "mpcg_pcg_solve_ref", true, d_S, d_Pinv, d_gamma, d_lambda, d_pcg_iters, d_pcg_exit, 1, MPCG_PRECOND_SS, pcg_max_iter, &rc)) return rc;
    bool order = false;
    return launch_pcg(h, solve_args<PcgArgs>(h, d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, d_pcg_iters, d_pcg_exit, pcg_max_iter, pcg_exit_tol, 3), 1,
                      static_cast<hipStream_t>(stream), 4, &order);
}

int mpcg_bt_spmv(mpcg_handle* h, const float* d_M, const float* d_x, float* d_y, uint32_t batch, int cols, void* stream) {
    if (!h) return MPCG_ERR_INVALID;
    if (h->generic) return fail(h, MPCG_ERR_UNSUPPORTED, "mpcg_bt_spmv: state_size = 14 only (other state sizes: PCG entry points through the generic kernel)");
    if (!d_M || !d_x || !d_y) return fail(h, MPCG_ERR_INVALID, "mpcg_bt_spmv: null device pointer");
    if (cols != 1 && cols != 3) return fail(h, MPCG_ERR_INVALID, "mpcg_bt_spmv: cols must be 1 or 3");
    if (batch == 0) return MPCG_OK;
    if (batch > h->max_batch) return fail(h, MPCG_ERR_INVALID, "mpcg_bt_spmv: batch exceeds max_batch");
    if (reinterpret_cast<uintptr_t>(d_M) & 15u) return fail(h, MPCG_ERR_INVALID, "mpcg_bt_spmv: d_M must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y)) & 7u)
        return fail(h, MPCG_ERR_INVALID, "mpcg_bt_spmv: d_x / d_y must be 8-byte aligned");
    HIP_TRY(h, hipSetDevice(h->device));
    SpmvArgs a{d_M, d_x, d_y, (int)h->N, (int)batch, cols};
    constexpr int NW = 4;
    const long total = (long)batch * h->N;
    const long tasks = h->spmv_mfma ? total : (total + SPMV_SPAN - 1) / SPMV_SPAN;     // a wavefront's unit: a block row (MFMA experiment) or a span of rows
    long blocks = (tasks + NW - 1) / NW;
    const long cap = (long)h->num_cus * h->spmv_blocks_per_cu;
    if (blocks > cap) blocks = cap;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (h->spmv_mfma) hipLaunchKernelGGL((bt_spmv_mfma_kernel<NW>), dim3((unsigned)blocks), dim3(NW * 64), 0, st, a);
    else if (h->nt_loads) hipLaunchKernelGGL((bt_spmv_kernel<NW, true>), dim3((unsigned)blocks), dim3(NW * 64), 0, st, a);
    else hipLaunchKernelGGL((bt_spmv_kernel<NW, false>), dim3((unsigned)blocks), dim3(NW * 64), 0, st, a);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}


int mpcg_probe_hbm_read(mpcg_handle* h, const void* d_src, size_t bytes, float* d_sink, void* stream) {
    if (!h) return MPCG_ERR_INVALID;
    if (!d_src || !d_sink) return fail(h, MPCG_ERR_INVALID, "mpcg_probe_hbm_read: null device pointer");
    if ((reinterpret_cast<uintptr_t>(d_src) & 15u) || (bytes & 15u)) return fail(h, MPCG_ERR_INVALID, "mpcg_probe_hbm_read: d_src must be 16-byte aligned and bytes a multiple of 16");
    if (bytes == 0) return MPCG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(hbm_read_probe_kernel, dim3((unsigned)(2 * h->num_cus)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const f4*>(d_src), d_sink, bytes / 16);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

int mpcg_convert_f32_to_f16(mpcg_handle* h, const float* d_src, uint16_t* d_dst, size_t count, void* stream) {
    if (!h) return MPCG_ERR_INVALID;
    if (!d_src || !d_dst) return fail(h, MPCG_ERR_INVALID, "mpcg_convert_f32_to_f16: null device pointer");
    if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 15u)
        return fail(h, MPCG_ERR_INVALID, "mpcg_convert_f32_to_f16: pointers must be 16-byte aligned");
    if (count == 0) return MPCG_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t blocks = (count + 2047) / 2048;
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d_src,
                       reinterpret_cast<_Float16*>(d_dst), count);
    HIP_TRY(h, hipGetLastError());
    return MPCG_OK;
}

int mpcg_pcg_solve_f16(mpcg_handle* h, const uint16_t* d_S16, const uint16_t* d_Pinv16, const float* d_gamma,
                       float* d_lambda, uint32_t batch, uint32_t max_iter, float exit_tol, mpcg_precond precond,
                       uint32_t* d_iters, uint8_t* d_max_iter_exit, void* stream) {
    if (h && h->generic)      // (before any argument is looked at)
        return fail(h, MPCG_ERR_UNSUPPORTED, "mpcg_pcg_solve_f16: state_size = 14 only (other state sizes: PCG entry points through the generic kernel)");
    int rc;
    if (solve_ends(h, "mpcg_pcg_solve_f16", false, d_S16, d_Pinv16, d_gamma, d_lambda, d_iters, d_max_iter_exit, batch, precond, max_iter, &rc)) return rc;
    bool order = false;
    return launch_pcg(h, solve_args<PcgArgs>(h, d_S16, d_Pinv16, d_gamma, d_lambda, (float*)nullptr, (float*)nullptr, d_iters, d_max_iter_exit, max_iter, exit_tol, (int)precond),
                      batch, static_cast<hipStream_t>(stream), 2, &order);
}

int mpcg_pcg_solve_f64(mpcg_handle* h, const double* d_S, const double* d_Pinv, const double* d_gamma, double* d_lambda,
                       uint32_t batch, uint32_t max_iter, double exit_tol, mpcg_precond precond,
                       uint32_t* d_iters, uint8_t* d_max_iter_exit, void* stream) {
    int rc;
    if (solve_ends(h, "mpcg_pcg_solve_f64", false, d_S, d_Pinv, d_gamma, d_lambda, d_iters, d_max_iter_exit, batch, precond, max_iter, &rc)) return rc;
    return launch_f64(h, solve_args<PcgArgs64>(h, d_S, d_Pinv, d_gamma, d_lambda, (double*)nullptr, (double*)nullptr, d_iters, d_max_iter_exit, max_iter, exit_tol, (int)precond),
                      batch, stream);
}

int mpcg_pcg_solve_ref_f64(mpcg_handle* h, double* d_S, double* d_Pinv, double* d_gamma, double* d_lambda,
                           double* d_r, double* d_p, double* /*d_v_temp*/, double* /*d_eta_new_temp*/,
                           uint32_t* d_pcg_iters, uint8_t* d_pcg_exit, uint32_t pcg_max_iter, double pcg_exit_tol, void* stream) {
    int rc;
    if (solve_ends(h, "mpcg_pcg_solve_ref_f64", true, d_S, d_Pinv, d_gamma, d_lambda, d_pcg_iters, d_pcg_exit, 1, MPCG_PRECOND_SS, pcg_max_iter, &rc)) return rc;
    return launch_f64(h, solve_args<PcgArgs64>(h, d_S, d_Pinv, d_gamma, d_lambda, d_r, d_p, d_pcg_iters, d_pcg_exit, pcg_max_iter, pcg_exit_tol, 3), 1, stream);
}

int mpcg_debug_read_cluster_scratch(mpcg_handle* h, unsigned long long* out, int count) {
    if (!h || !out || count < 0 || (size_t)count > cluster_alloc_words(h)) return MPCG_ERR_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return MPCG_ERR_HIP;
    return hipMemcpy(out, h->buf[BUF_CLUSTER].p, sizeof(unsigned long long) * (size_t)count, hipMemcpyDeviceToHost) == hipSuccess ? MPCG_OK : MPCG_ERR_HIP;
}

#ifdef MPCG_PROF
// diagnostic build only (tools/prof_phases.py): the s_memtime stamps of workgroup 0
int mpcg_debug_read_prof(long long* out, int count) {
    if (!out || count < 0 || count > 16 * 32) return MPCG_ERR_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return MPCG_ERR_HIP;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mpcg::g_pcg_prof), sizeof(long long) * (size_t)count) == hipSuccess ? MPCG_OK : MPCG_ERR_HIP;
}
// (entry time, exit time, HW_ID, XCC_ID) of the first `count` / 4 workgroups of the last lane-quad launch
int mpcg_debug_read_wg_prof(long long* out, int count) {
    if (!out || count < 0 || count > 4096 * 4) return MPCG_ERR_INVALID;
    if (hipDeviceSynchronize() != hipSuccess) return MPCG_ERR_HIP;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(mpcg::g_wg_prof), sizeof(long long) * (size_t)count) == hipSuccess ? MPCG_OK : MPCG_ERR_HIP;
}
#endif

}  // extern "C"
