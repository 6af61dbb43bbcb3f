// pcg_cluster.hip.h — the cluster runtime: what the three kernels that spread ONE trajectory over G workgroups on G CUs of one XCD share
// (pcg_lpkc_kernel, pcg_lpk_cluster.hip.h, float; pcg_lqkc_f64_kernel, pcg_lqk_cluster_f64.hip.h, and pcg_rplc_f64_kernel,
// pcg_rpl_cluster_f64.hip.h, double), and their host side: the scratch of epoch-tagged hand-off cells and completion flags.
// Hand-off = the R2 recipe of cdna_hip_programming.md §6 G16: {epoch, value} granules written with one relaxed agent-scope store and
// polled with relaxed agent-scope loads — the tag is the flag, no fences; every spin is bounded.  Persistent clusters draw trajectories
// from a queue; a member whose peers do not show up gives up, and completion counts tell the fix-up launch which trajectories to re-solve.
// A kernel brings its own layout of cells (slot and word constants: the template parameters below), its own LDS cells and barriers, the
// poll loop of its hand-off (which lanes poll what differs, and the loop is the one piece whose machine code does not survive a move
// into a function: DESIGN.md §3.3), and everything between two hand-offs.  (Rounds 1-2 had two more clustered kernels on this machinery — a row-triple one and a lane-per-block
// one; both retired in round 4, HISTORY.md.)
#pragma once
#include "pcg_kernels.hip.h"
#include "pcg_f64.hip.h"

namespace mpcg {

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef unsigned u4 __attribute__((ext_vector_type(4)));
// "This cluster gave up" flags: one per trajectory of the launch, each in a 128-byte line of its own at the FRONT of the
// scratch buffer, read by the fix-up launch with agent-scope loads.  They must not share a line with the polled cells: a
// plainly cached copy of such a line (left in some XCD's L2 by the fix-up kernel) made the next graph replay's pollers
// read last run's epochs and time out.
constexpr int CL_FLAG_STRIDE = 16;       // u64 words between flags
// A poll is one sc1 load + s_sleep (25-70 ns): 2^16 polls = 1.5-4.5 ms.  Members of a launch are dispatched within a
// microsecond of each other on a free GPU, so a wait this long means a peer is not resident (another stream holds its
// CU): the member gives up and the host-side fix-up launch re-solves the trajectory with the single-workgroup kernel.
constexpr unsigned CL_SPIN_LIMIT = 1u << 16;

struct ClusterArgs {
    int kl_max;                              // knots of the largest member
    PcgArgs p;
    unsigned long long* scratch;         // [clusters * G][LPKC_WG_WORDS] hand-off cells, zeroed before the launch
    unsigned long long* fail_flags;      // [batch][CL_FLAG_STRIDE], zeroed before the launch: count of members that finished the trajectory
    int G;
    unsigned long long* queue = nullptr; // next trajectory to hand out (zeroed before the launch)
    int batch = 0;                       // trajectories of the call
    int clusters = 0;                    // clusters of the launch (the grid holds 8 ceil(clusters / 8) of them)
    int l2_handoff = 1;                  // 1 = hand-offs through the XCD's L2 when all members of a cluster share an XCD (verified in the kernel)
    int test_fail = 0;                   // tests only ("cluster_test_fail"): the last member of cluster 0 gives up at the write-back of its first trajectory
};

struct ClusterArgs64 {
    PcgArgs64 p;
    unsigned long long* scratch;         // [clusters * G][LQKC_WG_WORDS or RPLC_WG_WORDS] hand-off cells, zeroed before the launch
    unsigned long long* fail_flags;      // [batch][CL_FLAG_STRIDE], zeroed before the launch: members that finished the trajectory
    unsigned long long* queue;           // next trajectory to hand out (zeroed before the launch)
    int G, batch, clusters, l2_handoff;
    int test_fail = 0;                   // tests only ("cluster_test_fail"): the last member of cluster 0 gives up at the write-back of its first trajectory
};

// Zero-fill of the cluster scratch (flags + hand-off cells) in front of every cluster launch.  A kernel of our own
// rather than hipMemsetAsync: captured into a hipGraph next to other fills, the memset NODE replayed with another
// node's fill value (ROCm 7.2; observed 7168 = the element count of a neighbouring tensor fill) — harmless for the
// epoch-tagged cells, fatal for the flags.
__global__ __launch_bounds__(256) void zero_words_kernel(unsigned long long* p, size_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) p[i] = 0ull;
}
// Behind a cluster launch that NO fix-up launch follows ("cluster_fixup" = 0, or a horizon the fix-up kernel cannot hold): every trajectory
// whose completion count is short of G is REPORTED here — d_iters = 0xFFFFFFFF, d_max_iter_exit = 2 — whatever the members themselves stored.
// A member that gives up writes that pair itself, but member 0 may still pass its last hand-off (the failed peer published before it timed
// out) and store a valid-looking count over it, and a cluster that gives up stops drawing from the queue: trajectories it would have drawn
// get no store at all.  The completion counts know both.
__global__ __launch_bounds__(256) void cluster_report_kernel(const unsigned long long* flags, int stride, unsigned long long G, int batch,
                                                             uint32_t* iters, uint8_t* max_iter_exit) {
    const int b = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (b >= batch) return;
    if (__hip_atomic_load(flags + (size_t)b * stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != G) {
        iters[b] = 0xFFFFFFFFu;
        max_iter_exit[b] = 2;
    }
}
// The same fill + the handle's copy of the caller's lambda ([batch][N][n], n32 dwords): what a fix-up launch warm-starts from (PcgArgs::lam0).
// One launch in front of every cluster launch.
__global__ __launch_bounds__(256) void cluster_prologue_kernel(unsigned long long* p, size_t count, const uint32_t* src, uint32_t* dst, size_t n32) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t j = i; j < count; j += stride) p[j] = 0ull;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0) {
        typedef unsigned u4v __attribute__((ext_vector_type(4)));
        const size_t n4 = n32 / 4;
        for (size_t j = i; j < n4; j += stride) reinterpret_cast<u4v*>(dst)[j] = reinterpret_cast<const u4v*>(src)[j];
        for (size_t j = 4 * n4 + i; j < n32; j += stride) dst[j] = src[j];
    } else {
        for (size_t j = i; j < n32; j += stride) dst[j] = src[j];
    }
}

// Granule accesses in the "uniform 64-bit base (SGPR pair) + 32-bit lane byte offset" addressing form, spelled out: left to
// the compiler, the per-lane addresses of the two exchange slots become 64-bit VGPR pointers that are hoisted out of the PCG
// loop — four registers the lane-pair kernel does not have; they spill, and the publishing wave reloads its store address from scratch
// right in front of every hand-off.  (s_nop 4: the base may just have been written by a v_readlane — an SGPR spill reload — and a
// VMEM instruction reading a VALU-written SGPR needs 5 wait states; the compiler's hazard recogniser does not look into asm.)
// sc1 = agent scope (write-through store / L2-coherent load), as __hip_atomic_*(relaxed, agent).
// WORD = compile-time word index inside the member's block of cells: the instruction's immediate offset, so that the two exchange
// slots and the hand-out word share ONE base register pair.
template <int WORD>
__device__ __forceinline__ void granule_store(gu64* sbase, unsigned byte_off, unsigned long long v) {
    asm volatile("s_nop 4\n\tglobal_store_dwordx2 %0, %1, %2 offset:%3 sc1" : : "v"(byte_off), "v"(v), "s"(sbase), "n"(8 * WORD) : "memory");
}
// The same store WITHOUT sc1: the granule stays in this XCD's L2, where a poller on the same XCD finds it (its sc1 load bypasses
// only L1) without the round trip to the memory side that a write-through store forces on both.  Only valid when the whole
// cluster sits on one XCD, which the members verify at start-up (cluster_on_one_xcd).
template <int WORD>
__device__ __forceinline__ void granule_store_l2(gu64* sbase, unsigned byte_off, unsigned long long v) {
    asm volatile("s_nop 4\n\tglobal_store_dwordx2 %0, %1, %2 offset:%3" : : "v"(byte_off), "v"(v), "s"(sbase), "n"(8 * WORD) : "memory");
}
template <int WORD>
__device__ __forceinline__ unsigned long long granule_load(const gu64* sbase, unsigned byte_off) {
    unsigned long long x;
    asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %1, %2 offset:%3 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(x) : "v"(byte_off), "s"(sbase), "n"(8 * WORD) : "memory");
    return x;
}

// 16-byte granules {tag, v0, v1, v2}: one dwordx4 store (observed untorn on gfx950, MI355X_MICROARCH.md "R2's granule"), three
// values per fabric / L2 transaction instead of one.  L2 = without sc1 (see granule_store_l2).
template <int WORD, bool L2>
__device__ __forceinline__ void granule_store16(gu64* sbase, unsigned byte_off, f4 v) {
    if constexpr (L2) asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 offset:%3\n\ts_nop 1" : : "v"(byte_off), "v"(v), "s"(sbase), "n"(8 * WORD) : "memory");
    else asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 offset:%3 sc1\n\ts_nop 1" : : "v"(byte_off), "v"(v), "s"(sbase), "n"(8 * WORD) : "memory");
}

// ---- granule coding ----
// 8-byte granule {value, tag}: the tag in the high word (wave partials of the float kernel, the hand-out word, the XCC word)
__device__ __forceinline__ unsigned long long granule_of(unsigned value, unsigned tag) { return ((unsigned long long)tag << 32) | value; }
// 16-byte granule of a double: {value lo, value hi, tag, 0}
__device__ __forceinline__ f4 granule_of(double v, unsigned tag) {
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
    return f4{__builtin_bit_cast(float, (unsigned)bits), __builtin_bit_cast(float, (unsigned)(bits >> 32)), __builtin_bit_cast(float, tag), 0.f};
}
__device__ __forceinline__ double granule_value(u4 x) { return __builtin_bit_cast(double, ((unsigned long long)x.y << 32) | (unsigned long long)x.x); }

// ---- workgroup -> member ----
// Members of a cluster share an XCD (workgroups go to the XCDs round-robin): workgroup b = 8 j + x holds member j % G of cluster
// 8 (j / G) + x; the grid's last clusters may not exist (`member` false: the workgroup leaves).  Member g owns knots [k0, k1).
struct ClusterPlace { int g, cl; bool member; };
__device__ __forceinline__ ClusterPlace cluster_place(int G, unsigned nclusters) {
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    ClusterPlace pl;
    pl.g = jx % G;
    pl.cl = (jx / G) * 8 + xcd;
    pl.member = (unsigned)pl.cl < nclusters;
    return pl;
}
__device__ __forceinline__ int cluster_first_knot(int g, int N, int G) { return (int)(((long)g * N) / G); }

// ---- are all members of this cluster on one XCD? ----
// Once per launch, one wavefront per member: publish {XCC id, 1} in word SLOT_X of the own cells, poll the G members' words (bounded),
// compare.  Wave-uniform result; a member that did not show up in time counts as "elsewhere" (write-through hand-offs are always valid).
template <int SLOT_X, int WG_WORDS>
__device__ __forceinline__ bool cluster_on_one_xcd(gu64* my_words, gu64* cl_words, int lane, int G) {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 0xf;
    if (lane == 0) granule_store<SLOT_X>(my_words, 0u, granule_of(xcc, 1u));
    unsigned long long x = 0;
    unsigned spins = 0;
    bool ok;
    do {
        ok = true;
        if (lane < G) {
            x = granule_load<SLOT_X>(cl_words, 8u * (unsigned)(lane * WG_WORDS));
            ok = (unsigned)(x >> 32) == 1u;
        }
        if (__all(ok)) break;
        __builtin_amdgcn_s_sleep(1);
    } while (++spins < (CL_SPIN_LIMIT >> 4));
    return __all(lane >= G || ((unsigned)(x >> 32) == 1u && (unsigned)x == xcc));
}

// ---- next trajectory of this cluster (from the second on: the first is the cluster's own index) ----
// The leader (member 0) draws from the queue and publishes {trajectory, sequence number} in word SLOT_T of its cells; the followers poll
// that word (bounded).  Each side is called by one wavefront: the leader's by its lane 0 alone.  kp: the kernel's argument struct in the
// constant address space.
template <int SLOT_T, typename KP>
__device__ __forceinline__ int cluster_hand_out(KP kp, gu64* my_words, unsigned seq, unsigned nclusters, bool same_xcd) {
    const int bn = (int)nclusters + (int)__hip_atomic_fetch_add(kp->queue, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (same_xcd) granule_store_l2<SLOT_T>(my_words, 0u, granule_of((unsigned)bn, seq));
    else granule_store<SLOT_T>(my_words, 0u, granule_of((unsigned)bn, seq));
    return bn;
}
struct ClusterDraw { int index; bool timed_out; };
template <int SLOT_T>
__device__ __forceinline__ ClusterDraw cluster_await_trajectory(const gu64* cl_words, unsigned seq) {
    unsigned long long x = 0;
    unsigned spins = 0;
    do {
        x = granule_load<SLOT_T>(cl_words, 0u);
        if ((unsigned)(x >> 32) == seq) break;
        __builtin_amdgcn_s_sleep(1);
    } while (++spins < CL_SPIN_LIMIT);
    return ClusterDraw{(int)(unsigned)x, spins >= CL_SPIN_LIMIT};
}

// ---- end of a trajectory ----
// A member that gave up (a poll of its timed out) reports the trajectory as abandoned and leaves lambda alone: the trajectory's completion
// count stays short of G, and the fix-up launch re-solves it from the handle's copy of lambda0 — its peers may be past their last hand-off
// and have written their knots.  The member then stops: it draws no further trajectory.
template <typename KP>
__device__ __forceinline__ void cluster_report_abandoned(KP kp, int b, int tid) {
    if (tid == 0) { kp->p.iters[b] = 0xFFFFFFFFu; kp->p.max_iter_exit[b] = 2; }
}
// A member that wrote its knots back: the leader stores the trajectory's outputs, every member counts itself in.
template <typename KP>
__device__ __forceinline__ void cluster_finish(KP kp, int b, bool leader, int tid, uint32_t iters, uint32_t max_iter_exit) {
    if (tid == 0) {
        if (leader) {
            kp->p.iters[b] = iters;
            kp->p.max_iter_exit[b] = (uint8_t)max_iter_exit;
        }
        __hip_atomic_fetch_add(kp->fail_flags + (size_t)b * CL_FLAG_STRIDE, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace mpcg
