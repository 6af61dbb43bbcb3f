/* mpcg.h — C ABI of libmpcg_hip.so: MI355X (gfx950) PCG solver for MPCGPU's block-tridiagonal
 * Schur system  S * lambda = gamma.
 *
 * This is the drop-in boundary for ONE path of A2R-Lab/MPCGPU: the linear-system solve inside
 * sqpSolvePcg (reference include/pcg/sqp.cuh:230).  Citations below are file:line in the reference
 * tree.  The reference's implementation of that path (pcg<T,STATE_SIZE,KNOT_POINTS>, pcg_config,
 * pcgSharedMemSize, checkPcgOccupancy) lives in its un-vendored submodule A2R-Lab/GBD-PCG; the
 * entry points here replace its call sites.
 *
 * Conventions (identical to the reference's device buffers):
 *   - S, Pinv: "bd" layout, per trajectory [N][3][n*n] floats; block (k,col) column-major at
 *     k*3n^2 + col*n^2; col 0/1/2 = left / diagonal / right block of block row k
 *     (include/pcg/linsys_setup.cuh:36-57, 490-507).  Stored NEGATED (:15-19).  Blocks (0,col 0) and
 *     (N-1,col 2) are never written by the reference (:97,118) and are never read here.
 *   - BLOCK SYMMETRY.  PCG needs symmetric S and Pinv, and the reference's are: it writes S[k,right] as the transposed copy of
 *     S[k+1,left] (include/pcg/linsys_setup.cuh:536-557, bit for bit) and forms the symmetric-stair Pinv[k,right] / Pinv[k+1,left] as the
 *     same triple product associated two ways (:97-136; in float they differ by ~3e-5 of the largest entry on the bench's systems).  The register-resident kernels that serve fp32 horizons above 32 knots by
 *     default ("last_kernel_family" 6, 7 and 11) READ ONLY THE LEFT AND DIAGONAL block columns and apply L_{k+1}^T where the reference's kernel
 *     reads block (k,right); the right blocks of d_S / d_Pinv may then hold anything (tests poison them with NaN).  On the reference's
 *     matrices the results agree to that round-off of Pinv (iterates after K iterations: 1e-6 .. 3e-5, inside the fp32 band; bit-identical for S).
 *     THE HANDLE CHECKS THIS ONCE, BY ITSELF (round 4): until it knows, every solve that would run a lower-triangle kernel is launched
 *     guarded — a check kernel tests
 *         max | M[k,right] - M[k+1,left]^T |  <=  1e-2 max | M[k,right], M[k+1,left] |     for M = S and (SS) Pinv, every k
 *     (a test for STRUCTURAL asymmetry — a caller-made Pinv — not for the rounding differences above)
 *     into a flag on the device, the lower-triangle kernel runs only if the flag is clear and a kernel that reads all three block columns
 *     only if it is set — so even the FIRST solve of a caller with a non-symmetric Pinv is the solve of its three columns.  The flag reaches
 *     the host by an asynchronous copy that later calls poll (no call synchronises, nothing is copied per solve once the answer is in):
 *     from then on the handle launches plain lower-triangle kernels ("symmetry_state" 1) or, after a violation, three-column kernels for
 *     good ("symmetry_state" 2; mpcg_last_error() carries a warning).  The latch is per handle: a caller that changes the structure of its
 *     matrices later must use a fresh handle — or "check_symmetry" = 1 (debug), which verifies every solve with a blocking 8-byte copy
 *     and reports the number of offending block pairs as "last_symmetry_violations".  A caller that fills ONLY the left and diagonal block
 *     columns (the right one unwritten) says so with "assume_symmetric" = 1 before its first solve: no check, lower-triangle kernels at
 *     once.  Families 0 and 5 read all three columns anyway; so does family 3 for floats.  DOUBLE PRECISION beyond 32 knots uses the same
 *     latch: the lane-quad kernels (families 9, 10: the lower block triangle in registers) and the streaming kernel (family 3: skips the right
 *     block column, a third of its HBM bytes) run once it says symmetric.  A handle that does not know yet checks the matrices of its first
 *     mpcg_pcg_solve_f64 call with ONE blocking 8-byte copy (never during graph capture: a captured call on such a handle runs a kernel that
 *     reads all three columns — family 8 up to 256 knots, family 3 beyond).
 *   - NON-FINITE DATA.  The trajectories of a batched call are independent: no result of a trajectory depends on the FLOATING-POINT DATA of another
 *     one, finite or not.  A trajectory whose arrays hold Inf or NaN — a diverged iterate, a solve mpcg_line_search_step_rho has given up and that
 *     the other stages keep computing — or finite values that overflow, or singular (all-zero) matrices, leaves every output of every other
 *     trajectory of the call bit for bit what healthy data in its place would have left, in every entry point and every build: the kernels that
 *     carry several trajectories in one wavefront (four 16-lane rows in mpcg_block_solve, the chunk-walking formation, mpcg_compute_dz,
 *     mpcg_generate_kkt, mpcg_compute_merit, mpcg_simulate, mpcg_inverse_dynamics; two items per packed value under "kkt_f32" = 1 and
 *     "merit_f32" = 1; the rows of the whole batch in mpcg_bt_spmv) select by predicate, reduce within a row, and let rows without an item redo a
 *     valid one without storing.  THE ONE HANDLE-WIDE EFFECT is the symmetry latch above: its check counts a NaN in an OFF-DIAGONAL block of d_S
 *     (or, symmetric stair, of d_Pinv) of ANY trajectory as a violation — also the NaN of Inf - Inf when both blocks of a pair hold an Inf; a lone Inf passes the relative test —
 *     so such a value in a call made while the latch is open sends the handle to the three-column kernels for good ("symmetry_state" 2: other bits and a
 *     slower kernel for every trajectory of every later call; never a wrong system).  Non-finite values in d_gamma, d_lambda or a diagonal block
 *     do not touch it, and neither does anything once the latch has resolved or under "assume_symmetric" = 1.  For the non-finite trajectory
 *     ITSELF: every call returns — every loop and every spin of a kernel is bounded by a host argument (max_iter, knot_points, the substep
 *     count) or a constant, never by data; |eta| < exit_tol is false for a NaN —, d_iters[b] <= max_iter, d_max_iter_exit[b] is 0 or 1 (no
 *     cluster gives such a trajectory up: its members see the same bits and agree), d_step[b] is -1 ("a NaN never wins") or MPCG_STEP_FROZEN,
 *     and the integer bookkeeping (d_traj_offset, d_done) goes on as for any other; its floating-point outputs are unspecified.  Integer arrays
 *     and host scalars are validated or clamped as each entry says.  tests/test_gpu_containment_*.py hold every entry to this.
 *   - gamma, lambda: [N][n] floats per trajectory; lambda is in/out (warm start,
 *     include/mpcsim.cuh:186,267,337).
 *   - every pointer named d_* is a DEVICE pointer on the handle's device; `stream` is a hipStream_t
 *     passed as void* (NULL = default stream).  Calls are stream-ordered and never synchronise.
 *   - batched entry points take `batch` independent trajectories stored back to back.
 *   - ALIGNMENT AND EXTENTS.  A device pointer needs the alignment of ITS ELEMENT (4 bytes for float, int32_t and uint32_t, 8 for double, 2 for
 *     the uint16_t of half storage, 1 for uint8_t) and nothing more — whatever vector width a kernel uses inside (16-byte accesses go to
 *     dword-aligned addresses all over the path: the Q blocks of d_G_dense lie 245 elements apart, x_k of d_xu 21 elements apart) — with these
 *     exceptions, each refused with MPCG_ERR_INVALID and a message that says "aligned", before anything is launched or written:
 *         mpcg_pcg_solve, mpcg_pcg_solve_ref    d_S and d_Pinv 16-byte aligned
 *         mpcg_bt_spmv                          d_M 16-byte aligned; d_x and d_y 8-byte aligned
 *         mpcg_convert_f32_to_f16               d_src and d_dst 16-byte aligned
 *         mpcg_pcg_solve_f16                    d_S16 and d_Pinv16 4-byte aligned
 *         mpcg_probe_hbm_read                   d_src 16-byte aligned
 *     (an exact-size hipMalloc satisfies all of them; a matrix at an odd offset inside a larger allocation may not).  NO ENTRY READS OR WRITES
 *     OUTSIDE THE EXTENTS GIVEN HERE for its arrays, writes an array declared const, or — the 12-argument entries, whose reference signature has
 *     no const — writes d_S, d_Pinv, d_gamma, d_v_temp or d_eta_new_temp; d_max_iter_exit / d_pcg_exit is written one byte per trajectory.  No
 *     kernel uses an atomic operation on caller memory (those there are act on handle-owned buffers and on LDS).  tests/test_gpu_arena_*.py hold
 *     every entry to this: all arrays of a call inside one allocation, each at exactly its smallest accepted alignment, guard bands between.
 *     LARGE EXTENTS.  Every array of a call may pass 2^31 and 2^32 bytes, and a trajectory's results do not depend on where in the batch it
 *     stands; tests/test_gpu_large_*.py hold the entries to this on either side of each line below.  Two entries SWITCH KERNELS, same bits:
 *         mpcg_form_schur(_rhov)(_f64), 14 x 7   batch x knot_points x 3 n^2 x sizeof(T) >= 2^31 (the bytes of d_S: from 913,046 knots in float,
 *                                                456,523 in double): the LDS kernels instead of the register-resident ones, whose byte offsets
 *                                                are 31-bit; "last_schur_chunk" then reads 0.  Like "schur_dpp" = 0 this route owns a staging
 *                                                buffer, so the FIRST such call of a handle allocates and is refused inside a stream capture.
 *         mpcg_compute_dz(_f64), 14 x 7          batch x knot_points x (n^2 + n m) x sizeof(T) >= 2^31 (from 1,826,092 knots in float, 913,046
 *                                                in double): the LDS kernel; "last_dz_route" reads 0.
 *     One line REFUSES: mpcg_form_schur(_rhov)(_f64) returns MPCG_ERR_UNSUPPORTED for batch x knot_points >= 2^31 (a knot's index is an int).
 *     Every other entry indexes with 64-bit offsets (the PCG kernels and mpcg_bt_spmv through one buffer resource per trajectory) and serves
 *     whatever batch <= max_batch the device memory holds; mpcg_convert_f32_to_f16 takes any count below 2^42.
 *   - GRAPH CAPTURE.  Every compute entry point is pure stream work and may be captured into a hipGraph.  What the float PCG entry points need
 *     is allocated by mpcg_create; mpcg_form_schur(_f64), mpcg_block_solve(_f64), mpcg_compute_merit(_f64) and a FORCED "cluster" on a horizon the automatic policy gives to one
 *     CU allocate a handle-owned work buffer at their first call (hipMalloc is not stream work): make that call once outside the capture — a
 *     first call on a capturing stream returns MPCG_ERR_INVALID with a message and leaves the capture intact.  linsys_t = double beyond 32
 *     knots (mpcg_pcg_solve_f64 / _ref_f64: cluster kernels with a queue + flags buffer and a double-sized copy of lambda0): mpcg_create makes
 *     those buffers while they are small (max_batch x knot_points x state_size x 8 B <= 8 MB — every handle of the C++ shim), larger handles at
 *     their first double solve outside a capture or when the caller sets "reserve_f64" = 1 ahead of it (float-only callers never pay for them).
 *
 * All functions return MPCG_OK (0) or a negative mpcg_status; mpcg_last_error() gives the text.
 * Nothing here falls back to a CPU implementation: without a gfx950 device every compute entry
 * point fails with MPCG_ERR_HIP.
 */
#ifndef MPCG_H
#define MPCG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): the BLOCK SYMMETRY contract is checked by the handle itself (a caller that fills ONLY the left + diagonal block columns must
 * set "assume_symmetric" = 1 — round-3 text allowed garbage in the right blocks without it); options pcg_lpb / cluster_lpb / cluster_lpk /
 * cluster_waves / cluster_adj / schur_fma / schur_inplace are gone; mpcg_probe_hbm_read and "kkt_analytic" are new.
 * This reaches the reference's real-time horizon too: float 16 < N <= 32 at >= 2.5 trajectories per CU runs a lower-triangle kernel since
 * round 5 (below that batch, and at N <= 16, the row-per-lane kernel reads all three columns as before) — such calls are launched GUARDED
 * (check kernel + two gated kernels) until the handle's latch resolves, for good on a handle whose matrices violated the contract, and results
 * differ bitwise between batch sizes either side of the threshold.  mpcg_get_option("symmetry_state") = 2 / the warning in mpcg_last_error()
 * say when a handle has been sent to the three-column kernels; the C++ shim prints that warning once per handle to stderr.
 * Round 6, same ABI: "reserve_f64" (below, GRAPH CAPTURE); a latch that resolved on block-Jacobi calls re-opens at the first SS call; the
 * default float kernel for 32 < knot_points <= 128 is the lane-quad kernel ("pcg_lqb", family 11) — another summation order: results differ
 * from round 5's in the last float bits (inside the stated band), and latency-sized calls at 33..64 knots, which the three-column row-per-lane
 * kernel served, now run a lower-triangle kernel too (guarded until the latch resolves; "pcg_lqb" = 0 restores round 5's choices). */
#define MPCG_ABI_VERSION 2

typedef enum mpcg_status {
    MPCG_OK = 0,
    MPCG_ERR_INVALID = -1,      /* bad argument (null pointer, batch > max_batch, ...) */
    MPCG_ERR_UNSUPPORTED = -2,  /* state_size / knot_points outside the compiled specialisations */
    MPCG_ERR_HIP = -3,          /* a HIP runtime call failed (text in mpcg_last_error) */
    MPCG_ERR_NOMEM = -4
} mpcg_status;

/* Preconditioner stored in d_Pinv (include/pcg/linsys_setup.cuh):
 * block-Jacobi = only the diagonal blocks Pinv[k,1] are read (:202-210, 510-524);
 * symmetric stair = all three block columns (:97-136). */
typedef enum mpcg_precond {
    MPCG_PRECOND_NONE = 0,       /* mpcg_form_schur only: S and gamma, no Pinv at all (for mpcg_block_solve) */
    MPCG_PRECOND_JACOBI = 1,
    MPCG_PRECOND_SS = 3
} mpcg_precond;

typedef struct mpcg_handle mpcg_handle;

/* Library / build identification. */
int mpcg_abi_version(void);
const char *mpcg_build_info(void);

/* Handle = per-device solver context for fixed (state_size, knot_points).  Replaces the
 * per-call cudaMalloc of PCG scratch in sqpSolvePcg (include/pcg/sqp.cuh:116-135): the solver
 * needs no global scratch at all (r, p, upsilon live in LDS), the handle caches launch configuration and owns
 * device buffers: allocated here, the hand-off cells of the float cluster kernel, the dispatch-order buffer of "sched_hint",
 * the pinned word of the symmetry latch, the copy of d_lambda a cluster follow-up launch starts from (knot_points > 128)
 * and, for handles with at most 8 MB of double iterates, the double cluster kernels' buffers (GRAPH CAPTURE); from their
 * first use on, the staging buffers of mpcg_form_schur(_f64), the seam buffer of the chunk-walking Schur kernel, the
 * sweep scratch of mpcg_block_solve, that of mpcg_block_solve_f64 and the point-merit scratch of mpcg_compute_merit(_f64).  max_batch bounds `batch` of later calls.  device < 0 = current device.  One handle per
 * (device, knot_points) and per concurrently used stream: calls on the same handle must not overlap on the host
 * side (launch knobs are chosen per call) and their device work must be ordered (one stream, or events) because
 * they share those buffers; different handles are independent. */
/* state_size = 14 (IIWA-14) with control_size = 7 is the tuned specialisation.  Any other 1 <= state_size <= 64 gets a handle that
 * serves, with n x n blocks in the same layouts and with the same semantics:
 *   - the PCG entry points (mpcg_pcg_solve, mpcg_pcg_solve_ref, mpcg_pcg_solve_f64, mpcg_pcg_solve_ref_f64, mpcg_pcg_lds_bytes,
 *     mpcg_check_pcg_occupancy) through a generic, functional kernel (matrices streamed every iteration; "last_kernel_family" = 3);
 *   - mpcg_form_schur(_f64), mpcg_compute_dz(_f64), mpcg_block_solve(_f64), mpcg_prep_csr and mpcg_bd_to_csr_lowertri through run-time-dimension
 *     kernels (operands in LDS; the same operation order as the tuned ones, i.e. the same bits as the reference arithmetic restated on the
 *     CPU), for any 1 <= control_size <= state_size — also control_size != 7 on a 14-state handle.  control_size = 0 or > state_size is
 *     MPCG_ERR_INVALID.  mpcg_form_schur(_f64) needs one block row's operands, 6 n^2 + 2 n m + 2 m^2 + 12 n + 4 m elements, in 160 KiB of
 *     LDS: every m <= n <= 32 in both precisions (and e.g. 40 x 10); beyond that it returns MPCG_ERR_UNSUPPORTED.  The others serve every
 *     such handle.  batch x knot_points < 2^31.
 * mpcg_bt_spmv, mpcg_pcg_solve_f16, mpcg_generate_kkt(_f64), mpcg_compute_merit(_f64) and mpcg_probe_hbm_read return MPCG_ERR_UNSUPPORTED on a handle with state_size != 14. */
int mpcg_create(mpcg_handle **out, int device, uint32_t state_size, uint32_t knot_points, uint32_t max_batch);
int mpcg_destroy(mpcg_handle *h);
const char *mpcg_last_error(const mpcg_handle *h);   /* h may be NULL: last error of mpcg_create */

/* Replaces pcgSharedMemSize<T>(state_size, knot_points) (include/pcg/sqp.cuh:151): the dynamic LDS bytes of
 * the launch a default-configured single-trajectory solve makes (the reference passes this value as the launch's
 * smem argument; here the library launches, the number is informational but exact: it equals the
 * "last_kernel_lds_bytes" option after such a solve).  0 if the shape is unsupported.  _f64: the same for
 * linsys_t = double (mpcg_pcg_solve_ref_f64). */
size_t mpcg_pcg_lds_bytes(uint32_t state_size, uint32_t knot_points);
size_t mpcg_pcg_lds_bytes_f64(uint32_t state_size, uint32_t knot_points);

/* Replaces checkPcgOccupancy<T>(kernel, threads, n, N) (examples/track_iiwa_pcg.cu:24).  The
 * reference aborts when its N cooperative blocks cannot be co-resident; this solver has no
 * inter-workgroup dependency, so the check cannot fail for a supported shape.  Writes the number
 * of trajectories one GPU solves concurrently (workgroups/CU * CUs) to *resident_trajectories. */
int mpcg_check_pcg_occupancy(mpcg_handle *h, uint32_t *resident_trajectories);

/* THE HOT PATH.  Replaces
 *   cudaLaunchCooperativeKernel(pcg<T,n,N>, N, PCG_NUM_THREADS, args, smem)  (include/pcg/sqp.cuh:230)
 * for `batch` trajectories at once.  For trajectory b:
 *   r = gamma - S lambda; rt = Pinv r; p = rt; eta = r.rt
 *   repeat <= max_iter: ups = S p; alpha = eta / (p.ups); lambda += alpha p; r -= alpha ups;
 *                       rt = Pinv r; eta' = r.rt; if |eta'| < exit_tol stop;
 *                       p = rt + (eta'/eta) p; eta = eta'
 * d_iters[b]         = completed lambda updates            (reference: d_pcg_iters, sqp.cuh:131-132)
 * d_max_iter_exit[b] = 1 if the loop ran out of iterations (reference: d_pcg_exit,  sqp.cuh:133-135,
 *                      meaning include/mpcsim.cuh:382-387), 0 if |eta| fell below exit_tol.
 * If |eta| < exit_tol already after the setup step, 0 iterations are done and the flag is 0.
 * max_iter / exit_tol are pcg_config<T>::pcg_max_iter / pcg_exit_tol (include/mpcsim.cuh:213-216). */
int mpcg_pcg_solve(mpcg_handle *h,
                   const float *d_S, const float *d_Pinv, const float *d_gamma, float *d_lambda,
                   uint32_t batch, uint32_t max_iter, float exit_tol, mpcg_precond precond,
                   uint32_t *d_iters, uint8_t *d_max_iter_exit, void *stream);

/* Same solve for ONE trajectory with exactly the reference kernel's 12 arguments, in order
 * (include/pcg/sqp.cuh:137-150).  d_r and d_p receive the final residual and search direction
 * (the reference uses them as global scratch): at a zero-iteration exit (|eta| < exit_tol after the setup step, or
 * max_iter = 0) d_r = gamma - S lambda0 and d_p = Pinv d_r, d_lambda untouched; at a tolerance exit after k iterations
 * r_k and the p that iteration k used (not updated, as in the reference); at a max_iter exit the updated p.
 * d_v_temp and d_eta_new_temp (the reference's
 * per-block partial-sum buffers, :124-125) are accepted and left untouched.  d_pcg_exit points
 * to a 1-byte bool as in the reference.  The symmetric-stair preconditioner is assumed, as in the
 * reference (its Pinv always carries the off-diagonal blocks). */
int mpcg_pcg_solve_ref(mpcg_handle *h,
                       float *d_S, float *d_Pinv, float *d_gamma, float *d_lambda,
                       float *d_r, float *d_p, float *d_v_temp, float *d_eta_new_temp,
                       uint32_t *d_pcg_iters, uint8_t *d_pcg_exit,
                       uint32_t pcg_max_iter, float pcg_exit_tol, void *stream);

/* Building block P2/P3 of the path, exposed for measurement and reuse: batched block-tridiagonal
 * matrix-vector product  y = M x  with M in bd layout (cols = 3) or its diagonal blocks only
 * (cols = 1).  x, y: [batch][N][n]. */
int mpcg_bt_spmv(mpcg_handle *h, const float *d_M, const float *d_x, float *d_y,
                 uint32_t batch, int cols, void *stream);

/* Measurement aid, not part of the path: read `bytes` bytes at d_src once (16-byte nontemporal loads,
 * two workgroups per CU, nothing else in the kernel) — the HBM read ceiling of THIS device for
 * mpcg_bt_spmv's roofline fraction to be read against (bench.py times it next to the SpMV).
 * d_src 16-byte aligned, bytes a multiple of 16; d_sink: 4 bytes of device memory (written only
 * if the data sum to one particular value). */
int mpcg_probe_hbm_read(mpcg_handle *h, const void *d_src, size_t bytes, float *d_sink, void *stream);

/* ---- reduced-precision matrix storage (BASELINE config 5's fp16 sweep) ----
 * S and Pinv may be kept in IEEE half precision (same bd layout, 2-byte elements): half the HBM
 * footprint and half the bytes of the one load per solve.  Beyond N = 36 the register-resident
 * kernels convert the blocks to fp32 once, while loading them; all arithmetic, gamma and lambda
 * stay fp32.  The solve is then exactly the fp32 PCG of the ROUNDED matrices: its
 * answer differs from the fp32-storage answer by the storage rounding (relative 2^-11 per entry), not
 * by anything iteration-dependent; entries must be within the half range (|x| < 65504).
 * mpcg_convert_f32_to_f16: round-to-nearest-even copy of `count` elements (any bd-layout buffer).
 * mpcg_pcg_solve_f16: mpcg_pcg_solve with d_S16 / d_Pinv16 produced by the conversion. */
int mpcg_convert_f32_to_f16(mpcg_handle *h, const float *d_src, uint16_t *d_dst, size_t count, void *stream);
int mpcg_pcg_solve_f16(mpcg_handle *h,
                       const uint16_t *d_S16, const uint16_t *d_Pinv16, const float *d_gamma, float *d_lambda,
                       uint32_t batch, uint32_t max_iter, float exit_tol, mpcg_precond precond,
                       uint32_t *d_iters, uint8_t *d_max_iter_exit, void *stream);

/* ---- the steps either side of the solve, same layouts as the reference ----
 *
 * mpcg_form_schur replaces form_schur_system<T>(state_size, control_size, knot_points, d_G_dense,
 * d_C_dense, d_g, d_c, d_S, d_Pinv, d_gamma, rho) (include/pcg/linsys_setup.cuh:620-656), batched:
 *   d_G_dense [batch][(n^2+m^2)N - m^2]  in: Q_0,R_0,...,Q_{N-1} (column-major blocks);  out: their
 *             inverses with rho added (the reference's in-place side effect, :371-380, consumed by dz)
 *   d_C_dense [batch][(n^2+nm)(N-1)]     -A_k, -B_k (already negated, include/common/kkt.cuh:115-116)
 *   d_g [batch][(n+m)N - m], d_c [batch][nN]
 *   d_S, d_Pinv, d_gamma                 outputs in the layouts mpcg_pcg_solve consumes
 * Blocks (0, left) and (N-1, right) of d_S and d_Pinv lie outside the matrix: NO routing of this entry writes them (the register-resident
 * formation at any "schur_chunk", the LDS kernels of "schur_dpp" = 0 / "producers_generic" = 1 / other shapes, float and double, scalar rho
 * and _rhov alike) — they keep the caller's bytes, as in the reference (:97, 118), and no solver entry reads them.  Every other element of
 * d_S and d_gamma, and all of d_G_dense, is written by every call.
 * precond = MPCG_PRECOND_NONE writes S and gamma only (d_Pinv is not touched and may be NULL): what
 * mpcg_block_solve needs; it saves the inversion of every diagonal block of S and the completion kernel's products.
 * precond = MPCG_PRECOND_JACOBI skips the symmetric-stair completion (:9-137): the off-diagonal
 * blocks of d_Pinv are then left untouched.  The first call allocates a handle-owned staging buffer
 * of max_batch * sizeof(G) (hipMalloc — not stream-ordered); later calls are purely stream-ordered.
 * Any 1 <= control_size <= state_size (mpcg_create): other shapes than 14 x 7 run the run-time-dimension kernels, whose staging buffer is
 * sized from the largest control_size the handle has seen — a later call with a larger one re-allocates it (after a device synchronisation,
 * refused inside a stream capture like every first call).
 *
 * mpcg_form_schur_rhov is mpcg_form_schur with ONE RHO PER TRAJECTORY, read from device memory: trajectory b is formed with d_rho[b] (d_rho
 * [batch] floats).  Everything else — layouts, side effects, preconditioner choices, routing between the register-resident and the
 * run-time-dimension kernels, "schur_chunk", the handle-owned buffers and what a first call inside a stream capture is refused for — is
 * mpcg_form_schur's; the additions are the same instructions, so a trajectory's outputs are bit for bit those of the scalar call with
 * rho = d_rho[b].  Because rho is read when the kernel RUNS, a captured graph of the call follows whatever mpcg_line_search_step_rho (below) has
 * written into d_rho since.  d_rho is device data and is NOT validated: a non-positive or NaN entry gives that trajectory what the scalar call would
 * give for it, nothing else.  MPCG_ERR_INVALID for d_rho == NULL.
 *
 * mpcg_compute_dz replaces compute_dz(state_size, control_size, knot_points, d_Ginv_dense, d_C_dense,
 * d_g, d_lambda, d_dz) (include/common/dz.cuh:124-136), batched; d_dz [batch][(n+m)N - m].  Any 1 <= control_size <= state_size <= 64;
 * pure stream work from the first call on. */
int mpcg_form_schur(mpcg_handle *h, uint32_t control_size, float *d_G_dense, const float *d_C_dense,
                    const float *d_g, const float *d_c, float *d_S, float *d_Pinv, float *d_gamma,
                    float rho, uint32_t batch, mpcg_precond precond, void *stream);
int mpcg_form_schur_rhov(mpcg_handle *h, uint32_t control_size, float *d_G_dense, const float *d_C_dense,
                         const float *d_g, const float *d_c, float *d_S, float *d_Pinv, float *d_gamma,
                         const float *d_rho /* [batch] */, uint32_t batch, mpcg_precond precond, void *stream);
int mpcg_compute_dz(mpcg_handle *h, uint32_t control_size, const float *d_Ginv_dense,
                    const float *d_C_dense, const float *d_g, const float *d_lambda, float *d_dz,
                    uint32_t batch, void *stream);

/* ---- CSR side of the reference's QDLDL twin (LINSYS_SOLVE == 0) ----
 * mpcg_prep_csr replaces prep_csr<<<N,64>>>(state_size, knot_points, d_col_ptr, d_row_ind)
 * (include/utils/csr.cuh:40-73; called once per SQP solve at include/qdldl/sqp.cuh:164): pattern of the lower
 * triangle, d_col_ptr [nN+1], d_row_ind [nnz], nnz = (N-1)n^2 + N n(n+1)/2 (include/qdldl/sqp.cuh:148).
 * mpcg_bd_to_csr_lowertri gathers the values form_schur_system_qdldl leaves in d_val
 * (include/qdldl/linsys_setup.cuh:339-351) from a bd-layout S: per trajectory [nnz] floats = mult * (left
 * block, then lower triangle of the diagonal block, row by row).  With the S of mpcg_form_schur (already
 * negated) mult = +1 reproduces the reference's numbers; gamma is shared by both paths.  The CPU LDL^T that consumes
 * them: the reference's own qdldl, or mpcg_ldl_* / mpcg_qdldl_solve_schur below.  Both serve every state size a handle can have. */
int mpcg_prep_csr(mpcg_handle *h, int32_t *d_col_ptr, int32_t *d_row_ind, void *stream);
int mpcg_bd_to_csr_lowertri(mpcg_handle *h, const float *d_S, float *d_val, float mult, uint32_t batch, void *stream);

/* linsys_t = double (USE_DOUBLES=1, include/common/settings.cuh:41-49): the same solve, same semantics, in double
 * precision.  Register-resident kernels up to 512 knots with block-symmetric matrices (one CU up to 64 knots, clusters of
 * CUs beyond; 256 otherwise), the streaming kernel (S and Pinv read every iteration, iterate vectors in LDS: knot_points
 * <= 350) for "cluster" = 0 and the horizons between (Options: kernel selection).  mpcg_pcg_solve_ref_f64 carries the reference kernel's 12 arguments for pcg<double, n, N>. */
int mpcg_pcg_solve_f64(mpcg_handle *h, const double *d_S, const double *d_Pinv, const double *d_gamma, double *d_lambda,
                       uint32_t batch, uint32_t max_iter, double exit_tol, mpcg_precond precond,
                       uint32_t *d_iters, uint8_t *d_max_iter_exit, void *stream);
int mpcg_pcg_solve_ref_f64(mpcg_handle *h, double *d_S, double *d_Pinv, double *d_gamma, double *d_lambda,
                           double *d_r, double *d_p, double *d_v_temp, double *d_eta_new_temp,
                           uint32_t *d_pcg_iters, uint8_t *d_pcg_exit, uint32_t pcg_max_iter, double pcg_exit_tol,
                           void *stream);

/* The steps either side of the solve for linsys_t = double: mpcg_form_schur / mpcg_compute_dz with every float replaced by double (same
 * layouts, same side effects, same preconditioner choices).  Functional twins — one wavefront per knot, operands in LDS — in the float
 * path's operation order: bit-identical to the oracle's double instantiation (tests/test_gpu_f64.py).  Shapes other than 14 x 7: as the float
 * entry points (tests/test_gpu_generic_producers.py).  mpcg_form_schur_rhov_f64: mpcg_form_schur_rhov in double, d_rho [batch] doubles. */
int mpcg_form_schur_f64(mpcg_handle *h, uint32_t control_size, double *d_G_dense, const double *d_C_dense,
                        const double *d_g, const double *d_c, double *d_S, double *d_Pinv, double *d_gamma,
                        double rho, uint32_t batch, mpcg_precond precond, void *stream);
int mpcg_form_schur_rhov_f64(mpcg_handle *h, uint32_t control_size, double *d_G_dense, const double *d_C_dense,
                             const double *d_g, const double *d_c, double *d_S, double *d_Pinv, double *d_gamma,
                             const double *d_rho /* [batch] */, uint32_t batch, mpcg_precond precond, void *stream);
int mpcg_compute_dz_f64(mpcg_handle *h, uint32_t control_size, const double *d_Ginv_dense,
                        const double *d_C_dense, const double *d_g, const double *d_lambda, double *d_dz,
                        uint32_t batch, void *stream);


/* Batched block-tridiagonal DIRECT solve of S lambda = gamma — the GPU-native counterpart of the reference's second
 * linear-system path (LINSYS_SOLVE == 0: qdldl_solve_schur, include/qdldl/sqp.cuh:22-49, called at :261-282 with
 * D2H(values, gamma) + CPU LDL^T + H2D(lambda) inside the timed region).  Reads d_S / d_gamma exactly as
 * mpcg_form_schur (or form_schur_system) left them, writes d_lambda (no warm start: lambda is output only).
 * Block LU without pivoting, pivot blocks eliminated by the reference's Gauss-Jordan scheme; four trajectories per
 * wavefront, serial in the knot index — the throughput solver for batches (1/50 of the flops of 167 PCG iterations),
 * while mpcg_pcg_solve keeps warm starts and the tolerance knob.  fp32 at cond ~1e5: relative error ~3e-4.
 * state_size != 14: one workgroup per trajectory with Delta_k, [U_k | y_k] and L_k in LDS, the same operation order and bits; every
 * state size a handle can have.
 * Scratch (max_batch x N x (n^2 + n) floats; 210 per knot at n = 14) is owned by the handle; the first call allocates it, later calls are
 * pure stream work (capturable into a graph).
 * Option "block_solve_f64" = 1 (default 0; any other value is MPCG_ERR_INVALID; read when the call is made, so a captured graph keeps what it
 * was captured with): float64 inside, float outputs — the same float d_S / d_gamma are widened on load (exact), the sweep and the back
 * substitution run in double through the scratch of mpcg_block_solve_f64 (allocated by the first such call, as there), and lambda is rounded
 * to float once, on store: the bits of the double sweep on the widened data, rounded.  A pivot-free block LU in float loses what the condition
 * number takes; on the 128-knot iiwa systems of the tests (cond 1e7) the float sweep is at 2e-3 of max |lambda|, this one at 3e-5.  With 0
 * nothing about the call changes. */
int mpcg_block_solve(mpcg_handle* h, const float* d_S, const float* d_gamma, float* d_lambda, uint32_t batch,
                     void* stream);

/* The same solve with linsys_t = double: reads d_S / d_gamma exactly as mpcg_form_schur_f64 left them (bd layout, stored negated, blocks
 * (0, left) and (N-1, right) never read), d_lambda is output only; the same errors in the same order (null pointer: MPCG_ERR_INVALID;
 * batch == 0: MPCG_OK, nothing launched; batch > max_batch: MPCG_ERR_INVALID).  The operation order of mpcg_block_solve with every
 * operation in double: bit-identical to the reference arithmetic restated on the CPU in double.  state_size 14: one trajectory per
 * wavefront, the columns of [Delta_k | U_k y_k] dealt over the four 16-lane DPP rows (csrc/block_solve.hip.h) at EVERY batch size —
 * the four-trajectories-per-wavefront layout is not built in double (its live set, ~100 doubles per lane, does not fit the register file
 * without spilling), so "block_solve_wide" is ignored by this entry and by "block_solve_f64" = 1.  Every other state size (1..64), and 14
 * under "producers_generic" = 1: the run-time-dimension LDS kernel in double (133,664 bytes of LDS at n = 64); same bits.
 * Scratch: a second handle-owned buffer, max_batch x N x (n^2 + n) doubles, allocated by the first call of this entry or of
 * mpcg_block_solve under "block_solve_f64" = 1 (refused on a capturing stream: GRAPH CAPTURE), freed by mpcg_destroy; the float solve's
 * scratch is never resized, freed or shared, so a captured float solve stays valid.  Later calls are pure stream work. */
int mpcg_block_solve_f64(mpcg_handle *h, const double *d_S, const double *d_gamma, double *d_lambda, uint32_t batch,
                         void *stream);

/* ---- the producer of the path's inputs: KKT block assembly ----
 * mpcg_generate_kkt replaces generate_kkt_submatrices<T><<<knot_points, KKT_THREADS, smem>>>(state_size, control_size, knot_points,
 * d_G_dense, d_C_dense, d_g, d_c, d_dynMem_const, timestep, d_eePos_traj, d_xs, d_xu) (include/common/kkt.cuh:22-163, launched at
 * include/pcg/sqp.cuh:190-204), batched, with the plant functions it calls (include/dynamics/iiwa/iiwa_eepos_plant.cuh:
 * forwardDynamicsAndGradient, trackingCostGradientAndHessian(_lastblock)) and the Euler integrator of
 * include/common/integrator.cuh.  Outputs in the layouts mpcg_form_schur consumes (C holds -A, -B; c_0 = x_0 - x_s).
 * The reference's d_dynMem_const (GRiD's robotModel) becomes an mpcg_plant: the robot as DATA — a fixed-base serial chain
 * of revolute joints given by the tables GRiD tabulates (all column-major; *_trig: entry idx = coef * sin(q_j) for j < nj,
 * coef * cos(q_{j-nj}) otherwise, replacing the constant at idx):
 *   X_const [nj*36] spatial transforms parent -> link, I_spatial [nj*36] spatial inertias, Xhom_const [nj*16] homogeneous
 *   transforms link -> parent.  mpcgpu_amd/data/iiwa14_model.json carries the KUKA iiwa 14 in exactly this form.
 * The cost is the reference's end-effector tracking cost: 1/2 |ee(q_k) - goal_k|^2 (xyz of d_eePos_traj [batch][N][6]) +
 * 1/2 qd_cost |qd|^2 + 1/2 r_cost |u|^2 with its Gauss-Newton Hessian.  Derivatives of the forward dynamics (the A, B blocks) come from the
 * ANALYTIC gradient recursion of the inverse dynamics — what the reference computes with GRiD's forwardDynamicsAndGradient
 * (iiwa_eepos_plant.cuh:127-155): a lane per column (7 x d/dq, 7 x d/dqd) propagates (dv, da) up the chain and dF down, next to the nominal
 * recursion in a 15th lane (csrc/kkt_plant.hip.h) — then -Minv dID; float64 on the device, float outputs.  Option "kkt_analytic" = 0 selects
 * the CHECKER instead: one-sided float64 differences (ID(. + h e_j) - u) / h, h = 3e-8 (the default of rounds 2-3).  Both agree with the float64
 * central-difference host restatement (oracle/iiwa_ref.py) to ~2e-7, the rounding of the float outputs; the analytic recursion stays there for
 * torques of any size (no (ID - u) / h term that amplifies what the explicitly inverted mass matrix leaves of ID(FD(u)) - u).
 * num_joints = 7 is the compiled specialisation.
 * mpcg_plant_create checks what the device kernel relies on and returns MPCG_ERR_UNSUPPORTED / MPCG_ERR_INVALID otherwise: every joint
 * rotates about its own z axis (X_k(q) = blkdiag(Rz(q), Rz(q)) X_k(0), the form of GRiD's tables), the spatial inertias are symmetric and of
 * the rigid-body form [[Ibar, skew(m c)], [skew(m c)^T, m 1]], and Xhom describes the same chain as X (the end-effector position and
 * Jacobian are taken from the spatial transforms on the device; Xhom is used for that consistency check only).
 * THE INTEGRATOR.  Option "integrator" = 0 (default) is explicit Euler, both updates from the old values: A = I + dt [[0, I], [dqdd/dq, dqdd/dqd]],
 * B = dt [0; Minv], c_{k+1} = x_{k+1} - (x_k + dt [qd; qdd]).  "integrator" = 1 is SEMI-IMPLICIT (symplectic) Euler, INTEGRATOR_TYPE == 1 of the reference
 * (include/common/integrator.cuh:22-57 defect, :59-100 A and B, :103-130 step; a template parameter of generate_kkt_submatrices, kkt.cuh:22): with the
 * same qdd = FD(q_k, qd_k, u_k),  qd' = qd + dt qdd,  q' = q + dt qd', so
 *   c_{k+1} = x_{k+1} - [q + dt (qd + dt qdd) ; qd + dt qdd]                   (c_0 = x_0 - x_s unchanged)
 *   A = I + dt [[dt dqdd/dq, I + dt dqdd/dqd], [dqdd/dq, dqdd/dqd]]            (the lower half unchanged, the upper half gains dt^2 x its derivative blocks)
 *   B = [dt^2 Minv ; dt Minv]                                                   (the top half is no longer zero)
 * stored as before (C = -A, -B, column-major); costs, layouts and the last-block quirk are unchanged.  The option is read when the call is made (a captured
 * graph keeps what it was captured with), takes 0 or 1 (anything else: MPCG_ERR_INVALID, the value stays) and is orthogonal to "kkt_analytic" and "kkt_f32":
 * every build has its semi-implicit instantiation (a compile-time parameter of the kernel: no run-time branch, the explicit instantiations are unchanged),
 * and mpcg_generate_kkt_f64 honours it too.  mpcg_compute_merit(_f64) reads the SAME option: a line search must measure the map this call linearised.
 * GRAVITY.  The reference hands gato_plant::GRAVITY<T>() (include/dynamics/iiwa/iiwa_eepos_plant.cuh:51) to every GRiD call, and GRiD uses it as the
 * acceleration the chain's root starts from: a_1 = X_1[:, 5] * gravity, a base spatial acceleration [0 0 0 0 0 g].  Here that is model data of the plant:
 * base_accel, the LINEAR spatial acceleration of the root in the base frame, three numbers.  GRiD's scalar g is base_accel = {0, 0, g}.  SIGN: it is the
 * acceleration the base is given, so the physical gravitational acceleration is its NEGATIVE — {0, 0, +9.81} models an arm standing on the ground with z
 * up (gravity pulls along -z).  mpcg_plant_create and mpcg_plant_create_iiwa14 make plants with {0, 0, 0}: the reference's constant is 0 because its iiwa
 * is gravity-compensated, and every output of such a plant is bit for bit what it was before the vector existed.  mpcg_plant_clone_gravity makes the plant
 * with another vector.  mpcg_generate_kkt(_f64), mpcg_compute_merit(_f64), mpcg_simulate(_f64) and mpcg_inverse_dynamics(_f64) all read the vector from the
 * plant THEY ARE GIVEN (every build: both gradient routes, "kkt_f32", "merit_f32", both integrators), so the controller's model and the simulated plant may
 * differ in it, as they may in "sim_integrator".  It enters the bias ID(q, qd, 0) — hence qdd = Minv (u - bias), A, B, the defects, the merit's violation
 * terms and the simulated state — and nothing else: the inertia matrix and the end-effector pose do not depend on it.
 *   mpcg_plant_clone_gravity   *out = a NEW plant, the tables of src with base_accel; src is not touched.  A clone and not a setter: kernels read the model
 *                              as invariant data and captured graphs keep the pointer, so a plant never changes after creation.  The clone owns its own
 *                              device allocation (on src's device); source and clone may be destroyed in either order.  It allocates and copies
 *                              (hipMalloc, blocking hipMemcpy), as mpcg_plant_create does: neither is stream work, neither may be called while a stream
 *                              of the calling thread is being captured.  MPCG_ERR_INVALID: a NULL argument or a non-finite component (*out = NULL).
 *   mpcg_plant_get_gravity     the plant's vector ({0, 0, 0} for mpcg_plant_create / _create_iiwa14); MPCG_ERR_INVALID: a NULL argument.
 * LIMITS.  The reference has no inequality constraints.  Here a plant may carry SOFT joint, velocity and torque limits as model data, like its gravity: per
 * joint a lower and an upper bound on q, qd and u (-INFINITY / +INFINITY: no bound on that side), one weight per kind, and flags.  With
 *     viol(x; lo, hi) = x > hi ? x - hi : (x < lo ? x - lo : 0)          (strict comparisons: a value ON a bound violates nothing, and neither does a NaN)
 * the running cost of the _xuref entries (below) given such a plant gains the one-sided quadratic penalty
 *     J_k += 1/2 q_weight sum_i viol(q_i)^2 + 1/2 qd_weight sum_i viol(qd_i)^2 + [k < N-1] 1/2 u_weight sum_i viol(u_i)^2.
 * It is C^1 and its Gauss-Newton Hessian is a non-negative diagonal, so mpcg_generate_kkt_xuref(_f64) adds w [viol != 0] to Q_k[i, i], Q_k[7 + i, 7 + i] and
 * R_k[i, i] and w viol to q_k[i], q_k[7 + i] and r_k[i] (the last block at x_{N-1}, where its joint-space terms are) — C and c are untouched, and the Schur
 * formation, both solvers, dz, the line search and the rho rule take it as they are.  mpcg_compute_merit_xuref(_f64) adds exactly the sum above, every knot at
 * its own state.  Every build honours it (both gradient routes, "kkt_f32" = 1 and 2, "merit_f32", both integrators, float and double) as one more value of the
 * kernels' compile-time cost, launched exactly when the plant given has limits: a plant without limits runs the device code it ran before.  The float builds
 * ("kkt_f32", "merit_f32") use the bounds and weights ROUNDED TO FLOAT; every other build, the float entries' default included, uses them as doubles.
 * A NaN state or control violates no bound: it adds nothing here and poisons what it poisoned before, its own trajectory only.
 * The PLAIN entries mpcg_generate_kkt(_f64) and mpcg_compute_merit(_f64) given a plant with limits return MPCG_ERR_UNSUPPORTED and launch nothing: use the
 * _xuref entries with the neutral cost (ee_cost = 1, q_cost = 0, no flags) — the two families differ in where the last block's velocity term is evaluated,
 * and a silent switch would change numbers.  mpcg_inverse_dynamics(_f64) ignores limits.
 * MPCG_LIMITS_SIM_SATURATE: mpcg_simulate(_f64) given such a plant clamps every control it applies to [u_lo, u_hi] (the double bounds, in either entry; a NaN
 * control passes) where it is loaded and widened — the actuator saturates — and changes nothing else.  Without the flag mpcg_simulate ignores limits.  The
 * controller's plant and the simulated plant may differ in this, as they may in gravity.
 *   mpcg_plant_clone_limits    *out = a NEW plant, the tables AND GRAVITY of src with the limits given (replacing any src had); a gravity clone of a limits
 *                              plant keeps its limits.  A clone and not a setter, with the allocation and capture rules of mpcg_plant_clone_gravity.
 *                              MPCG_ERR_INVALID (*out = NULL): a NULL argument; a NaN bound; lo > hi; lo = +inf or hi = -inf; a weight that is negative
 *                              or not finite; an unknown flag bit.
 *   mpcg_plant_get_limits      *has_limits = 1 and *out = the limits as given for a limits clone; 0 for any other plant (*out: no bounds, zero weights, no
 *                              flags).  MPCG_ERR_INVALID: a NULL argument. */
#define MPCG_LIMITS_SIM_SATURATE 1u
typedef struct mpcg_limits {
    double q_lo[7], q_hi[7], qd_lo[7], qd_hi[7], u_lo[7], u_hi[7]; /* -INFINITY / +INFINITY: no bound on that side */
    double q_weight, qd_weight, u_weight;                          /* finite, >= 0 */
    uint32_t flags;                                                /* MPCG_LIMITS_* */
} mpcg_limits;
typedef struct mpcg_plant mpcg_plant;
int mpcg_plant_create(mpcg_plant **out, int device, uint32_t num_joints, const double *X_const, const double *I_spatial,
                      const double *Xhom_const, const int32_t *X_trig_idx, const double *X_trig_coef, const int32_t *X_trig_j,
                      uint32_t n_X_trig, const int32_t *Xhom_trig_idx, const double *Xhom_trig_coef, const int32_t *Xhom_trig_j,
                      uint32_t n_Xhom_trig);
/* The KUKA LBR iiwa 14 of the reference from the tables built into the library (the same numbers as mpcgpu_amd/data/iiwa14_model.json):
 * replaces gato_plant::initializeDynamicsConstMem<T>() (include/dynamics/iiwa/iiwa_eepos_plant.cuh:63-66, called at include/mpcsim.cuh:194). */
int mpcg_plant_create_iiwa14(mpcg_plant **out, int device);
int mpcg_plant_clone_gravity(mpcg_plant **out, const mpcg_plant *src, const double base_accel[3]);
int mpcg_plant_get_gravity(const mpcg_plant *p, double out[3]);
int mpcg_plant_clone_limits(mpcg_plant **out, const mpcg_plant *src, const mpcg_limits *lim);
int mpcg_plant_get_limits(const mpcg_plant *p, mpcg_limits *out, int *has_limits);
int mpcg_plant_destroy(mpcg_plant *p);
/* mpcg_inverse_dynamics: d_tau[i] = ID(q_i, qd_i, qdd_i) of the plant, ITS GRAVITY INCLUDED, for count independent states (arrays [count][7]; d_qd and
 * d_qdd may each be NULL: zero).  With both NULL it returns the gravity torques — what the controls of a plan made for zero gravity must gain before a
 * loop over a gravity clone starts from it (u' = u + ID(q, 0, 0) keeps qdd, hence the plan a solution).  Float64 inside like the other plant kernels, the
 * sweep their bias lane runs (csrc/invdyn_plant.hip.h); the float entry rounds once on store, the _f64 entry reads and stores doubles.  Pure stream work
 * from the first call on (capturable); a state's result does not depend on the rest of the call.
 *   MPCG_ERR_INVALID       a NULL handle, plant, d_q or d_tau; count > max_batch x knot_points of the handle; a plant on another device
 *   MPCG_ERR_UNSUPPORTED   a handle whose state_size is not 14
 *   count == 0             MPCG_OK, nothing launched */
int mpcg_inverse_dynamics(mpcg_handle *h, const mpcg_plant *plant, const float *d_q, const float *d_qd /* NULL: 0 */,
                          const float *d_qdd /* NULL: 0 */, float *d_tau, uint32_t count, void *stream);
int mpcg_inverse_dynamics_f64(mpcg_handle *h, const mpcg_plant *plant, const double *d_q, const double *d_qd /* NULL: 0 */,
                              const double *d_qdd /* NULL: 0 */, double *d_tau, uint32_t count, void *stream);
int mpcg_generate_kkt(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size, float timestep, const float *d_eePos_traj,
                      const float *d_xs, const float *d_xu, float qd_cost, float r_cost, float *d_G_dense, float *d_C_dense,
                      float *d_g, float *d_c, uint32_t batch, void *stream);
/* mpcg_generate_kkt_f64: the producer of mpcg_form_schur(_rhov)_f64 (linsys_t = double, the reference's USE_DOUBLES build).  The same kernel arithmetic —
 * float64 inside, either gradient route of "kkt_analytic" — with every array in double: d_xu, d_xs and d_eePos_traj are read as doubles and used as they
 * are (no pass through float), timestep and the costs arrive as doubles, and the four outputs are the float64 values mpcg_generate_kkt rounds to float on
 * store — on float-representable inputs, rounding this entry's outputs to float gives mpcg_generate_kkt's bits.  Layouts, errors, batch == 0 and capture
 * behaviour are mpcg_generate_kkt's: pure stream work from the first call on.  "kkt_f32" does NOT apply to this entry (it selects a float build of the
 * float entry and is ignored here).  LDS and residency as the float entry's (csrc/kkt_plant.hip.h: a knot's outputs leave through the record region in
 * three pieces of at most 308 doubles). */
int mpcg_generate_kkt_f64(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size, double timestep, const double *d_eePos_traj,
                          const double *d_xs, const double *d_xu, double qd_cost, double r_cost, double *d_G_dense, double *d_C_dense,
                          double *d_g, double *d_c, uint32_t batch, void *stream);

/* ---- the stage behind dz: merit function and line search on the device ----
 * mpcg_compute_merit replaces the eight cooperative launches of ls_gato_compute_merit (include/common/merit.cuh:16-94, launched at
 * include/pcg/sqp.cuh:264-282) and compute_merit (merit.cuh:99-143), batched over trajectories AND step sizes in one call: for trajectory b and
 * step size a, at the trial iterate z = xu_b + step_sizes[a] * dz_b,
 *   d_merit[b][a] = sum_{k<N} J_k + mu ( sum_{k<N-1} | x_{k+1} - (x_k + dt [qd_k ; qdd_k]) |_1  +  [d_xs given] | x_0 - xs_b |_1 )
 *   J_k = 1/2 |ee(q_k) - goal_k[0:3]|^2 + 1/2 qd_cost |qd_k|^2 + [k < N-1] 1/2 r_cost |u_k|^2
 * with the plant functions the reference calls (gato_plant::trackingcost, include/dynamics/iiwa/iiwa_eepos_plant.cuh:242-290; integratorError
 * with the Euler integrator, include/common/integrator.cuh; forward dynamics of the mpcg_plant given, with that plant's gravity — GRAVITY under mpcg_plant_create —, as mpcg_generate_kkt).  The last
 * knot's cost is evaluated at its own state x_{N-1} against goal_{N-1} (merit.cuh:62) — not at x_{N-2} as the KKT stage's _lastblock does.
 * The initial-state term is what ls_gato_compute_merit adds in its last block (merit.cuh:68-77); the reference's compute_merit, which gives
 * the merit the line search compares against, leaves it out (:133-135): d_xs = NULL reproduces that.  Pass the same d_xs for both and all
 * numbers of a line search are the same function.
 *   step_sizes   HOST array of num_steps (1 .. MPCG_MAX_STEP_SIZES) values, copied into the launch (a captured graph keeps them); the
 *                reference's are -1 / 2^p (merit.cuh:47).  d_dz may be NULL if every step size is 0.
 *   d_merit      [batch][num_steps] floats
 * The trial iterate is formed in float with ONE rounding, fmaf(step, dz, xu) — with step 0 it is xu exactly — and everything behind it runs
 * in float64 (csrc/merit_plant.hip.h: the KKT kernel's round 0, a 16-lane group per (trajectory, step size, knot)); option "kkt_f32" does not
 * affect it — the merit has an option of its own: "merit_f32" = 1 (default 0) evaluates every point merit in PACKED FLOAT instead
 * (csrc/merit_plant_f32.hip.h: the reference's own arithmetic, merit.cuh with T = float; two items per 16-lane group, the float trial iterate used
 * as is, float model tables, sine / cosine in double and rounded; the seven lane shares of an item added in float, the knots of a row in
 * double as before, in the same scratch), for every call of the handle whatever its size.  The option is read when the call is made (a captured
 * graph keeps the build it was captured with); arguments, errors, the first-call allocation and mpcg_line_search_step(_rho) are the same, and
 * "kkt_f32" and "merit_f32" are independent.  With it a merit is within 1e-5 of the float64 restatement relative to max(1, |merit|) — the tested
 * limit; a numpy float32 restatement of the formula is within 2.5e-6 on the tests' inputs, the default within 5e-8 —, bitwise reproducible, independent of the batch and of the other step sizes all the same — which items share a
 * lane group depends on the call, a half's arithmetic does not — and the accepted merit is still the merit of the new iterate bit for bit.  Every sum has a fixed order (no atomics — the reference's atomicAdd is not reproduced): results are bitwise reproducible and a
 * number depends neither on the rest of the batch nor on the other step sizes of the call.  state_size 14 / control_size 7 only
 * (MPCG_ERR_UNSUPPORTED otherwise).  The first call allocates a handle-owned scratch of max_batch x 16 x knot_points doubles (hipMalloc — not
 * stream work: GRAPH CAPTURE above); later calls are pure stream work.
 * Option "integrator" = 1 (default 0; the option mpcg_generate_kkt reads — one knob for both on purpose) replaces the violation of a knot by that of the
 * semi-implicit Euler step (the reference's merit kernels take INTEGRATOR_TYPE as a template parameter, include/common/merit.cuh:99; integrator.cuh:22-57):
 *   | x_{k+1} - [q_k + dt (qd_k + dt qdd_k) ; qd_k + dt qdd_k] |_1
 * in the default build, with "merit_f32" = 1 and in mpcg_compute_merit_f64 alike; costs, the initial-state term, the one-rounding trial iterate and the
 * fixed-order sums are unchanged.  Read when the call is made.  With d_xs given and step size 0, merit(mu + 1) - merit(mu) is the 1-norm of the d_c
 * mpcg_generate_kkt stores under the same option value, to rounding (tested in double).
 *
 * mpcg_line_search_step is the reference's step selection and update (include/pcg/sqp.cuh:292-301, 317, 332-338, 352), per trajectory b:
 *   best = d_merit_ref[b]; p = -1;  for i in 0 .. num_steps-1: if (d_merit[b][i] < best) { best = d_merit[b][i]; p = i; }
 * (strict: the first of equals wins, a value equal to d_merit_ref is no improvement, a NaN never wins), then d_step[b] = p and, if p >= 0,
 * d_merit_ref[b] = best and every element xu = fmaf(step_sizes[p], dz, xu) — the very float mpcg_compute_merit evaluated, so the merit of the new
 * iterate at step size 0 IS the new d_merit_ref, bit for bit.  p = -1 leaves d_xu and d_merit_ref untouched.  No dynamics: every handle shape,
 * any 1 <= control_size <= state_size; d_dz, d_xu [batch][(n+m)N - m].  Pure stream work from the first call on.
 *
 * mpcg_line_search_step_rho is that step followed by the reference's rho adaptation (include/pcg/sqp.cuh:304-320), with rho, its growth
 * factor drho and a "finished" flag as device state per trajectory — d_rho is the vector mpcg_form_schur_rhov reads, so a batched SQP iteration
 * adapts rho without reading anything back, and one captured iteration replays for a whole solve.  Per trajectory b:
 *   d_done[b] != 0:  d_step[b] = MPCG_STEP_FROZEN and NOTHING else is written (d_xu, d_merit_ref, d_rho, d_drho, d_done stay as they are).  Any
 *                    non-zero value freezes: the caller may set the flag itself, e.g. on convergence.
 *   otherwise:       p, d_step, d_merit_ref and d_xu exactly as mpcg_line_search_step (the same code), then in float, one rounding per
 *                    operation, correctly rounded divisions:
 *                      p <  0 (no step):  drho = fmaxf(drho * rho_factor, rho_factor);        rho = fmaxf(rho * drho, rho_min);
 *                                         if (rho > rho_max) { rho = rho_reset; d_done[b] = 1; }     (the reference gives the solve up)
 *                      p >= 0:            drho = fminf(drho / rho_factor, 1.0f / rho_factor);  rho = fmaxf(rho * drho, rho_min)
 * The reference's constants: rho_factor 1.2, rho_min 1e-3, rho_max 10, rho_reset the caller's.  Finished trajectories are not compacted away:
 * the other stages keep computing them (wasted work, never wrong — this call no longer changes them).  d_rho, d_drho are device data and
 * are not validated.  Pure stream work from the first call on.
 *
 * All three calls:  MPCG_ERR_INVALID      a null required pointer; num_steps 0 or > MPCG_MAX_STEP_SIZES; batch > max_batch; d_dz == NULL with a
 *                                    non-zero step size; a plant on another device than the handle's; control_size 0 or > state_size (step);
 *                                    mpcg_line_search_step_rho: d_rho, d_drho or d_done NULL, a parameter that is not finite,
 *                                    rho_factor <= 1, rho_min <= 0, rho_max < rho_min
 *              MPCG_ERR_UNSUPPORTED  mpcg_compute_merit on anything but state_size 14 / control_size 7
 *              MPCG_OK               batch == 0: nothing is launched */
#define MPCG_MAX_STEP_SIZES 16
int mpcg_compute_merit(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size, float timestep,
                       const float *d_eePos_traj, const float *d_xs /* may be NULL */, const float *d_xu,
                       const float *d_dz /* may be NULL if every step size is 0 */,
                       const float *step_sizes /* HOST, num_steps values, copied into the launch */, uint32_t num_steps,
                       float mu, float qd_cost, float r_cost, float *d_merit /* [batch][num_steps] */,
                       uint32_t batch, void *stream);
int mpcg_line_search_step(mpcg_handle *h, uint32_t control_size, const float *d_merit, const float *step_sizes, uint32_t num_steps,
                          float *d_merit_ref /* [batch] in/out */, const float *d_dz, float *d_xu /* in/out */,
                          int32_t *d_step /* [batch] out */, uint32_t batch, void *stream);
#define MPCG_STEP_FROZEN (-2)
int mpcg_line_search_step_rho(mpcg_handle *h, uint32_t control_size, const float *d_merit, const float *step_sizes, uint32_t num_steps,
                              float *d_merit_ref /* [batch] in/out */, const float *d_dz, float *d_xu /* in/out */,
                              int32_t *d_step /* [batch] out */, float *d_rho /* [batch] in/out */, float *d_drho /* [batch] in/out */,
                              uint8_t *d_done /* [batch] in/out */, float rho_factor, float rho_min, float rho_max, float rho_reset,
                              uint32_t batch, void *stream);
/* The double twins (linsys_t = double): the consumers of mpcg_compute_dz_f64 and the producer of the rho vector mpcg_form_schur_rhov_f64 reads.  Everything
 * said above holds with every float replaced by double — layouts, side effects, error codes, batch == 0, capture behaviour:
 *   mpcg_compute_merit_f64         the trial iterate is fma(step, dz, xu) in DOUBLE with one rounding (step 0 reads no dz), the same float64 kernel behind
 *                                  it, the same scratch (shared with mpcg_compute_merit: whichever is called first allocates it, later calls of either
 *                                  are pure stream work) and the same fixed sum order; d_merit receives the double row sums themselves, with no final
 *                                  rounding.  "merit_f32" does NOT apply (it is ignored by this entry).
 *   mpcg_line_search_step_f64      strict <, the first of equals wins, a NaN never wins; xu = fma(step_sizes[p], dz, xu) — the very double
 *                                  mpcg_compute_merit_f64 evaluated, so the merit of the new iterate at step size 0 is the new d_merit_ref bit for bit.
 *   mpcg_line_search_step_rho_f64  the rho rule in double, one rounding per operation (correctly rounded products and quotients, fmax / fmin); the
 *                                  frozen and give-up semantics are unchanged. */
int mpcg_compute_merit_f64(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size, double timestep,
                           const double *d_eePos_traj, const double *d_xs /* may be NULL */, const double *d_xu,
                           const double *d_dz /* may be NULL if every step size is 0 */,
                           const double *step_sizes /* HOST, num_steps values, copied into the launch */, uint32_t num_steps,
                           double mu, double qd_cost, double r_cost, double *d_merit /* [batch][num_steps] */,
                           uint32_t batch, void *stream);
int mpcg_line_search_step_f64(mpcg_handle *h, uint32_t control_size, const double *d_merit, const double *step_sizes, uint32_t num_steps,
                              double *d_merit_ref /* [batch] in/out */, const double *d_dz, double *d_xu /* in/out */,
                              int32_t *d_step /* [batch] out */, uint32_t batch, void *stream);
int mpcg_line_search_step_rho_f64(mpcg_handle *h, uint32_t control_size, const double *d_merit, const double *step_sizes, uint32_t num_steps,
                                  double *d_merit_ref /* [batch] in/out */, const double *d_dz, double *d_xu /* in/out */,
                                  int32_t *d_step /* [batch] out */, double *d_rho /* [batch] in/out */, double *d_drho /* [batch] in/out */,
                                  uint8_t *d_done /* [batch] in/out */, double rho_factor, double rho_min, double rho_max, double rho_reset,
                                  uint32_t batch, void *stream);

/* ---- joint-space reference cost (xu_ref): mpcg_generate_kkt and mpcg_compute_merit with a generalised running cost ----
 * The cost the calls above know is the end-effector plant's (include/dynamics/iiwa/iiwa_eepos_plant.cuh).  The _xuref entries add the reference's other
 * plant (include/dynamics/iiwa/iiwa_plant.cuh: a joint-space plan tracked with Q_cost |q - q_ref|^2, QD_cost |qd - qd_ref|^2, R_cost |u|^2) and contain
 * both as special cases.  Trajectory b, knot k; the plan row ref = [q_ref(7), qd_ref(7), u_ref(7)]:
 *
 *     J_k = 1/2 ee_cost |ee(q_k) - goal_k[0:3]|^2 + 1/2 q_cost |q_k - q_ref|^2 + 1/2 qd_cost |qd_k - [QD_RELATIVE] qd_ref|^2
 *           + [k < N-1] 1/2 r_cost |u_k - [U_RELATIVE] u_ref|^2
 *     row(b, k) = clamp(off_b + k, 0, traj_steps - 1), evaluated in 64-bit;  off_b = d_traj_offset ? d_traj_offset[b] : 0
 *     plan_b    = d_xu_traj + b * traj_batch_stride * 21      (stride 0: one plan shared by the batch) — the plan, stride and offsets of mpcg_advance_horizon
 *
 * mpcg_generate_kkt_xuref(_f64) stores, in mpcg_generate_kkt(_f64)'s layouts and with its C, c, integrators ("integrator"), builds ("kkt_analytic", "kkt_f32")
 * and plant gravity (gq = J^T (ee - goal)):
 *     Q_k = blkdiag(ee_cost gq gq^T + q_cost I, qd_cost I),   R_k = r_cost I,
 *     q_k = [ee_cost gq + q_cost (q - q_ref); qd_cost (qd - [QD_RELATIVE] qd_ref)],   r_k = r_cost (u - [U_RELATIVE] u_ref).
 *   The last block (Q_{N-1}, q_{N-1}): the JOINT-SPACE terms are evaluated at x_{N-1} against row(b, N-1) (iiwa_plant.cuh:300-323; where the merit evaluates them).
 *   Its END-EFFECTOR term keeps the quirk of mpcg_generate_kkt (_lastblock): the pose of x_{N-2} against goal_{N-1} — the pose of x_{N-1} is not computed.
 *   ee_cost = 0, q_cost > 0, flags = QD_RELATIVE is iiwa_plant.cuh.  ee_cost = 1, q_cost = 0, flags = 0 gives mpcg_generate_kkt's numbers (a -0 may become +0)
 *   except the seven qd entries of q_{N-1}: qd_cost qd_{N-1}, not qd_cost qd_{N-2}.
 * mpcg_compute_merit_xuref(_f64) is mpcg_compute_merit(_f64) with J_k above, every knot (the last included) at its own state against its own row; violation
 *   terms, mu, d_xs, the one-rounding trial iterate, the fixed-order sums, "merit_f32" and the shared scratch with its first-call allocation are unchanged, and
 *   mpcg_line_search_step(_rho)(_f64) follow it as they are.
 * A plant with LIMITS (mpcg_plant_clone_limits, above) adds its penalty to J_k in both calls; these entries are the only ones that honour it.
 *
 * mpcg_xuref is a HOST struct, copied into the launch: a captured graph keeps its scalars and pointers.  d_traj_offset is DEVICE data read when the kernel
 * runs and is not validated (the clamp keeps every read inside the plan): a captured graph follows what mpcg_advance_horizon has written since.
 * The plan needs element alignment only; no byte outside traj_steps (+ (batch - 1) traj_batch_stride) rows of 21 elements is read.
 * d_eePos_traj may be NULL exactly when ee_cost == 0.
 *   MPCG_ERR_INVALID, nothing launched or written: ref or d_xu_traj NULL; traj_steps == 0; 0 < traj_batch_stride < traj_steps; a negative or non-finite
 *     ee_cost / q_cost; an unknown flag bit; d_eePos_traj NULL with ee_cost != 0; everything mpcg_generate_kkt / mpcg_compute_merit refuse.
 *   MPCG_ERR_UNSUPPORTED: anything but state_size 14 / control_size 7.  batch == 0: MPCG_OK.  Capture rules: those of the parent entries. */
#define MPCG_XUREF_QD_RELATIVE 1u
#define MPCG_XUREF_U_RELATIVE  2u
typedef struct mpcg_xuref {
    const void    *d_xu_traj;         /* plan rows of 21 elements of the ENTRY's type: float for the float entries, double for _f64 */
    uint32_t       traj_steps;        /* >= 1 */
    uint32_t       traj_batch_stride; /* 0 or >= traj_steps */
    const int32_t *d_traj_offset;     /* [batch] or NULL (= 0): device data, read when the kernel runs */
    double         ee_cost, q_cost;   /* finite, >= 0 */
    uint32_t       flags;             /* MPCG_XUREF_* */
} mpcg_xuref;
int mpcg_generate_kkt_xuref(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size, float timestep,
                            const float *d_eePos_traj /* may be NULL if ee_cost == 0 */, const float *d_xs, const float *d_xu,
                            float qd_cost, float r_cost, const mpcg_xuref *ref, float *d_G_dense, float *d_C_dense, float *d_g, float *d_c,
                            uint32_t batch, void *stream);
int mpcg_generate_kkt_xuref_f64(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size, double timestep,
                                const double *d_eePos_traj /* may be NULL if ee_cost == 0 */, const double *d_xs, const double *d_xu,
                                double qd_cost, double r_cost, const mpcg_xuref *ref, double *d_G_dense, double *d_C_dense, double *d_g, double *d_c,
                                uint32_t batch, void *stream);
int mpcg_compute_merit_xuref(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size, float timestep,
                             const float *d_eePos_traj /* may be NULL if ee_cost == 0 */, const float *d_xs /* may be NULL */, const float *d_xu,
                             const float *d_dz /* may be NULL if every step size is 0 */, const float *step_sizes, uint32_t num_steps,
                             float mu, float qd_cost, float r_cost, const mpcg_xuref *ref, float *d_merit /* [batch][num_steps] */,
                             uint32_t batch, void *stream);
int mpcg_compute_merit_xuref_f64(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size, double timestep,
                                 const double *d_eePos_traj /* may be NULL if ee_cost == 0 */, const double *d_xs /* may be NULL */, const double *d_xu,
                                 const double *d_dz /* may be NULL if every step size is 0 */, const double *step_sizes, uint32_t num_steps,
                                 double mu, double qd_cost, double r_cost, const mpcg_xuref *ref, double *d_merit /* [batch][num_steps] */,
                                 uint32_t batch, void *stream);

/* ---- plant simulation and horizon shift: the step between two SQP solves of the MPC loop (csrc/sim_plant.hip.h) ----
 * What simulateMPC does once per control update (reference include/mpcsim.cuh:288-348), batched, on the device, nothing read back.  Float, state_size
 * 14 / control_size 7 only (MPCG_ERR_UNSUPPORTED otherwise); both calls are pure stream work from the first call on (capturable).
 *
 * mpcg_simulate is simple_simulate (include/common/integrator.cuh:295-325) for the whole batch and all substeps in ONE launch: every trajectory's
 * plant state d_xs[b] is integrated over sim_time_us under the controls of the plan d_xu[b] (the reference passes d_xu_old, the PREVIOUS plan).
 * The schedule is evaluated in IEEE double:  ss = (double)sim_step, toff = time_offset_us * 1e-6, sim = sim_time_us * 1e-6;
 *   S = (uint32)(sim / ss) full substeps of dt = ss; substep s applies u of knot idx_s = (uint32)((toff + s * ss) / timestep);
 *   then one remainder substep of dt = (float)fmod(sim, ss) with the control of the LAST full substep (the reference does not recompute the index
 *   there, :322-324), or of (uint32)(toff / timestep) if S = 0.  A remainder of exactly 0 is not run: sim_time_us = 0 leaves d_xs bitwise unchanged.
 * A substep is explicit Euler from the old values, q += dt qd, qd += dt qdd, qdd = forward dynamics of the mpcg_plant given (its own gravity vector: GRAVITY under mpcg_plant_create) in float64
 * (the arithmetic of mpcg_generate_kkt's integrator defect).  Substeps are gated on their number, never on time accumulated in float.
 * A plant whose limits carry MPCG_LIMITS_SIM_SATURATE (mpcg_plant_clone_limits) clamps every control it applies to [u_lo, u_hi] as it is loaded; a NaN passes.
 * Option "sim_integrator" = 1 (default 0; 0 or 1, anything else MPCG_ERR_INVALID; read when the call is made) makes every substep SEMI-IMPLICIT Euler,
 * qd' = qd + dt qdd, q' = q + dt qd' (integrator.cuh:103-130, INTEGRATOR_TYPE == 1), for mpcg_simulate and mpcg_simulate_f64; the schedule, the clamp and
 * the float64 state carried across substeps are unchanged.  It is an option of its own, apart from "integrator", because the reference's plant simulation
 * is explicit Euler whatever the controller uses (simple_integrator_kernel calls integrator<T, 0, 0>, integrator.cuh:287): the default stays
 * reference-exact, and 1 is for a caller whose plant model is the controller's (one substep of dt = timestep is then mpcg_generate_kkt's x_{k+1} - c_{k+1}
 * under "integrator" = 1).
 * Two deliberate departures from the reference:
 *   - the state is carried in float64 across the substeps of a call and rounded to float ONCE, on store; the reference rounds after every substep
 *     (its T is float).  d_xs and the controls are read as float and widened.
 *   - a control index beyond the last control, idx > knot_points - 2, is clamped to knot_points - 2; the reference reads past its buffer there.
 * d_eePos (may be NULL): [batch][3], the end-effector position of the NEW state, float64 inside, rounded once (what mpcg_advance_horizon takes).
 * Results are bitwise reproducible and a trajectory's do not depend on the rest of the batch (no atomics).
 *   MPCG_ERR_INVALID   a null required pointer; sim_step <= 0, timestep <= 0, a negative time, a non-finite argument; more than
 *                      MPCG_SIM_MAX_SUBSTEPS full substeps (sim / ss >= 65537); batch > max_batch; a plant on another device.  Nothing is written.
 *
 * mpcg_advance_horizon is the rest of the control update (include/mpcsim.cuh:300-348), one workgroup per trajectory, dynamics-free, every source
 * read before it is overwritten.  A trajectory whose d_done[b] is non-zero on entry is FROZEN: nothing of it is written (as MPCG_STEP_FROZEN).
 *   shift = 0:  d_xu[b][0:14] = d_xs[b] (:348) and nothing else; only d_xu and d_xs are required (d_done is honoured if given).
 *   shift = 1, per trajectory, in the reference's order:
 *     d_tracking_error[b] = (|ee0 - goal[0]| + |ee1 - goal[1]|) + |ee2 - goal[2]| in float, in that order, d_eePos[b] against knot 0 of the
 *       UNSHIFTED goals (:303-306);
 *     d_traj_offset[b] += 1 (:310);
 *     just_shift of d_xu (integrator.cuh:258-263: knots 1..N-1 move to 0..N-2, the last moved knot carries no control); its tail u_{N-2}, x_{N-1}:
 *       if traj_offset + N < traj_steps, the 21 plan values at (n+m) * (traj_offset + xu_fill_lead) - m.  With xu_fill_lead = 0 that is :316
 *       literally — a quirk of the reference: its goal fill uses plan row traj_offset + N - 1, its xu fill does not.  A caller who wants the
 *       aligned row passes xu_fill_lead = N - 1.  Otherwise (:320-322) the final plan position, zero velocity, zero last control;
 *     just_shift(6, 0, N) of d_eePos_goal, its last knot from plan row traj_offset + N - 1, or traj_steps - 1 in the else branch (:326-334);
 *     just_shift(14, 0, N) of d_lambda: the last knot of lambda keeps its value (:337-338);
 *     the :348 copy; d_done[b] = 1 when traj_offset reaches traj_steps (:252).
 *   The plan: d_xu_traj traj_steps rows of n + m floats, d_eePos_traj traj_steps rows of 6; traj_batch_stride = 0: one plan shared by the batch,
 *   otherwise trajectory b's plan starts traj_batch_stride rows behind trajectory b-1's (>= traj_steps).  d_traj_offset is device data: a value
 *   that is no row of the plan takes the else branch.
 *   MPCG_ERR_INVALID   shift > 1; a null required pointer (shift = 1: every array, d_eePos included); traj_steps = 0; xu_fill_lead > N - 1;
 *                      0 < traj_batch_stride < traj_steps; batch > max_batch.  Nothing is written. */
#define MPCG_SIM_MAX_SUBSTEPS 65536
int mpcg_simulate(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size,
                  float *d_xs /* [batch][14] in/out */, const float *d_xu /* [batch][(n+m)N - m] */,
                  double timestep, double time_offset_us, double sim_time_us, float sim_step /* reference: 2e-4f */,
                  float *d_eePos /* [batch][3] or NULL */, uint32_t batch, void *stream);
int mpcg_advance_horizon(mpcg_handle *h, uint32_t control_size, uint32_t shift,
                         float *d_xu, float *d_lambda, float *d_eePos_goal /* in/out */,
                         const float *d_xs /* [batch][14] */, const float *d_eePos /* [batch][3]; needed when shift = 1 */,
                         const float *d_xu_traj, const float *d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride,
                         uint32_t xu_fill_lead, int32_t *d_traj_offset, int32_t *d_done /* [batch] in/out */,
                         float *d_tracking_error /* [batch] out */, uint32_t batch, void *stream);
/* The double twins (linsys_t = double, the reference's USE_DOUBLES build): with them a whole control update of the double build stays on the device.
 * Everything said above of mpcg_simulate and mpcg_advance_horizon holds with float replaced by double — layouts, side effects, the frozen
 * semantics of d_done, the error table (messages name the _f64 entry), batch == 0, nothing written on refusal, pure stream work from the first call
 * on (capturable).  What differs:
 *
 * mpcg_simulate_f64.  d_xs and the controls are read as doubles and used as they are: nothing passes through float.  The state is carried in float64
 * across the substeps, as in the float entry, and stored WITHOUT the final rounding; d_eePos likewise.  On float-representable inputs with the same
 * substep schedule, rounding this entry's outputs to float gives mpcg_simulate's bits.  The schedule is the reference's with T = double
 * (include/common/integrator.cuh:301-324), literally:  ss = sim_step, a double that is not passed through float;  S = (uint32)(sim / ss);
 *   idx_s = (uint32)((toff + s * ss) / timestep), one rounding per operation;  the remainder substep is dt = fmod(sim, ss) AS A DOUBLE (not rounded
 *   to float) with the control of the last full substep, or of (uint32)(toff / timestep) if S = 0;  a remainder of exactly 0 is not run.  The clamp
 *   to knot_points - 2 and the cap MPCG_SIM_MAX_SUBSTEPS are the float entry's.
 * A quirk of that arithmetic, reproduced literally (as xu_fill_lead = 0 is): with the reference's double substep 2e-4 and sim_time_us = 2000 the
 * quotient 0.002 / 0.0002 rounds to exactly 10, but ten times the double 0.0002 exceeds the double 0.002, so fmod(0.002, 0.0002) is
 * 0.00019999999999999996 (exact): the reference's double build runs TEN full substeps AND a remainder substep of almost a whole one.  A caller who
 * wants ten substeps passes a substep whose tenfold does not exceed sim, e.g. (double)2e-4f — the value the float entry has always used, with a
 * remainder of 5e-11 s.
 *
 * mpcg_advance_horizon_f64.  The same copies, in doubles; d_tracking_error[b] = (|ee0 - g0| + |ee1 - g1|) + |ee2 - g2| in double, in that order, one
 * rounding per operation. */
int mpcg_simulate_f64(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size,
                      double *d_xs /* [batch][14] in/out */, const double *d_xu /* [batch][(n+m)N - m] */,
                      double timestep, double time_offset_us, double sim_time_us, double sim_step /* reference with T = double: 2e-4 */,
                      double *d_eePos /* [batch][3] or NULL */, uint32_t batch, void *stream);
int mpcg_advance_horizon_f64(mpcg_handle *h, uint32_t control_size, uint32_t shift,
                             double *d_xu, double *d_lambda, double *d_eePos_goal /* in/out */,
                             const double *d_xs /* [batch][14] */, const double *d_eePos /* [batch][3]; needed when shift = 1 */,
                             const double *d_xu_traj, const double *d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride,
                             uint32_t xu_fill_lead, int32_t *d_traj_offset, int32_t *d_done /* [batch] in/out */,
                             double *d_tracking_error /* [batch] out */, uint32_t batch, void *stream);

/* ---- per-trajectory clocks: every trajectory of a batch on its own update schedule (csrc/sim_plant.hip.h) ----
 * The two calls above take ONE time offset, ONE simulated time and ONE shift decision per call: the clock bookkeeping of simulateMPC
 * (prev_simulation_time, time_since_timestep, shifted: include/mpcsim.cuh:280-352) is the caller's, in host scalars, the same for the whole batch.
 * The _clk entries keep it in device arrays, one element per trajectory: trajectories may update at different rates or phases (the reference's own
 * non-CONST_UPDATE_FREQ mode, simulation_time = sqp_solve_time_us, differs per trajectory as soon as iteration counts do), and ONE captured control
 * update follows whatever the arrays hold at each replay.  Float and _f64 twins as above (arrays double, sim_step a double, the remainder not rounded
 * to float); the time and clock arrays are double / int32 in both.  state_size 14 / control_size 7 only (MPCG_ERR_UNSUPPORTED); pure stream work,
 * capturable from the first call: no allocation, no read-back.  batch == 0 returns MPCG_OK.
 *
 * mpcg_simulate_clk.  Trajectory b gets exactly — bit for bit — what mpcg_simulate gives it with time_offset_us = d_time_offset_us[b] and
 * sim_time_us = d_sim_time_us[b]; everything said of mpcg_simulate holds per trajectory: the schedule with its remainder substep under the index of the
 * last full substep, the clamp to knot_points - 2, "a remainder of exactly 0 is not run", the float64 state rounded once on store, "sim_integrator"
 * and MPCG_LIMITS_SIM_SATURATE.  The host's part of the schedule — toff = t * 1e-6, sim = t * 1e-6, S = (uint32)(sim / ss), rem = (double)(T)fmod(sim, ss) —
 * is evaluated on the device in IEEE double, one rounding per operation (fmod is exact).  Four trajectories share a wavefront whose substep loop has
 * barriers: A WAVEFRONT TAKES AS LONG AS ITS LONGEST TRAJECTORY (a call as long as its longest wavefront); a trajectory's results do not depend on its
 * neighbours.
 *   d_done (may be NULL): a trajectory with d_done[b] != 0 on entry is FROZEN: nothing of it is written, neither d_xs nor d_eePos.
 *   A trajectory whose times are no schedule — non-finite or negative, or sim / ss >= 65537 (MPCG_SIM_MAX_SUBSTEPS) — is not simulated: nothing of it is
 *   written except d_done[b] = MPCG_DONE_BAD_CLOCK when d_done is given (without d_done it is skipped silently).  Its neighbours are unaffected.
 *   MPCG_ERR_INVALID   as mpcg_simulate for the arguments that remain (null d_xs / d_xu, sim_step <= 0, timestep <= 0, non-finite, batch > max_batch,
 *                      a plant on another device), and a null time array.  Nothing is written.
 *
 * mpcg_advance_horizon_clk.  mpcg_advance_horizon's arguments without `shift`, the knot spacing, the shift threshold in seconds (the reference's
 * SHIFT_THRESHOLD: (double)(T)(1 * timestep)) and the clock: d_sim_time_us [batch] (in), d_prev_sim_us [batch] (prev_simulation_time, us), d_since_s
 * [batch] (time_since_timestep, s), d_shifted [batch] (int32 0 / 1), in/out, and d_did_shift [batch] (out, may be NULL).  One workgroup per trajectory;
 * for every trajectory with d_done[b] == 0, include/mpcsim.cuh:294-352 literally, in double with one rounding per operation:
 *     since = d_since_s[b] + d_sim_time_us[b] * 1e-6
 *     shift = d_shifted[b] == 0 && since > shift_threshold_s
 *     exactly what mpcg_advance_horizon does to trajectory b with that shift (shift = 0: the start-state copy only, d_tracking_error[b] untouched)
 *     if (shift) shifted = 1
 *     if (since > timestep) { shifted = 0; since = fmod(since, timestep) }
 *     d_since_s[b] = since, d_shifted[b] = shifted, d_prev_sim_us[b] = d_sim_time_us[b], d_did_shift[b] = shift
 *   A FROZEN trajectory (d_done[b] != 0 on entry) keeps everything, its clock included; only d_did_shift[b] = 0 is written.
 *   A non-finite or negative d_sim_time_us[b] on a live trajectory sets d_done[b] = MPCG_DONE_BAD_CLOCK and writes nothing else.
 *   The reference hands prev_simulation_time to simple_simulate as the time offset (:288), not time_since_timestep: a loop passes d_prev_sim_us as
 *   mpcg_simulate_clk's d_time_offset_us —  per update: d_xu_old <- d_xu; mpcg_simulate_clk(d_xs, d_xu_old, d_prev_sim_us, d_sim_time_us);
 *   mpcg_advance_horizon_clk(..., d_sim_time_us, d_prev_sim_us, d_since_s, d_shifted).  A new loop starts from zeros in all three state arrays.
 *   MPCG_ERR_INVALID   a null array other than d_did_shift (any trajectory may shift: every array of mpcg_advance_horizon(shift = 1) is required, d_eePos and
 *                      d_done included); a non-finite or non-positive timestep; a non-finite or negative shift_threshold_s; traj_steps = 0;
 *                      xu_fill_lead > N - 1; 0 < traj_batch_stride < traj_steps; batch > max_batch.  Nothing is written. */
#define MPCG_DONE_BAD_CLOCK 2
int mpcg_simulate_clk(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size,
                      float *d_xs /* [batch][14] in/out */, const float *d_xu /* [batch][(n+m)N - m] */, double timestep,
                      const double *d_time_offset_us /* [batch] */, const double *d_sim_time_us /* [batch] */, float sim_step /* reference: 2e-4f */,
                      float *d_eePos /* [batch][3] or NULL */, int32_t *d_done /* [batch] in/out, or NULL */, uint32_t batch, void *stream);
int mpcg_simulate_clk_f64(mpcg_handle *h, const mpcg_plant *plant, uint32_t control_size,
                          double *d_xs /* [batch][14] in/out */, const double *d_xu /* [batch][(n+m)N - m] */, double timestep,
                          const double *d_time_offset_us /* [batch] */, const double *d_sim_time_us /* [batch] */, double sim_step,
                          double *d_eePos /* [batch][3] or NULL */, int32_t *d_done /* [batch] in/out, or NULL */, uint32_t batch, void *stream);
int mpcg_advance_horizon_clk(mpcg_handle *h, uint32_t control_size,
                             float *d_xu, float *d_lambda, float *d_eePos_goal /* in/out */,
                             const float *d_xs /* [batch][14] */, const float *d_eePos /* [batch][3] */,
                             const float *d_xu_traj, const float *d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride,
                             uint32_t xu_fill_lead, int32_t *d_traj_offset, int32_t *d_done /* [batch] in/out */,
                             float *d_tracking_error /* [batch] out */, double timestep, double shift_threshold_s,
                             const double *d_sim_time_us /* [batch] */, double *d_prev_sim_us, double *d_since_s, int32_t *d_shifted /* [batch] in/out */,
                             int32_t *d_did_shift /* [batch] out, or NULL */, uint32_t batch, void *stream);
int mpcg_advance_horizon_clk_f64(mpcg_handle *h, uint32_t control_size,
                                 double *d_xu, double *d_lambda, double *d_eePos_goal /* in/out */,
                                 const double *d_xs /* [batch][14] */, const double *d_eePos /* [batch][3] */,
                                 const double *d_xu_traj, const double *d_eePos_traj, uint32_t traj_steps, uint32_t traj_batch_stride,
                                 uint32_t xu_fill_lead, int32_t *d_traj_offset, int32_t *d_done /* [batch] in/out */,
                                 double *d_tracking_error /* [batch] out */, double timestep, double shift_threshold_s,
                                 const double *d_sim_time_us /* [batch] */, double *d_prev_sim_us, double *d_since_s, int32_t *d_shifted /* [batch] in/out */,
                                 int32_t *d_did_shift /* [batch] out, or NULL */, uint32_t batch, void *stream);

/* ---- LINSYS_SOLVE == 0 as a selectable solver: the reference's CPU LDL^T path ----
 * The reference's second linear-system path factors the (negated) Schur matrix on the HOST with QDLDL
 * (include/qdldl/sqp.cuh: pattern prep_csr :164 + QDLDL_etree :193 once per SQP call; per SQP iteration D2H(values,
 * gamma), qdldl_solve_schur = QDLDL_factor + QDLDL_solve :22-49, H2D(lambda) :261-282).  QDLDL (osqp/qdldl, float /
 * int32 build, Makefile:16) is an un-vendored submodule of the reference; libmpcg_hip carries its own implementation of
 * the same published algorithm (elimination tree, up-looking LDL^T without pivoting, triangular solves) so that the
 * A/B switch of include/mpcsim.cuh:21-25 exists in-tree.  These entry points are a SOLVER THE CALLER SELECTS, never a
 * fallback: no GPU entry point calls them.  mpcg_ldl_* are pure host code (no device needed).
 *   mpcg_ldl_create        pattern of the lower triangle in CSR (= include/utils/csr.cuh:40-73, identical to what
 *                          mpcg_prep_csr writes on the device) + elimination tree + workspace, for (state_size, knot_points)
 *   mpcg_ldl_pattern       host pointers to col_ptr [nN+1] / row_ind [nnz]; nnz = (N-1)n^2 + N n(n+1)/2 (:148)
 *   mpcg_ldl_solve         qdldl_solve_schur(:22-49): numeric factorisation of h_val [nnz] + solve; h_lambda may alias h_gamma
 *   mpcg_qdldl_solve_schur the reference's timed region (:268-273) on device buffers: D2H(d_val as mpcg_bd_to_csr_lowertri
 *                          / form_schur_system_qdldl left it, d_gamma), factor + solve, H2D(d_lambda); synchronises `stream`. */
typedef struct mpcg_ldl mpcg_ldl;
int mpcg_ldl_create(mpcg_ldl **out, uint32_t state_size, uint32_t knot_points);
int mpcg_ldl_destroy(mpcg_ldl *l);
int mpcg_ldl_pattern(const mpcg_ldl *l, const int32_t **h_col_ptr, const int32_t **h_row_ind, uint32_t *nnz, uint32_t *sum_lnz);
int mpcg_ldl_solve(mpcg_ldl *l, const float *h_val, const float *h_gamma, float *h_lambda);
int mpcg_qdldl_solve_schur(mpcg_handle *h, mpcg_ldl *l, const float *d_val, const float *d_gamma, float *d_lambda, void *stream);

/* Options (tuning / experiments; defaults are chosen by mpcg_create from knot_points and per call from the batch).
 * Kernel selection.  One row per branch of the launch plan (mpcg_pcg.hip: plan_f32, plan_f64; the measurements behind each row are there),
 * tried top to bottom; "auto" = no pcg_* knob set (any pcg_* knob switches the automatic choices off), C = CUs of the device, B = the call's
 * batch, family = "last_kernel_family".
 *   float / fp16 storage (mpcg_pcg_solve, _ref, _f16):
 *     state_size != 14                                                                   generic streaming kernel          3
 *     fp32, N <= 64, "pcg_rpl" != 0, and "pcg_rpl" = 1 or (auto, "cluster" <= 0, "pcg_lpk" != 1, not the half build below, and
 *       N <= 32 or B <= C with the lane-quad kernel not automatic)                         row-per-lane                      5
 *     N <= 128, "pcg_lpk" != 0, and "pcg_lpk" = 1, or auto with "cluster" <= 0 and N > 36 (N > 32 where the lane-quad kernel is
 *       automatic), or the half build: fp32, 16 < N <= 32, 2 B >= 5 C, auto, "pcg_rpl" != 1 — the lane-pair kernel      lane-pair         6
 *       ... in its place, fp32, "pcg_lqb" = 1, or "pcg_lqb", "pcg_lpk", "pcg_rpl" all -1, auto, "cluster" <= 0        lane-quad         11
 *     "cluster" = G, or auto with "cluster" = -1 and N > 128 (G = ceil(N / 128)); 2 <= G <= 8, G <= C, <= 128 knots per member
 *                                                                                        clustered lane-pair               7
 *     otherwise                                                                          row-pair (single workgroup)       0
 *   the calls above with family 6, 7 or 11 read only the lower block triangle; while the handle does not know the caller's matrices to be
 *   block-symmetric they run guarded, and once it knows they are not (BLOCK SYMMETRY):
 *     fp32, N <= 64, "pcg_rpl" != 0                                                      row-per-lane                      5
 *     otherwise                                                                          row-pair                          0
 *   double (mpcg_pcg_solve_f64, _ref_f64):
 *     N <= 64, "pcg_lqk" != 0, block-symmetric (the latch), and "pcg_lqk" = 1 or auto with "cluster" = -1 and N > 32 (or 16 < N and
 *       B >= 4 C)                                                                          lane-quad (one CU)                9
 *     N <= 32, "pcg_rpl" != 0, and "pcg_rpl" = 1 or auto                                 row-per-lane                      5
 *     state_size != 14                                                                   generic streaming kernel          3
 *     N > 32, "cluster" != 0, "pcg_lqk" != 0, block-symmetric, G = "cluster" or ceil(N / 64): 2 <= G <= 8, <= 64 knots per member
 *                                                                                        clustered lane-quad               10
 *     "cluster" != 0, G = "cluster" or ceil(N / 32): 2 <= G <= 8, <= 32 knots per member  clustered row-per-lane            8
 *     otherwise (the iterate vectors in LDS: N <= 350; two block columns once the latch says block-symmetric)
 *                                                                                        streaming                         3
 *   Clustered kernels: G CUs of one XCD per trajectory; members exchange inner-product partials and boundary knots through the XCD's L2
 *   ("cluster_l2" = 0: always write-through), so all members of a cluster must be resident: the launch holds as many clusters as fit the chip
 *   and each draws trajectories from a queue (any batch = one launch).  A cluster that cannot make progress (a peer not resident: another
 *   stream holds its CU) gives up after a bounded spin and a follow-up launch re-solves its trajectory — the lane-pair / lane-quad kernel up
 *   to 128 knots, else the row-pair kernel (double: the streaming kernel) — warm-started from the handle's own copy of d_lambda made in front
 *   of the cluster launch ("cluster_fixup" = 0, or a horizon the follow-up kernel cannot hold: no follow-up launch, d_iters = 0xFFFFFFFF and
 *   d_max_iter_exit = 2 for such a trajectory; "cluster_test_fail" = 1, tests only: one member gives up at its first write-back).
 *   Knobs of these rows: "rpl_waves" (row-per-lane wavefronts per trajectory: 0 auto, 4, 8, 16); the row-pair kernel's "pcg_waves" (4, 8 or
 *   16 wavefronts per trajectory workgroup), "pcg_reg_rows" (TRIPLES of block rows per matrix and wave kept in registers for the whole
 *   solve; only compiled (waves, rows) pairs are accepted at launch), "pcg_lds_rows" (triples per matrix and wave cached in LDS, -1 =
 *   what fits), "pcg_stream_bufs", "pcg_max_wg_per_cu", "lds_extra" (single-triple LDS slots beyond the uniform cache of the <.,.,1>
 *   kernels: -1 what fits, 0 none); "pcg16_*" = the same for fp16 storage.
 *   The family depends on knot_points AND on the call's batch.  Families sum the inner products in different orders, so the SAME trajectory
 *   solved alone and inside a large batch may differ in the last fp32 bits (and, near the tolerance, by an iteration); within one family
 *   results are bitwise reproducible run to run and independent of batch composition.  Pin a family with "pcg_rpl" / "pcg_lpk" / "pcg_lqb" /
 *   "rpl_waves" when bit-stability across batch sizes matters.  None of the residency knobs changes results within a lane-order family
 *   (bitwise identical, tested).
 * "sched_hint" (0 / 1, default 1): an mpcg_pcg_solve call with more trajectories than CUs that runs a register-resident kernel dispatches its
 *       trajectories longest-expected-first, the expectation being the iteration counts the handle's previous call with the same batch size
 *       wrote to d_iters — warm-started solves leave the loop at very different iterations and the dispatch order decides how well the chip stays
 *       filled: -25..35 % on such batches; a scheduling hint only, no result depends on it; one extra ~3 us kernel behind each such solve.
 * "check_symmetry" (debug, 0/1: see BLOCK SYMMETRY above).
 * Around the solve: "schur_dpp" (1: mpcg_form_schur's register-resident formation — a 16-lane DPP row walks a chunk of consecutive block rows, a second
 *       kernel closes the seams between chunks; 0: the LDS kernels, one workgroup per block row; same bits), "schur_chunk" (block rows per
 *       chunk: 0 = by call size, from one row per chunk for a single trajectory to 16 at 1024 x 128 knots; 1..2048 forced; same bits), "dz_dpp"
 *       (1: mpcg_compute_dz with four knots per wavefront, 0: the LDS kernel, one lane per element of dz; same bits), "block_solve_wide"
 *       (mpcg_block_solve: 1 one trajectory per wavefront, 0 four, -1 by batch size; same bits; not read by the double sweeps), "block_solve_f64"
 *       (mpcg_block_solve: 0, the default: the float sweep; 1: float64 inside, lambda rounded to float on store — see mpcg_block_solve; any other
 *       value is MPCG_ERR_INVALID), "producers_generic" (0 / 1, default 0; 1: on a
 *       14 x 7 handle mpcg_form_schur(_f64), mpcg_compute_dz(_f64) and mpcg_block_solve(_f64) run the run-time-dimension kernels every other shape
 *       gets — same bits, the A/B switch of tests and timings; "last_schur_chunk" then reads 0).  The library has ONE set of LDS kernels, the
 *       run-time-dimension ones: for formation and dz, "producers_generic" = 1 and "schur_dpp" = "dz_dpp" = 0 run the same kernels (the two
 *       differ in mpcg_block_solve only, which "schur_dpp" / "dz_dpp" leave register-resident); a 14 x 7 call too large for the 31-bit byte
 *       offsets of the register-resident kernels (from 913 k knots in float, 456 k in double) runs them as well.  "kkt_analytic" (mpcg_generate_kkt: 1 = the analytic gradient recursion of the inverse dynamics, the default;
 *       0 = one-sided float64 differences, the checker), "kkt_f32" (round 6; 1 = the analytic kernel with every recursion in float — linsys_t's own
 *       arithmetic, as the reference's GRiD<float> — and TWO knots per lane in packed float: outputs within 5e-6 of the float64 restatement (relative to max(1, |block|); worst of 1024 windows: 4e-6) instead of
 *       2e-7, 1.6x faster than the default on throughput-sized calls (0.204 against 0.330 ms per 1024 x 127 knots; a single trajectory: 20 against 16 us —
 *       the default is the one for latency-sized calls), a trajectory's results independent of the rest of the batch; 2 = the same arithmetic with one
 *       knot per lane (8 % faster than the default; differs from 1 by float rounding); 0, the default: float64 inside, results rounded to float on
 *       the way out), "merit_f32" (mpcg_compute_merit: 0, the default: float64 inside; 1: the point merits in packed float, two work items per
 *       16-lane group — see mpcg_compute_merit; any other value is MPCG_ERR_INVALID; independent of "kkt_f32"), "integrator" (mpcg_generate_kkt(_f64) and
 *       mpcg_compute_merit(_f64), every build: 0, the default: explicit Euler; 1: semi-implicit Euler, q' = q + dt qd' — see THE INTEGRATOR under mpcg_plant_create;
 *       any other value is MPCG_ERR_INVALID and leaves the value; read when the call is made; orthogonal to "kkt_analytic", "kkt_f32" and "merit_f32"),
 *       "sim_integrator" (mpcg_simulate(_f64): the same choice for the plant's substeps, 0 the default and the reference's — see mpcg_simulate;
 *       independent of "integrator"), "nt_loads" / "spmv_blocks_per_cu" (mpcg_bt_spmv), "spmv_mfma" (the MFMA experiment kernel).
 * "assume_symmetric" (0 / 1), "symmetry_state" (read-only; 0 unknown, 1 block-symmetric, 2 violated): see BLOCK SYMMETRY above.
 * "reserve_f64" (= 1: allocate the double cluster kernels' buffers now; see GRAPH CAPTURE above).
 * Read-only: "cluster_fixups" (trajectories re-solved by fix-up launches since mpcg_create — each costs 1.5-4.5 ms of spinning; blocking 8-byte
 *       D2H read), "last_symmetry_violations", "num_cus", "pcg_resident" (1 if the single-workgroup configuration streams nothing inside the PCG
 *       loop), "last_schur_chunk" (block rows per chunk of the last mpcg_form_schur, 0 = the LDS kernels), "last_dz_route" (the last
 *       mpcg_compute_dz(_f64): 1 = four knots per wavefront, 0 = the LDS kernel), "last_kernel_family" (kernel of the
 *       last solve: 0 single-workgroup row-pair, 3 generic, 5 row-per-lane, 6 lane-pair-per-knot, 7 clustered lane-pair, 8 clustered row-per-lane
 *       (double), 9 lane-quad-per-knot (double), 10 clustered lane-quad (double), 11 lane-quad-per-knot with both matrices per wavefront (float, round 6); 1, 2, 4 were kernels retired in round 4), "last_kernel_{waves,reg_rows,lds_rows,lds_extra,stream_bufs,cluster,lds_bytes}". */
int mpcg_set_option(mpcg_handle *h, const char *key, int value);
int mpcg_get_option(const mpcg_handle *h, const char *key, int *value);

#ifdef __cplusplus
}
#endif
#endif /* MPCG_H */
