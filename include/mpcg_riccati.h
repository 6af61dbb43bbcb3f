/* mpcg_riccati.h — C ABI of libmpcg_hip.so, second table: the feedback gains of the subproblem the two linear solvers solve.
 *
 * An MPC update hands three things per knot to the loop below it: the nominal (x_k, u_k) and the time-varying LQR gain
 * K_k = du_k/dx_k, so that the low-level loop runs  u = u_k + K_k (x - x_k)  between two updates.  Neither mpcg_pcg_solve nor
 * mpcg_block_solve can give K_k: both eliminate the primal variables and return multipliers, and the QP pins x_0.  A backward Riccati
 * sweep over the KKT blocks gives every K_k for about three times the flops of one mpcg_block_solve, with no Schur matrix and no
 * handle-owned scratch.  The conventions of mpcg.h hold (device pointers, streams, alignment and extents, non-finite data, return codes,
 * mpcg_last_error); MPCG_ABI_VERSION is unchanged.
 *
 * CALL IT BEFORE mpcg_form_schur.  The blocks are read from d_G_dense AS mpcg_generate_kkt LEFT THEM; mpcg_form_schur(_rhov)(_f64)
 * OVERWRITES d_G_dense WITH THE BLOCK INVERSES, and gains computed from those are garbage that no check can detect.
 *
 * The recursion (n = state_size of the handle, m = control_size, N = knot_points), per trajectory:
 *   Q_k (k = 0..N-1), R_k (k = 0..N-2)   column-major blocks of d_G_dense, slot k at k (n^2 + m^2), R_k behind Q_k (per trajectory
 *                                         (n^2 + m^2) N - m^2 elements)
 *   A_k = -C[k][0 : n^2], B_k = -C[k][n^2 : n^2 + n m]     d_C_dense stores -A_k, -B_k, slot k at k (n^2 + n m) (per trajectory
 *                                         (n^2 + n m)(N - 1) elements)
 *   rho                                   the regularisation mpcg_form_schur adds to every diagonal entry of every Q_k and R_k
 *
 *   P_{N-1} = Q_{N-1} + rho I
 *   for k = N-2 .. 0:
 *       H_uu = R_k + rho I + B_k^T P_{k+1} B_k        (m x m, symmetric positive definite for rho > 0)
 *       H_ux = B_k^T P_{k+1} A_k                      (m x n)
 *       K_k  = -H_uu^-1 H_ux                          (m x n)
 *       P_k  = Q_k + rho I + A_k^T P_{k+1} A_k + H_ux^T K_k      (stored exactly symmetric: the lower triangle, mirrored)
 *
 * K_k is du_k/dx_k of the regularised LQ subproblem; it does not depend on the sign convention of dz.
 * d_K: [batch][N-1][m n], each block column-major m x n with leading dimension m, like every other dense block of the path.
 *
 *   - RHO.  d_rho != NULL: trajectory b uses d_rho[b], read when the kernel runs — the vector mpcg_line_search_step_rho updates, so a captured
 *     graph follows it; the vector is device data and is not validated.  A trajectory's output is bit for bit that of the scalar call with
 *     rho = d_rho[b].  d_rho == NULL: the scalar `rho`, which must be finite and >= 0.
 *   - ARITHMETIC.  Float64 inside for both entries, as in the plant kernels: the float entry widens on load (exact) and rounds K once, on
 *     store.  H_uu is eliminated without pivoting (the Gauss-Jordan scheme of the path); the order of the sums is not part of the contract.
 *   - STREAM AND CAPTURE.  Pure stream work from the first call on, capturable: no handle-owned buffer (P never leaves the compute unit), no
 *     atomics, no option.
 *   - EXTENTS.  d_G_dense and d_C_dense are not written; d_K is written in full ((N - 1) m n elements per trajectory) and nothing else is.
 *     Element alignment only; 64-bit offsets.
 *   - TRAJECTORIES ARE INDEPENDENT: a wavefront and an LDS region each.  A trajectory's result depends neither on its position in the batch
 *     nor on its neighbours' data; one with NaN, Inf or all-zero blocks (a singular H_uu at rho = 0) leaves every other trajectory's K bit
 *     for bit unchanged, and the call still returns: every loop bound is a host argument.
 *   - RETURN CODES.  MPCG_ERR_INVALID, nothing launched or written: a NULL handle or a NULL d_G_dense, d_C_dense or d_K; control_size 0 or
 *     greater than state_size; batch > max_batch; a non-finite or negative `rho` with d_rho == NULL.  batch == 0: MPCG_OK, nothing
 *     launched.  knot_points == 1: MPCG_OK, nothing written (there are no controls).  MPCG_ERR_UNSUPPORTED: a shape whose LDS need
 *         8 (LD^2 + 2 LD (n + m) + LM (m + 2 n)) bytes,   LD = n rounded up to a multiple of 4, LM = m rounded up likewise
 *     exceeds 160 KiB (9,664 bytes at 14 x 7, 65,536 at 32 x 32: every m <= n <= 32 is served; n = 64 up to m = 28).  The message names the
 *     entry, _f64 included.  (A NULL handle leaves its message where a failed mpcg_create does: mpcg_last_error(NULL).)
 *   - KERNELS.  (14, 7) runs a build with the dimensions at compile time; every other shape of a handle — another state size, or another
 *     control_size on a 14-state handle — the same body with run-time dimensions. */
#ifndef MPCG_RICCATI_H
#define MPCG_RICCATI_H

#include "mpcg.h"

#ifdef __cplusplus
extern "C" {
#endif

int mpcg_riccati_gains(mpcg_handle *h, uint32_t control_size, const float *d_G_dense, const float *d_C_dense,
                       float rho, const float *d_rho /* [batch] or NULL */, float *d_K, uint32_t batch, void *stream);
int mpcg_riccati_gains_f64(mpcg_handle *h, uint32_t control_size, const double *d_G_dense, const double *d_C_dense,
                           double rho, const double *d_rho /* [batch] or NULL */, double *d_K, uint32_t batch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCG_RICCATI_H */
