/* grf_dense_solve.h -- dense exact GP regression: an fp64 Cholesky factorisation and triangular solves on the
 * device.  An additive companion of grf.h (same library, same status codes, GRF_ABI_VERSION unchanged): grf.h
 * keeps naming exactly what it named before.
 *
 * Serves the reference's dense model: experiments/sparse/scaling_exp/run_scaling_experiment.py:687-730
 * (DenseGPModel: gpflow.models.GPR(data, kernel, noise_variance), -log_marginal_likelihood(), predict_f) and the
 * Cora, traffic and mesh-ablation notebooks, which put the kernels of efficient_graph_gp/gpflow_kernels into the
 * same gpflow.models.GPR.  GPflow's GPR is a Cholesky of K + sigma^2 I and triangular solves; these are they.
 *
 * Layout.  Every matrix is row-major fp64 with a leading dimension.  A set of right-hand sides is stored one
 * right-hand side per ROW: nrhs x n at pitch ldb.  With that layout every block update is an A B^T product
 * (grf_gemm_nt_f64) and the panel of the factorisation is itself a set of right-hand sides.
 *
 * The factor F (n x n, ldf >= n) holds L in its lower triangle and L^T mirrored into the upper:
 *     F[i, j] = F[j, i] = L[max(i, j), min(i, j)],
 * so the rows of L^T's blocks are contiguous for the backward solve.  The block edge is GRF_DENSE_SOLVE_NB.
 *
 * Order rule (both entries; fp64 throughout, two calls give the same bits).  Every entry of L and of a solution
 * is produced by the substitution recurrence
 *     L[i, j] = (A[i, j] - sum_{k < j} L[i, k] L[j, k]) / L[j, j],   L[j, j] = sqrt(A[j, j] - sum_{k < j} L[j, k]^2),
 *     x[i]    = (b[i]    - sum_{k < i} L[i, k] x[k])    / L[i, i]    (L^T: k > i, L[k, i]),
 * where the sum is cut at the block edges: the part of the sum that belongs to an earlier block step is one
 * grf_gemm_nt_f64 accumulator chain (ascending k; inside an MFMA the instruction's own order) subtracted from the
 * entry by that step's update (alpha = -1, gamma = 1, Z aliasing C), the block steps in their order; the part
 * inside the entry's own block is one chain in ascending k of RN(RN(l * x) + s) (no contraction), then ONE
 * subtraction and ONE division by the pivot (or one square root).  No explicit inverse of a diagonal block, no
 * split-k, no floating-point atomics.  Hence the classical bounds hold as theorems (Higham, Accuracy and
 * Stability of Numerical Algorithms, 2nd ed., Thm 10.3 and Thm 8.5, which hold for any order of summation):
 *     |A - L L^T| <= gamma_{n+1} |L| |L^T|,    |b - T x| <= gamma_n |T| |x|,    gamma_k = k u / (1 - k u), u = 2^-53.
 */
#ifndef GRF_DENSE_SOLVE_H
#define GRF_DENSE_SOLVE_H

#include "grf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GRF_DENSE_SOLVE_NB 128

/* grf_potrf_f64: the lower Cholesky factor of a symmetric positive-definite A (n x n, lda >= n).  Only the lower
 * triangle and the diagonal of A are read; A is not modified.  Blocked right-looking: per block step, potf2 (one
 * workgroup, the nb x nb diagonal block in LDS, the column recurrence), the panel below it by trsm_block (each
 * panel row a solves L11 x = a), and the trailing update W22 <- W22 - L21 L21^T by grf_gemm_nt_f64 in its
 * symmetric mode on a workspace copy W of A (L21 is read from F).
 *   F       n x n, ldf >= n: L below, L^T mirrored above (see Layout); columns [n, ldf) are never written.
 *   logdet  one device double: 2 sum_i log L[i, i], the terms RN(2 log L[i, i]) added in ascending i.
 *   info    one device int32: 0, or the 1-based index of the first pivot that is not a positive finite number.
 *           Then logdet is NaN and the rest of F is unspecified; the call still returns GRF_OK, reads nothing
 *           out of bounds and does not spin (no control flow depends on the data).
 * No host read of device data.  n == 0 is GRF_EINVAL (logdet and info could not be written); n >= 2^31 is
 * GRF_EUNSUPPORTED, and so is an n whose copy pass would exceed one launch (2^32 work-items: one 256-thread
 * workgroup per 32 x 32 tile of the lower triangle, n > 185 000; no device holds such a matrix).  A leading
 * dimension so large that the matrix's byte span does not fit the address space is GRF_EINVAL.  A, F, the
 * workspace, logdet and info must not overlap.  Workspace: grf_potrf_f64_workspace_bytes(n) (the copy W, rows
 * padded to an even length). */
size_t grf_potrf_f64_workspace_bytes(int64_t n);
int32_t grf_potrf_f64(int64_t n, const double *A, int64_t lda, double *F, int64_t ldf, double *logdet,
                      int32_t *info, void *workspace, size_t workspace_bytes, grf_stream_t stream);

/* grf_trsm_f64: solves L x = b (transposed == 0) or L^T x = b (transposed != 0) in place for every row b of B
 * (nrhs x n, ldb >= n), with the factor F of grf_potrf_f64.  Blocks go ascending for L and descending for L^T; per
 * block step, trsm_block (the nb x nb diagonal block in LDS, one lane per right-hand side, forward or backward
 * substitution in order, every LDS read of the block a broadcast), then one grf_gemm_nt_f64 update of the
 * remaining columns from a copy of the block's solutions in the workspace.  Columns [n, ldb) of B are never
 * written.  n == 0 or nrhs == 0 touches nothing and returns GRF_OK; n or nrhs >= 2^31 is GRF_EUNSUPPORTED; a
 * leading dimension whose byte span does not fit the address space is GRF_EINVAL.  F, B and the workspace must not
 * overlap.  Workspace: grf_trsm_f64_workspace_bytes(n, nrhs) (nrhs x nb doubles). */
size_t grf_trsm_f64_workspace_bytes(int64_t n, int64_t nrhs);
int32_t grf_trsm_f64(int64_t n, int64_t nrhs, const double *F, int64_t ldf, int32_t transposed, double *B,
                     int64_t ldb, void *workspace, size_t workspace_bytes, grf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GRF_DENSE_SOLVE_H */
