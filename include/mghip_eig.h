/* mghip_eig.h -- the block eigensolver of libmghip.so: the lowest eigenpairs of A = coeff * Laplace_h or coeff * div(a grad .)
 * (coeff < 0, homogeneous Dirichlet ring) by LOBPCG with the multigrid cycle as preconditioner.  Same conventions as mghip.h:
 * C ABI, status codes, pitches in elements.  No reference counterpart.
 *
 * Inner product <u, v> = sum over interior cells (unweighted); every block vector has a zero ring.  With block size m:
 *   start   X = the caller's m vectors with the ring zeroed, Cholesky-orthonormalised; AX = A X; Rayleigh-Ritz on X^T A X.
 *   1       R_i = AX_i - lambda_i X_i, rel_i = ||R_i||_2 / lambda_i; hist[it] = max over i < nev; stop when it is < tol.
 *   2       W_i = num_cycles cycles from zero on the right-hand side R_i, every column (no locking).
 *   3       W = W - X (X^T W), Cholesky-orthonormalised (its Gram matrix is W^T W - (X^T W)^T (X^T W)); AW = A W.
 *   4, 5    G_B = S^T S and G_A = S^T A S for S = [X W P], symmetrised; P is Cholesky-orthonormalised through the Gram
 *           matrices (a change of basis on the host); Cholesky G_B = L L^T, eigh(L^-1 G_A L^-T), the lowest m pairs.
 *   6       P = [W P] C[m:], AP = [AW AP] C[m:], X = X C[:m] + P, AX = AX C[:m] + AP.
 * A failed Cholesky (non-positive or non-finite pivot) of P's block or of G_B drops P for that iteration (restarts += 1);
 * a failure in step 3, without P, or two restarts in a row end the solve with status 2 and the last X.
 * The host waits for the stream three times per iteration: for the norms of step 1, the Gram matrix of step 3 and the Gram
 * matrix of step 5.  What it sends (eigenvalues, coefficients) goes through pinned memory without a wait.
 *
 * A block is a run of columns `col_stride` elements apart, each an (nx, ld) fp64 array with 16-byte aligned rows (ld even).
 * The solver keeps two blocks of 6 m columns in the order [P X W AP AX AW] (S and A S adjacent, and so are the [P X] and
 * [AP AX] that step 6 writes) and alternates between them. */
#ifndef MGHIP_EIG_H
#define MGHIP_EIG_H

#include "mghip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_eig mg_eig;

typedef struct mg_eig_stats {
  double solve_seconds, precond_seconds;
  int32_t iterations, restarts, status;        /* status: 0 tolerance met, 1 max_iter, 2 breakdown */
} mg_eig_stats;

/* cfg as for mg_pcg_create (precision MG_PREC_DOUBLE, MG_PREC_SINGLE_MANAGED or MG_PREC_MIXED_LEVELS, fmg_cycles 0,
 * coeff < 0); 1 <= block_size <= 16, num_cycles >= 1.  Anything else: MG_ERR_INVALID_VALUE before any device work. */
int mg_eig_create(const mg_config* cfg, int block_size, int num_cycles, mg_eig** out);
int mg_eig_destroy(mg_eig* s);
const char* mg_eig_last_error(const mg_eig* s);
/* A = coeff * div(a grad .) for the block stencil and the preconditioner (NULL: constant coefficients) */
int mg_eig_set_coefficient(mg_eig* s, const void* a_host_or_null, int host_dtype);
/* x0_host: (block_size, nx, ny) start vectors of host_dtype; vectors_out: (nev, nx, ny) of host_dtype, scaled to
 * hx hy sum v^2 = 1; eigenvalues and residuals: block_size doubles; hist: hist_cap doubles (max_iter + 1 are written at
 * most); n_iter: completed iterations.  Start vectors that are linearly dependent on the interior cells, or that hold a NaN
 * or an Inf there (the Gram matrix of the block then has a non-finite row and cannot be factored), return
 * MG_ERR_INVALID_VALUE before the first iteration; the solver stays usable. */
int mg_eig_solve(mg_eig* s, int nev, const void* x0_host, int host_dtype, double tol, int max_iter, double* eigenvalues,
                 void* vectors_out, double* residuals, double* hist, int hist_cap, int* n_iter, int* converged,
                 mg_eig_stats* stats);
/* Step 5 on host arrays (n x n row-major, n <= 48, 1 <= m <= n): evals[m], coef[n x m] with coef^T G_B coef = I.
 * MG_OK, or 1 when G_B is not positive definite.  No device. */
int mg_eig_host_ritz(int n, int m, const double* ga, const double* gb, double* evals, double* coef);

/* Stateless device entry points on fp64 arrays: asynchronous on `stream` (nullable), scratch >= mg_dev_scratch_bytes(nx, ny),
 * the same bits on every run. */
/* av_c = A v_c on interior cells, 0 on the ring, for ncols columns in one launch (per cell: mg_dev_pcg_direction's q) */
int mg_dev_eig_apply(int nx, int ny, int ld, int ncols, int64_t col_stride, double hx, double hy, double coeff,
                     const double* a_or_null, const double* v, double* av, void* stream);
/* g[a * q + b] = sum over interior cells of u_a v_b, p <= 48, q <= 96.  Ring and pad columns are masked.  Where u and v lie in
 * one run of columns (v - u a multiple of col_stride, at most 144 columns in all) every column is read once.
 * Cost: a workgroup needs ceil16(p) x ceil16(q) doubles of scratch for its partial sums, and only as many workgroups run as
 * fit in mg_dev_scratch_bytes(nx, ny) (2048 doubles on grids up to about 1000 x 1000).  So for p > 16 or q > 48 on such grids
 * this call runs as ONE workgroup whatever the grid size: right, the same bits on every run, but its time grows with the grid
 * as a single CU's would.  It is the form for tests and small blocks; mg_eig_solve gives the kernel a scratch of its own
 * (1024 workgroups). */
int mg_dev_eig_gram(int nx, int ny, int ld, int64_t col_stride, int p, const double* u, int q, const double* v, void* scratch,
                    double* g_dev, void* stream);
/* out_b = sum_a coef[a][b] in_a (a < p <= 48, b < q <= 96; more than 48 outputs take a second pass over the inputs) on rows
 * 0 .. nx - 1, whole 16-byte vectors; coef_dev is p x q row-major on the device; out does not overlap in */
int mg_dev_eig_combine(int nx, int ny, int ld, int64_t col_stride, int p, const double* in, int q, const double* coef_dev,
                       double* out, void* stream);
/* r_c = ax_c - lambda_c x_c on interior cells (0 elsewhere), sumsq_dev[c] = sum r_c^2, c < ncols <= 16 */
int mg_dev_eig_residual(int nx, int ny, int ld, int ncols, int64_t col_stride, const double* x, const double* ax,
                        const double* lambda_dev, double* r, void* scratch, double* sumsq_dev, void* stream);
/* hipEvent-timed repetitions on the solver's own blocks: op 0 apply (m columns), 1 gram (3m x 6m), 2 combine (3m -> 2m),
 * 3 one preconditioner application */
int mg_eig_time_op(mg_eig* s, int op, int reps, double* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* MGHIP_EIG_H */
