/* mghip_ho.h -- the fourth-order compact nine-point ("Mehrstellen") discretisation of libmghip.so for the Krylov outer loop
 * of include/mghip.h.  Same conventions as mghip.h: C ABI, status codes, pitches in elements.  No reference counterpart: the
 * reference discretises with the five-point stencil only.
 *
 * For A = coeff (Laplacian_h - sigma), coeff < 0, constant coefficients, the scheme solves A4 u = R f on interior cells with
 *   R f  = (8 f_C + f_(i+1,j) + f_(i-1,j) + f_(i,j+1) + f_(i,j-1)) / 12              (reads f on the ring, never its corners)
 *   A4 u = -coeff [cC u_C + cE (u_(i+1,j) + u_(i-1,j)) + cN (u_(i,j+1) + u_(i,j-1)) - cK (the four corners)]
 *   ca = 1/hx^2, cb = 1/hy^2,  cC = (5/3)(ca+cb) + sigma 8/12,  cE = (cb - 5 ca)/6 + sigma/12,  cN = (ca - 5 cb)/6 + sigma/12,
 *   cK = (ca+cb)/12
 * (hx = hy: the classical 20 / -4 / -1 over 6 h^2).  Its truncation error is O(h^4) where the five-point stencil has O(h^2).
 * The Dirichlet data is the ring of the iterate; A4 also reads the ring's corners.  A4 is symmetric positive definite and
 * its symbol lies in [1/3, 1] times that of the five-point operator ([2/3, 1] for sigma = 0), so the five-point multigrid
 * cycle preconditions it unchanged.
 *
 * The rounding sequence is fixed: the four c's are computed once on the host in double, in the forms
 *   (5.0/3.0)*(ca+cb) + sigma*(8.0/12.0),  (cb - 5.0*ca)/6.0 + sigma/12.0,  (ca - 5.0*cb)/6.0 + sigma/12.0,  (ca+cb)/12.0
 * with ca = 1.0/(hx*hx), and per cell (dn / up: rows i+1 / i-1, ea / w: columns j+1 / j-1, C the centre)
 *   A4:  (-coeff) * (((cC*C + cE*(dn+up)) + cN*(ea+w)) - cK*((dn_e+dn_w)+(up_e+up_w)))
 *   R:   (8.0*f + ((dn+up) + (ea+w))) / 12.0
 * without FMA contraction.  All sums are per-workgroup partials and a fixed-order pass: the same bits on every run. */
#ifndef MGHIP_HO_H
#define MGHIP_HO_H

#include "mghip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The discretisation the outer loop of an mg_pcg iterates on: 2 (default) the five-point operator, bit for bit the loop
 * without this call; 4 the compact scheme.  Any other order: MG_ERR_INVALID_VALUE.  Order 4 needs constant coefficients: with a
 * coefficient field set it returns MG_ERR_STATE, and so does mg_pcg_set_coefficient(non-NULL) under order 4; either way the
 * solver is left as it was.  Under order 4 mg_pcg_solve / mg_pcg_solve_device form g = R f once per solve (one more field,
 * allocated when order 4 is first set), take the initial residual g - A4 x, q = A4 p and the true residual with the kernels
 * below, and leave the preconditioner -- the five-point cycle --, look-ahead, the flexible beta, mg_pcg_set_shift (which
 * reaches A4 and the engine), breakdown handling and mg_pcg_stats as they are.  The rhs is read on its ring (not at its
 * corners); the reported norms are sqrt(hx hy (sum of (R f - A4 x)^2 over interior cells)): the ring of the rhs, which is
 * data of the scheme here, does not enter them. */
int mg_pcg_set_order(mg_pcg* s, int order);

/* The field kernels, call by call: fp64 device arrays (nx, ny) with pitch `ld` (elements, even), 16-byte aligned;
 * asynchronous on `stream` (nullable); scratch >= mg_dev_scratch_bytes(); results are doubles in device memory.  Every kernel
 * stores exactly the cells [0, nx) x [0, ny) of its outputs; outputs are arrays of their own.
 *   direction: p_out = z + beta p_in (beta NULL: p_out = z, p_in is not read), q = A4 p_out, *pq_dev = p_out . q; 0 on the
 *              rings of p_out and q (the rings of z and p_in are not read).  The contract of mg_dev_pcg_direction.
 *   residual:  r = g - A4 x on interior cells, where x carries the Dirichlet ring (corners included); 0 on the ring of r;
 *              *rr_dev = the sum of r^2.
 *   rhs:       g = R f on interior cells; the ring of g is the ring of f. */
int mg_dev_ho_direction(int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, const double* z,
                        const double* p_in_or_null, double* p_out, double* q, const double* beta_dev_or_null, void* scratch,
                        double* pq_dev, void* stream);
int mg_dev_ho_residual(int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, const double* x, const double* g,
                       double* r, void* scratch, double* rr_dev, void* stream);
int mg_dev_ho_rhs(int nx, int ny, int ld, const double* f, double* g, void* stream);
/* host arrays (nx, ny), fp64: out = A4 u on interior cells and 0 on the ring (the ring of u is read); g = R f as above */
int mg_op_apply_ho(int nx, int ny, double hx, double hy, double coeff, double sigma, const double* u, double* out);
int mg_op_rhs_ho(int nx, int ny, const double* f, double* g);

#ifdef __cplusplus
}
#endif
#endif /* MGHIP_HO_H */
