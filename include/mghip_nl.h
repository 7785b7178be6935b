/* mghip_nl.h -- semilinear elliptic problems on the device: an inexact Newton method around the Krylov outer loop of
 * include/mghip.h (Newton - conjugate gradients - multigrid).  Same conventions as mghip.h: C ABI, status codes, pitches in
 * elements.  No reference counterpart: the reference has linear solvers only.
 *
 * Solve  N(u) = A u + g(u; x) = f  on interior cells, with the Dirichlet data on the ring of the initial iterate, where
 *   A = coeff (Laplacian_h - sigma)  or  coeff (div(a grad .) - sigma),  coeff < 0          (exactly mg_pcg's operator)
 *   g(u; x) = kappa w(x, y) phi(u),  kappa >= 0,  w >= 0 an optional weight field (NULL: w == 1)
 * and phi is one of the four kinds of mg_nl_kind.  All four are monotone (phi' >= 0), so the Jacobian
 *   J(u) = A + diag(c),  c = kappa w phi'(u) >= 0
 * is symmetric positive definite and conjugate gradients apply.  Non-monotone terms (Bratu's -lambda e^u) are out of scope
 * and REFUSED: kappa < 0, a non-finite kappa, or any non-finite or negative entry of w returns MG_ERR_INVALID_VALUE; the
 * check runs on the host array before any device work (mg_nl_set_nonlinearity, mg_op_nl_eval; mg_dev_nl_eval, whose w is a
 * device array, checks kappa only).
 *
 * The norm is ||F||_h = sqrt(hx hy (sum over interior cells of F^2)) with F = f - N(u); the ring of F is zero and the ring
 * of f is never read.
 *
 * The rounding sequence per interior cell is fixed (no FMA contraction):
 *   v  = u + t*delta                                   (delta NULL: v = u; on the ring v = u)
 *   r0 = f - A v                                       with the engine's own residual expression:
 *        constant:  f - coeff*(((dn+up)*ihx2 + (ea+w_)*ihy2) - v*diag),  ihx2 = 1/(hx*hx), diag = 2/(hx*hx) + 2/(hy*hy) [+ sigma]
 *        variable:  f - coeff*((sx*ihx2 + sy*ihy2) - v*D)  with the face means, sx, sy and D of mg_set_coefficient
 *   g  = (kappa*w)*phi(v)      (without w: kappa*phi(v))
 *   F  = r0 - g
 *   c  = (kappa*w)*phi'(v)     (without w: kappa*phi'(v))
 * with phi and phi' in the forms of the enum below; sinh, cosh and exp are the device math library's. */
#ifndef MGHIP_NL_H
#define MGHIP_NL_H

#include "mghip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MG_NL_LINEAR = 0,   /* phi = u,       phi' = 1         */
               MG_NL_CUBIC  = 1,   /* phi = (u*u)*u, phi' = 3.0*(u*u) */
               MG_NL_SINH   = 2,   /* phi = sinh u,  phi' = cosh u    */
               MG_NL_EXP    = 3 }  /* phi = exp u,   phi' = exp u     */ mg_nl_kind;

/* One pass per Newton trial: fp64 device arrays (nx, ny) with pitch `ld` (elements, even), 16-byte aligned; asynchronous on
 * `stream` (nullable); scratch >= mg_dev_scratch_bytes(nx, ny).  With v, F and c as above:
 *   u_out (nullable; ignored with delta NULL) := v on interior cells, the ring of u on the ring;
 *   F (nullable) := F on interior cells, 0 on the ring;   c (nullable) := c on interior cells, 0 on the ring;
 *   sums_dev[0] := the sum of F^2, sums_dev[1] := the sum of c, both over interior cells: per-workgroup partials followed by a
 *   fixed-order pass, the same bits on every run.
 * Exactly the cells [0, nx) x [0, ny) of each non-NULL output are stored; outputs are arrays of their own (u_out != u: a
 * neighbouring workgroup reads u on this tile's edge).  The ring of delta and the ring of f are not read.  A non-finite cell
 * of u or delta makes sums_dev[0] non-finite and leaves the cells outside its stencil as they would have been.
 * MG_NL_LINEAR with w := c, kappa = 1 gives b - (A x + c x): the residual of the reaction-field loop below. */
int mg_dev_nl_eval(int kind, int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, double kappa,
                   const double* a_or_null, const double* w_or_null, const double* u, const double* delta_or_null, double t,
                   const double* f, double* u_out_or_null, double* F_or_null, double* c_or_null, void* scratch, double* sums_dev,
                   void* stream);
/* host arrays (nx, ny), fp64: upload with the library's pitch, run the kernel, download; sums: 2 doubles on the host */
int mg_op_nl_eval(int kind, int nx, int ny, double hx, double hy, double coeff, double sigma, double kappa, const double* a_or_null,
                  const double* w_or_null, const double* u, const double* delta_or_null, double t, const double* f,
                  double* u_out_or_null, double* F_or_null, double* c_or_null, double* sums);

/* A reaction field in the Krylov outer loop: with a field set the outer operator of the mg_pcg is A + diag(c) -- q = A p + c p
 * in the direction kernel, the initial and the true residual from mg_dev_nl_eval's kernel in linear kind -- while the
 * preconditioner stays the engine's cycle with the SCALAR shift sigma + c_ref (mg_pcg_set_shift keeps setting sigma and
 * re-applies sigma + c_ref to the engine).  c_dev is an fp64 device array in the solver's pitch (ld must equal
 * mg_pitch_elems(MG_F64, ny)), 16-byte aligned, c >= 0 with a zero ring; it is NOT copied: the caller keeps it alive and may
 * rewrite it between solves.  NULL (c_ref is then ignored) returns to the loop as it is without this call, bit for bit.
 * Under mg_pcg_set_order(4): MG_ERR_STATE, and so is mg_pcg_set_order(4) with a field set.  c_ref < 0 or non-finite, or a
 * wrong pitch: MG_ERR_INVALID_VALUE.  An indefinite c needs no check of its own: the breakdown flag (status 2) catches it.
 * Look-ahead, the flexible beta, the stats and the norms are unchanged. */
int mg_pcg_set_reaction_device(mg_pcg* s, const double* c_dev_or_null, int ld, double c_ref);
/* mg_dev_pcg_direction with q = A p_out + c p_out (c: a field like a, its ring is not used) */
int mg_dev_pcg_direction_react(int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, const double* a_or_null,
                               const double* c, const double* z, const double* p_in_or_null, double* p_out, double* q,
                               const double* beta_dev_or_null, void* scratch, double* pq_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The Newton driver.  An mg_nl OWNS an mg_pcg (and through it the preconditioner engine) built from `cfg` under mg_pcg_create's
 * rules, two iterate buffers, two F / c pairs (current and trial), delta and the optional a and w.  All work is queued on the
 * engine's stream; per trial the host reads only the two sums.
 *
 *   1. eval at u0: ||F_0||, c and cbar = sums[1] / ((nx-2)(ny-2))
 *   2. for k = 0 ..: stop with status 0 when ||F_k|| < tol (absolute).  Forcing term (Eisenstat-Walker, choice 2):
 *      eta_0 = eta_max, eta_k = gamma (||F_k|| / ||F_{k-1}||)^2, raised to gamma eta_{k-1}^2 when that exceeds 0.1, clipped to
 *      [eta_min, eta_max]; forcing = MG_NL_FORCING_FIXED uses the constant `eta`.  Inner tolerance max(eta_k ||F_k||, 0.1 tol).
 *   3. mg_pcg_set_reaction_device(c, ld, cbar); delta = 0; conjugate gradients on J delta = F_k to the inner tolerance, at most
 *      max_inner iterations.  A breakdown with no accepted iteration: status 2.
 *   4. backtracking from t = 1: eval (u_k, delta, t) into the trial buffers; accept when the trial norm is finite and
 *      <= (1 - 1e-4 t) ||F_k||, then swap buffers; otherwise t /= 2, at most max_backtracks times; beyond that status 3 and u_k
 *      is returned.  An exp / sinh overflow therefore rejects the trial and never ends up in the iterate.
 *   5. max_newton reached: status 1.
 * norm_hist[k] is ||F_{k+1}||, inner_hist[k] the inner iterations, step_hist[k] the accepted t and eta_hist[k] the forcing
 * term of Newton step k + 1 (each array holds hist_cap entries; inner_hist, step_hist and eta_hist are nullable).
 * ------------------------------------------------------------------------------------------------ */
typedef struct mg_nl mg_nl;
typedef enum { MG_NL_FORCING_EISENSTAT_WALKER = 0, MG_NL_FORCING_FIXED = 1 } mg_nl_forcing;
typedef struct mg_nl_options {
  int32_t forcing;          /* mg_nl_forcing                                              default Eisenstat-Walker */
  int32_t max_backtracks;   /* halvings of the step after the full one                    default 10               */
  int32_t max_inner;        /* conjugate-gradient iterations per Newton step              default 100              */
  int32_t reserved;
  double eta;               /* the constant forcing term of MG_NL_FORCING_FIXED           default 1e-8             */
  double gamma, eta_max, eta_min;   /*                                                    defaults 0.9, 0.1, 1e-10 */
} mg_nl_options;
typedef struct mg_nl_stats {
  double solve_seconds;      /* host wall time of the device-resident solve                          */
  double initial_residual;   /* ||F_0||                                                               */
  double final_residual;     /* ||F|| of the returned iterate                                         */
  int32_t newton_iterations;
  int32_t inner_iterations;  /* conjugate-gradient iterations, all Newton steps together              */
  int32_t evaluations;       /* launches of the eval kernel by the driver (the inner loops' excluded) */
  int32_t status;            /* 0 tolerance met, 1 max_newton, 2 inner breakdown, 3 line search failed */
} mg_nl_stats;

int mg_nl_create(const mg_config* cfg, int num_cycles, int flexible, mg_nl** out);
int mg_nl_destroy(mg_nl* s);
const char* mg_nl_last_error(const mg_nl* s);
int mg_nl_options_default(mg_nl_options* opt);
/* as mg_pcg_set_coefficient / mg_pcg_set_shift (forwarded), for the eval kernel too */
int mg_nl_set_coefficient(mg_nl* s, const void* a_host_or_null, int host_dtype);
int mg_nl_set_shift(mg_nl* s, double sigma);
/* kind outside mg_nl_kind, kappa < 0 or non-finite, a negative or non-finite entry of w: MG_ERR_INVALID_VALUE, the solver is
 * left as it was.  w is an (nx, ny) host array of host_dtype (its ring is not used), NULL: w == 1. */
int mg_nl_set_nonlinearity(mg_nl* s, int kind, double kappa, const void* w_host_or_null, int host_dtype);
int mg_nl_set_options(mg_nl* s, const mg_nl_options* opt);
/* f, u0 (nullable: zero) and u_out are host arrays of host_dtype; the ring of u0 is the Dirichlet data */
int mg_nl_solve(mg_nl* s, const void* f, const void* u0_or_null, void* u_out, int host_dtype, double tol, int max_newton,
                double* norm_hist, int* inner_hist, double* step_hist, double* eta_hist, int hist_cap, int* n_newton,
                int* converged, mg_nl_stats* stats);
/* device arrays of `dtype` with pitches in elements; u_dev -- in: initial iterate + Dirichlet ring, out: the solution */
int mg_nl_solve_device(mg_nl* s, const void* f_dev, int ld_f, void* u_dev, int ld_u, int dtype, double tol, int max_newton,
                       double* norm_hist, int* inner_hist, double* step_hist, double* eta_hist, int hist_cap, int* n_newton,
                       int* converged, mg_nl_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* MGHIP_NL_H */
