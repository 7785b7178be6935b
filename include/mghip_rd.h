/* mghip_rd.h -- reaction-diffusion time stepping on the device: the heat stepper's three implicit schemes (include/mghip.h,
 * "Time stepping"; include/mghip_heat.h) with one Newton solve of include/mghip_nl.h per step.  Same conventions as mghip.h:
 * C ABI, status codes, pitches in elements.  No reference counterpart.
 *
 *   du/dt = alpha L_a u - kappa w(x, y) phi(u) + rho u + g(t) S(x, y)
 *
 * L_a is mg_dev_heat_rhs_var's operator (the five-point Laplacian without a field `a`), phi one of mg_nl_kind (monotone, so
 * kappa >= 0 and w >= 0: implicit), rho a finite scalar of either sign (explicit: extrapolated from old time levels -- what
 * convex splitting needs for Allen-Cahn, u - u^3: the cubic implicit, +u explicit), S an optional source profile.
 *
 * Every scheme is divided by alpha, as the heat stepper's.  The problem of one step is
 *   N(v) = (-L_a + lambda) v + (kappa/alpha) w phi(v) = f,      v = u^{n+1}, Dirichlet data on the ring of the initial iterate,
 * which is mg_nl's with coeff = -1, sigma = lambda and the strength ka = kappa/alpha (one division on the host).
 *
 * The right-hand side per interior cell, in exactly this association (no FMA contraction); uc = u, pv = u_prev, sc = S (0
 * without a source), lap = L_a u in heat_rhs_kernel's expression, ph = phi(uc) in mg_nl_kind's forms, dta = dt*alpha:
 *   implicit Euler   lambda = 1/(dt alpha)     f = (uc + dt*((g1*sc) + rho*uc)) / dta
 *   Crank-Nicolson   lambda = 2/(dt alpha)     h = (2.0*((uc + (dta*lap)/2) + (dt*((g0*sc) + (g1*sc)))/2)) / dta
 *                                              f = (h + r2a*E) - kw*ph,   kw = ka*w (ka without w),  r2a = (2.0*rho)/alpha,
 *                                              E = (3.0*uc - pv)/2 with a previous level (CN-AB2), else E = uc
 *   BDF2 (SBDF2)     lambda = 3/(2 dt alpha)   f = ((4.0*uc - pv)/(2*dt*alpha) + (g1*sc)/alpha) + ra*(2.0*uc - pv),  ra = rho/alpha
 * The ring of f is 0.  h and the first BDF2 term are heat_rhs_kernel's own expressions: with kappa = 0 and rho = 0 the output
 * equals mg_dev_heat_rhs_var's as numbers.  Explicit Euler (scheme 0) is refused.  BDF2 is started by the caller with one
 * Crank-Nicolson step.  The observed orders in time are 1, 2 and 2.
 *
 * The discrete free energy, for which the equation is the gradient flow  u_t = -(1/(hx hy)) dE/du  (g S == 0):
 *   E(u) = alpha G(u) + hx hy (kappa P(u) - rho Q(u)/2)
 *   G = the sum over cells of 0.5*((aip*(du*du))*(hy/hx) + (ajp*(dv*dv))*(hx/hy)),  du = u_dn - uc, dv = u_ea - uc: each cell
 *       owns the face to its next row (counted for rows 0 .. nx-2, columns 1 .. ny-2) and to its next column (rows 1 .. nx-2,
 *       columns 0 .. ny-2), which are the faces with at least one interior endpoint; aip = 0.5*(a_c + a_dn), ajp = 0.5*(a_c +
 *       a_ea) are mg_set_coefficient's face means (1 without a field, then the products by them are not formed).  Its gradient
 *       on interior cells is -hx hy L_a u for any ring data.
 *   P = the sum over interior cells of w*Phi(uc) (Phi(uc) without w),  Phi = (uc*uc)/2, ((uc*uc)*(uc*uc))/4, cosh(uc) - 1.0,
 *       exp(uc) for the four kinds: Phi' = phi, Phi >= 0.
 *   Q = the sum over interior cells of uc*uc.
 * Implicit Euler with rho >= 0 (convex splitting) decreases E for every dt > 0 (zero source, fixed ring):
 *   E(u^{n+1}) - E(u^n) <= -||u^{n+1} - u^n||_h^2 / dt + alpha ||F||_h ||u^{n+1} - u^n||_h,  F the step's Newton residual (of the
 *   equation divided by alpha, hence the factor). */
#ifndef MGHIP_RD_H
#define MGHIP_RD_H

#include "mghip_nl.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The right-hand side of one step in ONE pass, call by call: fp64 device arrays (nx, ny) with pitch `ld` (elements, even),
 * 16-byte aligned; asynchronous on `stream` (nullable); scratch >= mg_dev_scratch_bytes(nx, ny).  scheme is
 * MG_HEAT_IMPLICIT_EULER, MG_HEAT_CRANK_NICOLSON or MG_HEAT_BDF2; kind an mg_nl_kind (read by Crank-Nicolson only, as a and w
 * are); u_prev is required by BDF2, optional for Crank-Nicolson (NULL: E = u) and ignored by implicit Euler.  Exactly the cells
 * [0, nx) x [0, ny) of `out` are stored (whole 16-byte vectors where they hold no pad column), 0 on the ring; `out` overlaps
 * no input.  sumsq_dev_or_null := the sum of out^2 over the array: per-workgroup partials followed by a fixed-order pass, the
 * same bits on every run.  kappa < 0, a non-finite kappa, rho, dt or alpha, dt <= 0, alpha <= 0, scheme 0 or unknown, a kind
 * outside the enum: MG_ERR_INVALID_VALUE before any device work. */
int mg_dev_rd_rhs(int scheme, int kind, int nx, int ny, int ld, double hx, double hy, double alpha, double dt, double kappa,
                  double rho, const double* u, const double* u_prev_or_null, const double* src_or_null, const double* a_or_null,
                  const double* w_or_null, double g0, double g1, double* out, void* scratch, double* sumsq_dev_or_null,
                  void* stream);
/* sums3_dev := {G, P, Q} of the state u (above) in one pass, by the same fixed-order reduction.  scratch holds three sets of
 * partials: mg_dev_scratch_bytes(nx, ny) suffices unless nx < 64 and ny > 10000 (then MG_ERR_INVALID_VALUE).  A non-finite
 * cell makes the sums it enters non-finite: an interior cell all three, a ring cell G. */
int mg_dev_rd_energy(int kind, int nx, int ny, int ld, double hx, double hy, const double* a_or_null, const double* w_or_null,
                     const double* u, void* scratch, double* sums3_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The stepper.  An mg_rd OWNS an mg_nl (and through it the Krylov loop and the preconditioner engine) built from `cfg` under
 * mg_pcg_create's rules -- cfg.precision MG_PREC_DOUBLE, MG_PREC_SINGLE_MANAGED or MG_PREC_MIXED_LEVELS is the
 * PRECONDITIONER's, the state is always fp64; cfg.coeff must be -1 and cfg.fmg_cycles 0; alpha finite and > 0 --, four fp64
 * state slots, the right-hand side and the optional S, a and w.  All work is queued on the engine's stream; no field crosses
 * PCIe between steps.
 *
 * mg_rd_step(scheme, dt, src, prev, dst, g0, g1, edge4, tol, max_newton):
 *   1. f = rhs(slot src [, slot prev]) and ||f||_h = sqrt(hx hy sum f^2)
 *   2. mg_nl_set_shift(lambda) when lambda differs from the one the solver carries
 *   3. slot dst := slot src, then its ring from edge4 = {left, right, bottom, top} in mg_dev_heat_ring's order (the data of
 *      t + dt; NULL keeps src's ring)
 *   4. mg_nl_solve_device(f, slot dst) to the absolute tolerance tol * max(1, ||f||_h), at most max_newton Newton steps
 * g0, g1 are the source's time factors at t and t + dt.  prev is -1 for implicit Euler, a slot or -1 for Crank-Nicolson, a
 * slot for BDF2.  dst differs from src and prev; src and prev are never written.  A Newton status other than 0 (mg_nl_stats)
 * is converged = 0 with MG_OK and dst holds the last accepted iterate: a breakdown is not an error code.
 * MG_ERR_INVALID_VALUE, before any device work and with the stepper unchanged: a slot outside 0..3, dst == src or dst == prev,
 * BDF2 without prev, prev given to implicit Euler, dt <= 0 or non-finite, scheme 0 or unknown, max_newton < 1, a NaN tol,
 * non-finite g0 / g1.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mg_rd mg_rd;
typedef struct mg_rd_step_info {
  double lambda;             /* the shift of the step's inner problem                      */
  double rhs_norm;           /* ||f||_h                                                    */
  double initial_residual;   /* ||f - N(u_src with the new ring)||_h                       */
  double final_residual;     /* ||f - N(u_dst)||_h                                         */
  double solve_seconds;      /* mg_nl_stats.solve_seconds                                  */
  int32_t newton_iterations;
  int32_t inner_iterations;  /* conjugate-gradient iterations, all Newton steps together   */
  int32_t evaluations;
  int32_t status;            /* mg_nl_stats.status                                         */
  int32_t converged;
  int32_t reserved;
} mg_rd_step_info;           /* 64 bytes */

int mg_rd_create(const mg_config* cfg, double alpha, int num_cycles, int flexible, mg_rd** out);
int mg_rd_destroy(mg_rd* s);
const char* mg_rd_last_error(const mg_rd* s);
/* the state slots 0..3: host arrays (nx, ny) of host_dtype / device arrays of `dtype` with pitch ld (elements) */
int mg_rd_set_slot(mg_rd* s, int slot, const void* u_host, int host_dtype);
int mg_rd_get_slot(mg_rd* s, int slot, void* u_host, int host_dtype);
int mg_rd_set_slot_device(mg_rd* s, int slot, const void* u_dev, int ld, int dtype);
int mg_rd_get_slot_device(mg_rd* s, int slot, void* u_dev, int ld, int dtype);
/* the diffusivity field a(x, y) (host array; NULL: a == 1): any non-finite or <= 0 value is MG_ERR_INVALID_VALUE, checked on
 * the host array before any device work; forwarded to the mg_nl, and kept for the right-hand side and the energy */
int mg_rd_set_coefficient(mg_rd* s, const void* a_host_or_null, int host_dtype);
/* the source profile S(x, y) (host array; NULL: none) */
int mg_rd_set_source(mg_rd* s, const void* profile_host_or_null, int host_dtype);
/* -kappa w phi(u) + rho u.  mg_nl_set_nonlinearity's refusals hold for kind, kappa and w (checked on the host array first);
 * kappa/alpha goes to the mg_nl; a non-finite rho is refused.  Before this call: linear kind, kappa = 0, rho = 0. */
int mg_rd_set_reaction(mg_rd* s, int kind, double kappa, const void* w_host_or_null, int host_dtype, double rho);
int mg_rd_set_newton_options(mg_rd* s, const mg_nl_options* opt);
int mg_rd_step(mg_rd* s, int scheme, double dt, int src, int prev, int dst, double g0, double g1, const double* edge4_or_null,
               double tol, int max_newton, mg_rd_step_info* info);
/* out = {G, P, Q, E} of a slot (E formed on the host from the three device sums) */
int mg_rd_energy(mg_rd* s, int slot, double out[4]);
/* ||slot_a - slot_b||_h = sqrt(hx hy (sum over all cells of (a - b)^2)) */
int mg_rd_diff_norm(mg_rd* s, int slot_a, int slot_b, double* out);

#ifdef __cplusplus
}
#endif
#endif /* MGHIP_RD_H */
