/* mghip_flow.h -- 2-D incompressible flow in the vorticity / stream-function form on the multigrid engine of libmghip.so,
 * state resident on the device.  Same conventions as mghip.h: C ABI, status codes, pitches in elements; i is x, j is y.
 *
 *   w_t = J(psi, w) + nu lap w + F(x, y),   -lap psi = w,   u = psi_y,  v = -psi_x,   psi = 0 on the whole ring
 *
 * (one closed wall, no through-flow; F is an optional static forcing, the curl of a body force).  Crank-Nicolson for the
 * diffusion, variable-step Adams-Bashforth 2 for N = J + F.  With sigma = 2/(nu dt), k = 2/nu, r = dt/dt_prev:
 *
 *   (-lap + sigma) w_new = f,   f = (sigma*w + lap w) + k*((c0*N) + (c1*N_prev)),   c0 = 1 + r/2,  c1 = -r/2
 *   -lap psi_new = w_new on interior cells (right-hand side 0 on the ring), warm-started from psi
 *
 * f is 0 on the ring.  On the first step after mg_flow_set_state c0 = 1, c1 = 0, f = (sigma*w + lap w) + k*(c0*N) and N_prev
 * is not read.  lap is mg_op_apply(coeff = +1) bit for bit; J is Arakawa's nine-point Jacobian (1966), which conserves energy
 * and enstrophy, in this association (E/W = i +- 1, N/S = j +- 1, p = psi):
 *   J1 = (E(p)-W(p))*(N(w)-S(w)) - (N(p)-S(p))*(E(w)-W(w))
 *   J2 = ((E(p)*(NE(w)-SE(w)) - W(p)*(NW(w)-SW(w))) - N(p)*(NE(w)-NW(w))) + S(p)*(SE(w)-SW(w))
 *   J3 = ((NE(p)*(N(w)-E(w)) - SW(p)*(W(w)-S(w))) - NW(p)*(N(w)-W(w))) + SE(p)*(E(w)-S(w))
 *   J  = ((J1 + J2) + J3) / (12.0*hx*hy)
 * Walls: the Dirichlet data of the w solve is the ring of its initial guess, written from psi (the OLD time level) before the
 * solve: 0 (MG_FLOW_FREE_SLIP) or Thom's formula (MG_FLOW_NO_SLIP) with the wall speeds {left v, right v, bottom u, top u}
 *   left   (i = 0):      (2.0*(psi_w - psi_in))/(hx*hx) - (2.0*v_l)/hx       right (i = nx-1):  ... + (2.0*v_r)/hx
 *   bottom (j = 0):      (2.0*(psi_w - psi_in))/(hy*hy) + (2.0*u_b)/hy       top   (j = ny-1):  ... - (2.0*u_t)/hy
 * applied in this order, so corners carry bottom and top (mg_dev_heat_ring's order; corner vorticity only ever multiplies
 * ring psi = 0).  The wall value lags by one step: first order in dt at no-slip walls, second order elsewhere.
 *
 * mg_flow owns two engines built from one mg_config (psi: shift 0; w: shift sigma, mg_set_shift only when dt changes), the
 * fields w, psi, N, f and F, all on one stream.  cfg.precision must be MG_PREC_DOUBLE, cfg.coeff -1 and cfg.fmg_cycles 0, nu
 * finite and > 0, wall_kind one of the two codes: anything else returns MG_ERR_INVALID_VALUE before any device work.  Each
 * solve stops at ||r|| < tol * max(1, ||f||_h); tol = 0 runs exactly max_cycles cycles (mg_heat's conventions).  Per step two
 * small readbacks (sum f^2 and the velocity maximum; sum w^2 and max |w_new - w|) plus mg_iterate's mailbox; no field crosses
 * to the host.
 *
 * Special values.  Every maximum here (the velocity maximum m, max |w_new - w|) propagates NaN: it is NaN if any participating
 * value is, otherwise the maximum, which may be +Inf; for finite fields it is fmax's value bit for bit.  The sums are plain
 * IEEE sums of the participating cells (interior cells; ring, pad columns and rows outside the array never contribute).  A
 * step on a state that holds a NaN or an Inf (mg_flow_set_device copies what it is given; a run can also blow up by itself)
 * returns MG_OK: cfl, omega_change, the norms and the residuals of its info are non-finite wherever the restatement's are,
 * tol * max(1, NaN) is tol, both solves run max_cycles cycles and report converged = 0.  The stepper stays usable:
 * mg_flow_set_state with a finite field gives the steps of a fresh stepper. */
#ifndef MGHIP_FLOW_H
#define MGHIP_FLOW_H

#include "mghip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_flow mg_flow;
typedef enum { MG_FLOW_FREE_SLIP = 0, MG_FLOW_NO_SLIP = 1 } mg_flow_wall;
typedef enum { MG_FLOW_OMEGA = 0, MG_FLOW_PSI = 1, MG_FLOW_N = 2 } mg_flow_field;

typedef struct mg_flow_step_info {
  double sigma, c0, c1;
  double cfl;                 /* dt m / (2 hx hy), m = max(|N(p)-S(p)| + |E(p)-W(p)|) of the psi the step started from */
  double rhs_norm;            /* ||f||_h of the w solve */
  double omega_initial_residual, omega_final_residual;
  double psi_rhs_norm;        /* ||w_new||_h over interior cells */
  double psi_initial_residual, psi_final_residual;
  double omega_change;        /* max |w_new - w| over all cells (the ring of w already holds the new wall values) */
  double seconds;             /* host wall clock of the whole step */
  int32_t omega_cycles, psi_cycles;
  int32_t omega_converged, psi_converged;
} mg_flow_step_info;

int mg_flow_create(const mg_config* cfg, double nu, int wall_kind, mg_flow** out);
int mg_flow_destroy(mg_flow* s);
const char* mg_flow_last_error(const mg_flow* s);
/* wall speeds {left v, right v, bottom u, top u} (all 0 after create); finite.  Read by the next wall update. */
int mg_flow_set_walls(mg_flow* s, const double* speeds4);
/* static forcing F(x, y) (host array (nx, ny); NULL: none).  A non-finite value returns MG_ERR_INVALID_VALUE before any
 * device work and leaves the stepper as it was. */
int mg_flow_set_forcing(mg_flow* s, const void* f_host_or_null, int host_dtype);
/* w := the host array, psi := the solution of -lap psi = w from psi = 0, the ring of w := the wall values of that psi, and
 * the Adams-Bashforth history is cleared.  Only the psi_* fields (and seconds) of `info_or_null` are filled. */
int mg_flow_set_state(mg_flow* s, const void* omega_host, int host_dtype, double tol, int max_cycles, mg_flow_step_info* info_or_null);
/* which = MG_FLOW_OMEGA, MG_FLOW_PSI or MG_FLOW_N (N of the latest step: the N_prev of the next) */
int mg_flow_get(mg_flow* s, int which, void* host, int host_dtype);
/* the same into / from a device array of `dtype` with pitch ld >= ny (no host transfer); set copies the field as it is (no
 * solve, no wall update, the history flag unchanged) */
int mg_flow_get_device(mg_flow* s, int which, void* u_dev, int ld, int dtype);
int mg_flow_set_device(mg_flow* s, int which, const void* u_dev, int ld, int dtype);
int mg_flow_step(mg_flow* s, double dt, double tol, int max_cycles, mg_flow_step_info* info_or_null);
/* out = {sum psi*w, sum w^2} over interior cells: kinetic energy = 0.5 hx hy out[0], enstrophy = 0.5 hx hy out[1] */
int mg_flow_diagnostics(mg_flow* s, double out[2]);
/* m = max(|N(p)-S(p)| + |E(p)-W(p)|) of the current psi: a step of dt runs at cfl = dt m / (2 hx hy) */
int mg_flow_velocity_max(mg_flow* s, double* m);

/* ---- the kernels call by call (fp64 device arrays (nx, ny) with an even pitch ld >= ny in elements and 16-byte aligned
 * bases; scratch >= mg_dev_scratch_bytes(nx, ny); nullable stream; asynchronous).  Outputs are arrays of their own; rows
 * 0..nx-1 of an output are stored as whole 16-byte vectors up to column roundup(ny, 2) (a pad column there is written 0). ---- */
/* f and N as above (n_prev NULL: the first-step form; force NULL: N = J); out2_dev_or_null[0] = sum f^2, [1] = the velocity
 * maximum m */
int mg_dev_flow_rhs(int nx, int ny, int ld, double hx, double hy, double nu, double dt, double c0, double c1,
                    const double* psi, const double* omega, const double* n_prev_or_null, const double* force_or_null,
                    double* f_out, double* n_out, void* scratch, double* out2_dev_or_null, void* stream);
/* the ring of omega from psi (in place; the interior is untouched) */
int mg_dev_flow_wall(int nx, int ny, int ld, double hx, double hy, int wall_kind, const double* speeds4,
                     const double* psi, double* omega, void* stream);
/* out3_dev = {sum psi*w, sum w^2, velocity maximum m} over interior cells */
int mg_dev_flow_diag(int nx, int ny, int ld, const double* psi, const double* omega, void* scratch, double* out3_dev, void* stream);
/* out = w with a zero ring (the right-hand side of the psi solve); out2_dev_or_null[0] = sum out^2, [1] = max |w - w_old| over
 * all cells (0 without w_old) */
int mg_dev_flow_interior(int nx, int ny, int ld, const double* w, const double* w_old_or_null, double* out, void* scratch,
                         double* out2_dev_or_null, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGHIP_FLOW_H */
