/* mghip_heat.h -- extensions of the time stepper of libmghip.so (include/mghip.h, "Time stepping"): a diffusivity field and a
 * conjugate-gradient inner solver.  Same conventions as mghip.h: C ABI, status codes, pitches in elements. */
#ifndef MGHIP_HEAT_H
#define MGHIP_HEAT_H

#include "mghip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Variable diffusivity: mg_heat_set_coefficient(a) turns the equation into  du/dt = alpha div(a(x, y) grad u) + g(t) S(x, y).
 * alpha stays the scalar it is; `a` is a vertex field (nx, ny) in the engine's discretisation (mg_set_coefficient: face values
 * are arithmetic means, coarse levels take `a` injected).  Every formula of mghip.h's "Time stepping" block holds with lap replaced by
 *   L_a u = (sx*ihx2 + sy*ihy2) - u*D0,  sx = aip*dn + aim*up,  sy = ajp*ea + ajm*w,  D0 = (aip + aim)*ihx2 + (ajp + ajm)*ihy2,
 *   aip = 0.5*(a_c + a_dn), aim = 0.5*(a_c + a_up), ajp = 0.5*(a_c + a_e), ajm = 0.5*(a_c + a_w)
 * (the association of the engine's variable-coefficient residual; the ring values of `a` are read by the faces next to the
 * boundary), the shifts stay 1/(dt alpha), 2/(dt alpha), 3/(2 dt alpha), and the inner system is (-div(a grad) + lambda) u = f.
 * Any non-finite or <= 0 value of `a` returns MG_ERR_INVALID_VALUE before any device work and leaves the stepper as it was.
 * Otherwise the stepper keeps an fp64 device copy for the right-hand-side kernel (explicit Euler and Crank-Nicolson read it;
 * implicit Euler and BDF2 do not: their right-hand sides hold no operator) and forwards the array to its inner solver; the
 * shift the inner solver carried is set again with the next implicit step.  NULL returns to the constant operator and frees
 * the copy; without a coefficient nothing changes, bit for bit.  The engine refreshes the reciprocal diagonals of every level
 * on EVERY mg_set_shift under a coefficient (one pass over the hierarchy); the stepper calls it only when lambda changes, which
 * step doubling does three times per attempt (dt, dt/2, back to dt).
 *
 * Inner solver: mg_heat_create_ex(cfg, alpha, inner, num_cycles, flexible, out).  MG_HEAT_INNER_CYCLE is the plain multigrid
 * cycle described there (num_cycles and flexible are ignored; mg_heat_create is this with 0, 0).  With MG_HEAT_INNER_PCG the
 * stepper owns an mg_pcg built from cfg (num_cycles, flexible as in mg_pcg_create) in place of a bare engine: cfg.precision may
 * be MG_PREC_DOUBLE, MG_PREC_SINGLE_MANAGED or MG_PREC_MIXED_LEVELS -- the state, the right-hand side and the Krylov vectors
 * stay fp64, only the preconditioner runs in cfg.precision -- and cfg.coeff -1, cfg.fmg_cycles 0 are still required.  An
 * implicit step is then: f and sum f^2 -> mg_pcg_set_shift(lambda) when it changed -> mg_pcg_solve_device on the stepper's
 * arrays from the same initial iterate (ring included) -> dst.  The stopping rule is unchanged (mg_pcg's norm is what
 * mg_residual_norm gives; tol = 0 runs exactly max_cycles iterations); mg_heat_step_info keeps its layout, `cycles` is the
 * iteration count, solve_seconds mg_pcg's; a breakdown (status 2) is converged = 0, not an error code.  The plain cycle stalls
 * on jumping coefficients where the conjugate-gradient loop converges.  Slots, the ring order,
 * mg_heat_diff_norm and explicit Euler (no inner solver) are the same for both.
 * ------------------------------------------------------------------------------------------------ */
typedef enum { MG_HEAT_INNER_CYCLE = 0, MG_HEAT_INNER_PCG = 1 } mg_heat_inner;
int mg_heat_create_ex(const mg_config* cfg, double alpha, int inner, int num_cycles, int flexible, mg_heat** out);
/* the diffusivity field a(x, y) > 0 (host array; NULL: the constant operator, a == 1); both inner solvers */
int mg_heat_set_coefficient(mg_heat* s, const void* a_host_or_null, int host_dtype);
/* mg_dev_heat_rhs with lap = L_a u ("Variable diffusivity" above): `a` has the pitch and alignment of u and does not overlap
 * out; it is read by explicit Euler and Crank-Nicolson only (tile + halo staged in a second LDS array).  NULL: mg_dev_heat_rhs. */
int mg_dev_heat_rhs_var(int scheme, int nx, int ny, int ld, double hx, double hy, double alpha, double dt,
                        const double* u, const double* u_prev_or_null, const double* src_or_null, const double* a_or_null,
                        double g0, double g1, double* out, void* scratch, double* sumsq_dev_or_null, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGHIP_HEAT_H */
