/* mghip_line.h -- zebra line relaxation of libmghip.so (the smoother kinds MG_ZEBRA_X / MG_ZEBRA_Y / MG_ZEBRA_ALT of
 * include/mghip.h), call by call.  Same conventions as mghip.h: C ABI, status codes, pitches in elements.  No reference
 * counterpart: the reference has point smoothers only (its BlockDiagonalPreconditioner builds dense tridiagonal blocks).
 *
 * One sweep of one direction runs colour 0 then colour 1; the colour of a line is the parity of its grid index (the fixed j
 * of an X line, the fixed i of a Y line).  For every line of the colour it solves tridiag(-w, D, -w) x = b with
 *   w = 1 / h_par^2,  c = 1 / h_perp^2,  D = 2 w + 2 c + sigma,
 *   b = rhs + c (u_prev_line + u_next_line), plus w * ring value at the first and then at the last cell,
 * and sets u_line = u_line + omega (x - u_line) (omega == 1: u_line = x, without the two roundings): the sweeps relax -Laplace + sigma.  MG_ZEBRA_X lines run along i (all
 * interior i at a fixed j: implicit in x, for hx < hy), MG_ZEBRA_Y lines along j (contiguous in memory, for hy < hx);
 * MG_ZEBRA_ALT is an X sweep followed by a Y sweep.  The ring of u is never changed.
 *
 * A plan holds what is factored for one (dtype, direction, shape, spacings, sigma): all lines share one Toeplitz matrix, so
 * the pivots of its chunks, the chunk spikes and the pivots of the separator system are tables, computed in extended
 * precision on the host, rounded once to `dtype` and kept on the device; per-line arithmetic runs in `dtype`
 * (csrc/mg_line_kernels.hpp).  A workgroup keeps whole lines in LDS: lines of more than 16384 cells are refused
 * (MG_ERR_INVALID_VALUE).  Same bits on every run. */
#ifndef MGHIP_LINE_H
#define MGHIP_LINE_H

#include "mghip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_line_plan mg_line_plan;
/* direction: MG_ZEBRA_X or MG_ZEBRA_Y; (nx, ny) array with pitch ld (elements; a multiple of 16 bytes); sigma >= 0.
 * Bad arguments return MG_ERR_INVALID_VALUE before any device work. */
int mg_line_plan_create(int dtype, int direction, int nx, int ny, int ld, double hx, double hy, double sigma, mg_line_plan** out);
int mg_line_plan_destroy(mg_line_plan* p);
/* one colour pass in place on the device array u (16-byte aligned, as rhs), asynchronous on `stream`.  Rows 1 .. nx - 2 are
 * stored as whole 16-byte vectors (ring and pad columns with the bits they held), only where a vector holds a line of the colour. */
int mg_dev_line_colour(mg_line_plan* p, int colour, double omega, void* u, const void* rhs, void* stream);
/* nu sweeps on host arrays, like mg_op_rbgs; smoother = MG_ZEBRA_X | MG_ZEBRA_Y | MG_ZEBRA_ALT */
int mg_op_zebra(int dtype, int smoother, int nx, int ny, double hx, double hy, double sigma, double omega, int nu,
                const void* u, const void* rhs, void* out);
/* hipEvent-timed repetitions of one full sweep (both colours) of the plan's direction on arrays the call allocates */
int mg_line_time_sweep(mg_line_plan* p, int reps, double* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* MGHIP_LINE_H */
