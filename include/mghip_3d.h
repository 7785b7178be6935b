/* mghip_3d.h -- geometric multigrid in three dimensions on the device: A u = f with the seven-point operator
 * A = -(dxx + dyy + dzz) + sigma, sigma >= 0, constant coefficients, on a vertex-centred (nx, ny, nz) grid with Dirichlet data in
 * the boundary faces of the iterate.  A family of its own beside the 2-D engine of mghip.h: same conventions (C ABI, status
 * codes, mg_dtype, pitches in elements), prefix mg3_, no shared state.  No reference counterpart (the reference's
 * PoissonSolver3D raises NotImplementedError).
 *
 * LAYOUT.  Cell (i, j, k) of a field sits at element (i * ny + j) * ld + k: k is the fastest index, `ld` the row pitch in
 * elements (even, >= nz; mg_pitch_elems(dtype, nz) is the engine's own), ny * ld the plane stride.  Bases are 16-byte aligned; an fp32
 * pitch that is no multiple of 4 is served element by element instead of in 16-byte vectors.
 * The pad columns k >= nz of a row are never summed and never stored.  A cell is INTERIOR when 0 < i < nx-1, 0 < j < ny-1 and
 * 0 < k < nz-1; the other cells are the boundary faces.  Every kernel below stores interior cells only, unless it says otherwise.
 *
 * ARITHMETIC.  The library is built without FMA contraction, every operation below is one rounding in the field's type T, and
 * the association is exactly as written.  On the host, in double, then rounded to T:
 *   ihx2 = 1/(hx*hx), ihy2 = 1/(hy*hy), ihz2 = 1/(hz*hz),  diag = ((2*ihx2 + 2*ihy2) + 2*ihz2) + sigma,  w = omega/diag.
 * With c = u(i,j,k):
 *   operator   nb = ((ihx2*(u(i-1,j,k) + u(i+1,j,k))) + (ihy2*(u(i,j-1,k) + u(i,j+1,k)))) + (ihz2*(u(i,j,k-1) + u(i,j,k+1)))
 *              r  = f - (diag*c - nb)
 *   Jacobi     out = c + w*r                          (out of place, every interior cell)
 *   red-black  u   = c + w*r                          (in place, the interior cells with ((i + j + k + colour_offset) & 1) == colour)
 *   sum        of (double)r * (double)r over interior cells: per thread in i order, then per workgroup, then the fixed-order
 *              pass over the workgroups' partials -- no atomics, the same bits on every run
 *   restriction (27-point full weighting; coarse (I,J,K) sits on fine (2I,2J,2K)), with  m(a, b, c) = 0.5*b + 0.25*(a + c):
 *              along k first:  p(i,j) = m(r(i,j,2K-1), r(i,j,2K), r(i,j,2K+1))   for the nine lines i = 2I-1..2I+1, j = 2J-1..2J+1
 *              then along j:   q(i)   = m(p(i,2J-1), p(i,2J), p(i,2J+1))
 *              then along i:   coarse = m(q(2I-1), q(2I), q(2I+1))                 (interior coarse cells)
 *   prolongation (trilinear, correction add), fine cell (i,j,k), I = i/2, J = j/2, K = k/2 (integer division):
 *              along k first:  a(I',J') = e(I',J',K) for even k, 0.5*(e(I',J',K) + e(I',J',K+1)) for odd k
 *              then along j:   b(I')    = a(I',J)    for even j, 0.5*(a(I',J) + a(I',J+1))       for odd j
 *              then along i:   t        = b(I)       for even i, 0.5*(b(I) + b(I+1))             for odd i
 *              u = u + t                                                           (interior fine cells)
 *   up-cast add (precision `defect`):  u64 = u64 + (double)e32                     (interior cells)
 * The residual with fp32 output evaluates r in the type of u and f and rounds it once to fp32 on the store; its sum is of the
 * unrounded r.  The norm of a field is sqrt(hx*hy*hz * sum): of r^2 over interior cells (residual norms), of f^2 over every cell
 * (mg3_dev_norm).
 *
 * The point smoothers need hx ~ hy ~ hz: with unequal spacings the convergence factor degrades (plane or line smoothers and
 * semi-coarsening are not part of this family). */
#ifndef MGHIP_3D_H
#define MGHIP_3D_H

#include "mghip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { MG3_PREC_DOUBLE = 0, MG3_PREC_SINGLE = 1, MG3_PREC_DEFECT = 2 } mg3_precision;

typedef struct mg3_config {
  int32_t nx, ny, nz;
  int32_t max_levels;        /* >= 1                                                                       */
  double x0, x1, y0, y1, z0, z1;
  double sigma;              /* >= 0                                                                       */
  double omega;              /* the weight of both smoothers (1 is plain red-black Gauss-Seidel); finite, > 0 */
  int32_t cycle;             /* MG_CYCLE_V or MG_CYCLE_W                                                   */
  int32_t pre, post;         /* >= 0, pre + post >= 1                                                      */
  int32_t smoother;          /* MG_JACOBI or MG_RBGS                                                       */
  int32_t coarse_sweeps;     /* red-black sweeps (omega = 1) on the coarsest level; <= 0: the default, 64  */
  int32_t precision;         /* mg3_precision                                                              */
  int32_t device;
  int32_t reserved;
} mg3_config;                /* 112 bytes */

typedef struct mg3_stats {
  double initial_residual, final_residual, solve_seconds;
  int64_t device_bytes;      /* what mg3_create allocated on the device for this hierarchy and precision   */
  int32_t iterations, converged, levels, reserved;
} mg3_stats;                 /* 48 bytes */

/* ------------------------------------------------------------------------------------------------
 * The engine.  HIERARCHY: a level is coarsened, (n + 1) / 2 per axis, while all three extents are odd and the coarse extents
 * are >= 3, up to max_levels levels.  The coarsest level is solved by coarse_sweeps red-black sweeps (colour 0 then 1,
 * omega = 1) from the zero iterate: in ONE single-workgroup launch with u and f in LDS when no extent exceeds 17, by the colour
 * kernel otherwise.  Coarse levels carry zero boundary faces.  A hierarchy of ONE level has no coarse level: there the sweeps
 * run in place on the caller's own iterate with its Dirichlet faces (and, for `defect`, on the fp32 correction from zero), a
 * cycle is coarse_sweeps red-black sweeps and pre, post, omega and the smoother play no part.  One cycle on level l: pre sweeps, r = f - A u, coarse f =
 * restriction of r, coarse u = 0, one (V) or two (W) cycles on level l + 1, prolongation add, post sweeps.  A red-black sweep is
 * colour 0 then colour 1 with colour_offset 0.
 *
 * PRECISION: `double` and `single` keep every level in that type (host arrays of either dtype are converted on the way).
 * `defect`: the iterate, the right-hand side and the norm are fp64; one step is  r32 = fp32(f - A u)  ->  ONE fp32 cycle for
 * A e = r32 from e = 0  ->  u = u + (double)e.
 *
 * mg3_create returns MG_ERR_INVALID_VALUE before any device work for: an extent < 3, sigma < 0 or non-finite, a non-finite or
 * empty domain, pre + post = 0 or a negative count, max_levels < 1, a non-finite or non-positive omega, an unknown cycle,
 * smoother or precision.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mg3_handle mg3_handle;

int mg3_create(const mg3_config* cfg, mg3_handle** out);
int mg3_destroy(mg3_handle* h);
const char* mg3_last_error(const mg3_handle* h);
/* host arrays (nx, ny, nz), C order, of host_dtype.  The boundary faces of the solution are the Dirichlet data; those of the
 * right-hand side are never read */
int mg3_set_rhs(mg3_handle* h, const void* f_host, int host_dtype);
int mg3_set_solution(mg3_handle* h, const void* u_host, int host_dtype);
int mg3_get_solution(mg3_handle* h, void* u_host, int host_dtype);
/* device arrays of `dtype` with pitch ld (even, >= nz), 16-byte aligned; asynchronous on the handle's stream */
int mg3_set_rhs_device(mg3_handle* h, const void* f_dev, int ld, int dtype);
int mg3_set_solution_device(mg3_handle* h, const void* u_dev, int ld, int dtype);
int mg3_get_solution_device(mg3_handle* h, void* u_dev, int ld, int dtype);
/* u := 0 everywhere, faces included */
int mg3_zero_solution(mg3_handle* h);
/* queue n cycles (defect: n outer steps) on the handle's stream; no host wait */
int mg3_cycle(mg3_handle* h, int n);
/* sqrt(hx hy hz sum r^2) over interior cells of the current iterate (fp64 for `defect`) */
int mg3_residual_norm(mg3_handle* h, double* out);
/* hist[0] = the norm of the start, hist[k] after cycle k (as far as hist_cap reaches); stops when norm < tol (absolute) or
 * after max_iter cycles.  The host reads the norm once per cycle through a pinned mapped mailbox. */
int mg3_solve(mg3_handle* h, double tol, int max_iter, double* hist, int hist_cap, int* n_iter, int* converged, mg3_stats* stats);
/* wait for everything queued on the handle's stream */
int mg3_synchronize(mg3_handle* h);
int mg3_stream(mg3_handle* h, void** stream);
int mg3_num_levels(const mg3_handle* h, int* levels);
/* the device bytes mg3_create would allocate for cfg (the same refusals), without a device */
int mg3_device_bytes(const mg3_config* cfg, int64_t* bytes);

/* ------------------------------------------------------------------------------------------------
 * Stateless device forms, call by call: asynchronous on `stream` (nullable), any nx, ny, nz >= 3 and any even pitch >= nz.
 * MG_ERR_INVALID_VALUE before any device work: an extent < 3, an odd or too-small pitch, a NULL or misaligned pointer, an
 * unknown dtype, sigma < 0, non-finite or non-positive spacings, non-finite sigma or omega.
 * scratch >= mg3_dev_scratch_bytes(nx, ny, nz) bytes, 16-byte aligned (only read when a sum is asked for).
 * ------------------------------------------------------------------------------------------------ */
int mg3_dev_scratch_bytes(int nx, int ny, int nz, int64_t* bytes);
/* r = f - A u on interior cells (r NULL: not stored); u and f of `dtype` with pitch ld, r of r_dtype with pitch ld_r (fp32 from
 * fp64 is the defect step's; fp64 from fp32 is refused); sumsq_dev_or_null := sum r^2 */
int mg3_dev_residual(int dtype, int r_dtype, int nx, int ny, int nz, int ld, int ld_r, double hx, double hy, double hz, double sigma,
                     const void* u, const void* f, void* r_or_null, void* scratch, double* sumsq_dev_or_null, void* stream);
int mg3_dev_jacobi(int dtype, int nx, int ny, int nz, int ld, double hx, double hy, double hz, double sigma, double omega,
                   const void* u, const void* f, void* out, void* stream);
int mg3_dev_rbgs_colour(int dtype, int nx, int ny, int nz, int ld, double hx, double hy, double hz, double sigma, double omega,
                        int colour, int colour_offset, void* u, const void* f, void* stream);
/* fine (nxf, nyf, nzf), all odd and >= 5 -> coarse ((nxf+1)/2, ...): interior coarse cells */
int mg3_dev_restrict(int dtype, int nxf, int nyf, int nzf, int ldf, int ldc, const void* fine, void* coarse, void* stream);
/* u += P e on interior fine cells; the fine extents are 2 * coarse - 1 */
int mg3_dev_prolong_add(int dtype, int nxf, int nyf, int nzf, int ldf, int ldc, const void* e_coarse, void* u_fine, void* stream);
/* u64 += (double)e32 on interior cells */
int mg3_dev_upcast_add(int nx, int ny, int nz, int ld64, int ld32, const float* e32, double* u64, void* stream);
/* sumsq_dev := the sum of field^2 over [0,nx) x [0,ny) x [0,nz) */
int mg3_dev_norm(int dtype, int nx, int ny, int nz, int ld, const void* field, void* scratch, double* sumsq_dev, void* stream);
/* `sweeps` red-black sweeps (colour 0 then 1, colour_offset 0, omega = 1) in place on u: one single-workgroup launch in LDS when
 * no extent exceeds 17, else 2 * sweeps launches of the colour kernel.  *used_lds_or_null := which */
int mg3_dev_coarse_solve(int dtype, int nx, int ny, int nz, int ld, double hx, double hy, double hz, double sigma, int sweeps,
                         void* u, const void* f, int* used_lds_or_null, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGHIP_3D_H */
