// The kernel launchers of libmghip.so (mg_launch.hip, the one unit that instantiates the kernel templates): non-template
// functions over dtype codes, pointers and sizes, which the other units compile against as host code.
#pragma once

#include "mg_host.hpp"

namespace mgh {

// Row pitch in elements: rows start on 512-byte boundaries (every tile row segment is line aligned).
int pitch_elems(int dt, int ny);
// Upper bound of the per-workgroup partial sums any norm launch on an (nx, ny) field writes.
size_t max_partials(int nx, int ny);

void d_jacobi(int dt, const void* u, const void* rhs, void* out, int nx, int ny, int ld, double hx, double hy,
              double omega, hipStream_t st, bool fine = false, double sigma = 0.0);
void d_rbgs_colour(int dt, void* u, const void* rhs, int nx, int ny, int ld, double hx, double hy, double omega,
                   int colour, int poff, hipStream_t st, bool fine = false, double sigma = 0.0);
void d_residual(int dt, const void* u, const void* f, void* r, int nx, int ny, int ld, double hx, double hy,
                double coeff, hipStream_t st, bool fine = false, double sigma = 0.0);
// an int result is the number of norm partials written, unless said otherwise
int d_residual_norm(int dt, const void* u, const void* f, double* partials, int nx, int ny, int ld, double hx,
                    double hy, double coeff, hipStream_t st, bool fine = false, double sigma = 0.0);
int d_sumsq(int dt, const void* x, double* partials, int ld, int i_lo, int i_hi, int j_lo, int j_hi, hipStream_t st);
void launch_reduce(const double* partials, int n, double* out, hipStream_t st, mg::HostMailbox* mailbox = nullptr,
                   unsigned long long seq = 0);
void d_restrict_sub(int di, int dout, const void* fine, void* coarse, int ldf, int nxc, int nyc, int ldc, int sides,
                    hipStream_t st);
// whole-grid form: coarse dims follow from the fine ones and all four edges are physical boundaries
void d_restrict(int di, int dout, const void* fine, void* coarse, int nxf, int nyf, int ldf, int ldc, hipStream_t st);
// dc: dtype of the coarse field, df: of the fine field, dcomp: interpolation arithmetic (the fine GRID's dtype); add: u += P e,
// else u = P e.  Returns MG_OK, or MG_ERR_INVALID_VALUE for fp32 interpolation between fields that are not both fp32.
int d_prolong_sub(bool add, int dc, int df, int dcomp, const void* e, void* u, int nxf, int nyf, int ldf, int nxc, int nyc,
                  int ldc, int sides, hipStream_t st);
int d_prolong(bool add, int dc, int df, int dcomp, const void* e, void* u, int nxf, int nyf, int ldf, int ldc, hipStream_t st);
void d_convert(int di, int dout, const void* in, void* out, int nx, int ny, int ldi, int ldo, hipStream_t st);
// boundary ring of `in` -> boundary ring of `out` (the interior of `out` is left alone)
void d_convert_ring(int di, int dout, const void* in, void* out, int nx, int ny, int ldi, int ldo, hipStream_t st);
void d_zero_interior(int dt, void* u, int nx, int ny, int ld, hipStream_t st);
void d_coarse(int dt, void* u, const void* rhs, int nx, int ny, int ld, double hx, double hy, double coeff,
              double omega, double tol, int maxit, int* sweeps_dev, hipStream_t st, bool zero_init = false,
              const void* a = nullptr, double sigma = 0.0);
// variable coefficient: mode is mg::kVarJacobi / kVarRbgs / kVarResidual (any other: no launch); the residual's norm has a
// launcher of its own
void d_var(int mode, int dt, const void* u, const void* a, const void* f, void* out, int nx, int ny, int ld, double hx, double hy,
           double omega, double coeff, int colour, int poff, hipStream_t st, double sigma = 0.0);
int d_var_residual_norm(int dt, const void* u, const void* a, const void* f, double* partials, int nx, int ny, int ld, double hx,
                        double hy, double coeff, hipStream_t st, double sigma);
void d_inject(int di, int dout, const void* fine, void* coarse, int ldf, int nxc, int nyc, int ldc, int stride, hipStream_t st);
void d_rdiag(int dt, const void* a, void* rd, int nx, int ny, int ld, double hx, double hy, double sigma, hipStream_t st);
void d_inject_ring(int di, int dout, const void* fine, void* coarse, int nxf, int nyf, int ldf, int nxc, int nyc, int ldc,
                   hipStream_t st, int sides = mg::kAllSides, int ci_off = 0, int cj_off = 0);

struct LegGeom {      // what every fused launch needs
  int nx = 0, ny = 0, ld = 0, nxc = 0, nyc = 0, ldc = 0;
  double hx = 0, hy = 0, omega = 0, coeff = 0;
  int nsweep = 0, poff = 0;
  bool fine = false;
  // sub-domain extras (defaults = whole grid)
  int ci_off = 0, cj_off = 0, sides = mg::kAllSides;
  int ni_lo = -1, ni_hi = -1, nj_lo = -1, nj_hi = -1;     // norm window; -1: the interior
  int select = 0, in_i_lo = 0, in_i_hi = 0, in_j_lo = 0, in_j_hi = 0;   // tile selection (see mg::FusedArgs)
  double sigma = 0.0;                                                    // Helmholtz shift (see coefs)
  const void* acoef = nullptr;                                           // variable coefficient: vertex values (dtype / pitch of u)
  const void* rdiag = nullptr;                                           // ... and its reciprocal diagonal per cell (var_rdiag_kernel)
  int rb = 0;                                                            // 1: register-blocked legs on the bandwidth-bound levels
};
// g.rb: 0 never, 1 on levels above ~1100^2 cells (where a launch is bandwidth-bound), 2 on every level (tests)
bool use_rb(const LegGeom& g);

// The fused legs.  dt: dtype of the level, dx: of the coarse rhs (down) / correction (up), dcomp: interpolation dtype.
// d_up and d_span return -1 for an unsupported precision combination.
int d_span(int dt, int dcomp, const void* u, const void* rhs, void* out_mid, void* out_next, const void* e_c, void* rhs_c,
           double* partials, const LegGeom& g, int nsweep_pre, hipStream_t st, int sm = MG_JACOBI);
void d_down(int sm, int dt, int dx, const void* u, const void* rhs, void* out, void* rhs_c, const LegGeom& g, bool zero_init,
            hipStream_t st);
int d_up(int sm, int dt, int dx, int dcomp, const void* u, const void* rhs, void* out, const void* e_c, double* partials,
         const LegGeom& g, bool norm, hipStream_t st);
void d_sweeps(int sm, int dt, const void* u, const void* rhs, void* out, const LegGeom& g, hipStream_t st);

// The one-workgroup LDS tail (levels h->tail_start .. L-1).  tail_pool_bytes: its LDS pool for levels k .. L-1 with esz-byte
// upper levels and an esz_last-byte coarsest one; tail_set_attrs raises the dynamic LDS limit of every tail kernel.
constexpr size_t kTailPoolLimit = 150 * 1024;
size_t tail_pool_bytes(const mg_handle* h, int k, size_t esz, size_t esz_last);
int tail_set_attrs(size_t bytes);
void launch_tail(mg_handle* h, bool zero_top);

int launch_defect(mg_handle* h, bool update);
void d_stream_triad(int dt, const void* a, const void* b, void* out, int nx, int ny, int ld, hipStream_t st);
void d_residual_f32in_f64out(const float* u, const float* f, double* r, int nx, int ny, int ld_in, int ld_out, double hx,
                             double hy, double coeff, hipStream_t st);

}  // namespace mgh
