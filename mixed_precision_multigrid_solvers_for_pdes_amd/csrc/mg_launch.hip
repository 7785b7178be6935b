// The kernel-launch unit of libmghip.so: every launch of a mg:: kernel (mg_kernels.hpp, mg_rb_kernels.hpp), and with them
// every template instantiation, behind the non-template functions of mg_launch.hpp.
#include "mg_launch.hpp"
#include "mg_rb_kernels.hpp"

#include <cstring>

namespace mgh {

int pitch_elems(int dt, int ny) {
  const size_t bytes = ((size_t)ny * esize(dt) + 511) / 512 * 512;
  return (int)(bytes / esize(dt));
}

template <typename T>
mg::TileGeom make_geom(int nx, int ny, int ld, bool interior_only) {
  using S = mg::TileShape<T>;
  mg::TileGeom g;
  g.nx = nx; g.ny = ny; g.ld = ld;
  g.nyv = std::min(ld, (ny + S::N - 1) / S::N * S::N);
  g.i_org = interior_only ? 1 : 0;
  const int rows = interior_only ? nx - 2 : nx;
  const int cols = interior_only ? ny - 1 : ny;     // column ny-1 is boundary: never written by a smoother
  const int tiles_i = (rows + mg::kTI - 1) / mg::kTI;
  g.tiles_j = (cols + S::TJ - 1) / S::TJ;
  g.ntiles = tiles_i * g.tiles_j;
  return g;
}

// the grid-stride reductions use <= 2048 workgroups, the residual+norm kernel one per kTI-row tile, the fused up leg one per tile of
// its own (shorter) tile height; fp64 tiles are the narrowest (64 columns).
size_t max_partials(int nx, int ny) {
  const long long tj = (ny + 63) / 64 + 1;
  const int ti_min = std::min(mg::kTI, std::min(mg::kFusedTI, std::min(mg::kFusedTISmall, mg::kFusedTITiny)));
  const long long ti = (nx + ti_min - 1) / ti_min + 1;
  return (size_t)std::max<long long>(2048, ti * tj);
}

static int grid_for(long long work_items) {
  long long b = (work_items + mg::kBlock - 1) / mg::kBlock;
  return (int)std::max<long long>(1, std::min<long long>(b, 256 * 16));
}
// ------------------------------------------------------------------ typed launchers ------------
bool use_rb(const LegGeom& g) { return g.rb == 2 || (g.rb == 1 && (long long)g.nx * g.ny > 1100LL * 1100LL); }

// Arrays of more than ~100 MB cannot stay in the 256 MiB Infinity Cache from one leg to the next (u, t and rhs compete):
// their legs run with streaming hints (rb_leg_kernel TAG 2).  MG_RB_NT=0/1 overrides (experiments).
static bool rb_stream(const LegGeom& g, size_t esz) {
  static const int force = exp_env("MG_RB_NT", -1);
  if (force >= 0) return force != 0;
  return (size_t)g.nx * g.ld * esz > (size_t)100 << 20;
}

// One weighted-Jacobi sweep on a level above ~1100^2 cells: the register-blocked sweeps kernel with nsweep = 1 (same
// arithmetic, same ping-pong contract as jacobi_kernel: interior rows written, the ring of `out` already equals u's).
// MG_JACOBI_RB=0 keeps the LDS-tiled jacobi_kernel (A/B runs).
static bool jacobi_rb(int dt, const void* u, const void* rhs, void* out, int nx, int ny, int ld, double hx, double hy, double omega,
               hipStream_t st, double sigma) {
  static const int on = exp_env("MG_JACOBI_RB", 1);
  LegGeom g;
  g.nx = nx; g.ny = ny; g.ld = ld; g.hx = hx; g.hy = hy; g.omega = omega; g.nsweep = 1; g.fine = true;
  g.sigma = sigma; g.rb = 1;
  // only where the arrays stream from HBM (4097^2 fp64: 81 -> 78 us); Infinity-Cache-resident sweeps are faster LDS-tiled
  if (!on || !use_rb(g) || !rb_stream(g, esize(dt))) return false;
  d_sweeps(MG_JACOBI, dt, u, rhs, out, g, st);
  return true;
}

void d_jacobi(int dt, const void* u, const void* rhs, void* out, int nx, int ny, int ld, double hx, double hy,
              double omega, hipStream_t st, bool fine, double sigma) {
  if (jacobi_rb(dt, u, rhs, out, nx, ny, ld, hx, hy, omega, st, sigma) || nx < 3 || ny < 3) return;
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    const Coef c = coefs(hx, hy, sigma);
    const mg::TileGeom g = make_geom<T>(nx, ny, ld, true);
    auto k = c.pow2 ? (fine ? mg::jacobi_kernel<T, mg::kFineTag, false> : mg::jacobi_kernel<T, mg::kCoarseTag, false>)
                    : (fine ? mg::jacobi_kernel<T, mg::kFineTag, true> : mg::jacobi_kernel<T, mg::kCoarseTag, true>);
    hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, (const T*)u, (const T*)rhs, (T*)out,
                       g, (T)c.ihx2, (T)c.ihy2, (T)c.invD, (T)c.diag, (T)omega, (T)(1.0 - omega));
  });
}
void d_rbgs_colour(int dt, void* u, const void* rhs, int nx, int ny, int ld, double hx, double hy, double omega,
                   int colour, int poff, hipStream_t st, bool fine, double sigma) {
  if (nx < 3 || ny < 3) return;
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    const Coef c = coefs(hx, hy, sigma);
    const mg::TileGeom g = make_geom<T>(nx, ny, ld, true);
    auto k = c.pow2 ? (fine ? mg::rbgs_colour_kernel<T, mg::kFineTag, false> : mg::rbgs_colour_kernel<T, mg::kCoarseTag, false>)
                    : (fine ? mg::rbgs_colour_kernel<T, mg::kFineTag, true> : mg::rbgs_colour_kernel<T, mg::kCoarseTag, true>);
    hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, (T*)u, (const T*)rhs, g,
                       (T)c.ihx2, (T)c.ihy2, (T)c.invD, (T)c.diag, (T)omega, (T)(1.0 - omega), colour, poff & 1);
  });
}

// returns the number of partials written (0 when NORM is off)
template <bool WRITE_R, bool NORM>
int launch_residual(int dt, const void* u, const void* f, void* r, double* partials, int nx, int ny, int ld, double hx,
                    double hy, double coeff, hipStream_t st, bool fine, double sigma) {
  return with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    const Coef c = coefs(hx, hy, sigma);
    const mg::TileGeom g = make_geom<T>(nx, ny, ld, false);
    auto k = fine ? mg::residual_kernel<T, WRITE_R, NORM, mg::kFineTag> : mg::residual_kernel<T, WRITE_R, NORM, mg::kCoarseTag>;
    hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, (const T*)u,
                       (const T*)f, (T*)r, partials, g, (T)c.ihx2, (T)c.ihy2, (T)c.diag, (T)coeff);
    return NORM ? g.ntiles : 0;
  });
}
void d_residual(int dt, const void* u, const void* f, void* r, int nx, int ny, int ld, double hx, double hy,
                double coeff, hipStream_t st, bool fine, double sigma) {
  launch_residual<true, false>(dt, u, f, r, nullptr, nx, ny, ld, hx, hy, coeff, st, fine, sigma);
}
int d_residual_norm(int dt, const void* u, const void* f, double* partials, int nx, int ny, int ld, double hx,
                    double hy, double coeff, hipStream_t st, bool fine, double sigma) {
  return launch_residual<false, true>(dt, u, f, nullptr, partials, nx, ny, ld, hx, hy, coeff, st, fine, sigma);
}
int d_sumsq(int dt, const void* x, double* partials, int ld, int i_lo, int i_hi, int j_lo, int j_hi, hipStream_t st) {
  return with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    const int N = mg::VecW<T>::N;
    const long long vecs = (long long)std::max(0, i_hi - i_lo) * ((j_hi + N - 1) / N - j_lo / N);
    const int nb = std::min(grid_for(vecs), 2048);
    hipLaunchKernelGGL(mg::sumsq_kernel<T>, dim3(nb), dim3(mg::kBlock), 0, st, (const T*)x, partials, ld, i_lo, i_hi, j_lo,
                       j_hi);
    return nb;
  });
}

void launch_reduce(const double* partials, int n, double* out, hipStream_t st, mg::HostMailbox* mailbox, unsigned long long seq) {
  hipLaunchKernelGGL(mg::reduce_partials_kernel<0>, dim3(1), dim3(mg::kReduceBlock), 0, st, partials, n, out, mailbox, seq);
}

void d_restrict_sub(int di, int dout, const void* fine, void* coarse, int ldf, int nxc, int nyc, int ldc, int sides,
                    hipStream_t st) {
  with_dtype(di, dout, [&](auto ti, auto to) {
    using TI = decltype(ti); using TO = decltype(to);
    const int NO = mg::VecW<TO>::N;
    hipLaunchKernelGGL((mg::restrict_fw_kernel<TI, TO>), dim3(grid_for((long long)nxc * ((nyc + NO - 1) / NO))),
                       dim3(mg::kBlock), 0, st, (const TI*)fine, (TO*)coarse, ldf, nxc, nyc, ldc, sides);
  });
}
void d_restrict(int di, int dout, const void* fine, void* coarse, int nxf, int nyf, int ldf, int ldc, hipStream_t st) {
  d_restrict_sub(di, dout, fine, coarse, ldf, (nxf - 1) / 2 + 1, (nyf - 1) / 2 + 1, ldc, mg::kAllSides, st);
}
template <bool ADD>
int launch_prolong(int dc, int df, int dcomp, const void* e, void* u, int nxf, int nyf, int ldf, int nxc, int nyc, int ldc,
                  int sides, hipStream_t st) {
  return with_dtype(dc, df, dcomp, [&](auto tci, auto tf, auto tc) {
    using TCI = decltype(tci); using TF = decltype(tf); using TC = decltype(tc);
    if constexpr (!interp_ok<TF, TCI, TC>) return MG_ERR_INVALID_VALUE;
    else {
      const int N = mg::VecW<TF>::N;
      hipLaunchKernelGGL((mg::prolong_kernel<TCI, TF, TC, ADD>), dim3(grid_for((long long)nxf * ((nyf + N - 1) / N))),
                         dim3(mg::kBlock), 0, st, (const TCI*)e, (TF*)u, nxf, nyf, ldf, nxc, nyc, ldc, sides);
      return MG_OK;
    }
  });
}
void d_convert(int di, int dout, const void* in, void* out, int nx, int ny, int ldi, int ldo, hipStream_t st) {
  with_dtype(di, dout, [&](auto ti, auto to) {
    using TI = decltype(ti); using TO = decltype(to);
    hipLaunchKernelGGL((mg::convert_kernel<TI, TO>), dim3(grid_for((long long)nx * ny)), dim3(mg::kBlock), 0, st,
                       (const TI*)in, (TO*)out, nx, ny, ldi, ldo);
  });
}
void d_convert_ring(int di, int dout, const void* in, void* out, int nx, int ny, int ldi, int ldo, hipStream_t st) {
  with_dtype(di, dout, [&](auto ti, auto to) {
    using TI = decltype(ti); using TO = decltype(to);
    hipLaunchKernelGGL((mg::convert_ring_kernel<TI, TO>), dim3(grid_for(2LL * nx + 2LL * ny)), dim3(mg::kBlock), 0, st,
                       (const TI*)in, (TO*)out, nx, ny, ldi, ldo);
  });
}
void d_zero_interior(int dt, void* u, int nx, int ny, int ld, hipStream_t st) {
  if (nx < 3 || ny < 3) return;
  const long long vecs = (long long)(nx - 2) * ((ny + (int)(16 / esize(dt)) - 1) / (int)(16 / esize(dt)));
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mg::zero_interior_kernel<T>, dim3(grid_for(vecs)), dim3(mg::kBlock), 0, st, (T*)u, nx, ny, ld);
  });
}
void d_coarse(int dt, void* u, const void* rhs, int nx, int ny, int ld, double hx, double hy, double coeff,
              double omega, double tol, int maxit, int* sweeps_dev, hipStream_t st, bool zero_init,
              const void* a, double sigma) {
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    const Coef c = coefs(hx, hy, sigma);
    if (a) {          // variable coefficient: the general one-workgroup kernel
      if (zero_init) (void)hipMemsetAsync(u, 0, (size_t)nx * ld * sizeof(T), st);
      hipLaunchKernelGGL(mg::coarse_lexgs_kernel<T>, dim3(1), dim3(mg::kBlock), 0, st, (T*)u, (const T*)rhs, nx, ny, ld,
                         (T)(hx * hx), (T)(hy * hy), (T)omega, (T)(1.0 - omega), (T)c.diag, (T)coeff, hx * hy, tol, maxit,
                         sweeps_dev, (const T*)a, (T)sigma);
      return;
    }
    if (nx * ny <= mg::kCoarseLdsCells) {
      hipLaunchKernelGGL(mg::coarse_lexgs_small_kernel<T>, dim3(1), dim3(64), 0, st, (T*)u, (const T*)rhs, nx, ny, ld,
                         (T)(hx * hx), (T)(hy * hy), (T)omega, (T)(1.0 - omega), (T)c.diag, (T)coeff, hx * hy, tol, maxit,
                         sweeps_dev, zero_init ? 1 : 0, c.all_pow2 ? 1 : 0, sqrt_threshold(tol));
      return;
    }
    if (zero_init) (void)hipMemsetAsync(u, 0, (size_t)nx * ld * sizeof(T), st);
    hipLaunchKernelGGL(mg::coarse_lexgs_kernel<T>, dim3(1), dim3(mg::kBlock), 0, st, (T*)u, (const T*)rhs, nx, ny, ld,
                       (T)(hx * hx), (T)(hy * hy), (T)omega, (T)(1.0 - omega), (T)c.diag, (T)coeff, hx * hy, tol,
                       maxit, sweeps_dev, (const T*)nullptr);
  });
}

// ------------------------------------------------------------------ variable coefficient ------
template <int MODE>
int launch_var(int dt, const void* u, const void* a, const void* f, void* out, double* partials, int nx, int ny, int ld, double hx,
               double hy, double omega, double coeff, int colour, int poff, hipStream_t st, double sigma) {
  if (nx < 3 || ny < 3) return 0;
  return with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    const Coef c = coefs(hx, hy);
    const bool interior_only = (MODE == mg::kVarJacobi || MODE == mg::kVarRbgs);
    const mg::TileGeom g = make_geom<T>(nx, ny, ld, interior_only);
    hipLaunchKernelGGL((mg::varcoef_kernel<T, MODE>), dim3(g.ntiles), dim3(mg::kBlock), 0, st, (const T*)u, (const T*)a,
                       (const T*)f, (T*)out, partials, g, (T)c.ihx2, (T)c.ihy2, (T)omega, (T)(1.0 - omega), (T)coeff, colour,
                       poff & 1, (T)sigma);
    return g.ntiles;
  });
}
void d_inject(int di, int dout, const void* fine, void* coarse, int ldf, int nxc, int nyc, int ldc, int stride, hipStream_t st) {
  with_dtype(di, dout, [&](auto ti, auto to) {
    using TI = decltype(ti); using TO = decltype(to);
    hipLaunchKernelGGL((mg::inject_kernel<TI, TO>), dim3(grid_for((long long)nxc * nyc)), dim3(mg::kBlock), 0, st,
                       (const TI*)fine, (TO*)coarse, ldf, nxc, nyc, ldc, stride);
  });
}
void d_rdiag(int dt, const void* a, void* rd, int nx, int ny, int ld, double hx, double hy, double sigma, hipStream_t st) {
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    const Coef c = coefs(hx, hy);
    hipLaunchKernelGGL(mg::var_rdiag_kernel<T>, dim3(grid_for((long long)nx * ny)), dim3(mg::kBlock), 0, st, (const T*)a, (T*)rd, nx, ny, ld,
                       (T)c.ihx2, (T)c.ihy2, (T)sigma);
  });
}

// ------------------------------------------------------------------ fused legs ----------------
// the launch arguments of a leg whose tiles are TI rows high (the register-blocked legs re-tile them: rb_args)
template <typename T, int HALO, int TI>
mg::FusedArgs fused_args(const LegGeom& g, bool use_div) {
  using S = mg::FusedShape<T, HALO, TI>;
  mg::FusedArgs a;
  a.nx = g.nx; a.ny = g.ny; a.ld = g.ld;
  a.nyv = std::min(g.ld, (g.ny + S::N - 1) / S::N * S::N);
  const int tiles_i = (g.nx - 2 + TI - 1) / TI;
  a.tiles_j = (g.ny - 1 + S::TJ - 1) / S::TJ;
  a.ntiles = tiles_i * a.tiles_j;
  a.nsweep = g.nsweep; a.nsweep2 = 0; a.band = 1; a.use_div = use_div ? 1 : 0; a.colour_offset = g.poff & 1;
  a.pow2 = 0; a.neg_coeff_a = 0.0;
  a.nxc = g.nxc; a.nyc = g.nyc; a.ldc = g.ldc;
  a.ci_off = g.ci_off; a.cj_off = g.cj_off; a.sides = g.sides;
  a.ni_lo = 1; a.ni_hi = g.nx - 1; a.nj_lo = 1; a.nj_hi = g.ny - 1;
  if (g.ni_lo >= 0) { a.ni_lo = g.ni_lo; a.ni_hi = g.ni_hi; a.nj_lo = g.nj_lo; a.nj_hi = g.nj_hi; }
  a.select = g.select; a.in_i_lo = g.in_i_lo; a.in_i_hi = g.in_i_hi; a.in_j_lo = g.in_j_lo; a.in_j_hi = g.in_j_hi;
  static const int flags = exp_env("MG_EXP_FLAGS", 0);          // measurement builds only (mg_host.hpp: exp_env)
  a.exp_flags = flags;
  return a;
}

// Tile height by level size: 32 rows where the launch is bandwidth-bound, 16 where it is latency-bound (<= ~1025^2).
// Variable-coefficient red-black GS keeps 6 halo cells and the face means of every owned cell in registers: with 32-row
// tiles that is 176 VGPRs (one workgroup per CU); 16-row tiles stay at 100 (two).
inline bool small_tiles(const LegGeom& g, int sm = mg::kSmJacobi) {
  return (long long)g.nx * g.ny <= 1100LL * 1100LL || (g.acoef && sm == mg::kSmRbgs);
}
// 8-row tiles: legs on levels of <= ~520^2 cells (513^2 and below) (MG_EXP_TINY=n: up to n^2 cells, 0 keeps the 16-row tiles: experiments)
inline bool tiny_tiles(const LegGeom& g) {
  static const long long lim = exp_env("MG_EXP_TINY", 520);   // 0: off
  return lim > 0 && (long long)g.nx * g.ny <= lim * lim;
}

// ---- register-blocked legs (mg_rb_kernels.hpp): constant coefficients, levels above ~1100^2 cells ------------------
template <typename T, int HALO, int W, int RPT>
mg::FusedArgs rb_args(const LegGeom& g, bool use_div) {
  using S = mg::RbShape<T, HALO, W, RPT>;
  mg::FusedArgs a = fused_args<T, HALO, mg::kFusedTI>(g, use_div);
  const int tiles_i = (g.nx - 2 + S::TI - 1) / S::TI;
  a.tiles_j = (g.ny - 1 + S::TJ - 1) / S::TJ;
  a.ntiles = tiles_i * a.tiles_j;
  return a;
}
// kernel variant by streaming hints (TAG 2) -- VAR is a template argument of the launcher so that only the shapes in use
// are instantiated: constant coefficients 4 waves x 8 rows (fp64 red-black GS, whose halo is 6 rows: 8 x 8, a 64-row
// region of which 52 rows are tile instead of 20 of 32 -- down / up leg 95 / 98 -> 91 / 91 us at 4097^2; the other three
// lose 3-30 % with it), variable coefficients 8 waves x 4 rows (a 32-row region; the face means of 4 rows per lane keep
// the kernel at ~125 VGPRs instead of 256; 16 x 4 measured 192 / 194 us against 165 / 180)
// measurement builds (-DMG_EXPERIMENTS -DMG_EXP_VAR_W=16 / -DMG_EXP_RB_W=8): other workgroup shapes of the same kernels
#if !defined(MG_EXPERIMENTS) && (defined(MG_EXP_VAR_W) || defined(MG_EXP_RB_W))
#error "MG_EXP_* switches need -DMG_EXPERIMENTS (a measurement build, never the shipped library)"
#endif
#ifndef MG_EXP_VAR_W
#define MG_EXP_VAR_W 8
#endif
#ifndef MG_EXP_RB_W
#define MG_EXP_RB_W ((SM == mg::kSmRbgs && sizeof(T) == 8) ? 8 : 4)
#endif

// The four legs: down (nsweep sweeps + residual + full-weighting restriction to the interior coarse cells, into TX),
// up with or without the norm (u += P e from TX with TC arithmetic, nsweep sweeps [, sum of r^2 over interior cells]), and
// plain sweeps (nsweep <= 2 per launch).
enum LegKind { kLegDown, kLegUpNorm, kLegUp, kLegSweeps };
enum LegFamily { kLdsTiled, kRegBlocked };

// One leg launch.  LDS-tiled: TI-row tiles, kernel by coefficient and level (variable coefficients: one symbol for all
// levels, TAG 0).  Register-blocked: W waves x RPT rows, kernel by streaming hints.  coarse: the coarse rhs (down leg) or
// the coarse correction (up legs).  Returns the number of norm partials (0 without the norm).
template <int LEG, int FAM, typename T, typename TX, typename TC, int SM, int TI, int W = 0, int RPT = 0, bool VAR = false>
int launch_leg(const void* u, const void* rhs, void* out, const void* coarse, double* partials, const LegGeom& g, bool zero_init,
               hipStream_t st) {
  constexpr bool PROLONG = LEG == kLegUpNorm || LEG == kLegUp;
  constexpr int POST = LEG == kLegDown ? mg::kPostRestrict : LEG == kLegUpNorm ? mg::kPostNorm : mg::kPostNone;
  constexpr int HALO = 2 * mg::sweep_halo(SM) + (LEG == kLegDown ? 2 : LEG == kLegUpNorm ? 1 : 0);
  const Coef c = coefs(g.hx, g.hy, g.sigma);
  mg::FusedArgs a;
  const double coeff = LEG == kLegSweeps ? 0.0 : g.coeff;
  if constexpr (FAM == kRegBlocked) {
    a = rb_args<T, HALO, W, RPT>(g, !c.pow2);
    if (pow2_stencil(c, sizeof(T) == 8, g.acoef, g.sigma, coeff)) { a.pow2 = 1; a.neg_coeff_a = -(coeff * c.ihx2); }
  } else a = fused_args<T, HALO, TI>(g, !c.pow2);
  const bool nt = FAM == kRegBlocked && rb_stream(g, sizeof(T));
  auto pick = [&](auto zero) {
    constexpr bool Z = decltype(zero)::value;
    if constexpr (FAM == kRegBlocked) {
      return nt ? mg::rb_leg_kernel<T, HALO, PROLONG, POST, Z, TX, TC, 2, SM, W, RPT, VAR>
                : mg::rb_leg_kernel<T, HALO, PROLONG, POST, Z, TX, TC, 1, SM, W, RPT, VAR>;
    } else {
      return g.acoef ? mg::fused_jacobi_kernel<T, HALO, PROLONG, POST, Z, TX, TC, 0, SM, TI, true>
           : g.fine ? mg::fused_jacobi_kernel<T, HALO, PROLONG, POST, Z, TX, TC, 1, SM, TI>
                    : mg::fused_jacobi_kernel<T, HALO, PROLONG, POST, Z, TX, TC, 0, SM, TI>;
    }
  };
  auto k = pick(std::false_type());
  if constexpr (LEG == kLegDown) if (zero_init) k = pick(std::true_type());
  hipLaunchKernelGGL(k, dim3(a.ntiles), dim3(FAM == kRegBlocked ? W * 64 : mg::kFusedBlock), 0, st, (const T*)u, (const T*)rhs,
                     (T*)out, PROLONG ? (const TX*)coarse : nullptr, POST == mg::kPostRestrict ? (TX*)coarse : nullptr,
                     POST == mg::kPostNorm ? partials : nullptr, a, (T)c.ihx2, (T)c.ihy2, (T)c.invD, (T)c.diag, (T)g.omega,
                     (T)(1.0 - g.omega), (T)coeff, (const T*)g.acoef, (T)g.sigma, (const T*)g.rdiag);
  return POST == mg::kPostNorm ? a.ntiles : 0;
}
// the family and shape of a leg by level size
template <int LEG, typename T, typename TX, typename TC, int SM>
int launch_leg_sized(const void* u, const void* rhs, void* out, const void* coarse, double* partials, const LegGeom& g,
                     bool zero_init, hipStream_t st) {
  if (use_rb(g))
    return g.acoef ? launch_leg<LEG, kRegBlocked, T, TX, TC, SM, 0, MG_EXP_VAR_W, 4, true>(u, rhs, out, coarse, partials, g, zero_init, st)
                   : launch_leg<LEG, kRegBlocked, T, TX, TC, SM, 0, MG_EXP_RB_W, 8, false>(u, rhs, out, coarse, partials, g, zero_init, st);
  if (tiny_tiles(g)) return launch_leg<LEG, kLdsTiled, T, TX, TC, SM, mg::kFusedTITiny>(u, rhs, out, coarse, partials, g, zero_init, st);
  if (small_tiles(g, SM)) return launch_leg<LEG, kLdsTiled, T, TX, TC, SM, mg::kFusedTISmall>(u, rhs, out, coarse, partials, g, zero_init, st);
  return launch_leg<LEG, kLdsTiled, T, TX, TC, SM, mg::kFusedTI>(u, rhs, out, coarse, partials, g, zero_init, st);
}

// Spanning leg (rb_span_kernel): 8 waves x 8 rows -- the halo of two sweep sets + residual + restriction is 6 rows
// (Jacobi), 52 of the region's 64 rows are tile.  Returns the number of norm partials.
template <typename T, typename TX, typename TC, int SM>
int launch_span_rb(const void* u, const void* rhs, void* out_mid, void* out_next, const void* e_c, void* rhs_c, double* partials,
                   const LegGeom& g, int nsweep_pre, hipStream_t st) {
  constexpr int W = 8, RPT = 8;
  constexpr int HALO = 4 * mg::sweep_halo(SM) + 2;
  const Coef c = coefs(g.hx, g.hy, g.sigma);
  mg::FusedArgs a = rb_args<T, HALO, W, RPT>(g, !c.pow2);
  a.nsweep2 = nsweep_pre;
  if (pow2_stencil(c, sizeof(T) == 8, g.acoef, g.sigma, g.coeff)) { a.pow2 = 1; a.neg_coeff_a = -(g.coeff * c.ihx2); }
  static const int band = std::max(1, exp_env("MG_EXP_SPAN_BAND", 4));      // measurement builds: other band heights
  a.band = band;
  const bool nt = rb_stream(g, sizeof(T));
  auto k = out_mid ? (nt ? mg::rb_span_kernel<T, HALO, TX, TC, 2, SM, W, RPT, 1> : mg::rb_span_kernel<T, HALO, TX, TC, 1, SM, W, RPT, 1>)
                   : (nt ? mg::rb_span_kernel<T, HALO, TX, TC, 2, SM, W, RPT, 2> : mg::rb_span_kernel<T, HALO, TX, TC, 1, SM, W, RPT, 2>);
  hipLaunchKernelGGL(k, dim3(a.ntiles), dim3(W * 64), 0, st, (const T*)u, (const T*)rhs, (T*)out_mid, (T*)out_next, (const TX*)e_c,
                     (TX*)rhs_c, partials, a, (T)c.ihx2, (T)c.ihy2, (T)c.invD, (T)c.diag, (T)g.omega, (T)(1.0 - g.omega), (T)g.coeff);
  return a.ntiles;
}
int d_span(int dt, int dcomp, const void* u, const void* rhs, void* out_mid, void* out_next, const void* e_c, void* rhs_c,
           double* partials, const LegGeom& g, int nsweep_pre, hipStream_t st, int sm) {
  return with_dtype(dt, dcomp, [&](auto t, auto tc) {
    using T = decltype(t); using TC = decltype(tc);
    if constexpr (!interp_ok<T, T, TC>) return -1;
    else return with_smoother(sm, [&](auto s) {
      return launch_span_rb<T, T, TC, decltype(s)::value>(u, rhs, out_mid, out_next, e_c, rhs_c, partials, g, nsweep_pre, st);
    });
  });
}

void d_down(int sm, int dt, int dx, const void* u, const void* rhs, void* out, void* rhs_c, const LegGeom& g, bool zero_init,
            hipStream_t st) {
  with_dtype(dt, dx, [&](auto t, auto x) {
    using T = decltype(t);
    with_smoother(sm, [&](auto s) {
      launch_leg_sized<kLegDown, T, decltype(x), T, decltype(s)::value>(u, rhs, out, rhs_c, nullptr, g, zero_init, st);
    });
  });
}
int d_up(int sm, int dt, int dx, int dcomp, const void* u, const void* rhs, void* out, const void* e_c, double* partials,
         const LegGeom& g, bool norm, hipStream_t st) {
  return with_dtype(dt, dx, dcomp, [&](auto t, auto x, auto tc) {
    using T = decltype(t); using TX = decltype(x); using TC = decltype(tc);
    if constexpr (!interp_ok<T, TX, TC>) return -1;
    else return with_smoother(sm, [&](auto s) {
      constexpr int SM = decltype(s)::value;
      return norm ? launch_leg_sized<kLegUpNorm, T, TX, TC, SM>(u, rhs, out, e_c, partials, g, false, st)
                  : launch_leg_sized<kLegUp, T, TX, TC, SM>(u, rhs, out, e_c, partials, g, false, st);
    });
  });
}
void d_sweeps(int sm, int dt, const void* u, const void* rhs, void* out, const LegGeom& g, hipStream_t st) {
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    with_smoother(sm, [&](auto s) {
      launch_leg_sized<kLegSweeps, T, T, T, decltype(s)::value>(u, rhs, out, nullptr, nullptr, g, false, st);
    });
  });
}

void d_inject_ring(int di, int dout, const void* fine, void* coarse, int nxf, int nyf, int ldf, int nxc, int nyc, int ldc,
                   hipStream_t st, int sides, int ci_off, int cj_off) {
  with_dtype(di, dout, [&](auto ti, auto to) {
    using TI = decltype(ti); using TO = decltype(to);
    hipLaunchKernelGGL((mg::inject_ring_kernel<TI, TO>), dim3(grid_for(2 * (nxc + nyc))), dim3(mg::kBlock), 0, st,
                       (const TI*)fine, (TO*)coarse, nxf, nyf, ldf, nxc, nyc, ldc, sides, ci_off, cj_off);
  });
}
void d_var(int mode, int dt, const void* u, const void* a, const void* f, void* out, int nx, int ny, int ld, double hx, double hy,
           double omega, double coeff, int colour, int poff, hipStream_t st, double sigma) {
  auto go = [&](auto m) { launch_var<decltype(m)::value>(dt, u, a, f, out, nullptr, nx, ny, ld, hx, hy, omega, coeff, colour, poff, st, sigma); };
  if (mode == mg::kVarJacobi) go(std::integral_constant<int, mg::kVarJacobi>());
  else if (mode == mg::kVarRbgs) go(std::integral_constant<int, mg::kVarRbgs>());
  else if (mode == mg::kVarResidual) go(std::integral_constant<int, mg::kVarResidual>());      // any other mode: no launch
}

// ------------------------------------------------------------------ coarse tail (one workgroup, LDS) ----
// The tail's LDS pool: level l of k .. L-1 starts at byte off[l - k] (off may be null); returns the size of the pool.
static size_t tail_layout(const mg_handle* h, int k, size_t esz, size_t esz_last, int* off) {
  size_t b = 0;
  const size_t extra = h->varcoef ? 1 : 0;          // the coefficient field of every level rides along
  for (int l = k; l < h->L(); ++l) {
    if (off) off[l - k] = (int)b;
    const size_t cells = (size_t)h->lv[l].nx * h->lv[l].ny;
    b += (l == h->L() - 1) ? (2 + extra) * cells * esz_last : (3 + extra) * cells * esz;
    b = (b + 15) / 16 * 16;
  }
  return b + (size_t)mg::kPipeCells * mg::kPipeSlots * esz_last;   // snapshot ring of the pipelined coarsest solve
}
size_t tail_pool_bytes(const mg_handle* h, int k, size_t esz, size_t esz_last) { return tail_layout(h, k, esz, esz_last, nullptr); }

template <typename T, typename TCO, typename TC>
int tail_set_attr(size_t bytes) {
  return (hipFuncSetAttribute(reinterpret_cast<const void*>(&mg::coarse_tail_kernel<T, TCO, TC, false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess &&
          hipFuncSetAttribute(reinterpret_cast<const void*>(&mg::coarse_tail_kernel<T, TCO, TC, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess) ? MG_OK : MG_ERR_HIP;
}
int tail_set_attrs(size_t bytes) {
  return (tail_set_attr<double, double, double>(bytes) != MG_OK || tail_set_attr<float, float, float>(bytes) != MG_OK ||
          tail_set_attr<float, double, double>(bytes) != MG_OK) ? MG_ERR_HIP : MG_OK;
}

void launch_tail(mg_handle* h, bool zero_top) {
  const int k = h->tail_start, L = h->L();
  const int dt = h->level_dtype(k), dco = h->grid_dtype;
  mg::TailArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nlev = L - k; a.nops = h->tail_nops; a.pre = h->cfg.pre; a.post = h->cfg.post;
  a.ld_top = h->lv[k].ld[dt]; a.maxit = h->cfg.coarse_maxit;
  a.omega = h->cfg.omega; a.coeff = h->cfg.coeff; a.tol = h->cfg.coarse_tol; a.tol_x = sqrt_threshold(h->cfg.coarse_tol);
  a.smoother = (h->cfg.smoother == MG_RBGS) ? mg::kSmRbgs : mg::kSmJacobi; a.colour_offset = h->cfg.colour_offset & 1;
  a.sigma = h->sigma;
  a.direct = 0;
  if (h->tail_direct) {
    a.direct = 1;
    std::memcpy(a.minv, h->tail_minv, sizeof(a.minv));
    const Level& cl = h->lv[L - 1];
    if (cl.nx != 5 || cl.ny != 5) { a.minv_dev = h->d_minv; a.minv_n = h->minv_n; }
  }
  const bool var = h->varcoef;
  int offs[mg::kTailMaxLevels];
  const size_t pool = tail_layout(h, k, esize(dt), esize(dco), offs);
  for (int l = k; l < L; ++l) {
    const Level& v = h->lv[l];
    mg::TailLevel& t = a.lv[l - k];
    const Coef c = coefs(v.hx, v.hy, h->sigma);
    t.nx = v.nx; t.ny = v.ny; t.off = offs[l - k];
    t.ihx2 = c.ihx2; t.ihy2 = c.ihy2; t.invD = c.invD; t.diag = c.diag; t.hx2 = v.hx * v.hx; t.hy2 = v.hy * v.hy;
    t.hxhy = v.hx * v.hy; t.use_div = c.pow2 ? 0 : 1; t.exact_recip = c.all_pow2 ? 1 : 0;
    if (var) {     // hx^2, hy^2 powers of two are all the variable-coefficient solve needs to multiply by reciprocals
      int e = 0;
      t.exact_recip = (std::frexp(t.hx2, &e) == 0.5 && std::frexp(t.hy2, &e) == 0.5) ? 1 : 0;
      const int dl = (l == L - 1) ? dco : dt;
      a.a_lv[l - k] = v.a[dl]; a.a_ld[l - k] = v.ld[dl];
    }
  }
  Level& top = h->lv[k];
  const dim3 grid(1), block(mg::kTailBlock);
  with_tail_dtypes(dt, dco, [&](auto t, auto co) {
    using T = decltype(t); using TCO = decltype(co);
    auto k = var ? mg::coarse_tail_kernel<T, TCO, TCO, true> : mg::coarse_tail_kernel<T, TCO, TCO, false>;
    hipLaunchKernelGGL(k, grid, block, pool, h->stream, (const T*)top.rhs[dt], (T*)top.u[dt], h->d_tail_ops, a, zero_top ? 1 : 0,
                       h->d_int);
  });
}

int d_prolong_sub(bool add, int dc, int df, int dcomp, const void* e, void* u, int nxf, int nyf, int ldf, int nxc, int nyc,
                  int ldc, int sides, hipStream_t st) {
  return !add ? launch_prolong<false>(dc, df, dcomp, e, u, nxf, nyf, ldf, nxc, nyc, ldc, sides, st)
              : launch_prolong<true>(dc, df, dcomp, e, u, nxf, nyf, ldf, nxc, nyc, ldc, sides, st);
}
int d_prolong(bool add, int dc, int df, int dcomp, const void* e, void* u, int nxf, int nyf, int ldf, int ldc, hipStream_t st) {
  return d_prolong_sub(add, dc, df, dcomp, e, u, nxf, nyf, ldf, (nxf - 1) / 2 + 1, (nyf - 1) / 2 + 1, ldc, mg::kAllSides, st);
}

// ---- defect correction (MG_PREC_DEFECT): fp64 iterate and residual, fp32 cycles on the error equation -----------------
// One pass over the fine grid per outer step: u <- u + e (the fp32 correction of the cycle just run), r = f - A u in
// fp64, stored as the fp32 right-hand side of the next error equation (zero on boundary cells), sum r^2 for the norm.
// Returns the number of partials.
int launch_defect(mg_handle* h, bool update) {
  Level& v = h->lv[0];
  const Coef c = coefs(v.hx, v.hy, h->sigma);
  const long long pairs = (long long)v.nx * ((v.ny + 1) / 2);
  const int nb = std::min(grid_for(pairs), 2048);
  auto k = update ? mg::residual_xprec_kernel<double, double, float, true, true, true>
                  : mg::residual_xprec_kernel<double, double, float, false, true, true>;
  hipLaunchKernelGGL(k, dim3(nb), dim3(mg::kBlock), 0, h->stream, (const double*)v.u[MG_F64],
                     update ? (const float*)v.u[MG_F32] : nullptr, (const double*)v.rhs[MG_F64], (float*)v.rhs[MG_F32],
                     update ? (double*)v.t[MG_F64] : nullptr, h->partials, v.nx, v.ny, v.ld[MG_F64], v.ld[MG_F32], v.ld[MG_F64],
                     v.ld[MG_F32], c.ihx2, c.ihy2, c.diag, h->cfg.coeff);
  if (update) std::swap(v.u[MG_F64], v.t[MG_F64]);
  return nb;
}

int d_var_residual_norm(int dt, const void* u, const void* a, const void* f, double* partials, int nx, int ny, int ld, double hx,
                        double hy, double coeff, hipStream_t st, double sigma) {
  return launch_var<mg::kVarResidualNorm>(dt, u, a, f, nullptr, partials, nx, ny, ld, hx, hy, 1.0, coeff, 0, 0, st, sigma);
}

// mg_time_op op 11: the bare stream of one Jacobi sweep (same traffic, no stencil)
void d_stream_triad(int dt, const void* a, const void* b, void* out, int nx, int ny, int ld, hipStream_t st) {
  const int N = (int)(16 / esize(dt)), nyv = std::min(ld, (ny + N - 1) / N * N);
  const int tiles_j = (nyv / N + 63) / 64, tiles_i = (nx + 15) / 16;
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(mg::stream_triad_kernel<T>, dim3(tiles_i * tiles_j), dim3(256), 0, st, (const T*)a, (const T*)b, (T*)out, nx, nyv, ld, tiles_j);
  });
}
// r (fp64) = f - A u of fp32 fields
void d_residual_f32in_f64out(const float* u, const float* f, double* r, int nx, int ny, int ld_in, int ld_out, double hx,
                             double hy, double coeff, hipStream_t st) {
  const Coef c = coefs(hx, hy);
  const long long pairs = (long long)nx * ((ny + 1) / 2);
  hipLaunchKernelGGL((mg::residual_xprec_kernel<float, float, double, false, false, false>), dim3(grid_for(pairs)), dim3(mg::kBlock), 0,
                     st, u, (const float*)nullptr, f, r, (double*)nullptr, (double*)nullptr, nx, ny, ld_in, ld_in, ld_in,
                     ld_out, c.ihx2, c.ihy2, c.diag, coeff);
}

}  // namespace mgh

#if MG_EXP_TAIL_TRACE
// timing experiment: s_memtime stamps of the last coarse_tail_kernel launch (entry, prologue, after every op, exit)
extern "C" int mg_exp_tail_trace(long long* out64) {
  return hipMemcpyFromSymbol(out64, HIP_SYMBOL(mg::g_tail_trace), sizeof(long long) * 64) == hipSuccess ? MG_OK : MG_ERR_HIP;
}
#endif
