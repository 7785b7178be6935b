// The 3-D multigrid family of libmghip.so (include/mghip_3d.h): the seven-point Poisson / Helmholtz operator on a vertex-centred
// (nx, ny, nz) grid, weighted Jacobi and red-black Gauss-Seidel, 27-point full weighting, trilinear prolongation, V and W
// cycles in fp64, fp32 or as fp64 defect correction around ONE fp32 cycle.  This unit instantiates the kernels of
// mg_3d_kernels.hpp and holds their launchers, the stateless device forms and the engine (mg3_handle).  It shares nothing with the
// 2-D engine but mg_host.hpp's helpers, the pitch rule (mg_pitch_elems) and the fixed-order reduce with its host mailbox.
//
//   cycle(l):  pre sweeps -> r = f - A u -> f[l+1] = R r -> u[l+1] = 0 -> cycle(l+1) once (V) or twice (W) -> u += P u[l+1] -> post
//   cycle(L-1): coarse_sweeps red-black sweeps (one LDS launch up to 17^3)
//   defect:    r32 = fp32(f64 - A u64) -> e = 0 -> cycle(0) in fp32 on A e = r32 -> u64 += (double)e
#include "mg_host.hpp"
#include "../../include/mghip_3d.h"
#include "mg_3d_kernels.hpp"

#include <atomic>

using namespace mgh;

namespace {

struct Level3 {
  int nx = 0, ny = 0, nz = 0, ld = 0;
  double hx = 0, hy = 0, hz = 0;
  void* u = nullptr;      // iterate
  void* t = nullptr;      // Jacobi partner (the same boundary faces as u); NULL for red-black and on the coarsest level
  void* f = nullptr;      // right-hand side
  void* r = nullptr;      // residual (faces stay zero); NULL on the coarsest level
  size_t cells() const { return (size_t)nx * ny * ld; }
};

}  // namespace

struct mg3_handle {
  mg3_config cfg;
  std::vector<Level3> lv;
  int dt = MG_F64;                 // the hierarchy's dtype
  double* u64 = nullptr;           // defect: the fp64 iterate and right-hand side (pitch ld64)
  double* f64 = nullptr;
  int ld64 = 0;
  bool r32_current = false;        // defect: lv[0].f holds fp32(f64 - A u64) of the current iterate
  hipStream_t stream = nullptr;
  double* partials = nullptr;
  double* d_scalar = nullptr;
  double* h_scalar = nullptr;      // pinned host
  mg::HostMailbox* mbox = nullptr;       // pinned, mapped: the norm of every cycle arrives here
  mg::HostMailbox* mbox_dev = nullptr;
  unsigned long long mbox_seq = 0;
  int64_t bytes = 0;
  bool have_rhs = false;
  std::string err;
  int L() const { return (int)lv.size(); }
  bool defect() const { return cfg.precision == MG3_PREC_DEFECT; }
};

namespace {

// ---- geometry, coefficients, argument predicates ----
template <typename T> mg3::Geom3 geom3(int nx, int ny, int nz, int ld, int ld_out) {
  mg3::Geom3 g;
  g.nx = nx; g.ny = ny; g.nz = nz; g.ld = ld; g.ld_out = ld_out;
  g.tiles_j = (ny + mg3::kT3J - 1) / mg3::kT3J;
  g.tiles_k = (nz + mg3::Tile3<T>::TK - 1) / mg3::Tile3<T>::TK;
  g.chunks = (nx - 2 + mg3::kT3I - 1) / mg3::kT3I;
  return g;
}
int ntiles(const mg3::Geom3& g) { return g.tiles_j * g.tiles_k * g.chunks; }
// what the header states: formed in double, rounded to T
template <typename T> mg3::Coef3<T> coef3(double hx, double hy, double hz, double sigma, double omega) {
  const double ihx2 = 1.0 / (hx * hx), ihy2 = 1.0 / (hy * hy), ihz2 = 1.0 / (hz * hz);
  const double diag = ((2.0 * ihx2 + 2.0 * ihy2) + 2.0 * ihz2) + sigma;
  mg3::Coef3<T> c;
  c.ihx2 = (T)ihx2; c.ihy2 = (T)ihy2; c.ihz2 = (T)ihz2; c.diag = (T)diag; c.w = (T)(omega / diag);
  return c;
}
// partials any sum on an (nx, ny, nz) field writes at most: the fp64 tiling has the most workgroups
size_t max_partials3(int nx, int ny, int nz) {
  return std::max<size_t>((size_t)ntiles(geom3<double>(nx, ny, nz, nz, nz)), (size_t)mg3::kNormBlocks) + 1;
}
bool shape_ok(int nx, int ny, int nz) { return nx >= 3 && ny >= 3 && nz >= 3 && (double)nx * ny * nz < 2.0e9; }
bool ld_ok3(int nz, int ld) { return ld >= nz && ld % 2 == 0; }
bool spacing_ok(double hx, double hy, double hz) { return pos_finite(hx) && pos_finite(hy) && pos_finite(hz); }
bool sigma_ok(double sigma) { return sigma >= 0.0 && std::isfinite(sigma); }
int grid_for(long long total) { return (int)std::max<long long>(1, std::min<long long>((total + mg::kBlock - 1) / mg::kBlock, 1 << 16)); }

// ---- launchers (shared by the engine and the stateless forms); an int result is the number of partials ----
template <typename T, typename TR, int MODE, bool WRITE, bool NORM>
int launch_sweep(const void* u, const void* f, void* out, double* partials, int nx, int ny, int nz, int ld, int ld_out, double hx,
                 double hy, double hz, double sigma, double omega, int colour_par, hipStream_t st) {
  const mg3::Geom3 g = geom3<T>(nx, ny, nz, ld, ld_out);
  hipLaunchKernelGGL((mg3::mg3_sweep_kernel<T, TR, MODE, WRITE, NORM>), dim3(ntiles(g)), dim3(mg::kBlock), 0, st, (const T*)u,
                     (const T*)f, (TR*)out, partials, g, coef3<T>(hx, hy, hz, sigma, omega), colour_par);
  return ntiles(g);
}
void d3_jacobi(int dt, const void* u, const void* f, void* out, const Level3& v, double sigma, double omega, hipStream_t st) {
  with_dtype(dt, [&](auto x) {
    using T = decltype(x);
    launch_sweep<T, T, mg3::kM3Jacobi, true, false>(u, f, out, nullptr, v.nx, v.ny, v.nz, v.ld, v.ld, v.hx, v.hy, v.hz, sigma, omega, 0, st);
  });
}
void d3_colour(int dt, void* u, const void* f, const Level3& v, double sigma, double omega, int colour, int offset, hipStream_t st) {
  with_dtype(dt, [&](auto x) {
    using T = decltype(x);
    launch_sweep<T, T, mg3::kM3Colour, true, false>(u, f, u, nullptr, v.nx, v.ny, v.nz, v.ld, v.ld, v.hx, v.hy, v.hz, sigma, omega,
                                                    (colour ^ offset) & 1, st);
  });
}
// r (nullable) of rdt with pitch ld_r; partials (nullable): sum r^2
int d3_residual(int dt, int rdt, const void* u, const void* f, void* r, int ld_r, double* partials, const Level3& v, double sigma,
                hipStream_t st) {
  auto go = [&](auto x, auto y) {
    using T = decltype(x);
    using TR = decltype(y);
    auto a = [&](auto w, auto n) {
      return launch_sweep<T, TR, mg3::kM3Residual, decltype(w)::value, decltype(n)::value>(u, f, r, partials, v.nx, v.ny, v.nz, v.ld, ld_r,
                                                                                          v.hx, v.hy, v.hz, sigma, 1.0, 0, st);
    };
    using Y = std::true_type;
    using N = std::false_type;
    return r ? (partials ? a(Y(), Y()) : a(Y(), N())) : a(N(), Y());
  };
  if (dt == MG_F32) return go(float(), float());
  return rdt == MG_F32 ? go(double(), float()) : go(double(), double());
}
void d3_restrict(int dt, const void* fine, void* coarse, const Level3& vf, const Level3& vc, hipStream_t st) {
  const long long total = (long long)(vc.nx - 2) * (vc.ny - 2) * (vc.nz - 2);
  with_dtype(dt, [&](auto x) {
    using T = decltype(x);
    hipLaunchKernelGGL(mg3::mg3_restrict_kernel<T>, dim3(grid_for(total)), dim3(mg::kBlock), 0, st, (const T*)fine, (T*)coarse, vc.nx,
                       vc.ny, vc.nz, vf.ny, vf.ld, vc.ld);
  });
}
void d3_prolong_add(int dt, const void* e, void* u, const Level3& vf, const Level3& vc, hipStream_t st) {
  with_dtype(dt, [&](auto x) {
    using T = decltype(x);
    const int vpr = (vf.nz + mg::VecW<T>::N - 1) / mg::VecW<T>::N;
    const long long total = (long long)(vf.nx - 2) * (vf.ny - 2) * vpr;
    hipLaunchKernelGGL(mg3::mg3_prolong_add_kernel<T>, dim3(grid_for(total)), dim3(mg::kBlock), 0, st, (const T*)e, (T*)u, vf.nx, vf.ny,
                       vf.nz, vf.ld, vc.ny, vc.ld);
  });
}
void d3_upcast_add(const float* e, double* u, int nx, int ny, int nz, int ld64, int ld32, hipStream_t st) {
  const long long total = (long long)(nx - 2) * (ny - 2) * ((nz + 1) / 2);
  hipLaunchKernelGGL(mg3::mg3_upcast_add_kernel, dim3(grid_for(total)), dim3(mg::kBlock), 0, st, e, u, nx, ny, nz, ld64, ld32);
}
void d3_copy(int din, int dout, const void* in, void* out, int nx, int ny, int nz, int ld_in, int ld_out, hipStream_t st) {
  const long long rows = (long long)nx * ny;
  with_dtype(din, dout, [&](auto x, auto y) {
    using TI = decltype(x);
    using TO = decltype(y);
    hipLaunchKernelGGL((mg3::mg3_copy_kernel<TI, TO>), dim3(grid_for(rows * nz)), dim3(mg::kBlock), 0, st, (const TI*)in, (TO*)out, rows,
                       nz, ld_in, ld_out);
  });
}
int d3_sumsq(int dt, const void* x, double* partials, int nx, int ny, int nz, int ld, hipStream_t st) {
  const long long rows = (long long)nx * ny;
  return with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    const int vpr = (nz + mg::VecW<T>::N - 1) / mg::VecW<T>::N;
    const int n = (int)std::min<long long>(grid_for(rows * vpr), mg3::kNormBlocks);
    hipLaunchKernelGGL(mg3::mg3_sumsq_kernel<T>, dim3(n), dim3(mg::kBlock), 0, st, (const T*)x, partials, rows, nz, ld);
    return n;
  });
}
void d3_reduce(const double* partials, int n, double* out, hipStream_t st, mg::HostMailbox* mbox = nullptr, unsigned long long seq = 0) {
  hipLaunchKernelGGL(mg::reduce_partials_kernel<3>, dim3(1), dim3(mg::kReduceBlock), 0, st, partials, n, out, mbox, seq);
}
bool coarse_fits_lds(int nx, int ny, int nz) { return std::max(nx, std::max(ny, nz)) <= mg3::kCoarseLdsExtent; }
// `sweeps` red-black sweeps with omega = 1 in place; *used_lds (nullable): the single-workgroup path ran
int d3_coarse_solve(int dt, void* u, const void* f, const Level3& v, double sigma, int sweeps, bool* used_lds, hipStream_t st) {
  const bool lds = coarse_fits_lds(v.nx, v.ny, v.nz);
  if (used_lds) *used_lds = lds;
  if (!lds) {
    for (int s = 0; s < sweeps; ++s)
      for (int c = 0; c < 2; ++c) d3_colour(dt, u, f, v, sigma, 1.0, c, 0, st);
    return MG_OK;
  }
  return with_dtype(dt, [&](auto x) {
    using T = decltype(x);
    const int bytes = 2 * v.nx * v.ny * v.nz * (int)sizeof(T);
    HIPC(nullptr, hipFuncSetAttribute(reinterpret_cast<const void*>(&mg3::mg3_coarse_lds_kernel<T>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    hipLaunchKernelGGL(mg3::mg3_coarse_lds_kernel<T>, dim3(1), dim3(mg3::kCoarseLdsBlock), bytes, st, (T*)u, (const T*)f, v.nx, v.ny,
                       v.nz, v.ld, coef3<T>(v.hx, v.hy, v.hz, sigma, 1.0), sweeps);
    return (int)MG_OK;
  });
}
Level3 level_of(int nx, int ny, int nz, int ld, double hx, double hy, double hz) {
  Level3 v;
  v.nx = nx; v.ny = ny; v.nz = nz; v.ld = ld; v.hx = hx; v.hy = hy; v.hz = hz;
  return v;
}

// ---- the engine ----
int config_check(const mg3_config* c) {
  CHECK_ARG(c, "mg3: NULL configuration");
  CHECK_ARG(shape_ok(c->nx, c->ny, c->nz), "mg3: every extent must be >= 3 (and the grid below 2e9 cells)");
  CHECK_ARG(sigma_ok(c->sigma), "mg3: sigma must be finite and >= 0");
  for (double x : {c->x0, c->x1, c->y0, c->y1, c->z0, c->z1}) CHECK_ARG(std::isfinite(x), "mg3: the domain must be finite");
  CHECK_ARG(c->x1 > c->x0 && c->y1 > c->y0 && c->z1 > c->z0, "mg3: the domain is empty");
  CHECK_ARG(c->pre >= 0 && c->post >= 0 && c->pre + c->post >= 1, "mg3: at least one smoothing sweep (pre + post >= 1)");
  CHECK_ARG(c->max_levels >= 1, "mg3: max_levels must be >= 1");
  CHECK_ARG(pos_finite(c->omega), "mg3: omega must be finite and > 0");
  CHECK_ARG(c->cycle == MG_CYCLE_V || c->cycle == MG_CYCLE_W, "mg3: unknown cycle (MG_CYCLE_V or MG_CYCLE_W)");
  CHECK_ARG(c->smoother == MG_JACOBI || c->smoother == MG_RBGS, "mg3: unknown smoother (MG_JACOBI or MG_RBGS)");
  CHECK_ARG(c->precision >= MG3_PREC_DOUBLE && c->precision <= MG3_PREC_DEFECT, "mg3: unknown precision");
  return MG_OK;
}
int pitch3(int dt, int nz) {
  int ld = 0;
  (void)mg_pitch_elems(dt, nz, &ld);
  return ld;
}
// the hierarchy of a configuration (no pointers yet)
void plan_levels(mg3_handle* h) {
  const mg3_config& c = h->cfg;
  h->dt = c.precision == MG3_PREC_DOUBLE ? MG_F64 : MG_F32;
  int nx = c.nx, ny = c.ny, nz = c.nz;
  for (int l = 0; l < c.max_levels; ++l) {
    h->lv.push_back(level_of(nx, ny, nz, pitch3(h->dt, nz), (c.x1 - c.x0) / (nx - 1), (c.y1 - c.y0) / (ny - 1), (c.z1 - c.z0) / (nz - 1)));
    if (!(nx % 2 && ny % 2 && nz % 2) || nx < 5 || ny < 5 || nz < 5) break;
    nx = (nx + 1) / 2; ny = (ny + 1) / 2; nz = (nz + 1) / 2;
  }
  h->ld64 = pitch3(MG_F64, c.nz);
}
// every device allocation of the engine, in one place: visit(slot, bytes).  mg3_create allocates through it, mg3_device_bytes sums
template <typename F> int for_each_alloc(mg3_handle* h, F&& visit) {
  const size_t es = esize(h->dt);
  int rc;
  for (int l = 0; l < h->L(); ++l) {
    Level3& v = h->lv[l];
    const bool coarsest = l == h->L() - 1;
    if ((rc = visit(&v.u, v.cells() * es)) != MG_OK) return rc;
    if ((rc = visit(&v.f, v.cells() * es)) != MG_OK) return rc;
    if (!coarsest && (rc = visit(&v.r, v.cells() * es)) != MG_OK) return rc;
    if (!coarsest && h->cfg.smoother == MG_JACOBI && (rc = visit(&v.t, v.cells() * es)) != MG_OK) return rc;
  }
  if (h->defect()) {
    const size_t b = (size_t)h->cfg.nx * h->cfg.ny * h->ld64 * sizeof(double);
    if ((rc = visit((void**)&h->u64, b)) != MG_OK) return rc;
    if ((rc = visit((void**)&h->f64, b)) != MG_OK) return rc;
  }
  if ((rc = visit((void**)&h->partials, max_partials3(h->cfg.nx, h->cfg.ny, h->cfg.nz) * sizeof(double))) != MG_OK) return rc;
  return visit((void**)&h->d_scalar, 16);
}
void release(mg3_handle* h) {
  (void)for_each_alloc(h, [](void** p, size_t) { if (*p) { (void)hipFree(*p); *p = nullptr; } return (int)MG_OK; });
  if (h->h_scalar) { (void)hipHostFree(h->h_scalar); h->h_scalar = nullptr; }
  if (h->mbox) { (void)hipHostFree(h->mbox); h->mbox = nullptr; }
  if (h->stream) { (void)hipStreamDestroy(h->stream); h->stream = nullptr; }
}

int smooth(mg3_handle* h, int l, int sweeps) {
  Level3& v = h->lv[l];
  for (int s = 0; s < sweeps; ++s) {
    if (h->cfg.smoother == MG_JACOBI) {
      d3_jacobi(h->dt, v.u, v.f, v.t, v, h->cfg.sigma, h->cfg.omega, h->stream);
      std::swap(v.u, v.t);
    } else {
      for (int c = 0; c < 2; ++c) d3_colour(h->dt, v.u, v.f, v, h->cfg.sigma, h->cfg.omega, c, 0, h->stream);
    }
  }
  return MG_OK;
}
int cycle_level(mg3_handle* h, int l) {
  Level3& v = h->lv[l];
  if (l == h->L() - 1) {
    const int sweeps = h->cfg.coarse_sweeps > 0 ? h->cfg.coarse_sweeps : 64;
    const int rc = d3_coarse_solve(h->dt, v.u, v.f, v, h->cfg.sigma, sweeps, nullptr, h->stream);
    return rc == MG_OK ? MG_OK : fail(&h->err, rc, last_error());
  }
  Level3& c = h->lv[l + 1];
  smooth(h, l, h->cfg.pre);
  d3_residual(h->dt, h->dt, v.u, v.f, v.r, v.ld, nullptr, v, h->cfg.sigma, h->stream);
  d3_restrict(h->dt, v.r, c.f, v, c, h->stream);
  HIPC(&h->err, hipMemsetAsync(c.u, 0, c.cells() * esize(h->dt), h->stream));
  for (int visit = 0; visit < (h->cfg.cycle == MG_CYCLE_W ? 2 : 1); ++visit) {
    const int rc = cycle_level(h, l + 1);
    if (rc != MG_OK) return rc;
  }
  d3_prolong_add(h->dt, c.u, v.u, v, c, h->stream);
  smooth(h, l, h->cfg.post);
  return MG_OK;
}
// defect: lv[0].f := fp32(f64 - A u64); partials (nullable): sum of the fp64 r^2.  Returns the number of partials
int defect_residual(mg3_handle* h, bool with_norm) {
  Level3 v = h->lv[0];
  v.ld = h->ld64;
  const int n = d3_residual(MG_F64, MG_F32, h->u64, h->f64, h->lv[0].f, h->lv[0].ld, with_norm ? h->partials : nullptr, v, h->cfg.sigma,
                            h->stream);
  h->r32_current = true;
  return n;
}
int one_cycle(mg3_handle* h) {
  if (!h->defect()) return cycle_level(h, 0);
  Level3& v = h->lv[0];
  if (!h->r32_current) defect_residual(h, false);
  HIPC(&h->err, hipMemsetAsync(v.u, 0, v.cells() * sizeof(float), h->stream));
  if (v.t) HIPC(&h->err, hipMemsetAsync(v.t, 0, v.cells() * sizeof(float), h->stream));
  const int rc = cycle_level(h, 0);
  if (rc != MG_OK) return rc;
  d3_upcast_add((const float*)v.u, h->u64, v.nx, v.ny, v.nz, h->ld64, v.ld, h->stream);
  h->r32_current = false;
  return MG_OK;
}
// the sum of n partials to the host: through the mailbox (the host spins on the sequence number), else copy + synchronise
int reduce_to_host(mg3_handle* h, int n, double* value) {
  if (h->mbox_dev) {
    const unsigned long long seq = ++h->mbox_seq;
    d3_reduce(h->partials, n, h->d_scalar, h->stream, h->mbox_dev, seq);
    HIPC(&h->err, hipGetLastError());
    volatile unsigned long long* flag = &h->mbox->seq;
    const double t0 = now_s();
    long spins = 0;
    while (*flag != seq)
      if ((++spins & 0x3fff) == 0 && now_s() - t0 > 2.0) break;
    if (*flag != seq) HIPC(&h->err, hipStreamSynchronize(h->stream));
    if (*flag == seq) {
      std::atomic_thread_fence(std::memory_order_acquire);
      *value = *(volatile double*)&h->mbox->value;
      return MG_OK;
    }
  } else {
    d3_reduce(h->partials, n, h->d_scalar, h->stream);
  }
  HIPC(&h->err, hipMemcpyAsync(h->h_scalar, h->d_scalar, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  *value = *h->h_scalar;
  return MG_OK;
}
int norm_now(mg3_handle* h, double* out) {
  const Level3& v = h->lv[0];
  const int n = h->defect() ? defect_residual(h, true)
                            : d3_residual(h->dt, h->dt, v.u, v.f, nullptr, v.ld, h->partials, v, h->cfg.sigma, h->stream);
  double ss = 0.0;
  const int rc = reduce_to_host(h, n, &ss);
  if (rc != MG_OK) return rc;
  *out = std::sqrt(v.hx * v.hy * v.hz * ss);
  return MG_OK;
}
void* iterate(mg3_handle* h) { return h->defect() ? (void*)h->u64 : h->lv[0].u; }
int iterate_dtype(const mg3_handle* h) { return h->defect() ? MG_F64 : h->dt; }
int iterate_ld(const mg3_handle* h) { return h->defect() ? h->ld64 : h->lv[0].ld; }

// host array (nx, ny, nz) of hdt -> device field of ddt with pitch ld (converted on the host), and back; both wait for the stream
int put3(mg3_handle* h, void* dev, int ddt, int ld, const void* host, int hdt) {
  const size_t n = (size_t)h->cfg.nx * h->cfg.ny * h->cfg.nz, es = esize(ddt);
  std::vector<unsigned char> tmp;
  const void* src = host;
  if (hdt != ddt) {
    tmp.resize(n * es);
    if (ddt == MG_F64) for (size_t k = 0; k < n; ++k) ((double*)tmp.data())[k] = (double)((const float*)host)[k];
    else for (size_t k = 0; k < n; ++k) ((float*)tmp.data())[k] = (float)((const double*)host)[k];
    src = tmp.data();
  }
  HIPC(&h->err, hipMemcpy2DAsync(dev, (size_t)ld * es, src, (size_t)h->cfg.nz * es, (size_t)h->cfg.nz * es, (size_t)h->cfg.nx * h->cfg.ny,
                                 hipMemcpyHostToDevice, h->stream));
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  return MG_OK;
}
int get3(mg3_handle* h, void* host, int hdt, const void* dev, int ddt, int ld) {
  const size_t n = (size_t)h->cfg.nx * h->cfg.ny * h->cfg.nz, es = esize(ddt);
  std::vector<unsigned char> tmp;
  void* dst = host;
  if (hdt != ddt) { tmp.resize(n * es); dst = tmp.data(); }
  HIPC(&h->err, hipMemcpy2DAsync(dst, (size_t)h->cfg.nz * es, dev, (size_t)ld * es, (size_t)h->cfg.nz * es, (size_t)h->cfg.nx * h->cfg.ny,
                                 hipMemcpyDeviceToHost, h->stream));
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  if (hdt != ddt) {
    if (hdt == MG_F64) for (size_t k = 0; k < n; ++k) ((double*)host)[k] = (double)((const float*)tmp.data())[k];
    else for (size_t k = 0; k < n; ++k) ((float*)host)[k] = (float)((const double*)tmp.data())[k];
  }
  return MG_OK;
}
#define H3_ARG(cond, msg) do { if (!(cond)) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, msg); } while (0)
// after the iterate changed under the engine: the Jacobi partner carries the same faces
int iterate_changed(mg3_handle* h) {
  h->r32_current = false;
  Level3& v = h->lv[0];
  if (!h->defect() && v.t) HIPC(&h->err, hipMemcpyAsync(v.t, v.u, v.cells() * esize(h->dt), hipMemcpyDeviceToDevice, h->stream));
  return MG_OK;
}

}  // namespace

extern "C" {

int mg3_device_bytes(const mg3_config* cfg, int64_t* bytes) {
  const int rc = config_check(cfg);
  if (rc != MG_OK) return rc;
  CHECK_ARG(bytes, "mg3_device_bytes: NULL result");
  mg3_handle h;
  h.cfg = *cfg;
  plan_levels(&h);
  int64_t total = 0;
  (void)for_each_alloc(&h, [&](void**, size_t b) { total += (int64_t)b; return (int)MG_OK; });
  *bytes = total;
  return MG_OK;
}

int mg3_create(const mg3_config* cfg, mg3_handle** out) {
  const int ok = config_check(cfg);
  if (ok != MG_OK) return ok;
  CHECK_ARG(out, "mg3_create: NULL result");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, MG_ERR_NO_DEVICE, "mg3_create: no HIP device");
  CHECK_ARG(cfg->device >= 0 && cfg->device < ndev, "mg3_create: no such device");
  mg3_handle* h = new mg3_handle;
  h->cfg = *cfg;
  auto bail = [&](int code) { return create_fail(h, release, code); };
  if (hipSetDevice(cfg->device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    h->err = "mg3_create: cannot open the device";
    return bail(MG_ERR_HIP);
  }
  plan_levels(h);
  int rc = for_each_alloc(h, [&](void** p, size_t b) {
    const int r = alloc_zero(&h->err, p, b, h->stream);
    if (r == MG_OK) h->bytes += (int64_t)b;
    return r;
  });
  if (rc != MG_OK) return bail(rc);
  if (hipHostMalloc((void**)&h->h_scalar, sizeof(double)) != hipSuccess) { h->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  if (hipHostMalloc((void**)&h->mbox, sizeof(mg::HostMailbox), hipHostMallocMapped) == hipSuccess &&
      hipHostGetDevicePointer((void**)&h->mbox_dev, h->mbox, 0) == hipSuccess) {
    h->mbox->value = 0; h->mbox->seq = 0;
  } else {
    h->mbox_dev = nullptr;     // no mapped host memory: copy + stream synchronisation
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "mg3_create: the device failed"; return bail(MG_ERR_HIP); }
  *out = h;
  return MG_OK;
}

int mg3_destroy(mg3_handle* h) { return destroy_owned(h, h ? h->stream : nullptr, release); }

const char* mg3_last_error(const mg3_handle* h) { return h ? h->err.c_str() : last_error().c_str(); }

int mg3_set_rhs(mg3_handle* h, const void* f_host, int host_dtype) {
  H3_ARG(h && f_host && valid_dtype(host_dtype), "mg3_set_rhs: bad argument");
  (void)hipSetDevice(h->cfg.device);
  h->r32_current = false;
  h->have_rhs = true;
  return h->defect() ? put3(h, h->f64, MG_F64, h->ld64, f_host, host_dtype) : put3(h, h->lv[0].f, h->dt, h->lv[0].ld, f_host, host_dtype);
}
int mg3_set_solution(mg3_handle* h, const void* u_host, int host_dtype) {
  H3_ARG(h && u_host && valid_dtype(host_dtype), "mg3_set_solution: bad argument");
  (void)hipSetDevice(h->cfg.device);
  const int rc = put3(h, iterate(h), iterate_dtype(h), iterate_ld(h), u_host, host_dtype);
  return rc != MG_OK ? rc : iterate_changed(h);
}
int mg3_get_solution(mg3_handle* h, void* u_host, int host_dtype) {
  H3_ARG(h && u_host && valid_dtype(host_dtype), "mg3_get_solution: bad argument");
  (void)hipSetDevice(h->cfg.device);
  return get3(h, u_host, host_dtype, iterate(h), iterate_dtype(h), iterate_ld(h));
}
int mg3_set_rhs_device(mg3_handle* h, const void* f_dev, int ld, int dtype) {
  H3_ARG(h && f_dev && valid_dtype(dtype) && ld_ok3(h->cfg.nz, ld) && aligned16(f_dev), "mg3_set_rhs_device: bad pointer, dtype or pitch");
  (void)hipSetDevice(h->cfg.device);
  h->r32_current = false;
  h->have_rhs = true;
  if (h->defect()) d3_copy(dtype, MG_F64, f_dev, h->f64, h->cfg.nx, h->cfg.ny, h->cfg.nz, ld, h->ld64, h->stream);
  else d3_copy(dtype, h->dt, f_dev, h->lv[0].f, h->cfg.nx, h->cfg.ny, h->cfg.nz, ld, h->lv[0].ld, h->stream);
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}
int mg3_set_solution_device(mg3_handle* h, const void* u_dev, int ld, int dtype) {
  H3_ARG(h && u_dev && valid_dtype(dtype) && ld_ok3(h->cfg.nz, ld) && aligned16(u_dev), "mg3_set_solution_device: bad pointer, dtype or pitch");
  (void)hipSetDevice(h->cfg.device);
  d3_copy(dtype, iterate_dtype(h), u_dev, iterate(h), h->cfg.nx, h->cfg.ny, h->cfg.nz, ld, iterate_ld(h), h->stream);
  HIPC(&h->err, hipGetLastError());
  return iterate_changed(h);
}
int mg3_get_solution_device(mg3_handle* h, void* u_dev, int ld, int dtype) {
  H3_ARG(h && u_dev && valid_dtype(dtype) && ld_ok3(h->cfg.nz, ld) && aligned16(u_dev), "mg3_get_solution_device: bad pointer, dtype or pitch");
  (void)hipSetDevice(h->cfg.device);
  d3_copy(iterate_dtype(h), dtype, iterate(h), u_dev, h->cfg.nx, h->cfg.ny, h->cfg.nz, iterate_ld(h), ld, h->stream);
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}
int mg3_zero_solution(mg3_handle* h) {
  H3_ARG(h, "mg3_zero_solution: NULL handle");
  (void)hipSetDevice(h->cfg.device);
  HIPC(&h->err, hipMemsetAsync(iterate(h), 0, (size_t)h->cfg.nx * h->cfg.ny * iterate_ld(h) * esize(iterate_dtype(h)), h->stream));
  return iterate_changed(h);
}
int mg3_cycle(mg3_handle* h, int n) {
  H3_ARG(h && n >= 0, "mg3_cycle: bad argument");
  if (!h->have_rhs) return fail(&h->err, MG_ERR_STATE, "mg3_cycle: no right-hand side set");
  (void)hipSetDevice(h->cfg.device);
  for (int k = 0; k < n; ++k) {
    const int rc = one_cycle(h);
    if (rc != MG_OK) return rc;
  }
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}
int mg3_residual_norm(mg3_handle* h, double* out) {
  H3_ARG(h && out, "mg3_residual_norm: bad argument");
  if (!h->have_rhs) return fail(&h->err, MG_ERR_STATE, "mg3_residual_norm: no right-hand side set");
  (void)hipSetDevice(h->cfg.device);
  return norm_now(h, out);
}
int mg3_solve(mg3_handle* h, double tol, int max_iter, double* hist, int hist_cap, int* n_iter, int* converged, mg3_stats* stats) {
  H3_ARG(h && max_iter >= 0 && hist_cap >= 0 && (hist || hist_cap == 0) && !std::isnan(tol), "mg3_solve: bad argument");
  if (!h->have_rhs) return fail(&h->err, MG_ERR_STATE, "mg3_solve: no right-hand side set");
  (void)hipSetDevice(h->cfg.device);
  const double t0 = now_s();
  double norm = 0.0;
  int rc = norm_now(h, &norm);
  if (rc != MG_OK) return rc;
  const double first = norm;
  if (hist_cap > 0) hist[0] = norm;
  int it = 0;
  bool done = norm < tol;
  while (!done && it < max_iter) {
    if ((rc = one_cycle(h)) != MG_OK || (rc = norm_now(h, &norm)) != MG_OK) return rc;
    ++it;
    if (it < hist_cap) hist[it] = norm;
    done = norm < tol;
  }
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  if (n_iter) *n_iter = it;
  if (converged) *converged = done ? 1 : 0;
  if (stats) {
    stats->initial_residual = first; stats->final_residual = norm; stats->solve_seconds = now_s() - t0;
    stats->device_bytes = h->bytes;
    stats->iterations = it; stats->converged = done ? 1 : 0; stats->levels = h->L(); stats->reserved = 0;
  }
  return MG_OK;
}
int mg3_synchronize(mg3_handle* h) {
  H3_ARG(h, "mg3_synchronize: NULL handle");
  (void)hipSetDevice(h->cfg.device);
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  return MG_OK;
}
int mg3_stream(mg3_handle* h, void** stream) {
  H3_ARG(h && stream, "mg3_stream: bad argument");
  *stream = (void*)h->stream;
  return MG_OK;
}
int mg3_num_levels(const mg3_handle* h, int* levels) {
  CHECK_ARG(h && levels, "mg3_num_levels: bad argument");
  *levels = h->L();
  return MG_OK;
}

// ---- the stateless device forms ----
int mg3_dev_scratch_bytes(int nx, int ny, int nz, int64_t* bytes) {
  CHECK_ARG(bytes && shape_ok(nx, ny, nz), "mg3_dev_scratch_bytes: bad argument");
  *bytes = (int64_t)sizeof(double) * (int64_t)max_partials3(nx, ny, nz);
  return MG_OK;
}
int mg3_dev_residual(int dtype, int r_dtype, int nx, int ny, int nz, int ld, int ld_r, double hx, double hy, double hz, double sigma,
                     const void* u, const void* f, void* r, void* scratch, double* sumsq_dev, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && valid_dtype(r_dtype) && !(dtype == MG_F32 && r_dtype == MG_F64), "mg3_dev_residual: bad dtype");
  CHECK_ARG(shape_ok(nx, ny, nz) && ld_ok3(nz, ld) && (!r || ld_ok3(nz, ld_r)), "mg3_dev_residual: bad shape / pitch");
  CHECK_ARG(spacing_ok(hx, hy, hz) && sigma_ok(sigma), "mg3_dev_residual: bad spacing / sigma");
  CHECK_ARG(u && f && aligned16(u) && aligned16(f) && aligned16(r) && (r || sumsq_dev) && r != u && r != f, "mg3_dev_residual: bad pointer");
  CHECK_ARG(!sumsq_dev || (scratch && aligned16(scratch)), "mg3_dev_residual: a sum needs scratch");
  const Level3 v = level_of(nx, ny, nz, ld, hx, hy, hz);
  const int n = d3_residual(dtype, r_dtype, u, f, r, ld_r, sumsq_dev ? (double*)scratch : nullptr, v, sigma, (hipStream_t)stream);
  if (sumsq_dev) d3_reduce((const double*)scratch, n, sumsq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}
int mg3_dev_jacobi(int dtype, int nx, int ny, int nz, int ld, double hx, double hy, double hz, double sigma, double omega, const void* u,
                   const void* f, void* out, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && shape_ok(nx, ny, nz) && ld_ok3(nz, ld), "mg3_dev_jacobi: bad dtype / shape / pitch");
  CHECK_ARG(spacing_ok(hx, hy, hz) && sigma_ok(sigma) && std::isfinite(omega), "mg3_dev_jacobi: bad spacing / sigma / omega");
  CHECK_ARG(u && f && out && out != u && out != f && aligned16(u) && aligned16(f) && aligned16(out), "mg3_dev_jacobi: bad pointer");
  d3_jacobi(dtype, u, f, out, level_of(nx, ny, nz, ld, hx, hy, hz), sigma, omega, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}
int mg3_dev_rbgs_colour(int dtype, int nx, int ny, int nz, int ld, double hx, double hy, double hz, double sigma, double omega, int colour,
                        int colour_offset, void* u, const void* f, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && shape_ok(nx, ny, nz) && ld_ok3(nz, ld), "mg3_dev_rbgs_colour: bad dtype / shape / pitch");
  CHECK_ARG(spacing_ok(hx, hy, hz) && sigma_ok(sigma) && std::isfinite(omega), "mg3_dev_rbgs_colour: bad spacing / sigma / omega");
  CHECK_ARG((colour == 0 || colour == 1) && (colour_offset == 0 || colour_offset == 1), "mg3_dev_rbgs_colour: colour and colour_offset are 0 or 1");
  CHECK_ARG(u && f && u != f && aligned16(u) && aligned16(f), "mg3_dev_rbgs_colour: bad pointer");
  d3_colour(dtype, u, f, level_of(nx, ny, nz, ld, hx, hy, hz), sigma, omega, colour, colour_offset, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}
static bool transfer_shape_ok(int nxf, int nyf, int nzf) {
  return shape_ok(nxf, nyf, nzf) && nxf >= 5 && nyf >= 5 && nzf >= 5 && nxf % 2 && nyf % 2 && nzf % 2;
}
int mg3_dev_restrict(int dtype, int nxf, int nyf, int nzf, int ldf, int ldc, const void* fine, void* coarse, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && transfer_shape_ok(nxf, nyf, nzf), "mg3_dev_restrict: the fine extents are odd and >= 5");
  CHECK_ARG(ld_ok3(nzf, ldf) && ld_ok3((nzf + 1) / 2, ldc), "mg3_dev_restrict: bad pitch");
  CHECK_ARG(fine && coarse && fine != coarse && aligned16(fine) && aligned16(coarse), "mg3_dev_restrict: bad pointer");
  d3_restrict(dtype, fine, coarse, level_of(nxf, nyf, nzf, ldf, 1, 1, 1), level_of((nxf + 1) / 2, (nyf + 1) / 2, (nzf + 1) / 2, ldc, 1, 1, 1),
              (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}
int mg3_dev_prolong_add(int dtype, int nxf, int nyf, int nzf, int ldf, int ldc, const void* e_coarse, void* u_fine, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && transfer_shape_ok(nxf, nyf, nzf), "mg3_dev_prolong_add: the fine extents are odd and >= 5");
  CHECK_ARG(ld_ok3(nzf, ldf) && ld_ok3((nzf + 1) / 2, ldc), "mg3_dev_prolong_add: bad pitch");
  CHECK_ARG(e_coarse && u_fine && e_coarse != u_fine && aligned16(e_coarse) && aligned16(u_fine), "mg3_dev_prolong_add: bad pointer");
  d3_prolong_add(dtype, e_coarse, u_fine, level_of(nxf, nyf, nzf, ldf, 1, 1, 1),
                 level_of((nxf + 1) / 2, (nyf + 1) / 2, (nzf + 1) / 2, ldc, 1, 1, 1), (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}
int mg3_dev_upcast_add(int nx, int ny, int nz, int ld64, int ld32, const float* e32, double* u64, void* stream) {
  CHECK_ARG(shape_ok(nx, ny, nz) && ld_ok3(nz, ld64) && ld_ok3(nz, ld32), "mg3_dev_upcast_add: bad shape / pitch");
  CHECK_ARG(e32 && u64 && aligned16(e32) && aligned16(u64), "mg3_dev_upcast_add: bad pointer");
  d3_upcast_add(e32, u64, nx, ny, nz, ld64, ld32, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}
int mg3_dev_norm(int dtype, int nx, int ny, int nz, int ld, const void* field, void* scratch, double* sumsq_dev, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && shape_ok(nx, ny, nz) && ld_ok3(nz, ld), "mg3_dev_norm: bad dtype / shape / pitch");
  CHECK_ARG(field && scratch && sumsq_dev && aligned16(field) && aligned16(scratch), "mg3_dev_norm: bad pointer");
  const int n = d3_sumsq(dtype, field, (double*)scratch, nx, ny, nz, ld, (hipStream_t)stream);
  d3_reduce((const double*)scratch, n, sumsq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}
int mg3_dev_coarse_solve(int dtype, int nx, int ny, int nz, int ld, double hx, double hy, double hz, double sigma, int sweeps, void* u,
                         const void* f, int* used_lds, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && shape_ok(nx, ny, nz) && ld_ok3(nz, ld) && sweeps >= 0, "mg3_dev_coarse_solve: bad dtype / shape / pitch / sweeps");
  CHECK_ARG(spacing_ok(hx, hy, hz) && sigma_ok(sigma), "mg3_dev_coarse_solve: bad spacing / sigma");
  CHECK_ARG(u && f && u != f && aligned16(u) && aligned16(f), "mg3_dev_coarse_solve: bad pointer");
  bool lds = false;
  const int rc = d3_coarse_solve(dtype, u, f, level_of(nx, ny, nz, ld, hx, hy, hz), sigma, sweeps, &lds, (hipStream_t)stream);
  if (rc != MG_OK) return rc;
  if (used_lds) *used_lds = lds ? 1 : 0;
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

}  // extern "C"
