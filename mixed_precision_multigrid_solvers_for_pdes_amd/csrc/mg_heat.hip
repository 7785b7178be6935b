// The time stepper of libmghip.so: device-resident heat-equation steps  du/dt = alpha div(a grad u) + g(t) S(x, y)  (explicit and
// implicit Euler, Crank-Nicolson, BDF2; a == 1 unless mg_heat_set_coefficient gave a field) on top of the multigrid engine
// (include/mghip.h, "Time stepping"; include/mghip_heat.h for the field and the PCG inner solver).  This unit instantiates the kernels of mg_heat_kernels.hpp and holds the driver; the
// inner solver is an mg_handle of its own, driven through the device entry points of the C ABI (mg_set_rhs_device /
// mg_update_rhs_device, mg_set_shift, mg_iterate, mg_get_solution_device) on the engine's stream, where the stepper queues its
// own kernels too -- or an mg_pcg of its own (MG_HEAT_INNER_PCG), whose engine's stream then carries the stepper's work.
//
//   implicit step:  f = rhs(u_src [, u_prev]) and sum f^2  ->  engine rhs  ->  shift lambda  ->  initial guess u_src (or u_src
//   with the new ring)  ->  cycles until ||r|| < tol max(1, ||f||)  ->  u_dst  [-> ring of u_dst]
//   with PCG:       f and sum f^2  ->  shift lambda  ->  u_dst = the initial guess  ->  mg_pcg_solve_device(f, u_dst) to the same
//   tolerance  [-> ring of u_dst]
//
// The state lives in four slots; a step reads one (two for BDF2) and writes another, so step doubling and multistep schemes
// need no copy and no field crosses PCIe between steps.
#include "mg_host.hpp"
#include "mg_heat_kernels.hpp"

using namespace mgh;

namespace {
constexpr int kSlots = 4;
}

struct mg_heat {
  mg_config cfg;
  mg_handle* eng = nullptr;             // the inner engine: the stepper's own, or (inner == MG_HEAT_INNER_PCG) the one `pcg` owns
  mg_pcg* pcg = nullptr;
  int inner = MG_HEAT_INNER_CYCLE;
  int nx = 0, ny = 0, ld = 0;
  double hx = 0, hy = 0, alpha = 0;
  double* slot[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  double* rhs = nullptr;
  double* src = nullptr;                // source profile S (nullable)
  double* a = nullptr;                  // diffusivity field (nullable: the constant operator)
  double* partials = nullptr;
  double* d_sum = nullptr;              // device, one double
  double* h_sum = nullptr;              // pinned host
  double lambda = -1.0;                 // the shift the engine carries (< 0: none set yet)
  bool eng_has_rhs = false;
  std::vector<double> hist;
  std::string err;
};

namespace {

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
bool ld_ok(int ny, int ld) { return ld >= ny && ld % 2 == 0; }
// do the fields a and b (nx rows of pitch ld; b may be NULL) share an element?
bool overlap(const double* a, const double* b, int nx, int ld) {
  const uintptr_t n = (uintptr_t)nx * (uintptr_t)ld * sizeof(double), pa = (uintptr_t)a, pb = (uintptr_t)b;
  return b && pa < pb + n && pb < pa + n;
}

mg::TileGeom heat_geom(int nx, int ny, int ld) {
  using S = mg::TileShape<double>;
  mg::TileGeom g;
  g.nx = nx; g.ny = ny; g.ld = ld;
  g.nyv = std::min(ld, (ny + S::N - 1) / S::N * S::N);
  g.i_org = 0;                                             // the ring rows are stored too
  g.tiles_j = (ny + S::TJ - 1) / S::TJ;
  g.ntiles = (nx + mg::kTI - 1) / mg::kTI * g.tiles_j;
  return g;
}

// ---- launchers (shared by the driver and the stateless mg_dev_heat_* forms); an int result is the number of partials ----
template <int SCHEME>
int launch_rhs_scheme(const double* u, const double* u_prev, const double* src, const double* a, double* out, double* partials,
                      const mg::TileGeom& g, const mg::HeatCoef& c, hipStream_t st) {
  auto k = src ? mg::heat_rhs_kernel<SCHEME, true> : mg::heat_rhs_kernel<SCHEME, false>;
  if constexpr (SCHEME == mg::kHeatExplicit || SCHEME == mg::kHeatCn) {      // the schemes that evaluate the operator
    if (a) k = src ? mg::heat_rhs_kernel<SCHEME, true, true> : mg::heat_rhs_kernel<SCHEME, false, true>;
  }
  hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, u, u_prev, src, a, out, partials, g, c);
  return g.ntiles;
}

// a: the diffusivity field or NULL (implicit Euler and BDF2 launch the same kernels either way: no operator in their f)
int launch_rhs(int scheme, int nx, int ny, int ld, double hx, double hy, double alpha, double dt, const double* u,
               const double* u_prev, const double* src, const double* a, double g0, double g1, double* out, double* partials,
               hipStream_t st) {
  const mg::TileGeom g = heat_geom(nx, ny, ld);
  const Coef k = coefs(hx, hy);
  mg::HeatCoef c;
  c.ihx2 = k.ihx2; c.ihy2 = k.ihy2; c.diag = k.diag;
  c.a = alpha; c.dt = dt;
  c.dta = dt * alpha;
  c.two_dta = 2 * dt * alpha;
  c.g0 = g0; c.g1 = g1;
  switch (scheme) {
    case MG_HEAT_EXPLICIT_EULER: return launch_rhs_scheme<mg::kHeatExplicit>(u, u_prev, src, a, out, partials, g, c, st);
    case MG_HEAT_IMPLICIT_EULER: return launch_rhs_scheme<mg::kHeatImplicit>(u, u_prev, src, a, out, partials, g, c, st);
    case MG_HEAT_CRANK_NICOLSON: return launch_rhs_scheme<mg::kHeatCn>(u, u_prev, src, a, out, partials, g, c, st);
    default: return launch_rhs_scheme<mg::kHeatBdf2>(u, u_prev, src, a, out, partials, g, c, st);
  }
}

void launch_ring(double* u, int nx, int ny, int ld, const double* edge4, hipStream_t st) {
  const int nb = std::max(1, std::min(64, (2 * (nx + ny) + mg::kBlock - 1) / mg::kBlock));
  hipLaunchKernelGGL(mg::heat_ring_kernel, dim3(nb), dim3(mg::kBlock), 0, st, u, nx, ny, ld, edge4[0], edge4[1], edge4[2], edge4[3]);
}

int launch_diff(const double* a, const double* b, double* partials, int nx, int ny, int ld, hipStream_t st) {
  const int nyv = heat_geom(nx, ny, ld).nyv;
  const long long vecs = (long long)nx * (nyv / 2);
  const int nb = (int)std::max<long long>(1, std::min<long long>((vecs + mg::kBlock - 1) / mg::kBlock, 1024));
  hipLaunchKernelGGL(mg::heat_diff_sumsq_kernel, dim3(nb), dim3(mg::kBlock), 0, st, a, b, partials, nx, ny, nyv, ld);
  return nb;
}

void launch_sum(const double* partials, int n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(mg::heat_reduce_kernel, dim3(1), dim3(mg::kReduceBlock), 0, st, partials, n, out);
}

int hfail(mg_heat* s, int code, const std::string& msg) { return fail(s ? &s->err : nullptr, code, msg); }

// the engine's message joins the stepper's
int eng_rc(mg_heat* s, int rc) {
  if (rc != MG_OK) hfail(s, rc, std::string("inner solver: ") + mg_last_error(s->eng));
  return rc;
}
#define ENG(call) do { const int rc_ = eng_rc(s, (call)); if (rc_ != MG_OK) return rc_; } while (0)
int pcg_rc(mg_heat* s, int rc) {
  if (rc != MG_OK) hfail(s, rc, std::string("inner solver: ") + mg_pcg_last_error(s->pcg));
  return rc;
}
#define PCG(call) do { const int rc_ = pcg_rc(s, (call)); if (rc_ != MG_OK) return rc_; } while (0)

void release(mg_heat* s) {
  if (s->pcg) { (void)mg_pcg_destroy(s->pcg); s->pcg = nullptr; s->eng = nullptr; }      // the engine goes with its owner
  if (s->eng) { (void)mg_destroy(s->eng); s->eng = nullptr; }
  for (double** p : {&s->slot[0], &s->slot[1], &s->slot[2], &s->slot[3], &s->rhs, &s->src, &s->a, &s->partials, &s->d_sum})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (s->h_sum) { (void)hipHostFree(s->h_sum); s->h_sum = nullptr; }
}

size_t field_bytes(const mg_heat* s) { return (size_t)s->nx * s->ld * sizeof(double); }
bool slot_ok(int k) { return k >= 0 && k < kSlots; }

// host array (nx, ny) of hdt -> fp64 device field with the stepper's pitch, on the engine's stream (through its staging field)
int upload(mg_heat* s, double* dev, const void* host, int hdt) {
  hipStream_t st = s->eng->stream;
  const size_t es = esize(hdt);
  if (hdt == MG_F64) {
    HIPC(&s->err, hipMemcpy2DAsync(dev, (size_t)s->ld * 8, host, (size_t)s->ny * 8, (size_t)s->ny * 8, s->nx, hipMemcpyHostToDevice, st));
  } else {
    int lds = 0;
    (void)mg_pitch_elems(hdt, s->ny, &lds);
    HIPC(&s->err, hipMemcpy2DAsync(s->eng->staging, (size_t)lds * es, host, (size_t)s->ny * es, (size_t)s->ny * es, s->nx, hipMemcpyHostToDevice, st));
    const int rc = mg_dev_convert(hdt, MG_F64, s->nx, s->ny, lds, s->ld, s->eng->staging, dev, st);
    if (rc != MG_OK) return hfail(s, rc, mg_last_error(nullptr));
  }
  HIPC(&s->err, hipStreamSynchronize(st));      // the caller's array may go away
  return MG_OK;
}

int implicit_step(mg_heat* s, int scheme, double dt, int src, int prev, int dst, double g0, double g1, const double* edge4,
                  int bc_before_solve, double tol, int max_cycles, mg_heat_step_info* info) {
  hipStream_t st = s->eng->stream;
  const double dta = dt * s->alpha;
  const double lambda = scheme == MG_HEAT_IMPLICIT_EULER ? 1.0 / dta : scheme == MG_HEAT_CRANK_NICOLSON ? 2.0 / dta : 3.0 / (2 * dt * s->alpha);
  const int np = launch_rhs(scheme, s->nx, s->ny, s->ld, s->hx, s->hy, s->alpha, dt, s->slot[src], prev >= 0 ? s->slot[prev] : nullptr,
                            s->src, s->a, g0, g1, s->rhs, s->partials, st);
  launch_sum(s->partials, np, s->d_sum, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sum, s->d_sum, sizeof(double), hipMemcpyDeviceToHost, st));
  if (s->pcg) {
    // the conjugate-gradient loop iterates in place: dst := the initial guess (src, or src with the new ring), then the solve
    if (lambda != s->lambda) { PCG(mg_pcg_set_shift(s->pcg, lambda)); s->lambda = lambda; }
    HIPC(&s->err, hipMemcpyAsync(s->slot[dst], s->slot[src], field_bytes(s), hipMemcpyDeviceToDevice, st));
    if (bc_before_solve) launch_ring(s->slot[dst], s->nx, s->ny, s->ld, edge4, st);
    HIPC(&s->err, hipGetLastError());
    HIPC(&s->err, hipStreamSynchronize(st));                      // sum f^2 has arrived
    const double fnorm = std::sqrt(s->hx * s->hy * *s->h_sum);
    if ((int)s->hist.size() < max_cycles) s->hist.resize(max_cycles);
    int n = 0, conv = 0;
    mg_pcg_stats stats;
    PCG(mg_pcg_solve_device(s->pcg, s->rhs, s->ld, s->slot[dst], s->ld, MG_F64, tol * std::max(1.0, fnorm), max_cycles,
                            s->hist.data(), max_cycles, &n, &conv, &stats));
    if (!bc_before_solve && edge4) launch_ring(s->slot[dst], s->nx, s->ny, s->ld, edge4, st);
    HIPC(&s->err, hipGetLastError());
    if (info) {
      info->lambda = lambda;
      info->rhs_norm = fnorm;
      info->initial_residual = stats.initial_residual;
      info->final_residual = n > 0 ? s->hist[n - 1] : stats.initial_residual;
      info->solve_seconds = stats.solve_seconds;
      info->cycles = n;
      info->converged = conv;                                      // a breakdown (stats.status == 2) ends the solve unconverged
    }
    return MG_OK;
  }
  if (!s->eng_has_rhs) {
    ENG(mg_set_rhs_device(s->eng, s->rhs, s->ld, MG_F64));
    rhs_ring_is_zero(s->eng);      // f has a zero ring by construction: mg_iterate runs the loop mg_solve runs after an upload
    s->eng_has_rhs = true;
  } else {
    ENG(mg_update_rhs_device(s->eng, s->rhs, s->ld, MG_F64));
  }
  if (lambda != s->lambda) { ENG(mg_set_shift(s->eng, lambda)); s->lambda = lambda; }
  const double* guess = s->slot[src];
  if (bc_before_solve) {
    HIPC(&s->err, hipMemcpyAsync(s->slot[dst], s->slot[src], field_bytes(s), hipMemcpyDeviceToDevice, st));
    launch_ring(s->slot[dst], s->nx, s->ny, s->ld, edge4, st);
    HIPC(&s->err, hipGetLastError());
    guess = s->slot[dst];
  }
  ENG(set_u_device_impl(s->eng, guess, s->ld, MG_F64));
  HIPC(&s->err, hipStreamSynchronize(st));                        // sum f^2 has arrived
  const double fnorm = std::sqrt(s->hx * s->hy * *s->h_sum);
  if ((int)s->hist.size() < max_cycles) s->hist.resize(max_cycles);
  int n = 0, conv = 0;
  mg_stats stats;
  ENG(mg_iterate(s->eng, tol * std::max(1.0, fnorm), max_cycles, s->hist.data(), max_cycles, &n, &conv, nullptr, &stats));
  ENG(mg_get_solution_device(s->eng, s->slot[dst], s->ld, MG_F64));
  if (!bc_before_solve && edge4) launch_ring(s->slot[dst], s->nx, s->ny, s->ld, edge4, st);
  HIPC(&s->err, hipGetLastError());
  if (info) {
    info->lambda = lambda;
    info->rhs_norm = fnorm;
    info->initial_residual = stats.initial_residual;
    info->final_residual = n > 0 ? s->hist[n - 1] : stats.initial_residual;
    info->solve_seconds = stats.solve_seconds;
    info->cycles = n;
    info->converged = conv;
  }
  return MG_OK;
}

}  // namespace

#define CHECK_DEV(cond, msg) do { if (!(cond)) return fail(nullptr, MG_ERR_INVALID_VALUE, msg); } while (0)

extern "C" {

int mg_heat_create(const mg_config* cfg, double alpha, mg_heat** out) {
  return mg_heat_create_ex(cfg, alpha, MG_HEAT_INNER_CYCLE, 0, 0, out);
}

int mg_heat_create_ex(const mg_config* cfg, double alpha, int inner, int num_cycles, int flexible, mg_heat** out) {
  if (!cfg || !out) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_create: NULL argument");
  *out = nullptr;
  if (inner != MG_HEAT_INNER_CYCLE && inner != MG_HEAT_INNER_PCG) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_create: unknown inner solver");
  if (inner == MG_HEAT_INNER_CYCLE && cfg->precision != MG_PREC_DOUBLE)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_create: the inner solver runs in MG_PREC_DOUBLE");
  if (inner == MG_HEAT_INNER_PCG && cfg->precision != MG_PREC_DOUBLE && cfg->precision != MG_PREC_SINGLE_MANAGED &&
      cfg->precision != MG_PREC_MIXED_LEVELS)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_create: the preconditioner of the PCG inner solver runs in MG_PREC_DOUBLE, MG_PREC_SINGLE_MANAGED or MG_PREC_MIXED_LEVELS");
  if (cfg->coeff != -1.0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_create: coeff must be -1 (the steps solve (-Laplacian + lambda) u = f)");
  if (cfg->fmg_cycles != 0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_create: fmg_cycles must be 0 (a step starts from the old time level)");
  if (!(alpha > 0.0) || !std::isfinite(alpha)) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_create: alpha must be finite and > 0");
  mg_handle* eng = nullptr;
  mg_pcg* pcg = nullptr;
  int rc = inner == MG_HEAT_INNER_PCG ? mg_pcg_create(cfg, num_cycles, flexible, &pcg) : mg_create(cfg, &eng);
  if (rc != MG_OK) return rc;
  if (pcg) eng = pcg_engine(pcg);
  mg_heat* s = new mg_heat();
  s->cfg = *cfg;
  s->eng = eng;
  s->pcg = pcg;
  s->inner = inner;
  s->nx = cfg->nx; s->ny = cfg->ny;
  (void)mg_pitch_elems(MG_F64, cfg->ny, &s->ld);
  s->hx = eng->lv[0].hx; s->hy = eng->lv[0].hy;
  s->alpha = alpha;
  auto bail = [&](int code) { release(s); const std::string m = s->err; delete s; last_error() = m; return code; };
  hipStream_t st = eng->stream;
  for (double** p : {&s->slot[0], &s->slot[1], &s->slot[2], &s->slot[3], &s->rhs})
    if ((rc = alloc_zero(&s->err, (void**)p, field_bytes(s), st)) != MG_OK) return bail(rc);
  int64_t scratch = 0;
  (void)mg_dev_scratch_bytes(s->nx, s->ny, &scratch);
  if ((rc = alloc_zero(&s->err, (void**)&s->partials, (size_t)scratch, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->d_sum, sizeof(double), st)) != MG_OK) return bail(rc);
  if (hipHostMalloc((void**)&s->h_sum, sizeof(double)) != hipSuccess) { s->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  if (hipStreamSynchronize(st) != hipSuccess) { s->err = "hipStreamSynchronize failed"; return bail(MG_ERR_HIP); }
  *out = s;
  return MG_OK;
}

int mg_heat_destroy(mg_heat* s) {
  if (!s) return MG_OK;
  (void)hipSetDevice(s->cfg.device);
  if (s->eng && s->eng->stream) (void)hipStreamSynchronize(s->eng->stream);
  release(s);
  delete s;
  return MG_OK;
}

const char* mg_heat_last_error(const mg_heat* s) { return s ? s->err.c_str() : last_error().c_str(); }

int mg_heat_set_slot(mg_heat* s, int slot, const void* u_host, int host_dtype) {
  if (!s || !u_host || !valid_dtype(host_dtype) || !slot_ok(slot)) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_slot: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  return upload(s, s->slot[slot], u_host, host_dtype);
}

int mg_heat_get_slot(mg_heat* s, int slot, void* u_host, int host_dtype) {
  if (!s || !u_host || !valid_dtype(host_dtype) || !slot_ok(slot)) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_get_slot: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  return download(&s->err, u_host, host_dtype, s->slot[slot], MG_F64, s->ld, s->nx, s->ny, s->eng->staging, s->eng->stream);
}

int mg_heat_set_slot_device(mg_heat* s, int slot, const void* u_dev, int ld, int dtype) {
  if (!s || !u_dev || !valid_dtype(dtype) || !slot_ok(slot) || ld < s->ny) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_slot_device: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  const int rc = mg_dev_convert(dtype, MG_F64, s->nx, s->ny, ld, s->ld, u_dev, s->slot[slot], s->eng->stream);
  if (rc != MG_OK) return hfail(s, rc, mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
  return MG_OK;
}

int mg_heat_get_slot_device(mg_heat* s, int slot, void* u_dev, int ld, int dtype) {
  if (!s || !u_dev || !valid_dtype(dtype) || !slot_ok(slot) || ld < s->ny) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_get_slot_device: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  const int rc = mg_dev_convert(MG_F64, dtype, s->nx, s->ny, s->ld, ld, s->slot[slot], u_dev, s->eng->stream);
  if (rc != MG_OK) return hfail(s, rc, mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
  return MG_OK;
}

int mg_heat_set_source(mg_heat* s, const void* profile_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_source: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  if (!profile_host_or_null) {
    HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
    if (s->src) { (void)hipFree(s->src); s->src = nullptr; }
    return MG_OK;
  }
  if (!s->src) { const int rc = alloc_zero(&s->err, (void**)&s->src, field_bytes(s), s->eng->stream); if (rc != MG_OK) return rc; }
  return upload(s, s->src, profile_host_or_null, host_dtype);
}

int mg_heat_set_coefficient(mg_heat* s, const void* a_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_coefficient: bad argument");
  if (a_host_or_null) {                                           // before any device work
    const size_t n = (size_t)s->nx * s->ny;
    bool ok = true;
    if (host_dtype == MG_F64) { const double* p = (const double*)a_host_or_null; for (size_t k = 0; k < n && ok; ++k) ok = std::isfinite(p[k]) && p[k] > 0.0; }
    else { const float* p = (const float*)a_host_or_null; for (size_t k = 0; k < n && ok; ++k) ok = std::isfinite(p[k]) && p[k] > 0.0f; }
    if (!ok) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_coefficient: the diffusivity field must be finite and > 0 everywhere");
  }
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  if (s->pcg) PCG(mg_pcg_set_coefficient(s->pcg, a_host_or_null, host_dtype));
  else ENG(mg_set_coefficient(s->eng, a_host_or_null, host_dtype));
  // what the inner solver cached for the old operator goes: the shift (and with it the reciprocal diagonals) is set again by
  // the next implicit step, which hands the engine its right-hand side the way a first step does
  s->lambda = -1.0;
  s->eng_has_rhs = false;
  if (!a_host_or_null) {
    HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
    if (s->a) { (void)hipFree(s->a); s->a = nullptr; }
    return MG_OK;
  }
  if (!s->a) { const int rc = alloc_zero(&s->err, (void**)&s->a, field_bytes(s), s->eng->stream); if (rc != MG_OK) return rc; }
  return upload(s, s->a, a_host_or_null, host_dtype);
}

int mg_heat_step(mg_heat* s, int scheme, double dt, int src, int prev, int dst, double g0, double g1, const double* edge4_or_null,
                 int bc_before_solve, double tol, int max_cycles, mg_heat_step_info* info) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_step: NULL stepper");
  if (scheme < MG_HEAT_EXPLICIT_EULER || scheme > MG_HEAT_BDF2) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: unknown scheme");
  if (!(dt > 0.0) || !std::isfinite(dt)) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: dt must be finite and > 0");
  if (!slot_ok(src) || !slot_ok(dst) || src == dst) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: src and dst are two different slots 0..3");
  if (scheme == MG_HEAT_BDF2) {
    if (!slot_ok(prev) || prev == dst) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: BDF2 reads a prev slot 0..3 other than dst");
  } else if (prev != -1) {
    return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: prev is -1 unless the scheme is BDF2");
  }
  if (!std::isfinite(g0) || !std::isfinite(g1)) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: g0 / g1 not finite");
  if (bc_before_solve && !edge4_or_null) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: bc_before_solve needs edge values");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  if (scheme == MG_HEAT_EXPLICIT_EULER) {
    hipStream_t st = s->eng->stream;
    (void)launch_rhs(scheme, s->nx, s->ny, s->ld, s->hx, s->hy, s->alpha, dt, s->slot[src], nullptr, s->src, s->a, g0, g1,
                     s->slot[dst], s->partials, st);
    if (edge4_or_null) launch_ring(s->slot[dst], s->nx, s->ny, s->ld, edge4_or_null, st);
    HIPC(&s->err, hipGetLastError());
    if (info) { *info = mg_heat_step_info{}; info->converged = 1; }
    return MG_OK;
  }
  if (max_cycles < 1 || !(tol == tol)) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: max_cycles < 1 / tol is NaN");
  return implicit_step(s, scheme, dt, src, prev, dst, g0, g1, edge4_or_null, bc_before_solve, tol, max_cycles, info);
}

int mg_heat_diff_norm(mg_heat* s, int slot_a, int slot_b, double* out) {
  if (!s || !out || !slot_ok(slot_a) || !slot_ok(slot_b)) return hfail(s, MG_ERR_INVALID_VALUE, "mg_heat_diff_norm: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  hipStream_t st = s->eng->stream;
  const int n = launch_diff(s->slot[slot_a], s->slot[slot_b], s->partials, s->nx, s->ny, s->ld, st);
  launch_sum(s->partials, n, s->d_sum, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sum, s->d_sum, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(&s->err, hipStreamSynchronize(st));
  *out = std::sqrt(*s->h_sum);
  return MG_OK;
}

// ---- the field kernels, call by call (pitch in elements, nullable stream, scratch >= mg_dev_scratch_bytes()) ----
int mg_dev_heat_rhs(int scheme, int nx, int ny, int ld, double hx, double hy, double alpha, double dt, const double* u,
                    const double* u_prev_or_null, const double* src_or_null, double g0, double g1, double* out, void* scratch,
                    double* sumsq_dev_or_null, void* stream) {
  return mg_dev_heat_rhs_var(scheme, nx, ny, ld, hx, hy, alpha, dt, u, u_prev_or_null, src_or_null, nullptr, g0, g1, out, scratch,
                             sumsq_dev_or_null, stream);
}

int mg_dev_heat_rhs_var(int scheme, int nx, int ny, int ld, double hx, double hy, double alpha, double dt, const double* u,
                        const double* u_prev_or_null, const double* src_or_null, const double* a_or_null, double g0, double g1,
                        double* out, void* scratch, double* sumsq_dev_or_null, void* stream) {
  CHECK_DEV(scheme >= MG_HEAT_EXPLICIT_EULER && scheme <= MG_HEAT_BDF2, "mg_dev_heat_rhs: unknown scheme");
  CHECK_DEV(nx >= 3 && ny >= 3 && ld_ok(ny, ld), "mg_dev_heat_rhs: bad shape / pitch");
  CHECK_DEV(dt > 0.0 && std::isfinite(dt) && alpha > 0.0 && std::isfinite(alpha) && hx > 0.0 && hy > 0.0, "mg_dev_heat_rhs: dt, alpha and the spacings must be finite and > 0");
  CHECK_DEV(u && out && scratch, "mg_dev_heat_rhs: NULL pointer");
  CHECK_DEV(scheme != MG_HEAT_BDF2 || u_prev_or_null, "mg_dev_heat_rhs: BDF2 needs u_prev");
  CHECK_DEV(!overlap(out, u, nx, ld) && !overlap(out, u_prev_or_null, nx, ld) && !overlap(out, src_or_null, nx, ld) &&
            !overlap(out, a_or_null, nx, ld), "mg_dev_heat_rhs: out is an array of its own (it overlaps an input)");
  CHECK_DEV(aligned16(u) && aligned16(out) && aligned16(u_prev_or_null) && aligned16(src_or_null) && aligned16(a_or_null),
            "mg_dev_heat_rhs: unaligned pointer");
  const int n = launch_rhs(scheme, nx, ny, ld, hx, hy, alpha, dt, u, scheme == MG_HEAT_BDF2 ? u_prev_or_null : nullptr, src_or_null,
                           a_or_null, g0, g1, out, (double*)scratch, (hipStream_t)stream);
  if (sumsq_dev_or_null) launch_sum((double*)scratch, n, sumsq_dev_or_null, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_heat_ring(int nx, int ny, int ld, const double edge4[4], double* u, void* stream) {
  CHECK_DEV(nx >= 3 && ny >= 3 && ld_ok(ny, ld), "mg_dev_heat_ring: bad shape / pitch");
  CHECK_DEV(edge4 && u, "mg_dev_heat_ring: NULL pointer");
  launch_ring(u, nx, ny, ld, edge4, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_heat_diff_sumsq(int nx, int ny, int ld, const double* a, const double* b, void* scratch, double* sumsq_dev, void* stream) {
  CHECK_DEV(nx >= 3 && ny >= 3 && ld_ok(ny, ld), "mg_dev_heat_diff_sumsq: bad shape / pitch");
  CHECK_DEV(a && b && scratch && sumsq_dev, "mg_dev_heat_diff_sumsq: NULL pointer");
  CHECK_DEV(aligned16(a) && aligned16(b), "mg_dev_heat_diff_sumsq: unaligned pointer");
  const int n = launch_diff(a, b, (double*)scratch, nx, ny, ld, (hipStream_t)stream);
  launch_sum((double*)scratch, n, sumsq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

}  // extern "C"
