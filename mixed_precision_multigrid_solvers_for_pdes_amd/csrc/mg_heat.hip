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
  const mg::TileGeom g = field_geom(nx, ny, ld);
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
  const int nyv = field_geom(nx, ny, ld).nyv;
  const long long vecs = (long long)nx * (nyv / 2);
  const int nb = (int)std::max<long long>(1, std::min<long long>((vecs + mg::kBlock - 1) / mg::kBlock, 1024));
  hipLaunchKernelGGL(mg::heat_diff_sumsq_kernel, dim3(nb), dim3(mg::kBlock), 0, st, a, b, partials, nx, ny, nyv, ld);
  return nb;
}

void launch_sum(const double* partials, int n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(mg::reduce_rows_kernel<false>, dim3(1), dim3(mg::kReduceBlock), 0, st, partials, n, 0, 0, out);
}

void release(mg_heat* s) {
  if (s->pcg) { (void)mg_pcg_destroy(s->pcg); s->pcg = nullptr; s->eng = nullptr; }      // the engine goes with its owner
  if (s->eng) { (void)mg_destroy(s->eng); s->eng = nullptr; }
  for (double** p : {&s->slot[0], &s->slot[1], &s->slot[2], &s->slot[3], &s->rhs, &s->src, &s->a, &s->partials, &s->d_sum})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (s->h_sum) { (void)hipHostFree(s->h_sum); s->h_sum = nullptr; }
}

bool slot_ok(int k) { return k >= 0 && k < kSlots; }

// host array (nx, ny) of hdt -> fp64 device field with the stepper's pitch, on the engine's stream (through its staging field)
int put(mg_heat* s, double* dev, const void* host, int hdt) {
  return upload(&s->err, dev, MG_F64, s->ld, host, hdt, s->nx, s->ny, s->eng->staging, s->eng->stream);
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
    if (lambda != s->lambda) { OWNED(mg_pcg_set_shift(s->pcg, lambda), "inner solver: ", mg_pcg_last_error(s->pcg)); s->lambda = lambda; }
    HIPC(&s->err, hipMemcpyAsync(s->slot[dst], s->slot[src], field_bytes(s), hipMemcpyDeviceToDevice, st));
    if (bc_before_solve) launch_ring(s->slot[dst], s->nx, s->ny, s->ld, edge4, st);
    HIPC(&s->err, hipGetLastError());
    HIPC(&s->err, hipStreamSynchronize(st));                      // sum f^2 has arrived
    const double fnorm = std::sqrt(s->hx * s->hy * *s->h_sum);
    if ((int)s->hist.size() < max_cycles) s->hist.resize(max_cycles);
    int n = 0, conv = 0;
    mg_pcg_stats stats;
    OWNED(mg_pcg_solve_device(s->pcg, s->rhs, s->ld, s->slot[dst], s->ld, MG_F64, tol * std::max(1.0, fnorm), max_cycles,
                            s->hist.data(), max_cycles, &n, &conv, &stats), "inner solver: ", mg_pcg_last_error(s->pcg));
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
  // f has a zero ring by construction: mg_iterate runs the loop mg_solve runs after an upload
  OWNED(engine_set_rhs(s->eng, &s->eng_has_rhs, s->rhs, s->ld, true), "inner solver: ", mg_last_error(s->eng));
  if (lambda != s->lambda) { OWNED(mg_set_shift(s->eng, lambda), "inner solver: ", mg_last_error(s->eng)); s->lambda = lambda; }
  const double* guess = s->slot[src];
  if (bc_before_solve) {
    HIPC(&s->err, hipMemcpyAsync(s->slot[dst], s->slot[src], field_bytes(s), hipMemcpyDeviceToDevice, st));
    launch_ring(s->slot[dst], s->nx, s->ny, s->ld, edge4, st);
    HIPC(&s->err, hipGetLastError());
    guess = s->slot[dst];
  }
  OWNED(set_u_device_impl(s->eng, guess, s->ld, MG_F64), "inner solver: ", mg_last_error(s->eng));
  HIPC(&s->err, hipStreamSynchronize(st));                        // sum f^2 has arrived
  const double fnorm = std::sqrt(s->hx * s->hy * *s->h_sum);
  if ((int)s->hist.size() < max_cycles) s->hist.resize(max_cycles);
  int n = 0, conv = 0;
  mg_stats stats;
  OWNED(mg_iterate(s->eng, tol * std::max(1.0, fnorm), max_cycles, s->hist.data(), max_cycles, &n, &conv, nullptr, &stats), "inner solver: ", mg_last_error(s->eng));
  OWNED(mg_get_solution_device(s->eng, s->slot[dst], s->ld, MG_F64), "inner solver: ", mg_last_error(s->eng));
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
  auto bail = [&](int code) { return create_fail(s, release, code); };
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
  return destroy_owned(s, s && s->eng ? s->eng->stream : nullptr, release);
}

const char* mg_heat_last_error(const mg_heat* s) { return s ? s->err.c_str() : last_error().c_str(); }

int mg_heat_set_slot(mg_heat* s, int slot, const void* u_host, int host_dtype) {
  if (!s || !u_host || !valid_dtype(host_dtype) || !slot_ok(slot)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_slot: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  return put(s, s->slot[slot], u_host, host_dtype);
}

int mg_heat_get_slot(mg_heat* s, int slot, void* u_host, int host_dtype) {
  if (!s || !u_host || !valid_dtype(host_dtype) || !slot_ok(slot)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_get_slot: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  return download(&s->err, u_host, host_dtype, s->slot[slot], MG_F64, s->ld, s->nx, s->ny, s->eng->staging, s->eng->stream);
}

int mg_heat_set_slot_device(mg_heat* s, int slot, const void* u_dev, int ld, int dtype) {
  if (!s || !u_dev || !valid_dtype(dtype) || !slot_ok(slot) || ld < s->ny) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_slot_device: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_dev_convert(dtype, MG_F64, s->nx, s->ny, ld, s->ld, u_dev, s->slot[slot], s->eng->stream), "", mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
  return MG_OK;
}

int mg_heat_get_slot_device(mg_heat* s, int slot, void* u_dev, int ld, int dtype) {
  if (!s || !u_dev || !valid_dtype(dtype) || !slot_ok(slot) || ld < s->ny) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_get_slot_device: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_dev_convert(MG_F64, dtype, s->nx, s->ny, s->ld, ld, s->slot[slot], u_dev, s->eng->stream), "", mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
  return MG_OK;
}

int mg_heat_set_source(mg_heat* s, const void* profile_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_source: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  if (!profile_host_or_null) {
    HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
    if (s->src) { (void)hipFree(s->src); s->src = nullptr; }
    return MG_OK;
  }
  if (!s->src) { const int rc = alloc_zero(&s->err, (void**)&s->src, field_bytes(s), s->eng->stream); if (rc != MG_OK) return rc; }
  return put(s, s->src, profile_host_or_null, host_dtype);
}

int mg_heat_set_coefficient(mg_heat* s, const void* a_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_coefficient: bad argument");
  if (a_host_or_null) {                                           // before any device work
    const size_t n = (size_t)s->nx * s->ny;
    const bool ok = host_dtype == MG_F32 ? coefficient_ok((const float*)a_host_or_null, n) : coefficient_ok((const double*)a_host_or_null, n);
    if (!ok) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_set_coefficient: the diffusivity field must be finite and > 0 everywhere");
  }
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  if (s->pcg) OWNED(mg_pcg_set_coefficient(s->pcg, a_host_or_null, host_dtype), "inner solver: ", mg_pcg_last_error(s->pcg));
  else OWNED(mg_set_coefficient(s->eng, a_host_or_null, host_dtype), "inner solver: ", mg_last_error(s->eng));
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
  return put(s, s->a, a_host_or_null, host_dtype);
}

int mg_heat_step(mg_heat* s, int scheme, double dt, int src, int prev, int dst, double g0, double g1, const double* edge4_or_null,
                 int bc_before_solve, double tol, int max_cycles, mg_heat_step_info* info) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_heat_step: NULL stepper");
  if (scheme < MG_HEAT_EXPLICIT_EULER || scheme > MG_HEAT_BDF2) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: unknown scheme");
  if (!(dt > 0.0) || !std::isfinite(dt)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: dt must be finite and > 0");
  if (!slot_ok(src) || !slot_ok(dst) || src == dst) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: src and dst are two different slots 0..3");
  if (scheme == MG_HEAT_BDF2) {
    if (!slot_ok(prev) || prev == dst) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: BDF2 reads a prev slot 0..3 other than dst");
  } else if (prev != -1) {
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: prev is -1 unless the scheme is BDF2");
  }
  if (!std::isfinite(g0) || !std::isfinite(g1)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: g0 / g1 not finite");
  if (bc_before_solve && !edge4_or_null) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: bc_before_solve needs edge values");
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
  if (max_cycles < 1 || !(tol == tol)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_step: max_cycles < 1 / tol is NaN");
  return implicit_step(s, scheme, dt, src, prev, dst, g0, g1, edge4_or_null, bc_before_solve, tol, max_cycles, info);
}

int mg_heat_diff_norm(mg_heat* s, int slot_a, int slot_b, double* out) {
  if (!s || !out || !slot_ok(slot_a) || !slot_ok(slot_b)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_heat_diff_norm: bad argument");
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
  CHECK_ARG(scheme >= MG_HEAT_EXPLICIT_EULER && scheme <= MG_HEAT_BDF2, "mg_dev_heat_rhs: unknown scheme");
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_heat_rhs: bad shape / pitch");
  CHECK_ARG(dt > 0.0 && std::isfinite(dt) && alpha > 0.0 && std::isfinite(alpha) && hx > 0.0 && hy > 0.0, "mg_dev_heat_rhs: dt, alpha and the spacings must be finite and > 0");
  CHECK_ARG(u && out && scratch, "mg_dev_heat_rhs: NULL pointer");
  CHECK_ARG(scheme != MG_HEAT_BDF2 || u_prev_or_null, "mg_dev_heat_rhs: BDF2 needs u_prev");
  CHECK_ARG(!overlap(out, u, nx, ld) && !overlap(out, u_prev_or_null, nx, ld) && !overlap(out, src_or_null, nx, ld) &&
            !overlap(out, a_or_null, nx, ld), "mg_dev_heat_rhs: out is an array of its own (it overlaps an input)");
  CHECK_ARG(aligned16(u) && aligned16(out) && aligned16(u_prev_or_null) && aligned16(src_or_null) && aligned16(a_or_null),
            "mg_dev_heat_rhs: unaligned pointer");
  const int n = launch_rhs(scheme, nx, ny, ld, hx, hy, alpha, dt, u, scheme == MG_HEAT_BDF2 ? u_prev_or_null : nullptr, src_or_null,
                           a_or_null, g0, g1, out, (double*)scratch, (hipStream_t)stream);
  if (sumsq_dev_or_null) launch_sum((double*)scratch, n, sumsq_dev_or_null, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_heat_ring(int nx, int ny, int ld, const double edge4[4], double* u, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_heat_ring: bad shape / pitch");
  CHECK_ARG(edge4 && u, "mg_dev_heat_ring: NULL pointer");
  launch_ring(u, nx, ny, ld, edge4, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_heat_diff_sumsq(int nx, int ny, int ld, const double* a, const double* b, void* scratch, double* sumsq_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_heat_diff_sumsq: bad shape / pitch");
  CHECK_ARG(a && b && scratch && sumsq_dev, "mg_dev_heat_diff_sumsq: NULL pointer");
  CHECK_ARG(aligned16(a) && aligned16(b), "mg_dev_heat_diff_sumsq: unaligned pointer");
  const int n = launch_diff(a, b, (double*)scratch, nx, ny, ld, (hipStream_t)stream);
  launch_sum((double*)scratch, n, sumsq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

}  // extern "C"
