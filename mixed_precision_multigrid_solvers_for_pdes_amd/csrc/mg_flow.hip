// The flow stepper of libmghip.so: device-resident 2-D incompressible Navier-Stokes in the vorticity / stream-function form
// (include/mghip_flow.h) on top of the multigrid engine.  This unit instantiates the kernels of mg_flow_kernels.hpp and holds
// the driver; the two inner solvers are mg_handles of its own -- psi with shift 0, w with shift sigma = 2/(nu dt) -- driven
// through the device entry points of the C ABI (mg_set_rhs_device / mg_update_rhs_device, mg_set_shift, mg_iterate,
// mg_get_solution_device) exactly as mg_heat.hip drives its one; both run on the psi engine's stream, where the stepper queues
// its own kernels too.
//
//   step:  f, N = rhs(psi, w, N_prev) with sum f^2 and the velocity maximum  ->  w engine rhs  ->  shift sigma when dt changed
//          ->  ring of w from psi  ->  initial guess w  ->  cycles until ||r|| < tol max(1, ||f||)  ->  w_new
//          ->  g = w_new with a zero ring, sum g^2, max |w_new - w|  ->  psi engine rhs  ->  initial guess psi  ->  cycles  ->  psi
//
// w and N live in two buffers each that a step swaps, so no copy is made and no field crosses PCIe between steps.
#include "mg_host.hpp"
#include "../../include/mghip_flow.h"
#include "mg_flow_kernels.hpp"

using namespace mgh;

struct mg_flow {
  mg_config cfg;
  mg_handle* eng_psi = nullptr;         // -lap psi = w; its stream carries all of the stepper's work
  mg_handle* eng_w = nullptr;           // (-lap + sigma) w = f
  int nx = 0, ny = 0, ld = 0;
  double hx = 0, hy = 0, nu = 0;
  int wall = MG_FLOW_NO_SLIP;
  double speeds[4] = {0, 0, 0, 0};
  double* w = nullptr;                  // omega^n
  double* w_new = nullptr;
  double* psi = nullptr;
  double* n_cur = nullptr;              // N of the latest step (the next step's N_prev)
  double* n_new = nullptr;
  double* f = nullptr;                  // right-hand side of either solve (the engine keeps a copy of its own)
  double* force = nullptr;              // F (nullable)
  double* partials = nullptr;
  double* d_sc = nullptr;               // device, 4 doubles
  double* h_sc = nullptr;               // pinned host, 4 doubles
  double sigma = -1.0;                  // the shift the w engine carries (< 0: none set yet)
  double dt_prev = 0.0;
  bool have_prev = false;               // n_cur holds N of the step before
  bool w_has_rhs = false, psi_has_rhs = false;
  std::vector<double> hist;
  std::string err;
};

namespace {

// ---- launchers (shared by the driver and the stateless mg_dev_flow_* forms); an int result is the number of partials per
// result ----
int launch_rhs(int nx, int ny, int ld, double hx, double hy, double nu, double dt, double c0, double c1, const double* psi,
               const double* w, const double* n_prev, const double* force, double* f_out, double* n_out, double* partials,
               hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  const Coef k = coefs(hx, hy);
  mg::FlowCoef c;
  c.ihx2 = k.ihx2; c.ihy2 = k.ihy2; c.diag = k.diag;
  c.sigma = 2.0 / (nu * dt);
  c.k = 2.0 / nu;
  c.c0 = c0; c.c1 = c1;
  c.d12 = 12.0 * hx * hy;
  auto kern = n_prev ? (force ? mg::flow_rhs_kernel<true, true> : mg::flow_rhs_kernel<true, false>)
                     : (force ? mg::flow_rhs_kernel<false, true> : mg::flow_rhs_kernel<false, false>);
  hipLaunchKernelGGL(kern, dim3(g.ntiles), dim3(mg::kBlock), 0, st, psi, w, n_prev, force, f_out, n_out, partials, g, c);
  return g.ntiles;
}

void launch_wall(double* w, const double* psi, int nx, int ny, int ld, double hx, double hy, int kind, const double* sp,
                 hipStream_t st) {
  const int nb = std::max(1, std::min(64, (2 * (nx + ny) + mg::kBlock - 1) / mg::kBlock));
  hipLaunchKernelGGL(mg::flow_wall_kernel, dim3(nb), dim3(mg::kBlock), 0, st, w, psi, nx, ny, ld, kind, hx, hy, sp[0], sp[1], sp[2], sp[3]);
}

int stream_blocks(long long vecs) { return (int)std::max<long long>(1, std::min<long long>((vecs + mg::kBlock - 1) / mg::kBlock, 512)); }

int launch_interior(const double* w, const double* w_old, double* out, double* partials, int nx, int ny, int ld, hipStream_t st) {
  const int nyv = field_geom(nx, ny, ld).nyv;
  const int nb = stream_blocks((long long)nx * (nyv / 2));
  auto kern = w_old ? mg::flow_interior_kernel<true> : mg::flow_interior_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(nb), dim3(mg::kBlock), 0, st, w, w_old, out, partials, nx, ny, nyv, ld);
  return nb;
}

int launch_diag(const double* psi, const double* w, double* partials, int nx, int ny, int ld, hipStream_t st) {
  const int nyv = field_geom(nx, ny, ld).nyv;
  const int nb = stream_blocks((long long)(nx - 2) * (nyv / 2));
  hipLaunchKernelGGL(mg::flow_diag_kernel, dim3(nb), dim3(mg::kBlock), 0, st, psi, w, partials, nx, ny, nyv, ld);
  return nb;
}

// results: how many (workgroup b reduces partials[b n .. b n + n) into out[b]); bit b of max_mask: a maximum, not a sum
void launch_reduce_results(const double* partials, int n, int results, int max_mask, double* out, hipStream_t st) {
  hipLaunchKernelGGL(mg::reduce_rows_kernel<true>, dim3(results), dim3(mg::kReduceBlock), 0, st, partials, n, n, max_mask, out);
}

void release(mg_flow* s) {
  if (s->eng_w) { (void)mg_destroy(s->eng_w); s->eng_w = nullptr; }          // first: it runs on the other engine's stream
  if (s->eng_psi) { (void)mg_destroy(s->eng_psi); s->eng_psi = nullptr; }
  for (double** p : {&s->w, &s->w_new, &s->psi, &s->n_cur, &s->n_new, &s->f, &s->force, &s->partials, &s->d_sc})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (s->h_sc) { (void)hipHostFree(s->h_sc); s->h_sc = nullptr; }
}

hipStream_t stream_of(const mg_flow* s) { return s->eng_psi->stream; }

double* field_of(mg_flow* s, int which) {
  return which == MG_FLOW_OMEGA ? s->w : which == MG_FLOW_PSI ? s->psi : which == MG_FLOW_N ? s->n_cur : nullptr;
}

// host array (nx, ny) of hdt -> fp64 device field with the stepper's pitch, on the stepper's stream (through the staging field)
int put(mg_flow* s, double* dev, const void* host, int hdt) {
  return upload(&s->err, dev, MG_F64, s->ld, host, hdt, s->nx, s->ny, s->eng_psi->staging, stream_of(s));
}

bool all_finite(const void* host, int hdt, size_t n) {
  bool ok = true;
  if (hdt == MG_F64) { const double* p = (const double*)host; for (size_t k = 0; k < n && ok; ++k) ok = std::isfinite(p[k]); }
  else { const float* p = (const float*)host; for (size_t k = 0; k < n && ok; ++k) ok = std::isfinite(p[k]); }
  return ok;
}

struct SolveOut {
  double initial = 0, final = 0;
  int cycles = 0, converged = 0;
};

// hand `eng` the right-hand side s->f (zero ring) and the initial guess, wait for the two scalars at h_sc[slot .. slot + 1]
// (the first is sum f^2), run the cycles, copy the solution to dst
int solve_on(mg_flow* s, mg_handle* eng, bool* has_rhs, const double* guess, double* dst, int slot, double tol, int max_cycles,
             double* fnorm_out, SolveOut* out) {
  hipStream_t st = stream_of(s);
  // f has a zero ring by construction: mg_iterate runs the loop mg_solve runs after an upload
  OWNED(engine_set_rhs(eng, has_rhs, s->f, s->ld, true), "inner solver: ", mg_last_error(eng));
  OWNED(set_u_device_impl(eng, guess, s->ld, MG_F64), "inner solver: ", mg_last_error(eng));
  HIPC(&s->err, hipStreamSynchronize(st));                        // the scalars have arrived
  const double fnorm = std::sqrt(s->hx * s->hy * s->h_sc[slot]);
  if ((int)s->hist.size() < max_cycles) s->hist.resize(max_cycles);
  int n = 0, conv = 0;
  mg_stats stats;
  // A NaN norm: std::max(1.0, NaN) is 1.0, so the target is `tol` and no NaN residual is below it -- the solve runs to its
  // cap and reports converged = 0; the NaN itself is visible to the caller in rhs_norm.

  OWNED(mg_iterate(eng, tol * std::max(1.0, fnorm), max_cycles, s->hist.data(), max_cycles, &n, &conv, nullptr, &stats), "inner solver: ", mg_last_error(eng));
  OWNED(mg_get_solution_device(eng, dst, s->ld, MG_F64), "inner solver: ", mg_last_error(eng));
  *fnorm_out = fnorm;
  out->initial = stats.initial_residual;
  out->final = n > 0 ? s->hist[n - 1] : stats.initial_residual;
  out->cycles = n;
  out->converged = conv;
  return MG_OK;
}

// g = w_src with a zero ring -> s->f with {sum g^2, max |w_src - w_old|} -> the psi solve from the current psi, in place
int psi_solve(mg_flow* s, const double* w_src, const double* w_old, double tol, int max_cycles, mg_flow_step_info* info) {
  hipStream_t st = stream_of(s);
  const int np = launch_interior(w_src, w_old, s->f, s->partials, s->nx, s->ny, s->ld, st);
  launch_reduce_results(s->partials, np, 2, 2, s->d_sc + 2, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sc + 2, s->d_sc + 2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  double gnorm = 0.0;
  SolveOut so;
  const int rc = solve_on(s, s->eng_psi, &s->psi_has_rhs, s->psi, s->psi, 2, tol, max_cycles, &gnorm, &so);
  if (rc != MG_OK) return rc;
  if (info) {
    info->psi_rhs_norm = gnorm;
    info->psi_initial_residual = so.initial;
    info->psi_final_residual = so.final;
    info->psi_cycles = so.cycles;
    info->psi_converged = so.converged;
    info->omega_change = s->h_sc[3];
  }
  return MG_OK;
}

}  // namespace

extern "C" {

int mg_flow_create(const mg_config* cfg, double nu, int wall_kind, mg_flow** out) {
  if (!cfg || !out) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_flow_create: NULL argument");
  *out = nullptr;
  if (cfg->precision != MG_PREC_DOUBLE) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_flow_create: the inner solvers run in MG_PREC_DOUBLE");
  if (cfg->coeff != -1.0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_flow_create: coeff must be -1 (the steps solve (-Laplacian + sigma) w = f and -Laplacian psi = w)");
  if (cfg->fmg_cycles != 0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_flow_create: fmg_cycles must be 0 (a step starts from the old time level)");
  if (!(nu > 0.0) || !std::isfinite(nu)) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_flow_create: nu must be finite and > 0");
  if (wall_kind != MG_FLOW_FREE_SLIP && wall_kind != MG_FLOW_NO_SLIP) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_flow_create: unknown wall kind");
  mg_handle* ep = nullptr;
  int rc = mg_create(cfg, &ep);
  if (rc != MG_OK) return rc;
  mg_handle* ew = nullptr;
  if ((rc = mg_create(cfg, &ew)) != MG_OK) { const std::string m = last_error(); (void)mg_destroy(ep); last_error() = m; return rc; }
  mg_flow* s = new mg_flow();
  s->cfg = *cfg;
  s->eng_psi = ep;
  s->eng_w = ew;
  s->nx = cfg->nx; s->ny = cfg->ny;
  (void)mg_pitch_elems(MG_F64, cfg->ny, &s->ld);
  s->hx = ep->lv[0].hx; s->hy = ep->lv[0].hy;
  s->nu = nu;
  s->wall = wall_kind;
  auto bail = [&](int code) { return create_fail(s, release, code); };
  if ((rc = mg_set_stream(ew, ep->stream, 0)) != MG_OK) { s->err = mg_last_error(ew); return bail(rc); }      // one stream for everything
  hipStream_t st = ep->stream;
  for (double** p : {&s->w, &s->w_new, &s->psi, &s->n_cur, &s->n_new, &s->f})
    if ((rc = alloc_zero(&s->err, (void**)p, field_bytes(s), st)) != MG_OK) return bail(rc);
  int64_t scratch = 0;
  (void)mg_dev_scratch_bytes(s->nx, s->ny, &scratch);
  if ((rc = alloc_zero(&s->err, (void**)&s->partials, (size_t)scratch, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->d_sc, 4 * sizeof(double), st)) != MG_OK) return bail(rc);
  if (hipHostMalloc((void**)&s->h_sc, 4 * sizeof(double)) != hipSuccess) { s->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  if (hipStreamSynchronize(st) != hipSuccess) { s->err = "hipStreamSynchronize failed"; return bail(MG_ERR_HIP); }
  *out = s;
  return MG_OK;
}

int mg_flow_destroy(mg_flow* s) {
  if (!s) return MG_OK;
  (void)hipSetDevice(s->cfg.device);
  if (s->eng_psi && s->eng_psi->stream) (void)hipStreamSynchronize(s->eng_psi->stream);
  if (s->eng_w) (void)mg_set_stream(s->eng_w, nullptr, 1);        // back on its own stream before the shared one goes
  release(s);
  delete s;
  return MG_OK;
}

const char* mg_flow_last_error(const mg_flow* s) { return s ? s->err.c_str() : last_error().c_str(); }

int mg_flow_set_walls(mg_flow* s, const double* speeds4) {
  if (!s || !speeds4) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_set_walls: bad argument");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(speeds4[k])) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_set_walls: wall speeds must be finite");
  for (int k = 0; k < 4; ++k) s->speeds[k] = speeds4[k];
  return MG_OK;
}

int mg_flow_set_forcing(mg_flow* s, const void* f_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_set_forcing: bad argument");
  if (f_host_or_null && !all_finite(f_host_or_null, host_dtype, (size_t)s->nx * s->ny))          // before any device work
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_set_forcing: the forcing field must be finite everywhere");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  if (!f_host_or_null) {
    HIPC(&s->err, hipStreamSynchronize(stream_of(s)));
    if (s->force) { (void)hipFree(s->force); s->force = nullptr; }
    return MG_OK;
  }
  if (!s->force) { const int rc = alloc_zero(&s->err, (void**)&s->force, field_bytes(s), stream_of(s)); if (rc != MG_OK) return rc; }
  return put(s, s->force, f_host_or_null, host_dtype);
}

int mg_flow_set_state(mg_flow* s, const void* omega_host, int host_dtype, double tol, int max_cycles, mg_flow_step_info* info) {
  if (!s || !omega_host || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_set_state: bad argument");
  if (max_cycles < 1 || !(tol == tol)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_set_state: max_cycles < 1 / tol is NaN");
  if (!all_finite(omega_host, host_dtype, (size_t)s->nx * s->ny))
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_set_state: the vorticity must be finite everywhere");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  const double t0 = now_s();
  hipStream_t st = stream_of(s);
  int rc = put(s, s->w, omega_host, host_dtype);
  if (rc != MG_OK) return rc;
  HIPC(&s->err, hipMemsetAsync(s->psi, 0, field_bytes(s), st));
  if (info) *info = mg_flow_step_info{};
  if ((rc = psi_solve(s, s->w, nullptr, tol, max_cycles, info)) != MG_OK) return rc;
  launch_wall(s->w, s->psi, s->nx, s->ny, s->ld, s->hx, s->hy, s->wall, s->speeds, st);
  HIPC(&s->err, hipGetLastError());
  s->have_prev = false;
  s->dt_prev = 0.0;
  if (info) info->seconds = now_s() - t0;
  return MG_OK;
}

int mg_flow_get(mg_flow* s, int which, void* host, int host_dtype) {
  if (!s || !host || !valid_dtype(host_dtype) || !field_of(s, which)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_get: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  return download(&s->err, host, host_dtype, field_of(s, which), MG_F64, s->ld, s->nx, s->ny, s->eng_psi->staging, stream_of(s));
}

int mg_flow_get_device(mg_flow* s, int which, void* u_dev, int ld, int dtype) {
  if (!s || !u_dev || !valid_dtype(dtype) || !field_of(s, which) || ld < s->ny) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_get_device: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_dev_convert(MG_F64, dtype, s->nx, s->ny, s->ld, ld, field_of(s, which), u_dev, stream_of(s)), "", mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(stream_of(s)));
  return MG_OK;
}

int mg_flow_set_device(mg_flow* s, int which, const void* u_dev, int ld, int dtype) {
  if (!s || !u_dev || !valid_dtype(dtype) || !field_of(s, which) || ld < s->ny) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_set_device: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_dev_convert(dtype, MG_F64, s->nx, s->ny, ld, s->ld, u_dev, field_of(s, which), stream_of(s)), "", mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(stream_of(s)));
  return MG_OK;
}

int mg_flow_step(mg_flow* s, double dt, double tol, int max_cycles, mg_flow_step_info* info) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_flow_step: NULL stepper");
  if (!(dt > 0.0) || !std::isfinite(dt)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_step: dt must be finite and > 0");
  if (max_cycles < 1 || !(tol == tol)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_step: max_cycles < 1 / tol is NaN");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  const double t0 = now_s();
  hipStream_t st = stream_of(s);
  double c0 = 1.0, c1 = 0.0;
  if (s->have_prev) {
    const double r = dt / s->dt_prev;
    c0 = 1.0 + r / 2;
    c1 = -r / 2;
  }
  const double sigma = 2.0 / (s->nu * dt);
  const int np = launch_rhs(s->nx, s->ny, s->ld, s->hx, s->hy, s->nu, dt, c0, c1, s->psi, s->w, s->have_prev ? s->n_cur : nullptr,
                            s->force, s->f, s->n_new, s->partials, st);
  launch_reduce_results(s->partials, np, 2, 2, s->d_sc, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sc, s->d_sc, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  if (sigma != s->sigma) { OWNED(mg_set_shift(s->eng_w, sigma), "inner solver: ", mg_last_error(s->eng_w)); s->sigma = sigma; }
  // the Dirichlet data of the w solve: the wall values of psi^n, in place (f has been formed from the old ring)
  launch_wall(s->w, s->psi, s->nx, s->ny, s->ld, s->hx, s->hy, s->wall, s->speeds, st);
  HIPC(&s->err, hipGetLastError());
  double fnorm = 0.0;
  SolveOut so;
  int rc = solve_on(s, s->eng_w, &s->w_has_rhs, s->w, s->w_new, 0, tol, max_cycles, &fnorm, &so);
  if (rc != MG_OK) return rc;
  const double vmax = s->h_sc[1];
  if (info) {
    *info = mg_flow_step_info{};
    info->sigma = sigma; info->c0 = c0; info->c1 = c1;
    info->cfl = dt * vmax / (2 * s->hx * s->hy);
    info->rhs_norm = fnorm;
    info->omega_initial_residual = so.initial;
    info->omega_final_residual = so.final;
    info->omega_cycles = so.cycles;
    info->omega_converged = so.converged;
  }
  if ((rc = psi_solve(s, s->w_new, s->w, tol, max_cycles, info)) != MG_OK) return rc;
  std::swap(s->w, s->w_new);
  std::swap(s->n_cur, s->n_new);
  s->have_prev = true;
  s->dt_prev = dt;
  if (info) info->seconds = now_s() - t0;
  return MG_OK;
}

int mg_flow_diagnostics(mg_flow* s, double out[2]) {
  if (!s || !out) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_diagnostics: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  hipStream_t st = stream_of(s);
  const int np = launch_diag(s->psi, s->w, s->partials, s->nx, s->ny, s->ld, st);
  launch_reduce_results(s->partials, np, 3, 4, s->d_sc, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sc, s->d_sc, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(&s->err, hipStreamSynchronize(st));
  out[0] = s->h_sc[0];
  out[1] = s->h_sc[1];
  return MG_OK;
}

int mg_flow_velocity_max(mg_flow* s, double* m) {
  if (!s || !m) return sfail(s, MG_ERR_INVALID_VALUE, "mg_flow_velocity_max: bad argument");
  double two[2];
  const int rc = mg_flow_diagnostics(s, two);
  if (rc != MG_OK) return rc;
  *m = s->h_sc[2];
  return MG_OK;
}

// ---- the field kernels, call by call (pitch in elements, nullable stream, scratch >= mg_dev_scratch_bytes()) ----
int mg_dev_flow_rhs(int nx, int ny, int ld, double hx, double hy, double nu, double dt, double c0, double c1, const double* psi,
                    const double* omega, const double* n_prev_or_null, const double* force_or_null, double* f_out, double* n_out,
                    void* scratch, double* out2_dev_or_null, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_flow_rhs: bad shape / pitch");
  CHECK_ARG(dt > 0.0 && std::isfinite(dt) && nu > 0.0 && std::isfinite(nu) && hx > 0.0 && hy > 0.0 && std::isfinite(hx) && std::isfinite(hy),
            "mg_dev_flow_rhs: dt, nu and the spacings must be finite and > 0");
  CHECK_ARG(std::isfinite(c0) && std::isfinite(c1), "mg_dev_flow_rhs: c0 / c1 not finite");
  CHECK_ARG(psi && omega && f_out && n_out && scratch, "mg_dev_flow_rhs: NULL pointer");
  for (const double* o : {(const double*)f_out, (const double*)n_out})
    CHECK_ARG(!overlap(o, psi, nx, ld) && !overlap(o, omega, nx, ld) && !overlap(o, n_prev_or_null, nx, ld) &&
              !overlap(o, force_or_null, nx, ld), "mg_dev_flow_rhs: an output is an array of its own (it overlaps an input)");
  CHECK_ARG(!overlap(f_out, n_out, nx, ld), "mg_dev_flow_rhs: an output is an array of its own (f and N overlap)");
  CHECK_ARG(aligned16(psi) && aligned16(omega) && aligned16(n_prev_or_null) && aligned16(force_or_null) && aligned16(f_out) &&
            aligned16(n_out), "mg_dev_flow_rhs: unaligned pointer");
  const int n = launch_rhs(nx, ny, ld, hx, hy, nu, dt, c0, c1, psi, omega, n_prev_or_null, force_or_null, f_out, n_out,
                           (double*)scratch, (hipStream_t)stream);
  if (out2_dev_or_null) launch_reduce_results((double*)scratch, n, 2, 2, out2_dev_or_null, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_flow_wall(int nx, int ny, int ld, double hx, double hy, int wall_kind, const double* speeds4, const double* psi,
                     double* omega, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_flow_wall: bad shape / pitch");
  CHECK_ARG(hx > 0.0 && hy > 0.0 && std::isfinite(hx) && std::isfinite(hy), "mg_dev_flow_wall: the spacings must be finite and > 0");
  CHECK_ARG(wall_kind == MG_FLOW_FREE_SLIP || wall_kind == MG_FLOW_NO_SLIP, "mg_dev_flow_wall: unknown wall kind");
  CHECK_ARG(speeds4 && psi && omega, "mg_dev_flow_wall: NULL pointer");
  CHECK_ARG(!overlap(omega, psi, nx, ld), "mg_dev_flow_wall: omega and psi overlap");
  launch_wall(omega, psi, nx, ny, ld, hx, hy, wall_kind, speeds4, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_flow_diag(int nx, int ny, int ld, const double* psi, const double* omega, void* scratch, double* out3_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_flow_diag: bad shape / pitch");
  CHECK_ARG(psi && omega && scratch && out3_dev, "mg_dev_flow_diag: NULL pointer");
  CHECK_ARG(aligned16(psi) && aligned16(omega), "mg_dev_flow_diag: unaligned pointer");
  const int n = launch_diag(psi, omega, (double*)scratch, nx, ny, ld, (hipStream_t)stream);
  launch_reduce_results((double*)scratch, n, 3, 4, out3_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_flow_interior(int nx, int ny, int ld, const double* w, const double* w_old_or_null, double* out, void* scratch,
                         double* out2_dev_or_null, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_flow_interior: bad shape / pitch");
  CHECK_ARG(w && out && scratch, "mg_dev_flow_interior: NULL pointer");
  CHECK_ARG(!overlap(out, w, nx, ld) && !overlap(out, w_old_or_null, nx, ld), "mg_dev_flow_interior: out is an array of its own (it overlaps an input)");
  CHECK_ARG(aligned16(w) && aligned16(w_old_or_null) && aligned16(out), "mg_dev_flow_interior: unaligned pointer");
  const int n = launch_interior(w, w_old_or_null, out, (double*)scratch, nx, ny, ld, (hipStream_t)stream);
  if (out2_dev_or_null) launch_reduce_results((double*)scratch, n, 2, 2, out2_dev_or_null, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

}  // extern "C"
