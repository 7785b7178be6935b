// Semilinear elliptic problems of libmghip.so (include/mghip_nl.h): A u + kappa w phi(u) = f by an inexact Newton method whose
// state stays on the device.  This unit instantiates the kernel of mg_nl_kernels.hpp and holds its launcher (declared in
// mg_host.hpp; the Krylov loop of mg_pcg.hip takes its residuals under a reaction field from it), the stateless device form,
// the host-array form and the Newton driver.  The driver owns an mg_pcg and through it the preconditioner engine, on whose
// stream all of its work is queued:
//
//   eval(u_0): ||F_0||, c, cbar;  per step:  eta_k;  mg_pcg_set_reaction_device(c, cbar);  delta = 0;  CG on (A + diag(c)) delta = F_k;
//   t = 1: eval(u_k, delta, t) into the trial buffers -- accept when ||F_trial|| <= (1 - 1e-4 t) ||F_k|| and swap, else t /= 2.
//
// Per trial the host reads two doubles (the sum of F^2 and the sum of c).
#include "mg_launch.hpp"
#include "mg_nl_kernels.hpp"

#include "../../include/mghip_nl.h"

#include <cstdint>

using namespace mgh;

namespace mgh {

int d_nl_eval(int kind, const double* u, const double* delta, double t, const double* a, const double* w, const double* f,
              double* u_out, double* F, double* c, double* partials, int* second, int nx, int ny, int ld, double hx, double hy,
              double coeff, double sigma, double kappa, hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  const Coef cf = coefs(hx, hy, sigma);
  mg::NlArgs n;
  n.ihx2 = cf.ihx2; n.ihy2 = cf.ihy2; n.diag = cf.diag; n.coeff = coeff; n.sigma = sigma;
  n.kappa = kappa; n.t = t;
  n.second = (g.ntiles + 1) & ~1;             // even: both sets of partials start 16-byte aligned
  *second = n.second;
  auto launch = [&](auto k) {
    hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, u, delta, a, w, f, u_out, F, c, partials, g, n);
  };
  switch (kind) {
    case MG_NL_LINEAR: a ? launch(mg::nl_eval_kernel<mg::kNlLinear, true>) : launch(mg::nl_eval_kernel<mg::kNlLinear, false>); break;
    case MG_NL_CUBIC: a ? launch(mg::nl_eval_kernel<mg::kNlCubic, true>) : launch(mg::nl_eval_kernel<mg::kNlCubic, false>); break;
    case MG_NL_SINH: a ? launch(mg::nl_eval_kernel<mg::kNlSinh, true>) : launch(mg::nl_eval_kernel<mg::kNlSinh, false>); break;
    default: a ? launch(mg::nl_eval_kernel<mg::kNlExp, true>) : launch(mg::nl_eval_kernel<mg::kNlExp, false>); break;
  }
  return g.ntiles;
}

}  // namespace mgh

struct mg_nl {
  mg_config cfg;
  mg_pcg* pcg = nullptr;
  hipStream_t st = nullptr;             // the engine's stream
  int nx = 0, ny = 0, ld = 0;
  double hx = 0, hy = 0;
  double* u[2] = {nullptr, nullptr};    // the iterate and the trial iterate; u[cur] is current, as F[cur] and c[cur] are
  double* F[2] = {nullptr, nullptr};
  double* c[2] = {nullptr, nullptr};
  int cur = 0;
  double *delta = nullptr, *f = nullptr, *a = nullptr, *w = nullptr, *staging = nullptr;
  double* partials = nullptr;           // 2 x max_partials
  double* sums = nullptr;               // device, 2 doubles
  double* h_sums = nullptr;             // pinned host copy
  bool varcoef = false, has_w = false;
  int kind = MG_NL_LINEAR;
  double kappa = 0.0, sigma = 0.0;
  mg_nl_options opt;
  std::string err;
};

namespace mgh {
mg_handle* nl_engine(mg_nl* s) { return pcg_engine(s->pcg); }
}  // namespace mgh

namespace {

void options_default(mg_nl_options* o) {
  o->forcing = MG_NL_FORCING_EISENSTAT_WALKER;
  o->max_backtracks = 10;
  o->max_inner = 100;
  o->reserved = 0;
  o->eta = 1e-8;
  o->gamma = 0.9;
  o->eta_max = 0.1;
  o->eta_min = 1e-10;
}

void release(mg_nl* s) {
  if (s->pcg) { (void)mg_pcg_destroy(s->pcg); s->pcg = nullptr; }
  for (double** p : {&s->u[0], &s->u[1], &s->F[0], &s->F[1], &s->c[0], &s->c[1], &s->delta, &s->f, &s->a, &s->w, &s->staging,
                     &s->partials, &s->sums})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (s->h_sums) { (void)hipHostFree(s->h_sums); s->h_sums = nullptr; }
}

// host array (nx, ny) of hdt -> fp64 device field with the solver's pitch, on the engine's stream
int put(mg_nl* s, double* dev, const void* host, int hdt) {
  return upload(&s->err, dev, MG_F64, s->ld, host, hdt, s->nx, s->ny, s->staging, s->st);
}

// One Newton trial: v = u[cur] + t delta (with_delta) into u[into], F(v) and c(v) into F[into] and c[into]; the host gets the
// norm of F and the mean of c.  Without delta, u[into] is not written (into == cur: the current iterate's own F and c).
int eval(mg_nl* s, bool with_delta, double t, int into, double* norm, double* cbar) {
  int second = 0;
  const int n = d_nl_eval(s->kind, s->u[s->cur], with_delta ? s->delta : nullptr, t, s->varcoef ? s->a : nullptr,
                          s->has_w ? s->w : nullptr, s->f, with_delta ? s->u[into] : nullptr, s->F[into], s->c[into], s->partials,
                          &second, s->nx, s->ny, s->ld, s->hx, s->hy, s->cfg.coeff, s->sigma, s->kappa, s->st);
  launch_reduce(s->partials, n, s->sums, s->st);
  launch_reduce(s->partials + second, n, s->sums + 1, s->st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sums, s->sums, 2 * sizeof(double), hipMemcpyDeviceToHost, s->st));
  HIPC(&s->err, hipStreamSynchronize(s->st));
  *norm = std::sqrt(s->hx * s->hy * s->h_sums[0]);
  *cbar = s->h_sums[1] / ((double)(s->nx - 2) * (double)(s->ny - 2));
  return MG_OK;
}

// the loop of include/mghip_nl.h on the resident f and u[cur]
int solve_resident(mg_nl* s, double tol, int max_newton, double* norm_hist, int* inner_hist, double* step_hist, double* eta_hist,
                   int hist_cap, int* n_newton, int* converged, mg_nl_stats* stats) {
  const double t0 = now_s();
  const mg_nl_options& o = s->opt;
  std::vector<double> inner_norms((size_t)o.max_inner);
  double norm = 0, cbar = 0;
  int rc = eval(s, false, 0.0, s->cur, &norm, &cbar);
  if (rc != MG_OK) return rc;
  const double norm0 = norm;
  int evals = 1, inner_total = 0, k = 0, status = 1;
  double prev_norm = norm, prev_eta = o.eta_max;
  for (;;) {
    if (norm < tol) { status = 0; break; }
    if (k == max_newton) { status = 1; break; }
    if (!std::isfinite(norm) || !std::isfinite(cbar) || !(cbar >= 0.0)) { status = 2; break; }   // no SPD Jacobian to solve with
    double eta = o.eta;
    if (o.forcing != MG_NL_FORCING_FIXED) {
      if (k == 0) eta = o.eta_max;
      else {
        const double q = norm / prev_norm;
        eta = o.gamma * (q * q);
        const double guard = o.gamma * (prev_eta * prev_eta);
        if (guard > 0.1) eta = std::max(eta, guard);
        eta = std::min(std::max(eta, o.eta_min), o.eta_max);
      }
    }
    const double inner_tol = std::max(eta * norm, 0.1 * tol);
    OWNED(mg_pcg_set_reaction_device(s->pcg, s->c[s->cur], s->ld, cbar), "inner solver: ", mg_pcg_last_error(s->pcg));
    HIPC(&s->err, hipMemsetAsync(s->delta, 0, field_bytes(s), s->st));
    int n_in = 0, conv_in = 0;
    mg_pcg_stats ps;
    OWNED(mg_pcg_solve_device(s->pcg, s->F[s->cur], s->ld, s->delta, s->ld, MG_F64, inner_tol, o.max_inner, inner_norms.data(),
                            o.max_inner, &n_in, &conv_in, &ps), "inner solver: ", mg_pcg_last_error(s->pcg));
    inner_total += n_in;
    if (ps.status == 2 && n_in == 0) { status = 2; break; }
    // backtracking: the trial goes to the spare buffers, a rejected one is overwritten by the next
    const int trial = s->cur ^ 1;
    double t = 1.0, tn = 0, tc = 0;
    bool accepted = false;
    for (int b = 0; b <= o.max_backtracks; ++b) {
      if ((rc = eval(s, true, t, trial, &tn, &tc)) != MG_OK) return rc;
      ++evals;
      if (std::isfinite(tn) && tn <= (1.0 - 1e-4 * t) * norm) { accepted = true; break; }
      t *= 0.5;
    }
    if (!accepted) { status = 3; break; }
    s->cur = trial;
    prev_norm = norm; prev_eta = eta;
    norm = tn; cbar = tc;
    if (k < hist_cap) {
      norm_hist[k] = norm;
      if (inner_hist) inner_hist[k] = n_in;
      if (step_hist) step_hist[k] = t;
      if (eta_hist) eta_hist[k] = eta;
    }
    ++k;
  }
  // the inner solver goes back to the plain loop: the field it was lent is rewritten by the next solve
  OWNED(mg_pcg_set_reaction_device(s->pcg, nullptr, 0, 0.0), "inner solver: ", mg_pcg_last_error(s->pcg));
  *n_newton = k;
  *converged = status == 0 ? 1 : 0;
  if (stats) {
    stats->solve_seconds = now_s() - t0;
    stats->initial_residual = norm0;
    stats->final_residual = norm;
    stats->newton_iterations = k;
    stats->inner_iterations = inner_total;
    stats->evaluations = evals;
    stats->status = status;
  }
  return MG_OK;
}

int solve_args_ok(mg_nl* s, const char* who, const void* f, const void* out, int dtype, double tol, int max_newton, double* hist,
                  int hist_cap, int* n_newton, int* converged) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, std::string(who) + ": NULL solver");
  if (!f || !out || !hist || !n_newton || !converged) return sfail(s, MG_ERR_INVALID_VALUE, std::string(who) + ": NULL argument");
  if (!valid_dtype(dtype) || hist_cap < 1 || max_newton < 1 || !(tol == tol))
    return sfail(s, MG_ERR_INVALID_VALUE, std::string(who) + ": bad dtype / hist_cap < 1 / max_newton < 1 / tol is NaN");
  return MG_OK;
}

}  // namespace

extern "C" {

int mg_dev_nl_eval(int kind, int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, double kappa,
                   const double* a_or_null, const double* w_or_null, const double* u, const double* delta_or_null, double t,
                   const double* f, double* u_out_or_null, double* F_or_null, double* c_or_null, void* scratch, double* sums_dev,
                   void* stream) {
  CHECK_ARG(kind_ok(kind, MG_NL_LINEAR, MG_NL_EXP), "mg_dev_nl_eval: unknown nonlinearity");
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld) && operator_ok(hx, hy, coeff, sigma), "mg_dev_nl_eval: bad shape / pitch / spacing / shift");
  CHECK_ARG(kappa_ok(kappa), "mg_dev_nl_eval: kappa must be finite and >= 0 (monotone nonlinearities only)");
  CHECK_ARG(!delta_or_null || std::isfinite(t), "mg_dev_nl_eval: the step length must be finite");
  CHECK_ARG(u && f && scratch && sums_dev, "mg_dev_nl_eval: NULL pointer");
  double* uo = delta_or_null ? u_out_or_null : nullptr;
  for (const double* out : {(const double*)uo, (const double*)F_or_null, (const double*)c_or_null})
    CHECK_ARG(!out || (out != u && out != f && out != delta_or_null && out != a_or_null && out != w_or_null),
             "mg_dev_nl_eval: outputs are arrays of their own");
  CHECK_ARG((!uo || (uo != F_or_null && uo != c_or_null)) && (!F_or_null || F_or_null != c_or_null),
           "mg_dev_nl_eval: outputs are arrays of their own");
  CHECK_ARG(aligned16(u) && aligned16(f) && aligned16(delta_or_null) && aligned16(a_or_null) && aligned16(w_or_null) && aligned16(uo) &&
           aligned16(F_or_null) && aligned16(c_or_null) && aligned16(scratch), "mg_dev_nl_eval: unaligned pointer");
  int second = 0;
  const int n = d_nl_eval(kind, u, delta_or_null, t, a_or_null, w_or_null, f, uo, F_or_null, c_or_null, (double*)scratch, &second, nx,
                          ny, ld, hx, hy, coeff, sigma, kappa, (hipStream_t)stream);
  launch_reduce((double*)scratch, n, sums_dev, (hipStream_t)stream);
  launch_reduce((double*)scratch + second, n, sums_dev + 1, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_op_nl_eval(int kind, int nx, int ny, double hx, double hy, double coeff, double sigma, double kappa, const double* a_or_null,
                  const double* w_or_null, const double* u, const double* delta_or_null, double t, const double* f,
                  double* u_out_or_null, double* F_or_null, double* c_or_null, double* sums) {
  CHECK_ARG(kind_ok(kind, MG_NL_LINEAR, MG_NL_EXP), "mg_op_nl_eval: unknown nonlinearity");
  CHECK_ARG(nx >= 3 && ny >= 3 && operator_ok(hx, hy, coeff, sigma) && u && f && sums, "mg_op_nl_eval: bad argument");
  CHECK_ARG(kappa_ok(kappa), "mg_op_nl_eval: kappa must be finite and >= 0 (monotone nonlinearities only)");
  CHECK_ARG(!w_or_null || weight_ok(w_or_null, (size_t)nx * ny), "mg_op_nl_eval: the weight field must be finite and >= 0");
  CHECK_ARG(!delta_or_null || std::isfinite(t), "mg_op_nl_eval: the step length must be finite");
  const int ld = pitch_elems(MG_F64, ny);
  const size_t pitch = (size_t)ld * 8, wbytes = (size_t)ny * 8;
  const double* in[5] = {u, f, delta_or_null, a_or_null, w_or_null};
  double* out[3] = {delta_or_null ? u_out_or_null : nullptr, F_or_null, c_or_null};
  void *din[5] = {}, *dout[3] = {}, *dpart = nullptr, *dsums = nullptr;
  auto done = [&](int rc) {
    for (void* p : din) if (p) (void)hipFree(p);
    for (void* p : dout) if (p) (void)hipFree(p);
    if (dpart) (void)hipFree(dpart);
    if (dsums) (void)hipFree(dsums);
    return rc;
  };
  int ndev = 0;
  int rc = mg_device_count(&ndev);
  if (rc != MG_OK) return rc;
  if (ndev <= 0) return fail(nullptr, MG_ERR_NO_DEVICE, "no HIP device visible");
  for (int k = 0; k < 5; ++k)
    if (in[k] && (rc = alloc_zero(nullptr, &din[k], pitch * nx)) != MG_OK) return done(rc);
  for (int k = 0; k < 3; ++k)
    if (out[k] && (rc = alloc_zero(nullptr, &dout[k], pitch * nx)) != MG_OK) return done(rc);
  if ((rc = alloc_zero(nullptr, &dpart, sizeof(double) * 2 * max_partials(nx, ny))) != MG_OK ||
      (rc = alloc_zero(nullptr, &dsums, sizeof(double) * 2)) != MG_OK)
    return done(rc);
  if (hipDeviceSynchronize() != hipSuccess) return done(fail(nullptr, MG_ERR_HIP, "mg_op_nl_eval: upload failed"));
  for (int k = 0; k < 5; ++k)
    if (in[k] && hipMemcpy2D(din[k], pitch, in[k], wbytes, wbytes, nx, hipMemcpyHostToDevice) != hipSuccess)
      return done(fail(nullptr, MG_ERR_HIP, "mg_op_nl_eval: upload failed"));
  int second = 0;
  const int n = d_nl_eval(kind, (const double*)din[0], (const double*)din[2], t, (const double*)din[3], (const double*)din[4],
                          (const double*)din[1], (double*)dout[0], (double*)dout[1], (double*)dout[2], (double*)dpart, &second, nx, ny,
                          ld, hx, hy, coeff, sigma, kappa, nullptr);
  launch_reduce((double*)dpart, n, (double*)dsums, nullptr);
  launch_reduce((double*)dpart + second, n, (double*)dsums + 1, nullptr);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(sums, dsums, 2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return done(fail(nullptr, MG_ERR_HIP, "mg_op_nl_eval: kernel or download failed"));
  for (int k = 0; k < 3; ++k)
    if (out[k] && hipMemcpy2D(out[k], wbytes, dout[k], pitch, wbytes, nx, hipMemcpyDeviceToHost) != hipSuccess)
      return done(fail(nullptr, MG_ERR_HIP, "mg_op_nl_eval: kernel or download failed"));
  return done(MG_OK);
}

int mg_nl_options_default(mg_nl_options* opt) {
  if (!opt) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_nl_options_default: NULL argument");
  options_default(opt);
  return MG_OK;
}

int mg_nl_create(const mg_config* cfg, int num_cycles, int flexible, mg_nl** out) {
  if (!cfg || !out) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_nl_create: NULL argument");
  *out = nullptr;
  mg_pcg* pcg = nullptr;
  int rc = mg_pcg_create(cfg, num_cycles, flexible, &pcg);
  if (rc != MG_OK) return rc;
  mg_nl* s = new mg_nl();
  s->cfg = *cfg;
  s->pcg = pcg;
  mg_handle* eng = pcg_engine(pcg);
  s->st = eng->stream;
  s->nx = cfg->nx; s->ny = cfg->ny;
  s->ld = pitch_elems(MG_F64, cfg->ny);
  s->hx = eng->lv[0].hx; s->hy = eng->lv[0].hy;
  options_default(&s->opt);
  auto bail = [&](int code) { return create_fail(s, release, code); };
  for (double** p : {&s->u[0], &s->u[1], &s->F[0], &s->F[1], &s->c[0], &s->c[1], &s->delta, &s->f, &s->staging})
    if ((rc = alloc_zero(&s->err, (void**)p, field_bytes(s), s->st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->partials, sizeof(double) * 2 * max_partials(s->nx, s->ny), s->st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->sums, sizeof(double) * 2, s->st)) != MG_OK) return bail(rc);
  if (hipHostMalloc((void**)&s->h_sums, sizeof(double) * 2) != hipSuccess) { s->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  if (hipStreamSynchronize(s->st) != hipSuccess) { s->err = "hipStreamSynchronize failed"; return bail(MG_ERR_HIP); }
  *out = s;
  return MG_OK;
}

int mg_nl_destroy(mg_nl* s) {
  return destroy_owned(s, s ? s->st : nullptr, release);
}

const char* mg_nl_last_error(const mg_nl* s) { return s ? s->err.c_str() : last_error().c_str(); }

int mg_nl_set_coefficient(mg_nl* s, const void* a_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_set_coefficient: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_pcg_set_coefficient(s->pcg, a_host_or_null, host_dtype), "inner solver: ", mg_pcg_last_error(s->pcg));
  if (!a_host_or_null) { s->varcoef = false; return MG_OK; }
  if (!s->a) { const int rc = alloc_zero(&s->err, (void**)&s->a, field_bytes(s), s->st); if (rc != MG_OK) return rc; }
  const int rc = put(s, s->a, a_host_or_null, host_dtype);
  if (rc != MG_OK) return rc;
  s->varcoef = true;
  return MG_OK;
}

int mg_nl_set_shift(mg_nl* s, double sigma) {
  if (!s || !(sigma >= 0.0) || !std::isfinite(sigma)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_set_shift: sigma must be finite and >= 0");
  OWNED(mg_pcg_set_shift(s->pcg, sigma), "inner solver: ", mg_pcg_last_error(s->pcg));
  s->sigma = sigma;
  return MG_OK;
}

int mg_nl_set_nonlinearity(mg_nl* s, int kind, double kappa, const void* w_host_or_null, int host_dtype) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_nl_set_nonlinearity: NULL solver");
  if (!kind_ok(kind, MG_NL_LINEAR, MG_NL_EXP)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_set_nonlinearity: unknown nonlinearity (mg_nl_kind)");
  if (!kappa_ok(kappa)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_set_nonlinearity: kappa must be finite and >= 0 (monotone nonlinearities only)");
  if (!valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_set_nonlinearity: bad dtype");
  if (w_host_or_null) {
    const size_t n = (size_t)s->nx * s->ny;
    const bool ok = host_dtype == MG_F32 ? weight_ok((const float*)w_host_or_null, n) : weight_ok((const double*)w_host_or_null, n);
    if (!ok) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_set_nonlinearity: the weight field must be finite and >= 0 (monotone nonlinearities only)");
    HIPC(&s->err, hipSetDevice(s->cfg.device));
    if (!s->w) { const int rc = alloc_zero(&s->err, (void**)&s->w, field_bytes(s), s->st); if (rc != MG_OK) return rc; }
    const int rc = put(s, s->w, w_host_or_null, host_dtype);
    if (rc != MG_OK) return rc;
  }
  s->has_w = w_host_or_null != nullptr;
  s->kind = kind;
  s->kappa = kappa;
  return MG_OK;
}

int mg_nl_set_options(mg_nl* s, const mg_nl_options* o) {
  if (!s || !o) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_set_options: NULL argument");
  const bool ok = (o->forcing == MG_NL_FORCING_EISENSTAT_WALKER || o->forcing == MG_NL_FORCING_FIXED) && o->max_backtracks >= 0 &&
                  o->max_inner >= 1 && o->eta > 0.0 && o->eta < 1.0 && o->gamma > 0.0 && o->gamma <= 1.0 && o->eta_min > 0.0 &&
                  o->eta_min <= o->eta_max && o->eta_max < 1.0;
  if (!ok) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_set_options: forcing / max_backtracks >= 0 / max_inner >= 1 / 0 < eta < 1 / 0 < gamma <= 1 / 0 < eta_min <= eta_max < 1");
  s->opt = *o;
  return MG_OK;
}

int mg_nl_solve_device(mg_nl* s, const void* f_dev, int ld_f, void* u_dev, int ld_u, int dtype, double tol, int max_newton,
                       double* norm_hist, int* inner_hist, double* step_hist, double* eta_hist, int hist_cap, int* n_newton,
                       int* converged, mg_nl_stats* stats) {
  int rc = solve_args_ok(s, "mg_nl_solve_device", f_dev, u_dev, dtype, tol, max_newton, norm_hist, hist_cap, n_newton, converged);
  if (rc != MG_OK) return rc;
  if (ld_f < s->ny || ld_u < s->ny) return sfail(s, MG_ERR_INVALID_VALUE, "mg_nl_solve_device: pitch smaller than ny");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  d_convert(dtype, MG_F64, f_dev, s->f, s->nx, s->ny, ld_f, s->ld, s->st);
  d_convert(dtype, MG_F64, u_dev, s->u[s->cur], s->nx, s->ny, ld_u, s->ld, s->st);
  if ((rc = solve_resident(s, tol, max_newton, norm_hist, inner_hist, step_hist, eta_hist, hist_cap, n_newton, converged, stats)) != MG_OK) {
    (void)hipStreamSynchronize(s->st);
    return rc;
  }
  d_convert(MG_F64, dtype, s->u[s->cur], u_dev, s->nx, s->ny, s->ld, ld_u, s->st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipStreamSynchronize(s->st));
  return MG_OK;
}

int mg_nl_solve(mg_nl* s, const void* f, const void* u0_or_null, void* u_out, int host_dtype, double tol, int max_newton,
                double* norm_hist, int* inner_hist, double* step_hist, double* eta_hist, int hist_cap, int* n_newton,
                int* converged, mg_nl_stats* stats) {
  int rc = solve_args_ok(s, "mg_nl_solve", f, u_out, host_dtype, tol, max_newton, norm_hist, hist_cap, n_newton, converged);
  if (rc != MG_OK) return rc;
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  if ((rc = put(s, s->f, f, host_dtype)) != MG_OK) return rc;
  if (u0_or_null) { if ((rc = put(s, s->u[s->cur], u0_or_null, host_dtype)) != MG_OK) return rc; }
  else HIPC(&s->err, hipMemsetAsync(s->u[s->cur], 0, field_bytes(s), s->st));
  if ((rc = solve_resident(s, tol, max_newton, norm_hist, inner_hist, step_hist, eta_hist, hist_cap, n_newton, converged, stats)) != MG_OK) {
    (void)hipStreamSynchronize(s->st);
    return rc;
  }
  return download(&s->err, u_out, host_dtype, s->u[s->cur], MG_F64, s->ld, s->nx, s->ny, s->staging, s->st);
}

}  // extern "C"
