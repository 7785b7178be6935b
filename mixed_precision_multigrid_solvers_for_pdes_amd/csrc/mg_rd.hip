// The reaction-diffusion stepper of libmghip.so (include/mghip_rd.h): device-resident implicit Euler, Crank-Nicolson and BDF2
// steps of  du/dt = alpha L_a u - kappa w phi(u) + rho u + g(t) S  with one semilinear Newton solve per step.  This unit
// instantiates the kernels of mg_rd_kernels.hpp and holds the stateless device forms and the driver.  The driver owns an mg_nl
// (and through it the Krylov loop and the preconditioner engine), on whose stream all of its work is queued:
//
//   f = rhs(u_src [, u_prev]) and sum f^2  ->  shift lambda when it changed  ->  u_dst = u_src [-> ring of u_dst]  ->
//   mg_nl_solve_device(f, u_dst) to tol max(1, ||f||_h)
//
// The state lives in four slots, as the heat stepper's; the ring fill and the difference norm are that stepper's exported
// device forms (mg_dev_heat_ring, mg_dev_heat_diff_sumsq).  Per step the host reads sum f^2 and the Newton method's two sums
// per trial.
#include "mg_host.hpp"
#include "../../include/mghip_rd.h"
#include "mg_rd_kernels.hpp"

#include <cstdint>

using namespace mgh;

namespace {
constexpr int kSlots = 4;
}

struct mg_rd {
  mg_config cfg;
  mg_nl* nl = nullptr;
  mg_handle* eng = nullptr;             // the preconditioner engine the mg_nl's mg_pcg owns: its stream and its staging field
  int nx = 0, ny = 0, ld = 0;
  double hx = 0, hy = 0, alpha = 0;
  double* slot[kSlots] = {nullptr, nullptr, nullptr, nullptr};
  double* rhs = nullptr;
  double* src = nullptr;                // source profile S (nullable)
  double* a = nullptr;                  // diffusivity field (nullable: the constant operator)
  double* w = nullptr;                  // weight of the reaction term (used when has_w)
  bool has_w = false;
  int kind = MG_NL_LINEAR;
  double kappa = 0.0, rho = 0.0;
  double* partials = nullptr;           // three sets (the energy)
  double* d_sums = nullptr;             // device, 3 doubles
  double* h_sums = nullptr;             // pinned host
  double lambda = -1.0;                 // the shift the mg_nl carries (< 0: none set yet)
  std::vector<double> norm_hist;
  std::string err;
};

namespace {

bool scheme_ok(int scheme) { return scheme >= MG_HEAT_IMPLICIT_EULER && scheme <= MG_HEAT_BDF2; }
// the sets of partials of the energy start `second` doubles apart (even: each starts 16-byte aligned)
int energy_second(int nx, int ny, int ld) { return (field_geom(nx, ny, ld).ntiles + 1) & ~1; }

// ---- launchers (shared by the driver and the stateless mg_dev_rd_* forms); an int result is the number of partials ----
template <int KIND>
void launch_rhs_cn(bool var, const double* u, const double* u_prev, const double* src, const double* a, const double* w, double* out,
                   double* partials, const mg::TileGeom& g, const mg::RdCoef& c, hipStream_t st) {
  auto k = var ? mg::rd_rhs_kernel<mg::kRdCn, KIND, true> : mg::rd_rhs_kernel<mg::kRdCn, KIND, false>;
  hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, u, u_prev, src, a, w, out, partials, g, c);
}

// kappa is the equation's: the kernel takes kappa / alpha, the strength the Newton method carries
int launch_rhs(int scheme, int kind, int nx, int ny, int ld, double hx, double hy, double alpha, double dt, double kappa, double rho,
               const double* u, const double* u_prev, const double* src, const double* a, const double* w, double g0, double g1,
               double* out, double* partials, hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  const Coef k = coefs(hx, hy);
  mg::RdCoef c;
  c.ihx2 = k.ihx2; c.ihy2 = k.ihy2; c.diag = k.diag;
  c.a = alpha; c.dt = dt;
  c.dta = dt * alpha;
  c.two_dta = 2 * dt * alpha;
  c.g0 = g0; c.g1 = g1;
  c.ka = kappa / alpha;
  c.rho = rho;
  c.ra = rho / alpha;
  c.r2a = (2.0 * rho) / alpha;
  if (scheme == MG_HEAT_CRANK_NICOLSON) {
    switch (kind) {
      case MG_NL_LINEAR: launch_rhs_cn<mg::kRdLinear>(a != nullptr, u, u_prev, src, a, w, out, partials, g, c, st); break;
      case MG_NL_CUBIC: launch_rhs_cn<mg::kRdCubic>(a != nullptr, u, u_prev, src, a, w, out, partials, g, c, st); break;
      case MG_NL_SINH: launch_rhs_cn<mg::kRdSinh>(a != nullptr, u, u_prev, src, a, w, out, partials, g, c, st); break;
      default: launch_rhs_cn<mg::kRdExp>(a != nullptr, u, u_prev, src, a, w, out, partials, g, c, st); break;
    }
  } else {
    auto kern = scheme == MG_HEAT_IMPLICIT_EULER ? mg::rd_rhs_kernel<mg::kRdImplicit, mg::kRdLinear, false>
                                                 : mg::rd_rhs_kernel<mg::kRdBdf2, mg::kRdLinear, false>;
    hipLaunchKernelGGL(kern, dim3(g.ntiles), dim3(mg::kBlock), 0, st, u, scheme == MG_HEAT_BDF2 ? u_prev : nullptr, src,
                       (const double*)nullptr, (const double*)nullptr, out, partials, g, c);
  }
  return g.ntiles;
}

template <int KIND>
void launch_energy_kind(const double* u, const double* a, const double* w, double* partials, const mg::TileGeom& g, double rx,
                        double ry, int second, hipStream_t st) {
  auto k = a ? mg::rd_energy_kernel<KIND, true> : mg::rd_energy_kernel<KIND, false>;
  hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, u, a, w, partials, g, rx, ry, second);
}

// the three sums of one state into sums3 (device)
void launch_energy(int kind, int nx, int ny, int ld, double hx, double hy, const double* a, const double* w, const double* u,
                   double* partials, double* sums3, hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  const int second = energy_second(nx, ny, ld);
  const double rx = hy / hx, ry = hx / hy;
  switch (kind) {
    case MG_NL_LINEAR: launch_energy_kind<mg::kRdLinear>(u, a, w, partials, g, rx, ry, second, st); break;
    case MG_NL_CUBIC: launch_energy_kind<mg::kRdCubic>(u, a, w, partials, g, rx, ry, second, st); break;
    case MG_NL_SINH: launch_energy_kind<mg::kRdSinh>(u, a, w, partials, g, rx, ry, second, st); break;
    default: launch_energy_kind<mg::kRdExp>(u, a, w, partials, g, rx, ry, second, st); break;
  }
  hipLaunchKernelGGL(mg::reduce_rows_kernel<false>, dim3(3), dim3(mg::kReduceBlock), 0, st, partials, g.ntiles, second, 0, sums3);
}

void launch_sum(const double* partials, int n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(mg::reduce_rows_kernel<false>, dim3(1), dim3(mg::kReduceBlock), 0, st, partials, n, 0, 0, out);
}

void release(mg_rd* s) {
  if (s->nl) { (void)mg_nl_destroy(s->nl); s->nl = nullptr; s->eng = nullptr; }      // the engine goes with its owner
  for (double** p : {&s->slot[0], &s->slot[1], &s->slot[2], &s->slot[3], &s->rhs, &s->src, &s->a, &s->w, &s->partials, &s->d_sums})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (s->h_sums) { (void)hipHostFree(s->h_sums); s->h_sums = nullptr; }
}

bool slot_ok(int k) { return k >= 0 && k < kSlots; }

// host array (nx, ny) of hdt -> fp64 device field with the stepper's pitch, on the engine's stream (through its staging field)
int put(mg_rd* s, double* dev, const void* host, int hdt) {
  return upload(&s->err, dev, MG_F64, s->ld, host, hdt, s->nx, s->ny, s->eng->staging, s->eng->stream);
}

// (re)place the optional device field *dev by the host array, or free it for NULL
int set_field(mg_rd* s, double** dev, const void* host_or_null, int hdt) {
  if (!host_or_null) {
    HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
    if (*dev) { (void)hipFree(*dev); *dev = nullptr; }
    return MG_OK;
  }
  if (!*dev) { const int rc = alloc_zero(&s->err, (void**)dev, field_bytes(s), s->eng->stream); if (rc != MG_OK) return rc; }
  return put(s, *dev, host_or_null, hdt);
}

}  // namespace

extern "C" {

// ---- the field kernels, call by call (pitch in elements, nullable stream, scratch >= mg_dev_scratch_bytes()) ----
int mg_dev_rd_rhs(int scheme, int kind, int nx, int ny, int ld, double hx, double hy, double alpha, double dt, double kappa,
                  double rho, const double* u, const double* u_prev_or_null, const double* src_or_null, const double* a_or_null,
                  const double* w_or_null, double g0, double g1, double* out, void* scratch, double* sumsq_dev_or_null,
                  void* stream) {
  CHECK_ARG(scheme != MG_HEAT_EXPLICIT_EULER, "mg_dev_rd_rhs: explicit Euler is not a reaction-diffusion scheme (implicit Euler, Crank-Nicolson, BDF2)");
  CHECK_ARG(scheme_ok(scheme), "mg_dev_rd_rhs: unknown scheme");
  CHECK_ARG(kind_ok(kind, MG_NL_LINEAR, MG_NL_EXP), "mg_dev_rd_rhs: unknown nonlinearity (mg_nl_kind)");
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_rd_rhs: bad shape / pitch");
  CHECK_ARG(pos_finite(dt) && pos_finite(alpha) && pos_finite(hx) && pos_finite(hy), "mg_dev_rd_rhs: dt, alpha and the spacings must be finite and > 0");
  CHECK_ARG(kappa_ok(kappa) && std::isfinite(kappa / alpha), "mg_dev_rd_rhs: kappa must be finite and >= 0 (monotone nonlinearities only)");
  CHECK_ARG(std::isfinite(rho) && std::isfinite((2.0 * rho) / alpha), "mg_dev_rd_rhs: rho must be finite");
  CHECK_ARG(u && out && scratch, "mg_dev_rd_rhs: NULL pointer");
  CHECK_ARG(scheme != MG_HEAT_BDF2 || u_prev_or_null, "mg_dev_rd_rhs: BDF2 needs u_prev");
  const bool cn = scheme == MG_HEAT_CRANK_NICOLSON;
  const double* prev = scheme == MG_HEAT_IMPLICIT_EULER ? nullptr : u_prev_or_null;
  const double* a = cn ? a_or_null : nullptr;
  const double* w = cn ? w_or_null : nullptr;
  CHECK_ARG(!overlap(out, u, nx, ld) && !overlap(out, prev, nx, ld) && !overlap(out, src_or_null, nx, ld) &&
            !overlap(out, a, nx, ld) && !overlap(out, w, nx, ld), "mg_dev_rd_rhs: out is an array of its own (it overlaps an input)");
  CHECK_ARG(aligned16(u) && aligned16(out) && aligned16(prev) && aligned16(src_or_null) && aligned16(a) && aligned16(w),
            "mg_dev_rd_rhs: unaligned pointer");
  const int n = launch_rhs(scheme, kind, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, u, prev, src_or_null, a, w, g0, g1, out,
                           (double*)scratch, (hipStream_t)stream);
  if (sumsq_dev_or_null) launch_sum((double*)scratch, n, sumsq_dev_or_null, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_rd_energy(int kind, int nx, int ny, int ld, double hx, double hy, const double* a_or_null, const double* w_or_null,
                     const double* u, void* scratch, double* sums3_dev, void* stream) {
  CHECK_ARG(kind_ok(kind, MG_NL_LINEAR, MG_NL_EXP), "mg_dev_rd_energy: unknown nonlinearity (mg_nl_kind)");
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_rd_energy: bad shape / pitch");
  CHECK_ARG(pos_finite(hx) && pos_finite(hy), "mg_dev_rd_energy: the spacings must be finite and > 0");
  CHECK_ARG(u && scratch && sums3_dev, "mg_dev_rd_energy: NULL pointer");
  CHECK_ARG(aligned16(u) && aligned16(a_or_null) && aligned16(w_or_null), "mg_dev_rd_energy: unaligned pointer");
  int64_t bytes = 0;
  (void)mg_dev_scratch_bytes(nx, ny, &bytes);
  CHECK_ARG((int64_t)sizeof(double) * 3 * energy_second(nx, ny, ld) <= bytes, "mg_dev_rd_energy: the scratch of this shape does not hold three sets of partials");
  launch_energy(kind, nx, ny, ld, hx, hy, a_or_null, w_or_null, u, (double*)scratch, sums3_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

// ---- the driver ----
int mg_rd_create(const mg_config* cfg, double alpha, int num_cycles, int flexible, mg_rd** out) {
  if (!cfg || !out) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_rd_create: NULL argument");
  *out = nullptr;
  if (cfg->precision != MG_PREC_DOUBLE && cfg->precision != MG_PREC_SINGLE_MANAGED && cfg->precision != MG_PREC_MIXED_LEVELS)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_rd_create: the preconditioner runs in MG_PREC_DOUBLE, MG_PREC_SINGLE_MANAGED or MG_PREC_MIXED_LEVELS (the state is fp64)");
  if (cfg->coeff != -1.0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_rd_create: coeff must be -1 (the steps solve (-L_a + lambda) u + (kappa/alpha) w phi(u) = f)");
  if (cfg->fmg_cycles != 0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_rd_create: fmg_cycles must be 0 (a step starts from the old time level)");
  if (!pos_finite(alpha)) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_rd_create: alpha must be finite and > 0");
  mg_nl* nl = nullptr;
  int rc = mg_nl_create(cfg, num_cycles, flexible, &nl);
  if (rc != MG_OK) return rc;
  mg_rd* s = new mg_rd();
  s->cfg = *cfg;
  s->nl = nl;
  s->eng = nl_engine(nl);
  s->nx = cfg->nx; s->ny = cfg->ny;
  (void)mg_pitch_elems(MG_F64, cfg->ny, &s->ld);
  s->hx = s->eng->lv[0].hx; s->hy = s->eng->lv[0].hy;
  s->alpha = alpha;
  auto bail = [&](int code) { return create_fail(s, release, code); };
  hipStream_t st = s->eng->stream;
  for (double** p : {&s->slot[0], &s->slot[1], &s->slot[2], &s->slot[3], &s->rhs})
    if ((rc = alloc_zero(&s->err, (void**)p, field_bytes(s), st)) != MG_OK) return bail(rc);
  int64_t scratch = 0;
  (void)mg_dev_scratch_bytes(s->nx, s->ny, &scratch);
  scratch = std::max<int64_t>(scratch, (int64_t)sizeof(double) * 3 * energy_second(s->nx, s->ny, s->ld));
  if ((rc = alloc_zero(&s->err, (void**)&s->partials, (size_t)scratch, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->d_sums, 3 * sizeof(double), st)) != MG_OK) return bail(rc);
  if (hipHostMalloc((void**)&s->h_sums, 3 * sizeof(double)) != hipSuccess) { s->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  if (hipStreamSynchronize(st) != hipSuccess) { s->err = "hipStreamSynchronize failed"; return bail(MG_ERR_HIP); }
  *out = s;
  return MG_OK;
}

int mg_rd_destroy(mg_rd* s) {
  return destroy_owned(s, s && s->eng ? s->eng->stream : nullptr, release);
}

const char* mg_rd_last_error(const mg_rd* s) { return s ? s->err.c_str() : last_error().c_str(); }

int mg_rd_set_slot(mg_rd* s, int slot, const void* u_host, int host_dtype) {
  if (!s || !u_host || !valid_dtype(host_dtype) || !slot_ok(slot)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_slot: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  return put(s, s->slot[slot], u_host, host_dtype);
}

int mg_rd_get_slot(mg_rd* s, int slot, void* u_host, int host_dtype) {
  if (!s || !u_host || !valid_dtype(host_dtype) || !slot_ok(slot)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_get_slot: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  return download(&s->err, u_host, host_dtype, s->slot[slot], MG_F64, s->ld, s->nx, s->ny, s->eng->staging, s->eng->stream);
}

int mg_rd_set_slot_device(mg_rd* s, int slot, const void* u_dev, int ld, int dtype) {
  if (!s || !u_dev || !valid_dtype(dtype) || !slot_ok(slot) || ld < s->ny) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_slot_device: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_dev_convert(dtype, MG_F64, s->nx, s->ny, ld, s->ld, u_dev, s->slot[slot], s->eng->stream), "", mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
  return MG_OK;
}

int mg_rd_get_slot_device(mg_rd* s, int slot, void* u_dev, int ld, int dtype) {
  if (!s || !u_dev || !valid_dtype(dtype) || !slot_ok(slot) || ld < s->ny) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_get_slot_device: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_dev_convert(MG_F64, dtype, s->nx, s->ny, s->ld, ld, s->slot[slot], u_dev, s->eng->stream), "", mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(s->eng->stream));
  return MG_OK;
}

int mg_rd_set_source(mg_rd* s, const void* profile_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_source: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  return set_field(s, &s->src, profile_host_or_null, host_dtype);
}

int mg_rd_set_coefficient(mg_rd* s, const void* a_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_coefficient: bad argument");
  if (a_host_or_null) {                                           // before any device work
    const size_t n = (size_t)s->nx * s->ny;
    const bool ok = host_dtype == MG_F32 ? coefficient_ok((const float*)a_host_or_null, n) : coefficient_ok((const double*)a_host_or_null, n);
    if (!ok) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_coefficient: the diffusivity field must be finite and > 0 everywhere");
  }
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_nl_set_coefficient(s->nl, a_host_or_null, host_dtype), "Newton solver: ", mg_nl_last_error(s->nl));
  s->lambda = -1.0;                 // the shift (and with it the reciprocal diagonals) is set again by the next step
  return set_field(s, &s->a, a_host_or_null, host_dtype);
}

int mg_rd_set_reaction(mg_rd* s, int kind, double kappa, const void* w_host_or_null, int host_dtype, double rho) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_rd_set_reaction: NULL stepper");
  if (!kind_ok(kind, MG_NL_LINEAR, MG_NL_EXP)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_reaction: unknown nonlinearity (mg_nl_kind)");
  if (!kappa_ok(kappa) || !std::isfinite(kappa / s->alpha))
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_reaction: kappa must be finite and >= 0 (monotone nonlinearities only; rho carries a term of the other sign explicitly)");
  if (!std::isfinite(rho) || !std::isfinite((2.0 * rho) / s->alpha)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_reaction: rho must be finite");
  if (!valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_reaction: bad dtype");
  if (w_host_or_null) {
    const size_t n = (size_t)s->nx * s->ny;
    const bool ok = host_dtype == MG_F32 ? weight_ok((const float*)w_host_or_null, n) : weight_ok((const double*)w_host_or_null, n);
    if (!ok) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_set_reaction: the weight field must be finite and >= 0 (monotone nonlinearities only)");
  }
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_nl_set_nonlinearity(s->nl, kind, kappa / s->alpha, w_host_or_null, host_dtype), "Newton solver: ", mg_nl_last_error(s->nl));
  if (w_host_or_null) {
    if (!s->w) { const int rc = alloc_zero(&s->err, (void**)&s->w, field_bytes(s), s->eng->stream); if (rc != MG_OK) return rc; }
    const int rc = put(s, s->w, w_host_or_null, host_dtype);
    if (rc != MG_OK) return rc;
  }
  s->has_w = w_host_or_null != nullptr;
  s->kind = kind;
  s->kappa = kappa;
  s->rho = rho;
  return MG_OK;
}

int mg_rd_set_newton_options(mg_rd* s, const mg_nl_options* opt) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_rd_set_newton_options: NULL stepper");
  OWNED(mg_nl_set_options(s->nl, opt), "Newton solver: ", mg_nl_last_error(s->nl));
  return MG_OK;
}

int mg_rd_step(mg_rd* s, int scheme, double dt, int src, int prev, int dst, double g0, double g1, const double* edge4_or_null,
               double tol, int max_newton, mg_rd_step_info* info) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_rd_step: NULL stepper");
  if (scheme == MG_HEAT_EXPLICIT_EULER) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: explicit Euler is not a reaction-diffusion scheme (implicit Euler, Crank-Nicolson, BDF2)");
  if (!scheme_ok(scheme)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: unknown scheme");
  if (!pos_finite(dt) || !pos_finite(dt * s->alpha)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: dt must be finite and > 0");
  if (!slot_ok(src) || !slot_ok(dst) || src == dst) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: src and dst are two different slots 0..3");
  if (scheme == MG_HEAT_BDF2) {
    if (!slot_ok(prev) || prev == dst) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: BDF2 reads a prev slot 0..3 other than dst");
  } else if (scheme == MG_HEAT_CRANK_NICOLSON) {
    if (prev != -1 && (!slot_ok(prev) || prev == dst)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: Crank-Nicolson's prev is -1 or a slot 0..3 other than dst");
  } else if (prev != -1) {
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: prev is -1 for implicit Euler");
  }
  if (!std::isfinite(g0) || !std::isfinite(g1)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: g0 / g1 not finite");
  if (max_newton < 1 || !(tol == tol)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_step: max_newton < 1 / tol is NaN");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  hipStream_t st = s->eng->stream;
  const double dta = dt * s->alpha;
  const double lambda = scheme == MG_HEAT_IMPLICIT_EULER ? 1.0 / dta : scheme == MG_HEAT_CRANK_NICOLSON ? 2.0 / dta : 3.0 / (2 * dt * s->alpha);
  const int np = launch_rhs(scheme, s->kind, s->nx, s->ny, s->ld, s->hx, s->hy, s->alpha, dt, s->kappa, s->rho, s->slot[src],
                            prev >= 0 ? s->slot[prev] : nullptr, s->src, s->a, s->has_w ? s->w : nullptr, g0, g1, s->rhs,
                            s->partials, st);
  launch_sum(s->partials, np, s->d_sums, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sums, s->d_sums, sizeof(double), hipMemcpyDeviceToHost, st));
  if (lambda != s->lambda) { OWNED(mg_nl_set_shift(s->nl, lambda), "Newton solver: ", mg_nl_last_error(s->nl)); s->lambda = lambda; }
  // the Newton method iterates in place: dst := the initial iterate (src, or src with the ring of t + dt), then the solve
  HIPC(&s->err, hipMemcpyAsync(s->slot[dst], s->slot[src], field_bytes(s), hipMemcpyDeviceToDevice, st));
  if (edge4_or_null) OWNED(mg_dev_heat_ring(s->nx, s->ny, s->ld, edge4_or_null, s->slot[dst], st), "", mg_last_error(nullptr));
  HIPC(&s->err, hipStreamSynchronize(st));                        // sum f^2 has arrived
  const double fnorm = std::sqrt(s->hx * s->hy * s->h_sums[0]);
  if ((int)s->norm_hist.size() < max_newton) s->norm_hist.resize(max_newton);
  int n = 0, conv = 0;
  mg_nl_stats stats;
  OWNED(mg_nl_solve_device(s->nl, s->rhs, s->ld, s->slot[dst], s->ld, MG_F64, tol * std::max(1.0, fnorm), max_newton,
                        s->norm_hist.data(), nullptr, nullptr, nullptr, max_newton, &n, &conv, &stats), "Newton solver: ", mg_nl_last_error(s->nl));
  if (info) {
    info->lambda = lambda;
    info->rhs_norm = fnorm;
    info->initial_residual = stats.initial_residual;
    info->final_residual = stats.final_residual;
    info->solve_seconds = stats.solve_seconds;
    info->newton_iterations = stats.newton_iterations;
    info->inner_iterations = stats.inner_iterations;
    info->evaluations = stats.evaluations;
    info->status = stats.status;
    info->converged = conv;                                      // a breakdown or a failed line search ends the step unconverged
    info->reserved = 0;
  }
  return MG_OK;
}

int mg_rd_energy(mg_rd* s, int slot, double out[4]) {
  if (!s || !out || !slot_ok(slot)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_energy: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  hipStream_t st = s->eng->stream;
  launch_energy(s->kind, s->nx, s->ny, s->ld, s->hx, s->hy, s->a, s->has_w ? s->w : nullptr, s->slot[slot], s->partials, s->d_sums, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sums, s->d_sums, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(&s->err, hipStreamSynchronize(st));
  out[0] = s->h_sums[0]; out[1] = s->h_sums[1]; out[2] = s->h_sums[2];
  out[3] = s->alpha * out[0] + (s->hx * s->hy) * (s->kappa * out[1] - (s->rho * out[2]) / 2);
  return MG_OK;
}

int mg_rd_diff_norm(mg_rd* s, int slot_a, int slot_b, double* out) {
  if (!s || !out || !slot_ok(slot_a) || !slot_ok(slot_b)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_rd_diff_norm: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  hipStream_t st = s->eng->stream;
  OWNED(mg_dev_heat_diff_sumsq(s->nx, s->ny, s->ld, s->slot[slot_a], s->slot[slot_b], s->partials, s->d_sums, st), "", mg_last_error(nullptr));
  HIPC(&s->err, hipMemcpyAsync(s->h_sums, s->d_sums, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(&s->err, hipStreamSynchronize(st));
  *out = std::sqrt(s->hx * s->hy * s->h_sums[0]);
  return MG_OK;
}

}  // extern "C"
