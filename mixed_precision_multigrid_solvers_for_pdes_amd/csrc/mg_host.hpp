// Host-side types and helpers shared by the translation units of libmghip.so (mg_launch.hip: the kernel launchers;
// mg_engine.hip: the handle and the cycle driver; mg_solve.hip: norms, precision policy and the solve loop; mg_dev.hip: the
// stateless C ABI; mg_tail.hip: the register-resident coarse tail) and by the solver units on top of the engine (mg_pcg,
// mg_heat, mg_eig, mg_ho, mg_flow, mg_nl, mg_rd, mg_line).  What those units would otherwise each define lives here, once:
// the argument predicates and CHECK_ARG of the stateless device forms, the whole-field tile geometry (field_geom), the error
// plumbing of an object that owns an engine or another solver (sfail, OWNED), its create / destroy boilerplate (create_fail,
// destroy_owned) and, declared here and defined in mg_engine.hip, the host transfers (upload, download) and the hand-over of
// a right-hand side to an engine (engine_set_rhs, engine_precondition).  Launch shapes and their caps stay in the units.
// Internal: nothing here is part of the C ABI (include/mghip.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mghip.h"
#include "../../include/mghip_heat.h"
#include "mg_kernels.hpp"

struct mg_line_plan;   // mg_line.hip: the tables of one (dtype, direction, shape, spacings, sigma) of the zebra line smoothers
struct mg_nl;          // mg_nl.hip: the semilinear Newton driver

namespace mgh {

// The thread's last error message (mg_last_error(NULL)); the one definition is in mg_engine.hip.
std::string& last_error();
inline int fail(std::string* where, int code, const std::string& msg) {
  last_error() = msg;
  if (where) *where = msg;
  return code;
}
#define HIPC(errstr, call)                                                                         \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess)                                                                          \
      return fail(errstr, (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? MG_ERR_NO_DEVICE : \
                          (e_ == hipErrorOutOfMemory ? MG_ERR_ALLOC : MG_ERR_HIP),                 \
                  std::string(#call) + ": " + hipGetErrorString(e_));                              \
  } while (0)

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline size_t esize(int dt) { return dt == MG_F32 ? 4 : 8; }
inline bool valid_dtype(int dt) { return dt == MG_F32 || dt == MG_F64; }

// ---- what the solver units and the stateless device forms share ----
// an argument check of a stateless form (no object to keep the message: the thread's last error gets it)
#define CHECK_ARG(cond, msg) do { if (!(cond)) return fail(nullptr, MG_ERR_INVALID_VALUE, msg); } while (0)
// a failure of a solver object (nullable): the message goes to the object and to the thread
template <class S> int sfail(S* s, int code, const std::string& msg) { return fail(s ? &s->err : nullptr, code, msg); }
// a call into an object that `s` owns (an engine, an mg_pcg, an mg_nl) or into a stateless form of another unit: when it
// fails, its message (`owner_msg`, read after the call) joins s's under `prefix` and the calling function returns its code
#define OWNED(call, prefix, owner_msg) \
  do { const int rc_ = (call); if (rc_ != MG_OK) return sfail(s, rc_, std::string(prefix) + (owner_msg)); } while (0)
// a *_create that fails after the object exists: free what it holds, and leave its message as the thread's
template <class S> int create_fail(S* s, void (*release)(S*), int code) {
  release(s);
  const std::string m = s->err;
  delete s;
  last_error() = m;
  return code;
}
// *_destroy: wait for the stream that carries the object's work (NULL: none), then free what it holds
template <class S> int destroy_owned(S* s, hipStream_t st, void (*release)(S*)) {
  if (!s) return MG_OK;
  (void)hipSetDevice(s->cfg.device);
  if (st) (void)hipStreamSynchronize(st);
  release(s);
  delete s;
  return MG_OK;
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// pitch of an fp64 field: whole 16-byte vectors per row (mg_dev.hip has the dtype-aware rule)
inline bool ld_ok_f64(int ny, int ld) { return ld >= ny && ld % 2 == 0; }
// do the fp64 fields a and b (nx rows of pitch ld; b may be NULL) share an element?
inline bool overlap(const double* a, const double* b, int nx, int ld) {
  const uintptr_t n = (uintptr_t)nx * (uintptr_t)ld * sizeof(double), pa = (uintptr_t)a, pb = (uintptr_t)b;
  return b && pa < pb + n && pb < pa + n;
}
inline bool pos_finite(double x) { return x > 0.0 && std::isfinite(x); }
inline bool operator_ok(double hx, double hy, double coeff, double sigma) {
  return hx > 0.0 && hy > 0.0 && std::isfinite(hx) && std::isfinite(hy) && std::isfinite(coeff) && sigma >= 0.0 && std::isfinite(sigma);
}
// a nonlinearity of include/mghip_nl.h, which this header does not see: the caller names the first and the last kind
inline bool kind_ok(int kind, int first, int last) { return kind >= first && kind <= last; }
inline bool kappa_ok(double kappa) { return kappa >= 0.0 && std::isfinite(kappa); }
// every entry of a host field finite and >= 0 (a weight) / > 0 (a diffusivity)
template <typename T> bool weight_ok(const T* w, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!(w[k] >= T(0)) || !std::isfinite((double)w[k])) return false;
  return true;
}
template <typename T> bool coefficient_ok(const T* a, size_t n) {
  for (size_t k = 0; k < n; ++k)
    if (!(a[k] > T(0)) || !std::isfinite((double)a[k])) return false;
  return true;
}

// bytes of one fp64 field of a solver object
template <class S> size_t field_bytes(const S* s) { return (size_t)s->nx * s->ld * sizeof(double); }
// The tile geometry of a whole fp64 field, ring rows included (i_org = 0): what every LDS-tiled kernel of the solver units
// is launched over, one workgroup per tile.  (The engine's smoothers tile the interior alone: make_geom, mg_launch.hip.)
inline mg::TileGeom field_geom(int nx, int ny, int ld) {
  using S = mg::TileShape<double>;
  mg::TileGeom g;
  g.nx = nx; g.ny = ny; g.ld = ld;
  g.nyv = std::min(ld, (ny + S::N - 1) / S::N * S::N);
  g.i_org = 0;
  g.tiles_j = (ny + S::TJ - 1) / S::TJ;
  g.ntiles = (nx + mg::kTI - 1) / mg::kTI * g.tiles_j;
  return g;
}

// dtype codes -> element types: calls f with a float (MG_F32) or double (anything else) value per code, so that the
// generic lambda f names the types with decltype.  Every combination is instantiated: a site that accepts fewer rejects
// the others with if constexpr.
template <typename F> inline decltype(auto) with_dtype(int a, F&& f) { return a == MG_F32 ? f(float()) : f(double()); }
template <typename F> inline decltype(auto) with_dtype(int a, int b, F&& f) {
  return with_dtype(a, [&](auto x) -> decltype(auto) { return with_dtype(b, [&](auto y) -> decltype(auto) { return f(x, y); }); });
}
template <typename F> inline decltype(auto) with_dtype(int a, int b, int c, F&& f) {
  return with_dtype(a, b, [&](auto x, auto y) -> decltype(auto) { return with_dtype(c, [&](auto z) -> decltype(auto) { return f(x, y, z); }); });
}
template <typename F> inline decltype(auto) with_smoother(int sm, F&& f) {
  return sm == MG_RBGS ? f(std::integral_constant<int, mg::kSmRbgs>()) : f(std::integral_constant<int, mg::kSmJacobi>());
}
// fp32 interpolation (TC) only exists for an all-fp32 grid (fine T, coarse TX)
template <typename T, typename TX, typename TC>
constexpr bool interp_ok = !std::is_same_v<TC, float> || (std::is_same_v<T, float> && std::is_same_v<TX, float>);
// the coarse tails' (T, TCO) = (upper levels, coarsest level and interpolation): an fp64 tail (dt) is fp64 throughout, an fp32
// tail solves its coarsest level in the grid dtype dco.  Instantiates (double, double), (float, float), (float, double) in
// this order, which fixes where the tail kernels sit in the code object (their calls are PC-relative).
template <typename F> inline decltype(auto) with_tail_dtypes(int dt, int dco, F&& f) {
  return dt == MG_F64 ? f(double(), double()) : with_dtype(dco, [&](auto co) -> decltype(auto) { return f(float(), co); });
}

struct Coef {
  double ihx2, ihy2, diag, invD;
  bool pow2;       // 1/diag is exact: multiply instead of divide
  bool all_pow2;   // hx^2, hy^2 and diag are all powers of two
};
// sigma: Helmholtz shift, A = coeff * (Laplacian_h - sigma I) (coeff = -1: -Laplacian + sigma); it only moves the
// diagonal, so every constant-coefficient kernel serves the shifted operator unchanged (sigma = 0: the reference's).
inline Coef coefs(double hx, double hy, double sigma = 0.0) {
  Coef c;
  c.ihx2 = 1.0 / (hx * hx);
  c.ihy2 = 1.0 / (hy * hy);
  c.diag = 2.0 / (hx * hx) + 2.0 / (hy * hy);   // operators/laplacian.py:76, smoothers.py:65
  if (sigma != 0.0) c.diag += sigma;
  c.invD = 1.0 / c.diag;
  int e = 0;
  c.pow2 = std::frexp(c.diag, &e) == 0.5;
  c.all_pow2 = c.pow2 && std::frexp(hx * hx, &e) == 0.5 && std::frexp(hy * hy, &e) == 0.5;
  return c;
}

// Whether a register-blocked fp64 leg may evaluate its stencil in the exact-FMA forms of RowMath (mg_rb_kernels.hpp):
//   sweep      un = fma(S, a, f) * invD                          for   nb = a (dn + up) + a (ea + wv);  un = (f + nb) * invD
//   residual   r  = fma(-coeff a, fma(mid, -4, S), f)            for   r = f - coeff (((dn + up) a + (ea + wv) a) - mid D)
// with S = (dn + up) + (ea + wv).  Constant coefficients without a shift, 1/hx^2 = 1/hy^2 = a = 2^p, D = 4 a and coeff = 0 or
// +-2^k: every product of the plain forms is then a scaling by a power of two, which is exact and commutes with rounding, so
// a s1 + a s2 = a rn(s1 + s2) and each FMA rounds exactly once where the plain form rounds once: the same bits for every
// finite input, unless the plain form itself overflows on the way (|a S| beyond the largest double).  a >= 1 and
// |coeff| a >= 1 keep every scaling from shrinking a value, so none of them can round in the subnormal range.
inline bool pow2_stencil(const Coef& c, bool fp64, const void* acoef, double sigma, double coeff) {
  int e = 0;
  return fp64 && acoef == nullptr && sigma == 0.0 && c.all_pow2 && c.ihx2 == c.ihy2 && c.diag == 4.0 * c.ihx2 && c.ihx2 >= 1.0 &&
         (coeff == 0.0 || (std::frexp(std::fabs(coeff), &e) == 0.5 && std::fabs(coeff) * c.ihx2 >= 1.0));
}

// min{x >= 0 : sqrt(x) >= tol}: "sqrt(x) < tol" and "x < sqrt_threshold(tol)" decide alike for every double x (IEEE sqrt is
// correctly rounded, hence monotone) -- lets a latency-bound stop test skip the square root.  tol <= 0 never stops.
inline double sqrt_threshold(double tol) {
  if (!(tol > 0.0)) return 0.0;
  thread_local double last_tol = -1.0, last_thr = 0.0;       // one tolerance per solver in practice: launched per tail visit
  if (tol == last_tol) return last_thr;
  last_tol = tol;
  double y = tol * tol;
  while (y > 0.0 && std::sqrt(y) >= tol) y = std::nextafter(y, 0.0);
  while (std::sqrt(y) < tol) y = std::nextafter(y, INFINITY);
  last_thr = y;
  return y;
}

struct Level {
  int nx = 0, ny = 0;
  double hx = 0, hy = 0;
  int ld[2] = {0, 0};
  void* u[2] = {nullptr, nullptr};     // current iterate
  void* t[2] = {nullptr, nullptr};     // Jacobi ping-pong partner (same boundary ring as u)
  void* s[2] = {nullptr, nullptr};     // level 0, allocated on first use: third buffer of the spanning leg (cycle_span)
  void* rhs[2] = {nullptr, nullptr};
  void* r[2] = {nullptr, nullptr};     // residual
  void* a[2] = {nullptr, nullptr};     // diffusion coefficient (variable-coefficient operator), else null
  void* rd[2] = {nullptr, nullptr};    // its reciprocal diagonal 1 / D per cell (var_rdiag_kernel): what the sweeps multiply by
  mg_line_plan* lp[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // zebra line smoothers: plan per [dtype][0 X, 1 Y]
  double timings[3] = {0, 0, 0};       // smooth / restrict / prolong seconds (cfg.profile)
};


// Experiment switches (tile heights, streaming hints, schedule limits) are read from the environment only in measurement
// builds (-DMG_EXPERIMENTS, tools/README.md); the shipped library ignores them.
#ifdef MG_EXPERIMENTS
inline int exp_env(const char* name, int dflt) { const char* e = std::getenv(name); return e ? std::atoi(e) : dflt; }
#else
inline int exp_env(const char*, int dflt) { return dflt; }
#endif

}  // namespace mgh

struct mg_handle {
  mg_config cfg;
  std::vector<mgh::Level> lv;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;   // created by mg_create; `stream` may be redirected by mg_set_stream
  double* partials = nullptr;   // device: one fp64 partial per workgroup of the largest reduction (sized in mg_create)
  double* d_scalar = nullptr;   // device, one double
  int* d_int = nullptr;         // device, one int (coarse sweeps)
  double* h_scalar = nullptr;   // pinned host
  int* h_int = nullptr;         // pinned host
  mg::HostMailbox* mbox = nullptr;       // pinned, mapped: the norm of every iteration arrives here
  mg::HostMailbox* mbox_dev = nullptr;   // its device-side address
  unsigned long long mbox_seq = 0;
  void* staging = nullptr;      // fine-level sized fp64 staging for dtype-converting transfers
  int grid_dtype = MG_F64;      // the reference Grid's dtype: MG_F32 only for MG_PREC_SINGLE
  int phase = MG_F64;           // working precision of the adaptive policy
  bool promoted = false;        // one-way rule: fp32 -> fp64 happened
  double fp32_floor = 0.0;      // adaptive policy: eps32 * diag(A) * ||u||_h of the current solve's fp32 phase (0: not evaluated)
  int switch_reason = 0;        // why the fp32 phase of the current solve ended (mg_stats.switch_reason)
  bool have_rhs = false;
  bool varcoef = false;          // A = coeff * div(a grad .) with the per-level fields lv[l].a
  double sigma = 0.0;            // Helmholtz shift: A = coeff * (Laplacian - sigma I) on every level (mg_set_shift)
  double rd_sigma = -1.0;        // the shift the reciprocal diagonals lv[l].rd were computed for (< 0: stale)
  double ring_sumsq[2] = {0, 0};   // sum of f^2 over the boundary ring of the fine rhs, per dtype (r = f there)
  unsigned rhs_gen = 1;            // bumped by every new right-hand side
  unsigned rings_gen[2] = {0, 0};  // rhs_gen the coarse rhs rings of working precision p were injected for (adaptive policy)
  bool iterate_zero = false;       // the fine iterate is zero everywhere (mg_set_solution(NULL) / mg_zero_solution_device, no cycle since)
  unsigned zero_norm_gen[2] = {0, 0};   // ||f - A 0|| = ||f|| as the norm kernel sums it, per dtype, for right-hand side rhs_gen
  double zero_norm_val[2] = {0, 0};
  int norm_partials = 0;           // > 0: `partials` holds sum r^2 over interior cells of the CURRENT fine iterate
  int tail_start = -1;             // first level of the single-workgroup LDS tail (-1: none)
  bool span_ring[2] = {false, false};   // the third level-0 buffer (Level::s) carries the Dirichlet ring of this solve
  int tail2_start = -1;            // first level of the register-resident tail (mg_tail.hip; -1: none); it takes precedence
  int tail2_ntop = 0;              // points per side of that level (65, 33 or 17)
  int* d_tail_ops = nullptr;       // device copy of the tail schedule
  int tail_nops = 0;
  bool tail_direct = false;        // cfg.coarse_direct applies: 5 x 5 coarsest grid inside the tail; tail_minv is its inverse
  double tail_minv[81] = {0};
  double* d_minv = nullptr;        // a coarsest grid other than 5 x 5 with <= 64 unknowns: its n x n inverse on the device (LDS tail)
  int minv_n = 0;
  double tail_minv_sigma = -1.0;   // the shift tail_minv was built for (rebuilt when mg_set_shift changes it)
  std::string err;
  std::vector<double> adapt_hist;

  int L() const { return (int)lv.size(); }
  // visits of level l + 1 per visit of level l: V 1, W 2, F 2^(L-l-2) (multigrid.py:315-319)
  int visits(int l) const {
    return cfg.cycle == MG_CYCLE_W ? 2 : cfg.cycle == MG_CYCLE_F ? std::max(1, 1 << std::max(0, L() - l - 2)) : 1;
  }
  // precision a level computes in (solvers/multigrid.py:275-285 + core/precision.py:337-357); the coarsest
  // level is never converted by the reference (multigrid.py:270-272 returns first) and stays in the grid dtype.
  int level_dtype_in(int l, int ph) const {
    if (l == L() - 1) return grid_dtype;
    switch (cfg.precision) {
      case MG_PREC_SINGLE: return MG_F32;
      case MG_PREC_SINGLE_MANAGED: return MG_F32;
      case MG_PREC_DEFECT: return MG_F32;          // the error equation's hierarchy; the iterate itself is fp64 (iterate_dtype)
      case MG_PREC_MIXED_LEVELS: return (l >= (cfg.mixed_split > 0 ? cfg.mixed_split : L() / 2)) ? MG_F32 : MG_F64;
      case MG_PREC_ADAPTIVE: return ph;
      default: return MG_F64;
    }
  }
  int level_dtype(int l) const { return level_dtype_in(l, phase); }
  bool fused() const { return cfg.fused != 0 && (cfg.smoother == MG_JACOBI || cfg.smoother == MG_RBGS); }
  bool needs(int l, int dt) const {
    if (cfg.precision == MG_PREC_ADAPTIVE) return (l == L() - 1) ? dt == grid_dtype : true;
    if (cfg.precision == MG_PREC_DEFECT && l == 0 && dt == MG_F64) return true;      // fp64 iterate, its ping-pong partner and f
    return level_dtype(l) == dt;
  }
  // precision of the fine iterate the caller sets / gets: the level-0 working precision, except for defect correction
  int iterate_dtype() const { return cfg.precision == MG_PREC_DEFECT ? MG_F64 : level_dtype(0); }
};


namespace mgh {
// mg_tail.hip: the register-resident coarse tail (mg_tail_kernels.hpp).  tail2_plan decides whether it serves the handle's
// hierarchy (and from which level) and fills h->tail2_*; tail2_launch runs one visit of that sub-cycle on h->stream.
int tail2_plan(mg_handle* h);
int tail2_launch(mg_handle* h, bool zero_top);

// mg_line.hip: zebra line relaxation (mg_line_kernels.hpp).  dir: 0 X lines, 1 Y lines.  line_plan_set_sigma rebuilds the
// tables in place: the caller has waited for every launch that reads them.  d_line_colour: one colour pass, in place.
inline bool is_zebra(int sm) { return sm >= MG_ZEBRA_X && sm <= MG_ZEBRA_ALT; }
bool line_shape_ok(int nx, int ny);
int line_plan_make(int dtype, int dir, int nx, int ny, int ld, double hx, double hy, double sigma, mg_line_plan** out,
                   std::string* err);
void line_plan_free(mg_line_plan* p);
int line_plan_set_sigma(mg_line_plan* p, double sigma, std::string* err);
void d_line_colour(const mg_line_plan* p, int colour, double omega, void* u, const void* rhs, hipStream_t st);

// mg_ho.hip: the fourth-order compact nine-point operator A4 and its right-hand side average R (mg_ho_kernels.hpp;
// include/mghip_ho.h), fp64 fields with pitch ld, constant coefficients.  An int result is the number of partials written.
//   direction: p_out = z + beta p_in (beta NULL: z), q = A4 p_out, partials of p_out . q   (pcg_direction_kernel's contract)
//   residual:  r = g - A4 x on interior cells, 0 on the ring (r NULL: not stored), partials of the sum of r^2
//   rhs:       g = R f on interior cells, the ring of f on the ring
int d_ho_direction(const double* z, const double* p_in, double* p_out, double* q, const double* beta, double* partials, int nx,
                   int ny, int ld, double hx, double hy, double coeff, double sigma, hipStream_t st);
int d_ho_residual(const double* x, const double* g, double* r, double* partials, int nx, int ny, int ld, double hx, double hy,
                  double coeff, double sigma, hipStream_t st);
void d_ho_rhs(const double* f, double* g, int nx, int ny, int ld, hipStream_t st);

// mg_nl.hip: the one-pass kernel of the semilinear Newton method (mg_nl_kernels.hpp; include/mghip_nl.h), fp64 fields with
// pitch ld.  v = u + t delta (delta NULL: u), F = (f - A v) - kappa w phi(v), c = kappa w phi'(v) (w NULL: 1); u_out, F and c
// are nullable.  Returns the number of partials of the sum of F^2 at partials[0 ..]; as many of the sum of c start at
// partials[*second] (second is even; 2 * max_partials(nx, ny) doubles hold both).  The Krylov loop (mg_pcg.hip) takes its
// residuals under a reaction field from it: kind 0 (linear), kappa = 1, w = the field.
int d_nl_eval(int kind, const double* u, const double* delta, double t, const double* a, const double* w, const double* f,
              double* u_out, double* F, double* c, double* partials, int* second, int nx, int ny, int ld, double hx, double hy,
              double coeff, double sigma, double kappa, hipStream_t st);

// mg_engine.hip: what the solve loop (mg_solve.hip) and the stateless ABI (mg_dev.hip) use of the handle and cycle driver.
// hipMemset on device memory is asynchronous to the host and runs on the NULL stream, which a
// hipStreamNonBlocking stream does not wait for: alloc_zero zeroes on the stream that will use the memory.
int alloc_zero(std::string* err, void** p, size_t bytes, hipStream_t st = nullptr);
// host array (nx, ny) of hdt <-> device field of ddt with pitch ld, on st; another dtype goes through `staging` (a device
// field of the host dtype's pitch) and is cast on the device.  Both wait for st: the caller's array may go away
int upload(std::string* err, void* dev, int ddt, int ld, const void* host, int hdt, int nx, int ny, void* staging,
           hipStream_t st);
int download(std::string* err, void* host, int hdt, const void* dev, int ddt, int ld, int nx, int ny, void* staging,
             hipStream_t st);
int set_rhs_impl(mg_handle* h, const void* rhs, int hdt);
int set_u_impl(mg_handle* h, const void* u0, int hdt);
// the device form of set_u_impl(u0 != NULL): `u_dev` is an (nx, ny) device array of `dtype` with pitch `ld` (elements);
// asynchronous on the handle's stream.  For the units of the library that own an engine (mg_heat.hip)
int set_u_device_impl(mg_handle* h, const void* u_dev, int ld, int dtype);
// after mg_set_rhs_device: the ring of that right-hand side (and of every later mg_update_rhs_device) is zero, so its sum is 0
void rhs_ring_is_zero(mg_handle* h);
// hand an engine another unit owns the fp64 device right-hand side f (pitch ld): mg_set_rhs_device the first time (then,
// with ring_is_zero, rhs_ring_is_zero), mg_update_rhs_device afterwards; *has_rhs is the owner's flag.  Returns the
// engine's code (its message is mg_last_error(eng))
int engine_set_rhs(mg_handle* eng, bool* has_rhs, const double* f, int ld, bool ring_is_zero);
// z = M r: num_cycles cycles from the zero iterate on the engine (the ring of r is zero: mg_update_rhs_device's contract)
int engine_precondition(mg_handle* eng, bool* has_rhs, const double* r, double* z, int ld, int num_cycles);
// mg_pcg.hip: the preconditioner engine an mg_pcg owns (its stream carries all of the solver's work), for the unit of the
// library that owns an mg_pcg (mg_heat.hip) and queues its own kernels in between
mg_handle* pcg_engine(mg_pcg* s);
// mg_nl.hip: the same engine through the mg_nl that owns the mg_pcg, for the unit of the library that owns an mg_nl
// (mg_rd.hip): its stream carries the Newton method's work and the stepper's kernels in between
mg_handle* nl_engine(mg_nl* s);
void inject_rings(mg_handle* h, int ph, bool only_shared = false);
void inject_rings_once(mg_handle* h, int p);
// `part` (level 0 only) splits the fused cycle for speculative launching: the FRONT part (down leg + the whole
// sub-cycle below) never writes the buffer that holds the current fine iterate, only the BACK part (up leg) does.
constexpr int kPartFull = 0, kPartFront = 1, kPartBack = 2;
int cycle_fused(mg_handle* h, int l, bool zero_u, int part = kPartFull);
bool span_ok(const mg_handle* h);
int cycle_span(mg_handle* h, bool keep_mid);
int cycle_below_fine(mg_handle* h);
int fmg_init(mg_handle* h, int ncyc);
int defect_fmg(mg_handle* h, int ncyc);
int defect_cycle(mg_handle* h);
int run_cycle(mg_handle* h);
}  // namespace mgh
