// The stateless entry points of the C ABI (include/mghip.h): mg_dev_* on device arrays, mg_op_* on host arrays.  Argument
// checks here, launches through mg_launch.hpp: host code, no kernel is named.
#include "mg_launch.hpp"

using namespace mgh;

static bool ld_ok(int dt, int ny, int ld) { return ld >= ny && ((size_t)ld * esize(dt)) % 16 == 0; }

// what the fused-leg entry points share; register-blocked legs on blocks above ~1100^2 cells (same results, mg_config.fused = 2)
static LegGeom dev_leg_geom(int nx, int ny, int ld, int nxc, int nyc, int ldc, int ci_off, int cj_off, double hx, double hy,
                            double omega, double coeff, int nsweep, int colour_offset) {
  LegGeom g;
  g.nx = nx; g.ny = ny; g.ld = ld; g.nxc = nxc; g.nyc = nyc; g.ldc = ldc; g.ci_off = ci_off; g.cj_off = cj_off;
  g.hx = hx; g.hy = hy; g.omega = omega; g.coeff = coeff; g.nsweep = nsweep; g.poff = colour_offset;
  g.rb = 1;
  return g;
}

// device buffers of one host-pointer call (mg_op_*), freed on scope exit
struct Scratch {
  std::vector<void*> ptrs;
  hipStream_t st = nullptr;
  ~Scratch() { for (void* p : ptrs) (void)hipFree(p); }
  int get(void** p, int dt, int nx, int ny) {
    const size_t bytes = (size_t)nx * pitch_elems(dt, ny) * esize(dt);
    const int rc = alloc_zero(nullptr, p, bytes);
    if (rc == MG_OK) ptrs.push_back(*p);
    return rc;
  }
};
static int need_device() {
  int n = 0;
  const int rc = mg_device_count(&n);
  if (rc != MG_OK) return rc;
  if (n <= 0) return fail(nullptr, MG_ERR_NO_DEVICE, "no HIP device visible");
  return MG_OK;
}
static int up(void* dev, int dt, const void* host, int nx, int ny) {
  const int ld = pitch_elems(dt, ny);
  HIPC(nullptr, hipMemcpy2D(dev, (size_t)ld * esize(dt), host, (size_t)ny * esize(dt), (size_t)ny * esize(dt), nx, hipMemcpyHostToDevice));
  return MG_OK;
}
static int down(void* host, int dt, const void* dev, int nx, int ny) {
  const int ld = pitch_elems(dt, ny);
  HIPC(nullptr, hipDeviceSynchronize());
  HIPC(nullptr, hipMemcpy2D(host, (size_t)ny * esize(dt), dev, (size_t)ld * esize(dt), (size_t)ny * esize(dt), nx, hipMemcpyDeviceToHost));
  return MG_OK;
}
#define RC(x) do { const int rc_ = (x); if (rc_ != MG_OK) return rc_; } while (0)

extern "C" {

// ---------------------------------------------------------------- stateless, device arrays ----

int mg_dev_jacobi(int dtype, int nx, int ny, int ld, double hx, double hy, double omega, const void* u, const void* rhs,
                  void* out, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && nx >= 3 && ny >= 3 && ld_ok(dtype, ny, ld), "mg_dev_jacobi: bad shape / pitch");
  CHECK_ARG(u && rhs && out && u != out && aligned16(u) && aligned16(rhs) && aligned16(out), "mg_dev_jacobi: bad pointer");
  d_jacobi(dtype, u, rhs, out, nx, ny, ld, hx, hy, omega, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_rbgs_colour(int dtype, int nx, int ny, int ld, double hx, double hy, double omega, int colour, int colour_offset,
                       void* u, const void* rhs, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && nx >= 3 && ny >= 3 && ld_ok(dtype, ny, ld) && (colour == 0 || colour == 1), "mg_dev_rbgs_colour: bad argument");
  CHECK_ARG(u && rhs && aligned16(u) && aligned16(rhs), "mg_dev_rbgs_colour: bad pointer");
  d_rbgs_colour(dtype, u, rhs, nx, ny, ld, hx, hy, omega, colour, colour_offset, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_residual(int dtype, int nx, int ny, int ld, double hx, double hy, double coeff, const void* u, const void* f,
                    void* r, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && nx >= 3 && ny >= 3 && ld_ok(dtype, ny, ld), "mg_dev_residual: bad shape / pitch");
  CHECK_ARG(u && f && r && aligned16(u) && aligned16(f) && aligned16(r), "mg_dev_residual: bad pointer");
  d_residual(dtype, u, f, r, nx, ny, ld, hx, hy, coeff, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_residual_f32in_f64out(int nx, int ny, int ld_in, int ld_out, double hx, double hy, double coeff, const float* u,
                                 const float* f, double* r, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_in >= ny && ld_out >= ny, "mg_dev_residual_f32in_f64out: bad shape / pitch");
  CHECK_ARG(u && f && r, "mg_dev_residual_f32in_f64out: bad pointer");
  d_residual_f32in_f64out(u, f, r, nx, ny, ld_in, ld_out, hx, hy, coeff, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_scratch_bytes(int nx, int ny, int64_t* bytes) {
  CHECK_ARG(bytes && nx >= 1 && ny >= 1, "mg_dev_scratch_bytes: bad argument");
  *bytes = (int64_t)sizeof(double) * (int64_t)max_partials(nx, ny);
  return MG_OK;
}

int mg_dev_sumsq(int dtype, int ld, int i_lo, int i_hi, int j_lo, int j_hi, const void* field, void* scratch,
                 double* sumsq_dev, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && i_lo >= 0 && i_hi >= i_lo && j_lo >= 0 && j_hi >= j_lo && ld_ok(dtype, j_hi, ld), "mg_dev_sumsq: bad window / pitch");
  CHECK_ARG(field && scratch && sumsq_dev && aligned16(field), "mg_dev_sumsq: bad pointer");
  const int n = d_sumsq(dtype, field, (double*)scratch, ld, i_lo, i_hi, j_lo, j_hi, (hipStream_t)stream);
  launch_reduce((double*)scratch, n, sumsq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_restrict_fw(int in_dtype, int out_dtype, int nxf, int nyf, int ldf, int nxc, int nyc, int ldc, int sides,
                       const void* fine, void* coarse, void* stream) {
  CHECK_ARG(valid_dtype(in_dtype) && valid_dtype(out_dtype) && nxf >= 3 && nyf >= 3 && nxc >= 2 && nyc >= 2 && sides >= 0 && sides <= 15, "mg_dev_restrict_fw: bad argument");
  // interior coarse cells read fine rows/cols 2c-1..2c+1; a physical far edge is injected from fine 2(nc-1)
  CHECK_ARG(2 * (nxc - 2) + 1 <= nxf - 1 && 2 * (nyc - 2) + 1 <= nyf - 1, "Cannot restrict: coarse grid too large for the fine grid");
  CHECK_ARG((!(sides & 2) || 2 * (nxc - 1) <= nxf - 1) && (!(sides & 8) || 2 * (nyc - 1) <= nyf - 1), "Cannot restrict: coarse boundary outside the fine grid");
  CHECK_ARG(ld_ok(in_dtype, nyf, ldf) && ld_ok(out_dtype, nyc, ldc) && fine && coarse && aligned16(coarse), "mg_dev_restrict_fw: bad pitch / pointer");
  d_restrict_sub(in_dtype, out_dtype, fine, coarse, ldf, nxc, nyc, ldc, sides, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_prolong_add(int coarse_dtype, int fine_dtype, int compute_dtype, int nxf, int nyf, int ldf, int nxc, int nyc,
                       int ldc, int sides, const void* coarse, void* fine_u, void* stream) {
  CHECK_ARG(valid_dtype(coarse_dtype) && valid_dtype(fine_dtype) && valid_dtype(compute_dtype) && nxf >= 3 && nyf >= 3 && nxc >= 2 && nyc >= 2 && sides >= 0 && sides <= 15, "mg_dev_prolong_add: bad argument");
  CHECK_ARG(ld_ok(fine_dtype, nyf, ldf) && ldc >= nyc && coarse && fine_u && aligned16(fine_u), "mg_dev_prolong_add: bad pitch / pointer");
  const int rc = d_prolong_sub(true, coarse_dtype, fine_dtype, compute_dtype, coarse, fine_u, nxf, nyf, ldf, nxc, nyc, ldc, sides, (hipStream_t)stream);
  if (rc != MG_OK) return fail(nullptr, rc, "mg_dev_prolong_add: fp32 interpolation needs fp32 coarse and fine fields");
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

// ---- fused legs on device arrays (sub-domains: wide ghost zones, coarse offsets, norm window) --------------------
int mg_dev_down_leg(int smoother, int dtype, int coarse_dtype, int nx, int ny, int ld, int nxc, int nyc, int ldc, int ci_off,
                    int cj_off, double hx, double hy, double omega, double coeff, int nsweep, int zero_init, int colour_offset,
                    const void* u, const void* rhs, void* out, void* rhs_coarse, void* stream, int select, const int* inner_rect) {
  return mg_dev_down_leg_var(smoother, dtype, coarse_dtype, nx, ny, ld, nxc, nyc, ldc, ci_off, cj_off, hx, hy, omega, coeff, nsweep,
                             zero_init, colour_offset, u, rhs, out, rhs_coarse, stream, select, inner_rect, nullptr, nullptr);
}

int mg_dev_down_leg_var(int smoother, int dtype, int coarse_dtype, int nx, int ny, int ld, int nxc, int nyc, int ldc, int ci_off,
                        int cj_off, double hx, double hy, double omega, double coeff, int nsweep, int zero_init, int colour_offset,
                        const void* u, const void* rhs, void* out, void* rhs_coarse, void* stream, int select, const int* inner_rect,
                        const void* acoef, const void* rdiag) {
  CHECK_ARG((smoother == MG_JACOBI || smoother == MG_RBGS) && valid_dtype(dtype) && valid_dtype(coarse_dtype), "mg_dev_down_leg: bad smoother / dtype");
  CHECK_ARG((!acoef && !rdiag) || (acoef && rdiag && aligned16(acoef) && aligned16(rdiag)), "mg_dev_down_leg: coefficient and reciprocal diagonal come together, 16-byte aligned");
  CHECK_ARG(nx >= 3 && ny >= 3 && nxc >= 3 && nyc >= 3 && ld_ok(dtype, ny, ld) && ldc >= nyc && nsweep >= 0 && nsweep <= 2, "mg_dev_down_leg: bad shape / pitch / sweep count");
  CHECK_ARG(rhs && out && rhs_coarse && (zero_init || u) && u != out && aligned16(rhs) && aligned16(out) && (!u || aligned16(u)), "mg_dev_down_leg: bad pointer");
  LegGeom g = dev_leg_geom(nx, ny, ld, nxc, nyc, ldc, ci_off, cj_off, hx, hy, omega, coeff, nsweep, colour_offset);
  CHECK_ARG(select >= 0 && select <= 2 && (select == 0 || inner_rect), "mg_dev_down_leg: bad tile selection");
  if (select) { g.select = select; g.in_i_lo = inner_rect[0]; g.in_i_hi = inner_rect[1]; g.in_j_lo = inner_rect[2]; g.in_j_hi = inner_rect[3]; }
  g.acoef = acoef; g.rdiag = rdiag;
  d_down(smoother, dtype, coarse_dtype, u ? u : rhs, rhs, out, rhs_coarse, g, zero_init != 0, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_up_leg(int smoother, int dtype, int coarse_dtype, int compute_dtype, int nx, int ny, int ld, int nxc, int nyc, int ldc,
                  int ci_off, int cj_off, int sides, double hx, double hy, double omega, double coeff, int nsweep, int colour_offset,
                  const void* u, const void* rhs, void* out, const void* e_coarse, int norm, int ni_lo, int ni_hi, int nj_lo,
                  int nj_hi, void* scratch, double* sumsq_dev, void* stream) {
  return mg_dev_up_leg_var(smoother, dtype, coarse_dtype, compute_dtype, nx, ny, ld, nxc, nyc, ldc, ci_off, cj_off, sides, hx, hy, omega,
                           coeff, nsweep, colour_offset, u, rhs, out, e_coarse, norm, ni_lo, ni_hi, nj_lo, nj_hi, scratch, sumsq_dev,
                           stream, nullptr, nullptr);
}

int mg_dev_up_leg_var(int smoother, int dtype, int coarse_dtype, int compute_dtype, int nx, int ny, int ld, int nxc, int nyc, int ldc,
                      int ci_off, int cj_off, int sides, double hx, double hy, double omega, double coeff, int nsweep, int colour_offset,
                      const void* u, const void* rhs, void* out, const void* e_coarse, int norm, int ni_lo, int ni_hi, int nj_lo,
                      int nj_hi, void* scratch, double* sumsq_dev, void* stream, const void* acoef, const void* rdiag) {
  CHECK_ARG((smoother == MG_JACOBI || smoother == MG_RBGS) && valid_dtype(dtype) && valid_dtype(coarse_dtype) && valid_dtype(compute_dtype), "mg_dev_up_leg: bad smoother / dtype");
  CHECK_ARG((!acoef && !rdiag) || (acoef && rdiag && aligned16(acoef) && aligned16(rdiag)), "mg_dev_up_leg: coefficient and reciprocal diagonal come together, 16-byte aligned");
  CHECK_ARG(nx >= 3 && ny >= 3 && nxc >= 2 && nyc >= 2 && ld_ok(dtype, ny, ld) && ldc >= nyc && nsweep >= 0 && nsweep <= 2 && sides >= 0 && sides <= 15, "mg_dev_up_leg: bad shape / pitch / sweep count");
  CHECK_ARG(u && rhs && out && e_coarse && u != out && aligned16(u) && aligned16(rhs) && aligned16(out) && (!norm || (scratch && sumsq_dev)), "mg_dev_up_leg: bad pointer");
  LegGeom g = dev_leg_geom(nx, ny, ld, nxc, nyc, ldc, ci_off, cj_off, hx, hy, omega, coeff, nsweep, colour_offset);
  g.sides = sides;
  if (norm) { g.ni_lo = ni_lo; g.ni_hi = ni_hi; g.nj_lo = nj_lo; g.nj_hi = nj_hi; }
  g.acoef = acoef; g.rdiag = rdiag;
  const int n = d_up(smoother, dtype, coarse_dtype, compute_dtype, u, rhs, out, e_coarse, (double*)scratch, g, norm != 0, (hipStream_t)stream);
  if (n < 0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_dev_up_leg: fp32 interpolation needs fp32 coarse and fine fields");
  if (norm) launch_reduce((double*)scratch, n, sumsq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_span_leg_ok(int smoother, int dtype, int coarse_dtype, int compute_dtype, int nx, int ny) {
  if (smoother != MG_JACOBI || !valid_dtype(dtype) || coarse_dtype != dtype || !valid_dtype(compute_dtype)) return 0;
  if (dtype == MG_F64 && compute_dtype != MG_F64) return 0;
  LegGeom g;
  g.nx = nx; g.ny = ny; g.rb = 1;
  return use_rb(g) ? 1 : 0;
}

int mg_dev_span_leg(int smoother, int dtype, int coarse_dtype, int compute_dtype, int nx, int ny, int ld, int nxc, int nyc, int ldc,
                    int ci_off, int cj_off, int sides, double hx, double hy, double omega, double coeff, int nsweep_post,
                    int nsweep_pre, int colour_offset, const void* u, const void* rhs, void* out_mid, void* out_next,
                    const void* e_coarse, void* rhs_coarse, int ni_lo, int ni_hi, int nj_lo, int nj_hi, void* scratch,
                    double* sumsq_dev, void* stream) {
  CHECK_ARG(mg_dev_span_leg_ok(smoother, dtype, coarse_dtype, compute_dtype, nx, ny), "mg_dev_span_leg: weighted Jacobi on one dtype and arrays above ~1100^2 cells only");
  CHECK_ARG(nx >= 3 && ny >= 3 && nxc >= 2 && nyc >= 2 && ld_ok(dtype, ny, ld) && ldc >= nyc && nsweep_post >= 1 && nsweep_post <= 2 &&
            nsweep_pre >= 1 && nsweep_pre <= 2 && sides >= 0 && sides <= 15, "mg_dev_span_leg: bad shape / pitch / sweep count");
  CHECK_ARG(u && rhs && out_next && e_coarse && rhs_coarse && scratch && sumsq_dev && u != out_next && u != out_mid && out_mid != out_next &&
            aligned16(u) && aligned16(rhs) && aligned16(out_next) && (!out_mid || aligned16(out_mid)), "mg_dev_span_leg: bad pointer");
  LegGeom g = dev_leg_geom(nx, ny, ld, nxc, nyc, ldc, ci_off, cj_off, hx, hy, omega, coeff, nsweep_post, colour_offset);
  g.sides = sides;
  g.ni_lo = ni_lo; g.ni_hi = ni_hi; g.nj_lo = nj_lo; g.nj_hi = nj_hi;
  const int n = d_span(dtype, compute_dtype, u, rhs, out_mid, out_next, e_coarse, rhs_coarse, (double*)scratch, g, nsweep_pre, (hipStream_t)stream);
  if (n < 0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_dev_span_leg: unsupported precision combination");
  launch_reduce((double*)scratch, n, sumsq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_var_rdiag(int dtype, int nx, int ny, int ld, double hx, double hy, double sigma, const void* a, void* rdiag, void* stream) {
  CHECK_ARG(valid_dtype(dtype) && nx >= 3 && ny >= 3 && ld_ok(dtype, ny, ld) && sigma >= 0.0, "mg_dev_var_rdiag: bad shape / pitch / shift");
  CHECK_ARG(a && rdiag && a != rdiag, "mg_dev_var_rdiag: bad pointer");
  d_rdiag(dtype, a, rdiag, nx, ny, ld, hx, hy, sigma, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_inject_ring(int in_dtype, int out_dtype, int nxf, int nyf, int ldf, int nxc, int nyc, int ldc, int sides, int ci_off,
                       int cj_off, const void* fine, void* coarse, void* stream) {
  CHECK_ARG(valid_dtype(in_dtype) && valid_dtype(out_dtype) && nxf >= 3 && nyf >= 3 && nxc >= 2 && nyc >= 2 && ldf >= nyf && ldc >= nyc && fine && coarse && sides >= 0 && sides <= 15, "mg_dev_inject_ring: bad argument");
  d_inject_ring(in_dtype, out_dtype, fine, coarse, nxf, nyf, ldf, nxc, nyc, ldc, (hipStream_t)stream, sides, ci_off, cj_off);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_convert(int in_dtype, int out_dtype, int nx, int ny, int ldi, int ldo, const void* in, void* out, void* stream) {
  CHECK_ARG(valid_dtype(in_dtype) && valid_dtype(out_dtype) && nx >= 1 && ny >= 1 && ldi >= ny && ldo >= ny && in && out, "mg_dev_convert: bad argument");
  d_convert(in_dtype, out_dtype, in, out, nx, ny, ldi, ldo, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

// ---------------------------------------------------------------- stateless, host arrays ------

int mg_op_residual(int dtype, int nx, int ny, double hx, double hy, double coeff, const void* u, const void* f, void* r) {
  CHECK_ARG(valid_dtype(dtype) && u && f && r, "mg_op_residual: bad argument");
  CHECK_ARG(nx >= 3 && ny >= 3, "Cannot apply Laplacian to grid");   // operators/laplacian.py:55-56
  RC(need_device());
  Scratch s; void *du, *df, *dr;
  RC(s.get(&du, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny)); RC(s.get(&dr, dtype, nx, ny));
  RC(up(du, dtype, u, nx, ny)); RC(up(df, dtype, f, nx, ny));
  d_residual(dtype, du, df, dr, nx, ny, pitch_elems(dtype, ny), hx, hy, coeff, nullptr);
  return down(r, dtype, dr, nx, ny);
}

int mg_op_residual_mixed(int nx, int ny, double hx, double hy, double coeff, const float* u, const float* f, double* r) {
  CHECK_ARG(u && f && r, "mg_op_residual_mixed: bad argument");
  CHECK_ARG(nx >= 3 && ny >= 3, "Cannot apply Laplacian to grid");   // operators/laplacian.py:55-56
  RC(need_device());
  Scratch s; void *du, *df, *dr;
  RC(s.get(&du, MG_F32, nx, ny)); RC(s.get(&df, MG_F32, nx, ny)); RC(s.get(&dr, MG_F64, nx, ny));
  RC(up(du, MG_F32, u, nx, ny)); RC(up(df, MG_F32, f, nx, ny));
  RC(mg_dev_residual_f32in_f64out(nx, ny, pitch_elems(MG_F32, ny), pitch_elems(MG_F64, ny), hx, hy, coeff, (const float*)du, (const float*)df,
                                  (double*)dr, nullptr));
  return down(r, MG_F64, dr, nx, ny);
}

int mg_op_apply(int dtype, int nx, int ny, double hx, double hy, double coeff, const void* u, void* au) {
  CHECK_ARG(valid_dtype(dtype) && u && au, "mg_op_apply: bad argument");
  CHECK_ARG(nx >= 3 && ny >= 3, "Cannot apply Laplacian to grid");
  RC(need_device());
  // A u = 0 - (0 - A u): residual of a zero right-hand side under the negated coefficient (exact sign flips)
  Scratch s; void *du, *df, *dr;
  RC(s.get(&du, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny)); RC(s.get(&dr, dtype, nx, ny));
  RC(up(du, dtype, u, nx, ny));
  d_residual(dtype, du, df, dr, nx, ny, pitch_elems(dtype, ny), hx, hy, -coeff, nullptr);
  return down(au, dtype, dr, nx, ny);
}

int mg_op_norm(int dtype, int nx, int ny, double hx, double hy, const void* field, double* out) {
  CHECK_ARG(valid_dtype(dtype) && field && out && nx >= 1 && ny >= 1, "mg_op_norm: bad argument");
  RC(need_device());
  Scratch s; void* dfld; void* part; void* acc;
  RC(s.get(&dfld, dtype, nx, ny));
  RC(alloc_zero(nullptr, &part, sizeof(double) * 2048)); s.ptrs.push_back(part);
  RC(alloc_zero(nullptr, &acc, sizeof(double))); s.ptrs.push_back(acc);
  RC(up(dfld, dtype, field, nx, ny));
  const int n = d_sumsq(dtype, dfld, (double*)part, pitch_elems(dtype, ny), 0, nx, 0, ny, nullptr);
  launch_reduce((double*)part, n, (double*)acc, nullptr);
  double ss = 0;
  HIPC(nullptr, hipMemcpy(&ss, acc, sizeof(double), hipMemcpyDeviceToHost));
  *out = std::sqrt(hx * hy * ss);
  return MG_OK;
}

int mg_op_jacobi(int dtype, int nx, int ny, double hx, double hy, double omega, int nu, const void* u, const void* rhs, void* out) {
  CHECK_ARG(valid_dtype(dtype) && u && rhs && out && nu >= 0 && nx >= 3 && ny >= 3, "mg_op_jacobi: bad argument");
  RC(need_device());
  Scratch s; void *da, *db, *df;
  RC(s.get(&da, dtype, nx, ny)); RC(s.get(&db, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny));
  RC(up(da, dtype, u, nx, ny)); RC(up(db, dtype, u, nx, ny)); RC(up(df, dtype, rhs, nx, ny));
  for (int k = 0; k < nu; ++k) { d_jacobi(dtype, da, df, db, nx, ny, pitch_elems(dtype, ny), hx, hy, omega, nullptr); std::swap(da, db); }
  return down(out, dtype, da, nx, ny);
}

int mg_op_rbgs(int dtype, int nx, int ny, double hx, double hy, double omega, int nu, const void* u, const void* rhs, void* out) {
  CHECK_ARG(valid_dtype(dtype) && u && rhs && out && nu >= 0 && nx >= 3 && ny >= 3, "mg_op_rbgs: bad argument");
  RC(need_device());
  Scratch s; void *da, *df;
  RC(s.get(&da, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny));
  RC(up(da, dtype, u, nx, ny)); RC(up(df, dtype, rhs, nx, ny));
  for (int k = 0; k < nu; ++k)
    for (int c = 0; c < 2; ++c) d_rbgs_colour(dtype, da, df, nx, ny, pitch_elems(dtype, ny), hx, hy, omega, c, 0, nullptr);
  return down(out, dtype, da, nx, ny);
}


int mg_op_helmholtz(int dtype, int op, int nx, int ny, double hx, double hy, double coeff, double sigma, double omega, int nu,
                    const void* u, const void* f, void* out) {
  CHECK_ARG(valid_dtype(dtype) && u && f && out && nu >= 0 && nx >= 3 && ny >= 3 && op >= 0 && op <= 2 && sigma >= 0.0,
            "mg_op_helmholtz: bad argument");
  RC(need_device());
  const int ld = pitch_elems(dtype, ny);
  Scratch s; void *da, *db, *df;
  RC(s.get(&da, dtype, nx, ny)); RC(s.get(&db, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny));
  RC(up(da, dtype, u, nx, ny)); RC(up(db, dtype, u, nx, ny)); RC(up(df, dtype, f, nx, ny));
  if (op == 0) {
    d_residual(dtype, da, df, db, nx, ny, ld, hx, hy, coeff, nullptr, false, sigma);
    return down(out, dtype, db, nx, ny);
  }
  for (int k = 0; k < nu; ++k) {
    if (op == 1) { d_jacobi(dtype, da, df, db, nx, ny, ld, hx, hy, omega, nullptr, false, sigma); std::swap(da, db); }
    else for (int c = 0; c < 2; ++c) d_rbgs_colour(dtype, da, df, nx, ny, ld, hx, hy, omega, c, 0, nullptr, false, sigma);
  }
  return down(out, dtype, da, nx, ny);
}

int mg_op_residual_var(int dtype, int nx, int ny, double hx, double hy, double coeff, const void* a, const void* u, const void* f, void* r) {
  CHECK_ARG(valid_dtype(dtype) && a && u && f && r && nx >= 3 && ny >= 3, "mg_op_residual_var: bad argument");
  RC(need_device());
  Scratch s; void *da, *du, *df, *dr;
  RC(s.get(&da, dtype, nx, ny)); RC(s.get(&du, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny)); RC(s.get(&dr, dtype, nx, ny));
  RC(up(da, dtype, a, nx, ny)); RC(up(du, dtype, u, nx, ny)); RC(up(df, dtype, f, nx, ny));
  d_var(mg::kVarResidual, dtype, du, da, df, dr, nx, ny, pitch_elems(dtype, ny), hx, hy, 1.0, coeff, 0, 0, nullptr);
  return down(r, dtype, dr, nx, ny);
}

int mg_op_jacobi_var(int dtype, int nx, int ny, double hx, double hy, double omega, int nu, const void* a, const void* u, const void* rhs, void* out) {
  CHECK_ARG(valid_dtype(dtype) && a && u && rhs && out && nu >= 0 && nx >= 3 && ny >= 3, "mg_op_jacobi_var: bad argument");
  RC(need_device());
  Scratch s; void *dc, *da, *db, *df;
  RC(s.get(&dc, dtype, nx, ny)); RC(s.get(&da, dtype, nx, ny)); RC(s.get(&db, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny));
  RC(up(dc, dtype, a, nx, ny)); RC(up(da, dtype, u, nx, ny)); RC(up(db, dtype, u, nx, ny)); RC(up(df, dtype, rhs, nx, ny));
  for (int k = 0; k < nu; ++k) {
    d_var(mg::kVarJacobi, dtype, da, dc, df, db, nx, ny, pitch_elems(dtype, ny), hx, hy, omega, -1.0, 0, 0, nullptr);
    std::swap(da, db);
  }
  return down(out, dtype, da, nx, ny);
}

int mg_op_rbgs_var(int dtype, int nx, int ny, double hx, double hy, double omega, int nu, const void* a, const void* u, const void* rhs, void* out) {
  CHECK_ARG(valid_dtype(dtype) && a && u && rhs && out && nu >= 0 && nx >= 3 && ny >= 3, "mg_op_rbgs_var: bad argument");
  RC(need_device());
  Scratch s; void *dc, *da, *df;
  RC(s.get(&dc, dtype, nx, ny)); RC(s.get(&da, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny));
  RC(up(dc, dtype, a, nx, ny)); RC(up(da, dtype, u, nx, ny)); RC(up(df, dtype, rhs, nx, ny));
  for (int k = 0; k < nu; ++k)
    for (int c = 0; c < 2; ++c)
      d_var(mg::kVarRbgs, dtype, da, dc, df, da, nx, ny, pitch_elems(dtype, ny), hx, hy, omega, -1.0, c, 0, nullptr);
  return down(out, dtype, da, nx, ny);
}

int mg_op_restrict_fw(int in_dtype, int out_dtype, int nx, int ny, const void* fine, void* coarse) {
  CHECK_ARG(valid_dtype(in_dtype) && valid_dtype(out_dtype) && fine && coarse, "mg_op_restrict_fw: bad argument");
  CHECK_ARG(nx >= 3 && ny >= 3 && (nx - 1) % 2 == 0 && (ny - 1) % 2 == 0, "Cannot restrict: fine grid is not coarsenable");   // transfer.py:65-66
  RC(need_device());
  const int cx = (nx - 1) / 2 + 1, cy = (ny - 1) / 2 + 1;
  Scratch s; void *dfine, *dc;
  RC(s.get(&dfine, in_dtype, nx, ny)); RC(s.get(&dc, out_dtype, cx, cy));
  RC(up(dfine, in_dtype, fine, nx, ny));
  d_restrict(in_dtype, out_dtype, dfine, dc, nx, ny, pitch_elems(in_dtype, ny), pitch_elems(out_dtype, cy), nullptr);
  return down(coarse, out_dtype, dc, cx, cy);
}

int mg_op_prolong_bilinear(int in_dtype, int out_dtype, int ncx, int ncy, const void* coarse, void* fine) {
  CHECK_ARG(valid_dtype(in_dtype) && valid_dtype(out_dtype) && coarse && fine && ncx >= 2 && ncy >= 2, "mg_op_prolong_bilinear: bad argument");
  RC(need_device());
  const int nx = 2 * (ncx - 1) + 1, ny = 2 * (ncy - 1) + 1;
  Scratch s; void *dc, *dfine;
  RC(s.get(&dc, in_dtype, ncx, ncy)); RC(s.get(&dfine, out_dtype, nx, ny));
  RC(up(dc, in_dtype, coarse, ncx, ncy));
  // the interpolation runs in the FINE array's dtype (operators/transfer.py:207,236)
  const int rc = d_prolong(false, in_dtype, out_dtype, (in_dtype == MG_F32 && out_dtype == MG_F32) ? MG_F32 : MG_F64, dc, dfine,
                                  nx, ny, pitch_elems(out_dtype, ny), pitch_elems(in_dtype, ncy), nullptr);
  if (rc != MG_OK) return fail(nullptr, rc, "mg_op_prolong_bilinear: unsupported dtype combination");
  return down(fine, out_dtype, dfine, nx, ny);
}

int mg_op_coarse_solve(int dtype, int nx, int ny, double hx, double hy, double coeff, double tol, int maxit, const void* u0,
                       const void* rhs, void* out, int* sweeps) {
  CHECK_ARG(valid_dtype(dtype) && u0 && rhs && out && nx >= 3 && ny >= 3 && maxit >= 1, "mg_op_coarse_solve: bad argument");
  RC(need_device());
  Scratch s; void *du, *df; void* dsw;
  RC(s.get(&du, dtype, nx, ny)); RC(s.get(&df, dtype, nx, ny));
  RC(alloc_zero(nullptr, &dsw, sizeof(int))); s.ptrs.push_back(dsw);
  RC(up(du, dtype, u0, nx, ny)); RC(up(df, dtype, rhs, nx, ny));
  d_coarse(dtype, du, df, nx, ny, pitch_elems(dtype, ny), hx, hy, coeff, 1.0, tol, maxit, (int*)dsw, nullptr);
  RC(down(out, dtype, du, nx, ny));
  if (sweeps) HIPC(nullptr, hipMemcpy(sweeps, dsw, sizeof(int), hipMemcpyDeviceToHost));
  return MG_OK;
}

}  // extern "C"
