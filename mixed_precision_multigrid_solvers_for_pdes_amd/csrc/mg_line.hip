// Zebra line relaxation: plans (the tables of one level, direction and dtype), the colour-pass launcher and the entry points
// of include/mghip_line.h.  The one unit that instantiates mg_line_kernels.hpp.
#include "mg_launch.hpp"
#include "mg_line_kernels.hpp"

#include "../../include/mghip_line.h"

#include <cstdint>

struct mg_line_plan {
  int dtype = MG_F64, dir = mgl::kDirY, nx = 0, ny = 0, ld = 0;
  double hx = 0, hy = 0, sigma = 0;
  int n = 0, K = 0, mt = 0, G = 0, LS = 0;   // cells per line, periods, last chunk, lines per workgroup, LDS cells per line
  size_t lds = 0;                            // dynamic LDS bytes per workgroup
  double w = 0, c = 0, D = 0, e = 0;
  void* tab = nullptr;                       // device: the table block in `dtype`
};

namespace mgh {
namespace {

constexpr int kMaxLine = 16384;                       // cells per line a workgroup can keep in LDS (144 KiB, fp64)
constexpr size_t kLdsSoft = 64 * 1024, kLdsHard = 144 * 1024;

// tridiag(-w, D, -w) x = w e_0 of length len: the left spike of a chunk
void spike(long double w, long double D, int len, long double* out) {
  long double d[mgl::kPeriod], y[mgl::kPeriod];
  d[0] = D; y[0] = w / d[0];
  for (int t = 1; t < len; ++t) { d[t] = D - w * w / d[t - 1]; y[t] = w * y[t - 1] / d[t]; }
  out[len - 1] = y[len - 1];
  for (int t = len - 2; t >= 0; --t) out[t] = y[t] + (w / d[t]) * out[t + 1];
}

// round to the plan's dtype (what the kernel reads) and back: the separator system is built from the rounded spikes
long double rounded(long double v, int dt) { return dt == MG_F32 ? (long double)(float)v : (long double)(double)v; }

int build_tables(mg_line_plan* p, std::string* err) {
  const double hp = p->dir == mgl::kDirX ? p->hx : p->hy, hq = p->dir == mgl::kDirX ? p->hy : p->hx;
  p->w = 1.0 / (hp * hp); p->c = 1.0 / (hq * hq);          // w, c, D in double, as the point smoothers form theirs (coefs)
  p->D = 2.0 * p->w + 2.0 * p->c + p->sigma;
  const long double w = p->w;
  const long double D = p->D;
  const int K = p->K, KS = std::max(K - 1, 1), ntab = mgl::kTabS + 2 * KS;
  std::vector<long double> t(ntab, 0.0L);
  long double piv = D;
  for (int i = 0; i < mgl::kPeriod; ++i) {
    if (i > 0) piv = D - w * w / piv;
    t[mgl::kTabG + i] = 1.0L / piv;
    t[mgl::kTabM + i] = w / piv;
  }
  spike(w, D, mgl::kChunk, &t[mgl::kTabVL]);
  spike(w, D, p->mt, &t[mgl::kTabVT]);
  const long double v0 = rounded(t[mgl::kTabVL], p->dtype), vM = rounded(t[mgl::kTabVL + mgl::kChunk - 1], p->dtype),
                    v0t = rounded(t[mgl::kTabVT], p->dtype);
  const long double e = rounded(w * vM, p->dtype);
  p->e = (double)e;
  long double sp = 0;
  for (int q = 0; q < K - 1; ++q) {
    const long double diag = D - w * v0 - w * (q == K - 2 ? v0t : v0);
    sp = q == 0 ? diag : diag - e * e / sp;
    t[mgl::kTabS + q] = 1.0L / sp;
    t[mgl::kTabS + KS + q] = e / sp;
  }
  std::vector<unsigned char> buf((size_t)ntab * esize(p->dtype));
  for (int i = 0; i < ntab; ++i) {
    if (p->dtype == MG_F32) reinterpret_cast<float*>(buf.data())[i] = (float)t[i];
    else reinterpret_cast<double*>(buf.data())[i] = (double)t[i];
  }
  if (!p->tab) HIPC(err, hipMalloc(&p->tab, buf.size()));
  HIPC(err, hipMemcpy(p->tab, buf.data(), buf.size(), hipMemcpyHostToDevice));
  return MG_OK;
}

template <typename T, int DIR>
int launch(const mg_line_plan* p, int colour, double omega, void* u, const void* rhs, hipStream_t st) {
  constexpr int N = mgl::VecOf<T>::N;
  mgl::LineArgs<T> a;
  a.u = (T*)u; a.rhs = (const T*)rhs; a.tab = (const T*)p->tab;
  a.nx = p->nx; a.ny = p->ny; a.ld = p->ld; a.n = p->n; a.K = p->K; a.mt = p->mt; a.G = p->G; a.LS = p->LS;
  a.colour = colour;
  a.w = (T)p->w; a.c = (T)p->c; a.D = (T)p->D; a.e = (T)p->e; a.omega = (T)omega;
  int blocks;
  if (DIR == mgl::kDirY) {
    const int first = colour ? 1 : 2;
    a.count = first <= p->nx - 2 ? (p->nx - 2 - first) / 2 + 1 : 0;
    blocks = (a.count + p->G - 1) / p->G;
  } else {
    a.count = (p->ny + N - 1) / N;
    const int gv = p->G / (N / 2);
    blocks = (a.count + gv - 1) / gv;
  }
  if (blocks <= 0) return MG_OK;
  hipLaunchKernelGGL((mgl::line_colour_kernel<T, DIR>), dim3(blocks), dim3(mgl::kThreads), p->lds, st, a);
  return MG_OK;
}

template <typename T, int DIR> int raise_lds(size_t bytes, std::string* err) {
  HIPC(err, hipFuncSetAttribute(reinterpret_cast<const void*>(&mgl::line_colour_kernel<T, DIR>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return MG_OK;
}

}  // namespace

int line_plan_make(int dtype, int dir, int nx, int ny, int ld, double hx, double hy, double sigma, mg_line_plan** out,
                   std::string* err) {
  mg_line_plan* p = new mg_line_plan();
  p->dtype = dtype; p->dir = dir; p->nx = nx; p->ny = ny; p->ld = ld; p->hx = hx; p->hy = hy; p->sigma = sigma;
  p->n = (dir == mgl::kDirX ? nx : ny) - 2;
  p->K = (p->n + mgl::kPeriod - 1) / mgl::kPeriod;
  p->mt = p->n - (p->K - 1) * mgl::kPeriod;
  p->LS = (p->K * mgl::kCells) | 1;                 // odd: the line buffers of a workgroup start on different banks
  const size_t per_line = (size_t)(p->LS + 2 * p->K) * esize(dtype);
  if (dir == mgl::kDirY) {
    int g = std::min(64, std::max(1, (mgl::kThreads + p->K - 1) / p->K));
    while (g > 1 && g * per_line > kLdsSoft) --g;
    p->G = g;
  } else {
    const int lv = dtype == MG_F32 ? 2 : 1;
    int gv = (int)std::min<size_t>(16, kLdsSoft / (lv * per_line));
    if (gv < 4) gv = (int)std::min<size_t>(4, kLdsHard / (lv * per_line));   // long lines: fewer, at least 64-byte row segments
    p->G = std::max(gv, 1) * lv;
  }
  p->lds = (size_t)p->G * per_line;
  int rc = build_tables(p, err);
  if (rc == MG_OK && p->lds > 48 * 1024)
    rc = dtype == MG_F32 ? (dir == mgl::kDirX ? raise_lds<float, mgl::kDirX>(p->lds, err) : raise_lds<float, mgl::kDirY>(p->lds, err))
                         : (dir == mgl::kDirX ? raise_lds<double, mgl::kDirX>(p->lds, err) : raise_lds<double, mgl::kDirY>(p->lds, err));
  if (rc != MG_OK) { line_plan_free(p); return rc; }
  *out = p;
  return MG_OK;
}

void line_plan_free(mg_line_plan* p) {
  if (!p) return;
  if (p->tab) (void)hipFree(p->tab);
  delete p;
}

// the caller has waited for every launch that reads the old tables
int line_plan_set_sigma(mg_line_plan* p, double sigma, std::string* err) {
  p->sigma = sigma;
  return build_tables(p, err);
}

void d_line_colour(const mg_line_plan* p, int colour, double omega, void* u, const void* rhs, hipStream_t st) {
  if (p->dtype == MG_F32) {
    if (p->dir == mgl::kDirX) launch<float, mgl::kDirX>(p, colour, omega, u, rhs, st);
    else launch<float, mgl::kDirY>(p, colour, omega, u, rhs, st);
  } else {
    if (p->dir == mgl::kDirX) launch<double, mgl::kDirX>(p, colour, omega, u, rhs, st);
    else launch<double, mgl::kDirY>(p, colour, omega, u, rhs, st);
  }
}

bool line_shape_ok(int nx, int ny) { return nx >= 3 && ny >= 3 && nx - 2 <= kMaxLine && ny - 2 <= kMaxLine; }

}  // namespace mgh

using namespace mgh;

extern "C" {

int mg_line_plan_create(int dtype, int direction, int nx, int ny, int ld, double hx, double hy, double sigma, mg_line_plan** out) {
  CHECK_ARG(out, "mg_line_plan_create: out is NULL");
  *out = nullptr;
  CHECK_ARG(valid_dtype(dtype) && (direction == MG_ZEBRA_X || direction == MG_ZEBRA_Y), "mg_line_plan_create: bad dtype / direction");
  CHECK_ARG(nx >= 3 && ny >= 3 && ld >= ny && ((size_t)ld * esize(dtype)) % 16 == 0, "mg_line_plan_create: bad shape / pitch");
  CHECK_ARG(hx > 0.0 && hy > 0.0 && std::isfinite(hx) && std::isfinite(hy) && sigma >= 0.0 && std::isfinite(sigma),
             "mg_line_plan_create: spacings must be positive, sigma finite and >= 0");
  CHECK_ARG((direction == MG_ZEBRA_X ? nx : ny) - 2 <= kMaxLine, "mg_line_plan_create: lines of more than 16384 cells do not fit a workgroup's LDS");
  int ndev = 0;
  const int rc = mg_device_count(&ndev);
  if (rc != MG_OK) return rc;
  if (ndev <= 0) return fail(nullptr, MG_ERR_NO_DEVICE, "no HIP device visible");
  return line_plan_make(dtype, direction == MG_ZEBRA_X ? mgl::kDirX : mgl::kDirY, nx, ny, ld, hx, hy, sigma, out, nullptr);
}

int mg_line_plan_destroy(mg_line_plan* p) {
  line_plan_free(p);
  return MG_OK;
}

int mg_dev_line_colour(mg_line_plan* p, int colour, double omega, void* u, const void* rhs, void* stream) {
  CHECK_ARG(p && (colour == 0 || colour == 1) && std::isfinite(omega), "mg_dev_line_colour: bad argument");
  CHECK_ARG(u && rhs && u != rhs && aligned16(u) && aligned16(rhs), "mg_dev_line_colour: bad pointer");
  d_line_colour(p, colour, omega, u, rhs, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_op_zebra(int dtype, int smoother, int nx, int ny, double hx, double hy, double sigma, double omega, int nu,
                const void* u, const void* rhs, void* out) {
  CHECK_ARG(valid_dtype(dtype) && smoother >= MG_ZEBRA_X && smoother <= MG_ZEBRA_ALT && u && rhs && out && nu >= 0 && nx >= 3 && ny >= 3,
             "mg_op_zebra: bad argument");
  CHECK_ARG(hx > 0.0 && hy > 0.0 && std::isfinite(hx) && std::isfinite(hy) && sigma >= 0.0 && std::isfinite(sigma) && std::isfinite(omega),
             "mg_op_zebra: spacings must be positive, sigma finite and >= 0");
  CHECK_ARG((smoother == MG_ZEBRA_Y || nx - 2 <= kMaxLine) && (smoother == MG_ZEBRA_X || ny - 2 <= kMaxLine),
             "mg_op_zebra: lines of more than 16384 cells do not fit a workgroup's LDS");
  const int ld = pitch_elems(dtype, ny);
  const size_t pitch = (size_t)ld * esize(dtype), wbytes = (size_t)ny * esize(dtype);
  mg_line_plan* plan[2] = {nullptr, nullptr};
  void *du = nullptr, *df = nullptr;
  auto done = [&](int rc) {
    for (mg_line_plan* p : plan) line_plan_free(p);
    if (du) (void)hipFree(du);
    if (df) (void)hipFree(df);
    return rc;
  };
  int ndev = 0;
  int rc = mg_device_count(&ndev);
  if (rc != MG_OK) return rc;
  if (ndev <= 0) return fail(nullptr, MG_ERR_NO_DEVICE, "no HIP device visible");
  if ((rc = alloc_zero(nullptr, &du, pitch * nx)) != MG_OK || (rc = alloc_zero(nullptr, &df, pitch * nx)) != MG_OK) return done(rc);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy2D(du, pitch, u, wbytes, wbytes, nx, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy2D(df, pitch, rhs, wbytes, wbytes, nx, hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(nullptr, MG_ERR_HIP, "mg_op_zebra: upload failed"));
  int np = 0;
  if (smoother != MG_ZEBRA_Y && (rc = line_plan_make(dtype, mgl::kDirX, nx, ny, ld, hx, hy, sigma, &plan[np++], nullptr)) != MG_OK) return done(rc);
  if (smoother != MG_ZEBRA_X && (rc = line_plan_make(dtype, mgl::kDirY, nx, ny, ld, hx, hy, sigma, &plan[np++], nullptr)) != MG_OK) return done(rc);
  for (int k = 0; k < nu; ++k)
    for (int d = 0; d < np; ++d)
      for (int colour = 0; colour < 2; ++colour) d_line_colour(plan[d], colour, omega, du, df, nullptr);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy2D(out, wbytes, du, pitch, wbytes, nx, hipMemcpyDeviceToHost) != hipSuccess)
    return done(fail(nullptr, MG_ERR_HIP, "mg_op_zebra: sweep or download failed"));
  return done(MG_OK);
}

int mg_line_time_sweep(mg_line_plan* p, int reps, double* avg_ms) {
  CHECK_ARG(p && avg_ms && reps >= 1, "mg_line_time_sweep: bad argument");
  const size_t elems = (size_t)p->nx * p->ld, bytes = elems * esize(p->dtype);
  void *du = nullptr, *df = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto done = [&](int rc) {
    if (du) (void)hipFree(du);
    if (df) (void)hipFree(df);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
  };
  // pseudo-random operands in [-1, 1): a sweep of zeros runs at another clock than one of data
  std::vector<unsigned char> host(bytes);
  uint32_t s = 12345u;
  for (size_t i = 0; i < elems; ++i) {
    s = s * 1664525u + 1013904223u;
    const double v = (double)(s >> 8) / 8388608.0 - 1.0;
    if (p->dtype == MG_F32) reinterpret_cast<float*>(host.data())[i] = (float)v;
    else reinterpret_cast<double*>(host.data())[i] = v;
  }
  if (hipMalloc(&du, bytes) != hipSuccess || hipMalloc(&df, bytes) != hipSuccess) return done(fail(nullptr, MG_ERR_ALLOC, "mg_line_time_sweep: hipMalloc failed"));
  if (hipMemcpy(du, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(df, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    return done(fail(nullptr, MG_ERR_HIP, "mg_line_time_sweep: setup failed"));
  auto sweep = [&](int n) { for (int k = 0; k < n; ++k) for (int colour = 0; colour < 2; ++colour) d_line_colour(p, colour, 1.0, du, df, nullptr); };
  sweep(2);                                            // warm-up
  float ms = 0;
  if (hipEventRecord(e0, nullptr) != hipSuccess) return done(fail(nullptr, MG_ERR_HIP, "mg_line_time_sweep: hipEventRecord failed"));
  sweep(reps);
  if (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess ||
      hipGetLastError() != hipSuccess)
    return done(fail(nullptr, MG_ERR_HIP, "mg_line_time_sweep: timing failed"));
  *avg_ms = (double)ms / reps;
  return done(MG_OK);
}

}  // extern "C"
