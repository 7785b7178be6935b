// The fourth-order compact nine-point operator of libmghip.so (include/mghip_ho.h): this unit instantiates the kernels of
// mg_ho_kernels.hpp and holds their launchers (declared in mg_host.hpp; the Krylov loop of mg_pcg.hip calls them under
// mg_pcg_set_order(4)), the stateless device forms and the host-array forms.
#include "mg_launch.hpp"
#include "mg_ho_kernels.hpp"

#include "../../include/mghip_ho.h"

#include <cstdint>

namespace mgh {
namespace {

// the stencil weights, in exactly the forms include/mghip_ho.h states (the NumPy restatement computes the same bits)
mg::HoArgs ho_args(double hx, double hy, double coeff, double sigma) {
  const double ca = 1.0 / (hx * hx), cb = 1.0 / (hy * hy);
  mg::HoArgs c;
  c.cC = (5.0 / 3.0) * (ca + cb) + sigma * (8.0 / 12.0);
  c.cE = (cb - 5.0 * ca) / 6.0 + sigma / 12.0;
  c.cN = (ca - 5.0 * cb) / 6.0 + sigma / 12.0;
  c.cK = (ca + cb) / 12.0;
  c.mcoeff = -coeff;
  return c;
}

}  // namespace

int d_ho_direction(const double* z, const double* p_in, double* p_out, double* q, const double* beta, double* partials, int nx,
                   int ny, int ld, double hx, double hy, double coeff, double sigma, hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  hipLaunchKernelGGL(mg::ho_direction_kernel, dim3(g.ntiles), dim3(mg::kBlock), 0, st, z, p_in, p_out, q, beta, partials, g,
                     ho_args(hx, hy, coeff, sigma));
  return g.ntiles;
}

int d_ho_residual(const double* x, const double* g_rhs, double* r, double* partials, int nx, int ny, int ld, double hx, double hy,
                  double coeff, double sigma, hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  auto k = r ? mg::ho_residual_kernel<true> : mg::ho_residual_kernel<false>;
  hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, x, g_rhs, r, partials, g, ho_args(hx, hy, coeff, sigma));
  return g.ntiles;
}

void d_ho_rhs(const double* f, double* out, int nx, int ny, int ld, hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  hipLaunchKernelGGL(mg::ho_rhs_kernel, dim3(g.ntiles), dim3(mg::kBlock), 0, st, f, out, g);
}

}  // namespace mgh

using namespace mgh;


extern "C" {

int mg_dev_ho_direction(int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, const double* z,
                        const double* p_in_or_null, double* p_out, double* q, const double* beta_dev_or_null, void* scratch,
                        double* pq_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld) && operator_ok(hx, hy, coeff, sigma), "mg_dev_ho_direction: bad shape / pitch / spacing / shift");
  CHECK_ARG(z && p_out && q && scratch && pq_dev && (!beta_dev_or_null || p_in_or_null), "mg_dev_ho_direction: NULL pointer");
  CHECK_ARG(p_out != p_in_or_null && p_out != z && q != z && q != p_out && q != p_in_or_null, "mg_dev_ho_direction: p_out and q are arrays of their own");
  CHECK_ARG(aligned16(z) && aligned16(p_out) && aligned16(q) && aligned16(p_in_or_null) && aligned16(scratch), "mg_dev_ho_direction: unaligned pointer");
  const int n = d_ho_direction(z, beta_dev_or_null ? p_in_or_null : nullptr, p_out, q, beta_dev_or_null, (double*)scratch, nx, ny, ld,
                               hx, hy, coeff, sigma, (hipStream_t)stream);
  launch_reduce((double*)scratch, n, pq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_ho_residual(int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, const double* x, const double* g,
                       double* r, void* scratch, double* rr_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld) && operator_ok(hx, hy, coeff, sigma), "mg_dev_ho_residual: bad shape / pitch / spacing / shift");
  CHECK_ARG(x && g && r && scratch && rr_dev, "mg_dev_ho_residual: NULL pointer");
  CHECK_ARG(r != x && r != g, "mg_dev_ho_residual: r is an array of its own");
  CHECK_ARG(aligned16(x) && aligned16(g) && aligned16(r) && aligned16(scratch), "mg_dev_ho_residual: unaligned pointer");
  const int n = d_ho_residual(x, g, r, (double*)scratch, nx, ny, ld, hx, hy, coeff, sigma, (hipStream_t)stream);
  launch_reduce((double*)scratch, n, rr_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_ho_rhs(int nx, int ny, int ld, const double* f, double* g, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_ho_rhs: bad shape / pitch");
  CHECK_ARG(f && g && f != g, "mg_dev_ho_rhs: NULL pointer, or g is not an array of its own");
  CHECK_ARG(aligned16(f) && aligned16(g), "mg_dev_ho_rhs: unaligned pointer");
  d_ho_rhs(f, g, nx, ny, ld, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

// host arrays: upload with the library's pitch, run the kernel, download
static int ho_host(bool apply, int nx, int ny, double hx, double hy, double coeff, double sigma, const double* in, double* out) {
  const int ld = pitch_elems(MG_F64, ny);
  const size_t pitch = (size_t)ld * 8, wbytes = (size_t)ny * 8;
  void *din = nullptr, *dzero = nullptr, *dout = nullptr, *dpart = nullptr;
  auto done = [&](int rc) {
    for (void* p : {din, dzero, dout, dpart})
      if (p) (void)hipFree(p);
    return rc;
  };
  int ndev = 0;
  int rc = mg_device_count(&ndev);
  if (rc != MG_OK) return rc;
  if (ndev <= 0) return fail(nullptr, MG_ERR_NO_DEVICE, "no HIP device visible");
  if ((rc = alloc_zero(nullptr, &din, pitch * nx)) != MG_OK || (rc = alloc_zero(nullptr, &dout, pitch * nx)) != MG_OK) return done(rc);
  if (apply && ((rc = alloc_zero(nullptr, &dzero, pitch * nx)) != MG_OK ||
                (rc = alloc_zero(nullptr, &dpart, sizeof(double) * max_partials(nx, ny))) != MG_OK))
    return done(rc);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy2D(din, pitch, in, wbytes, wbytes, nx, hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(nullptr, MG_ERR_HIP, "mg_op_*_ho: upload failed"));
  if (apply) (void)d_ho_residual((const double*)din, (const double*)dzero, (double*)dout, (double*)dpart, nx, ny, ld, hx, hy, coeff, sigma, nullptr);
  else d_ho_rhs((const double*)din, (double*)dout, nx, ny, ld, nullptr);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy2D(out, wbytes, dout, pitch, wbytes, nx, hipMemcpyDeviceToHost) != hipSuccess)
    return done(fail(nullptr, MG_ERR_HIP, "mg_op_*_ho: kernel or download failed"));
  if (apply)                                           // the kernel gave 0 - A4 u, which is exact: negate (0 stays +0)
    for (size_t k = 0; k < (size_t)nx * ny; ++k) out[k] = 0.0 - out[k];
  return done(MG_OK);
}

int mg_op_apply_ho(int nx, int ny, double hx, double hy, double coeff, double sigma, const double* u, double* out) {
  CHECK_ARG(nx >= 3 && ny >= 3 && u && out && operator_ok(hx, hy, coeff, sigma), "mg_op_apply_ho: bad argument");
  return ho_host(true, nx, ny, hx, hy, coeff, sigma, u, out);
}

int mg_op_rhs_ho(int nx, int ny, const double* f, double* g) {
  CHECK_ARG(nx >= 3 && ny >= 3 && f && g, "mg_op_rhs_ho: bad argument");
  return ho_host(false, nx, ny, 1.0, 1.0, -1.0, 0.0, f, g);
}

}  // extern "C"
