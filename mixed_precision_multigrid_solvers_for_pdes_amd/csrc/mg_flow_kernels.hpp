// CDNA4 (gfx950) kernels of the device-resident vorticity / stream-function stepper (mg_flow.hip, include/mghip_flow.h):
// 2-D incompressible flow  w_t = J(psi, w) + nu lap w + F,  -lap psi = w,  u = psi_y, v = -psi_x.  fp64 only.
//
// Shared conventions: mg_tile.hpp.  i is x, j is y and contiguous.
//
// Per step and cell: the right-hand side 5 words (psi, w, N_prev in; f, N out; one more with a forcing field), the wall ring a
// perimeter, the right-hand side of the psi solve 3 (w_new, w_old in; w with a zero ring out), the diagnostics 2 (psi, w).
#pragma once

#include "mg_tile.hpp"

namespace mg {

// scalars of one step, formed on the host
struct FlowCoef {
  double ihx2, ihy2, diag;   // the residual kernels' stencil constants (mgh::coefs, no shift)
  double sigma;              // 2 / (nu dt)
  double k;                  // 2 / nu
  double c0, c1;             // Adams-Bashforth weights: 1 + r/2, -r/2 with r = dt / dt_prev (1, 0 on a first step)
  double d12;                // 12.0 * hx * hy
};

// one staged row of a thread's two columns with the column to either side: a[0] = j - 1, a[1], a[2] the pack, a[3] = j + 2
struct FlowRow {
  double a[4];
};
__device__ __forceinline__ FlowRow flow_row(const double* __restrict__ s, int row, int lc) {
  using S = TileShape<double>;
  FlowRow r;
  const Pack<double> p = *reinterpret_cast<const Pack<double>*>(s + row * S::SJ + lc);
  r.a[0] = s[row * S::SJ + lc - 1];
  r.a[1] = p.v[0];
  r.a[2] = p.v[1];
  r.a[3] = s[row * S::SJ + lc + S::N];
  return r;
}

// --------------------------------------------------------------------------------------------
// The right-hand side of the vorticity solve in ONE pass over the field.  With p = psi, w = omega, E/W = i +- 1, N/S = j +- 1:
//   J1 = (E(p)-W(p))*(N(w)-S(w)) - (N(p)-S(p))*(E(w)-W(w))
//   J2 = ((E(p)*(NE(w)-SE(w)) - W(p)*(NW(w)-SW(w))) - N(p)*(NE(w)-NW(w))) + S(p)*(SE(w)-SW(w))
//   J3 = ((NE(p)*(N(w)-E(w)) - SW(p)*(W(w)-S(w))) - NW(p)*(N(w)-W(w))) + SE(p)*(E(w)-S(w))
//   J  = ((J1 + J2) + J3) / (12.0*hx*hy)                       (Arakawa 1966; a true division)
//   N  = J + F                                                 (HAS_FORCE; else N = J)
//   f  = (sigma*w + lap) + k*((c0*N) + (c1*N_prev))            (HAS_PREV; else f = (sigma*w + lap) + k*(c0*N), N_prev unread)
// on interior cells, 0 on the ring of both outputs.  lap is lap5's constant-coefficient expression written on the FlowRows,
// ((E + W) ihx2 + (N + S) ihy2) - w diag: what mg_op_apply(coeff = +1) gives, bit for bit.  The tiles of psi AND w are staged;
// the Jacobian and lap run on the staged values (the halo holds the corners).  partials[b] = sum f^2 of workgroup b,
// partials[np + b] = max(|N(p)-S(p)| + |E(p)-W(p)|) over its interior cells (np = g.ntiles): the host forms
// cfl = dt m / (2 hx hy).
//   Stored: rows 0 .. nx - 1 of f and N as whole 16-byte vectors up to column roundup(ny, 2) (a pad column there is written
//   0).
// --------------------------------------------------------------------------------------------
template <bool HAS_PREV, bool HAS_FORCE>
__global__ __launch_bounds__(kBlock) void flow_rhs_kernel(const double* __restrict__ psi, const double* __restrict__ om,
                                                          const double* __restrict__ nprev, const double* __restrict__ force,
                                                          double* __restrict__ f_out, double* __restrict__ n_out,
                                                          double* __restrict__ partials, TileGeom g, FlowCoef c) {
  using S = TileShape<double>;
  static_assert(S::N == 2, "two columns per thread");
  __shared__ __attribute__((aligned(16))) double sp[S::LDS_ELEMS];
  __shared__ __attribute__((aligned(16))) double sw[S::LDS_ELEMS];
  __shared__ double red[kBlock / 64];
  __shared__ double redm[kBlock / 64];
  const TileAt t = tile_at(g);
  const int i0 = t.i0, j0 = t.j0, gj0 = t.gj0, lr = t.lr, lc = t.lc;

  Pack<double> pv[S::RPT], fv[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = i0 + lr + k;
    const bool in = gi < g.nx && gj0 < g.nyv;
    const size_t at = (size_t)gi * g.ld + gj0;
    pv[k] = (HAS_PREV && in) ? ldg(nprev + at) : zero_pack<double>();
    fv[k] = (HAS_FORCE && in) ? ldg(force + at) : zero_pack<double>();
  }
  stage_tile<double>(psi, sp, i0, j0, g.nx, g.nyv, g.ld);
  stage_tile<double>(om, sw, i0, j0, g.nx, g.nyv, g.ld);
  __syncthreads();

  FlowRow pu = flow_row(sp, lr + 0, lc), pm = flow_row(sp, lr + 1, lc);
  FlowRow wu = flow_row(sw, lr + 0, lc), wm = flow_row(sw, lr + 1, lc);
  double acc = 0.0, vmax = 0.0;
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const FlowRow pd = flow_row(sp, lr + k + 2, lc), wd = flow_row(sw, lr + k + 2, lc);
    const int gi = i0 + lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> of, on;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const int gj = gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      const int m = 1 + e;
      const double pE = pd.a[m], pW = pu.a[m], pN = pm.a[m + 1], pS = pm.a[m - 1];
      const double pNE = pd.a[m + 1], pSE = pd.a[m - 1], pNW = pu.a[m + 1], pSW = pu.a[m - 1];
      const double wE = wd.a[m], wW = wu.a[m], wN = wm.a[m + 1], wS = wm.a[m - 1];
      const double wNE = wd.a[m + 1], wSE = wd.a[m - 1], wNW = wu.a[m + 1], wSW = wu.a[m - 1];
      const double wc = wm.a[m];
      const double dpx = pE - pW, dpy = pN - pS;
      const double J1 = dpx * (wN - wS) - dpy * (wE - wW);
      const double J2 = ((pE * (wNE - wSE) - pW * (wNW - wSW)) - pN * (wNE - wNW)) + pS * (wSE - wSW);
      const double J3 = ((pNE * (wN - wE) - pSW * (wW - wS)) - pNW * (wN - wW)) + pSE * (wE - wS);
      const double J = ((J1 + J2) + J3) / c.d12;
      const double nn = HAS_FORCE ? J + fv[k].v[e] : J;
      const double lap = ((wE + wW) * c.ihx2 + (wN + wS) * c.ihy2) - wc * c.diag;
      const double ab = HAS_PREV ? (c.c0 * nn) + (c.c1 * pv[k].v[e]) : c.c0 * nn;
      const double val = (c.sigma * wc + lap) + c.k * ab;
      const double ov = interior ? val : 0.0;
      of.v[e] = ov;
      on.v[e] = interior ? nn : 0.0;
      acc += ov * ov;
      vmax = nan_max(vmax, interior ? fabs(dpy) + fabs(dpx) : 0.0);
    }
    if (gi < g.nx && gj0 < g.nyv) {
      stg(f_out + (size_t)gi * g.ld + gj0, of);
      stg(n_out + (size_t)gi * g.ld + gj0, on);
    }
    pu = pm; pm = pd;
    wu = wm; wm = wd;
  }
  const double sum = block_reduce_sum(acc, red);
  const double tm = block_reduce_max(vmax, redm);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = sum;
    partials[g.ntiles + blockIdx.x] = tm;
  }
}

constexpr int kFlowFreeSlip = 0, kFlowNoSlip = 1;

// The ring of w from psi: 0 (free slip) or Thom's formula with the wall speeds {left v, right v, bottom u, top u}:
//   left   (i = 0):      (2.0*(psi[0][j]    - psi[1][j]))/(hx*hx)    - (2.0*vl)/hx
//   right  (i = nx - 1): (2.0*(psi[nx-1][j] - psi[nx-2][j]))/(hx*hx) + (2.0*vr)/hx
//   bottom (j = 0):      (2.0*(psi[i][0]    - psi[i][1]))/(hy*hy)    + (2.0*ub)/hy
//   top    (j = ny - 1): (2.0*(psi[i][ny-1] - psi[i][ny-2]))/(hy*hy) - (2.0*ut)/hy
// applied in this order, so the corners carry bottom and top (heat_ring_kernel's order).  Each ring cell is written once;
// the interior is untouched.  A perimeter's worth of work.
__global__ __launch_bounds__(kBlock) void flow_wall_kernel(double* __restrict__ om, const double* __restrict__ psi, int nx, int ny,
                                                           int ld, int kind, double hx, double hy, double vl, double vr, double ub,
                                                           double ut) {
  const int n = 2 * ny + 2 * nx;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
    int i, j;
    ring_cell(t, nx, ny, i, j);
    if (t < 2 * ny && (j == 0 || j == ny - 1)) continue;      // the corners belong to the column passes
    double v = 0.0;
    if (kind == kFlowNoSlip) {
      const double pw = psi[(size_t)i * ld + j];
      if (j == ny - 1) v = (2.0 * (pw - psi[(size_t)i * ld + j - 1])) / (hy * hy) - (2.0 * ut) / hy;
      else if (j == 0) v = (2.0 * (pw - psi[(size_t)i * ld + 1])) / (hy * hy) + (2.0 * ub) / hy;
      else if (i == 0) v = (2.0 * (pw - psi[(size_t)ld + j])) / (hx * hx) - (2.0 * vl) / hx;
      else v = (2.0 * (pw - psi[(size_t)(i - 1) * ld + j])) / (hx * hx) + (2.0 * vr) / hx;
    }
    om[(size_t)i * ld + j] = v;
  }
}

// The right-hand side of the stream-function solve: out = w on interior cells, 0 on the ring (the engine's norm counts r = f
// there, and mg_update_rhs_device's contract is a zero ring), stored like flow_rhs_kernel's outputs.  partials[b] = sum out^2,
// partials[nb + b] = max |w - w_old| over all cells (nb = gridDim.x; HAS_OLD = false reads no w_old and gives 0).
template <bool HAS_OLD>
__global__ __launch_bounds__(kBlock) void flow_interior_kernel(const double* __restrict__ w, const double* __restrict__ w_old,
                                                               double* __restrict__ out, double* __restrict__ partials, int nx,
                                                               int ny, int nyv, int ld) {
  constexpr int N = VecW<double>::N;
  __shared__ double red[kBlock / 64];
  __shared__ double redm[kBlock / 64];
  const int vpr = nyv / N;
  const long long total = (long long)nx * vpr;
  double acc = 0.0, vmax = 0.0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int i = (int)(v / vpr), j = (int)(v % vpr) * N;
    const size_t at = (size_t)i * ld + j;
    const Pack<double> a = ldg(w + at);
    const Pack<double> b = HAS_OLD ? ldg(w_old + at) : zero_pack<double>();
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const bool interior = i >= 1 && i < nx - 1 && j + e >= 1 && j + e < ny - 1;
      const double ov = interior ? a.v[e] : 0.0;
      o.v[e] = ov;
      acc += ov * ov;
      if (HAS_OLD) vmax = nan_max(vmax, j + e < ny ? fabs(a.v[e] - b.v[e]) : 0.0);
    }
    stg(out + at, o);
  }
  const double t = block_reduce_sum(acc, red);
  const double tm = block_reduce_max(vmax, redm);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = t;
    partials[gridDim.x + blockIdx.x] = tm;
  }
}

// Diagnostics over interior cells: partials[b] = sum psi*w (kinetic energy is 0.5 hx hy of it when psi = 0 on the walls),
// partials[nb + b] = sum w^2 (enstrophy is 0.5 hx hy of it), partials[2 nb + b] = max(|N(p)-S(p)| + |E(p)-W(p)|), the
// velocity maximum flow_rhs_kernel forms (here from global loads: a diagnostic, the neighbours come from the caches).
__global__ __launch_bounds__(kBlock) void flow_diag_kernel(const double* __restrict__ psi, const double* __restrict__ w,
                                                           double* __restrict__ partials, int nx, int ny, int nyv, int ld) {
  constexpr int N = VecW<double>::N;
  __shared__ double red0[kBlock / 64];
  __shared__ double red1[kBlock / 64];
  __shared__ double redm[kBlock / 64];
  const int vpr = nyv / N;
  const long long total = (long long)(nx - 2) * vpr;
  double a0 = 0.0, a1 = 0.0, vmax = 0.0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int i = 1 + (int)(v / vpr), j = (int)(v % vpr) * N;
    const size_t at = (size_t)i * ld + j;
    const Pack<double> p = ldg(psi + at), q = ldg(w + at), pe = ldg(psi + at + ld), pw = ldg(psi + at - ld);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      if (j + e >= 1 && j + e < ny - 1) {
        a0 += p.v[e] * q.v[e];
        a1 += q.v[e] * q.v[e];
        const double pn = (e == N - 1) ? psi[at + N] : p.v[e + 1];
        const double ps = (e == 0) ? psi[at - 1] : p.v[e - 1];
        vmax = nan_max(vmax, fabs(pn - ps) + fabs(pe.v[e] - pw.v[e]));
      }
    }
  }
  const double t0 = block_reduce_sum(a0, red0);
  const double t1 = block_reduce_sum(a1, red1);
  const double tm = block_reduce_max(vmax, redm);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = t0;
    partials[gridDim.x + blockIdx.x] = t1;
    partials[2 * gridDim.x + blockIdx.x] = tm;
  }
}

}  // namespace mg
