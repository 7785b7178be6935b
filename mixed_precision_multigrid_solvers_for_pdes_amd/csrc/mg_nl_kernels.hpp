// CDNA4 (gfx950) kernel of the semilinear Newton method (mg_nl.hip; include/mghip_nl.h): one pass per Newton trial.  fp64 only.
// Instantiated by mg_nl.hip alone.
//
//   v = u + t delta  (delta == nullptr: v = u; on the ring v = u),  F = (f - A v) - g(v),  c = g'(v),  partials of the sum of
//   F^2 and of the sum of c over interior cells -- one launch.  g = (kappa w) phi(v), c = (kappa w) phi'(v) (w == nullptr:
//   kappa phi, kappa phi'), phi one of the four kinds of mg_nl_kind; f - A v is residual_kernel's / varcoef_kernel's own
//   expression, as in pcg_direction_kernel.
//
// Conventions as in mg_pcg_kernels.hpp: the 32 x 64 LDS tile with its one-cell halo, v formed on the tile plus halo while
// staging (VAR stages the coefficient next to it); u_out is a buffer of its OWN (a neighbouring workgroup reads u on this
// tile's edge cells as its halo); f and w are read once per cell straight into registers; sums are per-workgroup partials for
// a fixed-order pass; pad columns (>= ny) are never stored and never summed.  Stored: exactly the cells [0, nx) x [0, ny) of
// every non-null output -- the ring of u on the ring of u_out, 0 on the rings of F and c.
//
// Per cell: 2 words read (u, f) + delta, w, a where present (3 - 5), 3 written (u_out, F, c).
#pragma once

#include "mg_kernels.hpp"

namespace mg {

constexpr int kNlLinear = 0, kNlCubic = 1, kNlSinh = 2, kNlExp = 3;

// phi(v) and phi'(v) in the forms include/mghip_nl.h states
template <int KIND>
__device__ __forceinline__ void nl_phi(double v, double& ph, double& dph) {
  if (KIND == kNlLinear) { ph = v; dph = 1.0; }
  else if (KIND == kNlCubic) { const double vv = v * v; ph = vv * v; dph = 3.0 * vv; }
  else if (KIND == kNlSinh) { ph = sinh(v); dph = cosh(v); }
  else { ph = exp(v); dph = ph; }
}

// store the cells [gj0, gj0 + N) n [0, ny) of row gi (< nx): a whole vector (streamed), or cell by cell where
// the vector holds pad
__device__ __forceinline__ void nl_store(double* __restrict__ out, const Pack<double>& o, int gi, int gj0, const TileGeom& g) {
  constexpr int N = VecW<double>::N;
  double* row = out + (size_t)gi * g.ld + gj0;
  if (gj0 + N <= g.ny) {
    stg_nt(row, o);                 // streamed: none of the three outputs is read again by this launch
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (gj0 + e < g.ny) row[e] = o.v[e];
  }
}

struct NlArgs {
  double ihx2, ihy2, diag, coeff, sigma;   // the operator, as pcg_direction_kernel takes it
  double kappa, t;
  int second;                              // the partials of the sum of c start at partials[second]
};

template <int KIND, bool VAR>
__global__ __launch_bounds__(kBlock) void nl_eval_kernel(const double* __restrict__ u, const double* __restrict__ delta,
                                                         const double* __restrict__ a, const double* __restrict__ w,
                                                         const double* __restrict__ f, double* __restrict__ u_out,
                                                         double* __restrict__ F, double* __restrict__ cout,
                                                         double* __restrict__ partials, TileGeom g, NlArgs n) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  __shared__ __attribute__((aligned(16))) double sa[VAR ? S::LDS_ELEMS : S::N];
  __shared__ double red[kBlock / 64], red2[kBlock / 64];
  const int L = xcd_remap(blockIdx.x, g.ntiles);
  const int ti = L / g.tiles_j, tj = L - ti * g.tiles_j;
  const int i0 = g.i_org + ti * kTI, j0 = tj * S::TJ;
  const int cg = threadIdx.x % S::CG, rg = threadIdx.x / S::CG;
  const int gj0 = j0 + cg * S::N;
  const int lr = rg * S::RPT;
  const int lc = S::N + cg * S::N;

  Pack<double> fr[S::RPT], wr[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = i0 + lr + k;
    const bool in = gi < g.nx && gj0 < g.nyv;
    fr[k] = in ? ldg(f + (size_t)gi * g.ld + gj0) : zero_pack<double>();
    wr[k] = (in && w) ? ldg(w + (size_t)gi * g.ld + gj0) : zero_pack<double>();
  }
  // v on the tile plus its halo: u + t delta on interior cells, u on the ring, 0 outside the array
  for (int v = threadIdx.x; v < (kTI + 2) * S::VPR; v += kBlock) {
    const int r = v / S::VPR, c = v - r * S::VPR;
    const int gi = i0 - 1 + r, gj = j0 - S::N + c * S::N;
    Pack<double> o = zero_pack<double>();
    if (gi >= 0 && gi < g.nx && gj >= 0 && gj < g.nyv) {
      o = ldg(u + (size_t)gi * g.ld + gj);
      if (delta && gi >= 1 && gi < g.nx - 1) {
        const Pack<double> dd = ldg(delta + (size_t)gi * g.ld + gj);
#pragma unroll
        for (int e = 0; e < S::N; ++e)
          if (gj + e >= 1 && gj + e < g.ny - 1) o.v[e] = o.v[e] + n.t * dd.v[e];
      }
    }
    *reinterpret_cast<Pack<double>*>(s + r * S::SJ + c * S::N) = o;
  }
  if (VAR) stage_tile<double>(a, sa, i0, j0, g.nx, g.nyv, g.ld);
  __syncthreads();

  double acc = 0.0, acc2 = 0.0;
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int r = lr + k + 1;                       // LDS row of the centre
    const Pack<double> up = *reinterpret_cast<const Pack<double>*>(s + (r - 1) * S::SJ + lc);
    const Pack<double> mid = *reinterpret_cast<const Pack<double>*>(s + r * S::SJ + lc);
    const Pack<double> dn = *reinterpret_cast<const Pack<double>*>(s + (r + 1) * S::SJ + lc);
    const double left = s[r * S::SJ + lc - 1], right = s[r * S::SJ + lc + S::N];
    Pack<double> aup = zero_pack<double>(), amid = aup, adn = aup;
    double aleft = 0.0, aright = 0.0;
    if (VAR) {
      aup = *reinterpret_cast<const Pack<double>*>(sa + (r - 1) * S::SJ + lc);
      amid = *reinterpret_cast<const Pack<double>*>(sa + r * S::SJ + lc);
      adn = *reinterpret_cast<const Pack<double>*>(sa + (r + 1) * S::SJ + lc);
      aleft = sa[r * S::SJ + lc - 1];
      aright = sa[r * S::SJ + lc + S::N];
    }
    const int gi = i0 + lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> oF, oc;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const double wv = (e == 0) ? left : mid.v[e - 1];
      const double ea = (e == S::N - 1) ? right : mid.v[e + 1];
      double au;
      if (VAR) {
        const double aw = (e == 0) ? aleft : amid.v[e - 1];
        const double ae = (e == S::N - 1) ? aright : amid.v[e + 1];
        const double aip = 0.5 * (amid.v[e] + adn.v[e]), aim = 0.5 * (amid.v[e] + aup.v[e]);
        const double ajp = 0.5 * (amid.v[e] + ae), ajm = 0.5 * (amid.v[e] + aw);
        const double sx = aip * dn.v[e] + aim * up.v[e];
        const double sy = ajp * ea + ajm * wv;
        const double D0 = (aip + aim) * n.ihx2 + (ajp + ajm) * n.ihy2;
        const double D = (n.sigma != 0.0) ? D0 + n.sigma : D0;
        au = n.coeff * ((sx * n.ihx2 + sy * n.ihy2) - mid.v[e] * D);
      } else {
        au = n.coeff * (((dn.v[e] + up.v[e]) * n.ihx2 + (ea + wv) * n.ihy2) - mid.v[e] * n.diag);
      }
      double ph, dph;
      nl_phi<KIND>(mid.v[e], ph, dph);
      const double kw = w ? n.kappa * wr[k].v[e] : n.kappa;
      const double Fv = (fr[k].v[e] - au) - kw * ph;
      const double cv = kw * dph;
      const int gj = gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      oF.v[e] = interior ? Fv : 0.0;
      oc.v[e] = interior ? cv : 0.0;
      if (interior) { acc += Fv * Fv; acc2 += cv; }
    }
    if (gi < g.nx) {
      if (u_out) nl_store(u_out, mid, gi, gj0, g);
      if (F) nl_store(F, oF, gi, gj0, g);
      if (cout) nl_store(cout, oc, gi, gj0, g);
    }
  }
  const double t1 = block_reduce_sum(acc, red);
  const double t2 = block_reduce_sum(acc2, red2);
  if (threadIdx.x == 0) { partials[blockIdx.x] = t1; partials[n.second + blockIdx.x] = t2; }
}

}  // namespace mg
