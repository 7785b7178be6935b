// CDNA4 (gfx950) kernel of the semilinear Newton method (mg_nl.hip; include/mghip_nl.h): one pass per Newton trial.  fp64 only.
// Instantiated by mg_nl.hip alone.
//
//   v = u + t delta  (delta == nullptr: v = u; on the ring v = u),  F = (f - A v) - g(v),  c = g'(v),  partials of the sum of
//   F^2 and of the sum of c over interior cells -- one launch.  g = (kappa w) phi(v), c = (kappa w) phi'(v) (w == nullptr:
//   kappa phi, kappa phi'), phi one of the four kinds of mg_nl_kind; A v is lap5 with coeff and the shift, as in
//   pcg_direction_kernel.
//
// Shared conventions: mg_tile.hpp.  v is formed on the tile plus its halo while staging (VAR stages the coefficient next to
// it); u_out is a buffer of its OWN; f and w are read once per cell straight into registers.  Stored: exactly the cells
// [0, nx) x [0, ny) of every non-null output, streamed (none is read again by this launch) -- the ring of u on the ring of
// u_out, 0 on the rings of F and c.
//
// Per cell: 2 words read (u, f) + delta, w, a where present (3 - 5), 3 written (u_out, F, c).
#pragma once

#include "mg_tile.hpp"

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
  const TileAt t = tile_at(g);

  Pack<double> fr[S::RPT], wr[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = t.i0 + t.lr + k;
    const bool in = gi < g.nx && t.gj0 < g.nyv;
    fr[k] = in ? ldg(f + (size_t)gi * g.ld + t.gj0) : zero_pack<double>();
    wr[k] = (in && w) ? ldg(w + (size_t)gi * g.ld + t.gj0) : zero_pack<double>();
  }
  // v on the tile plus its halo: u + t delta on interior cells, u on the ring, 0 outside the array
  stage_tile_map(s, t, g, [&](int gi, int gj) {
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
    return o;
  });
  if (VAR) stage_tile<double>(a, sa, t.i0, t.j0, g.nx, g.nyv, g.ld);
  __syncthreads();

  double acc = 0.0, acc2 = 0.0;
  Rows3 v = rows3_start(s, t.lr + 1, t.lc), ar = rows3_start<VAR>(sa, t.lr + 1, t.lc);
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    rows3_advance(v, s, t.lr + k + 1, t.lc);
    rows3_advance<VAR>(ar, sa, t.lr + k + 1, t.lc);
    const int gi = t.i0 + t.lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> oF, oc;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const double au = n.coeff * lap5<VAR>(v, ar, e, n.ihx2, n.ihy2, n.diag, n.sigma);
      double ph, dph;
      nl_phi<KIND>(v.mid.v[e], ph, dph);
      const double kw = w ? n.kappa * wr[k].v[e] : n.kappa;
      const double Fv = (fr[k].v[e] - au) - kw * ph;
      const double cv = kw * dph;
      const int gj = t.gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      oF.v[e] = interior ? Fv : 0.0;
      oc.v[e] = interior ? cv : 0.0;
      if (interior) { acc += Fv * Fv; acc2 += cv; }
    }
    if (gi < g.nx) {
      if (u_out) store_cells<true>(u_out, v.mid, gi, t.gj0, g);
      if (F) store_cells<true>(F, oF, gi, t.gj0, g);
      if (cout) store_cells<true>(cout, oc, gi, t.gj0, g);
    }
  }
  const double t1 = block_reduce_sum(acc, red);
  const double t2 = block_reduce_sum(acc2, red2);
  if (threadIdx.x == 0) { partials[blockIdx.x] = t1; partials[n.second + blockIdx.x] = t2; }
}

}  // namespace mg
