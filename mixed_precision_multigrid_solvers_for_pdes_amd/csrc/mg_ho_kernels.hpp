// CDNA4 (gfx950) kernels of the fourth-order compact ("Mehrstellen") nine-point discretisation of -Laplace + sigma that the
// conjugate-gradient outer loop may run on (mg_pcg.hip, mg_pcg_set_order(4); include/mghip_ho.h).  fp64 only, constant
// coefficients only.  Instantiated by mg_ho.hip alone.
//
//   A4 u = -coeff * [ cC u_C + cE (u_(i+1,j) + u_(i-1,j)) + cN (u_(i,j+1) + u_(i,j-1)) - cK (the four corners) ]
//   R f  = (8 f_C + f_(i+1,j) + f_(i-1,j) + f_(i,j+1) + f_(i,j-1)) / 12
// and the scheme solves A4 u = R f on interior cells.  The four c's are computed once on the host (HoCoef, mg_host.hpp);
// the rounding sequence per cell is fixed (-ffp-contract=off keeps it):
//   A4:  (-coeff) * (((cC*C + cE*(dn+up)) + cN*(ea+w)) - cK*((dn_e+dn_w)+(up_e+up_w)))
//   R:   (8.0*f + ((dn+up) + (ea+w))) / 12.0
// with dn / up the rows i+1 / i-1 and ea / w the columns j+1 / j-1.
//
// Shared conventions: mg_tile.hpp.  The one-cell halo of the staged tile already holds the four corner neighbours: 4 words per
// cell in the direction kernel, as with the five-point operator.
#pragma once

#include "mg_tile.hpp"

namespace mg {

struct HoArgs {
  double cC, cE, cN, cK;   // the stencil weights
  double mcoeff;           // -coeff
};

// A4 at the LDS cells (r, lc .. lc + N) of a staged tile: Rows3 with the four corner neighbours of the vector
struct HoRows {
  Rows3 r;
  double up_w, up_e, dn_w, dn_e;
};
__device__ __forceinline__ HoRows ho_start(const double* s, int r, int lc) {
  using S = TileShape<double>;
  HoRows h;
  h.r = rows3_start(s, r, lc);
  h.r.left = s[(r - 1) * S::SJ + lc - 1];  h.r.right = s[(r - 1) * S::SJ + lc + S::N];
  h.up_w = h.up_e = 0.0;
  h.dn_w = s[r * S::SJ + lc - 1];          h.dn_e = s[r * S::SJ + lc + S::N];
  return h;
}
// the corner cells roll with the rows: rows3_advance's own loads of the centre row's neighbours are dead here
__device__ __forceinline__ void ho_advance(HoRows& h, const double* s, int r, int lc) {
  using S = TileShape<double>;
  const double mid_w = h.dn_w, mid_e = h.dn_e;
  h.up_w = h.r.left;  h.up_e = h.r.right;
  rows3_advance(h.r, s, r, lc);
  h.r.left = mid_w;  h.r.right = mid_e;
  h.dn_w = s[(r + 1) * S::SJ + lc - 1];  h.dn_e = s[(r + 1) * S::SJ + lc + S::N];
}
__device__ __forceinline__ double ho_apply(const HoRows& h, int e, const HoArgs& c) {
  constexpr int N = VecW<double>::N;
  const Rows3& u = h.r;
  const double dn_w = (e == 0) ? h.dn_w : u.dn.v[e - 1], dn_e = (e == N - 1) ? h.dn_e : u.dn.v[e + 1];
  const double up_w = (e == 0) ? h.up_w : u.up.v[e - 1], up_e = (e == N - 1) ? h.up_e : u.up.v[e + 1];
  return c.mcoeff * (((c.cC * u.mid.v[e] + c.cE * (u.dn.v[e] + u.up.v[e])) + c.cN * (u.ea(e) + u.w(e))) - c.cK * ((dn_e + dn_w) + (up_e + up_w)));
}

// --------------------------------------------------------------------------------------------
// p' = z + beta p  (beta == nullptr: p' = z, `p` is not read),  q = A4 p',  partials of p' . q -- pcg_direction_kernel's
// contract with the nine-point operator: the corners of the staged halo are p' too.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ho_direction_kernel(const double* __restrict__ z, const double* __restrict__ p_in,
                                                              double* __restrict__ p_out, double* __restrict__ q,
                                                              const double* __restrict__ beta_ptr, double* __restrict__ partials,
                                                              TileGeom g, HoArgs c) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  __shared__ double red[kBlock / 64];
  const TileAt t = tile_at(g);
  const double beta = beta_ptr ? *beta_ptr : 0.0;

  stage_tile_map(s, t, g, [&](int gi, int gj) { return direction_pack(z, beta_ptr ? p_in : nullptr, beta, gi, gj, g); });
  __syncthreads();

  double acc = 0.0;
  HoRows h = ho_start(s, t.lr + 1, t.lc);
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    ho_advance(h, s, t.lr + k + 1, t.lc);
    const int gi = t.i0 + t.lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const double au = ho_apply(h, e, c);
      const int gj = t.gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      o.v[e] = interior ? au : 0.0;
      if (interior) acc += h.r.mid.v[e] * au;
    }
    if (gi < g.nx) store_cells<false>(p_out, h.r.mid, q, o, gi, t.gj0, g);
  }
  const double sum = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// --------------------------------------------------------------------------------------------
// r = rhs - A4 x on interior cells (x carries the Dirichlet ring, corners included), 0 on the ring; partials of the sum of
// r^2 over interior cells.  WRITE_R = false only sums (the true residual of the returned iterate).  Stored: exactly the
// cells [0, nx) x [0, ny) of r.
// --------------------------------------------------------------------------------------------
template <bool WRITE_R>
__global__ __launch_bounds__(kBlock) void ho_residual_kernel(const double* __restrict__ x, const double* __restrict__ rhs,
                                                             double* __restrict__ r, double* __restrict__ partials, TileGeom g,
                                                             HoArgs c) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  __shared__ double red[kBlock / 64];
  const TileAt t = tile_at(g);

  Pack<double> f[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = t.i0 + t.lr + k;
    f[k] = (gi < g.nx && t.gj0 < g.nyv) ? ldg(rhs + (size_t)gi * g.ld + t.gj0) : zero_pack<double>();
  }
  stage_tile<double>(x, s, t.i0, t.j0, g.nx, g.nyv, g.ld);
  __syncthreads();

  double acc = 0.0;
  HoRows h = ho_start(s, t.lr + 1, t.lc);
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    ho_advance(h, s, t.lr + k + 1, t.lc);
    const int gi = t.i0 + t.lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const double au = ho_apply(h, e, c);
      const int gj = t.gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      const double rv = interior ? (f[k].v[e] - au) : 0.0;
      o.v[e] = rv;
      acc += rv * rv;
    }
    if (WRITE_R && gi < g.nx) store_cells<false>(r, o, gi, t.gj0, g);
  }
  const double sum = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// --------------------------------------------------------------------------------------------
// g = R f on interior cells (reads f on the ring, never its corners), the ring of g := the ring of f.  `out` is an array
// of its own.  Stored: exactly the cells [0, nx) x [0, ny) of out.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ho_rhs_kernel(const double* __restrict__ f, double* __restrict__ out, TileGeom g) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  const TileAt t = tile_at(g);
  stage_tile<double>(f, s, t.i0, t.j0, g.nx, g.nyv, g.ld);
  __syncthreads();
  Rows3 u = rows3_start(s, t.lr + 1, t.lc);
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    rows3_advance(u, s, t.lr + k + 1, t.lc);
    const int gi = t.i0 + t.lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const double rf = (8.0 * u.mid.v[e] + ((u.dn.v[e] + u.up.v[e]) + (u.ea(e) + u.w(e)))) / 12.0;
      const int gj = t.gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      o.v[e] = interior ? rf : u.mid.v[e];
    }
    if (gi < g.nx) store_cells<false>(out, o, gi, t.gj0, g);
  }
}

}  // namespace mg
