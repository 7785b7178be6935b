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
// Conventions as in mg_pcg_kernels.hpp: the 32 x 64 LDS tile with its one-cell halo (which already holds the four corner
// neighbours: 4 words per cell in the direction kernel, as with the five-point operator); sums are per-workgroup partials
// for a fixed-order pass; pad columns (>= ny) are never stored and never summed.
#pragma once

#include "mg_kernels.hpp"

namespace mg {

struct HoArgs {
  double cC, cE, cN, cK;   // the stencil weights
  double mcoeff;           // -coeff
};

// A4 at the LDS cells (r, lc .. lc + N) of a staged tile: rows r - 1, r, r + 1 with their left / right neighbours
struct HoRows {
  Pack<double> up, mid, dn;
  double up_w, up_e, mid_w, mid_e, dn_w, dn_e;
};
__device__ __forceinline__ HoRows ho_load_rows(const double* s, int r, int lc) {
  using S = TileShape<double>;
  HoRows h;
  h.up = *reinterpret_cast<const Pack<double>*>(s + (r - 1) * S::SJ + lc);
  h.mid = *reinterpret_cast<const Pack<double>*>(s + r * S::SJ + lc);
  h.dn = *reinterpret_cast<const Pack<double>*>(s + (r + 1) * S::SJ + lc);
  h.up_w = s[(r - 1) * S::SJ + lc - 1];  h.up_e = s[(r - 1) * S::SJ + lc + S::N];
  h.mid_w = s[r * S::SJ + lc - 1];       h.mid_e = s[r * S::SJ + lc + S::N];
  h.dn_w = s[(r + 1) * S::SJ + lc - 1];  h.dn_e = s[(r + 1) * S::SJ + lc + S::N];
  return h;
}
__device__ __forceinline__ double ho_apply(const HoRows& h, int e, const HoArgs& c) {
  constexpr int N = VecW<double>::N;
  const double w = (e == 0) ? h.mid_w : h.mid.v[e - 1], ea = (e == N - 1) ? h.mid_e : h.mid.v[e + 1];
  const double dn_w = (e == 0) ? h.dn_w : h.dn.v[e - 1], dn_e = (e == N - 1) ? h.dn_e : h.dn.v[e + 1];
  const double up_w = (e == 0) ? h.up_w : h.up.v[e - 1], up_e = (e == N - 1) ? h.up_e : h.up.v[e + 1];
  return c.mcoeff * (((c.cC * h.mid.v[e] + c.cE * (h.dn.v[e] + h.up.v[e])) + c.cN * (ea + w)) - c.cK * ((dn_e + dn_w) + (up_e + up_w)));
}

// store the cells [gj0, gj0 + N) n [0, ny) of row gi (< nx): a whole vector, or cell by cell where the vector holds pad
__device__ __forceinline__ void ho_store(double* __restrict__ out, const Pack<double>& o, int gi, int gj0, const TileGeom& g) {
  constexpr int N = VecW<double>::N;
  double* row = out + (size_t)gi * g.ld + gj0;
  if (gj0 + N <= g.ny) {
    stg(row, o);
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (gj0 + e < g.ny) row[e] = o.v[e];
  }
}

// --------------------------------------------------------------------------------------------
// p' = z + beta p  (beta == nullptr: p' = z, `p` is not read),  q = A4 p',  partials of p' . q -- pcg_direction_kernel's
// contract with the nine-point operator.  p' is formed on the tile plus its halo while staging (0 on the ring and outside
// the array), so the corners of the halo are p' too.  p_out is a buffer of its own (neighbouring workgroups read the old p
// on this tile's edge).  Stored: exactly the cells [0, nx) x [0, ny) of p_out and q (0 on the ring).
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ho_direction_kernel(const double* __restrict__ z, const double* __restrict__ p_in,
                                                              double* __restrict__ p_out, double* __restrict__ q,
                                                              const double* __restrict__ beta_ptr, double* __restrict__ partials,
                                                              TileGeom g, HoArgs c) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  __shared__ double red[kBlock / 64];
  const int L = xcd_remap(blockIdx.x, g.ntiles);
  const int ti = L / g.tiles_j, tj = L - ti * g.tiles_j;
  const int i0 = g.i_org + ti * kTI, j0 = tj * S::TJ;
  const double beta = beta_ptr ? *beta_ptr : 0.0;

  for (int v = threadIdx.x; v < (kTI + 2) * S::VPR; v += kBlock) {
    const int r = v / S::VPR, cv = v - r * S::VPR;
    const int gi = i0 - 1 + r, gj = j0 - S::N + cv * S::N;
    Pack<double> o = zero_pack<double>();
    if (gi >= 1 && gi < g.nx - 1 && gj >= 0 && gj < g.nyv) {
      const Pack<double> zz = ldg(z + (size_t)gi * g.ld + gj);
      Pack<double> pp = zero_pack<double>();
      if (beta_ptr) pp = ldg(p_in + (size_t)gi * g.ld + gj);
#pragma unroll
      for (int e = 0; e < S::N; ++e) {
        const bool interior = gj + e >= 1 && gj + e < g.ny - 1;
        const double pn = beta_ptr ? zz.v[e] + beta * pp.v[e] : zz.v[e];
        o.v[e] = interior ? pn : 0.0;
      }
    }
    *reinterpret_cast<Pack<double>*>(s + r * S::SJ + cv * S::N) = o;
  }
  __syncthreads();

  const int cg = threadIdx.x % S::CG, rg = threadIdx.x / S::CG;
  const int gj0 = j0 + cg * S::N;
  const int lr = rg * S::RPT;
  const int lc = S::N + cg * S::N;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const HoRows h = ho_load_rows(s, lr + k + 1, lc);
    const int gi = i0 + lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const double au = ho_apply(h, e, c);
      const int gj = gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      o.v[e] = interior ? au : 0.0;
      if (interior) acc += h.mid.v[e] * au;
    }
    if (gi < g.nx) {
      ho_store(p_out, h.mid, gi, gj0, g);
      ho_store(q, o, gi, gj0, g);
    }
  }
  const double t = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
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
  const int L = xcd_remap(blockIdx.x, g.ntiles);
  const int ti = L / g.tiles_j, tj = L - ti * g.tiles_j;
  const int i0 = g.i_org + ti * kTI, j0 = tj * S::TJ;
  const int cg = threadIdx.x % S::CG, rg = threadIdx.x / S::CG;
  const int gj0 = j0 + cg * S::N;
  const int lr = rg * S::RPT;
  const int lc = S::N + cg * S::N;

  Pack<double> f[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = i0 + lr + k;
    f[k] = (gi < g.nx && gj0 < g.nyv) ? ldg(rhs + (size_t)gi * g.ld + gj0) : zero_pack<double>();
  }
  stage_tile<double>(x, s, i0, j0, g.nx, g.nyv, g.ld);
  __syncthreads();

  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const HoRows h = ho_load_rows(s, lr + k + 1, lc);
    const int gi = i0 + lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const double au = ho_apply(h, e, c);
      const int gj = gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      const double rv = interior ? (f[k].v[e] - au) : 0.0;
      o.v[e] = rv;
      acc += rv * rv;
    }
    if (WRITE_R && gi < g.nx) ho_store(r, o, gi, gj0, g);
  }
  const double t = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// --------------------------------------------------------------------------------------------
// g = R f on interior cells (reads f on the ring, never its corners), the ring of g := the ring of f.  `out` is an array
// of its own.  Stored: exactly the cells [0, nx) x [0, ny) of out.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ho_rhs_kernel(const double* __restrict__ f, double* __restrict__ out, TileGeom g) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  const int L = xcd_remap(blockIdx.x, g.ntiles);
  const int ti = L / g.tiles_j, tj = L - ti * g.tiles_j;
  const int i0 = g.i_org + ti * kTI, j0 = tj * S::TJ;
  const int cg = threadIdx.x % S::CG, rg = threadIdx.x / S::CG;
  const int gj0 = j0 + cg * S::N;
  const int lr = rg * S::RPT;
  const int lc = S::N + cg * S::N;
  stage_tile<double>(f, s, i0, j0, g.nx, g.nyv, g.ld);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int r = lr + k + 1;
    const Pack<double> up = *reinterpret_cast<const Pack<double>*>(s + (r - 1) * S::SJ + lc);
    const Pack<double> mid = *reinterpret_cast<const Pack<double>*>(s + r * S::SJ + lc);
    const Pack<double> dn = *reinterpret_cast<const Pack<double>*>(s + (r + 1) * S::SJ + lc);
    const double left = s[r * S::SJ + lc - 1], right = s[r * S::SJ + lc + S::N];
    const int gi = i0 + lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const double w = (e == 0) ? left : mid.v[e - 1];
      const double ea = (e == S::N - 1) ? right : mid.v[e + 1];
      const double rf = (8.0 * mid.v[e] + ((dn.v[e] + up.v[e]) + (ea + w))) / 12.0;
      const int gj = gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      o.v[e] = interior ? rf : mid.v[e];
    }
    if (gi < g.nx) ho_store(out, o, gi, gj0, g);
  }
}

}  // namespace mg
