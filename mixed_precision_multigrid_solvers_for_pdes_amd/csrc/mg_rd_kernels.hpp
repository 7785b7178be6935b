// CDNA4 (gfx950) kernels of the device-resident reaction-diffusion stepper (mg_rd.hip; include/mghip_rd.h).  fp64 only.
// Instantiated by mg_rd.hip alone.  Shared conventions: mg_tile.hpp.
//
// Per cell: the right-hand side 2 words (u in, f out) + u_prev, S, a, w where present (Crank-Nicolson up to 6, BDF2 3 - 4,
// implicit Euler 2 - 3); the energy 1 word read (u) + a, w where present.
#pragma once

#include "mg_tile.hpp"

namespace mg {

constexpr int kRdImplicit = 1, kRdCn = 2, kRdBdf2 = 3;            // MG_HEAT_IMPLICIT_EULER, _CRANK_NICOLSON, _BDF2
constexpr int kRdLinear = 0, kRdCubic = 1, kRdSinh = 2, kRdExp = 3;   // mg_nl_kind

// phi(v) in the forms of mg_nl_kind
template <int KIND>
__device__ __forceinline__ double rd_phi(double v) {
  if (KIND == kRdLinear) return v;
  else if (KIND == kRdCubic) return (v * v) * v;
  else if (KIND == kRdSinh) return sinh(v);
  else return exp(v);
}

// its antiderivative Phi >= 0 in the forms include/mghip_rd.h states
template <int KIND>
__device__ __forceinline__ double rd_Phi(double v) {
  if (KIND == kRdLinear) return (v * v) / 2;
  else if (KIND == kRdCubic) return ((v * v) * (v * v)) / 4;
  else if (KIND == kRdSinh) return cosh(v) - 1.0;
  else return exp(v);
}

// scalars of one step, formed on the host
struct RdCoef {
  double ihx2, ihy2, diag;   // the residual kernels' stencil constants (no shift)
  double a, dt;              // alpha, step
  double dta;                // dt * alpha
  double two_dta;            // 2 * dt * alpha
  double g0, g1;             // time factors of the source at t and t + dt
  double ka;                 // kappa / alpha: the strength the Newton method carries
  double rho;
  double ra;                 // rho / alpha
  double r2a;                // (2 * rho) / alpha
};

// --------------------------------------------------------------------------------------------
// The right-hand side of one step in ONE pass, with the partials of the sum of out^2 (include/mghip_rd.h for the formulas and
// their association).
//   Crank-Nicolson evaluates the operator (lap5 without a shift) and phi(u) on the staged tile of u (VAR: and of a); KIND and
//   VAR are its template parameters alone.  Implicit Euler and BDF2 hold neither: u goes straight into registers and they are
//   instantiated once each (KIND = linear, VAR = false).
//   u_prev (BDF2; Crank-Nicolson when non-null), S and w (non-null) are read once per cell into registers: nullable at run
//   time (workgroup-uniform branches), so their presence multiplies no instantiation.
//   Stored: exactly the cells [0, nx) x [0, ny), 0 on the ring, streamed (out is not read again by this launch).
// --------------------------------------------------------------------------------------------
template <int SCHEME, int KIND, bool VAR>
__global__ __launch_bounds__(kBlock) void rd_rhs_kernel(const double* __restrict__ u, const double* __restrict__ u_prev,
                                                        const double* __restrict__ src, const double* __restrict__ a,
                                                        const double* __restrict__ w, double* __restrict__ out,
                                                        double* __restrict__ partials, TileGeom g, RdCoef c) {
  using S = TileShape<double>;
  constexpr bool CN = SCHEME == kRdCn;
  static_assert(CN || (!VAR && KIND == kRdLinear), "implicit Euler and BDF2 read neither the diffusivity field nor phi(u)");
  __shared__ __attribute__((aligned(16))) double s[CN ? S::LDS_ELEMS : S::N];
  __shared__ __attribute__((aligned(16))) double sa[VAR ? S::LDS_ELEMS : S::N];
  __shared__ double red[kBlock / 64];
  const TileAt t = tile_at(g);
  const bool has_prev = SCHEME == kRdBdf2 || (CN && u_prev != nullptr);
  const bool has_w = CN && w != nullptr;

  Pack<double> sv[S::RPT], pv[S::RPT], wv[S::RPT], uv[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = t.i0 + t.lr + k;
    const bool in = gi < g.nx && t.gj0 < g.nyv;
    const size_t at = (size_t)gi * g.ld + t.gj0;
    sv[k] = (src && in) ? ldg(src + at) : zero_pack<double>();
    pv[k] = (has_prev && in) ? ldg(u_prev + at) : zero_pack<double>();
    wv[k] = (has_w && in) ? ldg(w + at) : zero_pack<double>();
    uv[k] = (!CN && in) ? ldg(u + at) : zero_pack<double>();
  }
  if (CN) {
    stage_tile<double>(u, s, t.i0, t.j0, g.nx, g.nyv, g.ld);
    if (VAR) stage_tile<double>(a, sa, t.i0, t.j0, g.nx, g.nyv, g.ld);
    __syncthreads();
  }

  double acc = 0.0;
  Rows3 ur = rows3_start<CN>(s, t.lr + 1, t.lc), ar = rows3_start<VAR>(sa, t.lr + 1, t.lc);
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    rows3_advance<CN>(ur, s, t.lr + k + 1, t.lc);
    rows3_advance<VAR>(ar, sa, t.lr + k + 1, t.lc);
    if (!CN) ur.mid = uv[k];
    const int gi = t.i0 + t.lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const int gj = t.gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      const double uc = ur.mid.v[e];
      const double sc = sv[k].v[e];                     // 0 without a source
      const double pc = pv[k].v[e];
      double val;
      if (SCHEME == kRdImplicit) {
        val = (uc + c.dt * ((c.g1 * sc) + c.rho * uc)) / c.dta;
      } else if (CN) {
        const double lap = lap5<VAR>(ur, ar, e, c.ihx2, c.ihy2, c.diag, 0.0);
        const double h = (2.0 * ((uc + (c.dta * lap) / 2) + (c.dt * ((c.g0 * sc) + (c.g1 * sc))) / 2)) / c.dta;
        const double kw = has_w ? c.ka * wv[k].v[e] : c.ka;
        const double E = has_prev ? (3.0 * uc - pc) / 2 : uc;
        val = (h + c.r2a * E) - kw * rd_phi<KIND>(uc);      // the library call last: its ulps reach f unamplified
      } else {
        val = ((4.0 * uc - pc) / c.two_dta + (c.g1 * sc) / c.a) + c.ra * (2.0 * uc - pc);
      }
      const double ov = interior ? val : 0.0;
      o.v[e] = ov;
      acc += ov * ov;
    }
    if (gi < g.nx) store_cells<true>(out, o, gi, t.gj0, g);
  }
  const double sum = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// --------------------------------------------------------------------------------------------
// The three sums of the free energy in ONE pass over a state (include/mghip_rd.h): G (gradient), P (potential), Q (sum of
// squares); their partials start at partials[0], partials[second] and partials[2 * second].  The tile of u (VAR: and of a) is
// staged; each cell owns the face to its next row and the face to its next column; w (non-null) is read once per cell.
// Terms are selected, not multiplied by a mask: a non-finite cell reaches exactly the sums it enters.
// --------------------------------------------------------------------------------------------
template <int KIND, bool VAR>
__global__ __launch_bounds__(kBlock) void rd_energy_kernel(const double* __restrict__ u, const double* __restrict__ a,
                                                           const double* __restrict__ w, double* __restrict__ partials,
                                                           TileGeom g, double rx, double ry, int second) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  __shared__ __attribute__((aligned(16))) double sa[VAR ? S::LDS_ELEMS : S::N];
  __shared__ double red[3][kBlock / 64];
  const TileAt t = tile_at(g);

  Pack<double> wv[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = t.i0 + t.lr + k;
    wv[k] = (w && gi < g.nx && t.gj0 < g.nyv) ? ldg(w + (size_t)gi * g.ld + t.gj0) : zero_pack<double>();
  }
  stage_tile<double>(u, s, t.i0, t.j0, g.nx, g.nyv, g.ld);
  if (VAR) stage_tile<double>(a, sa, t.i0, t.j0, g.nx, g.nyv, g.ld);
  __syncthreads();

  double accG = 0.0, accP = 0.0, accQ = 0.0;
  Rows3 ur = rows3_start(s, t.lr + 1, t.lc), ar = rows3_start<VAR>(sa, t.lr + 1, t.lc);
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    rows3_advance(ur, s, t.lr + k + 1, t.lc);
    rows3_advance<VAR>(ar, sa, t.lr + k + 1, t.lc);
    const int gi = t.i0 + t.lr + k;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const int gj = t.gj0 + e;
      const double uc = ur.mid.v[e];
      const double du = ur.dn.v[e] - uc, dv = ur.ea(e) - uc;
      double fx = du * du, fy = dv * dv;
      if (VAR) {
        fx = (0.5 * (ar.mid.v[e] + ar.dn.v[e])) * fx;
        fy = (0.5 * (ar.mid.v[e] + ar.ea(e))) * fy;
      }
      const bool xface = gi < g.nx - 1 && gj >= 1 && gj < g.ny - 1;      // (gi, gj) - (gi + 1, gj)
      const bool yface = gi >= 1 && gi < g.nx - 1 && gj < g.ny - 1;      // (gi, gj) - (gi, gj + 1)
      const bool interior = yface && gj >= 1;
      const double tx = xface ? fx * rx : 0.0, ty = yface ? fy * ry : 0.0;
      accG += 0.5 * (tx + ty);
      const double Ph = rd_Phi<KIND>(uc);
      const double pt = w ? wv[k].v[e] * Ph : Ph;
      accP += interior ? pt : 0.0;
      accQ += interior ? uc * uc : 0.0;
    }
  }
  const double t0 = block_reduce_sum(accG, red[0]);
  const double t1 = block_reduce_sum(accP, red[1]);
  const double t2 = block_reduce_sum(accQ, red[2]);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = t0;
    partials[second + blockIdx.x] = t1;
    partials[2 * second + blockIdx.x] = t2;
  }
}

}  // namespace mg
