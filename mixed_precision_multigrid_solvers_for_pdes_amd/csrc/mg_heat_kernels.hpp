// CDNA4 (gfx950) kernels of the device-resident heat-equation stepper (mg_heat.hip).  fp64 only: the state of a time stepper
// is double, and so is the inner solve (include/mghip.h, "Time stepping").  Shared conventions: mg_tile.hpp.
//
// Per step and cell: the right-hand side 2 words (u in, f out; 3 with u_prev for BDF2, one more with a source profile, one
// more with a diffusivity field where the scheme evaluates the operator), the ring a perimeter, the difference norm of step
// doubling 2 (a, b).
#pragma once

#include "mg_tile.hpp"

namespace mg {

constexpr int kHeatExplicit = 0, kHeatImplicit = 1, kHeatCn = 2, kHeatBdf2 = 3;

// scalars of one step, formed on the host in the host stepper's order of operations
struct HeatCoef {
  double ihx2, ihy2, diag;   // the residual kernels' stencil constants (mgh::coefs, no shift)
  double a, dt;              // diffusivity, step
  double dta;                // dt * a
  double two_dta;            // 2 * dt * a
  double g0, g1;             // time factors of the source at t and t + dt
};

// --------------------------------------------------------------------------------------------
// The right-hand side of one step in ONE pass over the field, with sum out^2 over all cells of the array.
//   implicit Euler   f = (u + dt*(g1*S)) / (dt*a)
//   Crank-Nicolson   f = (2.0*((u + ((dt*a)*lap)/2) + (dt*((g0*S)+(g1*S)))/2)) / (dt*a)
//   BDF2             f = (4.0*u - u_prev)/(2*dt*a) + (g1*S)/a
//   explicit Euler   u_new = u + dt*((a*lap) + g0*S)            (not a right-hand side: the whole step)
// on interior cells, in exactly this association (applications/heat_equation.py:155-266 through our host stepper); the ring
// of the array is 0 for the three right-hand sides (the engine's norm counts r = f there) and u's own for the explicit step.
// lap is lap5 without a shift: what mg_op_apply(coeff = +1) gives, bit for bit.  HAS_SRC = false reads no S and evaluates the
// formulas with S = 0.
//   Explicit Euler and Crank-Nicolson need the stencil: the tile of u is staged in LDS.  The other two read u (and u_prev)
//   straight into registers.
//   Stored: rows 0 .. nx - 1 as whole 16-byte vectors up to column roundup(ny, 2) (a pad column there is written 0).
//   VAR (explicit Euler and Crank-Nicolson only: the other two hold no operator): lap = L_a u with the vertex field `a`, staged
//   next to u.  One more word per cell.
// --------------------------------------------------------------------------------------------
template <int SCHEME, bool HAS_SRC, bool VAR = false>
__global__ __launch_bounds__(kBlock) void heat_rhs_kernel(const double* __restrict__ u, const double* __restrict__ u_prev,
                                                          const double* __restrict__ src, const double* __restrict__ a,
                                                          double* __restrict__ out, double* __restrict__ partials, TileGeom g,
                                                          HeatCoef c) {
  using S = TileShape<double>;
  constexpr bool LAP = SCHEME == kHeatExplicit || SCHEME == kHeatCn;
  static_assert(LAP || !VAR, "implicit Euler and BDF2 never read the diffusivity field");
  __shared__ __attribute__((aligned(16))) double s[LAP ? S::LDS_ELEMS : S::N];
  __shared__ __attribute__((aligned(16))) double sa[VAR ? S::LDS_ELEMS : S::N];
  __shared__ double red[kBlock / 64];
  const TileAt t = tile_at(g);

  Pack<double> sv[S::RPT], pv[S::RPT], uv[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = t.i0 + t.lr + k;
    const bool in = gi < g.nx && t.gj0 < g.nyv;
    const size_t at = (size_t)gi * g.ld + t.gj0;
    sv[k] = (HAS_SRC && in) ? ldg(src + at) : zero_pack<double>();
    pv[k] = (SCHEME == kHeatBdf2 && in) ? ldg(u_prev + at) : zero_pack<double>();
    uv[k] = (!LAP && in) ? ldg(u + at) : zero_pack<double>();
  }
  if (LAP) {
    stage_tile<double>(u, s, t.i0, t.j0, g.nx, g.nyv, g.ld);
    if (VAR) stage_tile<double>(a, sa, t.i0, t.j0, g.nx, g.nyv, g.ld);
    __syncthreads();
  }

  double acc = 0.0;
  Rows3 ur = rows3_start<LAP>(s, t.lr + 1, t.lc), ar = rows3_start<VAR>(sa, t.lr + 1, t.lc);
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    rows3_advance<LAP>(ur, s, t.lr + k + 1, t.lc);
    rows3_advance<VAR>(ar, sa, t.lr + k + 1, t.lc);
    if (!LAP) ur.mid = uv[k];
    const int gi = t.i0 + t.lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const int gj = t.gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      const double uc = ur.mid.v[e];
      const double lap = LAP ? lap5<VAR>(ur, ar, e, c.ihx2, c.ihy2, c.diag, 0.0) : 0.0;
      const double sc = HAS_SRC ? sv[k].v[e] : 0.0;
      double val, ring = 0.0;
      if (SCHEME == kHeatExplicit) {
        val = uc + c.dt * ((c.a * lap) + c.g0 * sc);
        ring = uc;
      } else if (SCHEME == kHeatImplicit) {
        val = (uc + c.dt * (c.g1 * sc)) / c.dta;
      } else if (SCHEME == kHeatCn) {
        val = (2.0 * ((uc + (c.dta * lap) / 2) + (c.dt * ((c.g0 * sc) + (c.g1 * sc))) / 2)) / c.dta;
      } else {
        val = (4.0 * uc - pv[k].v[e]) / c.two_dta + (c.g1 * sc) / c.a;
      }
      const bool inside = gi < g.nx && gj < g.ny;
      const double ov = interior ? val : (inside ? ring : 0.0);
      o.v[e] = ov;
      acc += ov * ov;
    }
    if (gi < g.nx && t.gj0 < g.nyv) stg(out + (size_t)gi * g.ld + t.gj0, o);
  }
  const double sum = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// The Dirichlet ring of u from four scalars {left, right, bottom, top}, in the order the host stepper applies them
// (applications/heat_equation.py:499-577): left (i = 0, whole row), right (i = nx - 1), bottom (j = 0, whole column), top
// (j = ny - 1) -- so a corner carries the value of the later edge: bottom on column 0, top on column ny - 1.  Each cell is
// written once, with the value that order leaves there.
__global__ __launch_bounds__(kBlock) void heat_ring_kernel(double* __restrict__ u, int nx, int ny, int ld, double left,
                                                           double right, double bottom, double top) {
  const int n = 2 * ny + 2 * nx;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
    int i, j;
    ring_cell(t, nx, ny, i, j);
    if (t < 2 * ny && (j == 0 || j == ny - 1)) continue;      // the corners belong to the column passes
    const double v = (j == ny - 1) ? top : (j == 0) ? bottom : (i == 0) ? left : right;
    u[(size_t)i * ld + j] = v;
  }
}

// partials of sum (a - b)^2 over all cells [0, nx) x [0, ny), unweighted: what np.linalg.norm(a - b) squares to (the error
// estimate of step doubling).  16-byte vectors, pad columns masked.
__global__ __launch_bounds__(kBlock) void heat_diff_sumsq_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                                 double* __restrict__ partials, int nx, int ny, int nyv, int ld) {
  constexpr int N = VecW<double>::N;
  __shared__ double red[kBlock / 64];
  const int vpr = nyv / N;
  const long long total = (long long)nx * vpr;
  double acc = 0.0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int i = (int)(v / vpr), j = (int)(v % vpr) * N;
    const size_t at = (size_t)i * ld + j;
    const Pack<double> aa = ldg(a + at), bb = ldg(b + at);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      if (j + e < ny) {
        const double d = aa.v[e] - bb.v[e];
        acc += d * d;
      }
    }
  }
  const double t = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

}  // namespace mg
