// CDNA4 (gfx950) kernels of the device-resident heat-equation stepper (mg_heat.hip).  fp64 only: the state of a time stepper
// is double, and so is the inner solve (include/mghip.h, "Time stepping").
//
// Conventions (field layout as in mg_kernels.hpp): every field is (nx, ny) with an even pitch `ld` in elements and a 16-byte
// aligned base.  Sums are per-workgroup partials (block_reduce_sum) followed by heat_reduce_kernel, a fixed-order pass of one
// workgroup: no atomics, the same bits on every run.  Pad columns (>= ny) are masked out of the sums.
//
// Per step and cell: the right-hand side 2 words (u in, f out; 3 with u_prev for BDF2, one more with a source profile, one
// more with a diffusivity field where the scheme evaluates the operator), the ring a perimeter, the difference norm of step
// doubling 2 (a, b).
#pragma once

#include "mg_kernels.hpp"

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
// lap is residual_kernel's expression, ((dn + up) ihx2 + (ea + w) ihy2) - mid diag: what mg_op_apply(coeff = +1) gives, bit
// for bit.  HAS_SRC = false reads no S and evaluates the formulas with S = 0.
//   Explicit Euler and Crank-Nicolson need the stencil: LDS-tiled like residual_kernel (tile + 1-cell halo of u staged with
//   16-byte loads, the stencil runs on the staged values).  The other two read u (and u_prev) straight into registers.
//   Stored: rows 0 .. nx - 1 as whole 16-byte vectors up to column roundup(ny, 2) (a pad column there is written 0).  `out` is
//   an array of its own: neighbouring workgroups read u across tile edges.
//   VAR (explicit Euler and Crank-Nicolson only: the other two hold no operator): lap = L_a u = div(a grad u) with the vertex
//   field `a`, whose tile + halo is staged in a second LDS array next to u's (2 x 18.5 KB per workgroup, as
//   pcg_direction_kernel<true> and varcoef_kernel), in exactly their association:
//     aip = 0.5*(a_c + a_dn), aim = 0.5*(a_c + a_up), ajp = 0.5*(a_c + a_e), ajm = 0.5*(a_c + a_w)
//     lap = ((aip*dn + aim*up)*ihx2 + (ajp*ea + ajm*w)*ihy2) - uc*((aip + aim)*ihx2 + (ajp + ajm)*ihy2)
//   The ring values of `a` are read (the faces next to the boundary).  One more word per cell.
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
  const int L = xcd_remap(blockIdx.x, g.ntiles);
  const int ti = L / g.tiles_j, tj = L - ti * g.tiles_j;
  const int i0 = g.i_org + ti * kTI, j0 = tj * S::TJ;
  const int cg = threadIdx.x % S::CG, rg = threadIdx.x / S::CG;
  const int gj0 = j0 + cg * S::N;
  const int lr = rg * S::RPT;
  const int lc = S::N + cg * S::N;

  Pack<double> sv[S::RPT], pv[S::RPT], uv[S::RPT];
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    const int gi = i0 + lr + k;
    const bool in = gi < g.nx && gj0 < g.nyv;
    const size_t at = (size_t)gi * g.ld + gj0;
    sv[k] = (HAS_SRC && in) ? ldg(src + at) : zero_pack<double>();
    pv[k] = (SCHEME == kHeatBdf2 && in) ? ldg(u_prev + at) : zero_pack<double>();
    uv[k] = (!LAP && in) ? ldg(u + at) : zero_pack<double>();
  }
  if (LAP) {
    stage_tile<double>(u, s, i0, j0, g.nx, g.nyv, g.ld);
    if (VAR) stage_tile<double>(a, sa, i0, j0, g.nx, g.nyv, g.ld);
    __syncthreads();
  }

  Pack<double> up = zero_pack<double>(), mid = up, aup = up, amid = up;
  if (LAP) {
    up = *reinterpret_cast<const Pack<double>*>(s + (lr + 0) * S::SJ + lc);
    mid = *reinterpret_cast<const Pack<double>*>(s + (lr + 1) * S::SJ + lc);
  }
  if (VAR) {
    aup = *reinterpret_cast<const Pack<double>*>(sa + (lr + 0) * S::SJ + lc);
    amid = *reinterpret_cast<const Pack<double>*>(sa + (lr + 1) * S::SJ + lc);
  }
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    Pack<double> dn = zero_pack<double>();
    double left = 0.0, right = 0.0;
    if (LAP) {
      dn = *reinterpret_cast<const Pack<double>*>(s + (lr + k + 2) * S::SJ + lc);
      left = s[(lr + k + 1) * S::SJ + lc - 1];
      right = s[(lr + k + 1) * S::SJ + lc + S::N];
    } else {
      mid = uv[k];
    }
    Pack<double> adn = zero_pack<double>();
    double aleft = 0.0, aright = 0.0;
    if (VAR) {
      adn = *reinterpret_cast<const Pack<double>*>(sa + (lr + k + 2) * S::SJ + lc);
      aleft = sa[(lr + k + 1) * S::SJ + lc - 1];
      aright = sa[(lr + k + 1) * S::SJ + lc + S::N];
    }
    const int gi = i0 + lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      const int gj = gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      const double uc = mid.v[e];
      double lap = 0.0;
      if (LAP) {
        const double w = (e == 0) ? left : mid.v[e - 1];
        const double ea = (e == S::N - 1) ? right : mid.v[e + 1];
        if (VAR) {
          const double aw = (e == 0) ? aleft : amid.v[e - 1];
          const double ae = (e == S::N - 1) ? aright : amid.v[e + 1];
          const double aip = 0.5 * (amid.v[e] + adn.v[e]), aim = 0.5 * (amid.v[e] + aup.v[e]);
          const double ajp = 0.5 * (amid.v[e] + ae), ajm = 0.5 * (amid.v[e] + aw);
          const double sx = aip * dn.v[e] + aim * up.v[e];
          const double sy = ajp * ea + ajm * w;
          const double D0 = (aip + aim) * c.ihx2 + (ajp + ajm) * c.ihy2;
          lap = (sx * c.ihx2 + sy * c.ihy2) - uc * D0;
        } else {
          lap = ((dn.v[e] + up.v[e]) * c.ihx2 + (ea + w) * c.ihy2) - uc * c.diag;
        }
      }
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
    if (gi < g.nx && gj0 < g.nyv) stg(out + (size_t)gi * g.ld + gj0, o);
    if (LAP) {
      up = mid;
      mid = dn;
    }
    if (VAR) {
      aup = amid;
      amid = adn;
    }
  }
  const double t = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
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
    if (t < ny) { i = 0; j = t; }
    else if (t < 2 * ny) { i = nx - 1; j = t - ny; }
    else if (t < 2 * ny + nx) { i = t - 2 * ny; j = 0; }
    else { i = t - 2 * ny - nx; j = ny - 1; }
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

// One workgroup: the fixed-order sum of n partials (reduce_partials_kernel's pattern) into *out.
__global__ __launch_bounds__(kReduceBlock) void heat_reduce_kernel(const double* __restrict__ partials, int n,
                                                                   double* __restrict__ out) {
  __shared__ double red[kReduceBlock / 64];
  double a0 = 0.0, a1 = 0.0;
  int i = threadIdx.x;
  for (; i + kReduceBlock < n; i += 2 * kReduceBlock) { a0 += partials[i]; a1 += partials[i + kReduceBlock]; }
  for (; i < n; i += kReduceBlock) a0 += partials[i];
  const double t = block_reduce_sum<kReduceBlock / 64>(a0 + a1, red);
  if (threadIdx.x == 0) *out = t;
}

}  // namespace mg
