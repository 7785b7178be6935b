// CDNA4 (gfx950) kernels of the conjugate-gradient outer loop around the multigrid cycle (mg_pcg.hip).  fp64 only: the Krylov
// vectors are always double, whatever precision the preconditioner runs in.  Shared conventions: mg_tile.hpp.
//
// x carries the Dirichlet data on its ring and only its interior cells are ever changed; the rings of r, p, q and z are zero
// and stay zero.
//
// Per iteration and cell: direction 4 words (z, p in, p out, q; one more with the coefficient, one more with a reaction field), update 6 (p, q, x in/out, r in/out),
// dots 2 (r, z; 3 with q for the flexible beta).
#pragma once

#include "mg_tile.hpp"

namespace mg {

// --------------------------------------------------------------------------------------------
// p' = z + beta p  (beta == nullptr: p' = z, `p` is not read),  q = A p',  partials of p' . q -- one launch.
//   p' is formed on the tile plus its halo while staging (direction_pack; VAR stages the coefficient next to it), the tile
//   of p' is stored to p_out, the stencil runs on the staged p'.  p' is written to a buffer of its OWN: a neighbouring
//   workgroup reads the old p on this tile's edge cells as its halo, so an in-place update would race across workgroups.
//   q == -(f - A p') of residual_kernel / varcoef_kernel with f = 0.
//   Stored: exactly the cells [0, nx) x [0, ny) of p_out and q (0 on the ring).
//   REACT (include/mghip_nl.h, mg_pcg_set_reaction_device): the operator is A + diag(c), q = q0 + c*p' with q0 the expression
//   above; c is read once per cell straight into registers (its ring and pad are loaded and not used).
// --------------------------------------------------------------------------------------------
template <bool VAR, bool REACT>
__global__ __launch_bounds__(kBlock) void pcg_direction_kernel(const double* __restrict__ z, const double* __restrict__ p_in,
                                                               double* __restrict__ p_out, double* __restrict__ q,
                                                               const double* __restrict__ a, const double* __restrict__ creact,
                                                               const double* __restrict__ beta_ptr,
                                                               double* __restrict__ partials, TileGeom g, double ihx2, double ihy2,
                                                               double diag, double coeff, double sigma) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  __shared__ __attribute__((aligned(16))) double sa[VAR ? S::LDS_ELEMS : S::N];
  __shared__ double red[kBlock / 64];
  const TileAt t = tile_at(g);
  const double beta = beta_ptr ? *beta_ptr : 0.0;

  Pack<double> cr[REACT ? S::RPT : 1];
  if (REACT) {
#pragma unroll
    for (int k = 0; k < S::RPT; ++k) {
      const int gi = t.i0 + t.lr + k;
      cr[REACT ? k : 0] = (gi < g.nx && t.gj0 < g.nyv) ? ldg(creact + (size_t)gi * g.ld + t.gj0) : zero_pack<double>();
    }
  }

  stage_tile_map(s, t, g, [&](int gi, int gj) { return direction_pack(z, beta_ptr ? p_in : nullptr, beta, gi, gj, g); });
  if (VAR) stage_tile<double>(a, sa, t.i0, t.j0, g.nx, g.nyv, g.ld);
  __syncthreads();

  double acc = 0.0;
  Rows3 u = rows3_start(s, t.lr + 1, t.lc), ar = rows3_start<VAR>(sa, t.lr + 1, t.lc);
#pragma unroll
  for (int k = 0; k < S::RPT; ++k) {
    rows3_advance(u, s, t.lr + k + 1, t.lc);
    rows3_advance<VAR>(ar, sa, t.lr + k + 1, t.lc);
    const int gi = t.i0 + t.lr + k;
    const bool row_in = (gi >= 1) && (gi < g.nx - 1);
    Pack<double> o;
#pragma unroll
    for (int e = 0; e < S::N; ++e) {
      double au = coeff * lap5<VAR>(u, ar, e, ihx2, ihy2, diag, sigma);
      if (REACT) au = au + cr[REACT ? k : 0].v[e] * u.mid.v[e];
      const int gj = t.gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      o.v[e] = interior ? au : 0.0;
      if (interior) acc += u.mid.v[e] * au;
    }
    if (gi < g.nx) store_cells<false>(p_out, u.mid, q, o, gi, t.gj0, g);
  }
  const double sum = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// x += alpha p,  r -= alpha q  on interior cells, partials of r . r over them.  16-byte vectors over rows 1 .. nx - 2; the
// ring columns and pad of a vector are stored back with the bits they were read with.  alpha is a device double; alpha == 0
// (what pcg_scalars_kernel leaves after a breakdown) stores nothing.
__global__ __launch_bounds__(kBlock) void pcg_update_kernel(const double* __restrict__ alpha_ptr, const double* __restrict__ p,
                                                            const double* __restrict__ q, double* __restrict__ x,
                                                            double* __restrict__ r, double* __restrict__ partials, int nx, int ny,
                                                            int nyv, int ld) {
  constexpr int N = VecW<double>::N;
  __shared__ double red[kBlock / 64];
  const double alpha = *alpha_ptr;
  const int vpr = nyv / N;
  const long long total = (long long)(nx - 2) * vpr;
  double acc = 0.0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int i = 1 + (int)(v / vpr), j = (int)(v % vpr) * N;
    const size_t at = (size_t)i * ld + j;
    const Pack<double> pp = ldg(p + at), qq = ldg(q + at);
    Pack<double> xx = ldg(x + at), rr = ldg(r + at);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      if (j + e >= 1 && j + e < ny - 1) {
        xx.v[e] = xx.v[e] + alpha * pp.v[e];
        rr.v[e] = rr.v[e] - alpha * qq.v[e];
        acc += rr.v[e] * rr.v[e];
      }
    }
    if (alpha != 0.0) {
      stg(x + at, xx);
      stg(r + at, rr);
    }
  }
  const double t = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// partials of r . z over interior cells, with FLEX also of z . q (the flexible beta is -alpha (z . q) / (r . z)_old: no old
// residual is kept) in the same pass; the second set of partials starts at partials[second].
template <bool FLEX>
__global__ __launch_bounds__(kBlock) void pcg_dots_kernel(const double* __restrict__ r, const double* __restrict__ z,
                                                          const double* __restrict__ q, double* __restrict__ partials, int second,
                                                          int nx, int ny, int nyv, int ld) {
  constexpr int N = VecW<double>::N;
  __shared__ double red[kBlock / 64], red2[kBlock / 64];
  const int vpr = nyv / N;
  const long long total = (long long)(nx - 2) * vpr;
  double acc = 0.0, acc2 = 0.0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int i = 1 + (int)(v / vpr), j = (int)(v % vpr) * N;
    const size_t at = (size_t)i * ld + j;
    const Pack<double> rr = ldg(r + at), zz = ldg(z + at);
    Pack<double> qq = zero_pack<double>();
    if (FLEX) qq = ldg(q + at);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      if (j + e >= 1 && j + e < ny - 1) {
        acc += rr.v[e] * zz.v[e];
        if (FLEX) acc2 += zz.v[e] * qq.v[e];
      }
    }
  }
  const double t = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
  if (FLEX) {
    const double t2 = block_reduce_sum(acc2, red2);
    if (threadIdx.x == 0) partials[second + blockIdx.x] = t2;
  }
}

// the boundary ring of a field := 0 (the initial residual: r = f - A x on interior cells, 0 on the ring)
__global__ __launch_bounds__(kBlock) void pcg_zero_ring_kernel(double* __restrict__ r, int nx, int ny, int ld) {
  const int n = 2 * ny + 2 * nx;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
    int i, j;
    ring_cell(t, nx, ny, i, j);
    r[(size_t)i * ld + j] = 0.0;
  }
}

// The scalar block of one solver (device doubles) and the mailbox its norm travels through.
constexpr int kPcgRz = 0, kPcgRzOld = 1, kPcgZq = 2, kPcgPq = 3, kPcgAlpha = 4, kPcgBeta = 5, kPcgRr = 6, kPcgFlag = 7,
              kPcgPostRr = 8, kPcgPostFlag = 9,   // what the last norm operation posted (later operations may move the flag)
              kPcgScalars = 10;
constexpr int kPcgBeta0 = 0;   // after the dots of the first iteration: rz only, the breakdown flag is cleared
constexpr int kPcgBetaFr = 1;  // after the dots: beta = rz / rz_old (Fletcher-Reeves)
constexpr int kPcgBetaFlex = 2;// after the dots: beta = -alpha (z . q) / rz_old (Polak-Ribiere, flexible)
constexpr int kPcgAlphaOp = 3; // after the direction: alpha = rz / pq; pq <= 0 or non-finite, or rz non-finite, sets the flag and alpha = 0
constexpr int kPcgNormOp = 4;  // after the update: rr, posted with the flag to the mailbox

struct PcgMailbox {
  double rr;
  double flag;
  unsigned long long seq;
};

// One workgroup: reduce the partial sums of the launch before it and advance the scalar block (see the kPcg* operations).
__global__ __launch_bounds__(kReduceBlock) void pcg_scalars_kernel(int op, const double* __restrict__ pa, int na,
                                                                   const double* __restrict__ pb, int nb, double* __restrict__ sc,
                                                                   PcgMailbox* mailbox, unsigned long long seq) {
  __shared__ double red[kReduceBlock / 64], red2[kReduceBlock / 64];
  const double ta = reduce_fixed(pa, na, red);
  const double tb = (nb > 0) ? reduce_fixed(pb, nb, red2) : 0.0;
  if (threadIdx.x != 0) return;
  if (op == kPcgBeta0) {
    sc[kPcgRz] = ta; sc[kPcgRzOld] = ta; sc[kPcgZq] = 0.0; sc[kPcgBeta] = 0.0; sc[kPcgFlag] = 0.0;
  } else if (op == kPcgBetaFr || op == kPcgBetaFlex) {
    const double old = sc[kPcgRz];
    sc[kPcgRzOld] = old; sc[kPcgRz] = ta; sc[kPcgZq] = tb;
    sc[kPcgBeta] = (op == kPcgBetaFlex) ? -sc[kPcgAlpha] * tb / old : ta / old;
  } else if (op == kPcgAlphaOp) {
    // p . A p <= 0 or non-finite, or a non-finite r . z (alpha would be NaN or Inf with no flag raised)
    const bool bad = !(ta > 0.0) || !(ta <= 1.79769313486231570815e308) || !(fabs(sc[kPcgRz]) <= 1.79769313486231570815e308);
    sc[kPcgPq] = ta;
    sc[kPcgAlpha] = bad ? 0.0 : sc[kPcgRz] / ta;
    if (bad) sc[kPcgFlag] = 1.0;
  } else {
    sc[kPcgRr] = ta; sc[kPcgPostRr] = ta; sc[kPcgPostFlag] = sc[kPcgFlag];
    if (mailbox) {
      mailbox->rr = ta;
      mailbox->flag = sc[kPcgFlag];
      __threadfence_system();
      __hip_atomic_store(&mailbox->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

}  // namespace mg
