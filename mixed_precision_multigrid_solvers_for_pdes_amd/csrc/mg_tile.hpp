// What the fp64 kernels of the solver modules share (mg_pcg_, mg_heat_, mg_rd_, mg_nl_, mg_eig_, mg_ho_ and mg_flow_kernels.hpp;
// nothing else includes this header): the walk over an LDS tile, the five-point operator, the masked row store, the ring
// decode and the fixed-order reduction.  A convention stated here is stated nowhere else.
//
// Fields (layout of mg_kernels.hpp): (nx, ny) with an even pitch `ld` in elements and a 16-byte aligned base.  A pad column
// (>= ny) is never summed, and never stored except by the kernels that say they store whole vectors up to nyv.
// Tile kernels: one workgroup per 32 x 64 tile (TileShape<double>, XCD-aware tile order), the tile plus its one-cell halo
// staged in LDS (18.5 KB per staged field), each thread 4 rows x one 16-byte vector; fields read once per cell go straight
// into registers.  An output is an array of its OWN wherever the staged field is read across tile edges.
// Sums and maxima: per-workgroup partials (block_reduce_sum / block_reduce_max), then a fixed-order pass of one workgroup
// per result (reduce_fixed): no atomics, the same bits on every run.
#pragma once

#include "mg_kernels.hpp"

namespace mg {

// Where the calling thread works: (i0, j0) the first cell of its workgroup's tile, gj0 the first column of its vector,
// lr its first tile row (LDS row lr + k + 1 is the centre of its k-th row), lc the LDS column of its vector.
struct TileAt {
  int i0, j0, gj0, lr, lc;
};
__device__ __forceinline__ TileAt tile_at(const TileGeom& g) {
  using S = TileShape<double>;
  const int L = xcd_remap(blockIdx.x, g.ntiles);
  const int ti = L / g.tiles_j, tj = L - ti * g.tiles_j;
  const int cg = threadIdx.x % S::CG, rg = threadIdx.x / S::CG;
  TileAt t;
  t.i0 = g.i_org + ti * kTI;
  t.j0 = tj * S::TJ;
  t.gj0 = t.j0 + cg * S::N;
  t.lr = rg * S::RPT;
  t.lc = S::N + cg * S::N;
  return t;
}

// stage_tile with the values formed on the way in: s := f(gi, gj) for every 16-byte vector of the tile plus its halo, (gi, gj)
// the vector's first cell -- outside the array too, so f decides what is zero.
template <typename F>
__device__ __forceinline__ void stage_tile_map(double* __restrict__ s, const TileAt& t, const TileGeom& g, F f) {
  using S = TileShape<double>;
  for (int v = threadIdx.x; v < (kTI + 2) * S::VPR; v += kBlock) {
    const int r = v / S::VPR, c = v - r * S::VPR;
    *reinterpret_cast<Pack<double>*>(s + r * S::SJ + c * S::N) = f(t.i0 - 1 + r, t.j0 - S::N + c * S::N);
  }
}

// The search direction of the Krylov loops as stage_tile_map's value: z + beta p on interior cells (p == nullptr: z, and p is
// not read), 0 on the ring, the pad and outside the array -- whatever z and p hold there.
__device__ __forceinline__ Pack<double> direction_pack(const double* __restrict__ z, const double* __restrict__ p, double beta,
                                                       int gi, int gj, const TileGeom& g) {
  constexpr int N = VecW<double>::N;
  Pack<double> o = zero_pack<double>();
  if (gi >= 1 && gi < g.nx - 1 && gj >= 0 && gj < g.nyv) {
    const Pack<double> zz = ldg(z + (size_t)gi * g.ld + gj);
    Pack<double> pp = zero_pack<double>();
    if (p) pp = ldg(p + (size_t)gi * g.ld + gj);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const bool interior = gj + e >= 1 && gj + e < g.ny - 1;
      const double pn = p ? zz.v[e] + beta * pp.v[e] : zz.v[e];
      o.v[e] = interior ? pn : 0.0;
    }
  }
  return o;
}

// The staged rows r - 1, r, r + 1 at a thread's vector, with the cell to either side of the centre row: a window that rolls
// down the thread's rows, so that each staged row is read from LDS once (loading three rows per centre row costs more LDS
// reads: the compiler does not merge them all).  rows3_start(s, r, lc) holds rows r - 1 and r for the first advance to centre
// row r; rows3_advance(h, s, r, lc) moves to centre row r, one below the last.  PRESENT = false reads nothing and leaves
// zeros (the coefficient field of a constant-coefficient instantiation).
struct Rows3 {
  Pack<double> up, mid, dn;
  double left, right;
  __device__ __forceinline__ double w(int e) const { return (e == 0) ? left : mid.v[e - 1]; }
  __device__ __forceinline__ double ea(int e) const { return (e == VecW<double>::N - 1) ? right : mid.v[e + 1]; }
};
template <bool PRESENT = true>
__device__ __forceinline__ Rows3 rows3_start(const double* s, int r, int lc) {
  using S = TileShape<double>;
  Rows3 h;
  h.up = h.mid = h.dn = zero_pack<double>();
  h.left = h.right = 0.0;
  if (PRESENT) {
    h.mid = *reinterpret_cast<const Pack<double>*>(s + (r - 1) * S::SJ + lc);
    h.dn = *reinterpret_cast<const Pack<double>*>(s + r * S::SJ + lc);
  }
  return h;
}
template <bool PRESENT = true>
__device__ __forceinline__ void rows3_advance(Rows3& h, const double* s, int r, int lc) {
  using S = TileShape<double>;
  if (PRESENT) {
    h.up = h.mid;
    h.mid = h.dn;
    h.dn = *reinterpret_cast<const Pack<double>*>(s + (r + 1) * S::SJ + lc);
    h.left = s[r * S::SJ + lc - 1];
    h.right = s[r * S::SJ + lc + S::N];
  }
}

// The five-point operator at cell e of the centre row, without `coeff`, in ONE association for every solver module -- that
// of residual_kernel (constant coefficient; `diag` carries the shift) and of varcoef_kernel (VAR: L_a u = div(a grad u) with
// the vertex field a, whose ring is read):
//   ((dn + up)*ihx2 + (ea + w)*ihy2) - c*diag
//   aip = 0.5*(a_c + a_dn), aim = 0.5*(a_c + a_up), ajp = 0.5*(a_c + a_e), ajm = 0.5*(a_c + a_w)
//   ((aip*dn + aim*up)*ihx2 + (ajp*ea + ajm*w)*ihy2) - c*(((aip + aim)*ihx2 + (ajp + ajm)*ihy2) [+ sigma where sigma != 0])
// What mg_op_apply(coeff = +1) gives, bit for bit.  A caller without a shift passes a literal 0.0 and the select folds away.
template <bool VAR>
__device__ __forceinline__ double lap5(const Rows3& u, const Rows3& a, int e, double ihx2, double ihy2, double diag,
                                       double sigma) {
  if (VAR) {
    const double aip = 0.5 * (a.mid.v[e] + a.dn.v[e]), aim = 0.5 * (a.mid.v[e] + a.up.v[e]);
    const double ajp = 0.5 * (a.mid.v[e] + a.ea(e)), ajm = 0.5 * (a.mid.v[e] + a.w(e));
    const double sx = aip * u.dn.v[e] + aim * u.up.v[e];
    const double sy = ajp * u.ea(e) + ajm * u.w(e);
    const double D0 = (aip + aim) * ihx2 + (ajp + ajm) * ihy2;
    const double D = (sigma != 0.0) ? D0 + sigma : D0;
    return (sx * ihx2 + sy * ihy2) - u.mid.v[e] * D;
  }
  return ((u.dn.v[e] + u.up.v[e]) * ihx2 + (u.ea(e) + u.w(e)) * ihy2) - u.mid.v[e] * diag;
}

// Store the cells [gj0, gj0 + N) n [0, ny) of row gi (< nx): a whole vector, or cell by cell where the vector holds pad.
// STREAM stores the vector with the non-temporal hint: for an output nothing reads again soon.
template <bool STREAM>
__device__ __forceinline__ void store_cells(double* __restrict__ out, const Pack<double>& o, int gi, int gj0, const TileGeom& g) {
  constexpr int N = VecW<double>::N;
  double* row = out + (size_t)gi * g.ld + gj0;
  if (gj0 + N <= g.ny) {
    if (STREAM) stg_nt(row, o);
    else stg(row, o);
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (gj0 + e < g.ny) row[e] = o.v[e];
  }
}
// The same for two outputs under ONE branch: the direction kernels' p' and q (two calls of the form above cost
// pcg_direction_kernel 8 % at 4097^2).
template <bool STREAM>
__device__ __forceinline__ void store_cells(double* __restrict__ out, const Pack<double>& o, double* __restrict__ out2,
                                            const Pack<double>& o2, int gi, int gj0, const TileGeom& g) {
  constexpr int N = VecW<double>::N;
  double* row = out + (size_t)gi * g.ld + gj0;
  double* row2 = out2 + (size_t)gi * g.ld + gj0;
  if (gj0 + N <= g.ny) {
    if (STREAM) { stg_nt(row, o); stg_nt(row2, o2); }
    else { stg(row, o); stg(row2, o2); }
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (gj0 + e < g.ny) { row[e] = o.v[e]; row2[e] = o2.v[e]; }
  }
}

// Cell t of the 2 ny + 2 nx passes over the boundary ring: row 0, row nx - 1, column 0, column ny - 1, in this order.  Each
// corner comes up twice, in a row pass and in a column pass.
__device__ __forceinline__ void ring_cell(int t, int nx, int ny, int& i, int& j) {
  if (t < ny) { i = 0; j = t; }
  else if (t < 2 * ny) { i = nx - 1; j = t - ny; }
  else if (t < 2 * ny + nx) { i = t - 2 * ny; j = 0; }
  else { i = t - 2 * ny - nx; j = ny - 1; }
}

// Fixed-order sum of n partials by a whole workgroup of kReduceBlock threads (reduce_partials_kernel's pattern); valid in
// thread 0.  `red` is kReduceBlock / 64 doubles of LDS of its own.
__device__ __forceinline__ double reduce_fixed(const double* __restrict__ partials, int n, double* red) {
  double a0 = 0.0, a1 = 0.0;
  int i = threadIdx.x;
  for (; i + kReduceBlock < n; i += 2 * kReduceBlock) { a0 += partials[i]; a1 += partials[i + kReduceBlock]; }
  for (; i < n; i += kReduceBlock) a0 += partials[i];
  return block_reduce_sum<kReduceBlock / 64>(a0 + a1, red);
}

// The maximum that keeps a NaN: fmax returns the operand that is NOT one, which would report a field that has blown up as
// a field at rest.  Every maximum of the solver modules -- per thread, per wave, per block, reduce_rows_kernel -- is formed
// with it, so the result is NaN if any participating value is; for other operands it is fmax's value, bit for bit.
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double wave_reduce_max(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = nan_max(x, __shfl_down(x, o, 64));
  return x;
}
// Maximum over the block of NW waves; result valid in thread 0.  `red` is >= NW doubles of LDS of its own.
template <int NW = kBlock / 64>
__device__ __forceinline__ double block_reduce_max(double x, double* red) {
  x = wave_reduce_max(x);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = x;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    t = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) t = nan_max(t, red[w]);
  }
  return t;
}

// One workgroup per result: workgroup b reduces the n partials that start at partials[b * stride] into out[b], in a fixed
// order -- a sum, or (WITH_MAX) a maximum where bit b of `max_mask` is set.  A template, so that every unit that launches it
// may define it.
template <bool WITH_MAX>
__global__ __launch_bounds__(kReduceBlock) void reduce_rows_kernel(const double* __restrict__ partials, int n, int stride,
                                                                   int max_mask, double* __restrict__ out) {
  __shared__ double red[kReduceBlock / 64];
  const double* p = partials + (size_t)blockIdx.x * stride;
  double t;
  if (WITH_MAX && ((max_mask >> blockIdx.x) & 1)) {
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += kReduceBlock) m = nan_max(m, p[i]);
    t = block_reduce_max<kReduceBlock / 64>(m, red);
  } else {
    t = reduce_fixed(p, n, red);
  }
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}

}  // namespace mg
