// CDNA4 (gfx950) kernels of the block eigensolver (mg_eig.hip): LOBPCG around the multigrid cycle.  fp64 only: the block
// vectors are always double, whatever precision the preconditioner runs in.
//
// Shared conventions: mg_tile.hpp.  A block is a run of columns, each an (nx, ld) field, `col_stride` elements apart.  Inner
// products run over interior cells only: the ring and the pad columns (>= ny) of an operand are masked, never assumed to be
// zero.
//
// Per cell and call: gram reads each of its columns once (p + q words, or their union where u and v share columns), combine
// reads p and writes q, apply reads 1 and writes 1 per column (2 with the coefficient), residual reads 2 and writes 1.
#pragma once

#include "mg_tile.hpp"

namespace mg {

constexpr int kEigMaxP = 48, kEigMaxQ = 96;      // gram: p <= 48 rows, q <= 96 columns of G (3 x 6 blocks of 16 x 16)
constexpr int kEigKC = 64;                       // cells of one gram tile: a 512-byte row segment of every column
constexpr int kEigKCP = kEigKC + 2;              // LDS stride of a column: the 32 lanes of a half wave (16 columns x 2 cells) hit 32 distinct bank pairs
constexpr int kEigWaveBlocks = 5;                // 16 x 16 blocks of G one wave accumulates: ceil(3 * 6 / 4)
constexpr int kEigGramLdsBytes = (kEigMaxP + kEigMaxQ) * kEigKCP * 8;

typedef double eig_v4d __attribute__((ext_vector_type(4)));

struct EigGramArgs {
  const double* seg0;      // staged into LDS columns [0, n0)
  const double* seg1;      // ... [n0, n0 + n1); n1 == 0 where u and v lie in one run of columns
  int n0, n1;
  int uo, vo;              // LDS column of u_0 and of v_0
  int p, q;
  int nx, ny, ld;
  long long col_stride;
  int tiles_j, ntiles;     // tiles of kEigKC cells over rows 1 .. nx - 2
  int direct;              // 1: one workgroup, G goes straight to `out` (p x q); 0: padded partial blocks
};

// --------------------------------------------------------------------------------------------
// G[a][b] = sum over interior cells of u_a v_b as one tall-skinny product on the matrix cores.
//   A workgroup walks tiles of kEigKC cells of one grid row: every staged column's segment goes to LDS with coalesced 16-byte
//   loads (ring and pad cells as 0.0, whatever they hold), then each wave runs v_mfma_f64_16x16x4_f64 over the tile for the
//   16 x 16 blocks of G it owns (block index mod 4 == wave): operand A is u[column l & 15][cell l >> 4], operand B is
//   v[cell l >> 4][column l & 15], one double per lane, zero for the columns that pad p and q to multiples of 16.  The
//   loads of the workgroup's next tile are issued before that loop and land in registers under it.  The
//   accumulator of lane l holds G[row (l >> 4) + 4 reg][column l & 15] of its block (the f64 map, not the f32 one).
//   At the end the workgroup writes its blocks to partials[blockIdx.x][PB * 16][QB * 16]; eig_gram_reduce_kernel sums them.
// --------------------------------------------------------------------------------------------
template <int NLD>      // 16-byte vectors a thread stages per tile: (n0 + n1) * (kEigKC / 2) <= NLD * kBlock
__global__ __launch_bounds__(kBlock) void eig_gram_kernel(EigGramArgs g, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double eig_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int PB = (g.p + 15) >> 4, QB = (g.q + 15) >> 4, nblk = PB * QB;
  eig_v4d acc[kEigWaveBlocks];
  int aoff[kEigWaveBlocks], boff[kEigWaveBlocks];
#pragma unroll
  for (int t = 0; t < kEigWaveBlocks; ++t) {
    acc[t] = eig_v4d{0.0, 0.0, 0.0, 0.0};
    const int blk = wave + 4 * t;
    const int pb = blk / QB, qb = blk - pb * QB;
    const int a = pb * 16 + li, b = qb * 16 + li;
    aoff[t] = (blk < nblk && a < g.p) ? (g.uo + a) * kEigKCP + lk : -1;
    boff[t] = (blk < nblk && b < g.q) ? (g.vo + b) * kEigKCP + lk : -1;
  }
  const int nvec = (g.n0 + g.n1) * (kEigKC / 2);
  // The next tile travels from HBM into registers while the matrix cores work on the staged one: `pre` is only touched
  // again (masked and written to LDS) after the MFMA loop.
  Pack<double> pre[NLD];
  auto fetch = [&](int tile) {
    const int ti = tile / g.tiles_j, tj = tile - ti * g.tiles_j;
    const int gi = 1 + ti, j0 = tj * kEigKC;
#pragma unroll
    for (int s = 0; s < NLD; ++s) {
      const int v = threadIdx.x + s * kBlock;
      pre[s] = zero_pack<double>();
      if (v < nvec) {
        const int c = v / (kEigKC / 2), k = (v - c * (kEigKC / 2)) * 2;
        const double* base = c < g.n0 ? g.seg0 + (long long)c * g.col_stride : g.seg1 + (long long)(c - g.n0) * g.col_stride;
        const int gj = j0 + k;
        if (gj + 2 <= g.ld && gj < g.ny - 1) pre[s] = ldg(base + (size_t)gi * g.ld + gj);
      }
    }
  };
  auto stage = [&](int tile) {
    const int j0 = (tile % g.tiles_j) * kEigKC;
#pragma unroll
    for (int s = 0; s < NLD; ++s) {
      const int v = threadIdx.x + s * kBlock;
      if (v < nvec) {
        const int c = v / (kEigKC / 2), k = (v - c * (kEigKC / 2)) * 2;
        const int gj = j0 + k;
        Pack<double> x = pre[s];
        if (gj < 1) x.v[0] = 0.0;
        if (gj + 1 >= g.ny - 1) x.v[1] = 0.0;
        *reinterpret_cast<Pack<double>*>(eig_lds + c * kEigKCP + k) = x;
      }
    }
  };
  int tile = blockIdx.x;
  if (tile < g.ntiles) fetch(tile);
  for (; tile < g.ntiles; tile += gridDim.x) {
    stage(tile);
    __syncthreads();
    if (tile + (int)gridDim.x < g.ntiles) fetch(tile + gridDim.x);
#pragma unroll 2
    for (int k0 = 0; k0 < kEigKC; k0 += 4) {
#pragma unroll
      for (int t = 0; t < kEigWaveBlocks; ++t) {
        if (wave + 4 * t < nblk) {               // wave-uniform
          const double a = aoff[t] >= 0 ? eig_lds[aoff[t] + k0] : 0.0;
          const double b = boff[t] >= 0 ? eig_lds[boff[t] + k0] : 0.0;
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  const int QP = QB * 16;
#pragma unroll
  for (int t = 0; t < kEigWaveBlocks; ++t) {
    const int blk = wave + 4 * t;
    if (blk < nblk) {
      const int pb = blk / QB, qb = blk - pb * QB;
      const int col = qb * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = pb * 16 + lk + 4 * r;
        if (g.direct) {
          if (row < g.p && col < g.q) out[row * g.q + col] = acc[t][r];
        } else {
          out[(size_t)blockIdx.x * (PB * 16 * QP) + row * QP + col] = acc[t][r];
        }
      }
    }
  }
}

// G[a][b] = sum over workgroups w = 0 .. nwg - 1 of partials[w][a][b], four interleaved chains in a fixed order
__global__ __launch_bounds__(kBlock) void eig_gram_reduce_kernel(const double* __restrict__ partials, int nwg, int p, int q,
                                                                 int QP, int blk_elems, double* __restrict__ g) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= p * q) return;
  const int a = idx / q, b = idx - a * q;
  const double* src = partials + a * QP + b;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int w = 0;
  for (; w + 3 < nwg; w += 4) {
    s0 += src[(size_t)w * blk_elems];
    s1 += src[(size_t)(w + 1) * blk_elems];
    s2 += src[(size_t)(w + 2) * blk_elems];
    s3 += src[(size_t)(w + 3) * blk_elems];
  }
  for (; w < nwg; ++w) s0 += src[(size_t)w * blk_elems];
  g[idx] = (s0 + s1) + (s2 + s3);
}

// --------------------------------------------------------------------------------------------
// out_b = sum_a coef[a][b] in_a for b < q on rows 0 .. nx - 1, as whole 16-byte vectors over columns [0, nyv).  The
//   coefficients sit in LDS, padded to QT columns; a thread carries one vector of every output (2 QT accumulators) while the
//   p inputs stream past once.  FMA chains in the order a = 0 .. p - 1.  `out` does not overlap `in`.  `coef` is row-major with
//   `qs` doubles per row: a launch forms q <= QT of its columns.
// --------------------------------------------------------------------------------------------
template <int QT>
__global__ __launch_bounds__(kBlock) void eig_combine_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                             const double* __restrict__ coef, int qs, int p, int q, int nx,
                                                             int nyv, int ld, long long col_stride) {
  __shared__ __attribute__((aligned(16))) double sc[kEigMaxP * QT];
  for (int i = threadIdx.x; i < p * QT; i += kBlock) {
    const int a = i / QT, b = i - a * QT;
    sc[i] = b < q ? coef[a * qs + b] : 0.0;
  }
  __syncthreads();
  const int vpr = nyv / 2;
  const long long total = (long long)nx * vpr;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int i = (int)(v / vpr), j = (int)(v % vpr) * 2;
    const size_t at = (size_t)i * ld + j;
    double acc0[QT], acc1[QT];
#pragma unroll
    for (int b = 0; b < QT; ++b) { acc0[b] = 0.0; acc1[b] = 0.0; }
#pragma unroll 2
    for (int a = 0; a < p; ++a) {
      const Pack<double> x = ldg(in + (long long)a * col_stride + at);
#pragma unroll
      for (int b = 0; b < QT; b += 2) {
        const Pack<double> c = *reinterpret_cast<const Pack<double>*>(sc + a * QT + b);
        acc0[b] = __builtin_fma(c.v[0], x.v[0], acc0[b]);
        acc1[b] = __builtin_fma(c.v[0], x.v[1], acc1[b]);
        acc0[b + 1] = __builtin_fma(c.v[1], x.v[0], acc0[b + 1]);
        acc1[b + 1] = __builtin_fma(c.v[1], x.v[1], acc1[b + 1]);
      }
    }
#pragma unroll
    for (int b = 0; b < QT; ++b) {
      if (b < q) {
        Pack<double> o;
        o.v[0] = acc0[b]; o.v[1] = acc1[b];
        stg(out + (long long)b * col_stride + at, o);
      }
    }
  }
}

// --------------------------------------------------------------------------------------------
// av_c = A v_c on interior cells, 0 on the ring, column c = blockIdx.z: pcg_direction_kernel's q with beta == nullptr and no
//   shift (only interior cells of v are read), the same bits per cell.
//   Stored: exactly the cells [0, nx) x [0, ny) of av.
// --------------------------------------------------------------------------------------------
template <bool VAR>
__global__ __launch_bounds__(kBlock) void eig_apply_kernel(const double* __restrict__ v_all, double* __restrict__ av_all,
                                                           const double* __restrict__ a, long long col_stride, TileGeom g,
                                                           double ihx2, double ihy2, double diag, double coeff) {
  using S = TileShape<double>;
  __shared__ __attribute__((aligned(16))) double s[S::LDS_ELEMS];
  __shared__ __attribute__((aligned(16))) double sa[VAR ? S::LDS_ELEMS : S::N];
  const double* __restrict__ z = v_all + (long long)blockIdx.z * col_stride;
  double* __restrict__ q = av_all + (long long)blockIdx.z * col_stride;
  const TileAt t = tile_at(g);

  stage_tile_map(s, t, g, [&](int gi, int gj) { return direction_pack(z, nullptr, 0.0, gi, gj, g); });
  if (VAR) stage_tile<double>(a, sa, t.i0, t.j0, g.nx, g.nyv, g.ld);
  __syncthreads();

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
      const double au = coeff * lap5<VAR>(u, ar, e, ihx2, ihy2, diag, 0.0);
      const int gj = t.gj0 + e;
      const bool interior = row_in && gj >= 1 && gj < g.ny - 1;
      o.v[e] = interior ? au : 0.0;
    }
    if (gi < g.nx) store_cells<false>(q, o, gi, t.gj0, g);
  }
}

// r_c = ax_c - lambda_c x_c on interior cells, 0 on the ring and on pad cells below nyv (rows 0 .. nx - 1 are stored as whole
// 16-byte vectors), and the partials of sum r_c^2: partials[c * gridDim.x + blockIdx.x], column c = blockIdx.z.
__global__ __launch_bounds__(kBlock) void eig_residual_kernel(const double* __restrict__ x_all, const double* __restrict__ ax_all,
                                                              const double* __restrict__ lambda, double* __restrict__ r_all,
                                                              double* __restrict__ partials, int nx, int ny, int nyv, int ld,
                                                              long long col_stride) {
  __shared__ double red[kBlock / 64];
  const int c = blockIdx.z;
  const double lam = lambda[c];
  const double* __restrict__ x = x_all + (long long)c * col_stride;
  const double* __restrict__ ax = ax_all + (long long)c * col_stride;
  double* __restrict__ r = r_all + (long long)c * col_stride;
  const int vpr = nyv / 2;
  const long long total = (long long)nx * vpr;
  double acc = 0.0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int i = (int)(v / vpr), j = (int)(v % vpr) * 2;
    const size_t at = (size_t)i * ld + j;
    Pack<double> o = zero_pack<double>();
    if (i >= 1 && i < nx - 1) {
      const Pack<double> xx = ldg(x + at), aa = ldg(ax + at);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (j + e >= 1 && j + e < ny - 1) {
          o.v[e] = aa.v[e] - lam * xx.v[e];
          acc += o.v[e] * o.v[e];
        }
      }
    }
    stg(r + at, o);
  }
  const double t = block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[(size_t)c * gridDim.x + blockIdx.x] = t;
}

// out[c] = sum of partials[c * n .. c * n + n - 1] in a fixed order; one workgroup per column
__global__ __launch_bounds__(kBlock) void eig_reduce_cols_kernel(const double* __restrict__ partials, int n, double* __restrict__ out) {
  __shared__ double red[kBlock / 64];
  const double* src = partials + (size_t)blockIdx.x * n;
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) a += src[i];
  const double t = block_reduce_sum(a, red);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// the boundary ring of column blockIdx.z := 0 (the caller's start vectors)
__global__ __launch_bounds__(kBlock) void eig_zero_ring_kernel(double* __restrict__ v_all, int nx, int ny, int ld, long long col_stride) {
  double* r = v_all + (long long)blockIdx.z * col_stride;
  const int n = 2 * ny + 2 * nx;
  for (int t = blockIdx.x * kBlock + threadIdx.x; t < n; t += gridDim.x * kBlock) {
    int i, j;
    ring_cell(t, nx, ny, i, j);
    r[(size_t)i * ld + j] = 0.0;
  }
}

}  // namespace mg
