// Kernels of the 3-D multigrid family (include/mghip_3d.h states the layout and the association of every formula; nothing here
// may round differently).  Cell (i, j, k) sits at (i * ny + j) * ld + k, k fastest.
//
// The hot kernels -- Jacobi sweep, colour pass, residual -- are one template, mg3_sweep_kernel.  A workgroup of 256 threads owns
// a (j, k) tile of kT3J rows x kT3RowBytes bytes and a chunk of kT3I planes along i, and marches along i: thread (tj, tv) holds
// one 16-byte vector of row j0 + tj.  The planes i-1, i and i+1 of its own column roll through registers (the load of plane
// i+1 is issued before plane i is staged); plane i goes to LDS with a one-cell halo, from which the j-1 / j+1 vectors and the
// two k neighbours outside the thread's own vector are read.  Per chunk every cell of u is read from HBM once, plus the halo
// (the (kT3J + 2)(TK + 2) / (kT3J TK) - 1 of the tile, and 2 planes per kT3I for the chunk).  The i axis is chunked so that a
// 257^3 level gives 17 x 9 x 8 = 1224 workgroups (fp64) where the (j, k) tiles alone would give 153.
//
// Every sum is per-workgroup partials (block_reduce_sum) followed by reduce_partials_kernel: no atomics, the same bits on every
// run.  The transfers, the up-cast add, the copy and the norm are grid-stride kernels; the coarsest solve keeps u and f in LDS.
#pragma once

#include "mg_kernels.hpp"

namespace mg3 {

using mg::Pack;
using mg::VecW;
using mg::kBlock;

constexpr int kT3J = 16;            // tile rows (j)
constexpr int kT3RowBytes = 256;    // bytes of one tile row along k (32 fp64 / 64 fp32: 16 vectors)
constexpr int kT3I = 32;            // planes of one i chunk
constexpr int kM3Jacobi = 0, kM3Colour = 1, kM3Residual = 2;
constexpr int kCoarseLdsExtent = 17;                  // the coarsest solve runs in LDS when no extent exceeds this
constexpr int kCoarseLdsBlock = 1024;
constexpr int kNormBlocks = 1024;                     // workgroups of mg3_sumsq_kernel at most

template <typename T> struct Tile3 {
  static constexpr int N = VecW<T>::N;
  static constexpr int TK = kT3RowBytes / (int)sizeof(T);     // tile columns (k)
  static constexpr int VK = TK / N;                           // vectors per tile row = 16
  static constexpr int SK = TK + 2 * N;                       // LDS row stride: one vector of halo on each side keeps rows aligned
  static constexpr int LDS_ELEMS = (kT3J + 2) * SK;
  static_assert(VK * kT3J == kBlock, "one vector per thread");
  static_assert(2 * TK + 2 * kT3J <= kBlock, "one halo cell per thread");
};

struct Geom3 {
  int nx, ny, nz, ld;               // extents and row pitch (elements)
  int ld_out;                       // row pitch of the output (differs for the fp32 residual of fp64 fields)
  int tiles_j, tiles_k, chunks;     // workgroups = tiles_j * tiles_k * chunks
};
template <typename T> struct Coef3 { T ihx2, ihy2, ihz2, diag, w; };

// The vector at row[kv]: one 16-byte load where the pitch keeps every row 16-byte aligned (ld a multiple of N: always for fp64,
// and for the engine's own pitch) and holds the vector whole, else the elements below nz one by one (zeros above).  The choice
// is uniform over a launch.
template <typename T> __device__ __forceinline__ Pack<T> load_vec(const T* row, int kv, int nz, int ld) {
  constexpr int N = VecW<T>::N;
  if (ld % N == 0 && kv + N <= ld) return mg::ldg(row + kv);
  Pack<T> p = mg::zero_pack<T>();
#pragma unroll
  for (int e = 0; e < N; ++e)
    if (kv + e < nz) p.v[e] = row[kv + e];
  return p;
}
// Store the elements of p at row[kv ..] whose k lies in [k_lo, k_hi): one 16-byte store when that is all of them and the rows
// are 16-byte aligned
template <typename TO, typename T> __device__ __forceinline__ void store_vec(TO* row, int kv, const Pack<T>& p, int k_lo, int k_hi, int ld) {
  constexpr int N = VecW<T>::N;
  if constexpr (std::is_same_v<TO, T>) {
    if (ld % N == 0 && kv >= k_lo && kv + N <= k_hi) { mg::stg(row + kv, p); return; }
  }
#pragma unroll
  for (int e = 0; e < N; ++e)
    if (kv + e >= k_lo && kv + e < k_hi) row[kv + e] = (TO)p.v[e];
}

// MODE kM3Jacobi: out = u + w r (out of place).  kM3Colour: the same in place (out == u) on the cells with ((i + j + k) & 1) ==
// colour_par.  kM3Residual: out = r when WRITE, partials[workgroup] = sum r^2 when NORM.  Interior cells only.
template <typename T, typename TR, int MODE, bool WRITE, bool NORM>
__global__ __launch_bounds__(kBlock) void mg3_sweep_kernel(const T* u, const T* __restrict__ f, TR* out, double* __restrict__ partials,
                                                           Geom3 g, Coef3<T> c, int colour_par) {
  using S = Tile3<T>;
  constexpr int N = S::N;
  __shared__ __attribute__((aligned(16))) T s[S::LDS_ELEMS];
  __shared__ double red[kBlock / 64];
  const int b = blockIdx.x;
  const int tile_k = b % g.tiles_k, tile_j = (b / g.tiles_k) % g.tiles_j, chunk = b / (g.tiles_k * g.tiles_j);
  const int j0 = tile_j * kT3J, k0 = tile_k * S::TK;
  const int t = threadIdx.x, tj = t / S::VK, tv = t - tj * S::VK;
  const int j = j0 + tj, kv = k0 + tv * N;
  const int i_lo = 1 + chunk * kT3I, i_hi = min(i_lo + kT3I, g.nx - 1);
  const size_t plane = (size_t)g.ny * g.ld, plane_out = (size_t)g.ny * g.ld_out;
  const bool valid = j < g.ny && kv < g.nz;
  const bool row_interior = j >= 1 && j < g.ny - 1;
  const size_t row = (size_t)j * g.ld;

  // the halo cell this thread brings (one per thread; h_lds < 0: none)
  int h_lds = -1;
  size_t h_off = 0;
  {
    int jj = 0, kk = 0, l = -1;
    if (t < S::TK) { jj = j0 - 1; kk = k0 + t; l = N + t; }
    else if (t < 2 * S::TK) { jj = j0 + kT3J; kk = k0 + t - S::TK; l = (kT3J + 1) * S::SK + N + (t - S::TK); }
    else if (t < 2 * S::TK + kT3J) { jj = j0 + (t - 2 * S::TK); kk = k0 - 1; l = (t - 2 * S::TK + 1) * S::SK + N - 1; }
    else if (t < 2 * S::TK + 2 * kT3J) { jj = j0 + (t - 2 * S::TK - kT3J); kk = k0 + S::TK; l = (t - 2 * S::TK - kT3J + 1) * S::SK + N + S::TK; }
    if (l >= 0 && jj >= 0 && jj < g.ny && kk >= 0 && kk < g.nz) { h_lds = l; h_off = (size_t)jj * g.ld + kk; }
  }

  Pack<T> prev = mg::zero_pack<T>(), cur = prev;
  T hv = T(0);
  if (i_lo < i_hi) {
    if (valid) {
      prev = load_vec(u + (size_t)(i_lo - 1) * plane + row, kv, g.nz, g.ld);
      cur = load_vec(u + (size_t)i_lo * plane + row, kv, g.nz, g.ld);
    }
    if (h_lds >= 0) hv = u[(size_t)i_lo * plane + h_off];
  }
  double acc = 0.0;
  T* mine = s + (tj + 1) * S::SK + N + tv * N;
  for (int i = i_lo; i < i_hi; ++i) {
    Pack<T> nxt = mg::zero_pack<T>(), fv = nxt;
    if (valid) {
      nxt = load_vec(u + (size_t)(i + 1) * plane + row, kv, g.nz, g.ld);
      fv = load_vec(f + (size_t)i * plane + row, kv, g.nz, g.ld);
    }
    T hn = T(0);
    if (h_lds >= 0 && i + 1 < i_hi) hn = u[(size_t)(i + 1) * plane + h_off];
    __syncthreads();                                   // the reads of the plane before are done
    *reinterpret_cast<Pack<T>*>(mine) = cur;
    if (h_lds >= 0) s[h_lds] = hv;
    __syncthreads();
    if (valid && row_interior) {
      const Pack<T> jm = *reinterpret_cast<const Pack<T>*>(mine - S::SK), jp = *reinterpret_cast<const Pack<T>*>(mine + S::SK);
      const T left = mine[-1], right = mine[N];
      Pack<T> o;
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const int k = kv + e;
        const T km = e > 0 ? cur.v[e - 1] : left, kp = e < N - 1 ? cur.v[e + 1] : right;
        const T nb = ((c.ihx2 * (prev.v[e] + nxt.v[e])) + (c.ihy2 * (jm.v[e] + jp.v[e]))) + (c.ihz2 * (km + kp));
        const T r = fv.v[e] - (c.diag * cur.v[e] - nb);
        const bool interior = k >= 1 && k < g.nz - 1;
        if (MODE == kM3Residual) {
          o.v[e] = r;
          if (NORM && interior) acc += (double)r * (double)r;
        } else {
          const T un = cur.v[e] + c.w * r;
          o.v[e] = (MODE == kM3Jacobi || ((i + j + k) & 1) == colour_par) ? un : cur.v[e];
        }
      }
      if (WRITE) store_vec(out + (size_t)i * plane_out + (size_t)j * g.ld_out, kv, o, 1, g.nz - 1, g.ld_out);
    }
    prev = cur; cur = nxt; hv = hn;
  }
  if (NORM) {
    const double tot = mg::block_reduce_sum(acc, red);
    if (t == 0) partials[b] = tot;
  }
}

template <typename T> __device__ __forceinline__ T fw1(T a, T b, T c) { return T(0.5) * b + T(0.25) * (a + c); }

// 27-point full weighting, one interior coarse cell per thread (consecutive threads along K): along k, then j, then i
template <typename T>
__global__ __launch_bounds__(kBlock) void mg3_restrict_kernel(const T* __restrict__ fine, T* __restrict__ coarse, int nxc, int nyc,
                                                              int nzc, int nyf, int ldf, int ldc) {
  const int mk = nzc - 2, mj = nyc - 2;
  const long long total = (long long)(nxc - 2) * mj * mk;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int K = 1 + (int)(v % mk), J = 1 + (int)((v / mk) % mj), I = 1 + (int)(v / ((long long)mk * mj));
    T q[3];
#pragma unroll
    for (int di = 0; di < 3; ++di) {
      T p[3];
#pragma unroll
      for (int dj = 0; dj < 3; ++dj) {
        const T* row = fine + ((size_t)(2 * I - 1 + di) * nyf + (2 * J - 1 + dj)) * ldf + 2 * K;
        p[dj] = fw1(row[-1], row[0], row[1]);
      }
      q[di] = fw1(p[0], p[1], p[2]);
    }
    coarse[((size_t)I * nyc + J) * ldc + K] = fw1(q[0], q[1], q[2]);
  }
}

// u += P e on interior fine cells: one vector of an interior row per thread; the averages along k, then j, then i
template <typename T>
__global__ __launch_bounds__(kBlock) void mg3_prolong_add_kernel(const T* __restrict__ e, T* __restrict__ u, int nx, int ny, int nz,
                                                                 int ldf, int nyc, int ldc) {
  constexpr int N = VecW<T>::N;
  const int vpr = (nz + N - 1) / N, mj = ny - 2;
  const long long total = (long long)(nx - 2) * mj * vpr;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int kv = (int)(v % vpr) * N, j = 1 + (int)((v / vpr) % mj), i = 1 + (int)(v / ((long long)vpr * mj));
    T* row = u + ((size_t)i * ny + j) * ldf;
    Pack<T> p = load_vec(row, kv, nz, ldf);
    const int I = i >> 1, J = j >> 1;
    const bool iodd = i & 1, jodd = j & 1;
#pragma unroll
    for (int x = 0; x < N; ++x) {
      const int k = kv + x;
      if (k < 1 || k >= nz - 1) continue;
      const int K = k >> 1;
      const bool kodd = k & 1;
      auto ek = [&](int Ip, int Jp) {
        const T* cr = e + ((size_t)Ip * nyc + Jp) * ldc;
        return kodd ? T(0.5) * (cr[K] + cr[K + 1]) : cr[K];
      };
      auto ej = [&](int Ip) { return jodd ? T(0.5) * (ek(Ip, J) + ek(Ip, J + 1)) : ek(Ip, J); };
      const T t = iodd ? T(0.5) * (ej(I) + ej(I + 1)) : ej(I);
      p.v[x] = p.v[x] + t;
    }
    store_vec(row, kv, p, 1, nz - 1, ldf);
  }
}

// u64 += (double)e32 on interior cells (the defect step)
__global__ __launch_bounds__(kBlock) void mg3_upcast_add_kernel(const float* __restrict__ e, double* __restrict__ u, int nx, int ny,
                                                                int nz, int ld64, int ld32) {
  constexpr int N = VecW<double>::N;
  const int vpr = (nz + N - 1) / N, mj = ny - 2;
  const long long total = (long long)(nx - 2) * mj * vpr;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const int kv = (int)(v % vpr) * N, j = 1 + (int)((v / vpr) % mj), i = 1 + (int)(v / ((long long)vpr * mj));
    double* row = u + ((size_t)i * ny + j) * ld64;
    const float* er = e + ((size_t)i * ny + j) * ld32;
    Pack<double> p = load_vec(row, kv, nz, ld64);
#pragma unroll
    for (int x = 0; x < N; ++x)
      if (kv + x >= 1 && kv + x < nz - 1) p.v[x] = p.v[x] + (double)er[kv + x];
    store_vec(row, kv, p, 1, nz - 1, ld64);
  }
}

// out = (TOUT)in on every cell of [0,nx) x [0,ny) x [0,nz): the hand-over of a caller's device array (any even pitch, either
// dtype) to the engine's field and back.  One element per thread, consecutive threads along k
template <typename TIN, typename TOUT>
__global__ __launch_bounds__(kBlock) void mg3_copy_kernel(const TIN* __restrict__ in, TOUT* __restrict__ out, long long rows, int nz,
                                                          int ld_in, int ld_out) {
  const long long total = rows * nz;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const long long r = v / nz;
    const int k = (int)(v - r * nz);
    out[(size_t)r * ld_out + k] = (TOUT)in[(size_t)r * ld_in + k];
  }
}

// partials[workgroup] = sum of x^2 over the workgroup's share of [0,nx) x [0,ny) x [0,nz) (rows = nx * ny); the grid is fixed by
// the shape alone, so the sum has the same bits on every run
template <typename T>
__global__ __launch_bounds__(kBlock) void mg3_sumsq_kernel(const T* __restrict__ x, double* __restrict__ partials, long long rows, int nz,
                                                           int ld) {
  constexpr int N = VecW<T>::N;
  __shared__ double red[kBlock / 64];
  const int vpr = (nz + N - 1) / N;
  const long long total = rows * vpr;
  double acc = 0.0;
  for (long long v = (long long)blockIdx.x * kBlock + threadIdx.x; v < total; v += (long long)gridDim.x * kBlock) {
    const long long r = v / vpr;
    const int kv = (int)(v - r * vpr) * N;
    const Pack<T> p = load_vec(x + (size_t)r * ld, kv, nz, ld);
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (kv + e < nz) acc += (double)p.v[e] * (double)p.v[e];
  }
  const double tot = mg::block_reduce_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// The coarsest solve: `sweeps` red-black sweeps (colour 0 then 1) in ONE workgroup with u and f in LDS (dense, nx * ny * nz
// each; the launcher sizes the dynamic LDS).  The update is the colour pass's, c.w = 1 / diag.
template <typename T>
__global__ __launch_bounds__(kCoarseLdsBlock) void mg3_coarse_lds_kernel(T* __restrict__ u, const T* __restrict__ f, int nx, int ny,
                                                                         int nz, int ld, Coef3<T> c, int sweeps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mg3_pool[];
  const int n = nx * ny * nz;
  T* su = reinterpret_cast<T*>(mg3_pool);
  T* sf = su + n;
  for (int v = threadIdx.x; v < n; v += kCoarseLdsBlock) {
    const int k = v % nz, r = v / nz;
    su[v] = u[(size_t)r * ld + k];
    sf[v] = f[(size_t)r * ld + k];
  }
  __syncthreads();
  const int mk = nz - 2, mj = ny - 2, ni = (nx - 2) * mj * mk;
  const int sj = nz, si = ny * nz;
  for (int sweep = 0; sweep < sweeps; ++sweep) {
    for (int colour = 0; colour < 2; ++colour) {
      for (int v = threadIdx.x; v < ni; v += kCoarseLdsBlock) {
        const int k = 1 + v % mk, j = 1 + (v / mk) % mj, i = 1 + v / (mk * mj);
        if (((i + j + k) & 1) != colour) continue;
        const int x = i * si + j * sj + k;
        const T nb = ((c.ihx2 * (su[x - si] + su[x + si])) + (c.ihy2 * (su[x - sj] + su[x + sj]))) + (c.ihz2 * (su[x - 1] + su[x + 1]));
        const T r = sf[x] - (c.diag * su[x] - nb);
        su[x] = su[x] + c.w * r;
      }
      __syncthreads();
    }
  }
  for (int v = threadIdx.x; v < ni; v += kCoarseLdsBlock) {
    const int k = 1 + v % mk, j = 1 + (v / mk) % mj, i = 1 + v / (mk * mj);
    u[((size_t)i * ny + j) * ld + k] = su[i * si + j * sj + k];
  }
}

}  // namespace mg3
