// Zebra line relaxation (MG_ZEBRA_X / MG_ZEBRA_Y): one colour pass = one launch of line_colour_kernel<T, DIR>.
//
// Every line of the colour solves tridiag(-w, D, -w) x = b, b = rhs + c (u_prev_line + u_next_line) (+ w * ring value at the
// two ends), and is relaxed as u += omega (x - u).  All lines of a level share the Toeplitz matrix, so everything that is
// factored is a table (mg_line.hip builds it in long double on the host and rounds it once to T).
//
// A line is cut into periods of 32 cells: a chunk of 31 cells and one separator (the last period is a chunk of 1 .. 32 cells
// without a separator).  A workgroup owns G whole lines in LDS and runs, with one thread per (line, period):
//   stage   b, assembled from coalesced 16-byte loads, into the line buffers (33 LDS cells per period: lanes of consecutive
//           periods hit distinct banks);
//   A       per chunk  w yf = VL . b  and  w yl = reverse(VL) . b : w times the first / last entry of the chunk's zero-boundary
//           solution, VL = w T_31^-1 e_0 (all weights positive: the sums are well conditioned);
//   B       per line the Schur complement on the separators,
//             (D - w VL[0] - w VL'[0]) s_q - w VL[30] (s_q-1 + s_q+1) = b_sq + w yl_q + w yf_q+1,
//           by the Thomas recurrences with tabulated pivots (one lane per line; K - 1 <= a few hundred steps);
//   C       per chunk the Thomas solve with w s folded into the first / last right-hand side (componentwise backward stable:
//           no superposition of spikes, whose cancellation near a zero crossing of x costs tens of eps);
//   R, E    one refinement of the separators: r_q = b_sq + w (x_last + x_first) - D s_q from the chunk solutions as computed,
//           the same Schur solve for ds, s += ds, x += ds_left VL + ds_right reverse(VL).  The corrections are O(100 eps) of
//           x, so their own rounding is invisible, and the separator rows end as consistent as the chunk rows (A .. C alone
//           leave them at 5 .. 18 eps of |T||x| + |b|; with the refinement every row stays below 1.3);
//   store   u += omega (x - u) (omega == 1: x itself) as whole 16-byte vectors; ring and pad entries are written back with the bits they held.
// Y lines (fixed i, contiguous j): a vector belongs to one line.  X lines (fixed j): a vector holds the lines of both colours,
// a workgroup owns G / LV adjacent vectors of every row.  Fixed order everywhere: same bits on every run.
#pragma once

#include <hip/hip_runtime.h>

namespace mgl {

constexpr int kDirX = 0, kDirY = 1;
constexpr int kPeriod = 32, kChunk = 31, kCells = 33;   // cells per period; chunk length; LDS cells per period
constexpr int kThreads = 256;
// table block (elements of T): reciprocal pivots g, multipliers m = w g, spikes VL (full chunk) and VT (last chunk), then the
// Schur recurrences' sg[K - 1], sm[K - 1]
constexpr int kTabG = 0, kTabM = 32, kTabVL = 64, kTabVT = 96, kTabS = 128;

template <typename T> struct VecOf;
template <> struct VecOf<double> { using type = double2; static constexpr int N = 2; };
template <> struct VecOf<float> { using type = float4; static constexpr int N = 4; };

template <typename T> struct LineArgs {
  T* u;
  const T* rhs;
  const T* tab;
  int nx, ny, ld;
  int n, K, mt;        // cells per line, periods per line, cells of the last chunk (1 .. 32)
  int G, LS;           // lines per workgroup, LDS cells per line buffer
  int colour, count;   // Y: lines of this colour; X: 16-byte vectors per row
  T w, c, D, e, omega;
};

template <typename T, int DIR>
__global__ __launch_bounds__(kThreads) void line_colour_kernel(const LineArgs<T> a) {
  using V = typename VecOf<T>::type;
  constexpr int N = VecOf<T>::N, LV = N / 2;
  union Pack { V v; T e[N]; };
  extern __shared__ __align__(16) unsigned char line_lds[];
  T* B = reinterpret_cast<T*>(line_lds);          // [G][LS]  b, then x
  T* RF = B + (size_t)a.G * a.LS;                 // [G][K]   w yf, then ds
  T* RL = RF + (size_t)a.G * a.K;                 // [G][K]   w yl, then s
  const int tid = threadIdx.x, K = a.K, G = a.G, LS = a.LS, ld = a.ld;
  const T w = a.w, c = a.c;
  const T* __restrict__ tab = a.tab;
  const int first = a.colour ? 1 : 2;             // Y: first row of the colour
  const int GV = G / LV;                          // X: vectors per workgroup
  auto valid = [&](int l) {
    if (DIR == kDirY) return blockIdx.x * G + l < a.count;
    const int pv = blockIdx.x * GV + l / LV, j = pv * N + a.colour + 2 * (l % LV);
    return pv < a.count && j >= 1 && j <= a.ny - 2;
  };

  // ---- stage: b into the line buffers ----------------------------------------------------------------------------------
  if (DIR == kDirY) {
    const int nvec = (a.ny + N - 1) / N;
    for (int idx = tid; idx < G * nvec; idx += kThreads) {
      const int l = idx / nvec, v = idx - l * nvec;
      if (!valid(l)) continue;
      const size_t row = (size_t)(first + 2 * (blockIdx.x * G + l)) * ld;
      const int j0 = v * N;
      Pack f, up, dn;
      f.v = *reinterpret_cast<const V*>(a.rhs + row + j0);
      up.v = *reinterpret_cast<const V*>(a.u + row - ld + j0);
      dn.v = *reinterpret_cast<const V*>(a.u + row + ld + j0);
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const int j = j0 + q;
        if (j < 1 || j > a.ny - 2) continue;
        T b = f.e[q] + c * (up.e[q] + dn.e[q]);
        if (j == 1) b += w * a.u[row];
        if (j == a.ny - 2) b += w * a.u[row + a.ny - 1];
        const int cell = j - 1;
        B[l * LS + cell + cell / kPeriod] = b;
      }
    }
  } else {
    for (int idx = tid; idx < (a.nx - 2) * GV; idx += kThreads) {
      const int ii = idx / GV, v = idx - ii * GV, pv = blockIdx.x * GV + v;
      if (pv >= a.count) continue;
      const int j0 = pv * N;
      const size_t row = (size_t)(ii + 1) * ld;
      Pack f, uu;
      f.v = *reinterpret_cast<const V*>(a.rhs + row + j0);
      uu.v = *reinterpret_cast<const V*>(a.u + row + j0);
      T ext = 0;                                   // the neighbour that lives in the adjacent vector
      if (a.colour == 0) { if (j0 > 0) ext = a.u[row + j0 - 1]; }
      else if (j0 + N < a.ny) ext = a.u[row + j0 + N];
#pragma unroll
      for (int q = 0; q < LV; ++q) {
        const int j = j0 + a.colour + 2 * q;
        if (j < 1 || j > a.ny - 2) continue;
        // compile-time vector indices only (q is unrolled): a runtime index would put the vector in scratch
        const T fe = a.colour ? f.e[2 * q + 1] : f.e[2 * q];
        const T left = a.colour ? uu.e[2 * q] : (q == 0 ? ext : uu.e[q == 0 ? 0 : 2 * q - 1]);
        const T right = a.colour ? (q == LV - 1 ? ext : uu.e[q == LV - 1 ? 0 : 2 * q + 2]) : uu.e[2 * q + 1];
        T b = fe + c * (left + right);
        if (ii == 0) b += w * a.u[j];
        if (ii == a.nx - 3) b += w * a.u[(size_t)(a.nx - 1) * ld + j];
        B[(v * LV + q) * LS + ii + ii / kPeriod] = b;
      }
    }
  }
  __syncthreads();

  // one Schur solve per line, lanes 0 .. G - 1: forward and backward Thomas recurrences in place on x[0 .. K - 2]
  auto schur = [&](T* x) {
    T acc = 0;
    for (int q = 0; q < K - 1; ++q) { acc = (x[q] + a.e * acc) * tab[kTabS + q]; x[q] = acc; }
    acc = 0;
    for (int q = K - 2; q >= 0; --q) { acc = x[q] + tab[kTabS + (K - 1) + q] * acc; x[q] = acc; }
  };

  if (K > 1) {
    // ---- A: w yf, w yl of every chunk ------------------------------------------------------------------------------------
    for (int it = tid; it < G * K; it += kThreads) {
      const int l = it / K, k = it - l * K;
      if (!valid(l)) continue;
      const bool full = k < K - 1;
      const int len = full ? kChunk : a.mt;
      const T* Bp = B + l * LS + k * kCells;
      T wyf = 0, wyl = 0;
#pragma unroll
      for (int t = 0; t < kPeriod; ++t) {
        if (t >= len) continue;
        const T bt = Bp[t];
        const T vl = tab[kTabVL + (t < kChunk ? t : 0)], vt = tab[kTabVT + t];
        wyf += (full ? vl : vt) * bt;
        if (t < kChunk) wyl += tab[kTabVL + (kChunk - 1 - t < 0 ? 0 : kChunk - 1 - t)] * bt;
      }
      RF[l * K + k] = wyf;
      RL[l * K + k] = wyl;
    }
    __syncthreads();
    // ---- B: separators ---------------------------------------------------------------------------------------------------
    if (tid < G && valid(tid)) {
      T* S = RL + tid * K;
      const T* F = RF + tid * K;
      const T* Bl = B + tid * LS;
      for (int q = 0; q < K - 1; ++q) S[q] = Bl[q * kCells + kChunk] + (S[q] + F[q + 1]);
      schur(S);
    }
    __syncthreads();
  }

  // ---- C: chunk solves with the separators folded in -----------------------------------------------------------------------
  for (int it = tid; it < G * K; it += kThreads) {
    const int l = it / K, k = it - l * K;
    if (!valid(l)) continue;
    const bool full = k < K - 1;
    const int len = full ? kChunk : a.mt;
    T* Bp = B + l * LS + k * kCells;
    const T sp = k > 0 ? RL[l * K + k - 1] : T(0), sn = full ? RL[l * K + k] : T(0);
    T y[kPeriod];
#pragma unroll
    for (int t = 0; t < kPeriod; ++t) {
      if (t >= len) continue;
      T bt = Bp[t];
      if (t == 0) bt += w * sp;
      if (t == len - 1 && full) bt += w * sn;
      y[t] = t == 0 ? bt * tab[kTabG] : (bt + w * y[t > 0 ? t - 1 : 0]) * tab[kTabG + t];
    }
    T xn = 0;
#pragma unroll
    for (int t = kPeriod - 1; t >= 0; --t) {
      if (t >= len) continue;
      xn = t == len - 1 ? y[t] : y[t] + tab[kTabM + t] * xn;
      Bp[t] = xn;
    }
  }
  __syncthreads();

  if (K > 1) {
    // ---- R: refine the separators against the chunk solutions as computed --------------------------------------------------
    if (tid < G && valid(tid)) {
      T* S = RL + tid * K;
      T* dS = RF + tid * K;
      const T* Bl = B + tid * LS;
      for (int q = 0; q < K - 1; ++q)
        dS[q] = (Bl[q * kCells + kChunk] + w * (Bl[q * kCells + kChunk - 1] + Bl[(q + 1) * kCells])) - a.D * S[q];
      schur(dS);
      for (int q = 0; q < K - 1; ++q) S[q] += dS[q];
    }
    __syncthreads();
    // ---- E: spikes of the correction; the separator cell takes its value ----------------------------------------------------
    for (int it = tid; it < G * K; it += kThreads) {
      const int l = it / K, k = it - l * K;
      if (!valid(l)) continue;
      const bool full = k < K - 1;
      const int len = full ? kChunk : a.mt;
      T* Bp = B + l * LS + k * kCells;
      const T dp = k > 0 ? RF[l * K + k - 1] : T(0), dn = full ? RF[l * K + k] : T(0);
#pragma unroll
      for (int t = 0; t < kPeriod; ++t) {
        if (t >= len) continue;
        T corr = 0;
        if (k > 0) corr = dp * (full ? tab[kTabVL + (t < kChunk ? t : 0)] : tab[kTabVT + t]);
        if (full) corr += dn * tab[kTabVL + (kChunk - 1 - t < 0 ? 0 : kChunk - 1 - t)];
        Bp[t] += corr;
      }
      if (full) Bp[kChunk] = RL[l * K + k];
    }
    __syncthreads();
  }

  // omega == 1 stores x itself: u + (x - u) would round once more, by up to eps |u| where x passes through zero
  const bool unit = a.omega == T(1);
  auto relax = [&](T old, T x) { return unit ? x : old + a.omega * (x - old); };
  // ---- store ---------------------------------------------------------------------------------------------------------------
  if (DIR == kDirY) {
    const int nvec = (a.ny + N - 1) / N;
    for (int idx = tid; idx < G * nvec; idx += kThreads) {
      const int l = idx / nvec, v = idx - l * nvec;
      if (!valid(l)) continue;
      const size_t row = (size_t)(first + 2 * (blockIdx.x * G + l)) * ld;
      const int j0 = v * N;
      Pack o;
      o.v = *reinterpret_cast<const V*>(a.u + row + j0);
#pragma unroll
      for (int q = 0; q < N; ++q) {
        const int j = j0 + q;
        if (j < 1 || j > a.ny - 2) continue;
        const int cell = j - 1;
        o.e[q] = relax(o.e[q], B[l * LS + cell + cell / kPeriod]);
      }
      *reinterpret_cast<V*>(a.u + row + j0) = o.v;
    }
  } else {
    for (int idx = tid; idx < (a.nx - 2) * GV; idx += kThreads) {
      const int ii = idx / GV, v = idx - ii * GV, pv = blockIdx.x * GV + v;
      if (pv >= a.count) continue;
      const int j0 = pv * N;
      const size_t row = (size_t)(ii + 1) * ld;
      Pack o;
      o.v = *reinterpret_cast<const V*>(a.u + row + j0);
      bool any = false;
#pragma unroll
      for (int q = 0; q < LV; ++q) {
        const int j = j0 + a.colour + 2 * q;
        if (j < 1 || j > a.ny - 2) continue;
        any = true;
        const T x = B[(v * LV + q) * LS + ii + ii / kPeriod];
        if (a.colour) o.e[2 * q + 1] = relax(o.e[2 * q + 1], x);
        else o.e[2 * q] = relax(o.e[2 * q], x);
      }
      if (any) *reinterpret_cast<V*>(a.u + row + j0) = o.v;
    }
  }
}

}  // namespace mgl
