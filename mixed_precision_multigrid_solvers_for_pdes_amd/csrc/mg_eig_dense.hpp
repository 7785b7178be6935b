// Small dense symmetric routines of the block eigensolver (mg_eig.hip), host only: plain C++ on row-major arrays, no HIP, no
// external LAPACK.  n <= kMaxN = 48 (three blocks of 16 columns); all work arrays are on the stack.
//   cholesky            G = L L^T in place (lower triangle); false on a non-positive or non-finite pivot
//   chol_orth_transform T = D^-1/2 L^-T with D = diag(G), L L^T = D^-1/2 G D^-1/2: U T has orthonormal columns when G = U^T U
//   jacobi_eigh         cyclic Jacobi: A = V diag(w) V^T, w ascending
//   ritz                lowest m eigenpairs of G_A c = lambda G_B c with C^T G_B C = I
#pragma once

#include <cmath>

namespace mgd {

constexpr int kMaxN = 48;

inline bool cholesky(int n, double* a, int lda) {
  for (int j = 0; j < n; ++j) {
    double d = a[j * lda + j];
    for (int k = 0; k < j; ++k) d -= a[j * lda + k] * a[j * lda + k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double l = std::sqrt(d);
    a[j * lda + j] = l;
    for (int i = j + 1; i < n; ++i) {
      double s = a[i * lda + j];
      for (int k = 0; k < j; ++k) s -= a[i * lda + k] * a[j * lda + k];
      a[i * lda + j] = s / l;
    }
  }
  return true;
}

// x := L^-1 x for the lower-triangular L (n x n, pitch lda); x is a vector with stride incx
inline void forward_solve(int n, const double* l, int lda, double* x, int incx) {
  for (int i = 0; i < n; ++i) {
    double s = x[i * incx];
    for (int k = 0; k < i; ++k) s -= l[i * lda + k] * x[k * incx];
    x[i * incx] = s / l[i * lda + i];
  }
}

// x := L^-T x
inline void backward_solve_t(int n, const double* l, int lda, double* x, int incx) {
  for (int i = n - 1; i >= 0; --i) {
    double s = x[i * incx];
    for (int k = i + 1; k < n; ++k) s -= l[k * lda + i] * x[k * incx];
    x[i * incx] = s / l[i * lda + i];
  }
}

// g: n x n Gram matrix (only its lower triangle and diagonal are read); t: n x n, upper triangular on return
inline bool chol_orth_transform(int n, const double* g, double* t) {
  if (n < 1 || n > kMaxN) return false;
  double l[kMaxN * kMaxN], dm[kMaxN];
  for (int i = 0; i < n; ++i) {
    const double d = g[i * n + i];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    dm[i] = 1.0 / std::sqrt(d);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) l[i * n + j] = g[i * n + j] * dm[i] * dm[j];
  if (!cholesky(n, l, n)) return false;
  for (int j = 0; j < n; ++j) {                     // column j of L^-1 by forward substitution on e_j, stored as row j of L^-T
    double col[kMaxN];
    for (int i = 0; i < n; ++i) col[i] = (i == j) ? 1.0 : 0.0;
    forward_solve(n, l, n, col, 1);
    for (int i = 0; i < n; ++i) t[j * n + i] = (i >= j) ? dm[j] * col[i] : 0.0;
  }
  return true;
}

// a: n x n symmetric (destroyed); v: n x n, column k is the eigenvector of w[k]; w ascending
inline void jacobi_eigh(int n, double* a, double* v, double* w) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) v[i * n + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) off += std::fabs(a[i * n + j]);
    if (off == 0.0) break;
    for (int p = 0; p < n - 1; ++p) {
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[p * n + q];
        if (apq == 0.0) continue;
        const double g = 100.0 * std::fabs(apq);
        if (sweep > 3 && std::fabs(a[p * n + p]) + g == std::fabs(a[p * n + p]) && std::fabs(a[q * n + q]) + g == std::fabs(a[q * n + q])) {
          a[p * n + q] = a[q * n + p] = 0.0;
          continue;
        }
        const double theta = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {               // A := A J
          const double akp = a[k * n + p], akq = a[k * n + q];
          a[k * n + p] = c * akp - s * akq;
          a[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {               // A := J^T A
          const double apk = a[p * n + k], aqk = a[q * n + k];
          a[p * n + k] = c * apk - s * aqk;
          a[q * n + k] = s * apk + c * aqk;
        }
        a[p * n + q] = a[q * n + p] = 0.0;
        for (int k = 0; k < n; ++k) {
          const double vkp = v[k * n + p], vkq = v[k * n + q];
          v[k * n + p] = c * vkp - s * vkq;
          v[k * n + q] = s * vkp + c * vkq;
        }
      }
    }
  }
  for (int i = 0; i < n; ++i) w[i] = a[i * n + i];
  for (int i = 0; i < n - 1; ++i) {                  // selection sort, columns of v follow
    int k = i;
    for (int j = i + 1; j < n; ++j)
      if (w[j] < w[k]) k = j;
    if (k != i) {
      const double tw = w[i]; w[i] = w[k]; w[k] = tw;
      for (int r = 0; r < n; ++r) { const double tv = v[r * n + i]; v[r * n + i] = v[r * n + k]; v[r * n + k] = tv; }
    }
  }
}

// ga, gb: n x n (symmetrised here); evals: m; coef: n x m row-major.  0, or 1 when G_B is not positive definite.
inline int ritz(int n, int m, const double* ga, const double* gb, double* evals, double* coef) {
  if (n < 1 || n > kMaxN || m < 1 || m > n) return -1;
  double l[kMaxN * kMaxN], a[kMaxN * kMaxN], v[kMaxN * kMaxN], w[kMaxN];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      l[i * n + j] = 0.5 * (gb[i * n + j] + gb[j * n + i]);
      a[i * n + j] = a[j * n + i] = 0.5 * (ga[i * n + j] + ga[j * n + i]);
    }
  if (!cholesky(n, l, n)) return 1;
  for (int j = 0; j < n; ++j) forward_solve(n, l, n, a + j, n);          // A := L^-1 A, column by column
  for (int i = 0; i < n; ++i) forward_solve(n, l, n, a + i * n, 1);      // A := A L^-T, row by row
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < i; ++j) a[i * n + j] = a[j * n + i] = 0.5 * (a[i * n + j] + a[j * n + i]);
  jacobi_eigh(n, a, v, w);
  for (int k = 0; k < m; ++k) {
    double col[kMaxN];
    for (int i = 0; i < n; ++i) col[i] = v[i * n + k];
    backward_solve_t(n, l, n, col, 1);
    for (int i = 0; i < n; ++i) coef[i * m + k] = col[i];
    evals[k] = w[k];
  }
  return 0;
}

}  // namespace mgd
