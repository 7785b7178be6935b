// Stand-alone check of the host-only dense routines of the block eigensolver (csrc/mg_eig_dense.hpp), meant to be built
// with -fsanitize=address,undefined and run on the CPU (tests/test_eig_cpu.py does): every routine at n = 1, 3, 18, 48 on
// deterministic pseudo-random symmetric positive definite pairs, plus the refusals.  Exit status 0: all checks passed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "mg_eig_dense.hpp"

namespace {
unsigned long long state = 88172645463325252ull;
double rnd() {                       // xorshift64, uniform in (-1, 1)
  state ^= state << 13; state ^= state >> 7; state ^= state << 17;
  return (double)(state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}
int failures = 0;
void expect(bool ok, const char* what, int n) {
  if (!ok) { std::printf("FAILED: %s (n = %d)\n", what, n); ++failures; }
}
// B^T B + shift I
std::vector<double> spd(int n, double shift) {
  std::vector<double> b(n * n), g(n * n);
  for (double& x : b) x = rnd();
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = i == j ? shift : 0.0;
      for (int k = 0; k < n; ++k) s += b[k * n + i] * b[k * n + j];
      g[i * n + j] = s;
    }
  return g;
}
}  // namespace

int main() {
  for (int n : {1, 3, 18, 48}) {
    const std::vector<double> ga = spd(n, 0.5), gb = spd(n, 1.0);
    const int m = n < 3 ? n : n / 3;
    std::vector<double> ev(m), c(n * m);
    expect(mgd::ritz(n, m, ga.data(), gb.data(), ev.data(), c.data()) == 0, "ritz succeeds", n);
    double worst = 0.0, orth = 0.0;
    for (int k = 0; k < m; ++k) {
      for (int i = 0; i < n; ++i) {
        double r = 0.0;
        for (int j = 0; j < n; ++j) r += (ga[i * n + j] - ev[k] * gb[i * n + j]) * c[j * m + k];
        worst = std::fmax(worst, std::fabs(r));
      }
      if (k > 0) expect(ev[k] >= ev[k - 1], "eigenvalues ascend", n);
      for (int l = 0; l < m; ++l) {
        double s = 0.0;
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j) s += c[i * m + k] * gb[i * n + j] * c[j * m + l];
        orth = std::fmax(orth, std::fabs(s - (k == l ? 1.0 : 0.0)));
      }
    }
    expect(worst < 1e-10 * n, "G_A c = lambda G_B c", n);
    expect(orth < 1e-11 * n, "C^T G_B C = I", n);

    std::vector<double> t(n * n);
    expect(mgd::chol_orth_transform(n, gb.data(), t.data()), "chol_orth_transform succeeds", n);
    double dev = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int k = 0; k < n; ++k)
          for (int l = 0; l < n; ++l) s += t[k * n + i] * gb[k * n + l] * t[l * n + j];
        dev = std::fmax(dev, std::fabs(s - (i == j ? 1.0 : 0.0)));
      }
    expect(dev < 1e-10 * n, "T^T G T = I", n);

    std::vector<double> sing = gb;                  // the Gram matrix of a block with a zero vector: a zero pivot
    for (int j = 0; j < n; ++j) sing[(n - 1) * n + j] = sing[j * n + n - 1] = 0.0;
    expect(mgd::ritz(n, m, ga.data(), sing.data(), ev.data(), c.data()) == 1, "ritz refuses a singular G_B", n);
    expect(!mgd::chol_orth_transform(n, sing.data(), t.data()), "chol_orth_transform refuses a singular G", n);
    std::vector<double> bad = gb;
    bad[0] = std::nan("");
    expect(mgd::ritz(n, m, ga.data(), bad.data(), ev.data(), c.data()) == 1, "ritz refuses a NaN pivot", n);
    bad[0] = -1.0;
    expect(!mgd::chol_orth_transform(n, bad.data(), t.data()), "chol_orth_transform refuses a negative diagonal", n);
  }
  double one = 1.0, e = 0.0, c = 0.0;
  expect(mgd::ritz(0, 1, &one, &one, &e, &c) == -1 && mgd::ritz(49, 1, &one, &one, &e, &c) == -1 && mgd::ritz(1, 2, &one, &one, &e, &c) == -1,
         "ritz refuses n outside 1 .. 48 and m > n", 0);
  std::printf(failures ? "%d checks failed\n" : "all dense checks passed\n", failures);
  return failures ? 1 : 0;
}
