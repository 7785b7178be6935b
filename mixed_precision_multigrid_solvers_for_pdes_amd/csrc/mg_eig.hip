// The block eigensolver of libmghip.so (include/mghip_eig.h): LOBPCG for the lowest eigenpairs of the engine's operator with
// the multigrid cycle as preconditioner.  This unit instantiates the kernels of mg_eig_kernels.hpp and holds the driver; the
// dense m x m .. 3m x 3m algebra runs on the host (mg_eig_dense.hpp).  The preconditioner is an mg_handle of its own, driven
// through the device entry points of the C ABI (mg_set_rhs_device / mg_update_rhs_device, mg_zero_solution_device, mg_cycle,
// mg_get_solution_device) on the engine's stream, where the solver queues its own kernels too.
//
// Blocks: two runs of 6 m columns [P X W AP AX AW].  An iteration reads the current block and writes [P X] and [AP AX] of the
// other one (step 6), whose W and AW columns serve as scratch before that.  The host waits three times per iteration: for the
// m residual norms, for the (2m x m) Gram matrix [X W]^T W of step 3 and for the (3m x 6m) Gram matrix S^T [S AS] of step 5.
// What it sends (eigenvalues, coefficient matrices) is written to a ring of pinned slots and copied asynchronously: no wait.
#include "mg_launch.hpp"
#include "mg_eig_kernels.hpp"
#include "mg_eig_dense.hpp"
#include "../../include/mghip_eig.h"

using namespace mgh;

namespace {
constexpr int kMaxBlock = 16;
constexpr int kTimedIters = 64;         // iterations whose preconditioner is bracketed by events (the rest: their mean)
constexpr int kGramWorkgroups = 1024;   // partial blocks the solver's own scratch has room for: 4 workgroups per CU (the register budget of m <= 8)
constexpr int kSlotP = 0, kSlotX = 1, kSlotW = 2, kSlotAP = 3, kSlotAX = 4, kSlotAW = 5;
constexpr int kHostDoubles = mg::kEigMaxP * mg::kEigMaxQ;
constexpr int kSendSlots = 4, kSendDoubles = mg::kEigMaxP * mg::kEigMaxP;   // pinned slots for host -> device coefficients
}  // namespace

struct mg_eig {
  mg_config cfg;
  mg_handle* eng = nullptr;
  int nx = 0, ny = 0, ld = 0, m = 0, num_cycles = 1;
  double hx = 0, hy = 0;
  long long cs = 0;                     // col_stride = nx * ld
  double* blk[2] = {nullptr, nullptr};
  double *a = nullptr, *staging = nullptr;
  double* scratch = nullptr;
  size_t scratch_doubles = 0;
  double *g_dev = nullptr, *coef_dev = nullptr, *lam_dev = nullptr, *sumsq_dev = nullptr;
  double* h_pin = nullptr;              // pinned host: kHostDoubles, what the device sends back
  double* h_send = nullptr;             // pinned host: kSendSlots x kSendDoubles, what the host sends
  int send_next = 0, sends_in_flight = 0;   // slots written since the host last waited for the stream
  bool varcoef = false, eng_has_rhs = false;
  hipEvent_t ev[2 * kTimedIters] = {};
  int nev = 0;
  std::string err;
  double* col(int b, int slot, int i = 0) const { return blk[b] + ((long long)slot * m + i) * cs; }
};

namespace {

int nyv_of(int ny, int ld) { return std::min(ld, (ny + 1) / 2 * 2); }

int stream_blocks(long long vecs, int cap) {
  return (int)std::max<long long>(1, std::min<long long>((vecs + mg::kBlock - 1) / mg::kBlock, cap));
}

// ---- launchers (shared by the driver and the stateless mg_dev_eig_* forms) ----
void launch_apply(const double* v, double* av, const double* a, int ncols, long long cs, int nx, int ny, int ld, double hx, double hy,
                  double coeff, hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  const Coef c = coefs(hx, hy, 0.0);
  auto k = a ? mg::eig_apply_kernel<true> : mg::eig_apply_kernel<false>;
  hipLaunchKernelGGL(k, dim3(g.ntiles, 1, ncols), dim3(mg::kBlock), 0, st, v, av, a, cs, g, c.ihx2, c.ihy2, c.diag, coeff);
}

// the LDS a gram launch may ask for is raised once per process
int gram_attrs() {
  static const int rc = [] {
    const hipError_t e = hipFuncSetAttribute((const void*)mg::eig_gram_kernel<18>, hipFuncAttributeMaxDynamicSharedMemorySize, mg::kEigGramLdsBytes);
    return e == hipSuccess ? MG_OK : MG_ERR_HIP;
  }();
  return rc;
}

// cap: doubles of `scratch`
int launch_gram(int p, const double* u, int q, const double* v, long long cs, int nx, int ny, int ld, double* scratch, size_t cap,
                double* g_dev, hipStream_t st) {
  if (gram_attrs() != MG_OK) return MG_ERR_HIP;
  mg::EigGramArgs g;
  g.p = p; g.q = q; g.nx = nx; g.ny = ny; g.ld = ld; g.col_stride = cs;
  // distance in elements on integers: u and v may be unrelated allocations
  const long long d = (long long)((intptr_t)(uintptr_t)v - (intptr_t)(uintptr_t)u) / (long long)sizeof(double);
  const long long off = d / cs;
  if (d % cs == 0 && std::max<long long>(p, off + q) - std::min<long long>(0, off) <= mg::kEigMaxP + mg::kEigMaxQ &&
      off <= p && off + q >= 0) {                      // one run of columns (overlapping or adjacent): stage it once
    const long long lo = std::min<long long>(0, off), hi = std::max<long long>(p, off + q);
    g.seg0 = u + lo * cs; g.n0 = (int)(hi - lo);
    g.seg1 = nullptr; g.n1 = 0;
    g.uo = (int)-lo; g.vo = (int)(off - lo);
  } else {
    g.seg0 = u; g.n0 = p; g.seg1 = v; g.n1 = q; g.uo = 0; g.vo = p;
  }
  g.tiles_j = (nyv_of(ny, ld) + mg::kEigKC - 1) / mg::kEigKC;
  g.ntiles = (nx - 2) * g.tiles_j;
  const int PP = (p + 15) / 16 * 16, QP = (q + 15) / 16 * 16;
  long long nwg = std::min<long long>(std::min<long long>(g.ntiles, kGramWorkgroups), (long long)(cap / ((size_t)PP * QP)));
  g.direct = nwg <= 1 ? 1 : 0;
  if (nwg < 1) nwg = 1;
  const size_t lds = (size_t)(g.n0 + g.n1) * mg::kEigKCP * sizeof(double);
  const int ncol = g.n0 + g.n1;                        // 32 vectors per column and tile, 256 threads
  auto k = ncol <= 48 ? mg::eig_gram_kernel<6> : (ncol <= 96 ? mg::eig_gram_kernel<12> : mg::eig_gram_kernel<18>);
  hipLaunchKernelGGL(k, dim3((unsigned)nwg), dim3(mg::kBlock), lds, st, g, g.direct ? g_dev : scratch);
  if (!g.direct)
    hipLaunchKernelGGL(mg::eig_gram_reduce_kernel, dim3((p * q + mg::kBlock - 1) / mg::kBlock), dim3(mg::kBlock), 0, st, scratch, (int)nwg,
                       p, q, QP, PP * QP, g_dev);
  return MG_OK;
}

void launch_combine(int p, const double* in, int q, const double* coef_dev, double* out, long long cs, int nx, int ny, int ld,
                    hipStream_t st) {
  const int nyv = nyv_of(ny, ld);
  const int nb = stream_blocks((long long)nx * (nyv / 2), 2048);
  for (int b0 = 0; b0 < q; b0 += 48) {                 // more than 48 outputs: another pass over the inputs
    const int qc = std::min(48, q - b0);
    auto k = qc <= 16 ? mg::eig_combine_kernel<16> : (qc <= 32 ? mg::eig_combine_kernel<32> : mg::eig_combine_kernel<48>);
    hipLaunchKernelGGL(k, dim3(nb), dim3(mg::kBlock), 0, st, in, out + (long long)b0 * cs, coef_dev + b0, q, p, qc, nx, nyv, ld, cs);
  }
}

void launch_residual(int ncols, const double* x, const double* ax, const double* lam_dev, double* r, long long cs, int nx, int ny,
                     int ld, double* scratch, size_t cap, double* sumsq_dev, hipStream_t st) {
  const int nyv = nyv_of(ny, ld);
  const int nb = stream_blocks((long long)nx * (nyv / 2), (int)std::min<size_t>(512, cap / ncols));
  hipLaunchKernelGGL(mg::eig_residual_kernel, dim3(nb, 1, ncols), dim3(mg::kBlock), 0, st, x, ax, lam_dev, r, scratch, nx, ny, nyv, ld, cs);
  hipLaunchKernelGGL(mg::eig_reduce_cols_kernel, dim3(ncols), dim3(mg::kBlock), 0, st, scratch, nb, sumsq_dev);
}

void release(mg_eig* s) {
  if (s->eng) { (void)mg_destroy(s->eng); s->eng = nullptr; }
  for (double** p : {&s->blk[0], &s->blk[1], &s->a, &s->staging, &s->scratch, &s->g_dev, &s->coef_dev, &s->lam_dev, &s->sumsq_dev})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (s->h_pin) { (void)hipHostFree(s->h_pin); s->h_pin = nullptr; }
  if (s->h_send) { (void)hipHostFree(s->h_send); s->h_send = nullptr; }
  for (int k = 0; k < s->nev; ++k) (void)hipEventDestroy(s->ev[k]);
  s->nev = 0;
}

// host array (nx, ny) of hdt -> fp64 device field with the solver's pitch, on the engine's stream
int put(mg_eig* s, double* dev, const void* host, int hdt) {
  return upload(&s->err, dev, MG_F64, s->ld, host, hdt, s->nx, s->ny, s->staging, s->eng->stream);
}

// w = M r: num_cycles cycles from the zero iterate on the engine (the ring of r is zero: mg_update_rhs_device's contract)
int precondition(mg_eig* s, const double* r, double* w) {
  OWNED(engine_precondition(s->eng, &s->eng_has_rhs, r, w, s->ld, s->num_cycles), "preconditioner: ", mg_last_error(s->eng));
  return MG_OK;
}

// n doubles device -> pinned host, and wait (one of the three synchronisations of an iteration)
int fetch(mg_eig* s, const double* dev, int n) {
  hipStream_t st = s->eng->stream;
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_pin, dev, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIPC(&s->err, hipStreamSynchronize(st));
  s->sends_in_flight = 0;
  return MG_OK;
}

// n <= kSendDoubles host doubles -> dev without waiting: they go through the next pinned slot, which the copy engine reads
// after this call returns.  A slot is rewritten only after the host has waited for the stream since it was last queued
// (every fetch does); a run of kSendSlots sends without one waits itself, which no path of the solver reaches.
int send(mg_eig* s, double* dev, const double* host, int n) {
  hipStream_t st = s->eng->stream;
  if (s->sends_in_flight >= kSendSlots) { HIPC(&s->err, hipStreamSynchronize(st)); s->sends_in_flight = 0; }
  double* slot = s->h_send + (size_t)s->send_next * kSendDoubles;
  s->send_next = (s->send_next + 1) % kSendSlots;
  ++s->sends_in_flight;
  std::copy(host, host + n, slot);
  HIPC(&s->err, hipMemcpyAsync(dev, slot, sizeof(double) * n, hipMemcpyHostToDevice, st));
  return MG_OK;
}

// p x q host coefficients -> coef_dev (stream-ordered behind the launches that still read it), then out = in . coef
int combine(mg_eig* s, int p, const double* in, int q, const double* coef, double* out) {
  const int rc = send(s, s->coef_dev, coef, p * q);
  if (rc != MG_OK) return rc;
  launch_combine(p, in, q, s->coef_dev, out, s->cs, s->nx, s->ny, s->ld, s->eng->stream);
  return MG_OK;
}

int gram(mg_eig* s, int p, const double* u, int q, const double* v) {
  if (launch_gram(p, u, q, v, s->cs, s->nx, s->ny, s->ld, s->scratch, s->scratch_doubles, s->g_dev, s->eng->stream) != MG_OK)
    return sfail(s, MG_ERR_HIP, "mg_eig: hipFuncSetAttribute failed");
  return fetch(s, s->g_dev, p * q);
}

void apply(mg_eig* s, const double* v, double* av, int ncols) {
  launch_apply(v, av, s->varcoef ? s->a : nullptr, ncols, s->cs, s->nx, s->ny, s->ld, s->hx, s->hy, s->cfg.coeff, s->eng->stream);
}

int solve(mg_eig* s, int nev, const void* x0, int hdt, double tol, int max_iter, double* evals, void* vecs, double* resid,
          double* hist, int hist_cap, int* n_iter, int* converged, mg_eig_stats* stats) {
  hipStream_t st = s->eng->stream;
  const double t0 = now_s();
  const int m = s->m, nx = s->nx, ny = s->ny;
  const size_t host_col = (size_t)nx * ny * esize(hdt);
  int rc;
  for (int b = 0; b < 2; ++b) HIPC(&s->err, hipMemsetAsync(s->blk[b], 0, field_bytes(s) * 6 * m, st));
  for (int i = 0; i < m; ++i)
    if ((rc = put(s, s->col(0, kSlotX, i), (const char*)x0 + i * host_col, hdt)) != MG_OK) return rc;
  hipLaunchKernelGGL(mg::eig_zero_ring_kernel, dim3(std::max(1, std::min(64, (2 * (nx + ny) + mg::kBlock - 1) / mg::kBlock)), 1, m),
                     dim3(mg::kBlock), 0, st, s->col(0, kSlotX), nx, ny, s->ld, s->cs);

  double T[mgd::kMaxN * mgd::kMaxN], lam[kMaxBlock], rel[kMaxBlock];
  // start: X orthonormal in block 1, AX = A X, Rayleigh-Ritz on X^T A X, the rotated pair in block 0
  if ((rc = gram(s, m, s->col(0, kSlotX), m, s->col(0, kSlotX))) != MG_OK) return rc;
  if (!mgd::chol_orth_transform(m, s->h_pin, T))
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_eig_solve: the start vectors are linearly dependent (or not finite) on the interior cells");
  if ((rc = combine(s, m, s->col(0, kSlotX), m, T, s->col(1, kSlotX))) != MG_OK) return rc;
  apply(s, s->col(1, kSlotX), s->col(1, kSlotAX), m);
  if ((rc = gram(s, m, s->col(1, kSlotX), m, s->col(1, kSlotAX))) != MG_OK) return rc;
  {
    double A[kMaxBlock * kMaxBlock];
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) A[i * m + j] = 0.5 * (s->h_pin[i * m + j] + s->h_pin[j * m + i]);
    mgd::jacobi_eigh(m, A, T, lam);
  }
  if ((rc = combine(s, m, s->col(1, kSlotX), m, T, s->col(0, kSlotX))) != MG_OK) return rc;
  if ((rc = combine(s, m, s->col(1, kSlotAX), m, T, s->col(0, kSlotAX))) != MG_OK) return rc;

  int cur = 0, it = 0, status = 1, restarts = 0, in_a_row = 0, timed = 0, applied = 0;
  bool have_p = false, conv = false;
  for (;; ++it) {
    const int nxt = cur ^ 1;
    // 1: residuals into the AW columns, their norms
    if ((rc = send(s, s->lam_dev, lam, m)) != MG_OK) return rc;
    launch_residual(m, s->col(cur, kSlotX), s->col(cur, kSlotAX), s->lam_dev, s->col(cur, kSlotAW), s->cs, nx, ny, s->ld, s->scratch,
                    s->scratch_doubles, s->sumsq_dev, st);
    if ((rc = fetch(s, s->sumsq_dev, m)) != MG_OK) return rc;
    double worst = 0.0;
    for (int i = 0; i < m; ++i) {
      rel[i] = std::sqrt(s->h_pin[i]) / lam[i];
      if (i < nev && !(rel[i] <= worst)) worst = rel[i];        // a NaN sticks
    }
    if (it < hist_cap) hist[it] = worst;
    if (worst < tol) { conv = true; status = 0; break; }
    if (it >= max_iter) break;
    // 2: W_i = M R_i
    const bool ev_ok = it < kTimedIters && s->nev == 2 * kTimedIters;
    if (ev_ok) HIPC(&s->err, hipEventRecord(s->ev[2 * it], st));
    for (int i = 0; i < m; ++i)
      if ((rc = precondition(s, s->col(cur, kSlotAW, i), s->col(cur, kSlotW, i))) != MG_OK) return rc;
    if (ev_ok) { HIPC(&s->err, hipEventRecord(s->ev[2 * it + 1], st)); ++timed; }
    ++applied;
    // 3: W := (W - X C) T with C = X^T W and T from the Gram matrix W^T W - C^T C of W - X C
    if ((rc = gram(s, 2 * m, s->col(cur, kSlotX), m, s->col(cur, kSlotW))) != MG_OK) return rc;
    {
      const double* C = s->h_pin;                    // m x m
      const double* WW = s->h_pin + m * m;
      double G[kMaxBlock * kMaxBlock], coef[2 * kMaxBlock * kMaxBlock];
      for (int i = 0; i < m; ++i)
        for (int j = 0; j <= i; ++j) {
          double cc = 0.0;
          for (int k = 0; k < m; ++k) cc += C[k * m + i] * C[k * m + j];
          G[i * m + j] = G[j * m + i] = 0.5 * (WW[i * m + j] + WW[j * m + i]) - cc;
        }
      if (!mgd::chol_orth_transform(m, G, T)) { status = 2; break; }
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
          double ct = 0.0;
          for (int k = 0; k < m; ++k) ct += C[i * m + k] * T[k * m + j];
          coef[i * m + j] = -ct;
          coef[(m + i) * m + j] = T[i * m + j];
        }
      if ((rc = combine(s, 2 * m, s->col(cur, kSlotX), m, coef, s->col(nxt, kSlotW))) != MG_OK) return rc;
    }
    HIPC(&s->err, hipMemcpyAsync(s->col(cur, kSlotW), s->col(nxt, kSlotW), field_bytes(s) * m, hipMemcpyDeviceToDevice, st));
    apply(s, s->col(cur, kSlotW), s->col(cur, kSlotAW), m);
    // 4, 5: S^T [S AS] in one pass; physical order [P X W], logical order [X W P]
    if ((rc = gram(s, 3 * m, s->col(cur, kSlotP), 6 * m, s->col(cur, kSlotP))) != MG_OK) return rc;
    const int n3 = 3 * m;
    double GB[mgd::kMaxN * mgd::kMaxN], GA[mgd::kMaxN * mgd::kMaxN], Cr[mgd::kMaxN * kMaxBlock], Tp[kMaxBlock * kMaxBlock], ev[kMaxBlock];
    // The dense algebra works in the algorithm's order S = [X W P]; the device holds [P X W], so that the [P X] and [AP AX]
    // step 6 writes are adjacent (one combine call each) and [X W] is for step 3.  phys: logical index -> device column.
    auto phys = [m](int l) { return l < 2 * m ? l + m : l - 2 * m; };
    bool dropped = false, ok = false;
    for (int attempt = 0; attempt < 2 && !ok; ++attempt) {
      const bool use_p = have_p && !dropped;
      const int n = use_p ? 3 * m : 2 * m;
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          const int pi = phys(i), pj = phys(j);
          GB[i * n + j] = 0.5 * (s->h_pin[pi * 2 * n3 + pj] + s->h_pin[pj * 2 * n3 + pi]);
          GA[i * n + j] = 0.5 * (s->h_pin[pi * 2 * n3 + n3 + pj] + s->h_pin[pj * 2 * n3 + n3 + pi]);
        }
      if (use_p) {                                   // 4: P := P Tp, as a change of basis of the Gram matrices
        double Gp[kMaxBlock * kMaxBlock];
        for (int i = 0; i < m; ++i)
          for (int j = 0; j < m; ++j) Gp[i * m + j] = GB[(2 * m + i) * n + 2 * m + j];
        if (!mgd::chol_orth_transform(m, Gp, Tp)) { dropped = true; continue; }
        for (double* M : {GB, GA}) {
          double tmp[kMaxBlock];
          for (int i = 0; i < n; ++i) {              // columns of the P block
            for (int j = 0; j < m; ++j) { double v = 0.0; for (int k = 0; k <= j; ++k) v += M[i * n + 2 * m + k] * Tp[k * m + j]; tmp[j] = v; }
            for (int j = 0; j < m; ++j) M[i * n + 2 * m + j] = tmp[j];
          }
          for (int j = 0; j < n; ++j) {              // rows of the P block
            for (int i = 0; i < m; ++i) { double v = 0.0; for (int k = 0; k <= i; ++k) v += Tp[k * m + i] * M[(2 * m + k) * n + j]; tmp[i] = v; }
            for (int i = 0; i < m; ++i) M[(2 * m + i) * n + j] = tmp[i];
          }
        }
      }
      if (mgd::ritz(n, m, GA, GB, ev, Cr) != 0) {
        if (use_p) { dropped = true; continue; }
        break;
      }
      ok = true;
      if (use_p) {                                   // coefficients of the P the device holds: Tp C_P
        double tmp[kMaxBlock * kMaxBlock];
        for (int i = 0; i < m; ++i)
          for (int j = 0; j < m; ++j) { double v = 0.0; for (int k = i; k < m; ++k) v += Tp[i * m + k] * Cr[(2 * m + k) * m + j]; tmp[i * m + j] = v; }
        for (int i = 0; i < m * m; ++i) Cr[2 * m * m + i] = tmp[i];
      } else {
        for (int i = 0; i < m * m; ++i) Cr[2 * m * m + i] = 0.0;
      }
    }
    if (dropped) { ++restarts; ++in_a_row; } else in_a_row = 0;
    if (!ok || in_a_row >= 2) { status = 2; break; }
    // 6: [P' X'] = S K and [AP' AX'] = AS K with K (3m x 2m, rows in physical order): P' = W C_W + P C_P, X' = X C_X + P'
    {
      double K[mgd::kMaxN * 2 * kMaxBlock];
      for (int l = 0; l < n3; ++l) {
        const int r = phys(l);
        for (int j = 0; j < m; ++j) {
          const double c = Cr[l * m + j];
          K[r * 2 * m + j] = l < m ? 0.0 : c;
          K[r * 2 * m + m + j] = c;
        }
      }
      if (dropped || !have_p) {                      // their coefficients are zero, but 0 * inf is not
        HIPC(&s->err, hipMemsetAsync(s->col(cur, kSlotP), 0, field_bytes(s) * m, st));
        HIPC(&s->err, hipMemsetAsync(s->col(cur, kSlotAP), 0, field_bytes(s) * m, st));
      }
      if ((rc = send(s, s->coef_dev, K, n3 * 2 * m)) != MG_OK) return rc;
      launch_combine(n3, s->col(cur, kSlotP), 2 * m, s->coef_dev, s->col(nxt, kSlotP), s->cs, nx, ny, s->ld, st);
      launch_combine(n3, s->col(cur, kSlotAP), 2 * m, s->coef_dev, s->col(nxt, kSlotAP), s->cs, nx, ny, s->ld, st);
    }
    for (int i = 0; i < m; ++i) lam[i] = ev[i];
    have_p = true;
    cur = nxt;
  }
  // the returned vectors: hx hy sum v^2 = 1
  {
    double D[kMaxBlock * kMaxBlock];
    const double sc = 1.0 / std::sqrt(s->hx * s->hy);
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) D[i * m + j] = i == j ? sc : 0.0;
    if ((rc = combine(s, m, s->col(cur, kSlotX), m, D, s->col(cur ^ 1, kSlotX))) != MG_OK) return rc;
    HIPC(&s->err, hipGetLastError());
    for (int i = 0; i < nev; ++i)
      if ((rc = download(&s->err, (char*)vecs + i * host_col, hdt, s->col(cur ^ 1, kSlotX, i), MG_F64, s->ld, nx, ny, s->staging, st)) != MG_OK)
        return rc;
  }
  HIPC(&s->err, hipStreamSynchronize(st));
  const double t1 = now_s();
  double pre_ms = 0;
  for (int k = 0; k < timed; ++k) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, s->ev[2 * k], s->ev[2 * k + 1]) == hipSuccess) pre_ms += ms;
  }
  if (timed > 0 && applied > timed) pre_ms *= (double)applied / timed;
  for (int i = 0; i < m; ++i) { evals[i] = lam[i]; resid[i] = rel[i]; }
  *n_iter = it;
  *converged = conv ? 1 : 0;
  if (stats) {
    stats->solve_seconds = t1 - t0;
    stats->precond_seconds = pre_ms * 1e-3;
    stats->iterations = it;
    stats->restarts = restarts;
    stats->status = status;
  }
  return MG_OK;
}

}  // namespace

extern "C" {

int mg_eig_create(const mg_config* cfg, int block_size, int num_cycles, mg_eig** out) {
  if (!cfg || !out) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_eig_create: NULL argument");
  *out = nullptr;
  if (cfg->precision != MG_PREC_DOUBLE && cfg->precision != MG_PREC_SINGLE_MANAGED && cfg->precision != MG_PREC_MIXED_LEVELS)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_eig_create: the preconditioner runs in MG_PREC_DOUBLE, MG_PREC_SINGLE_MANAGED or MG_PREC_MIXED_LEVELS");
  if (cfg->fmg_cycles != 0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_eig_create: fmg_cycles must be 0 (the preconditioner starts from zero)");
  if (!(cfg->coeff < 0.0)) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_eig_create: the eigensolver needs an SPD operator (coeff < 0)");
  if (block_size < 1 || block_size > kMaxBlock) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_eig_create: block_size must be 1 .. 16");
  if (num_cycles < 1) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_eig_create: num_cycles < 1");
  mg_handle* eng = nullptr;
  int rc = mg_create(cfg, &eng);
  if (rc != MG_OK) return rc;
  mg_eig* s = new mg_eig();
  s->cfg = *cfg;
  s->eng = eng;
  s->nx = cfg->nx; s->ny = cfg->ny;
  s->ld = pitch_elems(MG_F64, cfg->ny);
  s->cs = (long long)s->nx * s->ld;
  s->hx = eng->lv[0].hx; s->hy = eng->lv[0].hy;
  s->m = block_size;
  s->num_cycles = num_cycles;
  auto bail = [&](int code) { return create_fail(s, release, code); };
  hipStream_t st = eng->stream;
  for (int b = 0; b < 2; ++b)
    if ((rc = alloc_zero(&s->err, (void**)&s->blk[b], field_bytes(s) * 6 * block_size, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->staging, field_bytes(s), st)) != MG_OK) return bail(rc);
  const int PP = (3 * block_size + 15) / 16 * 16, QP = (6 * block_size + 15) / 16 * 16;
  s->scratch_doubles = std::max<size_t>((size_t)kGramWorkgroups * PP * QP, max_partials(s->nx, s->ny));
  if ((rc = alloc_zero(&s->err, (void**)&s->scratch, sizeof(double) * s->scratch_doubles, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->g_dev, sizeof(double) * kHostDoubles, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->coef_dev, sizeof(double) * mg::kEigMaxP * mg::kEigMaxP, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->lam_dev, sizeof(double) * kMaxBlock, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->sumsq_dev, sizeof(double) * kMaxBlock, st)) != MG_OK) return bail(rc);
  if (hipHostMalloc((void**)&s->h_pin, sizeof(double) * kHostDoubles) != hipSuccess) { s->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  if (hipHostMalloc((void**)&s->h_send, sizeof(double) * kSendSlots * kSendDoubles) != hipSuccess) { s->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  for (; s->nev < 2 * kTimedIters; ++s->nev)
    if (hipEventCreate(&s->ev[s->nev]) != hipSuccess) break;
  if (hipStreamSynchronize(st) != hipSuccess) { s->err = "hipStreamSynchronize failed"; return bail(MG_ERR_HIP); }
  *out = s;
  return MG_OK;
}

int mg_eig_destroy(mg_eig* s) {
  return destroy_owned(s, s && s->eng ? s->eng->stream : nullptr, release);
}

const char* mg_eig_last_error(const mg_eig* s) { return s ? s->err.c_str() : last_error().c_str(); }

int mg_eig_set_coefficient(mg_eig* s, const void* a_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_eig_set_coefficient: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_set_coefficient(s->eng, a_host_or_null, host_dtype), "preconditioner: ", mg_last_error(s->eng));
  if (!a_host_or_null) { s->varcoef = false; return MG_OK; }
  if (!s->a) { const int rc = alloc_zero(&s->err, (void**)&s->a, field_bytes(s), s->eng->stream); if (rc != MG_OK) return rc; }
  const int rc = put(s, s->a, a_host_or_null, host_dtype);
  if (rc != MG_OK) return rc;
  s->varcoef = true;
  return MG_OK;
}

int mg_eig_solve(mg_eig* s, int nev, const void* x0_host, int host_dtype, double tol, int max_iter, double* eigenvalues,
                 void* vectors_out, double* residuals, double* hist, int hist_cap, int* n_iter, int* converged, mg_eig_stats* stats) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_eig_solve: NULL solver");
  if (!x0_host || !eigenvalues || !vectors_out || !residuals || !hist || !n_iter || !converged)
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_eig_solve: NULL argument");
  if (!valid_dtype(host_dtype) || hist_cap < 1 || max_iter < 0 || !(tol == tol) || nev < 1 || nev > s->m)
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_eig_solve: bad dtype / hist_cap < 1 / max_iter < 0 / tol is NaN / nev outside 1 .. block_size");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  const int rc = solve(s, nev, x0_host, host_dtype, tol, max_iter, eigenvalues, vectors_out, residuals, hist, hist_cap, n_iter, converged, stats);
  if (rc != MG_OK) (void)hipStreamSynchronize(s->eng->stream);
  return rc;
}

int mg_eig_host_ritz(int n, int m, const double* ga, const double* gb, double* evals, double* coef) {
  if (!ga || !gb || !evals || !coef || n < 1 || n > mgd::kMaxN || m < 1 || m > n)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_eig_host_ritz: NULL argument or n outside 1 .. 48 or m outside 1 .. n");
  return mgd::ritz(n, m, ga, gb, evals, coef);
}

int mg_dev_eig_apply(int nx, int ny, int ld, int ncols, int64_t col_stride, double hx, double hy, double coeff, const double* a_or_null,
                     const double* v, double* av, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld) && ncols >= 1 && ncols <= 65535 && col_stride >= (int64_t)nx * ld && col_stride % 2 == 0,
            "mg_dev_eig_apply: bad shape / pitch / column count / column stride");
  CHECK_ARG(v && av && v != av && aligned16(v) && aligned16(av) && aligned16(a_or_null), "mg_dev_eig_apply: NULL, unaligned or aliased pointer");
  launch_apply(v, av, a_or_null, ncols, col_stride, nx, ny, ld, hx, hy, coeff, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_eig_gram(int nx, int ny, int ld, int64_t col_stride, int p, const double* u, int q, const double* v, void* scratch,
                    double* g_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld) && col_stride >= (int64_t)nx * ld && col_stride % 2 == 0, "mg_dev_eig_gram: bad shape / pitch / column stride");
  CHECK_ARG(p >= 1 && p <= mg::kEigMaxP && q >= 1 && q <= mg::kEigMaxQ, "mg_dev_eig_gram: p outside 1 .. 48 or q outside 1 .. 96");
  CHECK_ARG(u && v && scratch && g_dev && aligned16(u) && aligned16(v) && aligned16(scratch), "mg_dev_eig_gram: NULL or unaligned pointer");
  if (launch_gram(p, u, q, v, col_stride, nx, ny, ld, (double*)scratch, max_partials(nx, ny), g_dev, (hipStream_t)stream) != MG_OK)
    return fail(nullptr, MG_ERR_HIP, "mg_dev_eig_gram: hipFuncSetAttribute failed");
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_eig_combine(int nx, int ny, int ld, int64_t col_stride, int p, const double* in, int q, const double* coef_dev, double* out,
                       void* stream) {
  CHECK_ARG(nx >= 1 && ny >= 1 && ld_ok_f64(ny, ld) && col_stride >= (int64_t)nx * ld && col_stride % 2 == 0, "mg_dev_eig_combine: bad shape / pitch / column stride");
  CHECK_ARG(p >= 1 && p <= mg::kEigMaxP && q >= 1 && q <= mg::kEigMaxQ, "mg_dev_eig_combine: p outside 1 .. 48 or q outside 1 .. 96");
  CHECK_ARG(in && out && coef_dev && aligned16(in) && aligned16(out), "mg_dev_eig_combine: NULL or unaligned pointer");
  CHECK_ARG(out + (int64_t)q * col_stride <= in || in + (int64_t)p * col_stride <= out, "mg_dev_eig_combine: out overlaps in");
  launch_combine(p, in, q, coef_dev, out, col_stride, nx, ny, ld, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_eig_residual(int nx, int ny, int ld, int ncols, int64_t col_stride, const double* x, const double* ax, const double* lambda_dev,
                        double* r, void* scratch, double* sumsq_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld) && ncols >= 1 && ncols <= kMaxBlock && col_stride >= (int64_t)nx * ld && col_stride % 2 == 0,
            "mg_dev_eig_residual: bad shape / pitch / column count / column stride");
  CHECK_ARG(x && ax && lambda_dev && r && scratch && sumsq_dev && r != x && r != ax && aligned16(x) && aligned16(ax) && aligned16(r),
            "mg_dev_eig_residual: NULL, unaligned or aliased pointer");
  launch_residual(ncols, x, ax, lambda_dev, r, col_stride, nx, ny, ld, (double*)scratch, max_partials(nx, ny), sumsq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_eig_time_op(mg_eig* s, int op, int reps, double* avg_ms) {
  if (!s || !avg_ms || reps < 1 || op < 0 || op > 3) return sfail(s, MG_ERR_INVALID_VALUE, "mg_eig_time_op: bad argument");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  hipStream_t st = s->eng->stream;
  const int m = s->m;
  hipEvent_t e0, e1;
  HIPC(&s->err, hipEventCreate(&e0));
  HIPC(&s->err, hipEventCreate(&e1));
  int rc = MG_OK;
  auto once = [&]() -> int {
    switch (op) {
      case 0: apply(s, s->col(0, kSlotW), s->col(0, kSlotAW), m); return MG_OK;
      case 1:
        return launch_gram(3 * m, s->col(0, kSlotP), 6 * m, s->col(0, kSlotP), s->cs, s->nx, s->ny, s->ld, s->scratch, s->scratch_doubles,
                           s->g_dev, st);
      case 2: launch_combine(3 * m, s->col(0, kSlotP), 2 * m, s->coef_dev, s->col(1, kSlotP), s->cs, s->nx, s->ny, s->ld, st); return MG_OK;
      default: return precondition(s, s->col(0, kSlotAW), s->col(0, kSlotW));
    }
  };
  for (int k = 0; k < 2 && rc == MG_OK; ++k) rc = once();              // warm-up
  if (rc == MG_OK && hipEventRecord(e0, st) != hipSuccess) rc = MG_ERR_HIP;
  for (int k = 0; k < reps && rc == MG_OK; ++k) rc = once();
  if (rc == MG_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipGetLastError() != hipSuccess)) rc = MG_ERR_HIP;
  float ms = 0;
  if (rc == MG_OK && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = MG_ERR_HIP;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc != MG_OK) return s->err.empty() ? sfail(s, rc, "mg_eig_time_op: a HIP call failed") : rc;
  *avg_ms = (double)ms / reps;
  return MG_OK;
}

}  // extern "C"
