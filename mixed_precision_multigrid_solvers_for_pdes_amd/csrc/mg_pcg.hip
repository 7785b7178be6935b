// The Krylov outer loop of libmghip.so: device-resident preconditioned conjugate gradients with the multigrid cycle as
// preconditioner (include/mghip.h, "Krylov outer loop").  This unit instantiates the kernels of mg_pcg_kernels.hpp and holds
// the driver; the preconditioner is an mg_handle of its own, driven through the device entry points of the C ABI
// (mg_set_rhs_device / mg_update_rhs_device, mg_zero_solution_device, mg_cycle, mg_get_solution_device) on the engine's stream,
// where the solver queues its own kernels too.
//
//   r = f - A x (0 on the ring);  per iteration:  z = M r;  rz = r.z [, zq = z.q];  beta;  p = z + beta p, q = A p, pq = p.q;
//   alpha = rz / pq;  x += alpha p, r -= alpha q, rr = r.r;  ||r|| = sqrt(hx hy (rr + sum of f^2 over the ring)) < tol ?
//
// Everything up to alpha of iteration k + 1 writes only z, p, q and scalars, so with lookahead it is queued before the host waits
// for the norm of iteration k (a solve that ends there synchronises and drops it): the device never idles on the host.
//
// Under mg_pcg_set_order(4) (include/mghip_ho.h) A is the compact nine-point operator A4 and f is replaced by g = R f, formed
// once per solve; the kernels are those of mg_ho.hip (d_ho_*), everything else -- the five-point preconditioner included -- is
// the same code.
//
// Under mg_pcg_set_reaction_device (include/mghip_nl.h) A is A + diag(c) for a caller's field c: the direction kernel adds
// c p to q, the initial and the true residual come from the Newton method's eval kernel in linear kind (mg_nl.hip,
// d_nl_eval), and the engine preconditions with the scalar shift sigma + c_ref.  Without a field nothing here changes.
#include "mg_launch.hpp"
#include "mg_pcg_kernels.hpp"

#include "../../include/mghip_ho.h"
#include "../../include/mghip_nl.h"

#include <atomic>

using namespace mgh;

namespace {
constexpr int kTimedIters = 128;     // iterations whose preconditioner is bracketed by events (the rest: their mean)
constexpr int kHostScalars = 8;
// slots of the solver's scalar block past mg::kPcgScalars
constexpr int kRing0 = mg::kPcgScalars, kRr0 = kRing0 + 4, kTrue = kRr0 + 1, kNumScalars = kTrue + 1;
}  // namespace

struct mg_pcg {
  mg_config cfg;
  mg_handle* eng = nullptr;
  int nx = 0, ny = 0, ld = 0, nyv = 0;
  double hx = 0, hy = 0;
  int num_cycles = 1, flexible = 0;
  bool lookahead = true;
  double *x = nullptr, *r = nullptr, *z = nullptr, *q = nullptr, *f = nullptr, *a = nullptr, *staging = nullptr;
  double* p[2] = {nullptr, nullptr};
  int cur = 0;                          // p[cur] is the current direction
  double* partials = nullptr;           // 2 x np: the dots kernel's second sum starts at np
  int np = 0;
  double* sc = nullptr;                 // device scalar block (kNumScalars doubles)
  double* h_sc = nullptr;               // pinned host copy of its tail
  mg::PcgMailbox* mbox = nullptr;       // pinned, mapped
  mg::PcgMailbox* mbox_dev = nullptr;
  unsigned long long seq = 0;
  double sigma = 0.0;
  bool varcoef = false;
  int order = 2;                        // 2: the five-point operator, 4: the compact nine-point scheme (mg_pcg_set_order)
  double* g = nullptr;                  // order 4: R f of the current solve (allocated when order 4 is first set)
  const double* creact = nullptr;       // the caller's reaction field c (mg_pcg_set_reaction_device): A + diag(c); not owned
  double c_ref = 0.0;                   // ... and the scalar the preconditioner stands in for it with: shift sigma + c_ref
  bool eng_has_rhs = false;
  hipEvent_t ev[2 * kTimedIters] = {};
  int nev = 0;
  std::string err;
};

namespace {

int stream_blocks(int nx, int nyv) {
  const long long vecs = (long long)(nx - 2) * (nyv / 2);
  return (int)std::max<long long>(1, std::min<long long>((vecs + mg::kBlock - 1) / mg::kBlock, 1024));
}

// ---- launchers (shared by the driver and the stateless mg_dev_pcg_* forms); an int result is the number of partials ----
int launch_direction(const double* z, const double* p_in, double* p_out, double* q, const double* a, const double* creact,
                     const double* beta, double* partials, int nx, int ny, int ld, double hx, double hy, double coeff, double sigma,
                     hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  const Coef c = coefs(hx, hy, sigma);
  auto k = creact ? (a ? mg::pcg_direction_kernel<true, true> : mg::pcg_direction_kernel<false, true>)
                  : (a ? mg::pcg_direction_kernel<true, false> : mg::pcg_direction_kernel<false, false>);
  hipLaunchKernelGGL(k, dim3(g.ntiles), dim3(mg::kBlock), 0, st, z, p_in, p_out, q, a, creact, beta, partials, g, c.ihx2, c.ihy2,
                     c.diag, coeff, sigma);
  return g.ntiles;
}

int launch_update(const double* alpha, const double* p, const double* q, double* x, double* r, double* partials, int nx, int ny,
                  int ld, hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  const int nb = stream_blocks(nx, g.nyv);
  hipLaunchKernelGGL(mg::pcg_update_kernel, dim3(nb), dim3(mg::kBlock), 0, st, alpha, p, q, x, r, partials, nx, ny, g.nyv, ld);
  return nb;
}

int launch_dots(const double* r, const double* z, const double* q, double* partials, int second, int nx, int ny, int ld,
                hipStream_t st) {
  const mg::TileGeom g = field_geom(nx, ny, ld);
  const int nb = stream_blocks(nx, g.nyv);
  auto k = q ? mg::pcg_dots_kernel<true> : mg::pcg_dots_kernel<false>;
  hipLaunchKernelGGL(k, dim3(nb), dim3(mg::kBlock), 0, st, r, z, q, partials, second, nx, ny, g.nyv, ld);
  return nb;
}

void launch_scalars(int op, const double* pa, int na, const double* pb, int nb, double* sc, mg::PcgMailbox* mbox,
                    unsigned long long seq, hipStream_t st) {
  hipLaunchKernelGGL(mg::pcg_scalars_kernel, dim3(1), dim3(mg::kReduceBlock), 0, st, op, pa, na, pb, nb, sc, mbox, seq);
}

void release(mg_pcg* s) {
  if (s->eng) { (void)mg_destroy(s->eng); s->eng = nullptr; }
  for (double** p : {&s->x, &s->r, &s->z, &s->q, &s->f, &s->a, &s->g, &s->staging, &s->p[0], &s->p[1], &s->partials, &s->sc})
    if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (s->h_sc) { (void)hipHostFree(s->h_sc); s->h_sc = nullptr; }
  if (s->mbox) { (void)hipHostFree(s->mbox); s->mbox = nullptr; }
  for (int k = 0; k < s->nev; ++k) (void)hipEventDestroy(s->ev[k]);
  s->nev = 0;
}

// host array (nx, ny) of hdt -> fp64 device field with the solver's pitch, on the engine's stream
int put(mg_pcg* s, double* dev, const void* host, int hdt) {
  return upload(&s->err, dev, MG_F64, s->ld, host, hdt, s->nx, s->ny, s->staging, s->eng->stream);
}

// everything of iteration k that x and r do not depend on: z, the dots, beta, the new direction, q and alpha
int front(mg_pcg* s, int k) {
  hipStream_t st = s->eng->stream;
  const bool timed = k < kTimedIters && s->nev == 2 * kTimedIters;
  if (timed) HIPC(&s->err, hipEventRecord(s->ev[2 * k], st));
  OWNED(engine_precondition(s->eng, &s->eng_has_rhs, s->r, s->z, s->ld, s->num_cycles), "preconditioner: ", mg_last_error(s->eng));      // z = M r
  if (timed) HIPC(&s->err, hipEventRecord(s->ev[2 * k + 1], st));
  const bool flex = s->flexible && k > 0;
  const int nd = launch_dots(s->r, s->z, flex ? s->q : nullptr, s->partials, s->np, s->nx, s->ny, s->ld, st);
  launch_scalars(k == 0 ? mg::kPcgBeta0 : (flex ? mg::kPcgBetaFlex : mg::kPcgBetaFr), s->partials, nd, s->partials + s->np,
                 flex ? nd : 0, s->sc, nullptr, 0, st);
  const int nxt = s->cur ^ 1;
  const double* p_old = k == 0 ? nullptr : s->p[s->cur];
  const double* beta = k == 0 ? nullptr : s->sc + mg::kPcgBeta;
  const int nq = s->order == 4
      ? d_ho_direction(s->z, p_old, s->p[nxt], s->q, beta, s->partials, s->nx, s->ny, s->ld, s->hx, s->hy, s->cfg.coeff, s->sigma, st)
      : launch_direction(s->z, p_old, s->p[nxt], s->q, s->varcoef ? s->a : nullptr, s->creact, beta, s->partials, s->nx, s->ny,
                         s->ld, s->hx, s->hy, s->cfg.coeff, s->sigma, st);
  s->cur = nxt;
  launch_scalars(mg::kPcgAlphaOp, s->partials, nq, nullptr, 0, s->sc, nullptr, 0, st);
  HIPC(&s->err, hipGetLastError());
  return MG_OK;
}

// x += alpha p, r -= alpha q, rr; returns the mailbox sequence number the norm arrives under
int back(mg_pcg* s, unsigned long long* seq) {
  hipStream_t st = s->eng->stream;
  const int nu = launch_update(s->sc + mg::kPcgAlpha, s->p[s->cur], s->q, s->x, s->r, s->partials, s->nx, s->ny, s->ld, st);
  *seq = ++s->seq;
  launch_scalars(mg::kPcgNormOp, s->partials, nu, nullptr, 0, s->sc, s->mbox_dev, *seq, st);
  HIPC(&s->err, hipGetLastError());
  return MG_OK;
}

// Spin on the mailbox; after 2 s of silence (or without a mailbox) synchronise the stream and copy the scalars instead.
int wait_norm(mg_pcg* s, unsigned long long seq, double* rr, double* flag) {
  hipStream_t st = s->eng->stream;
  if (s->mbox_dev) {
    volatile unsigned long long* fl = &s->mbox->seq;
    const double t0 = now_s();
    long spins = 0;
    while (*fl != seq) {
      if ((++spins & 0x3fff) == 0 && now_s() - t0 > 2.0) break;
    }
    if (*fl == seq) {
      std::atomic_thread_fence(std::memory_order_acquire);
      *rr = *(volatile double*)&s->mbox->rr;
      *flag = *(volatile double*)&s->mbox->flag;
      return MG_OK;
    }
  }
  // the posted pair is rewritten by the next norm operation only, which is not queued before this one has been read
  HIPC(&s->err, hipMemcpyAsync(s->h_sc, s->sc + mg::kPcgPostRr, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(&s->err, hipStreamSynchronize(st));
  *rr = s->h_sc[0];
  *flag = s->h_sc[1];
  return MG_OK;
}

int solve_resident(mg_pcg* s, double tol, int max_iter, double* hist, int hist_cap, int* n_iter, int* converged,
                   mg_pcg_stats* stats) {
  hipStream_t st = s->eng->stream;
  const double t0 = now_s();
  const int nx = s->nx, ny = s->ny, ld = s->ld;
  const bool ho = s->order == 4;
  if (ho) {
    // g = R f; r = g - A4 x with a zero ring and the sum of r^2 in one launch.  The ring of f is data of the scheme here and
    // does not enter the norm: the four ring sums are zero
    HIPC(&s->err, hipMemsetAsync(s->sc + kRing0, 0, 4 * sizeof(double), st));
    d_ho_rhs(s->f, s->g, nx, ny, ld, st);
    const int n = d_ho_residual(s->x, s->g, s->r, s->partials, nx, ny, ld, s->hx, s->hy, s->cfg.coeff, s->sigma, st);
    launch_reduce(s->partials, n, s->sc + kRr0, st);
  } else {
    // sum of f^2 over the ring (r = f there in the project's norm), r = f - A x with a zero ring, sum of r^2
    const int win[4][4] = {{0, 1, 0, ny}, {nx - 1, nx, 0, ny}, {1, nx - 1, 0, 1}, {1, nx - 1, ny - 1, ny}};
    for (int k = 0; k < 4; ++k) {
      const int n = d_sumsq(MG_F64, s->f, s->partials, ld, win[k][0], win[k][1], win[k][2], win[k][3], st);
      launch_reduce(s->partials, n, s->sc + kRing0 + k, st);
    }
    if (s->creact) {
      // r = f - (A x + c x) with a zero ring and the sum of r^2 in one launch (the eval kernel, linear kind, w = c)
      int second = 0;
      const int n = d_nl_eval(MG_NL_LINEAR, s->x, nullptr, 0.0, s->varcoef ? s->a : nullptr, s->creact, s->f, nullptr, s->r, nullptr,
                              s->partials, &second, nx, ny, ld, s->hx, s->hy, s->cfg.coeff, s->sigma, 1.0, st);
      launch_reduce(s->partials, n, s->sc + kRr0, st);
    } else {
      if (s->varcoef) d_var(mg::kVarResidual, MG_F64, s->x, s->a, s->f, s->r, nx, ny, ld, s->hx, s->hy, 1.0, s->cfg.coeff, 0, 0, st, s->sigma);
      else d_residual(MG_F64, s->x, s->f, s->r, nx, ny, ld, s->hx, s->hy, s->cfg.coeff, st, false, s->sigma);
      hipLaunchKernelGGL(mg::pcg_zero_ring_kernel, dim3(std::max(1, std::min(64, (2 * (nx + ny) + mg::kBlock - 1) / mg::kBlock))),
                         dim3(mg::kBlock), 0, st, s->r, nx, ny, ld);
      const int n = d_sumsq(MG_F64, s->r, s->partials, ld, 1, nx - 1, 1, ny - 1, st);
      launch_reduce(s->partials, n, s->sc + kRr0, st);
    }
  }
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sc, s->sc + kRing0, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(&s->err, hipStreamSynchronize(st));
  const double ring = (s->h_sc[0] + s->h_sc[1]) + (s->h_sc[2] + s->h_sc[3]);
  const double hh = s->hx * s->hy;
  const double norm0 = std::sqrt(hh * (s->h_sc[4] + ring));

  int n = 0, status = 1, fronts = 0, rc = MG_OK;
  bool conv = false;
  double last = norm0;
  if (norm0 < tol) { conv = true; status = 0; }
  else if ((rc = front(s, 0)) == MG_OK) {
    fronts = 1;
    for (int k = 0; k < max_iter; ++k) {
      unsigned long long seq = 0;
      if ((rc = back(s, &seq)) != MG_OK) break;
      const bool more = k + 1 < max_iter;
      if (s->lookahead && more) { if ((rc = front(s, k + 1)) != MG_OK) break; ++fronts; }
      double rr = 0, flag = 0;
      if ((rc = wait_norm(s, seq, &rr, &flag)) != MG_OK) break;
      if (flag != 0.0) { status = 2; break; }        // p . A p <= 0 or non-finite: x and r are those of iteration k
      last = std::sqrt(hh * (rr + ring));
      if (k < hist_cap) hist[k] = last;
      n = k + 1;
      if (last < tol) { conv = true; status = 0; break; }
      if (!s->lookahead && more) { if ((rc = front(s, k + 1)) != MG_OK) break; ++fronts; }
    }
  }
  if (rc != MG_OK) { (void)hipStreamSynchronize(st); return rc; }
  // the true residual of the returned iterate, by the engine's own residual-norm kernels (what mg_residual_norm computes)
  int second = 0;      // with a reaction field the eval kernel sums over interior cells only: the ring of f is added below
  const int nt = ho ? d_ho_residual(s->x, s->g, nullptr, s->partials, nx, ny, ld, s->hx, s->hy, s->cfg.coeff, s->sigma, st)
      : s->creact ? d_nl_eval(MG_NL_LINEAR, s->x, nullptr, 0.0, s->varcoef ? s->a : nullptr, s->creact, s->f, nullptr, nullptr, nullptr,
                              s->partials, &second, nx, ny, ld, s->hx, s->hy, s->cfg.coeff, s->sigma, 1.0, st)
      : s->varcoef
      ? d_var_residual_norm(MG_F64, s->x, s->a, s->f, s->partials, nx, ny, ld, s->hx, s->hy, s->cfg.coeff, st, s->sigma)
      : d_residual_norm(MG_F64, s->x, s->f, s->partials, nx, ny, ld, s->hx, s->hy, s->cfg.coeff, st, false, s->sigma);
  launch_reduce(s->partials, nt, s->sc + kTrue, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipMemcpyAsync(s->h_sc, s->sc + kTrue, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPC(&s->err, hipStreamSynchronize(st));           // also retires (and thereby drops) a queued lookahead
  const double true_res = std::sqrt(hh * (s->creact ? s->h_sc[0] + ring : s->h_sc[0]));
  const double t1 = now_s();
  double pre_ms = 0;
  const int timed = s->nev == 2 * kTimedIters ? std::min(fronts, kTimedIters) : 0;
  for (int k = 0; k < timed; ++k) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, s->ev[2 * k], s->ev[2 * k + 1]) == hipSuccess) pre_ms += ms;
  }
  if (timed > 0 && fronts > timed) pre_ms *= (double)fronts / timed;
  *n_iter = n;
  *converged = conv ? 1 : 0;
  if (stats) {
    stats->solve_seconds = t1 - t0;
    stats->precond_seconds = pre_ms * 1e-3;
    stats->initial_residual = norm0;
    stats->true_residual = true_res;
    stats->iterations = n;
    stats->status = status;
  }
  (void)last;
  return MG_OK;
}

int solve_args_ok(mg_pcg* s, const char* who, const void* rhs, const void* out, int dtype, double tol, int max_iter, double* hist,
                  int hist_cap, int* n_iter, int* converged) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, std::string(who) + ": NULL solver");
  if (!rhs || !out || !hist || !n_iter || !converged) return sfail(s, MG_ERR_INVALID_VALUE, std::string(who) + ": NULL argument");
  if (!valid_dtype(dtype) || hist_cap < 1 || max_iter < 1 || !(tol == tol))
    return sfail(s, MG_ERR_INVALID_VALUE, std::string(who) + ": bad dtype / hist_cap < 1 / max_iter < 1 / tol is NaN");
  return MG_OK;
}

}  // namespace

namespace mgh {
mg_handle* pcg_engine(mg_pcg* s) { return s ? s->eng : nullptr; }
}  // namespace mgh

extern "C" {

int mg_pcg_create(const mg_config* cfg, int num_cycles, int flexible, mg_pcg** out) {
  if (!cfg || !out) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pcg_create: NULL argument");
  *out = nullptr;
  if (cfg->precision != MG_PREC_DOUBLE && cfg->precision != MG_PREC_SINGLE_MANAGED && cfg->precision != MG_PREC_MIXED_LEVELS)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pcg_create: the preconditioner runs in MG_PREC_DOUBLE, MG_PREC_SINGLE_MANAGED or MG_PREC_MIXED_LEVELS");
  if (cfg->fmg_cycles != 0) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pcg_create: fmg_cycles must be 0 (the preconditioner starts from zero)");
  if (!(cfg->coeff < 0.0)) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pcg_create: conjugate gradients need an SPD operator (coeff < 0)");
  if (num_cycles < 1) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pcg_create: num_cycles < 1");
  mg_handle* eng = nullptr;
  int rc = mg_create(cfg, &eng);
  if (rc != MG_OK) return rc;
  mg_pcg* s = new mg_pcg();
  s->cfg = *cfg;
  s->eng = eng;
  s->nx = cfg->nx; s->ny = cfg->ny;
  s->ld = pitch_elems(MG_F64, cfg->ny);
  s->nyv = field_geom(s->nx, s->ny, s->ld).nyv;
  s->hx = eng->lv[0].hx; s->hy = eng->lv[0].hy;
  s->num_cycles = num_cycles;
  s->flexible = flexible < 0 ? (cfg->smoother != MG_JACOBI || cfg->pre != cfg->post) : (flexible != 0);
  auto bail = [&](int code) { return create_fail(s, release, code); };
  hipStream_t st = eng->stream;
  for (double** p : {&s->x, &s->r, &s->z, &s->q, &s->f, &s->staging, &s->p[0], &s->p[1]})
    if ((rc = alloc_zero(&s->err, (void**)p, field_bytes(s), st)) != MG_OK) return bail(rc);
  s->np = (int)max_partials(s->nx, s->ny);
  if ((rc = alloc_zero(&s->err, (void**)&s->partials, sizeof(double) * 2 * s->np, st)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&s->err, (void**)&s->sc, sizeof(double) * kNumScalars, st)) != MG_OK) return bail(rc);
  if (hipHostMalloc((void**)&s->h_sc, sizeof(double) * kHostScalars) != hipSuccess) { s->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  if (hipHostMalloc((void**)&s->mbox, sizeof(mg::PcgMailbox), hipHostMallocMapped) == hipSuccess &&
      hipHostGetDevicePointer((void**)&s->mbox_dev, s->mbox, 0) == hipSuccess) {
    s->mbox->rr = 0; s->mbox->flag = 0; s->mbox->seq = 0;
  } else {
    s->mbox_dev = nullptr;        // no mapped host memory: copy + stream synchronisation per iteration
  }
  for (; s->nev < 2 * kTimedIters; ++s->nev)
    if (hipEventCreate(&s->ev[s->nev]) != hipSuccess) break;
  if (hipStreamSynchronize(st) != hipSuccess) { s->err = "hipStreamSynchronize failed"; return bail(MG_ERR_HIP); }
  *out = s;
  return MG_OK;
}

int mg_pcg_destroy(mg_pcg* s) {
  return destroy_owned(s, s && s->eng ? s->eng->stream : nullptr, release);
}

const char* mg_pcg_last_error(const mg_pcg* s) { return s ? s->err.c_str() : last_error().c_str(); }

int mg_pcg_set_lookahead(mg_pcg* s, int on) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pcg_set_lookahead: NULL solver");
  s->lookahead = on != 0;
  return MG_OK;
}

int mg_pcg_set_coefficient(mg_pcg* s, const void* a_host_or_null, int host_dtype) {
  if (!s || !valid_dtype(host_dtype)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_pcg_set_coefficient: bad argument");
  if (a_host_or_null && s->order == 4)
    return sfail(s, MG_ERR_STATE, "mg_pcg_set_coefficient: the fourth-order scheme needs constant coefficients (mg_pcg_set_order(2) first)");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  OWNED(mg_set_coefficient(s->eng, a_host_or_null, host_dtype), "preconditioner: ", mg_last_error(s->eng));
  if (!a_host_or_null) { s->varcoef = false; return MG_OK; }
  if (!s->a) { const int rc = alloc_zero(&s->err, (void**)&s->a, field_bytes(s), s->eng->stream); if (rc != MG_OK) return rc; }
  const int rc = put(s, s->a, a_host_or_null, host_dtype);
  if (rc != MG_OK) return rc;
  s->varcoef = true;
  return MG_OK;
}

int mg_pcg_set_order(mg_pcg* s, int order) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pcg_set_order: NULL solver");
  if (order != 2 && order != 4) return sfail(s, MG_ERR_INVALID_VALUE, "mg_pcg_set_order: order must be 2 or 4");
  if (order == 4 && s->varcoef)
    return sfail(s, MG_ERR_STATE, "mg_pcg_set_order: the fourth-order scheme needs constant coefficients (mg_pcg_set_coefficient(NULL) first)");
  if (order == 4 && s->creact)
    return sfail(s, MG_ERR_STATE, "mg_pcg_set_order: the fourth-order scheme takes no reaction field (mg_pcg_set_reaction_device(NULL) first)");
  if (order == 4 && !s->g) {
    HIPC(&s->err, hipSetDevice(s->cfg.device));
    const int rc = alloc_zero(&s->err, (void**)&s->g, field_bytes(s), s->eng->stream);
    if (rc != MG_OK) return rc;
  }
  s->order = order;
  return MG_OK;
}

int mg_pcg_set_shift(mg_pcg* s, double sigma) {
  if (!s || !(sigma >= 0.0) || !std::isfinite(sigma)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_pcg_set_shift: sigma must be finite and >= 0");
  OWNED(mg_set_shift(s->eng, s->creact ? sigma + s->c_ref : sigma), "preconditioner: ", mg_last_error(s->eng));
  s->sigma = sigma;
  return MG_OK;
}

int mg_pcg_set_reaction_device(mg_pcg* s, const double* c_dev_or_null, int ld, double c_ref) {
  if (!s) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pcg_set_reaction_device: NULL solver");
  if (!c_dev_or_null) {
    if (s->creact) OWNED(mg_set_shift(s->eng, s->sigma), "preconditioner: ", mg_last_error(s->eng));
    s->creact = nullptr;
    s->c_ref = 0.0;
    return MG_OK;
  }
  if (s->order == 4)
    return sfail(s, MG_ERR_STATE, "mg_pcg_set_reaction_device: the fourth-order scheme takes no reaction field (mg_pcg_set_order(2) first)");
  if (!(c_ref >= 0.0) || !std::isfinite(c_ref)) return sfail(s, MG_ERR_INVALID_VALUE, "mg_pcg_set_reaction_device: c_ref must be finite and >= 0");
  if (ld != s->ld || !aligned16(c_dev_or_null))
    return sfail(s, MG_ERR_INVALID_VALUE, "mg_pcg_set_reaction_device: the field has the solver's pitch (mg_pitch_elems) and 16-byte alignment");
  OWNED(mg_set_shift(s->eng, s->sigma + c_ref), "preconditioner: ", mg_last_error(s->eng));
  s->creact = c_dev_or_null;
  s->c_ref = c_ref;
  return MG_OK;
}

int mg_pcg_solve_device(mg_pcg* s, const void* rhs_dev, int ld_rhs, void* x_dev, int ld_x, int dtype, double tol, int max_iter,
                        double* hist, int hist_cap, int* n_iter, int* converged, mg_pcg_stats* stats) {
  int rc = solve_args_ok(s, "mg_pcg_solve_device", rhs_dev, x_dev, dtype, tol, max_iter, hist, hist_cap, n_iter, converged);
  if (rc != MG_OK) return rc;
  if (ld_rhs < s->ny || ld_x < s->ny) return sfail(s, MG_ERR_INVALID_VALUE, "mg_pcg_solve_device: pitch smaller than ny");
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  hipStream_t st = s->eng->stream;
  d_convert(dtype, MG_F64, rhs_dev, s->f, s->nx, s->ny, ld_rhs, s->ld, st);
  d_convert(dtype, MG_F64, x_dev, s->x, s->nx, s->ny, ld_x, s->ld, st);
  if ((rc = solve_resident(s, tol, max_iter, hist, hist_cap, n_iter, converged, stats)) != MG_OK) return rc;
  d_convert(MG_F64, dtype, s->x, x_dev, s->nx, s->ny, s->ld, ld_x, st);
  HIPC(&s->err, hipGetLastError());
  HIPC(&s->err, hipStreamSynchronize(st));
  return MG_OK;
}

int mg_pcg_solve(mg_pcg* s, const void* rhs, const void* u0_or_null, void* u_out, int host_dtype, double tol, int max_iter,
                 double* hist, int hist_cap, int* n_iter, int* converged, mg_pcg_stats* stats) {
  int rc = solve_args_ok(s, "mg_pcg_solve", rhs, u_out, host_dtype, tol, max_iter, hist, hist_cap, n_iter, converged);
  if (rc != MG_OK) return rc;
  HIPC(&s->err, hipSetDevice(s->cfg.device));
  hipStream_t st = s->eng->stream;
  if ((rc = put(s, s->f, rhs, host_dtype)) != MG_OK) return rc;
  if (u0_or_null) { if ((rc = put(s, s->x, u0_or_null, host_dtype)) != MG_OK) return rc; }
  else HIPC(&s->err, hipMemsetAsync(s->x, 0, field_bytes(s), st));
  if ((rc = solve_resident(s, tol, max_iter, hist, hist_cap, n_iter, converged, stats)) != MG_OK) return rc;
  return download(&s->err, u_out, host_dtype, s->x, MG_F64, s->ld, s->nx, s->ny, s->staging, st);
}

// ---- the field kernels, call by call (pitch in elements, nullable stream, scratch >= mg_dev_scratch_bytes()) ----
int mg_dev_pcg_direction(int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, const double* a_or_null,
                         const double* z, const double* p_in_or_null, double* p_out, double* q, const double* beta_dev_or_null,
                         void* scratch, double* pq_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld) && sigma >= 0.0, "mg_dev_pcg_direction: bad shape / pitch / shift");
  CHECK_ARG(z && p_out && q && scratch && pq_dev && (!beta_dev_or_null || p_in_or_null), "mg_dev_pcg_direction: NULL pointer");
  CHECK_ARG(p_out != p_in_or_null && p_out != z && q != z && q != p_out && q != p_in_or_null, "mg_dev_pcg_direction: p_out and q are arrays of their own");
  CHECK_ARG(aligned16(z) && aligned16(p_out) && aligned16(q) && aligned16(p_in_or_null) && aligned16(a_or_null), "mg_dev_pcg_direction: unaligned pointer");
  const int n = launch_direction(z, beta_dev_or_null ? p_in_or_null : nullptr, p_out, q, a_or_null, nullptr, beta_dev_or_null,
                                 (double*)scratch, nx, ny, ld, hx, hy, coeff, sigma, (hipStream_t)stream);
  launch_reduce((double*)scratch, n, pq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_pcg_direction_react(int nx, int ny, int ld, double hx, double hy, double coeff, double sigma, const double* a_or_null,
                               const double* c, const double* z, const double* p_in_or_null, double* p_out, double* q,
                               const double* beta_dev_or_null, void* scratch, double* pq_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld) && sigma >= 0.0, "mg_dev_pcg_direction_react: bad shape / pitch / shift");
  CHECK_ARG(c && z && p_out && q && scratch && pq_dev && (!beta_dev_or_null || p_in_or_null), "mg_dev_pcg_direction_react: NULL pointer");
  CHECK_ARG(p_out != p_in_or_null && p_out != z && q != z && q != p_out && q != p_in_or_null && p_out != c && q != c,
            "mg_dev_pcg_direction_react: p_out and q are arrays of their own");
  CHECK_ARG(aligned16(z) && aligned16(p_out) && aligned16(q) && aligned16(p_in_or_null) && aligned16(a_or_null) && aligned16(c),
            "mg_dev_pcg_direction_react: unaligned pointer");
  const int n = launch_direction(z, beta_dev_or_null ? p_in_or_null : nullptr, p_out, q, a_or_null, c, beta_dev_or_null,
                                 (double*)scratch, nx, ny, ld, hx, hy, coeff, sigma, (hipStream_t)stream);
  launch_reduce((double*)scratch, n, pq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_pcg_update(int nx, int ny, int ld, const double* alpha_dev, const double* p, const double* q, double* x, double* r,
                      void* scratch, double* rr_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_pcg_update: bad shape / pitch");
  CHECK_ARG(alpha_dev && p && q && x && r && scratch && rr_dev && x != r, "mg_dev_pcg_update: bad pointer");
  CHECK_ARG(aligned16(p) && aligned16(q) && aligned16(x) && aligned16(r), "mg_dev_pcg_update: unaligned pointer");
  const int n = launch_update(alpha_dev, p, q, x, r, (double*)scratch, nx, ny, ld, (hipStream_t)stream);
  launch_reduce((double*)scratch, n, rr_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_pcg_dots(int nx, int ny, int ld, const double* r, const double* z, const double* q_or_null, void* scratch,
                    double* rz_dev, double* zq_dev, void* stream) {
  CHECK_ARG(nx >= 3 && ny >= 3 && ld_ok_f64(ny, ld), "mg_dev_pcg_dots: bad shape / pitch");
  CHECK_ARG(r && z && scratch && rz_dev && (!q_or_null || zq_dev), "mg_dev_pcg_dots: bad pointer");
  CHECK_ARG(aligned16(r) && aligned16(z) && aligned16(q_or_null), "mg_dev_pcg_dots: unaligned pointer");
  const int n = launch_dots(r, z, q_or_null, (double*)scratch, 1024, nx, ny, ld, (hipStream_t)stream);   // <= 1024 workgroups, scratch >= 2048 doubles
  launch_reduce((double*)scratch, n, rz_dev, (hipStream_t)stream);
  if (q_or_null) launch_reduce((double*)scratch + 1024, n, zq_dev, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

int mg_dev_pcg_scalars(int op, const double* partials_a, int na, const double* partials_b, int nb, double* scalars, void* stream) {
  CHECK_ARG(op >= mg::kPcgBeta0 && op <= mg::kPcgNormOp && partials_a && na >= 1 && nb >= 0 && (nb == 0 || partials_b) && scalars,
            "mg_dev_pcg_scalars: bad argument");
  launch_scalars(op, partials_a, na, partials_b, nb, scalars, nullptr, 0, (hipStream_t)stream);
  HIPC(nullptr, hipGetLastError());
  return MG_OK;
}

}  // extern "C"
