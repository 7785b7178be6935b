// The solve loop of libmghip.so: the norm path (device reduction, host mailbox), the adaptive precision policy
// (core/precision.py), and mg_iterate / mg_solve with speculative launching.  Host code: the cycles are mg_engine.hip's,
// every kernel is behind mg_launch.hpp.
#include "mg_launch.hpp"

#include <atomic>
#include <cstring>

namespace mgh {

// ---- the norm path -------------------------------------------------------------------------
// Reduce `n` partial sums and bring the scalar to the host.  Fast path: the kernel posts it to the mapped
// mailbox and the host spins on the sequence number (a few microseconds after the kernel retires); if nothing
// arrives within 2 s, or there is no mailbox, fall back to copy + stream synchronisation.
// launch half (mailbox only): returns the sequence number to wait for
static unsigned long long reduce_post(mg_handle* h, int n) {
  const unsigned long long seq = ++h->mbox_seq;
  launch_reduce(h->partials, n, h->d_scalar, h->stream, h->mbox_dev, seq);
  return seq;
}

// Spin until the mailbox carries `seq`; after 2 s of silence synchronise the stream instead (slow or faulted device: this
// reports the error, if any).  *arrived: the mailbox carries `seq` and *value is its scalar.
static int mailbox_wait(mg_handle* h, unsigned long long seq, double* value, bool* arrived) {
  volatile unsigned long long* flag = &h->mbox->seq;
  const double t0 = now_s();
  long spins = 0;
  while (*flag != seq) {
    if ((++spins & 0x3fff) == 0 && now_s() - t0 > 2.0) break;
  }
  if (*flag != seq) HIPC(&h->err, hipStreamSynchronize(h->stream));
  *arrived = *flag == seq;
  if (!*arrived) return MG_OK;
  std::atomic_thread_fence(std::memory_order_acquire);
  *value = *(volatile double*)&h->mbox->value;
  return MG_OK;
}

static int reduce_wait(mg_handle* h, unsigned long long seq, double* value) {
  bool arrived = false;
  const int rc = mailbox_wait(h, seq, value, &arrived);
  if (rc != MG_OK) return rc;
  return arrived ? MG_OK : fail(&h->err, MG_ERR_HIP, "norm mailbox was never written");
}

static int reduce_to_host(mg_handle* h, int n, double* value) {
  if (h->mbox_dev) {
    const unsigned long long seq = reduce_post(h, n);
    HIPC(&h->err, hipGetLastError());
    bool arrived = false;
    const int rc = mailbox_wait(h, seq, value, &arrived);
    if (rc != MG_OK || arrived) return rc;
  } else {
    launch_reduce(h->partials, n, h->d_scalar, h->stream);
  }
  HIPC(&h->err, hipMemcpyAsync(h->h_scalar, h->d_scalar, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  *value = *h->h_scalar;
  return MG_OK;
}

// the discrete L2 norm on level v from a sum of squares over its cells: over all of them, or over the interior cells plus
// `ring`, the sum over the boundary ring
static double h_norm(const Level& v, double ss) { return std::sqrt(v.hx * v.hy * ss); }
static double h_norm(const Level& v, double ss, double ring) { return std::sqrt(v.hx * v.hy * (ss + ring)); }

static int fine_norm(mg_handle* h, double* out) {
  Level& v = h->lv[0];
  double ss = 0;
  int rc;
  if (h->cfg.precision == MG_PREC_DEFECT) {       // ||f - A u|| of the fp64 iterate (the fp32 rhs is rewritten with the same defect)
    if (h->varcoef) return fail(&h->err, MG_ERR_INVALID_VALUE, "defect correction runs the constant-coefficient operator");
    if ((rc = reduce_to_host(h, launch_defect(h, false), &ss)) != MG_OK) return rc;
    *out = h_norm(v, ss);
    return MG_OK;
  }
  const int dt = h->level_dtype(0);
  if (h->norm_partials > 0 && h->ring_sumsq[dt] >= 0) {   // the up leg of the last cycle already summed r^2 over the interior cells
    if ((rc = reduce_to_host(h, h->norm_partials, &ss)) != MG_OK) return rc;
    *out = h_norm(v, ss, h->ring_sumsq[dt]);
    return MG_OK;
  }
  // the norm of the zero iterate is ||f||, whatever the operator: computed once per right-hand side (by the same kernel, so
  // with the same bits) and remembered -- repeated solves of one right-hand side from the zero guess skip the pass
  if (h->iterate_zero && h->zero_norm_gen[dt] == h->rhs_gen) { *out = h->zero_norm_val[dt]; return MG_OK; }
  const int n = h->varcoef
      ? d_var_residual_norm(dt, v.u[dt], v.a[dt], v.rhs[dt], h->partials, v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.coeff, h->stream,
                            h->sigma)
      : d_residual_norm(dt, v.u[dt], v.rhs[dt], h->partials, v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.coeff, h->stream, true,
                        h->sigma);
  if ((rc = reduce_to_host(h, n, &ss)) != MG_OK) return rc;
  *out = h_norm(v, ss);
  if (h->iterate_zero) { h->zero_norm_gen[dt] = h->rhs_gen; h->zero_norm_val[dt] = *out; }
  return MG_OK;
}

// ---- the adaptive precision policy ---------------------------------------------------------
// in-device cast of the fine iterate when the adaptive policy changes the working precision
// iterate_is_zero: the iterate is zero everywhere and the caller starts the coming cycle from the zero iterate without
// reading it (cycle_fused(..., zero_u = true)): only the (zero) boundary rings of the two buffers are written.
static int switch_phase(mg_handle* h, int to, bool iterate_is_zero = false) {
  if (h->cfg.precision != MG_PREC_ADAPTIVE || to == h->phase) return MG_OK;
  Level& v = h->lv[0];
  const int from = h->phase;
  if (h->L() > 1) {   // with a single level the only level is the coarsest and lives in the grid dtype
    if (iterate_is_zero) d_convert_ring(from, to, v.u[from], v.u[to], v.nx, v.ny, v.ld[from], v.ld[to], h->stream);
    else d_convert(from, to, v.u[from], v.u[to], v.nx, v.ny, v.ld[from], v.ld[to], h->stream);
    // the ping-pong partner only needs the boundary ring (the first leg rewrites its interior)
    if (v.t[to]) d_convert_ring(from, to, v.u[from], v.t[to], v.nx, v.ny, v.ld[from], v.ld[to], h->stream);
  }
  h->phase = to;
  h->norm_partials = 0;
  inject_rings_once(h, to);
  return MG_OK;
}

// core/precision.py:189-246 should_promote_precision, on the last five residual norms
static bool stagnating(const std::vector<double>& hist) {
  if (hist.size() < 5) return false;
  const double* r = hist.data() + hist.size() - 5;
  double sum = 0; int n = 0;
  for (int i = 1; i < 5; ++i) if (r[i - 1] > 0) { sum += r[i] / r[i - 1]; ++n; }
  if (n) {
    if (sum / n > 0.9) return true;
    double rel = 0; int m = 0;
    for (int i = 1; i < 5; ++i) if (r[i - 1] > 0) { rel += std::fabs(r[i] - r[i - 1]) / r[i - 1]; ++m; }
    if (m && rel / m < 1e-3) return true;
  }
  bool inc = true;
  for (int i = 1; i < 5; ++i) inc = inc && (r[i] >= r[i - 1] * 0.99);
  return inc;
}

constexpr double kEps32 = 5.9604644775390625e-8;      // 2^-24

// The residual an fp32 iterate can reach: every cell's r = f - A u carries the rounding of diag(A) u, so ||r||_h settles at
// about eps32 * diag(A) * ||u||_h (measured: 1.8 against 2.0 at 4097^2, 1.9e-3 against 1.95e-3 at 129^2) -- h^-2 times the
// round-off of u.  Within a factor 2 of it another fp32 cycle cannot lower the residual: the policy promotes at once
// instead of waiting for the five-norm stagnation window (core/precision.py:189-246) to fill with a flat history.
static bool at_fp32_floor(const mg_handle* h, double rn) { return h->fp32_floor > 0.0 && rn <= 2.0 * h->fp32_floor; }

// Before the first cycle the same floor can be bounded from above: ||u|| <= ||f|| / lambda_min with lambda_min =
// |coeff| pi^2 (1/Lx^2 + 1/Ly^2) + sigma of the Dirichlet problem, so floor / ||r_0|| <= eps32 diag(A) / lambda_min -- a number
// that depends on the grid only (1.2e-8 / h^2 on the unit square: 0.2 at 4097^2, 0.013 at 1025^2).  Cycles contract ||r|| by
// ~0.15, so the fp32 phase is good for log(that) / log(0.15) cycles; entering and leaving it costs about one cycle's saving
// (two ring conversions, the ||u|| pass, the cast of the iterate, no speculative front part across either switch): the policy
// takes the fp32 phase only when it is good for at least two cycles, and stays in double otherwise -- an adaptive solve then
// never loses to a double one.
static bool fp32_phase_pays(const mg_handle* h) {
  const Level& v = h->lv[0];
  const double lx = h->cfg.x1 - h->cfg.x0, ly = h->cfg.y1 - h->cfg.y0, pi = 3.14159265358979323846;
  const double lam = std::fabs(h->cfg.coeff) * pi * pi * (1.0 / (lx * lx) + 1.0 / (ly * ly)) + h->sigma;
  const double ratio = kEps32 * coefs(v.hx, v.hy, h->sigma).diag / lam;
  return ratio > 0.0 && std::log(ratio) / std::log(0.15) >= 2.0;
}

// The one-way adaptive rule (documented in mghip.h) has not promoted for good yet ...
static bool one_way_pending(const mg_handle* h) {
  return h->cfg.precision == MG_PREC_ADAPTIVE && !h->cfg.adaptive_reference_rule && !h->promoted;
}
// ... and its fp32 phase is still open: the solve runs in fp32 and the policy may yet promote it
static bool fp32_phase_open(const mg_handle* h) { return one_way_pending(h) && h->phase == MG_F32; }

// core/precision.py:270-302 update_precision (+ the one-way variant documented in mghip.h): the precision the coming
// cycle runs in.  Pure -- `*promote` says whether taking the decision also ends the adaptive phase for good.
static int adapt_target(const mg_handle* h, double rn, bool* promote) {
  *promote = false;
  if (h->cfg.precision != MG_PREC_ADAPTIVE) return h->phase;
  const double thr = h->cfg.switch_threshold;
  double pts = 0;
  for (auto& l : h->lv) pts += (double)l.nx * l.ny;
  const double mem = pts * esize(h->phase) * 4.0;                       // precision.py:136-153
  const bool mem_down = mem > h->cfg.memory_threshold_gb * 1024.0 * 1024.0 * 1024.0;
  int to = h->phase;
  if (h->cfg.adaptive_reference_rule) {
    if (mem_down || (h->phase == MG_F64 && rn > thr * 100)) { if (h->phase == MG_F64) to = MG_F32; }
    else if (h->phase == MG_F32 && rn < thr * 10) to = MG_F64;
  } else if (one_way_pending(h)) {
    if (h->phase == MG_F64 && (mem_down || (rn > thr * 100 && fp32_phase_pays(h))) && h->adapt_hist.empty()) to = MG_F32;
    else if (fp32_phase_open(h) && (rn < thr * 10 || stagnating(h->adapt_hist) || at_fp32_floor(h, rn))) { to = MG_F64; *promote = true; }
  }
  return to;
}

static int adapt(mg_handle* h, double rn, bool iterate_is_zero = false) {
  bool promote = false;
  const int to = adapt_target(h, rn, &promote);
  if (promote) {
    h->promoted = true;
    h->switch_reason = rn < h->cfg.switch_threshold * 10 ? 1 : (stagnating(h->adapt_hist) ? 2 : 3);
  } else if (one_way_pending(h) && h->phase == MG_F64 && to == MG_F64 && h->adapt_hist.empty() &&
             rn > h->cfg.switch_threshold * 100) {
    h->switch_reason = 4;                                  // the fp32 phase was declined a priori (fp32_phase_pays)
    h->promoted = true;                                    // ... for good: the rest of the solve is a double solve
  }
  return switch_phase(h, to, iterate_is_zero);
}

// Once per solve, after the first fp32 cycle (no front part of the next cycle is queued yet): ||u||_h of the fp32 iterate
// -> the residual this precision can reach (at_fp32_floor)
static int measure_fp32_floor(mg_handle* h) {
  Level& v0 = h->lv[0];
  const int np = d_sumsq(MG_F32, v0.u[MG_F32], h->partials, v0.ld[MG_F32], 0, v0.nx, 0, v0.ny, h->stream);
  double su = 0;
  const int rc = reduce_to_host(h, np, &su);
  if (rc != MG_OK) return rc;
  h->norm_partials = 0;                     // `partials` no longer holds this cycle's sum of r^2
  h->fp32_floor = kEps32 * coefs(v0.hx, v0.hy, h->sigma).diag * h_norm(v0, su);
  return MG_OK;
}

// ---- the solve loop --------------------------------------------------------------------------
struct Solve {             // one mg_iterate / mg_solve call
  mg_handle* h;
  double tol; int max_iter; double* hist; int hist_cap; int32_t* prec_hist; mg_stats* st;
  double t0 = 0;           // start of the solve
  double rn = 0;           // the latest residual norm
  double prev_rn = 0;      // the norm before `rn` (speculation heuristics)
  int it = 0, conv = 0, switches = 0;
  bool can_spec = false;   // speculative launching applies to this solve
  bool zero_first = false; // the first cycle's level-0 down leg starts from the zero iterate without reading it
  bool spec = false;       // the front part of the coming cycle is already queued
};

static int cycle_rc(mg_handle* h, int rc) {
  return rc == MG_OK ? MG_OK : fail(&h->err, rc, "cycle: unsupported precision combination");
}

// a queued front part is dropped: one pointer swap is undone and lv[0].u is the iterate again
static void undo_front(Solve& s) {
  Level& v0 = s.h->lv[0];
  const int d0 = s.h->level_dtype(0);
  std::swap(v0.u[d0], v0.t[d0]);
  s.spec = false;
}

// norm and precision code of cycle s.it into the histories; true when the norm meets the tolerance
static bool record(Solve& s, int prec_code) {
  if (s.it <= s.hist_cap) s.hist[s.it - 1] = s.rn;
  if (s.prec_hist && s.it <= s.hist_cap) s.prec_hist[s.it - 1] = prec_code;
  if (s.rn < s.tol) s.conv = 1;                                 // solvers/base.py:134 (absolute)
  return s.conv != 0;
}

static int solve_begin(Solve& s) {
  mg_handle* h = s.h;
  // reset the adaptive state (PrecisionManager starts every solve from default_precision = double)
  if (h->cfg.precision == MG_PREC_ADAPTIVE) {
    const int rc0 = switch_phase(h, MG_F64);
    if (rc0 != MG_OK) return rc0;
    h->promoted = false;
    h->adapt_hist.clear();
  }
  h->fp32_floor = 0.0;
  h->switch_reason = 0;
  h->span_ring[0] = h->span_ring[1] = false;
  for (auto& l : h->lv) l.timings[0] = l.timings[1] = l.timings[2] = 0;
  s.t0 = now_s();
  const int rc = fine_norm(h, &s.rn);
  if (rc != MG_OK) return rc;
  const bool zero_start = h->iterate_zero;    // the first cycle may start from the zero iterate without reading it
  h->iterate_zero = false;                    // cycles follow
  s.st->initial_residual = s.rn;
  // Speculative launching: while the norm of cycle `it` travels to the host, the FRONT part of cycle it+1 (level-0
  // down leg and everything below it) is already queued -- it never touches the buffer holding the iterate of
  // cycle `it`.  If that norm ends the solve or changes the working precision, the front part is simply dropped
  // (one pointer swap is undone); results are identical to the one-cycle-at-a-time loop.
  s.can_spec = h->cfg.speculate != 0 && h->fused() && h->L() > 1 && h->mbox_dev && h->cfg.pre <= 2 &&
               h->cfg.post <= 2 && !h->cfg.profile && h->ring_sumsq[0] >= 0 && h->ring_sumsq[1] >= 0;
  s.zero_first = zero_start && s.can_spec && h->cfg.pre >= 1;
  return MG_OK;
}

// coarse sweep count, stats and the caller's counters
static int solve_end(Solve& s, int* n_iter, int* converged) {
  mg_handle* h = s.h;
  if (s.spec) undo_front(s);
  if (s.it > s.max_iter) s.it = s.max_iter;
  HIPC(&h->err, hipMemcpyAsync(h->h_int, h->d_int, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  s.st->last_coarse_sweeps = *h->h_int;
  s.st->solve_seconds = now_s() - s.t0;
  s.st->precision_switches = s.switches;
  s.st->switch_reason = h->switch_reason;
  s.st->fp32_floor = h->fp32_floor;
  if (n_iter) *n_iter = s.it;
  if (converged) *converged = s.conv;
  return MG_OK;
}

// Outer loop of defect correction: fine_norm left the defect of the initial iterate in the fp32 rhs; each step runs one
// fp32 cycle from zero on it, then ONE pass that updates the fp64 iterate, forms the next defect and its norm.
static int defect_loop(Solve& s) {
  mg_handle* h = s.h;
  if (h->L() < 2) return fail(&h->err, MG_ERR_INVALID_VALUE, "defect correction needs at least two levels");
  inject_rings(h, h->phase);                      // zero rings of every coarse rhs (the error vanishes on the boundary)
  for (s.it = 1; s.it <= s.max_iter; ++s.it) {
    int rc = cycle_rc(h, defect_cycle(h));
    if (rc != MG_OK) return rc;
    double ss = 0;
    if ((rc = reduce_to_host(h, launch_defect(h, true), &ss)) != MG_OK) return rc;
    s.rn = h_norm(h->lv[0], ss);
    if (record(s, 3)) break;
  }
  return MG_OK;
}

// the policy's decision on the norm of the cycle before (solvers/multigrid.py:224-227)
static int adapt_step(Solve& s) {
  mg_handle* h = s.h;
  const int before = h->phase;
  int rc;
  if (s.spec && h->cfg.precision == MG_PREC_ADAPTIVE) {
    // would the policy switch?  After the speculative swap lv[0].u is the WRONG buffer to convert: drop the queued
    // front part first, then switch from the untouched iterate
    bool promote = false;
    if (adapt_target(h, s.rn, &promote) != h->phase) undo_front(s);
    rc = adapt(h, s.rn);
  } else {
    // a solve from the zero guess: the first cycle's level-0 down leg runs from the zero iterate without reading it
    // (the kernels' ZERO_INIT form, as on every coarse level), so a precision switch before it has nothing to convert
    rc = adapt(h, s.rn, s.zero_first && s.it == 1);
  }
  if (rc == MG_OK && h->phase != before) {
    ++s.switches;
    if (h->cfg.adaptive_reference_rule == 0) h->adapt_hist.clear();
  }
  return rc;
}

static int plain_step(Solve& s) {
  const int rc = cycle_rc(s.h, run_cycle(s.h));
  return rc != MG_OK ? rc : fine_norm(s.h, &s.rn);             // multigrid.py:233
}

// A queued front part is wasted work when the norm in flight switches the working precision (its level-0 leg runs in the
// old one) or ends the solve: would the front part of cycle it + 1, queued behind cycle it, be wasted?
static bool front_would_be_wasted(const Solve& s) {
  const mg_handle* h = s.h;
  // extrapolate the norm in flight from the last two of the fp32 phase: no speculation across a switch the policy would
  // take on it (threshold reached, or the stagnation window filling up with a flat history)
  if (fp32_phase_open(h) && h->adapt_hist.size() >= 2) {
    const double prev = h->adapt_hist[h->adapt_hist.size() - 2];
    const double rho = prev > 0 ? std::min(1.0, s.rn / prev) : 1.0;
    std::vector<double> guess(h->adapt_hist);
    guess.push_back(s.rn * rho);
    if (s.rn * rho < h->cfg.switch_threshold * 10 || stagnating(guess)) return true;
  }
  // ... nor across the end of the solve: the norm in flight, extrapolated the same way, meets the tolerance
  if (s.it >= 2 && s.prev_rn > 0 && s.rn * std::min(1.0, s.rn / s.prev_rn) < s.tol) return true;
  // ... nor before the fp32 residual floor of this solve is known: it is evaluated from the iterate this cycle leaves,
  // right after its norm (measure_fp32_floor), and usually ends the fp32 phase there
  return fp32_phase_open(h) && h->fp32_floor == 0.0;
}

// cycle s.it with its norm in flight while the front part of cycle it + 1 is queued
static int spec_step(Solve& s) {
  mg_handle* h = s.h;
  int rc;
  h->norm_partials = 0;
  if (!s.spec && (rc = cycle_rc(h, cycle_fused(h, 0, s.zero_first && s.it == 1, kPartFront))) != MG_OK) return rc;
  s.spec = false;
  const bool go = s.it < s.max_iter && !front_would_be_wasted(s);     // queue the front part of cycle it + 1 behind this cycle
  unsigned long long seq;
  if (go && span_ok(h)) {
    // up leg of this cycle and down leg of the next in one level-0 launch (cycle_span).  The iterate of THIS cycle is
    // stored unless nothing can end the solve or change the precision on its norm: no tolerance to meet (tol <= 0, a
    // fixed number of cycles) and no adaptive switch pending
    const bool may_switch = h->cfg.precision == MG_PREC_ADAPTIVE && (!h->promoted || h->cfg.adaptive_reference_rule);
    const bool keep_mid = s.tol > 0 || may_switch;
    if ((rc = cycle_rc(h, cycle_span(h, keep_mid))) != MG_OK) return rc;
    seq = reduce_post(h, h->norm_partials);
    if ((rc = cycle_rc(h, cycle_below_fine(h))) != MG_OK) return rc;
    s.spec = true;
  } else {
    if ((rc = cycle_rc(h, cycle_fused(h, 0, false, kPartBack))) != MG_OK) return rc;
    seq = reduce_post(h, h->norm_partials);
    if (go) {
      if ((rc = cycle_rc(h, cycle_fused(h, 0, false, kPartFront))) != MG_OK) return rc;
      s.spec = true;
    }
  }
  HIPC(&h->err, hipGetLastError());
  double ss = 0;
  if ((rc = reduce_wait(h, seq, &ss)) != MG_OK) return rc;
  s.prev_rn = s.rn;
  s.rn = h_norm(h->lv[0], ss, h->ring_sumsq[h->level_dtype(0)]);
  if (s.spec) h->norm_partials = 0;        // `partials` still describes cycle `it`, but lv[0].u is ahead of it
  return MG_OK;
}

static int cycle_loop(Solve& s) {
  mg_handle* h = s.h;
  for (s.it = 1; s.it <= s.max_iter; ++s.it) {
    int rc = adapt_step(s);
    if (rc != MG_OK) return rc;
    if ((rc = s.can_spec ? spec_step(s) : plain_step(s)) != MG_OK) return rc;
    h->adapt_hist.push_back(s.rn);
    if (fp32_phase_open(h) && h->fp32_floor == 0.0 && !s.spec && (rc = measure_fp32_floor(h)) != MG_OK) return rc;
    if (record(s, h->cfg.precision == MG_PREC_MIXED_LEVELS ? 2 : h->level_dtype(0))) break;
  }
  return MG_OK;
}

static int iterate_impl(mg_handle* h, double tol, int max_iter, double* hist, int hist_cap, int* n_iter,
                        int* converged, int32_t* prec_hist, mg_stats* st) {
  Solve s{h, tol, max_iter, hist, hist_cap, prec_hist, st};
  int rc = solve_begin(s);
  if (rc != MG_OK) return rc;
  if ((rc = h->cfg.precision == MG_PREC_DEFECT ? defect_loop(s) : cycle_loop(s)) != MG_OK) return rc;
  return solve_end(s, n_iter, converged);
}

}  // namespace mgh

using namespace mgh;

extern "C" {

int mg_residual_norm(mg_handle* h, double* out) {
  if (!h || !out) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_residual_norm: bad argument");
  if (!h->have_rhs) return fail(&h->err, MG_ERR_STATE, "mg_residual_norm before mg_set_rhs");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  return fine_norm(h, out);
}

int mg_set_working_precision(mg_handle* h, int dtype) {
  if (!h || !valid_dtype(dtype)) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "bad argument");
  if (h->cfg.precision != MG_PREC_ADAPTIVE) return fail(&h->err, MG_ERR_STATE, "working precision is fixed unless precision = MG_PREC_ADAPTIVE");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  return switch_phase(h, dtype);
}

int mg_iterate(mg_handle* h, double tol, int max_iter, double* hist, int hist_cap, int* n_iter, int* converged,
               int32_t* prec_hist, mg_stats* stats) {
  if (!h) return fail(nullptr, MG_ERR_STATE, "Multigrid not properly setup or grid mismatch");
  if (max_iter < 1 || (hist_cap > 0 && !hist)) return fail(&h->err, MG_ERR_INVALID_VALUE, "mg_iterate: bad argument");
  if (!h->have_rhs) return fail(&h->err, MG_ERR_STATE, "mg_iterate before mg_set_rhs");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  mg_stats st;
  std::memset(&st, 0, sizeof(st));
  const int rc = iterate_impl(h, tol, max_iter, hist, hist_cap, n_iter, converged, prec_hist, &st);
  if (stats) *stats = st;
  return rc;
}

int mg_solve(mg_handle* h, const void* rhs, const void* u0, void* u_out, int host_dtype, double tol, int max_iter,
             double* hist, int hist_cap, int* n_iter, int* converged, int32_t* prec_hist, mg_stats* stats) {
  if (!h) return fail(nullptr, MG_ERR_STATE, "Multigrid not properly setup or grid mismatch");
  if (!rhs || !u_out || !valid_dtype(host_dtype) || max_iter < 1 || (hist_cap > 0 && !hist))
    return fail(&h->err, MG_ERR_INVALID_VALUE, "mg_solve: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  mg_stats st;
  std::memset(&st, 0, sizeof(st));
  if (h->cfg.precision == MG_PREC_ADAPTIVE) h->phase = MG_F64;   // upload into the fp64 iterate
  double t0 = now_s();
  int rc = set_rhs_impl(h, rhs, host_dtype);
  if (rc != MG_OK) return rc;
  rc = set_u_impl(h, u0, host_dtype);
  if (rc != MG_OK) return rc;
  st.h2d_seconds = now_s() - t0;
  if (h->cfg.fmg_cycles > 0 && !u0) {                        // gpu/gpu_solver.py:583: FMG only without an initial guess
    rc = h->cfg.precision == MG_PREC_DEFECT ? defect_fmg(h, h->cfg.fmg_cycles) : fmg_init(h, h->cfg.fmg_cycles);
    if (rc != MG_OK) return fail(&h->err, rc, "fmg: unsupported precision combination");
  }
  rc = iterate_impl(h, tol, max_iter, hist, hist_cap, n_iter, converged, prec_hist, &st);
  if (rc != MG_OK) return rc;
  t0 = now_s();
  Level& v = h->lv[0];
  const int dt = h->iterate_dtype();
  rc = download(&h->err, u_out, host_dtype, v.u[dt], dt, v.ld[dt], v.nx, v.ny, h->staging, h->stream);
  if (rc != MG_OK) return rc;
  st.d2h_seconds = now_s() - t0;
  if (stats) *stats = st;
  return MG_OK;
}

}  // extern "C"
