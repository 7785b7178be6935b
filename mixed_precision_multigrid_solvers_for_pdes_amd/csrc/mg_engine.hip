// The engine of libmghip.so: the handle's lifecycle, the V/W/F-cycle driver (reference: solvers/multigrid.py:184-337,
// gpu/gpu_solver.py:186-446), coarse-tail planning, the full-multigrid start, and the handle-bound entry points of the
// C ABI (include/mghip.h) other than the solve loop's (mg_solve.hip).  Host code: every kernel is behind mg_launch.hpp.
// No Python, no torch types: plain pointers and sizes.
#include "mg_launch.hpp"

#include <cstring>

namespace mgh {

std::string& last_error() {
  thread_local std::string msg;
  return msg;
}

// ------------------------------------------------------------------ host <-> device helpers -----
int upload(std::string* err, void* dev, int ddt, int ld, const void* host, int hdt, int nx, int ny, void* staging,
           hipStream_t st) {
  if (ddt == hdt) {
    HIPC(err, hipMemcpy2DAsync(dev, (size_t)ld * esize(ddt), host, (size_t)ny * esize(hdt), (size_t)ny * esize(hdt), nx,
                               hipMemcpyHostToDevice, st));
  } else {   // upload in the host dtype into staging (pitch = ld of the HOST dtype), then cast on the device
    const int lds = pitch_elems(hdt, ny);
    HIPC(err, hipMemcpy2DAsync(staging, (size_t)lds * esize(hdt), host, (size_t)ny * esize(hdt), (size_t)ny * esize(hdt),
                               nx, hipMemcpyHostToDevice, st));
    d_convert(hdt, ddt, staging, dev, nx, ny, lds, ld, st);
  }
  HIPC(err, hipStreamSynchronize(st));
  return MG_OK;
}

int download(std::string* err, void* host, int hdt, const void* dev, int ddt, int ld, int nx, int ny, void* staging,
             hipStream_t st) {
  if (ddt == hdt) {
    HIPC(err, hipMemcpy2DAsync(host, (size_t)ny * esize(hdt), dev, (size_t)ld * esize(ddt), (size_t)ny * esize(hdt), nx,
                               hipMemcpyDeviceToHost, st));
  } else {
    const int lds = pitch_elems(hdt, ny);
    d_convert(ddt, hdt, dev, staging, nx, ny, ld, lds, st);
    HIPC(err, hipMemcpy2DAsync(host, (size_t)ny * esize(hdt), staging, (size_t)lds * esize(hdt), (size_t)ny * esize(hdt),
                               nx, hipMemcpyDeviceToHost, st));
  }
  HIPC(err, hipStreamSynchronize(st));
  return MG_OK;
}

// cfg.fused: 0 one launch per operator, 1 LDS-tiled fused legs, 2 register-blocked legs on the large levels (LDS-tiled
// below), 3 register-blocked legs on every level
static int rb_mode(const mg_handle* h) { return h->cfg.fused == 2 ? 1 : (h->cfg.fused == 3 ? 2 : 0); }

// the fused-leg geometry of level l (dtype dt) with level l + 1 (dtype dc) below it; dc < 0: no coarse level (sweeps)
static LegGeom leg_geom(const mg_handle* h, int l, int dt, int dc) {
  const Level& f = h->lv[l];
  LegGeom g;
  g.nx = f.nx; g.ny = f.ny; g.ld = f.ld[dt]; g.hx = f.hx; g.hy = f.hy;
  if (dc >= 0) { const Level& c = h->lv[l + 1]; g.nxc = c.nx; g.nyc = c.ny; g.ldc = c.ld[dc]; }
  g.omega = h->cfg.omega; g.coeff = h->cfg.coeff; g.poff = h->cfg.colour_offset; g.fine = l == 0;
  g.sigma = h->sigma;
  g.rb = rb_mode(h);
  if (h->varcoef) { g.acoef = f.a[dt]; g.rdiag = f.rd[dt]; }
  return g;
}

int alloc_zero(std::string* err, void** p, size_t bytes, hipStream_t st) {
  HIPC(err, hipMalloc(p, bytes));
  HIPC(err, hipMemsetAsync(*p, 0, bytes, st));
  return MG_OK;
}

static void release(mg_handle* h) {
  for (auto& l : h->lv)
    for (int d = 0; d < 2; ++d)
      for (void* p : {l.u[d], l.t[d], l.s[d], l.rhs[d], l.r[d], l.a[d], l.rd[d]})
        if (p) (void)hipFree(p);
  for (auto& l : h->lv)
    for (auto& per_dtype : l.lp)
      for (mg_line_plan*& p : per_dtype) { line_plan_free(p); p = nullptr; }
  if (h->d_tail_ops) (void)hipFree(h->d_tail_ops);
  if (h->partials) (void)hipFree(h->partials);
  if (h->d_scalar) (void)hipFree(h->d_scalar);
  if (h->d_int) (void)hipFree(h->d_int);
  if (h->d_minv) (void)hipFree(h->d_minv);
  if (h->staging) (void)hipFree(h->staging);
  if (h->mbox) (void)hipHostFree(h->mbox);
  if (h->h_scalar) (void)hipHostFree(h->h_scalar);
  if (h->h_int) (void)hipHostFree(h->h_int);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
}

// reciprocal diagonals of every level and precision, for the current coefficient and shift (variable coefficients only)
static void refresh_rdiag(mg_handle* h) {
  if (!h->varcoef || h->rd_sigma == h->sigma) return;
  for (auto& v : h->lv)
    for (int dt = 0; dt < 2; ++dt)
      if (v.a[dt] && v.rd[dt]) d_rdiag(dt, v.a[dt], v.rd[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->sigma, h->stream);
  h->rd_sigma = h->sigma;
}

// ---- the cycle -----------------------------------------------------------------------------
struct StageTimer {
  mg_handle* h; Level* lv; int slot; double t0 = 0;
  StageTimer(mg_handle* h_, Level* lv_, int slot_) : h(h_), lv(lv_), slot(slot_) {
    if (h->cfg.profile) { (void)hipStreamSynchronize(h->stream); t0 = now_s(); }
  }
  ~StageTimer() {
    if (h->cfg.profile) { (void)hipStreamSynchronize(h->stream); lv->timings[slot] += now_s() - t0; }
  }
};

static void smooth(mg_handle* h, int l, int nu) {
  Level& v = h->lv[l];
  const int dt = h->level_dtype(l);
  StageTimer tm(h, &v, 0);
  for (int s = 0; s < nu; ++s) {
    if (h->varcoef && h->cfg.smoother == MG_JACOBI) {
      d_var(mg::kVarJacobi, dt, v.u[dt], v.a[dt], v.rhs[dt], v.t[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.omega,
                            h->cfg.coeff, 0, 0, h->stream, h->sigma);
      std::swap(v.u[dt], v.t[dt]);
    } else if (h->varcoef && h->cfg.smoother == MG_RBGS) {
      for (int colour = 0; colour < 2; ++colour)
        d_var(mg::kVarRbgs, dt, v.u[dt], v.a[dt], v.rhs[dt], v.u[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.omega,
                            h->cfg.coeff, colour, h->cfg.colour_offset, h->stream, h->sigma);
    } else if (h->cfg.smoother == MG_JACOBI) {
      d_jacobi(dt, v.u[dt], v.rhs[dt], v.t[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.omega, h->stream, l == 0, h->sigma);
      std::swap(v.u[dt], v.t[dt]);
    } else if (h->cfg.smoother == MG_RBGS) {
      for (int colour = 0; colour < 2; ++colour)
        d_rbgs_colour(dt, v.u[dt], v.rhs[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.omega, colour,
                      h->cfg.colour_offset, h->stream, l == 0, h->sigma);
    } else if (is_zebra(h->cfg.smoother)) {   // an X sweep, a Y sweep or both: colour 0 then colour 1 of the lines
      for (int dir = 0; dir < 2; ++dir)
        for (int colour = 0; colour < 2 && v.lp[dt][dir]; ++colour)
          d_line_colour(v.lp[dt][dir], colour, h->cfg.omega, v.u[dt], v.rhs[dt], h->stream);
    } else {   // MG_LEXGS: exactly `nu` sweeps (tol < 0 never triggers the early exit)
      d_coarse(dt, v.u[dt], v.rhs[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.coeff, h->cfg.omega, -1.0, nu - s,
               nullptr, h->stream, false, h->varcoef ? v.a[dt] : nullptr, h->sigma);
      break;
    }
  }
}

static void coarse_solve(mg_handle* h, int l, bool zero_init = false) {
  Level& v = h->lv[l];
  const int dt = h->level_dtype(l);
  // solvers/multigrid.py:119-124: the default coarse solver is GaussSeidelSmoother(omega = 1)
  d_coarse(dt, v.u[dt], v.rhs[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.coeff, 1.0, h->cfg.coarse_tol,
           h->cfg.coarse_maxit, h->d_int, h->stream, zero_init, h->varcoef ? v.a[dt] : nullptr, h->sigma);
}

static int cycle(mg_handle* h, int l) {
  const int L = h->L();
  if (l == L - 1) { coarse_solve(h, l); return MG_OK; }
  Level& f = h->lv[l];
  Level& c = h->lv[l + 1];
  const int dt = h->level_dtype(l), dc = h->level_dtype(l + 1);
  if (h->cfg.pre > 0) smooth(h, l, h->cfg.pre);
  {
    StageTimer tm(h, &f, 1);
    if (h->varcoef)
      d_var(mg::kVarResidual, dt, f.u[dt], f.a[dt], f.rhs[dt], f.r[dt], f.nx, f.ny, f.ld[dt], f.hx, f.hy, 1.0,
                              h->cfg.coeff, 0, 0, h->stream, h->sigma);
    else
      d_residual(dt, f.u[dt], f.rhs[dt], f.r[dt], f.nx, f.ny, f.ld[dt], f.hx, f.hy, h->cfg.coeff, h->stream, l == 0, h->sigma);
    d_restrict(dt, dc, f.r[dt], c.rhs[dc], f.nx, f.ny, f.ld[dt], c.ld[dc], h->stream);
  }
  (void)hipMemsetAsync(c.u[dc], 0, (size_t)c.nx * c.ld[dc] * esize(dc), h->stream);
  for (int k = 0, n = h->visits(l); k < n; ++k) {
    const int rc = cycle(h, l + 1);
    if (rc != MG_OK) return rc;
  }
  {
    StageTimer tm(h, &f, 2);
    const int rc = d_prolong(true, dc, dt, h->grid_dtype, c.u[dc], f.u[dt], f.nx, f.ny, f.ld[dt], c.ld[dc], h->stream);
    if (rc != MG_OK) return rc;
  }
  if (h->cfg.post > 0) smooth(h, l, h->cfg.post);
  return MG_OK;
}


static void tail_schedule(const mg_handle* h, int k, int l, int zero_flag, std::vector<int>& ops) {
  const int L = h->L();
  if (l == L - 1) { ops.push_back(mg::kTailSolve | ((l - k) << 8) | (zero_flag << 16)); return; }
  ops.push_back(mg::kTailDown | ((l - k) << 8) | (zero_flag << 16));
  for (int r = 0, n = h->visits(l); r < n; ++r) tail_schedule(h, k, l + 1, r == 0 ? 1 : 0, ops);
  ops.push_back(mg::kTailUp | ((l - k) << 8));
}

// mg_config.coarse_direct: 1 or < 0 (the host side's default) the nine unknowns of a 5 x 5 coarsest grid are solved directly,
// 0 by the reference's iteration to coarse_tol (bit-identical to it; what the parity tests pin).  W- and F-cycles visit the
// coarsest level 2^(L-1) times per cycle and spent most of their time in that iteration; a V-cycle saves its ~20 sweeps.
static bool want_direct(const mg_handle* h) {
  const int L = h->L();
  const int n = (h->lv[L - 1].nx - 2) * (h->lv[L - 1].ny - 2);          // unknowns of the coarsest grid: 9 for the 5 x 5 of every
  if (n < 1 || n > 64) return false;                                    // 2^k + 1 square, 21 for the 9 x 5 of a 2:1 domain
  return h->cfg.coarse_direct != 0;
}

// Decide where the tail starts: the first level k >= 1 whose sub-hierarchy fits the LDS pool, has at most
// kTailMaxLevels levels and (per-level MIXED policy) one dtype on levels k .. L-2.
static int plan_tail_lds(mg_handle* h) {
  h->tail_start = -1;
  h->tail2_start = -1;
  h->tail_direct = false;
  if (h->d_tail_ops) { (void)hipFree(h->d_tail_ops); h->d_tail_ops = nullptr; }      // re-planned when the operator changes
  const int L = h->L();
  if (!h->fused() || L < 3 || h->cfg.pre > 8 || h->cfg.post > 8) return MG_OK;
  const size_t esz_last = esize(h->grid_dtype);
  static const int max_top = exp_env("MG_EXP_TAIL_MAXN", 0);   // experiment: largest top level
  for (int k = 1; k <= L - 2; ++k) {
    if (L - k > mg::kTailMaxLevels) continue;
    const size_t esz = (h->cfg.precision == MG_PREC_ADAPTIVE) ? 8 : esize(h->level_dtype_in(k, MG_F64));
    if (tail_pool_bytes(h, k, esz, esz_last) > kTailPoolLimit) continue;
    // A 65^2 fp64 level costs more as two stages of the one-workgroup tail (12 us: five LDS reads per cell and stage through
    // one CU's LDS) than as two launches of its own (2 x 4.8 us): fp64 tails start at 33^2 (bench step -8 us, W(2,2) -3 %,
    // config 1 / 2 -10 / -6 %; profiles/README.md).  fp32 levels move half the bytes and stay in the tail from 65^2.
    const int cap = max_top > 0 ? max_top : (esz == 8 ? 33 : 65);
    if (std::max(h->lv[k].nx, h->lv[k].ny) > cap) continue;
    bool uniform = true;
    for (int l = k; l <= L - 2; ++l) uniform = uniform && (h->level_dtype_in(l, MG_F64) == h->level_dtype_in(k, MG_F64));
    if (!uniform) continue;
    h->tail_start = k;
    break;
  }
  h->tail_direct = false;
  h->tail_minv_sigma = -1.0;
  if (h->tail_start < 0) return MG_OK;
  h->tail_direct = want_direct(h);
  std::vector<int> ops;
  tail_schedule(h, h->tail_start, h->tail_start, 2, ops);
  h->tail_nops = (int)ops.size();
  HIPC(&h->err, hipMalloc((void**)&h->d_tail_ops, sizeof(int) * ops.size()));
  HIPC(&h->err, hipMemcpy(h->d_tail_ops, ops.data(), sizeof(int) * ops.size(), hipMemcpyHostToDevice));
  if (tail_set_attrs(kTailPoolLimit + 1024) != MG_OK) h->tail_start = -1;
  return MG_OK;
}
static int plan_tail(mg_handle* h) {
  int rc = plan_tail_lds(h);
  if (rc != MG_OK) return rc;
  rc = tail2_plan(h);                       // the register-resident tail takes precedence where it applies
  if (rc == MG_OK && h->tail2_start >= 0) h->tail_direct = want_direct(h);
  return rc;
}

// Inverse of the coarsest 5 x 5 system the smoothers relax: (-div(a grad .) + sigma) u = f on the nine interior cells,
// zero ring (a == 1 without a coefficient field).  Gaussian elimination with partial pivoting in long double.
static int build_coarse_inverse(mg_handle* h) {
  const Level& v = h->lv[h->L() - 1];
  const int cnx = v.nx, cny = v.ny, my = cny - 2, n = (cnx - 2) * my;
  if (n < 1 || n > 64) return fail(&h->err, MG_ERR_INVALID_VALUE, "coarse_direct: the coarsest grid has more than 64 unknowns");
  std::vector<double> a((size_t)cnx * cny, 1.0);
  if (h->varcoef) {
    const int dt = h->grid_dtype;
    std::vector<unsigned char> buf((size_t)cnx * v.ld[dt] * esize(dt));
    HIPC(&h->err, hipMemcpyAsync(buf.data(), v.a[dt], buf.size(), hipMemcpyDeviceToHost, h->stream));
    HIPC(&h->err, hipStreamSynchronize(h->stream));
    for (int i = 0; i < cnx; ++i)
      for (int j = 0; j < cny; ++j)
        a[(size_t)i * cny + j] = dt == MG_F32 ? (double)reinterpret_cast<const float*>(buf.data())[(size_t)i * v.ld[dt] + j]
                                              : reinterpret_cast<const double*>(buf.data())[(size_t)i * v.ld[dt] + j];
  }
  const long double ihx2 = 1.0L / ((long double)v.hx * v.hx), ihy2 = 1.0L / ((long double)v.hy * v.hy);
  const int w = 2 * n;
  std::vector<long double> M((size_t)n * w, 0.0L);      // [A | I], unknown (i, j) at p = (i - 1) my + (j - 1)
  for (int p = 0; p < n; ++p) {
    M[(size_t)p * w + n + p] = 1.0L;
    const int i = p / my + 1, j = p % my + 1;
    const long double c = a[(size_t)i * cny + j];
    const long double aip = 0.5L * (c + a[(size_t)(i + 1) * cny + j]), aim = 0.5L * (c + a[(size_t)(i - 1) * cny + j]);
    const long double ajp = 0.5L * (c + a[(size_t)i * cny + j + 1]), ajm = 0.5L * (c + a[(size_t)i * cny + j - 1]);
    M[(size_t)p * w + p] = (aip + aim) * ihx2 + (ajp + ajm) * ihy2 + (long double)h->sigma;
    if (i < cnx - 2) M[(size_t)p * w + p + my] = -aip * ihx2;
    if (i > 1) M[(size_t)p * w + p - my] = -aim * ihx2;
    if (j < my) M[(size_t)p * w + p + 1] = -ajp * ihy2;
    if (j > 1) M[(size_t)p * w + p - 1] = -ajm * ihy2;
  }
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r) if (fabsl(M[(size_t)r * w + c]) > fabsl(M[(size_t)piv * w + c])) piv = r;
    if (M[(size_t)piv * w + c] == 0.0L) return fail(&h->err, MG_ERR_INVALID_VALUE, "coarse_direct: singular coarsest system");
    if (piv != c) for (int q = 0; q < w; ++q) std::swap(M[(size_t)piv * w + q], M[(size_t)c * w + q]);
    const long double d = 1.0L / M[(size_t)c * w + c];
    for (int q = 0; q < w; ++q) M[(size_t)c * w + q] *= d;
    for (int r = 0; r < n; ++r) {
      if (r == c || M[(size_t)r * w + c] == 0.0L) continue;
      const long double f = M[(size_t)r * w + c];
      for (int q = 0; q < w; ++q) M[(size_t)r * w + q] -= f * M[(size_t)c * w + q];
    }
  }
  if (n == 9) {
    for (int p = 0; p < 9; ++p)
      for (int q = 0; q < 9; ++q) h->tail_minv[p * 9 + q] = (double)M[(size_t)p * w + 9 + q];
  }
  if (cnx != 5 || cny != 5) {      // the LDS tail streams the rows of the inverse from device memory
    std::vector<double> inv((size_t)n * n);
    for (int p = 0; p < n; ++p)
      for (int q = 0; q < n; ++q) inv[(size_t)p * n + q] = (double)M[(size_t)p * w + n + q];
    if (!h->d_minv) HIPC(&h->err, hipMalloc((void**)&h->d_minv, sizeof(double) * 64 * 64));
    HIPC(&h->err, hipStreamSynchronize(h->stream));                  // no launch in flight reads the old inverse
    HIPC(&h->err, hipMemcpy(h->d_minv, inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice));
    h->minv_n = n;
  }
  h->tail_minv_sigma = h->sigma;
  return MG_OK;
}

// the sweeps of one side of a level beyond the two its leg takes: two per launch
static void extra_sweeps(mg_handle* h, Level& f, int dt, LegGeom& g, int extra) {
  for (; extra > 0; extra -= g.nsweep) {
    g.nsweep = std::min(2, extra);
    d_sweeps(h->cfg.smoother, dt, f.u[dt], f.rhs[dt], f.t[dt], g, h->stream);
    std::swap(f.u[dt], f.t[dt]);
  }
}

// Fused V/W/F-cycle: two launches per level (down leg, up leg) instead of nine.  Same arithmetic per cell.
// zero_u: the iterate of this level is the zero correction and need not be read (first visit of a coarse level).
// part: see mg_host.hpp.
int cycle_fused(mg_handle* h, int l, bool zero_u, int part) {
  const int L = h->L();
  Level& f = h->lv[l];
  const int dt = h->level_dtype(l);
  const size_t bytes = (size_t)f.nx * f.ld[dt] * esize(dt);
  // the LDS tail only where the register-resident one does not apply (a variable-coefficient fp32 hierarchy could enter the
  // LDS tail one level earlier, at 65^2: 107 us per launch against two 33^2 register tails and one pair of legs, ~70)
  const bool tail2 = l == h->tail2_start, tail_lds = l == h->tail_start && h->tail2_start < 0;
  if ((tail2 || tail_lds) && h->cfg.tail != 0) {
    if (h->tail_direct && h->tail_minv_sigma != h->sigma) { const int rc = build_coarse_inverse(h); if (rc != MG_OK) return rc; }
    if (tail2) return tail2_launch(h, zero_u);
    launch_tail(h, zero_u);
    return MG_OK;
  }
  if (l == L - 1) {
    coarse_solve(h, l, zero_u);
    return MG_OK;
  }
  Level& c = h->lv[l + 1];
  const int dc = h->level_dtype(l + 1);
  const bool fine = (l == 0);
  const int sm = h->cfg.smoother;
  LegGeom g = leg_geom(h, l, dt, dc);
  if (part != kPartBack) {
    StageTimer tm(h, &f, 0);
    if (h->cfg.pre > 2 && zero_u) { (void)hipMemsetAsync(f.u[dt], 0, bytes, h->stream); zero_u = false; }
    extra_sweeps(h, f, dt, g, h->cfg.pre - 2);
    g.nsweep = std::min(2, h->cfg.pre);
    d_down(sm, dt, dc, f.u[dt], f.rhs[dt], f.t[dt], c.rhs[dc], g, zero_u, h->stream);
    std::swap(f.u[dt], f.t[dt]);
  }
  for (int k = 0, n = h->visits(l); k < n && part != kPartBack; ++k) {
    const int rc = cycle_fused(h, l + 1, k == 0);
    if (rc != MG_OK) return rc;
  }
  if (part != kPartFront) {
    StageTimer tm(h, &f, 2);
    const bool want_norm = fine && h->cfg.post <= 2 && h->cfg.precision != MG_PREC_DEFECT;   // defect correction: the norm is the fp64 defect's
    g.nsweep = std::min(2, h->cfg.post);
    const int n = d_up(sm, dt, dc, h->grid_dtype, f.u[dt], f.rhs[dt], f.t[dt], c.u[dc], h->partials, g, want_norm, h->stream);
    if (n < 0) return MG_ERR_INVALID_VALUE;
    std::swap(f.u[dt], f.t[dt]);
    if (fine) h->norm_partials = want_norm ? n : 0;
    extra_sweeps(h, f, dt, g, h->cfg.post - 2);
  }
  return MG_OK;
}

// Spanning leg: the BACK part of the running cycle (level-0 up leg) and the FRONT part of the next one (level-0 down leg,
// then everything below) with ONE level-0 launch in place of two.  Buffers: u holds the pre-smoothed iterate of the running
// cycle; the kernel writes the iterate of that cycle to t (keep_mid; dropped when the caller knows the solve cannot end
// there) and the pre-smoothed iterate of the next cycle to the third buffer s.  Afterwards u = s (what the next up leg
// reads), t = the iterate (undo_front's swap brings it back), s = the buffer just consumed.
bool span_ok(const mg_handle* h) {
  if (h->cfg.speculate < 2 || !h->fused() || h->L() < 3 || h->varcoef) return false;
  if (h->cfg.pre < 1 || h->cfg.pre > 2 || h->cfg.post < 1 || h->cfg.post > 2 || h->cfg.precision == MG_PREC_DEFECT) return false;
  if (!use_rb(leg_geom(h, 0, h->level_dtype(0), h->level_dtype(1)))) return false;   // bandwidth-bound levels only
  return h->level_dtype(0) == h->level_dtype(1) && (h->level_dtype(0) == MG_F32 || h->grid_dtype == MG_F64);
}
int cycle_span(mg_handle* h, bool keep_mid) {
  Level& f = h->lv[0];
  Level& c = h->lv[1];
  const int dt = h->level_dtype(0), dc = h->level_dtype(1);
  if (!f.s[dt]) {
    const int rc = alloc_zero(&h->err, &f.s[dt], (size_t)f.nx * f.ld[dt] * esize(dt), h->stream);
    if (rc != MG_OK) return rc;
    h->span_ring[dt] = false;
  }
  if (!h->span_ring[dt]) {                                           // the Dirichlet ring, once per solve and working precision
    d_convert_ring(dt, dt, f.u[dt], f.s[dt], f.nx, f.ny, f.ld[dt], f.ld[dt], h->stream);
    h->span_ring[dt] = true;
  }
  LegGeom g = leg_geom(h, 0, dt, dc);
  g.acoef = g.rdiag = nullptr;                                       // constant coefficients only (span_ok)
  g.nsweep = h->cfg.post;
  const int n = d_span(dt, h->grid_dtype, f.u[dt], f.rhs[dt], keep_mid ? f.t[dt] : nullptr, f.s[dt], c.u[dc], c.rhs[dc], h->partials, g,
                       h->cfg.pre, h->stream, h->cfg.smoother);
  if (n < 0) return MG_ERR_INVALID_VALUE;
  void* consumed = f.u[dt];
  f.u[dt] = f.s[dt];
  f.s[dt] = consumed;
  h->norm_partials = n;
  return MG_OK;
}
// ... and the rest of that front part: the sub-cycle(s) below level 0 (queued after the norm reduction of the cycle before)
int cycle_below_fine(mg_handle* h) {
  for (int k = 0, n = h->visits(0); k < n; ++k) {
    const int rc = cycle_fused(h, 1, k == 0);
    if (rc != MG_OK) return rc;
  }
  return MG_OK;
}

// Full-multigrid initial guess (solvers/advanced_multigrid.py:626-683, gpu/gpu_solver.py:603-652): restrict the rhs to
// every level (full weighting), solve the coarsest level from zero, then walk up: u_l = P u_{l+1}, followed by
// `ncyc` cycles of the sub-hierarchy that starts at level l.  The boundary ring of the fine iterate (Dirichlet data)
// is kept; coarser rings are zero.
int fmg_init(mg_handle* h, int ncyc) {
  h->iterate_zero = false;
  const int L = h->L();
  if (L < 2) return MG_OK;
  h->norm_partials = 0;
  for (int l = 0; l + 1 < L; ++l) {
    Level& f = h->lv[l];
    Level& c = h->lv[l + 1];
    const int dt = h->level_dtype(l), dc = h->level_dtype(l + 1);
    d_restrict(dt, dc, f.rhs[dt], c.rhs[dc], f.nx, f.ny, f.ld[dt], c.ld[dc], h->stream);
  }
  {
    Level& v = h->lv[L - 1];
    const int dt = h->level_dtype(L - 1);
    (void)hipMemsetAsync(v.u[dt], 0, (size_t)v.nx * v.ld[dt] * esize(dt), h->stream);
    coarse_solve(h, L - 1, false);
  }
  for (int l = L - 2; l >= 0; --l) {
    Level& f = h->lv[l];
    Level& c = h->lv[l + 1];
    const int dt = h->level_dtype(l), dc = h->level_dtype(l + 1);
    const size_t bytes = (size_t)f.nx * f.ld[dt] * esize(dt);
    if (l > 0) {
      (void)hipMemsetAsync(f.u[dt], 0, bytes, h->stream);
      if (f.t[dt]) (void)hipMemsetAsync(f.t[dt], 0, bytes, h->stream);
    } else {
      // keep the Dirichlet ring, zero the interior (whatever an initial guess or earlier cycles left there); the
      // ping-pong partner t carries the same ring by invariant and is fully rewritten by the first leg
      d_zero_interior(dt, f.u[dt], f.nx, f.ny, f.ld[dt], h->stream);
    }
    // interior cells: u = P e  (add = false writes every cell the interpolation defines, ring included: e ring is 0);
    // level 0: u = ring + P e on the interior == (ring-only field) + P e everywhere, because (P e)[ring] = 0
    if (d_prolong(l == 0, dc, dt, h->grid_dtype, c.u[dc], f.u[dt], f.nx, f.ny, f.ld[dt], c.ld[dc], h->stream) != MG_OK) return MG_ERR_INVALID_VALUE;
    for (int k = 0; k < ncyc; ++k) {
      const int rc = (h->fused()) ? cycle_fused(h, l, false) : cycle(h, l);
      if (rc != MG_OK) return rc;
    }
  }
  h->norm_partials = 0;
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}

// The boundary ring of every coarse rhs is the injected fine ring (r = f on boundary cells, injection on the
// coarse boundary: operators/laplacian.py:117-118, operators/transfer.py:109-113): constant over a solve, so it
// is written here once per rhs (and per working precision) instead of in every cycle.
// only_shared: just the coarse arrays that BOTH working precisions of the adaptive policy use (the fp64 coarsest level: its
// ring is the injected ring of an fp32 rhs in one phase and of the fp64 rhs in the other); the rest is still valid.
void inject_rings(mg_handle* h, int ph, bool only_shared) {
  for (int l = 0; l + 1 < h->L(); ++l) {
    Level& f = h->lv[l];
    Level& c = h->lv[l + 1];
    const int dt = h->level_dtype_in(l, ph), dc = h->level_dtype_in(l + 1, ph);
    if (only_shared && h->level_dtype_in(l + 1, MG_F32) != h->level_dtype_in(l + 1, MG_F64)) continue;
    d_inject_ring(dt, dc, f.rhs[dt], c.rhs[dc], f.nx, f.ny, f.ld[dt], c.nx, c.ny, c.ld[dc], h->stream);
  }
}

// ... for working precision p, unless that was done for this right-hand side already: then only the shared arrays
void inject_rings_once(mg_handle* h, int p) {
  if (!h->have_rhs) return;
  inject_rings(h, p, h->rings_gen[p] == h->rhs_gen);
  h->rings_gen[p] = h->rhs_gen;
}

// Full-multigrid start under defect correction (MG_PREC_DEFECT): the fp32 hierarchy solves the ERROR equation, so the FMG
// pass runs on A e = f - A u0 from the zero correction, u0 the WHOLE resident fp64 iterate, interior included (mg_solve calls it
// with the Dirichlet ring alone: FMG only without an initial guess; after mg_set_solution(u0) + mg_fmg the interior of u0 is
// part of the defect), and the result is added to the fp64 iterate -- the defect loop then starts from u0 + e instead of
// discarding the FMG work.  Unlike fmg_init under the other policies it does not forget the interior of the iterate: the
// answer is u0 + e, never a guess built from f and the ring alone (tests/test_gpu_defect_policy.py pins both starts).
int defect_fmg(mg_handle* h, int ncyc) {
  if (h->varcoef) return MG_ERR_INVALID_VALUE;
  if (h->L() < 2) return MG_OK;
  Level& v = h->lv[0];
  (void)launch_defect(h, false);                     // rhs[fp32] = f - A u (zero ring)
  inject_rings(h, h->phase);                               // (zero) rings of every coarse rhs
  const size_t bytes = (size_t)v.nx * v.ld[MG_F32] * 4;
  (void)hipMemsetAsync(v.u[MG_F32], 0, bytes, h->stream);
  if (v.t[MG_F32]) (void)hipMemsetAsync(v.t[MG_F32], 0, bytes, h->stream);
  const int rc = fmg_init(h, ncyc);                  // e in lv[0].u[fp32]
  if (rc != MG_OK) return rc;
  (void)launch_defect(h, true);                      // u <- u + e in fp64 (and the next defect)
  h->norm_partials = 0;
  h->iterate_zero = false;
  return MG_OK;
}

// one fp32 cycle from the zero correction on the current defect (left in lv[0].u[fp32])
int defect_cycle(mg_handle* h) {
  h->norm_partials = 0;
  h->iterate_zero = false;
  if (h->L() == 1) {                     // a single level: the "cycle" is the coarsest solve, in the grid dtype (fp64)
    return MG_ERR_INVALID_VALUE;
  }
  if (h->fused()) return cycle_fused(h, 0, true);
  Level& v = h->lv[0];
  (void)hipMemsetAsync(v.u[MG_F32], 0, (size_t)v.nx * v.ld[MG_F32] * 4, h->stream);
  return cycle(h, 0);
}

int run_cycle(mg_handle* h) {
  h->norm_partials = 0;
  h->iterate_zero = false;
  if (h->cfg.precision == MG_PREC_DEFECT) {            // one outer step: defect, fp32 cycle, update
    if (h->varcoef) return MG_ERR_INVALID_VALUE;
    (void)launch_defect(h, false);
    inject_rings(h, h->phase);
    const int rc = defect_cycle(h);
    if (rc != MG_OK) return rc;
    (void)launch_defect(h, true);
    return MG_OK;
  }
  if (h->fused() && h->L() > 1) return cycle_fused(h, 0, false);
  return cycle(h, 0);
}

// sum of f^2 over the boundary ring of the fine rhs (4 windows of the device reduction), per allocated dtype
static int ring_sums(mg_handle* h) {
  Level& v = h->lv[0];
  for (int dt = 0; dt < 2; ++dt) {
    h->ring_sumsq[dt] = 0;
    if (!v.rhs[dt]) continue;
    const int win[4][4] = {{0, 1, 0, v.ny}, {v.nx - 1, v.nx, 0, v.ny}, {1, v.nx - 1, 0, 1}, {1, v.nx - 1, v.ny - 1, v.ny}};
    for (int k = 0; k < 4; ++k) {
      const int n = d_sumsq(dt, v.rhs[dt], h->partials, v.ld[dt], win[k][0], win[k][1], win[k][2], win[k][3], h->stream);
      launch_reduce(h->partials, n, h->d_scalar, h->stream);
      HIPC(&h->err, hipMemcpyAsync(h->h_scalar, h->d_scalar, sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPC(&h->err, hipStreamSynchronize(h->stream));
      h->ring_sumsq[dt] += *h->h_scalar;
    }
  }
  return MG_OK;
}

static int rhs_changed(mg_handle* h) {
  h->have_rhs = true;
  h->norm_partials = 0;
  ++h->rhs_gen;
  inject_rings_once(h, h->phase);
  return ring_sums(h);
}

int set_rhs_impl(mg_handle* h, const void* rhs, int hdt) {
  Level& v = h->lv[0];
  for (int dt = 0; dt < 2; ++dt)
    if (v.rhs[dt]) {
      const int rc = upload(&h->err, v.rhs[dt], dt, v.ld[dt], rhs, hdt, v.nx, v.ny, h->staging, h->stream);
      if (rc != MG_OK) return rc;
    }
  return rhs_changed(h);
}

int set_u_impl(mg_handle* h, const void* u0, int hdt) {
  Level& v = h->lv[0];
  // Adaptive policy: every solve starts in double (PrecisionManager's default precision, core/precision.py:26-45), so a
  // new initial guess goes straight into the fp64 iterate instead of being converted up when the solve begins
  if (h->cfg.precision == MG_PREC_ADAPTIVE && h->phase != MG_F64 && h->L() > 1) {
    h->phase = MG_F64;
    inject_rings_once(h, MG_F64);
  }
  const int dt = h->iterate_dtype();
  h->norm_partials = 0;
  h->iterate_zero = (u0 == nullptr);
  if (u0) {
    int rc = upload(&h->err, v.u[dt], dt, v.ld[dt], u0, hdt, v.nx, v.ny, h->staging, h->stream);
    if (rc != MG_OK) return rc;
    if (v.t[dt])     // the ping-pong partner must carry the same boundary ring
      d_convert_ring(dt, dt, v.u[dt], v.t[dt], v.nx, v.ny, v.ld[dt], v.ld[dt], h->stream);
  } else {
    HIPC(&h->err, hipMemsetAsync(v.u[dt], 0, (size_t)v.nx * v.ld[dt] * esize(dt), h->stream));
    if (v.t[dt]) HIPC(&h->err, hipMemsetAsync(v.t[dt], 0, (size_t)v.nx * v.ld[dt] * esize(dt), h->stream));
  }
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  return MG_OK;
}

// set_u_impl(u0 != NULL) for an initial guess that is already on the device: converted on the handle's stream instead of
// uploaded, the same state changes, no synchronisation
int set_u_device_impl(mg_handle* h, const void* u_dev, int ld, int dtype) {
  if (!h || !u_dev || !valid_dtype(dtype) || ld < h->lv[0].ny)
    return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "set_u_device_impl: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  Level& v = h->lv[0];
  if (h->cfg.precision == MG_PREC_ADAPTIVE && h->phase != MG_F64 && h->L() > 1) {
    h->phase = MG_F64;
    inject_rings_once(h, MG_F64);
  }
  const int dt = h->iterate_dtype();
  h->norm_partials = 0;
  h->iterate_zero = false;
  d_convert(dtype, dt, u_dev, v.u[dt], v.nx, v.ny, ld, v.ld[dt], h->stream);
  if (v.t[dt]) d_convert_ring(dt, dt, v.u[dt], v.t[dt], v.nx, v.ny, v.ld[dt], v.ld[dt], h->stream);
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}

// The caller of mg_set_rhs_device / mg_update_rhs_device states that the boundary ring of the fine right-hand side is zero
// (a residual, the right-hand side of a time step).  mg_set_rhs_device leaves the ring's sum of squares unknown (< 0: it
// would cost a host round trip), which keeps the solve loop off the cached up-leg norm and the speculative launches
// (fine_norm and solve_begin in mg_solve.hip test ring_sumsq >= 0); mg_update_rhs_device keeps whatever is recorded.
// With a zero ring the sum is known to be 0, and mg_iterate runs the loop mg_solve runs after a host upload.
void rhs_ring_is_zero(mg_handle* h) { h->ring_sumsq[MG_F32] = h->ring_sumsq[MG_F64] = 0.0; }

int engine_set_rhs(mg_handle* eng, bool* has_rhs, const double* f, int ld, bool ring_is_zero) {
  if (*has_rhs) return mg_update_rhs_device(eng, f, ld, MG_F64);
  const int rc = mg_set_rhs_device(eng, f, ld, MG_F64);
  if (rc != MG_OK) return rc;
  if (ring_is_zero) rhs_ring_is_zero(eng);
  *has_rhs = true;
  return MG_OK;
}

int engine_precondition(mg_handle* eng, bool* has_rhs, const double* r, double* z, int ld, int num_cycles) {
  int rc = engine_set_rhs(eng, has_rhs, r, ld, false);
  if (rc == MG_OK) rc = mg_zero_solution_device(eng);
  if (rc == MG_OK) rc = mg_cycle(eng, num_cycles);
  if (rc == MG_OK) rc = mg_get_solution_device(eng, z, ld, MG_F64);
  return rc;
}

}  // namespace mgh

using namespace mgh;

// =================================================================== C ABI =====================
extern "C" {

const char* mg_version(void) { return "mghip 0.1 (gfx950)"; }

int mg_device_count(int* count) {
  if (!count) return fail(nullptr, MG_ERR_INVALID_VALUE, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return fail(nullptr, MG_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
  *count = n;
  return MG_OK;
}

const char* mg_last_error(const mg_handle* h) { return h ? h->err.c_str() : last_error().c_str(); }

int mg_pitch_elems(int dtype, int ny, int* ld) {
  if (!valid_dtype(dtype) || ny < 1 || !ld) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_pitch_elems: bad argument");
  *ld = pitch_elems(dtype, ny);
  return MG_OK;
}

int mg_create(const mg_config* cfg, mg_handle** out) {
  if (!cfg || !out) return fail(nullptr, MG_ERR_INVALID_VALUE, "mg_create: NULL argument");
  *out = nullptr;
  if (cfg->nx < 3 || cfg->ny < 3)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "Grid must have at least 3 points in each direction");   // core/grid.py:34-35
  if (cfg->cycle < MG_CYCLE_V || cfg->cycle > MG_CYCLE_F) return fail(nullptr, MG_ERR_INVALID_VALUE, "unknown cycle type");
  if (cfg->smoother < MG_JACOBI || cfg->smoother > MG_ZEBRA_ALT) return fail(nullptr, MG_ERR_INVALID_VALUE, "unknown smoother");
  if (is_zebra(cfg->smoother) && cfg->colour_offset != 0)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "line smoothers serve a single domain: colour_offset must be 0");
  if (is_zebra(cfg->smoother) && !line_shape_ok(cfg->smoother == MG_ZEBRA_Y ? 3 : cfg->nx, cfg->smoother == MG_ZEBRA_X ? 3 : cfg->ny))
    return fail(nullptr, MG_ERR_INVALID_VALUE, "line smoothers: lines of more than 16384 cells do not fit a workgroup's LDS");
  if (cfg->precision < MG_PREC_DOUBLE || cfg->precision > MG_PREC_DEFECT) return fail(nullptr, MG_ERR_INVALID_VALUE, "unknown precision policy");
  if (cfg->pre < 0 || cfg->post < 0 || cfg->max_levels < 1 || cfg->coarse_maxit < 1)
    return fail(nullptr, MG_ERR_INVALID_VALUE, "negative sweep count / max_levels < 1 / coarse_maxit < 1");
  if (!(cfg->x1 > cfg->x0) || !(cfg->y1 > cfg->y0)) return fail(nullptr, MG_ERR_INVALID_VALUE, "empty domain");

  int ndev = 0;
  int rc = mg_device_count(&ndev);
  if (rc != MG_OK) return rc;
  if (ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, MG_ERR_NO_DEVICE, "no such HIP device");
  HIPC(nullptr, hipSetDevice(cfg->device));

  mg_handle* h = new mg_handle();
  h->cfg = *cfg;
  h->grid_dtype = (cfg->precision == MG_PREC_SINGLE) ? MG_F32 : MG_F64;
  h->phase = MG_F64;
  // hierarchy: solvers/multigrid.py:135-171
  int nx = cfg->nx, ny = cfg->ny;
  for (int level = 0; level < cfg->max_levels; ++level) {
    if (level > 0) {
      if ((nx - 1) % 2 != 0 || (ny - 1) % 2 != 0) break;          // core/grid.py:148-149
      const int cx = (nx - 1) / 2 + 1, cy = (ny - 1) / 2 + 1;
      if (cx < 5 || cy < 5) break;                                 // multigrid.py:158-160
      nx = cx; ny = cy;
    }
    Level l;
    l.nx = nx; l.ny = ny;
    l.hx = (cfg->x1 - cfg->x0) / (nx - 1);
    l.hy = (cfg->y1 - cfg->y0) / (ny - 1);
    l.ld[0] = pitch_elems(MG_F32, ny);
    l.ld[1] = pitch_elems(MG_F64, ny);
    h->lv.push_back(l);
  }
  auto bail = [&](int code) { release(h); std::string m = h->err; delete h; last_error() = m; return code; };
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) { h->err = "hipStreamCreate failed"; return bail(MG_ERR_HIP); }
  h->stream = h->own_stream;
  for (int l = 0; l < h->L(); ++l) {
    Level& v = h->lv[l];
    for (int dt = 0; dt < 2; ++dt) {
      if (!h->needs(l, dt)) continue;
      const size_t bytes = (size_t)v.nx * v.ld[dt] * esize(dt);
      if ((rc = alloc_zero(&h->err, &v.u[dt], bytes, h->stream)) != MG_OK) return bail(rc);
      if ((rc = alloc_zero(&h->err, &v.rhs[dt], bytes, h->stream)) != MG_OK) return bail(rc);
      const bool master = cfg->precision == MG_PREC_DEFECT && l == 0 && dt == MG_F64;     // iterate + partner + f only
      if (l < h->L() - 1 || master) {
        if (!master && (rc = alloc_zero(&h->err, &v.r[dt], bytes, h->stream)) != MG_OK) return bail(rc);
        if ((master || cfg->smoother == MG_JACOBI || h->fused()) && (rc = alloc_zero(&h->err, &v.t[dt], bytes, h->stream)) != MG_OK) return bail(rc);
      }
    }
  }
  if (is_zebra(cfg->smoother))     // the smoothed levels own their plans, one per allocated dtype; the coarsest keeps its solve
    for (int l = 0; l + 1 < h->L(); ++l) {
      Level& v = h->lv[l];
      for (int dt = 0; dt < 2; ++dt)
        for (int dir = 0; dir < 2 && v.u[dt]; ++dir) {
          if (cfg->smoother == (dir == 0 ? MG_ZEBRA_Y : MG_ZEBRA_X)) continue;
          if ((rc = line_plan_make(dt, dir, v.nx, v.ny, v.ld[dt], v.hx, v.hy, 0.0, &v.lp[dt][dir], &h->err)) != MG_OK) return bail(rc);
        }
    }
  {
    const size_t np = max_partials(cfg->nx, cfg->ny);
    if ((rc = alloc_zero(&h->err, (void**)&h->partials, sizeof(double) * np, h->stream)) != MG_OK) return bail(rc);
  }
  if ((rc = alloc_zero(&h->err, (void**)&h->d_scalar, sizeof(double), h->stream)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&h->err, (void**)&h->d_int, sizeof(int), h->stream)) != MG_OK) return bail(rc);
  if ((rc = alloc_zero(&h->err, &h->staging, (size_t)cfg->nx * pitch_elems(MG_F64, cfg->ny) * 8, h->stream)) != MG_OK) return bail(rc);
  if (hipHostMalloc((void**)&h->h_scalar, sizeof(double)) != hipSuccess ||
      hipHostMalloc((void**)&h->h_int, sizeof(int)) != hipSuccess) { h->err = "hipHostMalloc failed"; return bail(MG_ERR_ALLOC); }
  if (hipHostMalloc((void**)&h->mbox, sizeof(mg::HostMailbox), hipHostMallocMapped) == hipSuccess &&
      hipHostGetDevicePointer((void**)&h->mbox_dev, h->mbox, 0) == hipSuccess) {
    h->mbox->value = 0; h->mbox->seq = 0;
  } else {
    h->mbox_dev = nullptr;     // no mapped host memory: fall back to copy + stream synchronisation
  }
  if ((rc = plan_tail(h)) != MG_OK) return bail(rc);
  if (hipStreamSynchronize(h->stream) != hipSuccess) { h->err = "hipStreamSynchronize failed"; return bail(MG_ERR_HIP); }
  *out = h;
  return MG_OK;
}

int mg_destroy(mg_handle* h) {
  if (!h) return MG_OK;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  release(h);
  delete h;
  return MG_OK;
}

int mg_num_levels(const mg_handle* h, int* n) {
  if (!h || !n) return fail(nullptr, MG_ERR_INVALID_VALUE, "NULL argument");
  *n = h->L();
  return MG_OK;
}

int mg_level_shape(const mg_handle* h, int level, int* nx, int* ny) {
  if (!h || !nx || !ny || level < 0 || level >= h->L()) return fail(nullptr, MG_ERR_INVALID_VALUE, "bad level");
  *nx = h->lv[level].nx; *ny = h->lv[level].ny;
  return MG_OK;
}

int mg_level_timings(const mg_handle* h, int level, double out3[3]) {
  if (!h || !out3 || level < 0 || level >= h->L()) return fail(nullptr, MG_ERR_INVALID_VALUE, "bad level");
  for (int k = 0; k < 3; ++k) out3[k] = h->lv[level].timings[k];
  return MG_OK;
}

int mg_get_stream(mg_handle* h, void** stream) {
  if (!h || !stream) return fail(nullptr, MG_ERR_INVALID_VALUE, "NULL argument");
  *stream = (void*)h->stream;
  return MG_OK;
}

int mg_set_stream(mg_handle* h, void* stream, int use_own) {
  if (!h) return fail(nullptr, MG_ERR_INVALID_VALUE, "NULL handle");
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  h->stream = use_own ? h->own_stream : (hipStream_t)stream;
  return MG_OK;
}

int mg_set_rhs_device(mg_handle* h, const void* rhs_dev, int ld, int dtype) {
  if (!h || !rhs_dev || !valid_dtype(dtype) || ld < h->lv[0].ny) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_set_rhs_device: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  Level& v = h->lv[0];
  for (int dt = 0; dt < 2; ++dt)
    if (v.rhs[dt]) d_convert(dtype, dt, rhs_dev, v.rhs[dt], v.nx, v.ny, ld, v.ld[dt], h->stream);
  h->have_rhs = true;
  h->norm_partials = 0;
  ++h->rhs_gen;
  inject_rings_once(h, h->phase);   // asynchronous; the ring sum (host round trip) is only needed by mg_residual_norm
  h->ring_sumsq[0] = h->ring_sumsq[1] = -1.0;
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}

int mg_update_rhs_device(mg_handle* h, const void* rhs_dev, int ld, int dtype) {
  if (!h || !rhs_dev || !valid_dtype(dtype) || ld < h->lv[0].ny) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_update_rhs_device: bad argument");
  if (!h->have_rhs) return fail(&h->err, MG_ERR_STATE, "mg_update_rhs_device before mg_set_rhs / mg_set_rhs_device");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  Level& v = h->lv[0];
  for (int dt = 0; dt < 2; ++dt)
    if (v.rhs[dt]) d_convert(dtype, dt, rhs_dev, v.rhs[dt], v.nx, v.ny, ld, v.ld[dt], h->stream);
  h->norm_partials = 0;
  // a new right-hand side as far as cached norms go, the same one as far as the coarse rhs rings and their sums go
  const unsigned old_gen = h->rhs_gen++;
  for (int p = 0; p < 2; ++p)
    if (h->rings_gen[p] == old_gen) h->rings_gen[p] = h->rhs_gen;
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}

int mg_zero_solution_device(mg_handle* h) {
  if (!h) return fail(nullptr, MG_ERR_INVALID_VALUE, "NULL handle");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  h->norm_partials = 0;
  h->iterate_zero = true;
  Level& v = h->lv[0];
  const int dt = h->iterate_dtype();
  HIPC(&h->err, hipMemsetAsync(v.u[dt], 0, (size_t)v.nx * v.ld[dt] * esize(dt), h->stream));
  if (v.t[dt]) HIPC(&h->err, hipMemsetAsync(v.t[dt], 0, (size_t)v.nx * v.ld[dt] * esize(dt), h->stream));
  return MG_OK;
}

int mg_get_solution_device(mg_handle* h, void* u_dev, int ld, int dtype) {
  if (!h || !u_dev || !valid_dtype(dtype) || ld < h->lv[0].ny) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_get_solution_device: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  Level& v = h->lv[0];
  const int dt = h->iterate_dtype();
  d_convert(dt, dtype, v.u[dt], u_dev, v.nx, v.ny, v.ld[dt], ld, h->stream);
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}

int mg_synchronize(mg_handle* h) {
  if (!h) return fail(nullptr, MG_ERR_INVALID_VALUE, "NULL handle");
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  return MG_OK;
}

int mg_set_rhs(mg_handle* h, const void* rhs, int host_dtype) {
  if (!h || !rhs || !valid_dtype(host_dtype)) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_set_rhs: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  return set_rhs_impl(h, rhs, host_dtype);
}


int mg_set_coefficient(mg_handle* h, const void* a_host, int host_dtype) {
  if (!h || !valid_dtype(host_dtype)) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_set_coefficient: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  if (a_host && is_zebra(h->cfg.smoother))
    return fail(&h->err, MG_ERR_STATE, "mg_set_coefficient: the line smoothers relax the constant-coefficient operator (a variable "
                                       "coefficient needs a matrix per line)");
  if (a_host && h->cfg.precision == MG_PREC_DEFECT)
    return fail(&h->err, MG_ERR_INVALID_VALUE, "mg_set_coefficient: defect correction (MG_PREC_DEFECT) runs the constant-coefficient operator");
  h->norm_partials = 0;
  if (!a_host) {                                           // back to the constant-coefficient operator
    const bool was = h->varcoef;
    h->varcoef = false;
    return was ? plan_tail(h) : MG_OK;
  }
  // The coefficient lives in every precision a level may compute in.  Level l takes every 2^l-th vertex value of the
  // caller's array (injection = re-discretisation), cast ONCE from the caller's dtype to the level's: no level ever
  // sees a value that went through a narrower precision on the way down.
  Level& v0 = h->lv[0];
  const int lds = pitch_elems(host_dtype, v0.ny);
  HIPC(&h->err, hipMemcpy2DAsync(h->staging, (size_t)lds * esize(host_dtype), a_host, (size_t)v0.ny * esize(host_dtype),
                                 (size_t)v0.ny * esize(host_dtype), v0.nx, hipMemcpyHostToDevice, h->stream));
  for (int l = 0; l < h->L(); ++l) {
    Level& v = h->lv[l];
    for (int dt = 0; dt < 2; ++dt) {
      if (!v.u[dt]) continue;
      if (!v.a[dt]) { const int rc = alloc_zero(&h->err, &v.a[dt], (size_t)v.nx * v.ld[dt] * esize(dt), h->stream); if (rc != MG_OK) return rc; }
      if (!v.rd[dt]) { const int rc = alloc_zero(&h->err, &v.rd[dt], (size_t)v.nx * v.ld[dt] * esize(dt), h->stream); if (rc != MG_OK) return rc; }
      d_inject(host_dtype, dt, h->staging, v.a[dt], lds, v.nx, v.ny, v.ld[dt], 1 << l, h->stream);
    }
  }
  const bool was = h->varcoef;
  h->varcoef = true;
  h->rd_sigma = -1.0;                                      // new coefficient: new reciprocal diagonals
  refresh_rdiag(h);
  HIPC(&h->err, hipStreamSynchronize(h->stream));
  h->tail_minv_sigma = -1.0;                               // a direct coarsest solve needs the inverse of the NEW operator
  return was ? MG_OK : plan_tail(h);                       // the LDS tail carries one more array per level
}

int mg_set_shift(mg_handle* h, double sigma) {
  if (!h || !(sigma >= 0.0) || !std::isfinite(sigma))
    return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_set_shift: sigma must be finite and >= 0");
  const bool changed = h->sigma != sigma;
  h->sigma = sigma;
  h->norm_partials = 0;     // a cached sum r^2 belongs to the previous operator
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  refresh_rdiag(h);         // variable coefficients: the reciprocal diagonals carry the shift
  if (changed && is_zebra(h->cfg.smoother)) {            // sigma is in the diagonal of every line's matrix: new tables
    HIPC(&h->err, hipStreamSynchronize(h->stream));      // no launch in flight reads the old ones
    for (auto& v : h->lv)
      for (auto& per_dtype : v.lp)
        for (mg_line_plan* p : per_dtype)
          if (p) { const int rc = line_plan_set_sigma(p, sigma, &h->err); if (rc != MG_OK) return rc; }
  }
  return MG_OK;
}

int mg_set_solution(mg_handle* h, const void* u0, int host_dtype) {
  if (!h || !valid_dtype(host_dtype)) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_set_solution: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  return set_u_impl(h, u0, host_dtype);
}

int mg_get_solution(mg_handle* h, void* u_out, int host_dtype) {
  if (!h || !u_out || !valid_dtype(host_dtype)) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_get_solution: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  Level& v = h->lv[0];
  const int dt = h->iterate_dtype();
  return download(&h->err, u_out, host_dtype, v.u[dt], dt, v.ld[dt], v.nx, v.ny, h->staging, h->stream);
}

int mg_fmg(mg_handle* h, int cycles_per_level) {
  if (!h || cycles_per_level < 0) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_fmg: bad argument");
  if (!h->have_rhs) return fail(&h->err, MG_ERR_STATE, "mg_fmg before mg_set_rhs");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  const int rc = h->cfg.precision == MG_PREC_DEFECT ? defect_fmg(h, cycles_per_level) : fmg_init(h, cycles_per_level);
  if (rc != MG_OK) return fail(&h->err, rc, h->varcoef && h->cfg.precision == MG_PREC_DEFECT
                                                 ? "mg_fmg: defect correction runs the constant-coefficient operator"
                                                 : "mg_fmg: unsupported precision combination");
  return MG_OK;
}

int mg_cycle(mg_handle* h, int ncycles) {
  if (!h || ncycles < 0) return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_cycle: bad argument");
  if (!h->have_rhs) return fail(&h->err, MG_ERR_STATE, "mg_cycle before mg_set_rhs");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  for (int k = 0; k < ncycles; ++k) {
    const int rc = run_cycle(h);
    if (rc != MG_OK) return fail(&h->err, rc, "cycle: unsupported precision combination");
  }
  HIPC(&h->err, hipGetLastError());
  return MG_OK;
}

int mg_time_op(mg_handle* h, int op, int level, int dtype, int reps, double* avg_ms) {
  if (!h || !avg_ms || reps < 1 || level < 0 || level >= h->L() || !valid_dtype(dtype))
    return fail(h ? &h->err : nullptr, MG_ERR_INVALID_VALUE, "mg_time_op: bad argument");
  HIPC(&h->err, hipSetDevice(h->cfg.device));
  Level& v = h->lv[level];
  const int dt = dtype;
  if (op != 6 && (!v.u[dt] || !v.rhs[dt])) return fail(&h->err, MG_ERR_STATE, "mg_time_op: level has no arrays of that dtype");
  if ((op == 0 || op == 10) && h->cfg.smoother != MG_JACOBI) return fail(&h->err, MG_ERR_STATE, "mg_time_op: jacobi needs a Jacobi-configured handle");
  if ((op == 0 || (op >= 7 && op <= 9)) && !v.t[dt]) return fail(&h->err, MG_ERR_STATE, "mg_time_op: no ping-pong buffer on this level");
  if ((op == 2 || op == 4 || op == 5 || op == 7 || op == 8) && (level >= h->L() - 1 || !v.r[dt])) return fail(&h->err, MG_ERR_STATE, "mg_time_op: no coarser level");
  static const int exp_nsweep = exp_env("MG_EXP_NSWEEP", 2);
  h->norm_partials = 0;
  if (level == 0 && (op == 0 || op == 1 || (op >= 5 && op <= 9) || op == 12 || op == 13)) h->iterate_zero = false;    // these rewrite the fine iterate
  // op 10: the single-sweep Jacobi kernel rotating over independent {u, rhs, out} sets whose total exceeds three
  // times the 256 MiB Infinity Cache, so that no launch finds its operands on die: the HBM-proper smoother figure
  std::vector<void*> hbm_sets;
  struct FreeSets { std::vector<void*>& v; ~FreeSets() { for (void* p : v) (void)hipFree(p); } } free_sets{hbm_sets};
  int nsets = 0, set_idx = 0;
  if (op == 10 || op == 11) {
    const size_t bytes = (size_t)v.nx * v.ld[dt] * esize(dt);
    nsets = std::max<int>(3, (int)((768ull << 20) / (3 * bytes)) + 1);
    for (int k = 0; k < 3 * nsets; ++k) {
      void* p = nullptr;
      HIPC(&h->err, hipMalloc(&p, bytes));
      hbm_sets.push_back(p);
      HIPC(&h->err, hipMemcpyAsync(p, (k % 3 == 1) ? v.rhs[dt] : v.u[dt], bytes, hipMemcpyDeviceToDevice, h->stream));
    }
  }
  hipEvent_t e0, e1;
  HIPC(&h->err, hipEventCreate(&e0));
  HIPC(&h->err, hipEventCreate(&e1));
  auto run = [&](int n) -> int {
    for (int k = 0; k < n; ++k) {
      switch (op) {
        case 10: { void** b = hbm_sets.data() + 3 * (set_idx++ % nsets);
                   d_jacobi(dt, b[0], b[1], b[2], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.omega, h->stream, level == 0); } break;
        case 11: { void** b = hbm_sets.data() + 3 * (set_idx++ % nsets);       // the bare stream: same traffic, no stencil
                   d_stream_triad(dt, b[0], b[1], b[2], v.nx, v.ny, v.ld[dt], h->stream); } break;
        case 0: d_jacobi(dt, v.u[dt], v.rhs[dt], v.t[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.omega, h->stream, level == 0);
                std::swap(v.u[dt], v.t[dt]); break;
        case 1: for (int c = 0; c < 2; ++c) d_rbgs_colour(dt, v.u[dt], v.rhs[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.omega, c, h->cfg.colour_offset, h->stream, level == 0); break;
        case 2: d_residual(dt, v.u[dt], v.rhs[dt], v.r[dt], v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.coeff, h->stream, level == 0); break;
        case 3: { const int n2 = d_residual_norm(dt, v.u[dt], v.rhs[dt], h->partials, v.nx, v.ny, v.ld[dt], v.hx, v.hy, h->cfg.coeff, h->stream, level == 0);
                  launch_reduce(h->partials, n2, h->d_scalar, h->stream); } break;
        case 4: { Level& c = h->lv[level + 1]; const int dc = c.rhs[dt] ? dt : 1 - dt;
                  d_restrict(dt, dc, v.r[dt], c.rhs[dc], v.nx, v.ny, v.ld[dt], c.ld[dc], h->stream); } break;
        case 5: { Level& c = h->lv[level + 1]; const int dc = c.u[dt] ? dt : 1 - dt;
                  if (d_prolong(true, dc, dt, h->grid_dtype, c.u[dc], v.u[dt], v.nx, v.ny, v.ld[dt], c.ld[dc], h->stream) != MG_OK) return MG_ERR_INVALID_VALUE; } break;
        case 6: { const int rc = run_cycle(h); if (rc != MG_OK) return rc; } break;
        case 7: { Level& c = h->lv[level + 1]; const int dc = c.rhs[dt] ? dt : 1 - dt;          // down leg
                  LegGeom g = leg_geom(h, level, dt, dc); g.nsweep = exp_nsweep;
                  d_down(h->cfg.smoother, dt, dc, v.u[dt], v.rhs[dt], v.t[dt], c.rhs[dc], g, false, h->stream);
                  std::swap(v.u[dt], v.t[dt]); } break;
        case 8: { Level& c = h->lv[level + 1]; const int dc = c.u[dt] ? dt : 1 - dt;            // up leg (+ norm on level 0)
                  LegGeom g = leg_geom(h, level, dt, dc); g.nsweep = exp_nsweep;
                  if (d_up(h->cfg.smoother, dt, dc, h->grid_dtype, v.u[dt], v.rhs[dt], v.t[dt], c.u[dc], h->partials, g, level == 0, h->stream) < 0) return MG_ERR_INVALID_VALUE;
                  std::swap(v.u[dt], v.t[dt]); } break;
        case 9: { LegGeom g = leg_geom(h, level, dt, -1); g.nsweep = exp_nsweep;
                  d_sweeps(h->cfg.smoother, dt, v.u[dt], v.rhs[dt], v.t[dt], g, h->stream);
                  std::swap(v.u[dt], v.t[dt]); } break;
        case 12: case 13: {                                                                      // spanning leg, with / without the store of the iterate in between
                  const int phase0 = h->phase;
                  if (h->cfg.precision == MG_PREC_ADAPTIVE) h->phase = dt;                       // time the leg of either working precision
                  const bool ok = level == 0 && span_ok(h) && h->level_dtype(0) == dt;
                  const int rc2 = ok ? cycle_span(h, op == 12) : MG_ERR_INVALID_VALUE;
                  h->phase = phase0;
                  if (rc2 != MG_OK) return rc2; } break;
        default: return MG_ERR_INVALID_VALUE;
      }
    }
    return MG_OK;
  };
  int rc = run(1);   // warm-up
  if (rc != MG_OK) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return fail(&h->err, rc, "mg_time_op: unsupported op"); }
  HIPC(&h->err, hipEventRecord(e0, h->stream));
  rc = run(reps);
  HIPC(&h->err, hipEventRecord(e1, h->stream));
  HIPC(&h->err, hipEventSynchronize(e1));
  float ms = 0;
  HIPC(&h->err, hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  *avg_ms = (double)ms / reps;
  // Outside the timed interval: leave the handle as a fresh one with this right-hand side and iterate would be.
  // op 4 wrote the ring of the coarse rhs from lv[level].r, which the fused legs never write (they restrict into the interior
  // only and rely on the rings injected once per right-hand side): inject the rings again, for either working precision.
  if (op == 4) {
    h->rings_gen[0] = h->rings_gen[1] = 0;
    inject_rings_once(h, h->phase);
  }
  // ops 12 / 13: cycle_span marked `partials` as the sum r^2 of the current iterate, but lv[0].u is already the pre-smoothed
  // iterate of the NEXT cycle (the solve loop drops the mark the same way once its front part is queued)
  if (op == 12 || op == 13) h->norm_partials = 0;
  return rc;
}

}  // extern "C"
