"""The reaction-diffusion stepper (include/mghip_rd.h, csrc/mg_rd.hip) on a GPU: its two kernels call by call against the NumPy
restatement tests/rd_reference.py (pinned on the CPU by tests/test_rd_cpu.py), single steps of the driver against the dense
exact Newton method from the device's own states, the closed-form eigenmode factors, the decay of the free energy under convex
splitting, the driver's semantics and refusals, and ReactionDiffusionSolver.

Kernel shapes and the Field harness are tests/test_gpu_ho.py's; the rule for sinh and exp is tests/test_gpu_nl.py's: K_ULP ulp
of the reaction term plus one ulp of the result.

Steps are compared by the one bound the problem gives: N(v) = (-L_a + lambda) v + (kappa/alpha) w phi(v) is strongly monotone
with constant >= lambda (a > 0, w >= 0, phi' >= 0), so two approximate solutions of N(v) = f with the same ring differ by at
most (||F_1||_h + ||F_2||_h) / lambda in the h-norm, F_i their residuals."""
import ctypes as C
import math

import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib

import nl_reference as NL
import rd_reference as RD
from test_gpu_ho import KERNEL_SHAPES, SENTINEL, Field, _p, _pitch, _ring, _same_bits, _scalar, _scratch, _spacings, _torch
from test_gpu_nl import K_ULP, _ulps

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
KIND_NAMES = ["linear", "cubic", "sinh", "exp"]
IE, CN, BDF2 = 1, 2, 3
SCHEME_NAMES = {IE: RD.IMPLICIT, CN: RD.CN, BDF2: RD.BDF2}


def _kernel_inputs(nx, ny):
    rng = np.random.default_rng(nx * 17 + ny)
    u = np.clip(6.0 * rng.standard_normal((nx, ny)), -15.0, 15.0)             # sinh, cosh and exp inside [-20, 20]
    up = np.clip(6.0 * rng.standard_normal((nx, ny)), -15.0, 15.0)
    S = 100.0 * rng.standard_normal((nx, ny))
    a = 1.0 + 0.5 * rng.random((nx, ny)) + 50.0 * (rng.random((nx, ny)) > 0.7)
    w = rng.random((nx, ny)) * (rng.random((nx, ny)) > 0.3)                   # zeros among the weights
    ring = np.zeros((nx, ny), dtype=bool); ring[0] = ring[-1] = True; ring[:, 0] = ring[:, -1] = True
    up[ring] = np.nan                                                         # the rings of u_prev, S and w are not used
    S[ring] = np.nan
    w[ring] = np.nan
    return u, up, S, a, w


def _rhs(scheme, kind, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, fu, fp, fs, fa, fw, g0, g1, fout, scratch, ssq):
    _lib.check(_lib.load().mg_dev_rd_rhs(scheme, kind, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, fu.ptr, fp.ptr if fp else None,
                                         fs.ptr if fs else None, fa.ptr if fa else None, fw.ptr if fw else None, g0, g1, fout.ptr,
                                         _p(scratch), _p(ssq), None))
    _torch().cuda.synchronize()
    return float(ssq.cpu()[0])


# ------------------------------------------------------------------------------------------ 1. the right-hand side, call by call
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d" % s for s in KERNEL_SHAPES])
def test_rhs_kernel(shape):
    nx, ny = shape
    ld = _pitch(ny)
    hx, hy = _spacings(nx, ny)
    u, up, S, a, w = _kernel_inputs(nx, ny)
    fu, fp, fs, fa, fw = Field(u, ld), Field(up, ld), Field(S, ld), Field(a, ld), Field(w, ld)
    scratch = _scratch(nx, ny)
    alpha, dt, kappa, rho, g0, g1 = 0.37, 0.013, 0.7, -1.9, 0.8, -1.25
    combos = [(IE, 0, False, False, vs, False) for vs in (False, True)] + [(BDF2, 0, False, False, vs, True) for vs in (False, True)]
    combos += [(CN, kind, va, vw, vs, vp) for kind in range(4) for va in (False, True) for vw in (False, True)
               for vs in (False, True) for vp in (False, True)]
    worst = {2: 0.0, 3: 0.0}
    for scheme, kind, va, vw, vs, vp in combos:
        want = RD.rhs(SCHEME_NAMES[scheme], kind, u, dt, alpha, hx, hy, kappa, rho, up if vp else None, S if vs else None,
                      a if va else None, w if vw else None, g0, g1)
        fout, ssq = Field(u, ld, fill=SENTINEL), _scalar()
        got_sum = _rhs(scheme, kind, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, fu, fp if vp else None, fs if vs else None,
                       fa if va else None, fw if vw else None, g0, g1, fout, scratch, ssq)
        what = "%s %s %dx%d a %s w %s S %s prev %s" % (SCHEME_NAMES[scheme], KIND_NAMES[kind], nx, ny, va, vw, vs, vp)
        assert fout.outside_untouched(), "stored outside [0, nx) x [0, ny): " + what
        got = fout.field()
        assert not _ring(got).any(), "ring: " + what
        if scheme != CN or kind < 2:
            assert _same_bits(got, want), "f: " + what
        else:
            i = slice(1, -1)
            kw = (kappa / alpha) * (w[i, i] if vw else 1.0)
            term = np.zeros_like(u)
            term[i, i] = kw * NL.phi(kind, u[i, i])[0]
            assert _ulps(got, want, term), "f: " + what
            d = np.abs(got - want)[i, i] / np.spacing(np.abs(term[i, i]) + np.abs(want[i, i]) + 1e-300)
            worst[kind] = max(worst[kind], float(d.max()))
        ref = math.fsum((got * got).ravel().tolist())
        assert abs(got_sum - ref) <= 1e-13 * ref, "sum f^2: %s: %r vs %r" % (what, got_sum, ref)
    print("%dx%d largest distance in ulp: sinh %r exp %r" % (nx, ny, worst[2], worst[3]))
    # implicit Euler and BDF2 read neither kind, a nor w; implicit Euler reads no u_prev
    for scheme in (IE, BDF2):
        plain, full = Field(u, ld, fill=SENTINEL), Field(u, ld, fill=SENTINEL)
        s1 = _rhs(scheme, 0, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, fu, fp if scheme == BDF2 else None, fs, None, None, g0, g1,
                  plain, scratch, _scalar())
        s2 = _rhs(scheme, 3, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, fu, fp, fs, fa, fw, g0, g1, full, scratch, _scalar())
        assert s1 == s2 and plain.numpy().tobytes() == full.numpy().tobytes(), scheme
    # two runs give identical bits; the sum is nullable
    one, two = Field(u, ld, fill=SENTINEL), Field(u, ld, fill=SENTINEL)
    s1 = _rhs(CN, 2, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, fu, fp, fs, fa, fw, g0, g1, one, scratch, _scalar())
    s2 = _rhs(CN, 2, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, fu, fp, fs, fa, fw, g0, g1, two, scratch, _scalar())
    assert s1 == s2 and one.numpy().tobytes() == two.numpy().tobytes()
    three = Field(u, ld, fill=SENTINEL)
    _lib.check(_lib.load().mg_dev_rd_rhs(CN, 2, nx, ny, ld, hx, hy, alpha, dt, kappa, rho, fu.ptr, fp.ptr, fs.ptr, fa.ptr, fw.ptr, g0, g1,
                                         three.ptr, _p(scratch), None, None))
    _torch().cuda.synchronize()
    assert three.numpy().tobytes() == one.numpy().tobytes()
    # kappa = rho = 0: the heat stepper's right-hand side, as numbers
    for scheme in (IE, CN, BDF2):
        for va in (False, True):
            for kind in ((0,) if scheme != CN else range(4)):
                mine, heat = Field(u, ld, fill=SENTINEL), Field(u, ld, fill=SENTINEL)
                s1 = _rhs(scheme, kind, nx, ny, ld, hx, hy, alpha, dt, 0.0, 0.0, fu, fp if scheme == BDF2 else None, fs,
                          fa if va else None, fw, g0, g1, mine, scratch, _scalar())
                ssq = _scalar()
                _lib.check(_lib.load().mg_dev_heat_rhs_var(scheme, nx, ny, ld, hx, hy, alpha, dt, fu.ptr, fp.ptr if scheme == BDF2 else None,
                                                           fs.ptr, fa.ptr if va else None, g0, g1, heat.ptr, _p(scratch), _p(ssq), None))
                _torch().cuda.synchronize()
                assert np.array_equal(mine.field(), heat.field()), (scheme, va, kind)
                assert abs(s1 - float(ssq.cpu()[0])) <= 1e-13 * s1
    for fld in (fu, fp, fs, fa, fw):
        assert fld.outside_untouched(whole=True), "an input was written"


# ------------------------------------------------------------------------------------------ 2. the energy sums, call by call
def _energy(kind, nx, ny, ld, hx, hy, fa, fw, fu, scratch):
    sums = _torch().full((3,), float("nan"), dtype=_torch().float64, device="cuda")
    _lib.check(_lib.load().mg_dev_rd_energy(kind, nx, ny, ld, hx, hy, fa.ptr if fa else None, fw.ptr if fw else None, fu.ptr,
                                            _p(scratch), _p(sums), None))
    _torch().cuda.synchronize()
    return [float(x) for x in sums.cpu()]


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d" % s for s in KERNEL_SHAPES])
def test_energy_kernel(shape):
    nx, ny = shape
    ld = _pitch(ny)
    hx, hy = _spacings(nx, ny)
    u, _, _, a, w = _kernel_inputs(nx, ny)
    fu, fa, fw = Field(u, ld), Field(a, ld), Field(w, ld)
    scratch = _scratch(nx, ny)
    tol = 1e-13 + (K_ULP + 1) * EPS
    for kind in range(4):
        for va in (False, True):
            for vw in (False, True):
                got = _energy(kind, nx, ny, ld, hx, hy, fa if va else None, fw if vw else None, fu, scratch)
                terms = RD.energy_terms(kind, u, hx, hy, a if va else None, w if vw else None)
                what = "%s %dx%d a %s w %s" % (KIND_NAMES[kind], nx, ny, va, vw)
                for name, g, t in zip("GPQ", got, terms):
                    assert np.all(t >= 0.0)
                    ref = math.fsum(t.ravel().tolist())
                    print(what, name, g, ref)
                    assert abs(g - ref) <= tol * ref, "%s: %s: %r vs %r" % (name, what, g, ref)
                assert _energy(kind, nx, ny, ld, hx, hy, fa if va else None, fw if vw else None, fu, scratch) == got, what
    # a NaN cell makes the sums it enters non-finite: an interior cell all three, a ring cell G alone, a corner none
    clean = _energy(1, nx, ny, ld, hx, hy, fa, fw, fu, scratch)
    for (bi, bj), enters in (((nx // 2, ny // 2), (True, True, True)), ((0, ny // 2), (True, False, False)),
                             ((nx // 2, ny - 1), (True, False, False)), ((nx - 1, ny - 1), (False, False, False))):
        ub = u.copy()
        ub[bi, bj] = np.nan
        got = _energy(1, nx, ny, ld, hx, hy, fa, fw, Field(ub, ld), scratch)
        for g, c, e in zip(got, clean, enters):
            assert (not math.isfinite(g)) if e else g == c, ((bi, bj), got, clean)
    for fld in (fu, fa, fw):
        assert fld.outside_untouched(whole=True), "an input was written"


# ------------------------------------------------------------------------------------------ the driver, through the C ABI
BASE = dict(x0=0.0, x1=1.0, y0=0.0, y1=1.0, coeff=-1.0, cycle=0, pre=2, post=2, smoother=0, omega=0.8, coarse_tol=1e-12,
            coarse_maxit=1000, switch_threshold=1e-6, memory_threshold_gb=4.0, adaptive_reference_rule=0, device=0, profile=0,
            colour_offset=0, fused=2, tail=1, fmg_cycles=0, speculate=2, coarse_direct=0, mixed_split=0)


class Stepper:
    """a thin owner of one mg_rd"""

    def __init__(self, nx, ny, alpha, precision=_lib.MG_PREC_DOUBLE, max_levels=3):
        self.lib = _lib.load()
        self.nx, self.ny, self.alpha = nx, ny, alpha
        self.hx, self.hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
        cfg = _lib.MgConfig(**dict(BASE, nx=nx, ny=ny, max_levels=max_levels, precision=precision))
        self.h = C.c_void_p(None)
        _lib.check(self.lib.mg_rd_create(C.byref(cfg), alpha, 1, -1, C.byref(self.h)))

    def close(self):
        if self.h.value:
            self.lib.mg_rd_destroy(self.h)
            self.h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def ok(self, rc):
        assert rc == _lib.MG_OK, (rc, self.lib.mg_rd_last_error(self.h))

    def set(self, slot, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        self.ok(self.lib.mg_rd_set_slot(self.h, slot, _lib.ptr(u), _lib.MG_F64))

    def get(self, slot):
        out = np.empty((self.nx, self.ny))
        self.ok(self.lib.mg_rd_get_slot(self.h, slot, _lib.ptr(out), _lib.MG_F64))
        return out

    def fields(self, a=None, S=None):
        for fn, arr in ((self.lib.mg_rd_set_coefficient, a), (self.lib.mg_rd_set_source, S)):
            arr = None if arr is None else np.ascontiguousarray(arr, dtype=np.float64)
            self.ok(fn(self.h, None if arr is None else _lib.ptr(arr), _lib.MG_F64))

    def reaction(self, kind, kappa, w=None, rho=0.0):
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        return self.lib.mg_rd_set_reaction(self.h, kind, kappa, None if w is None else _lib.ptr(w), _lib.MG_F64, rho)

    def step_rc(self, scheme, dt, src, prev, dst, g0=1.0, g1=1.0, edge4=None, tol=1e-10, max_newton=30):
        info = _lib.MgRdStepInfo()
        e = None if edge4 is None else (C.c_double * 4)(*edge4)
        return self.lib.mg_rd_step(self.h, scheme, dt, src, prev, dst, g0, g1, e, tol, max_newton, C.byref(info)), info

    def step(self, *args, **kw):
        rc, info = self.step_rc(*args, **kw)
        self.ok(rc)
        return info

    def energy(self, slot):
        out = (C.c_double * 4)()
        self.ok(self.lib.mg_rd_energy(self.h, slot, out))
        return list(out)

    def diff(self, sa, sb):
        out = C.c_double(0.0)
        self.ok(self.lib.mg_rd_diff_norm(self.h, sa, sb, C.byref(out)))
        return out.value


def _norm_h(d, hx, hy):
    return float(np.sqrt(hx * hy * np.sum(d[1:-1, 1:-1] ** 2)))


def _step_problem(nx, ny):
    """jumping a, w with zeros, a source, two states with non-zero rings"""
    rng = np.random.default_rng(nx * 3 + ny)
    X, Y = NL.mesh(nx, ny)
    a = np.where((X - 0.5) ** 2 + (Y - 0.5) ** 2 < 0.09, 30.0, 1.0)
    w = rng.random((nx, ny)) * (rng.random((nx, ny)) > 0.3)
    S = 3.0 * np.sin(np.pi * X) * np.cos(2 * np.pi * Y)
    u0 = 0.8 * np.sin(2 * np.pi * X) * np.cos(np.pi * Y) + 0.2 * rng.standard_normal((nx, ny))
    u1 = u0 + 0.05 * rng.standard_normal((nx, ny))
    return a, w, S, u0, u1


_REFERENCE_STEPS = {}


def _reference_step(key, *args, **kw):
    """rd_reference.step, computed once per distinct input and shared between the precisions"""
    if key not in _REFERENCE_STEPS:
        _REFERENCE_STEPS[key] = RD.step(*args, **kw)
    return _REFERENCE_STEPS[key]


# ------------------------------------------------------------------------------------------ 3. one step against the reference
@pytest.mark.parametrize("precision", ["double", "single_managed"])
@pytest.mark.parametrize("kind", [1, 2], ids=["cubic", "sinh"])
@pytest.mark.parametrize("shape", [(17, 17), (17, 33)], ids=["17x17", "17x33"])
def test_one_step_against_the_dense_newton(shape, kind, precision):
    nx, ny = shape
    alpha, kappa, rho, dt, tol = 0.3, 2.0, 1.5, 0.01, 1e-10
    a, w, S, u0, u1 = _step_problem(nx, ny)
    edge4 = (0.3, -0.2, 0.1, 0.45)
    with Stepper(nx, ny, alpha, mg.krylov.PRECISIONS[precision]) as s:
        s.fields(a, S)
        s.ok(s.reaction(kind, kappa, w, rho))
        s.set(0, u0)
        s.set(1, u1)
        for scheme, prev in ((IE, -1), (CN, -1), (CN, 0), (BDF2, 0)):
            info = s.step(scheme, dt, 1, prev, 2, 0.7, 1.1, edge4, tol)
            got = s.get(2)
            want, ri = _reference_step((nx, ny, kind, scheme, prev), SCHEME_NAMES[scheme], kind, u1, dt, alpha, kappa, rho,
                                       u_prev=u0 if prev >= 0 else None, S=S, a=a, w=w, g0=0.7, g1=1.1, edge4=edge4, tol=tol)
            lam = RD.lam(SCHEME_NAMES[scheme], dt, alpha)
            err, bound = _norm_h(got - want, s.hx, s.hy), (info.final_residual + ri["final_residual"]) / lam
            print(SCHEME_NAMES[scheme], KIND_NAMES[kind], shape, precision, "prev", prev, "newton", info.newton_iterations, "inner",
                  info.inner_iterations, "residuals", info.final_residual, ri["final_residual"], "error", err, "bound", bound)
            assert info.converged == 1 and info.status == 0 and ri["converged"]
            assert getattr(info, "lambda") == lam and info.rhs_norm == pytest.approx(ri["rhs_norm"], rel=1e-12)
            assert info.final_residual < tol * max(1.0, info.rhs_norm)
            assert _ring(got).tobytes() == _ring(want).tobytes()
            assert err <= bound


def test_float32_host_arrays_give_the_bits_of_their_float64_values():
    """mg_rd_set_coefficient, mg_rd_set_source, mg_rd_set_reaction and mg_rd_set_slot with float32 host arrays (staged in fp32,
    cast to fp64 on the device) against the same calls with the same values as float64: the cast is exact, so the slot and a
    Crank-Nicolson step give the same bits."""
    nx, ny = 17, 33
    a, w, S, u0, _ = (f.astype(np.float32) for f in _step_problem(nx, ny))
    out = []
    for dt, code in ((np.float32, _lib.MG_F32), (np.float64, _lib.MG_F64)):
        fa, fw, fS, fu = (np.ascontiguousarray(f, dtype=dt) for f in (a, w, S, u0))
        with Stepper(nx, ny, 0.3) as s:
            s.ok(s.lib.mg_rd_set_coefficient(s.h, _lib.ptr(fa), code))
            s.ok(s.lib.mg_rd_set_source(s.h, _lib.ptr(fS), code))
            s.ok(s.lib.mg_rd_set_reaction(s.h, 1, 2.0, _lib.ptr(fw), code, 1.5))
            s.ok(s.lib.mg_rd_set_slot(s.h, 1, _lib.ptr(fu), code))
            info = s.step(CN, 0.01, 1, -1, 2, 0.7, 1.1, None, 1e-10)
            out.append((s.get(1), s.get(2), info.newton_iterations, info.inner_iterations, info.final_residual))
    assert out[0][0].tobytes() == u0.astype(np.float64).tobytes()
    assert np.isfinite(out[0][1]).all() and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2:] == out[1][2:]


@pytest.mark.parametrize("precision", ["double", "single_managed"])
def test_bdf2_run_step_by_step(precision):
    """8 steps (Crank-Nicolson, then BDF2), each compared with the reference's step from the DEVICE's own two states"""
    nx, ny, kind = 17, 33, 1
    alpha, kappa, rho, dt, tol = 0.3, 2.0, 1.5, 0.01, 1e-10
    a, w, S, u0, _ = _step_problem(nx, ny)
    g = lambda t: math.cos(3.0 * t)
    with Stepper(nx, ny, alpha, mg.krylov.PRECISIONS[precision]) as s:
        s.fields(a, S)
        s.ok(s.reaction(kind, kappa, w, rho))
        s.set(0, u0)
        cur, prev = 0, -1
        for k in range(8):
            scheme = CN if k == 0 else BDF2
            dst = next(j for j in range(4) if j not in (cur, prev))
            t = k * dt
            edge4 = (0.1 * (k + 1), -0.05 * k, 0.02, 0.3)
            u_cur, u_prev = s.get(cur), (s.get(prev) if prev >= 0 else None)
            info = s.step(scheme, dt, cur, prev, dst, g(t), g(t + dt), edge4, tol)
            got = s.get(dst)
            want, ri = RD.step(SCHEME_NAMES[scheme], kind, u_cur, dt, alpha, kappa, rho, u_prev=u_prev, S=S, a=a, w=w, g0=g(t),
                               g1=g(t + dt), edge4=edge4, tol=tol)
            lam = RD.lam(SCHEME_NAMES[scheme], dt, alpha)
            err, bound = _norm_h(got - want, s.hx, s.hy), (info.final_residual + ri["final_residual"]) / lam
            print("step", k, SCHEME_NAMES[scheme], precision, "newton", info.newton_iterations, "error", err, "bound", bound)
            assert info.converged == 1 and ri["converged"] and err <= bound
            assert s.get(cur).tobytes() == u_cur.tobytes()
            prev, cur = cur, dst


# ------------------------------------------------------------------------------------------ 4. the eigenmode factors
@pytest.mark.parametrize("case", [(IE, None), (CN, None), (CN, 0.8), (BDF2, 1.15)], ids=["implicit_euler", "cn", "cn_ab2", "bdf2"])
def test_eigenmode_factors(case):
    """linear kind on sin(pi x) sin(pi y), scaled so that ||f||_h < 1: the step stops at ||F||_h < tol, so its distance to
    factor * phi is below tol / lambda in the h-norm (plus the rounding of forming factor * phi)"""
    scheme, c = case
    nx, ny, dt, alpha, kappa, rho, tol = 17, 33, 0.02, 0.3, 2.5, 1.75, 1e-10
    phi, lam_h = RD.eigenmode(nx, ny)
    phi = 1e-3 * phi
    with Stepper(nx, ny, alpha) as s:
        s.ok(s.reaction(0, kappa, None, rho))
        s.set(0, phi)
        if c is not None:
            s.set(1, c * phi)
        info = s.step(scheme, dt, 0, -1 if c is None else 1, 2, tol=tol)
        got = s.get(2)
    factor = RD.eigen_factor(SCHEME_NAMES[scheme], dt, alpha, lam_h, kappa, rho, c)
    lam = RD.lam(SCHEME_NAMES[scheme], dt, alpha)
    err = _norm_h(got - factor * phi, 1.0 / (nx - 1), 1.0 / (ny - 1))
    print(SCHEME_NAMES[scheme], c, "factor", factor, "error", err, "tol / lambda", tol / lam, "rhs norm", info.rhs_norm)
    assert info.converged == 1 and info.rhs_norm < 1.0 and info.final_residual < tol
    assert err <= tol / lam + 8 * EPS * _norm_h(phi, 1.0 / (nx - 1), 1.0 / (ny - 1))


# ------------------------------------------------------------------------------------------ 5. energy decay
@pytest.mark.parametrize("dt", [0.1, 1.0, 10.0, 100.0])
def test_convex_splitting_decreases_the_energy(dt):
    """Allen-Cahn by convex splitting (implicit Euler, cubic implicit, +u explicit), zero ring, from noise: after every step
    E_new - E <= -||d||_h^2 / dt + r ||d||_h + rounding, d = u_new - u, r the step's final residual; the rounding term is
    N eps sum |terms| over the terms of both energies"""
    n, alpha, kappa, rho, tol = 33, 1e-3, 1.0, 1.0, 1e-8
    rng = np.random.default_rng(11)
    u0 = np.zeros((n, n))
    u0[1:-1, 1:-1] = 0.1 * rng.standard_normal((n - 2, n - 2))
    with Stepper(n, n, alpha, max_levels=4) as s:
        s.ok(s.reaction(1, kappa, None, rho))
        s.set(0, u0)
        cur = 0
        E = s.energy(cur)
        for k in range(12):
            dst = cur ^ 1
            info = s.step(IE, dt, cur, -1, dst, tol=tol)
            E_new = s.energy(dst)
            d = s.diff(cur, dst)
            u_old, u_new = s.get(cur), s.get(dst)
            mags = 0.0
            for v in (u_old, u_new):
                G, P, Q = (math.fsum(t.ravel().tolist()) for t in RD.energy_terms(1, v, s.hx, s.hy))
                mags += alpha * G + s.hx * s.hy * (kappa * P + rho * Q / 2)
            rounding = 3 * n * n * EPS * mags
            lhs, rhs = E_new[3] - E[3], -d * d / dt + info.final_residual * d + rounding
            print("dt", dt, "step", k, "E", E_new[3], "dE", lhs, "bound", rhs, "max |u|", float(np.max(np.abs(u_new))), "newton",
                  info.newton_iterations)
            assert info.converged == 1
            assert d == pytest.approx(_norm_h(u_new - u_old, s.hx, s.hy), rel=1e-12)
            ref = RD.energy(1, u_new, s.hx, s.hy, alpha, kappa, rho)
            assert E_new[3] == pytest.approx(ref["energy"], rel=1e-12, abs=rounding)
            assert lhs <= rhs
            cur, E = dst, E_new


# ------------------------------------------------------------------------------------------ 6. driver semantics
def test_driver_semantics_and_refusals():
    nx, ny, alpha, dt = 17, 33, 0.3, 0.01
    a, w, S, u0, u1 = _step_problem(nx, ny)
    I = _lib.MG_ERR_INVALID_VALUE
    with Stepper(nx, ny, alpha) as s:
        s.fields(a, S)
        s.ok(s.reaction(1, 2.0, w, 1.5))
        s.set(0, u0)
        s.set(1, u1)
        # src and prev keep their bits; two equal steps report the same lambda and give the same bits
        i1 = s.step(BDF2, dt, 1, 0, 2)
        first = s.get(2)
        i2 = s.step(BDF2, dt, 1, 0, 3)
        assert s.get(0).tobytes() == u0.tobytes() and s.get(1).tobytes() == u1.tobytes()
        assert getattr(i1, "lambda") == getattr(i2, "lambda") == 3.0 / (2 * dt * alpha)
        assert s.get(3).tobytes() == first.tobytes() and i1.final_residual == i2.final_residual
        # another lambda in between, then the first again: the same bits once more
        s.step(IE, 2 * dt, 1, -1, 3)
        s.step(BDF2, dt, 1, 0, 3)
        assert s.get(3).tobytes() == first.tobytes()
        # the ring: NULL keeps src's, edge4 overwrites it in the heat stepper's order (corners carry bottom / top)
        assert _ring(first).tobytes() == _ring(u1).tobytes()
        edge4 = (1.0, 2.0, 3.0, 4.0)
        s.step(CN, dt, 1, 0, 2, edge4=edge4)
        got = s.get(2)
        want = RD.set_ring(u1.copy(), edge4)
        assert _ring(got).tobytes() == _ring(want).tobytes()
        assert (got[0, 0], got[0, -1], got[-1, 0], got[-1, -1], got[0, 5], got[-1, 5]) == (3.0, 4.0, 3.0, 4.0, 1.0, 2.0)
        # the difference norm
        assert s.diff(1, 2) == pytest.approx(float(np.sqrt(s.hx * s.hy * np.sum((u1 - got) ** 2))), rel=1e-13)
        assert s.diff(2, 2) == 0.0
        # every refusal leaves the stepper as it was
        before = [s.get(k).tobytes() for k in range(4)]
        nan, inf = float("nan"), float("inf")
        for args in ((IE, dt, 4, -1, 1), (IE, dt, 0, -1, 4), (IE, dt, -1, -1, 1), (IE, dt, 0, -1, 0), (IE, dt, 0, 2, 1),
                     (CN, dt, 0, 1, 1), (CN, dt, 0, 7, 1), (BDF2, dt, 0, -1, 1), (BDF2, dt, 0, 1, 1), (BDF2, dt, 0, 4, 1),
                     (IE, 0.0, 0, -1, 1), (IE, -dt, 0, -1, 1), (IE, inf, 0, -1, 1), (IE, nan, 0, -1, 1), (0, dt, 0, -1, 1),
                     (4, dt, 0, -1, 1), (-1, dt, 0, -1, 1)):
            rc, _ = s.step_rc(*args)
            assert rc == I, args
        assert b"mg_rd_step" in s.lib.mg_rd_last_error(s.h)
        assert s.step_rc(IE, dt, 0, -1, 1, max_newton=0)[0] == I and s.step_rc(IE, dt, 0, -1, 1, tol=nan)[0] == I
        assert s.step_rc(IE, dt, 0, -1, 1, g0=inf)[0] == I
        for kind, kappa, wt, rho in ((4, 1.0, None, 0.0), (-1, 1.0, None, 0.0), (1, -1.0, None, 0.0), (1, nan, None, 0.0),
                                     (1, 1.0, None, nan), (1, 1.0, None, inf), (1, 1.0, -np.ones((nx, ny)), 0.0),
                                     (1, 1.0, np.full((nx, ny), nan), 0.0)):
            assert s.reaction(kind, kappa, wt, rho) == I, (kind, kappa, rho)
        bad = a.copy(); bad[3, 4] = 0.0
        assert s.lib.mg_rd_set_coefficient(s.h, _lib.ptr(bad), _lib.MG_F64) == I
        out4 = (C.c_double * 4)()
        assert s.lib.mg_rd_energy(s.h, 4, out4) == I and s.lib.mg_rd_diff_norm(s.h, 0, -1, out4) == I
        assert s.lib.mg_rd_set_slot(s.h, 4, _lib.ptr(u0), _lib.MG_F64) == I and s.lib.mg_rd_get_slot(s.h, -1, _lib.ptr(u0), _lib.MG_F64) == I
        assert [s.get(k).tobytes() for k in range(4)] == before
        s.step(BDF2, dt, 1, 0, 3)                                              # the reaction and the field are the ones set before
        assert s.get(3).tobytes() == first.tobytes()
    # max_newton = 1 on a stiff cubic step: unconverged, not an error, dst finite
    with Stepper(nx, ny, 1e-3) as s:
        s.ok(s.reaction(1, 50.0, None, 0.0))
        s.set(0, 3.0 * u0)
        rc, info = s.step_rc(IE, 10.0, 0, -1, 1, max_newton=1)
        print("stiff step: status", info.status, "residuals", info.initial_residual, info.final_residual)
        assert rc == _lib.MG_OK and info.converged == 0 and info.status != 0 and info.newton_iterations <= 1
        assert np.all(np.isfinite(s.get(1))) and info.final_residual <= info.initial_residual


# ------------------------------------------------------------------------------------------ 7. the Python class
def test_reaction_diffusion_solver():
    n = 33
    grid = mg.Grid(n, n)
    rng = np.random.default_rng(2)
    u0 = np.zeros((n, n))
    u0[1:-1, 1:-1] = 0.1 * rng.standard_normal((n - 2, n - 2))
    with mg.ReactionDiffusionSolver(grid, 1e-3, nonlinearity="cubic", strength=1.0, linear_growth=1.0, scheme="implicit_euler") as s:
        s.set_state(u0)
        e0 = s.energy()
        ref = RD.energy(1, u0, grid.hx, grid.hy, 1e-3, 1.0, 1.0)
        assert e0["energy"] == pytest.approx(ref["energy"], rel=1e-12) and e0["sum_squares"] == pytest.approx(ref["sum_squares"], rel=1e-13)
        times, states = s.advance(1.0, 0.1, save_interval=4)
        assert np.allclose(times, [0.0, 0.4, 0.8, 1.0]) and len(states) == 4 and s.steps == 10 and s.time == 1.0
        assert states[0].tobytes() == u0.tobytes() and states[-1].tobytes() == s.state.tobytes()
        assert all(h[3] for h in s.history)
        assert s.energy()["energy"] < e0["energy"]
        # a device round trip
        torch = _torch()
        t = torch.zeros((n, n + 6), dtype=torch.float64, device="cuda")
        s.get_device(t)
        assert t[:, :n].cpu().numpy().tobytes() == s.state.tobytes()
        s.set_device(2.0 * t)
        assert s.state.tobytes() == (2.0 * states[-1]).tobytes()
        s.close()
        s.close()
    # BDF2 with a separable source, a field and a weight: Crank-Nicolson first, then BDF2; an unconverged step raises
    X, Y = grid.X, grid.Y
    src = mg.SeparableSource(lambda x, y: np.sin(np.pi * x) * np.sin(2 * np.pi * y), lambda t: math.cos(3.0 * t))
    with mg.ReactionDiffusionSolver(grid, 0.05, strength=4.0, linear_growth=3.0, source=src, conductivity=lambda x, y: 1.0 + x,
                                    weight=np.ones((n, n)), scheme="bdf2", precision="single_managed") as s:
        s.set_state(1.5 * np.sin(np.pi * X) * np.sin(np.pi * Y))
        infos = [s.step(0.01) for _ in range(3)]
        assert [i["scheme"] for i in infos] == ["crank_nicolson", "bdf2", "bdf2"] and all(i["converged"] for i in infos)
        assert infos[1]["lambda"] == 3.0 / (2 * 0.01 * 0.05)
        s.max_newton = 1
        s.tolerance = 1e-14
        with pytest.raises(RuntimeError, match="step 4.*max_newton"):
            s.advance(1.0, 0.3)
