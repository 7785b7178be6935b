"""The semilinear Newton method on a GPU (include/mghip_nl.h, csrc/mg_nl.hip, nonlinear.py): the eval kernel and the
reaction-field direction kernel call by call against the NumPy restatement tests/nl_reference.py (pinned on the CPU by
tests/test_nl_cpu.py); conjugate gradients with a reaction field; whole Newton solves.

Kernel shapes and the Field / sentinel / guard-row harness are those of tests/test_gpu_ho.py: 34 x 67 and 70 x 131 are the
smallest shapes with a second tile row, a second tile column, a partial last tile and an odd ny whose last vector is half pad.

sinh, cosh and exp are the device math library's: K_ULP is twice the largest distance to NumPy's measured on the device over
[-20, 20], and the kernel's F and c may differ from the restatement's by K_ULP ulp of the g (resp. c) term
plus one ulp of the result.  Everything else the kernel computes is pinned bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib

import nl_reference as NL
import pcg_reference as R
from test_gpu_ho import KERNEL_SHAPES, OPERATORS, SENTINEL, Field, _p, _pitch, _ring, _same_bits, _scalar, _scratch, _spacings, _torch

pytestmark = pytest.mark.gpu

K_ULP = 2            # 2 x the measured 1 ulp (sinh, cosh, exp against NumPy on [-20, 20])
KIND_NAMES = ["linear", "cubic", "sinh", "exp"]
LMIN = 19.0          # lambda_min(-Laplacian_h) >= 19.7 on the unit square for h <= 1/32


def _sums():
    return _torch().full((2,), float("nan"), dtype=_torch().float64, device="cuda")


def _kernel_inputs(nx, ny):
    rng = np.random.default_rng(nx * 13 + ny)
    u = np.clip(6.0 * rng.standard_normal((nx, ny)), -15.0, 15.0)             # v = u + t delta stays inside [-20, 20]
    delta = np.clip(2.0 * rng.standard_normal((nx, ny)), -5.0, 5.0)
    f = 100.0 * rng.standard_normal((nx, ny))
    a = 1.0 + 0.5 * rng.random((nx, ny)) + 50.0 * (rng.random((nx, ny)) > 0.7)
    w = rng.random((nx, ny)) * (rng.random((nx, ny)) > 0.3)                   # zeros among the weights
    ring = np.zeros((nx, ny), dtype=bool); ring[0] = ring[-1] = True; ring[:, 0] = ring[:, -1] = True
    delta[ring] = np.nan                                                      # the rings of delta and f are not read
    f[ring] = np.nan
    return u, delta, f, a, w


def _eval(kind, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa, fw, fu, fd, t, ff, outs, scratch, sums):
    fuo, fF, fc = outs
    _lib.check(_lib.load().mg_dev_nl_eval(kind, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa.ptr if fa else None, fw.ptr if fw else None,
                                          fu.ptr, fd.ptr if fd else None, t, ff.ptr, fuo.ptr if fuo else None, fF.ptr if fF else None,
                                          fc.ptr if fc else None, _p(scratch), _p(sums), None))
    _torch().cuda.synchronize()
    return [float(x) for x in sums.cpu()]


def _ulps(got, want, term):
    """|got - want| <= K_ULP ulp of `term` + one ulp of the result"""
    return bool(np.all(np.abs(got - want) <= K_ULP * np.spacing(np.abs(term)) + np.spacing(np.abs(want))))


# ------------------------------------------------------------------------------------------ 1. the eval kernel, call by call
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d" % s for s in KERNEL_SHAPES])
def test_eval_kernel(shape):
    nx, ny = shape
    ld = _pitch(ny)
    hx, hy = _spacings(nx, ny)
    u, delta, f, a, w = _kernel_inputs(nx, ny)
    fu, fd, ff, fa, fw = Field(u, ld), Field(delta, ld), Field(f, ld), Field(a, ld), Field(w, ld)
    scratch = _scratch(nx, ny)
    kappa = 0.7
    combos = [(va, vw, t) for va in (False, True) for vw in (False, True) for t in (None, 1.0, 0.25)]
    worst = {2: [0.0, 0.0], 3: [0.0, 0.0]}
    for kind in range(4):
        for n, (va, vw, t) in enumerate(combos):
            sigma, coeff = OPERATORS[(n + kind) % len(OPERATORS)]
            want = NL.evaluate(kind, u, f, hx, hy, coeff, sigma, kappa, a if va else None, w if vw else None,
                               None if t is None else delta, 1.0 if t is None else t)
            outs = [Field(u, ld, fill=SENTINEL) for _ in range(3)]
            sums = _sums()
            got = _eval(kind, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa if va else None, fw if vw else None, fu,
                        None if t is None else fd, 7.0 if t is None else t, ff, outs, scratch, sums)
            what = "%s %dx%d var %s w %s t %r sigma %g coeff %g" % (KIND_NAMES[kind], nx, ny, va, vw, t, sigma, coeff)
            assert all(o.outside_untouched() for o in outs), "stored outside [0, nx) x [0, ny): " + what
            gF, gc = outs[1].field(), outs[2].field()
            if t is None:
                assert outs[0].outside_untouched(whole=True), "u_out is ignored without delta: " + what
            else:
                assert _same_bits(outs[0].field(), want["v"]), "u_out: " + what
                assert _ring(outs[0].field()).tobytes() == _ring(u).tobytes(), "ring of u_out: " + what
            assert not _ring(gF).any() and not _ring(gc).any(), "rings of F and c: " + what
            if kind < 2:
                assert _same_bits(gF, want["F"]), "F: " + what
                assert _same_bits(gc, want["c"]), "c: " + what
            else:
                assert _ulps(gF, want["F"], want["g"]), "F: " + what
                assert _ulps(gc, want["c"], want["c"]), "c: " + what
                i = slice(1, -1)
                dF = np.abs(gF - want["F"])[i, i] / np.spacing(np.abs(want["g"][i, i]) + np.abs(want["F"][i, i]) + 1e-300)
                dc = np.abs(gc - want["c"])[i, i] / np.spacing(np.abs(want["c"][i, i]) + 1e-300)
                worst[kind] = [max(worst[kind][0], float(dF.max())), max(worst[kind][1], float(dc.max()))]
            ref = (math.fsum((gF * gF).ravel().tolist()), math.fsum(gc.ravel().tolist()))
            assert abs(got[0] - ref[0]) <= 1e-13 * ref[0], "sum F^2: %s: %r vs %r" % (what, got[0], ref[0])
            assert abs(got[1] - ref[1]) <= 1e-13 * abs(ref[1]), "sum c: %s: %r vs %r" % (what, got[1], ref[1])
    print("%dx%d largest distance in ulp (F, c): sinh %r exp %r" % (nx, ny, worst[2], worst[3]))
    # each output is nullable: the others and the sums keep their bits; two runs give identical bits
    sigma, coeff = OPERATORS[1]
    full = [Field(u, ld, fill=SENTINEL) for _ in range(3)]
    s_full = _eval(2, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa, fw, fu, fd, 0.25, ff, full, scratch, _sums())
    again = [Field(u, ld, fill=SENTINEL) for _ in range(3)]
    assert _eval(2, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa, fw, fu, fd, 0.25, ff, again, scratch, _sums()) == s_full
    assert all(x.numpy().tobytes() == y.numpy().tobytes() for x, y in zip(full, again))
    for skip in range(3):
        outs = [None if k == skip else Field(u, ld, fill=SENTINEL) for k in range(3)]
        assert _eval(2, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa, fw, fu, fd, 0.25, ff, outs, scratch, _sums()) == s_full
        assert all(o is None or o.numpy().tobytes() == x.numpy().tobytes() for o, x in zip(outs, full)), skip
    s_none = _eval(2, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa, fw, fu, fd, 0.25, ff, [None, None, None], scratch, _sums())
    assert s_none == s_full
    # a non-finite cell of u: the sum of F^2 is non-finite, the cells outside its stencil are unaffected
    for bad in (np.nan, np.inf):
        ub = u.copy()
        bi, bj = nx // 2, ny // 2
        ub[bi, bj] = bad
        outs = [Field(u, ld, fill=SENTINEL) for _ in range(3)]
        s_bad = _eval(1, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa, fw, Field(ub, ld), None, 0.0, ff, outs, scratch, _sums())
        good = [Field(u, ld, fill=SENTINEL) for _ in range(3)]
        _eval(1, nx, ny, ld, hx, hy, coeff, sigma, kappa, fa, fw, fu, None, 0.0, ff, good, scratch, _sums())
        assert not math.isfinite(s_bad[0])
        far = np.ones((nx, ny), dtype=bool)
        far[bi, bj] = far[bi - 1, bj] = far[bi + 1, bj] = far[bi, bj - 1] = far[bi, bj + 1] = False
        assert _same_bits(outs[1].field()[far], good[1].field()[far])
        far[bi - 1, bj] = far[bi + 1, bj] = far[bi, bj - 1] = far[bi, bj + 1] = True
        assert _same_bits(outs[2].field()[far], good[2].field()[far])
    for fld in (fu, fd, ff, fa, fw):
        assert fld.outside_untouched(whole=True), "an input was written"
    # the host-array form is the same kernel
    hF, hc, hs = np.full((nx, ny), SENTINEL), np.full((nx, ny), SENTINEL), np.zeros(2)
    f0 = np.where(np.isnan(f), 0.0, f)
    _lib.check(_lib.load().mg_op_nl_eval(1, nx, ny, hx, hy, coeff, sigma, kappa, _lib.ptr(a), _lib.ptr(w), _lib.ptr(u), None, 0.0,
                                         _lib.ptr(f0), None, _lib.ptr(hF), _lib.ptr(hc), _lib.ptr(hs)))
    want = NL.evaluate(1, u, f0, hx, hy, coeff, sigma, kappa, a, w)
    assert _same_bits(hF, want["F"]) and _same_bits(hc, want["c"]) and abs(hs[0] - want["sums"][0]) <= 1e-13 * want["sums"][0]


# ------------------------------------------------------------------------------------------ 2. the reaction-field direction kernel
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d" % s for s in KERNEL_SHAPES])
def test_direction_kernel_with_a_reaction_field(shape):
    nx, ny = shape
    lib, ld = _lib.load(), _pitch(ny)
    hx, hy = _spacings(nx, ny)
    rng = np.random.default_rng(nx * 17 + ny)
    z, p = rng.standard_normal((nx, ny)), rng.standard_normal((nx, ny))          # their rings are not read
    a = 1.0 + 0.5 * rng.random((nx, ny)) + 50.0 * (rng.random((nx, ny)) > 0.7)
    c = 300.0 * rng.random((nx, ny))
    c[:, : ny // 2] = 0.0                                                         # zero on half the grid
    c[0] = c[-1] = np.nan; c[:, 0] = c[:, -1] = np.nan                             # its ring is not used
    fz, fp, fa, fcr = Field(z, ld), Field(p, ld), Field(a, ld), Field(c, ld)
    scratch = _scratch(nx, ny)
    for n, (sigma, coeff) in enumerate(OPERATORS):
        for coef in (None, a):
            beta = None if n % 2 else -0.625
            want_p = R.zero_ring(z) if beta is None else R.zero_ring(z + beta * p)
            want_q = NL.apply_A(want_p, hx, hy, coeff, sigma, coef)
            want_q[1:-1, 1:-1] = want_q[1:-1, 1:-1] + c[1:-1, 1:-1] * want_p[1:-1, 1:-1]
            fpo, fq = Field(z, ld, fill=SENTINEL), Field(z, ld, fill=SENTINEL)
            pq = _scalar()
            bdev = None if beta is None else _scalar(beta)
            _lib.check(lib.mg_dev_pcg_direction_react(nx, ny, ld, hx, hy, coeff, sigma, fa.ptr if coef is not None else None, fcr.ptr,
                                                      fz.ptr, fp.ptr, fpo.ptr, fq.ptr, None if bdev is None else _p(bdev),
                                                      _p(scratch), _p(pq), None))
            _torch().cuda.synchronize()
            what = "%dx%d sigma %g coeff %g var %s beta %r" % (nx, ny, sigma, coeff, coef is not None, beta)
            assert fpo.outside_untouched() and fq.outside_untouched(), "stored outside [0, nx) x [0, ny): " + what
            assert _same_bits(fpo.field(), want_p), "p: " + what
            assert _same_bits(fq.field(), want_q), "q: " + what
            assert not _ring(fq.field()).any(), "ring: " + what
            ref = math.fsum((want_p * want_q).ravel().tolist())
            assert abs(float(pq.cpu()[0]) - ref) <= 1e-13 * abs(ref), "p.q: %s" % what
    for fld in (fz, fp, fa, fcr):
        assert fld.outside_untouched(whole=True), "an input was written"


# ------------------------------------------------------------------------------------------ 3. conjugate gradients with a reaction field
def _smoother():
    return mg.JacobiSmoother(relaxation_parameter=0.8)


def _pcg(n, tol, a=None, order=2):
    s = mg.PCGSolver(max_levels=R.full_levels(n, n), max_iterations=60, tolerance=tol, pre_smooth_iterations=2, post_smooth_iterations=2,
                     order=order)
    s.setup(mg.Grid(n, n), mg.LaplacianOperator(coefficient=-1.0) if a is None else mg.DiffusionOperator(a), smoother=_smoother())
    return s


def _device_field(c):
    """c in the solver's pitch on the device -> (tensor, pointer, pitch)"""
    nx, ny = c.shape
    ld = _pitch(ny) - 8
    host = np.zeros((nx, ld))
    host[:, :ny] = c
    t = _torch().from_numpy(host).cuda()
    return t, C.c_void_p(t.data_ptr()), ld


def _l2(v, n):
    return float(np.sqrt(np.sum(v * v)) / (n - 1))


def test_pcg_constant_reaction_field_is_the_shifted_solve():
    n, sigma, s0 = 65, 0.37, 40.0
    lib = _lib.load()
    b = R.random_rhs(n, n, 7)
    tol = 1e-10 * _l2(b, n)
    shifted = _pcg(n, tol)
    want, winfo = shifted.solve(shifted.grid, mg.HelmholtzOperator(sigma + s0), b)
    shifted.close()
    s = _pcg(n, tol)
    t, cptr, ld = _device_field(R.zero_ring(np.full((n, n), s0)))
    assert lib.mg_pcg_set_reaction_device(s._engine._h, cptr, ld, s0) == _lib.MG_OK
    got, info = s.solve(s.grid, mg.HelmholtzOperator(sigma), b)
    s.close()
    err = _l2(got - want, n)
    print("iterations", info["iterations"], winfo["iterations"], "||x - x_shift||_h", err, "tol / lambda_min", tol / (LMIN + sigma + s0),
          "true residuals", info["true_residual"], winfo["true_residual"])
    assert info["converged"] and winfo["converged"]
    assert abs(info["iterations"] - winfo["iterations"]) <= 1
    assert err <= tol / (LMIN + sigma + s0)
    assert abs(info["true_residual"] - info["final_residual"]) <= 1e-2 * info["final_residual"]


@pytest.mark.parametrize("var", [False, True], ids=["laplace", "varcoef"])
def test_pcg_checkerboard_reaction_field_equals_the_restated_loop(var):
    n = 65
    lib = _lib.load()
    a = R.smooth_coefficient(n, n) if var else None
    c = R.zero_ring(np.where(R.checkerboard(n, n, 8, 2.0) > 1.5, 500.0, 0.0))
    c_ref = float(np.sum(c) / (n - 2) ** 2)
    b = R.random_rhs(n, n, 9)
    tol = 1e-10 * _l2(b, n)
    p = NL.Problem("linear", n, n, 1.0, a=a)
    want, winfo = NL.pcg_react(p, p.oracle(c_ref), b, c, tol=tol, max_iterations=60)
    s = _pcg(n, tol, a)
    t, cptr, ld = _device_field(c)
    assert lib.mg_pcg_set_reaction_device(s._engine._h, cptr, ld, c_ref) == _lib.MG_OK
    got, info = s.solve(s.grid, s.operator, b)
    s.close()
    print("iterations", info["iterations"], winfo["iterations"], "history", info["residual_history"], winfo["residual_history"])
    assert info["converged"] and winfo["converged"] and info["iterations"] == winfo["iterations"]
    # the tolerances of tests/test_gpu_pcg.py::test_solve_equals_restatement
    np.testing.assert_allclose(info["residual_history"], winfo["residual_history"], rtol=1e-10, atol=0)
    assert float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want)))
    np.testing.assert_allclose(info["initial_residual"], winfo["initial_residual"], rtol=1e-12)
    np.testing.assert_allclose(info["true_residual"], winfo["true_residual"], rtol=1e-6)


def test_pcg_clearing_the_field_restores_the_plain_loop_and_refusals():
    n = 33
    lib = _lib.load()
    b = R.random_rhs(n, n, 3)
    tol = 1e-10 * _l2(b, n)
    s, fresh = _pcg(n, tol), _pcg(n, tol)
    h = s._engine._h
    x0, i0 = fresh.solve(fresh.grid, mg.HelmholtzOperator(0.37), b)
    t, cptr, ld = _device_field(R.zero_ring(np.full((n, n), 25.0)))
    assert lib.mg_pcg_set_reaction_device(h, cptr, ld, 25.0) == _lib.MG_OK
    x1, i1 = s.solve(s.grid, mg.HelmholtzOperator(0.37), b)
    assert i1["converged"] and not _same_bits(x0, x1)
    assert lib.mg_pcg_set_reaction_device(h, None, 0, 0.0) == _lib.MG_OK
    x2, i2 = s.solve(s.grid, mg.HelmholtzOperator(0.37), b)
    assert _same_bits(x0, x2) and i0["residual_history"] == i2["residual_history"] and i0["true_residual"] == i2["true_residual"]
    assert i0["initial_residual"] == i2["initial_residual"]
    # refusals: c_ref, the pitch, order 4 either way round; the solver stays the plain one
    I, S = _lib.MG_ERR_INVALID_VALUE, _lib.MG_ERR_STATE
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.mg_pcg_set_reaction_device(h, cptr, ld, bad) == I and b"c_ref" in lib.mg_pcg_last_error(h)
    assert lib.mg_pcg_set_reaction_device(h, cptr, ld + 2, 1.0) == I and b"pitch" in lib.mg_pcg_last_error(h)
    x3, i3 = s.solve(s.grid, mg.HelmholtzOperator(0.37), b)
    assert _same_bits(x0, x3) and i0["residual_history"] == i3["residual_history"]
    s._engine.set_order(4)
    assert lib.mg_pcg_set_reaction_device(h, cptr, ld, 1.0) == S and b"fourth-order" in lib.mg_pcg_last_error(h)
    assert lib.mg_pcg_set_reaction_device(h, None, 0, 0.0) == _lib.MG_OK           # clearing is never refused
    s._engine.set_order(2)
    assert lib.mg_pcg_set_reaction_device(h, cptr, ld, 1.0) == _lib.MG_OK
    assert lib.mg_pcg_set_order(h, 4) == S and b"reaction" in lib.mg_pcg_last_error(h)
    with pytest.raises(ValueError, match="reaction"):
        s._engine.set_order(4)
    assert s._engine.order == 2
    s.close(); fresh.close()


# ------------------------------------------------------------------------------------------ 4. Newton solves
def _newton(n, kind, kappa, a=None, w=None, **kw):
    op = mg.LaplacianOperator(coefficient=-1.0) if a is None else mg.DiffusionOperator(a)
    s = mg.SemilinearSolver(nonlinearity=kind, strength=kappa, weight=w, max_levels=R.full_levels(n, n), **kw)
    s.setup(mg.Grid(n, n), op, smoother=_smoother())
    return s


def _histories_agree(got, want, f0, rtol=1e-5):
    """relative rtol at every step whose norm is above 1e-7 ||F_0||"""
    for k, (g, x) in enumerate(zip(got, want)):
        if x > 1e-7 * f0:
            assert abs(g - x) <= rtol * x, (k, g, x)


@pytest.mark.parametrize("n", [33, 65])
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_manufactured_problem(kind, n):
    """u* = 2 sin(pi x) sin(pi y), f := N_h(u*).  For monotone g, F(u) - F(u*) = (A + D)(u - u*) with D >= 0, so
    ||u - u*||_h <= ||F(u)||_h / lambda_min(A) up to ||F(u*)||_h, which is rounding (~1e-12 here, against a final residual that
    the inner tolerance floor 0.1 tol keeps near 1e-7 ... 1e-9: the slack between 19 and 19.7 covers it)."""
    p = NL.Problem(kind, n, n, 3.0)
    us = NL.manufactured(n, n)
    f = p.N(us)
    s = _newton(n, kind, 3.0, tolerance=1e-6)
    u, info = s.solve(f, initial_guess=np.zeros((n, n)))
    s.close()
    err, final = mg.Grid(n, n).l2_norm(u - us), info["true_residual"]
    print(kind, n, info["status"], "newton", info["newton_iterations"], "inner", info["inner_iterations"], "history", info["residual_history"],
          "eta", info["forcing_terms"], "steps", info["step_lengths"], "error", err, "||F|| / 19", final / LMIN, "||F(u*)||", p.norm(p.evaluate(us, f)["F"]))
    assert info["status"] == "converged" and info["converged"] and final < 1e-6
    assert final == (info["residual_history"][-1] if info["residual_history"] else info["initial_residual"])
    assert abs(p.norm(p.evaluate(u, f)["F"]) - final) <= 1e-6 * final + 1e-11      # the reported norm is the iterate's own
    assert err <= final / LMIN
    assert _ring(u).tobytes() == _ring(np.zeros((n, n))).tobytes()


@pytest.mark.parametrize("kind", KIND_NAMES)
def test_against_the_dense_exact_newton(kind):
    n = 33
    p = NL.Problem(kind, n, n, 3.0)
    f = p.N(NL.manufactured(n, n))
    u0 = np.zeros((n, n))
    want, winfo = NL.newton(p, f, u0, 1e-9, inner="dense")
    s = _newton(n, kind, 3.0, tolerance=1e-9, forcing="fixed", eta=1e-8)
    got, info = s.solve(f, initial_guess=u0)
    s.close()
    print(kind, "device", info["residual_history"], info["inner_iterations"], "dense", winfo["residual_history"])
    assert info["status"] == "converged" and winfo["converged"]
    np.testing.assert_allclose(info["initial_residual"], winfo["initial_residual"], rtol=1e-12)
    _histories_agree(info["residual_history"], winfo["residual_history"], winfo["initial_residual"])
    n_cmp = min(len(info["step_lengths"]), len(winfo["step_lengths"]))
    assert info["step_lengths"][:n_cmp] == winfo["step_lengths"][:n_cmp] and abs(info["newton_iterations"] - winfo["newton_iterations"]) <= 1
    assert info["forcing_terms"] == [1e-8] * info["newton_iterations"]


def test_line_search():
    """sinh from u0 = 0 with a right-hand side large enough that the exact Newton step overshoots"""
    n = 33
    p = NL.Problem("sinh", n, n, 1.0)
    f = p.N(4.0 * NL.manufactured(n, n))
    u0 = np.zeros((n, n))
    want, winfo = NL.newton(p, f, u0, 1e-8, inner="dense")
    assert winfo["converged"] and winfo["backtracks"] >= 1 and winfo["step_lengths"][0] < 1.0, winfo["step_lengths"]
    s = _newton(n, "sinh", 1.0, tolerance=1e-8, forcing="fixed", eta=1e-8)
    got, info = s.solve(f, initial_guess=u0)
    print("steps", info["step_lengths"], winfo["step_lengths"], "history", info["residual_history"], winfo["residual_history"],
          "evaluations", info["evaluations"], winfo["evaluations"])
    assert info["status"] == "converged" and info["step_lengths"] == winfo["step_lengths"]
    assert info["evaluations"] == 1 + sum(1 + int(round(-math.log2(t))) for t in info["step_lengths"])    # one launch per trial
    _histories_agree(info["residual_history"], winfo["residual_history"], winfo["initial_residual"])
    s.close()
    rng = np.random.default_rng(2)
    start = R.zero_ring(0.1 * rng.standard_normal((n, n)))
    s = _newton(n, "sinh", 1.0, tolerance=1e-8, forcing="fixed", eta=1e-8, max_backtracks=0)
    got, info = s.solve(f, initial_guess=start)
    s.close()
    assert info["status"] == "line_search_failed" and not info["converged"] and info["newton_iterations"] == 0
    assert got.tobytes() == start.tobytes() and info["true_residual"] == info["initial_residual"]


_PB = {}


def _poisson_boltzmann(n, precision):
    """a = 1 inside a disc and 80 outside, w = 0 inside and 1 outside, a charge inside the disc near its surface.  The forcing
    term is fixed at 1e-10: the inner solve leaves a linear residual of up to eta ||F_k|| in F_(k+1), which two preconditioner
    precisions leave differently, and ||F_k|| / ||F_(k+1)|| reaches 3e3 on the quadratic tail of this problem -- eta = 1e-10
    keeps that share of the compared norms below 1e-6, under the 1e-5 they must agree to."""
    if (n, precision) not in _PB:
        a, w = NL.disc(n, n)
        X, Y = NL.mesh(n, n)
        f = 1e5 * np.exp(-((X - 0.5) ** 2 + (Y - 0.25) ** 2) / 0.004)
        s = _newton(n, "sinh", 100.0, a=a, w=w, tolerance=1e-8, precision=precision, forcing="fixed", eta=1e-10)
        u, info = s.solve(f, initial_guess=np.zeros((n, n)))
        s.close()
        print("Poisson-Boltzmann", n, precision, info["status"], "history", info["residual_history"], "inner", info["inner_iterations"],
              "steps", info["step_lengths"])
        _PB[(n, precision)] = (NL.Problem("sinh", n, n, 100.0, a=a, w=w), f, u, info)
    return _PB[(n, precision)]


@pytest.mark.parametrize("n", [33, 65])
def test_poisson_boltzmann_shape(n):
    p, f, ud, di = _poisson_boltzmann(n, "double")
    _, _, us, si = _poisson_boltzmann(n, "single_managed")
    assert di["status"] == "converged" and si["status"] == "converged"
    assert di["newton_iterations"] == si["newton_iterations"] and di["step_lengths"] == si["step_lengths"]
    _histories_agree(si["residual_history"], di["residual_history"], di["initial_residual"])
    if n == 33:
        # the dense reference stops at 1e-10: F cannot be evaluated below ~2e-11 on this problem (a = 80, u ~ 150), and its own
        # residual (3.7e-11, a tenth of the device's final one) sits inside the gap between lambda_min(A_h) and lambda_min(J)
        want, winfo = NL.newton(p, f, np.zeros((n, n)), 1e-10, inner="dense")
        lmin = float(np.linalg.eigvalsh(NL.jacobian_dense(p, np.zeros((n, n))))[0])
        assert winfo["converged"]
        _histories_agree(di["residual_history"], winfo["residual_history"], winfo["initial_residual"])
        for u, info in ((ud, di), (us, si)):
            err = mg.Grid(n, n).l2_norm(u - want)
            print("error", err, "||F_final|| / lambda_min", info["true_residual"] / lmin, "lambda_min", lmin)
            assert err <= info["true_residual"] / lmin


def test_linear_kind_is_one_step_and_equals_pcg():
    n, kappa = 65, 40.0
    b = R.random_rhs(n, n, 5)
    f0 = _l2(b, n)
    s = _newton(n, "linear", kappa, tolerance=1e-7 * f0, forcing="fixed", eta=1e-8)
    u, info = s.solve(b)
    s.close()
    pc = _pcg(n, 1e-8 * f0)
    x, pinfo = pc.solve(pc.grid, mg.HelmholtzOperator(kappa), b)
    pc.close()
    err = _l2(u - x, n)
    print("newton", info["newton_iterations"], info["inner_iterations"], info["residual_history"], "pcg", pinfo["iterations"], "diff", err)
    assert info["status"] == "converged" and info["newton_iterations"] == 1 and info["step_lengths"] == [1.0]
    assert pinfo["converged"] and abs(info["inner_iterations"][0] - pinfo["iterations"]) <= 1
    # both residuals are below 1e-7 ||b||: the two solutions differ by at most their sum over lambda_min(A + kappa)
    assert err <= (info["true_residual"] + pinfo["true_residual"]) / (LMIN + kappa)
    np.testing.assert_allclose(info["initial_residual"], f0, rtol=1e-12)


def test_float32_host_arrays_give_the_bits_of_their_float64_values():
    """set_coefficient, set_nonlinearity and solve with float32 host arrays (staged in fp32, cast to fp64 on the device) against
    the same calls with the same values as float64: the cast is exact, so the Newton method runs on the same bits (the fp32 solve
    returns them rounded to fp32 once)."""
    from mixed_precision_multigrid_solvers_for_pdes_amd.nonlinear import SemilinearEngine
    nx, ny = 9, 17
    rng = np.random.default_rng(3)
    f = rng.standard_normal((nx, ny)).astype(np.float32)
    u0 = (0.1 * rng.standard_normal((nx, ny))).astype(np.float32)
    a, w = ((1.0 + rng.random((nx, ny))).astype(np.float32) for _ in range(2))
    out = []
    for dt in (np.float32, np.float64):
        with SemilinearEngine(nx, ny, max_levels=3) as e:
            e.set_coefficient(a.astype(dt))
            e.set_nonlinearity("cubic", 2.0, w.astype(dt))
            out.append(e.solve(f.astype(dt), u0.astype(dt), tol=1e-9))
    (u32, i32), (u64, i64) = out
    assert u32.dtype == np.float32 and np.isfinite(u32).all() and i64["converged"]
    assert u32.tobytes() == u64.astype(np.float32).tobytes()
    for key in ("newton_iterations", "inner_iterations", "residual_history", "step_lengths", "initial_residual", "true_residual"):
        assert i32[key] == i64[key], key


def test_statuses_limits_and_abi_refusals():
    n = 33
    lib = _lib.load()
    p = NL.Problem("exp", n, n, 3.0)
    f = p.N(NL.manufactured(n, n))
    s = _newton(n, "exp", 3.0, tolerance=1e-8)
    u1, i1 = s.solve(f)
    for key in ("newton_iterations", "inner_iterations", "residual_history", "step_lengths", "forcing_terms", "status", "true_residual"):
        assert key in i1, key
    assert i1["status"] == "converged" and i1["newton_iterations"] == len(i1["residual_history"]) == len(i1["inner_iterations"])
    assert i1["total_inner_iterations"] == sum(i1["inner_iterations"]) and i1["forcing_terms"][0] == 0.1
    u2, i2 = s.solve(f)                                                            # the same object again: the same bits
    assert u1.tobytes() == u2.tobytes() and i1["residual_history"] == i2["residual_history"]
    assert i1["inner_iterations"] == i2["inner_iterations"] and i1["step_lengths"] == i2["step_lengths"]
    h = s._engine._h
    I = _lib.MG_ERR_INVALID_VALUE
    assert lib.mg_nl_set_nonlinearity(h, 4, 1.0, None, _lib.MG_F64) == I and b"nonlinearity" in lib.mg_nl_last_error(h)
    assert lib.mg_nl_set_nonlinearity(h, 3, -1.0, None, _lib.MG_F64) == I and b"kappa" in lib.mg_nl_last_error(h)
    w = np.ones((n, n)); w[5, 6] = -1e-3
    assert lib.mg_nl_set_nonlinearity(h, 3, 3.0, _lib.ptr(w), _lib.MG_F64) == I and b"weight" in lib.mg_nl_last_error(h)
    with pytest.raises(ValueError, match="weight"):
        s._engine.set_nonlinearity("exp", 3.0, w)
    u3, i3 = s.solve(f)                                                            # a refused call leaves the solver as it was
    assert u1.tobytes() == u3.tobytes()
    s.close()
    s = _newton(n, "exp", 3.0, tolerance=1e-8, max_newton=1)
    u, info = s.solve(f)
    s.close()
    assert info["status"] == "max_newton" and not info["converged"] and info["newton_iterations"] == 1
    np.testing.assert_allclose(info["residual_history"][0], i1["residual_history"][0], rtol=0, atol=0)
