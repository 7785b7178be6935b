"""The fourth-order compact nine-point scheme (include/mghip_ho.h, csrc/mg_ho.hip) on a GPU: its three kernels call by call,
bit for bit against the NumPy restatement tests/ho_reference.py (pinned on the CPU by tests/test_ho_cpu.py); whole solves of
the manufactured problem through PCGSolver(order=4) -- fourth-order error, iteration counts against the order-2 loop, the
restatement's loop, fp32 preconditioners; order 2 left bit for bit as it was; and the refusals.

Kernel shapes: 34 x 67 and 70 x 131 are the smallest with a second tile row (32 rows), a second tile column (64 columns), a
partial last tile and an odd ny whose last 16-byte vector is half pad; every field has the library's pitch + 8.

Solves stop at 1e-12 ||f||_h.  Under order 4 the norm runs over interior cells only (the ring of f is data of the scheme);
the order-2 runs they are compared with get the same f with a zeroed ring -- order 2 never reads the ring of f except as a
floor under its norm -- so both loops stop on the same quantity."""
import ctypes as C
import math

import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib

import ho_reference as H
import pcg_reference as R

pytestmark = pytest.mark.gpu

GUARD = 2
SENTINEL = -7.25e300          # what outputs, pad columns and guard rows hold before a call
KERNEL_SHAPES = [(5, 5), (9, 17), (33, 33), (34, 67), (70, 131)]
OPERATORS = [(0.0, -1.0), (37.5, -2.5), (37.5, -1.0), (0.0, -2.5)]


def _torch():
    import torch
    return torch


def _pitch(ny):
    ld = C.c_int(0)
    _lib.check(_lib.load().mg_pitch_elems(_lib.MG_F64, ny, C.byref(ld)))
    return ld.value + 8


class Field:
    """an (nx, ny) fp64 device field with pitch ld between guard rows; guards and pad columns hold SENTINEL"""

    def __init__(self, arr, ld, fill=None):
        nx, ny = arr.shape
        host = np.full((nx + 2 * GUARD, ld), SENTINEL)
        host[GUARD:GUARD + nx, :ny] = arr if fill is None else fill
        self.nx, self.ny, self.ld = nx, ny, ld
        self.t = _torch().from_numpy(host).cuda()
        self.start = host.copy()
        self.ptr = C.c_void_p(self.t[GUARD:].data_ptr())

    def numpy(self):
        return self.t.cpu().numpy()

    def field(self):
        return self.numpy()[GUARD:GUARD + self.nx, :self.ny]

    def outside_untouched(self, whole=False):
        """guards and pad columns (whole: every cell) still hold the bits they started with"""
        now, start = self.numpy().view(np.uint64), self.start.view(np.uint64)
        mask = np.ones(now.shape, dtype=bool)
        if not whole:
            mask[GUARD:GUARD + self.nx, :self.ny] = False
        return bool(np.all(now[mask] == start[mask]))


def _scalar(value=np.nan):
    return _torch().tensor([value], dtype=_torch().float64, device="cuda")


def _scratch(nx, ny):
    n = C.c_int64(0)
    _lib.check(_lib.load().mg_dev_scratch_bytes(nx, ny, C.byref(n)))
    return _torch().full((n.value // 8,), float("nan"), dtype=_torch().float64, device="cuda")


def _p(t):
    return C.c_void_p(t.data_ptr())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a) + 0.0, np.ascontiguousarray(b) + 0.0          # -0 -> +0: the sign of a zero is not pinned
    return bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


def _ring(a):
    mask = np.ones(a.shape, dtype=bool)
    mask[1:-1, 1:-1] = False
    return a[mask]


def _spacings(nx, ny):
    return 1.0 / (nx - 1), 0.75 / (ny - 1)


# ------------------------------------------------------------------------------------------ 1. kernels, call by call
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d" % s for s in KERNEL_SHAPES])
def test_direction_kernel(shape):
    nx, ny = shape
    lib, ld = _lib.load(), _pitch(ny)
    hx, hy = _spacings(nx, ny)
    rng = np.random.default_rng(nx * 7 + ny)
    z, p = rng.standard_normal((nx, ny)), rng.standard_normal((nx, ny))          # their rings are not read
    for sigma, coeff in OPERATORS:
        for beta in (None, -0.625):
            want_p = R.zero_ring(z) if beta is None else R.zero_ring(z + beta * p)
            want_q = H.apply_A4(want_p, hx, hy, coeff, sigma)
            fz, fp = Field(z, ld), Field(p, ld, fill=np.nan if beta is None else None)
            fpo, fq = Field(z, ld, fill=SENTINEL), Field(z, ld, fill=SENTINEL)
            pq, scratch = _scalar(), _scratch(nx, ny)
            bdev = None if beta is None else _scalar(beta)
            _lib.check(lib.mg_dev_ho_direction(nx, ny, ld, hx, hy, coeff, sigma, fz.ptr, fp.ptr, fpo.ptr, fq.ptr,
                                               None if bdev is None else _p(bdev), _p(scratch), _p(pq), None))
            _torch().cuda.synchronize()
            what = "%dx%d sigma %g coeff %g beta %r" % (nx, ny, sigma, coeff, beta)
            assert fz.outside_untouched(whole=True) and fp.outside_untouched(whole=True), "an input was written: " + what
            assert fpo.outside_untouched() and fq.outside_untouched(), "stored outside [0, nx) x [0, ny): " + what
            got_p, got_q = fpo.field(), fq.field()
            assert _same_bits(got_p, want_p), "p: " + what
            assert _same_bits(got_q, want_q), "q: " + what
            assert not _ring(got_p).any() and not _ring(got_q).any(), "ring: " + what
            ref = math.fsum((want_p * want_q).ravel().tolist())
            got = float(pq.cpu()[0])
            print(what, "p.q", got, ref)
            assert abs(got - ref) <= 1e-13 * abs(ref), "p.q: %s: %r vs %r" % (what, got, ref)


@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d" % s for s in KERNEL_SHAPES])
def test_rhs_and_residual_kernels(shape):
    nx, ny = shape
    lib, ld = _lib.load(), _pitch(ny)
    hx, hy = _spacings(nx, ny)
    rng = np.random.default_rng(nx * 11 + ny)
    f, x = rng.standard_normal((nx, ny)), rng.standard_normal((nx, ny))          # x: a non-zero ring, corners included
    ff, fg = Field(f, ld), Field(f, ld, fill=SENTINEL)
    _lib.check(lib.mg_dev_ho_rhs(nx, ny, ld, ff.ptr, fg.ptr, None))
    _torch().cuda.synchronize()
    g = fg.field().copy()
    assert ff.outside_untouched(whole=True) and fg.outside_untouched()
    assert _same_bits(g, H.rhs_average(f))
    assert _ring(g).tobytes() == _ring(f).tobytes()
    for sigma, coeff in OPERATORS:
        want = H.residual(x, g, hx, hy, coeff, sigma)
        fx, fgg, fr = Field(x, ld), Field(g, ld), Field(x, ld, fill=SENTINEL)
        rr, scratch = _scalar(), _scratch(nx, ny)
        _lib.check(lib.mg_dev_ho_residual(nx, ny, ld, hx, hy, coeff, sigma, fx.ptr, fgg.ptr, fr.ptr, _p(scratch), _p(rr), None))
        _torch().cuda.synchronize()
        what = "%dx%d sigma %g coeff %g" % (nx, ny, sigma, coeff)
        assert fx.outside_untouched(whole=True) and fgg.outside_untouched(whole=True) and fr.outside_untouched(), what
        got = fr.field()
        assert _same_bits(got, want), "r: " + what
        assert not _ring(got).any()
        ref = math.fsum((want * want).ravel().tolist())
        assert abs(float(rr.cpu()[0]) - ref) <= 1e-13 * ref, "sum r^2: %s: %r vs %r" % (what, float(rr.cpu()[0]), ref)
        # the corners of x are read: another corner value changes the cells next to it and no others
        x2 = x.copy(); x2[0, 0] += 1.0
        assert H.residual(x2, g, hx, hy, coeff, sigma)[1, 1] != want[1, 1]
    # the host-array forms are the same kernels
    out = np.full((nx, ny), SENTINEL)
    _lib.check(lib.mg_op_rhs_ho(nx, ny, _lib.ptr(f), _lib.ptr(out)))
    assert _same_bits(out, H.rhs_average(f))
    _lib.check(lib.mg_op_apply_ho(nx, ny, hx, hy, -2.5, 37.5, _lib.ptr(x), _lib.ptr(out)))
    assert _same_bits(out, H.apply_A4(x, hx, hy, -2.5, 37.5))


# ------------------------------------------------------------------------------------------ 2. whole solves
def _smoother(name):
    return mg.JacobiSmoother(relaxation_parameter=0.8) if name == "jacobi" else mg.GaussSeidelSmoother(red_black=True, relaxation_parameter=1.0)


def _operator(sigma):
    return mg.HelmholtzOperator(sigma) if sigma else mg.LaplacianOperator(coefficient=-1.0)


def _problem(nx, ny, sigma):
    u, f = H.manufactured(nx, ny, sigma)
    u0 = u.copy()
    u0[1:-1, 1:-1] = 0.0
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    tol = 1e-12 * float(np.sqrt(hx * hy * np.sum(f * f)))
    return u, f, u0, tol


def _make(nx, ny, sigma, smoother, precision, order):
    _, _, _, tol = _problem(nx, ny, sigma)
    s = mg.PCGSolver(max_levels=R.full_levels(nx, ny), max_iterations=60, tolerance=tol, cycle_type="V", pre_smooth_iterations=2,
                     post_smooth_iterations=2, precision=precision, order=order)
    s.setup(mg.Grid(nx, ny), _operator(sigma), smoother=_smoother(smoother))
    return s


_DEVICE, _REFERENCE = {}, {}


def _device(nx, ny, sigma=0.0, smoother="jacobi", precision="double", order=4):
    """(x, info, max error) of one device solve of the manufactured problem, computed once per case"""
    key = (nx, ny, sigma, smoother, precision, order)
    if key not in _DEVICE:
        u, f, u0, _ = _problem(nx, ny, sigma)
        s = _make(*key)
        x, info = s.solve(s.grid, s.operator, f if order == 4 else R.zero_ring(f), initial_guess=u0)
        s.close()
        _DEVICE[key] = (x, info, float(np.max(np.abs(x - u))))
        print("device", key, "iterations", info["iterations"], info["status"], "error", _DEVICE[key][2], "true residual / tol",
              info["true_residual"] / s.tolerance)
    return _DEVICE[key]


def _reference(nx, ny, sigma=0.0, smoother="jacobi", precision="double"):
    """the restatement's order-4 loop on the same problem, computed once per case"""
    key = (nx, ny, sigma, smoother, precision)
    if key not in _REFERENCE:
        u, f, u0, tol = _problem(nx, ny, sigma)
        mgo = R.make_oracle(nx, ny, None, 2, 2, "jacobi" if smoother == "jacobi" else "rbgs", 0.8 if smoother == "jacobi" else 1.0, shift=sigma)
        x, info = H.pcg(mgo, f, u0=u0, tol=tol, max_iterations=60, flexible=R.default_flexible(smoother, 2, 2),
                        pm=R.precision_manager(precision))
        _REFERENCE[key] = (x, info, float(np.max(np.abs(x - u))))
    return _REFERENCE[key]


CASES = [(33, 33, 0.0, "jacobi", "double"), (65, 65, 0.0, "jacobi", "double"), (129, 129, 0.0, "jacobi", "double"),
         (33, 65, 0.0, "jacobi", "double"), (65, 65, 500.0, "jacobi", "double"), (65, 65, 0.0, "rbgs", "double"),
         (33, 33, 0.0, "jacobi", "single_managed"), (65, 65, 0.0, "jacobi", "single_managed"),
         (129, 129, 0.0, "jacobi", "single_managed"), (33, 65, 0.0, "jacobi", "single_managed")]


@pytest.mark.parametrize("case", CASES, ids=["%dx%d_s%g_%s_%s" % c for c in CASES])
def test_solve_of_the_manufactured_problem(case):
    nx, ny, sigma, smoother, precision = case
    u, f, u0, tol = _problem(nx, ny, sigma)
    got, info, err = _device(nx, ny, sigma, smoother, precision)
    want, winfo, werr = _reference(nx, ny, sigma, smoother, precision)
    print(case, "iterations", info["iterations"], winfo["iterations"], "error", err, werr, "max |x - restatement|",
          float(np.max(np.abs(got - want))))
    print("history", info["residual_history"], winfo["residual_history"])
    assert info["status"] == "converged" and info["converged"] and info["order"] == 4
    assert info["flexible"] == R.default_flexible(smoother, 2, 2)
    assert _ring(got).tobytes() == _ring(u0).tobytes()                 # the Dirichlet data, bit for bit
    assert winfo["converged"]
    if precision == "double":           # the tolerances of tests/test_gpu_pcg.py::test_solve_equals_restatement
        assert info["iterations"] == winfo["iterations"]
        np.testing.assert_allclose(info["residual_history"], winfo["residual_history"], rtol=1e-10, atol=0)
        assert float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want)))
        np.testing.assert_allclose(info["initial_residual"], winfo["initial_residual"], rtol=1e-12)
    else:                               # ... and of test_fp32_preconditioner
        assert info["final_residual"] < tol
        assert info["iterations"] <= winfo["iterations"] + 2
        assert err <= 10 * werr


def test_error_is_fourth_order_and_iterations_stay_within_twice_order_2():
    errs = [_device(n, n)[2] for n in (33, 65, 129)]
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("order-4 errors", errs, "ratios", ratios)
    assert all(r >= 14.0 for r in ratios), (errs, ratios)
    e2 = _device(129, 129, order=2)[2]
    print("order-2 error at 129^2", e2, "order-4 error at 65^2", errs[1])
    assert _device(129, 129, order=2)[1]["converged"]
    assert errs[1] * 100.0 < e2
    for nx, ny, sigma, smoother, precision in CASES:
        i4 = _device(nx, ny, sigma, smoother, precision)[1]
        i2 = _device(nx, ny, sigma, smoother, precision, order=2)[1]
        print((nx, ny, sigma, smoother, precision), "iterations order 4 / order 2", i4["iterations"], i2["iterations"])
        assert i2["converged"] and i2["order"] == 2 and i4["iterations"] <= 2 * i2["iterations"]
    e_double, e_single = _device(129, 129)[2], _device(129, 129, precision="single_managed")[2]
    print("129^2 error, double / single_managed preconditioner", e_double, e_single)
    assert abs(e_single - e_double) <= 0.05 * e_double


def test_solve_device_equals_the_host_solve():
    torch = _torch()
    nx, ny = 33, 65
    u, f, u0, tol = _problem(nx, ny, 0.0)
    got, info, _ = _device(nx, ny)
    s = _make(nx, ny, 0.0, "jacobi", "double", 4)
    ld = ny + 5                                                       # a caller's pitch, not the library's
    rhs_t = torch.full((nx, ld), float("nan"), dtype=torch.float64, device="cuda")
    x_t = rhs_t.clone()
    rhs_t[:, :ny] = torch.from_numpy(f).cuda()
    x_t[:, :ny] = torch.from_numpy(u0).cuda()
    dinfo = s._engine.solve_device(rhs_t, x_t, tol, 60)
    torch.cuda.synchronize()
    s.close()
    assert dinfo["status"] == "converged" and dinfo["order"] == 4
    assert _same_bits(x_t[:, :ny].cpu().numpy(), got)
    assert bool(torch.isnan(x_t[:, ny:]).all()) and bool(torch.isnan(rhs_t[:, ny:]).all())
    assert dinfo["residual_history"] == info["residual_history"] and dinfo["iterations"] == info["iterations"]


# ------------------------------------------------------------------------------------------ 3. order 2 is untouched
def test_order_2_is_bit_identical_and_switching_reproduces_order_4():
    n = 33
    b = R.random_rhs(n, n, 3)
    u, f, u0, _ = _problem(n, n, 0.0)
    tol = 1e-10 * float(np.sqrt(np.sum(b * b)) / (n - 1))

    def make():
        s = mg.PCGSolver(max_levels=R.full_levels(n, n), max_iterations=40, tolerance=tol, pre_smooth_iterations=2, post_smooth_iterations=2)
        s.setup(mg.Grid(n, n), mg.LaplacianOperator(coefficient=-1.0), smoother=_smoother("jacobi"))
        return s

    never, explicit, switched = make(), make(), make()
    x0, i0 = never.solve(never.grid, never.operator, b)
    explicit._engine.set_order(2)
    x1, i1 = explicit.solve(explicit.grid, explicit.operator, b)
    assert i0["converged"] and i0["order"] == 2 and _same_bits(x0, x1) and i0["residual_history"] == i1["residual_history"]
    assert i0["true_residual"] == i1["true_residual"] and i0["initial_residual"] == i1["initial_residual"]
    switched._engine.set_order(4)
    xa, ia = switched.solve(switched.grid, switched.operator, f, initial_guess=u0)
    switched._engine.set_order(2)
    x2, i2 = switched.solve(switched.grid, switched.operator, b)
    assert i2["order"] == 2 and _same_bits(x0, x2) and i0["residual_history"] == i2["residual_history"]
    assert i0["true_residual"] == i2["true_residual"]
    switched._engine.set_order(4)
    xb, ib = switched.solve(switched.grid, switched.operator, f, initial_guess=u0)
    assert ia["order"] == ib["order"] == 4 and ia["iterations"] > 0
    assert _same_bits(xa, xb) and ia["residual_history"] == ib["residual_history"] and ia["true_residual"] == ib["true_residual"]
    for s in (never, explicit, switched):
        s.close()


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_handle_usable():
    n = 33
    lib = _lib.load()
    u, f, u0, tol = _problem(n, n, 0.0)
    a = R.smooth_coefficient(n, n)
    b = R.random_rhs(n, n, 1)
    s = _make(n, n, 0.0, "jacobi", "double", 4)
    first, info = s.solve(s.grid, s.operator, f, initial_guess=u0)
    h = s._engine._h
    # order 3
    assert lib.mg_pcg_set_order(h, 3) == _lib.MG_ERR_INVALID_VALUE and b"order" in lib.mg_pcg_last_error(h)
    with pytest.raises(ValueError, match="order"):
        s._engine.set_order(3)
    # set_coefficient(a) under order 4
    assert lib.mg_pcg_set_coefficient(h, _lib.ptr(a), _lib.MG_F64) == _lib.MG_ERR_STATE
    with pytest.raises(ValueError, match="constant coefficients"):
        s._engine.set_coefficient(a)
    s._engine.set_coefficient(None)                                   # clearing a coefficient is not refused
    again, ainfo = s.solve(s.grid, s.operator, f, initial_guess=u0)
    assert s._engine.order == 4 and ainfo["order"] == 4
    assert _same_bits(first, again) and info["residual_history"] == ainfo["residual_history"]
    s.close()
    # order 4 after set_coefficient(a): the solver stays the variable-coefficient order-2 solver it was
    v = mg.PCGSolver(max_levels=R.full_levels(n, n), max_iterations=60, tolerance=1e-8, pre_smooth_iterations=2, post_smooth_iterations=2)
    v.setup(mg.Grid(n, n), mg.DiffusionOperator(a), smoother=_smoother("jacobi"))
    before, binfo = v.solve(v.grid, v.operator, b)
    assert lib.mg_pcg_set_order(v._engine._h, 4) == _lib.MG_ERR_STATE
    with pytest.raises(ValueError, match="constant coefficients"):
        v._engine.set_order(4)
    after, cinfo = v.solve(v.grid, v.operator, b)
    assert v._engine.order == 2 and cinfo["order"] == 2 and binfo["converged"]
    assert _same_bits(before, after) and binfo["residual_history"] == cinfo["residual_history"]
    v.close()
    # PCGSolver(order=4) with a DiffusionOperator
    w = mg.PCGSolver(order=4)
    with pytest.raises(NotImplementedError, match="constant coefficients"):
        w.setup(mg.Grid(n, n), mg.DiffusionOperator(a))
    assert w._engine is None
