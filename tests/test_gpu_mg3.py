"""The GPU half of the 3-D multigrid family's tests (tests/test_mg3_cpu.py is the CPU half): every mg3_dev_* kernel call by call
against the NumPy restatement tests/mg3_reference.py, bit for bit in fp64 and fp32, on guarded arrays (NaN planes below and above,
NaN pad columns, the engine's pitch and the smallest even one) at the shapes where the tiling can go wrong; then the engine's
cycles, solves, precisions and entry points against the restatement's."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _build, _lib
from mixed_precision_multigrid_solvers_for_pdes_amd.engine3d import check3

import mg3_reference as R

pytestmark = pytest.mark.gpu

_text = open(os.path.join(_build.CSRC, "mg_3d_kernels.hpp")).read()
T3J = int(re.search(r"constexpr int kT3J = (\d+);", _text).group(1))
T3ROW = int(re.search(r"constexpr int kT3RowBytes = (\d+);", _text).group(1))
T3I = int(re.search(r"constexpr int kT3I = (\d+);", _text).group(1))
LDS_EXTENT = int(re.search(r"constexpr int kCoarseLdsExtent = (\d+);", _text).group(1))
DTYPES = [np.float64, np.float32]
EQUAL_DOMAIN = (0.0, 0.25, 0.0, 0.5, 0.0, 1.0)          # 9 x 17 x 33 with equal spacings


def edge(e):
    return [e - 1, e, e + 1, e + 2, 2 * e - 1, 2 * e, 2 * e + 1, 2 * e + 2]


def shapes_for(dtype):
    tk = T3ROW // np.dtype(dtype).itemsize
    out = [(3, 3, 3), (3, 3, 9), (5, 5, 5), (5, 9, 17), (6, 7, 10)]
    out += [(n + 2, 5, 6) for n in edge(T3I)] + [(n, 5, 6) for n in (T3I - 1, T3I, 2 * T3I)]      # interior planes and planes
    out += [(5, n, 6) for n in edge(T3J)] + [(4, n + 2, 5) for n in (T3J - 1, T3J, 2 * T3J)]
    out += [(5, 4, n) for n in edge(tk)] + [(4, 5, n + 2) for n in (tk - 1, tk, 2 * tk)]
    return out


CASES = [(s, dt) for dt in DTYPES for s in shapes_for(dt)]
CASE_IDS = ["%dx%dx%d-%s" % (s + (np.dtype(dt).name,)) for s, dt in CASES]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def pitches(dtype, nz):
    ld = C.c_int(0)
    _lib.check(_lib.load().mg_pitch_elems(_lib.dtype_code(dtype), nz, C.byref(ld)))
    return [ld.value, nz + (nz & 1)]


class Guarded:
    """a device field (nx, ny, ld) between NaN guard planes, pads NaN; `a` (nx, ny, nz) fills the cells"""

    def __init__(self, torch, a, ld):
        self.torch, self.shape, self.ld = torch, a.shape, ld
        nx, ny, nz = a.shape
        es = a.dtype.itemsize
        self.g = 1 if (ny * ld * es) % 16 == 0 else 2                      # guard planes: the field's base stays 16-byte aligned
        host = np.full((nx + 2 * self.g, ny, ld), np.nan, dtype=a.dtype)
        host[self.g:self.g + nx, :, :nz] = a
        self.before = host.copy()
        self.full = torch.from_numpy(host).to("cuda")
        self.ptr = C.c_void_p(self.full[self.g:].data_ptr())
        assert self.ptr.value % 16 == 0

    def host(self):
        return self.full.cpu().numpy()

    def cells(self):
        nx, ny, nz = self.shape
        return self.host()[self.g:self.g + nx, :, :nz]

    def outside_untouched(self):
        """guard planes and pad columns hold the NaNs they were given, bit for bit"""
        nx, ny, nz = self.shape
        now, was = self.host().copy(), self.before.copy()
        now[self.g:self.g + nx, :, :nz] = 0
        was[self.g:self.g + nx, :, :nz] = 0
        return now.tobytes() == was.tobytes()

    def unwritten(self):
        return self.host().tobytes() == self.before.tobytes()


def scratch_for(torch, lib, shape):
    n = C.c_int64(0)
    check3(lib.mg3_dev_scratch_bytes(*shape, C.byref(n)))
    t = torch.zeros(n.value // 8 + 2, dtype=torch.float64, device="cuda")
    return t, C.c_void_p(t.data_ptr()), C.c_void_p(t[-1:].data_ptr())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def faces_equal(a, b):
    m = np.ones(a.shape, dtype=bool)
    m[1:-1, 1:-1, 1:-1] = False
    return a[m].tobytes() == b[m].tobytes()


def fields(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape).astype(dtype), rng.standard_normal(shape).astype(dtype)


# ------------------------------------------------------------------------------------------ kernels, call by call
@pytest.mark.parametrize("shape,dtype", CASES, ids=CASE_IDS)
def test_sweep_kernels_bit_for_bit(torch, lib, shape, dtype):
    """Jacobi, both colours with both offsets, and the residual with its sum: the same bits as the restatement; inputs unwritten,
    nothing stored outside the field, boundary faces untouched"""
    u, f = fields(shape, dtype, 11)
    h, sigma, omega = (0.11, 0.13, 0.09), 0.7, 0.8
    code = _lib.dtype_code(dtype)
    for ld in pitches(dtype, shape[2]):
        du, df = Guarded(torch, u, ld), Guarded(torch, f, ld)
        # Jacobi (out of place; `out` starts as another field, whose faces must survive)
        other = fields(shape, dtype, 12)[0]
        dout = Guarded(torch, other, ld)
        check3(lib.mg3_dev_jacobi(code, *shape, ld, *h, sigma, omega, du.ptr, df.ptr, dout.ptr, None))
        torch.cuda.synchronize()
        got, want = dout.cells(), R.jacobi(u, f, h, sigma, omega)
        assert same_bits(got[R.INT], want[R.INT]), "jacobi"
        assert faces_equal(got, other) and dout.outside_untouched() and du.unwritten() and df.unwritten()
        # the residual and its sum, twice
        dr = Guarded(torch, other, ld)
        st, sp, ss = scratch_for(torch, lib, shape)
        sums = []
        for _ in range(2):
            check3(lib.mg3_dev_residual(code, code, *shape, ld, ld, *h, sigma, du.ptr, df.ptr, dr.ptr, sp, ss, None))
            torch.cuda.synchronize()
            sums.append(float(st[-1].item()))
        want = R.residual(u, f, h, sigma)
        assert same_bits(dr.cells()[R.INT], want[R.INT]), "residual"
        assert faces_equal(dr.cells(), other) and dr.outside_untouched() and du.unwritten() and df.unwritten()
        exact = R.sumsq(want[R.INT])
        print(shape, np.dtype(dtype).name, ld, "sum", sums[0], "fsum", exact)
        assert sums[0] == sums[1] and abs(sums[0] - exact) <= 1e-13 * exact
        check3(lib.mg3_dev_residual(code, code, *shape, ld, ld, *h, sigma, du.ptr, df.ptr, None, sp, ss, None))     # the sum alone
        torch.cuda.synchronize()
        assert float(st[-1].item()) == sums[0]
        # the colour passes
        for offset in (0, 1):
            for colour in (0, 1):
                dv = Guarded(torch, u, ld)
                check3(lib.mg3_dev_rbgs_colour(code, *shape, ld, *h, sigma, omega, colour, offset, dv.ptr, df.ptr, None))
                torch.cuda.synchronize()
                want = R.colour_pass(u, f, h, sigma, omega, colour, offset)
                assert same_bits(dv.cells(), want), ("colour", colour, offset)
                assert dv.outside_untouched() and df.unwritten()


@pytest.mark.parametrize("shape", [(5, 5, 5), (5, 9, 17), (6, 7, 10), (T3I + 3, 5, 6), (5, T3J + 1, 6), (5, 4, T3ROW // 8 + 1)],
                         ids=lambda s: "%dx%dx%d" % s)
def test_residual_fp32_from_fp64_and_upcast_add(torch, lib, shape):
    """the two mixed-type kernels of the defect step"""
    u, f = fields(shape, np.float64, 21)
    h, sigma = (0.11, 0.13, 0.09), 0.3
    for ld64, ld32 in zip(pitches(np.float64, shape[2]), pitches(np.float32, shape[2])):
        du, df = Guarded(torch, u, ld64), Guarded(torch, f, ld64)
        junk = fields(shape, np.float32, 22)[0]
        dr = Guarded(torch, junk, ld32)
        st, sp, ss = scratch_for(torch, lib, shape)
        check3(lib.mg3_dev_residual(_lib.MG_F64, _lib.MG_F32, *shape, ld64, ld32, *h, sigma, du.ptr, df.ptr, dr.ptr, sp, ss, None))
        torch.cuda.synchronize()
        want = R.residual(u, f, h, sigma)
        assert same_bits(dr.cells()[R.INT], want.astype(np.float32)[R.INT])
        assert faces_equal(dr.cells(), junk) and dr.outside_untouched() and du.unwritten() and df.unwritten()
        exact = R.sumsq(want[R.INT])
        assert abs(float(st[-1].item()) - exact) <= 1e-13 * exact               # the sum is of the unrounded residual
        e = fields(shape, np.float32, 23)[0]
        de, dv = Guarded(torch, e, ld32), Guarded(torch, u, ld64)
        check3(lib.mg3_dev_upcast_add(*shape, ld64, ld32, de.ptr, dv.ptr, None))
        torch.cuda.synchronize()
        want = u.copy()
        want[R.INT] = u[R.INT] + e[R.INT].astype(np.float64)
        assert same_bits(dv.cells(), want) and dv.outside_untouched() and de.unwritten()


TRANSFER_SHAPES = [(5, 5, 5), (5, 9, 17), (7, 5, 9), (9, 7, 5), (5, 5, 67), (2 * T3I + 3, 5, 5), (5, 2 * T3J + 3, 7), (9, 9, 131)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", TRANSFER_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_transfers_bit_for_bit(torch, lib, shape, dtype):
    code = _lib.dtype_code(dtype)
    cshape = tuple((n + 1) // 2 for n in shape)
    r, u = fields(shape, dtype, 31)
    e, old = fields(cshape, dtype, 32)
    for ldf, ldc in zip(pitches(dtype, shape[2]), pitches(dtype, cshape[2])):
        dr, dc = Guarded(torch, r, ldf), Guarded(torch, old, ldc)
        check3(lib.mg3_dev_restrict(code, *shape, ldf, ldc, dr.ptr, dc.ptr, None))
        torch.cuda.synchronize()
        assert same_bits(dc.cells()[R.INT], R.restrict(r)[R.INT])
        assert faces_equal(dc.cells(), old) and dc.outside_untouched() and dr.unwritten()
        de, du = Guarded(torch, e, ldc), Guarded(torch, u, ldf)
        check3(lib.mg3_dev_prolong_add(code, *shape, ldf, ldc, de.ptr, du.ptr, None))
        torch.cuda.synchronize()
        assert same_bits(du.cells(), R.prolong_add(u, e))
        assert du.outside_untouched() and de.unwritten()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 3, 3), (5, 9, 17), (6, 7, 10), (T3I + 3, T3J + 1, 70)], ids=lambda s: "%dx%dx%d" % s)
def test_norm_sums_every_cell_in_a_fixed_order(torch, lib, shape, dtype):
    a = fields(shape, dtype, 41)[0]
    for ld in pitches(dtype, shape[2]):
        da = Guarded(torch, a, ld)
        st, sp, ss = scratch_for(torch, lib, shape)
        got = []
        for _ in range(2):
            check3(lib.mg3_dev_norm(_lib.dtype_code(dtype), *shape, ld, da.ptr, sp, ss, None))
            torch.cuda.synchronize()
            got.append(float(st[-1].item()))
        exact = R.sumsq(a)
        assert got[0] == got[1] and abs(got[0] - exact) <= 1e-13 * exact and da.unwritten()
    grid = mg.Grid3D(*shape, domain=(0, 1, 0, 2, 0, 3))
    assert grid.l2_norm(a) == pytest.approx(math.sqrt(grid.hx * grid.hy * grid.hz * R.sumsq(a)), rel=1e-13)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 3, 3), (5, 5, 5), (9, 9, 9), (17, 17, 17), (5, 9, 33)], ids=lambda s: "%dx%dx%d" % s)
def test_coarse_solve_both_paths(torch, lib, shape, dtype):
    """64 red-black sweeps: one LDS launch when no extent exceeds 17, the colour kernel otherwise"""
    u, f = fields(shape, dtype, 51)
    h = R.spacings(shape)
    want = R.coarse_solve(u, f, h, 0.0, 64)
    for ld in pitches(dtype, shape[2]):
        du, df = Guarded(torch, u, ld), Guarded(torch, f, ld)
        used = C.c_int(-1)
        check3(lib.mg3_dev_coarse_solve(_lib.dtype_code(dtype), *shape, ld, *h, 0.0, 64, du.ptr, df.ptr, C.byref(used), None))
        torch.cuda.synchronize()
        assert used.value == (1 if max(shape) <= LDS_EXTENT else 0)
        got = du.cells()
        diff = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
        print(shape, np.dtype(dtype).name, "lds" if used.value else "colour kernel", "max diff", diff)
        if dtype == np.float64:
            assert diff <= 1e-13 * float(np.max(np.abs(want)))
        else:
            assert same_bits(got, want)
        assert faces_equal(got, u) and du.outside_untouched() and df.unwritten()


# ------------------------------------------------------------------------------------------ cycles
LEVELS = [((17, 17, 17), R.Config().domain), ((33, 33, 33), R.Config().domain), ((9, 17, 33), EQUAL_DOMAIN)]


@pytest.fixture(scope="module")
def problems():
    out = {}
    for shape, domain in LEVELS:
        rng = np.random.default_rng(7)
        f = rng.standard_normal(shape)
        u0 = np.zeros(shape)
        for face in [(0,), (-1,), (slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0), (slice(None), slice(None), -1)]:
            u0[face] = rng.standard_normal(u0[face].shape)
        out[shape] = (f, u0, domain)
    return out


@pytest.mark.parametrize("precision", ["double", "single"])
@pytest.mark.parametrize("smoother", ["jacobi", "rbgs"])
@pytest.mark.parametrize("cycle", ["V", "W"])
@pytest.mark.parametrize("shape", [s for s, _ in LEVELS], ids=lambda s: "%dx%dx%d" % s)
def test_three_cycles_follow_the_restatement(problems, shape, cycle, smoother, precision):
    f, u0, domain = problems[shape]
    dtype = np.float64 if precision == "double" else np.float32
    tol_u, tol_n = (1e-13, 1e-12) if precision == "double" else (1e-5, 1e-5)
    cfg = R.Config(domain=domain, cycle=cycle, smoother=smoother)
    u, fr = u0.astype(dtype), f.astype(dtype)
    with mg.Multigrid3DEngine(*shape, domain=domain, cycle=cycle, smoother=smoother, precision=precision) as eng:
        assert eng.num_levels == len(R.hierarchy(shape, 10))
        eng.set_rhs(f)
        eng.set_solution(u0)
        for k in range(3):
            eng.cycle(1)
            u = R.cycle(u, fr, cfg)
            got, want_norm = eng.solution(dtype=dtype), R.residual_norm(u, fr, cfg)
            diff = float(np.max(np.abs(got.astype(np.float64) - u.astype(np.float64))))
            norm = eng.residual_norm()
            print(shape, cycle, smoother, precision, "cycle", k + 1, "diff", diff, "norm", norm, "restatement", want_norm)
            assert diff <= tol_u * float(np.max(np.abs(u)))
            assert abs(norm - want_norm) <= tol_n * want_norm
        three = eng.solution(dtype=dtype)
        eng.set_solution(u0)
        eng.cycle(3)
        assert same_bits(eng.solution(dtype=dtype), three)


@pytest.mark.parametrize("smoother", ["jacobi", "rbgs"])
def test_defect_steps_follow_the_restatement(problems, smoother):
    """three outer steps, with and without a norm in between (the norm's residual pass is reused as the next step's right-hand side)"""
    shape = (17, 17, 17)
    f, u0, domain = problems[shape]
    cfg = R.Config(domain=domain, smoother=smoother)
    u = u0.copy()
    with mg.Multigrid3DEngine(*shape, domain=domain, smoother=smoother, precision="defect") as eng:
        eng.set_rhs(f)
        eng.set_solution(u0)
        for k in range(3):
            eng.cycle(1)
            u = R.defect_step(u, f, cfg)
            got = eng.solution()
            diff = float(np.max(np.abs(got - u)))
            print("defect", smoother, "step", k + 1, "diff", diff)
            assert diff <= 1e-13 * float(np.max(np.abs(u)))
            if k == 1:
                want = R.residual_norm(u, f, cfg)
                assert abs(eng.residual_norm() - want) <= 1e-12 * want
        three = eng.solution()
        eng.set_solution(u0)
        eng.cycle(3)
        assert same_bits(eng.solution(), three)


# ------------------------------------------------------------------------------------------ solves
@pytest.fixture(scope="module")
def solve33():
    shape = (33, 33, 33)
    rng = np.random.default_rng(3)
    f = rng.standard_normal(shape)
    cfg = R.Config(smoother="rbgs")
    fnorm = R.norm(f, R.spacings(shape))
    u, hist, conv = R.solve(np.zeros(shape), f, cfg, 1e-12 * fnorm, 40)
    assert conv
    return dict(shape=shape, f=f, cfg=cfg, fnorm=fnorm, u=u, hist=hist)


def cycles_to(hist, tol):
    return next(k for k, v in enumerate(hist) if v < tol)


def test_solve_double_counts_and_history(solve33):
    s = solve33
    with mg.Multigrid3DEngine(*s["shape"], smoother="rbgs") as eng:
        eng.set_rhs(s["f"])
        hist, conv = eng.solve(1e-10 * s["fnorm"], 40)
    want = cycles_to(s["hist"], 1e-10 * s["fnorm"])
    print("cycles", len(hist) - 1, "restatement", want)
    assert conv and abs(len(hist) - 1 - want) <= 1
    for k in range(min(len(hist), want + 1)):
        assert abs(hist[k] - s["hist"][k]) <= 1e-10 * s["hist"][k], k


def test_solve_single_stalls_and_says_so(solve33):
    s = solve33
    with mg.Multigrid3DEngine(*s["shape"], smoother="rbgs", precision="single") as eng:
        eng.set_rhs(s["f"])
        hist, conv = eng.solve(1e-10 * s["fnorm"], 20)
        print("single: relative history", [v / s["fnorm"] for v in hist])
        assert not conv and len(hist) - 1 == 20 and eng.last_stats.converged == 0 and eng.last_stats.iterations == 20


def test_solve_defect_reaches_double_accuracy(solve33):
    s = solve33
    tol = 1e-12 * s["fnorm"]
    with mg.Multigrid3DEngine(*s["shape"], smoother="rbgs", precision="defect") as eng:
        eng.set_rhs(s["f"])
        hist, conv = eng.solve(tol, 40)
        got = eng.solution()
    need = cycles_to(s["hist"], tol)
    print("defect steps", len(hist) - 1, "double cycles", need, "relative history", [v / s["fnorm"] for v in hist])
    assert conv and len(hist) - 1 <= need + 2
    assert float(np.max(np.abs(got - s["u"]))) <= 1e-10 * float(np.max(np.abs(s["u"])))


@pytest.mark.parametrize("precision", ["double", "defect"])
def test_harmonic_function_with_dirichlet_faces(precision):
    shape = (17, 17, 17)
    X, Y, Z = R.mesh(shape)
    exact = X + 2 * Y - 3 * Z
    u0 = exact.copy()
    u0[R.INT] = 0.0
    with mg.Multigrid3DEngine(*shape, smoother="rbgs", precision=precision) as eng:
        eng.set_rhs(np.zeros(shape))
        eng.set_solution(u0)
        eng.cycle(25)
        got = eng.solution()
    err = float(np.max(np.abs(got - exact)))
    print("harmonic", precision, "max error", err)
    assert err <= 1e-12 and faces_equal(got, exact)


def test_shifted_operator():
    shape, sigma = (17, 17, 17), 100.0
    rng = np.random.default_rng(9)
    f = rng.standard_normal(shape)
    cfg = R.Config(sigma=sigma)
    fnorm = R.norm(f, R.spacings(shape))
    u, want, conv = R.solve(np.zeros(shape), f, cfg, 1e-10 * fnorm, 40)
    with mg.Multigrid3DEngine(*shape, sigma=sigma) as eng:
        eng.set_rhs(f)
        hist, ok = eng.solve(1e-10 * fnorm, 40)
        got = eng.solution()
    assert conv and ok and len(hist) == len(want)
    assert np.allclose(hist, want, rtol=1e-10, atol=0.0)
    assert float(np.max(np.abs(got - u))) <= 1e-12 * float(np.max(np.abs(u)))
    assert float(np.max(np.abs(R.residual(got, f, R.spacings(shape), sigma)[R.INT]))) <= 1e-8 * float(np.max(np.abs(f)))


@pytest.mark.parametrize("precision", ["double", "single", "defect"])
def test_host_and_device_entry_points_give_the_same_bits(torch, problems, precision):
    shape = (9, 17, 33)
    f, u0, domain = problems[shape]
    results = []
    for form in ("host", "device64", "device32_padded"):
        with mg.Multigrid3DEngine(*shape, domain=domain, precision=precision) as eng:
            if form == "host":
                eng.set_rhs(f.astype(np.float32) if precision == "single" else f)
                eng.set_solution(u0)
                eng.cycle(2)
                results.append(eng.solution())
            else:
                tdt = torch.float64 if form == "device64" else torch.float32
                pad = 0 if form == "device64" else 8                  # a pitch of 42 floats: rows 8-byte aligned
                tf = torch.zeros(shape[:2] + (shape[2] + 1 + pad,), dtype=tdt, device="cuda")
                tu, out = torch.zeros_like(tf), torch.full_like(tf, float("nan"))
                tf[:, :, :shape[2]] = torch.from_numpy(f).to("cuda")
                tu[:, :, :shape[2]] = torch.from_numpy(u0).to("cuda")
                eng.set_rhs(tf)
                eng.set_solution(tu)
                eng.cycle(2)
                eng.solution(out=out)
                assert bool(torch.isnan(out[:, :, shape[2]:]).all())
                results.append(out[:, :, :shape[2]].cpu().numpy().astype(np.float64))
    if precision == "single":
        assert same_bits(results[0], results[1]) and same_bits(results[0], results[2])
    else:
        assert same_bits(results[0], results[1])          # an fp32 tensor rounds f and the faces on the way in
        assert float(np.max(np.abs(results[2] - results[0]))) <= 1e-5 * float(np.max(np.abs(results[0])))


def test_poisson_solver_3d_is_second_order():
    def exact(X, Y, Z):
        return np.sin(np.pi * X) * np.sin(np.pi * Y) * np.sin(np.pi * Z)
    problem = mg.applications.PoissonProblem("sine", lambda X, Y, Z: 3 * np.pi**2 * exact(X, Y, Z), exact,
                                {"type": "dirichlet", "value": 0.0}, (0, 1, 0, 1, 0, 1))
    solver = mg.PoissonSolver3D(tolerance=1e-10, smoother="rbgs")
    res = [solver.solve_poisson_problem_3d(problem, n, n, n) for n in (17, 33)]
    assert all(r["solver_info"]["converged"] for r in res) and res[1]["grid_size"] == (33, 33, 33)
    assert set(res[0]) == {"problem_name", "grid_size", "domain", "solution", "solve_time", "solver_info", "errors", "solver_type",
                           "use_gpu", "mixed_precision", "analytical_solution"}
    ratio = res[0]["errors"]["max_error"] / res[1]["errors"]["max_error"]
    print("max errors", [r["errors"]["max_error"] for r in res], "ratio", ratio)
    assert 3.9 <= ratio <= 4.1                                      # tests/test_mg3_cpu.py's window
    assert res[1]["solver_info"]["device_bytes"] == solver.get_memory_requirements_3d(33, 33, 33)["device_bytes"]
    with pytest.raises(NotImplementedError):
        solver.solve_poisson_problem_3d(mg.applications.PoissonProblem("n", problem.source_function, None, {"type": "neumann"}, problem.domain), 9, 9, 9)
