"""Device-resident preconditioned conjugate gradients with the multigrid cycle as preconditioner (include/mghip.h, "Krylov
outer loop"): the fp64 Krylov loop, its vectors and its scalars stay on the device; the preconditioner is an engine of its own
that may run in fp64, in fp32 on every level but the coarsest ("single_managed") or in fp32 on the coarser half ("mixed").

PCGEngine is the thin owner of one mg_pcg; PCGSolver has the shape of MultigridSolver (setup / solve)."""
import ctypes as C

import numpy as np

from . import _lib
from .engine import _direct_code
from .smoothers import GaussSeidelSmoother, IterativeSolver

PRECISIONS = {"double": _lib.MG_PREC_DOUBLE, "single_managed": _lib.MG_PREC_SINGLE_MANAGED, "mixed": _lib.MG_PREC_MIXED_LEVELS}


def _pcg_check(rc, handle=None):
    if rc == _lib.MG_OK:
        return
    msg = _lib.load().mg_pcg_last_error(handle)
    msg = (msg.decode() if msg else "") or f"mghip error {rc}"
    if rc in (_lib.MG_ERR_INVALID_VALUE, _lib.MG_ERR_STATE):
        raise ValueError(msg)
    if rc == _lib.MG_ERR_ALLOC:
        raise MemoryError(msg)
    raise RuntimeError("mghip: " + msg)


class PCGEngine:
    """Owns one mg_pcg: the Krylov vectors and the preconditioner engine.  The leading arguments are the fields of mg_config
    (the preconditioner's configuration); flexible: True / False / None (auto: True unless the smoother is Jacobi with
    pre == post, the one symmetric configuration)."""

    def __init__(self, nx, ny, domain=(0.0, 1.0, 0.0, 1.0), coeff=-1.0, max_levels=4, cycle="V", pre=2, post=2,
                 smoother=_lib.MG_JACOBI, omega=0.8, coarse_tol=1e-12, coarse_maxit=1000, precision=_lib.MG_PREC_DOUBLE,
                 num_cycles=1, flexible=None, device=0, fused=2, tail=True, fmg_cycles=0, coarse_direct=None):
        lib = _lib.load()
        if isinstance(cycle, str):
            if cycle not in _lib.CYCLES:
                raise ValueError(f"unknown cycle type {cycle!r}")
            cycle = _lib.CYCLES[cycle]
        cfg = _lib.MgConfig(int(nx), int(ny), float(domain[0]), float(domain[1]), float(domain[2]), float(domain[3]),
                            float(coeff), int(max_levels), int(cycle), int(pre), int(post), int(smoother), float(omega),
                            float(coarse_tol), int(coarse_maxit), int(precision), 1e-6, 4.0, 0, int(device), 0, 0, int(fused),
                            int(tail), int(fmg_cycles), 2, _direct_code(coarse_direct), 0)
        self.cfg = cfg
        self.nx, self.ny = int(nx), int(ny)
        self._h = C.c_void_p(None)
        self._lib = lib
        _pcg_check(lib.mg_pcg_create(C.byref(cfg), int(num_cycles), -1 if flexible is None else int(bool(flexible)),
                                     C.byref(self._h)))
        self.flexible = bool(smoother != _lib.MG_JACOBI or pre != post) if flexible is None else bool(flexible)
        self.order = 2

    def _check(self, rc):
        _pcg_check(rc, self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mg_pcg_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_coefficient(self, a):
        """A = coeff * div(a grad .) for the outer operator and the preconditioner (None: constant coefficients)"""
        if a is None:
            self._check(self._lib.mg_pcg_set_coefficient(self._h, None, _lib.MG_F64))
            return
        a = _lib.as_c(a)
        if a.shape != (self.nx, self.ny):
            raise ValueError(f"coefficient shape {a.shape} doesn't match grid shape {(self.nx, self.ny)}")
        self._check(self._lib.mg_pcg_set_coefficient(self._h, _lib.ptr(a), _lib.dtype_code(a.dtype)))

    def set_shift(self, sigma):
        self._check(self._lib.mg_pcg_set_shift(self._h, float(sigma)))

    def set_order(self, order):
        """2 (default): the five-point operator; 4: the fourth-order compact nine-point scheme (include/mghip_ho.h), constant
        coefficients only.  The preconditioner is the five-point cycle either way."""
        self._check(self._lib.mg_pcg_set_order(self._h, int(order)))
        self.order = int(order)

    def set_lookahead(self, on):
        self._check(self._lib.mg_pcg_set_lookahead(self._h, int(bool(on))))

    def _info(self, hist, nit, conv, stats):
        n = nit.value
        h = [hist[i] for i in range(n)]
        return {"iterations": n, "converged": bool(conv.value), "residual_history": h,
                "final_residual": h[-1] if h else stats.initial_residual, "true_residual": stats.true_residual,
                "initial_residual": stats.initial_residual, "status": _lib.PCG_STATUS.get(stats.status, stats.status),
                "flexible": self.flexible, "order": self.order, "solve_seconds": stats.solve_seconds, "precond_seconds": stats.precond_seconds}

    def solve(self, rhs, u0=None, tol=1e-8, max_iterations=50):
        """host arrays in, host array out (the dtype of rhs: float32 or float64); the ring of u0 is the Dirichlet data"""
        rhs = _lib.as_c(rhs)
        if rhs.shape != (self.nx, self.ny):
            raise ValueError("PCG solver not properly setup or grid mismatch")
        u0c = None if u0 is None else np.ascontiguousarray(u0, dtype=rhs.dtype)
        if u0c is not None and u0c.shape != rhs.shape:
            raise ValueError("initial guess shape does not match the grid")
        if max_iterations < 1:
            raise ValueError("max_iterations must be >= 1")
        out = np.empty_like(rhs)
        hist = (C.c_double * max_iterations)()
        nit, conv = C.c_int(0), C.c_int(0)
        stats = _lib.MgPcgStats()
        self._check(self._lib.mg_pcg_solve(self._h, _lib.ptr(rhs), None if u0c is None else _lib.ptr(u0c), _lib.ptr(out),
                                           _lib.dtype_code(rhs.dtype), float(tol), int(max_iterations), hist, max_iterations,
                                           C.byref(nit), C.byref(conv), C.byref(stats)))
        return out, self._info(hist, nit, conv, stats)

    def solve_device(self, rhs_t, x_t, tol=1e-8, max_iterations=50):
        """2-D device tensors (nx, >= ny) of one dtype; x_t holds the initial guess and Dirichlet ring and receives the solution"""
        if rhs_t.dtype != x_t.dtype or tuple(rhs_t.shape)[0] != self.nx or tuple(x_t.shape)[0] != self.nx:
            raise ValueError("PCG solver not properly setup or grid mismatch")
        if max_iterations < 1:
            raise ValueError("max_iterations must be >= 1")
        dt = _lib.dtype_code(str(rhs_t.dtype).split(".")[-1])
        hist = (C.c_double * max_iterations)()
        nit, conv = C.c_int(0), C.c_int(0)
        stats = _lib.MgPcgStats()
        self._check(self._lib.mg_pcg_solve_device(self._h, C.c_void_p(rhs_t.data_ptr()), int(rhs_t.stride(0)),
                                                  C.c_void_p(x_t.data_ptr()), int(x_t.stride(0)), dt, float(tol),
                                                  int(max_iterations), hist, max_iterations, C.byref(nit), C.byref(conv),
                                                  C.byref(stats)))
        return self._info(hist, nit, conv, stats)


class PCGSolver:
    """Conjugate gradients for A u = f (A = -Laplacian, -Laplacian + shift or -div(a grad .)) preconditioned by `num_cycles`
    multigrid cycles, on the device.  Shaped like MultigridSolver: setup(fine_grid, operator, ...), solve(grid, operator, rhs).

    precision is the PRECONDITIONER's ("double", "single_managed", "mixed"); the outer loop is always fp64.  flexible=None
    picks the flexible beta whenever the cycle is not symmetric (anything but Jacobi with pre == post).

    order=4 discretises -Laplacian (+ shift) with the fourth-order compact nine-point scheme (include/mghip_ho.h): the loop
    solves A4 u = R f, preconditioned by the same five-point cycle.  The right-hand side is then read on its ring too (the
    Dirichlet data is still the ring of the initial guess), the residual norms run over interior cells only, and the
    operator must have constant coefficients."""

    def __init__(self, max_levels=4, max_iterations=50, tolerance=1e-8, cycle_type="V", pre_smooth_iterations=2,
                 post_smooth_iterations=2, num_cycles=1, flexible=None, precision="double", device_id=0,
                 coarse_tolerance=1e-12, coarse_max_iterations=1000, coarse_direct=None, order=2):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)} (the preconditioner's; the Krylov loop is fp64), "
                             f"not {precision!r}")
        cycle_type = getattr(cycle_type, "value", cycle_type)
        if cycle_type not in _lib.CYCLES:
            raise ValueError(f"unknown cycle type {cycle_type!r}")
        if int(num_cycles) < 1:
            raise ValueError("num_cycles must be >= 1")
        if order not in (2, 4):
            raise ValueError(f"order must be 2 (five-point) or 4 (compact nine-point), not {order!r}")
        if int(max_iterations) < 1:
            raise ValueError("max_iterations must be >= 1")
        if pre_smooth_iterations < 0 or post_smooth_iterations < 0 or pre_smooth_iterations + post_smooth_iterations == 0:
            raise ValueError("the preconditioner needs at least one smoothing sweep")
        self.name = "PCG"
        self.max_levels, self.max_iterations, self.tolerance = int(max_levels), int(max_iterations), float(tolerance)
        self.cycle_type = cycle_type
        self.pre_smooth_iterations, self.post_smooth_iterations = int(pre_smooth_iterations), int(post_smooth_iterations)
        self.num_cycles, self.flexible, self.precision = int(num_cycles), flexible, precision
        self.device_id = device_id
        self.coarse_tolerance, self.coarse_max_iterations, self.coarse_direct = coarse_tolerance, coarse_max_iterations, coarse_direct
        self.order = int(order)
        self.grid = self.operator = self._engine = None

    def setup(self, fine_grid, operator, restriction_op=None, prolongation_op=None, smoother=None):
        if restriction_op is not None and restriction_op.method != "full_weighting":
            raise NotImplementedError("the accelerated path implements full_weighting restriction")
        if prolongation_op is not None and prolongation_op.method != "bilinear":
            raise NotImplementedError("the accelerated path implements bilinear prolongation")
        if smoother is None:
            smoother = GaussSeidelSmoother(red_black=True)
        if hasattr(smoother, "resolve"):               # LineRelaxationSmoother: "auto" against this grid, operator check
            smoother.resolve(fine_grid, operator)
        if not isinstance(smoother, IterativeSolver) or smoother.kind is None:
            raise TypeError("smoother must be a JacobiSmoother / GaussSeidelSmoother (or subclass)")
        if smoother.kind == _lib.MG_LEXGS:
            raise NotImplementedError("the preconditioner smooths with weighted Jacobi or red-black Gauss-Seidel")
        coeff = float(getattr(operator, "coefficient", -1.0))
        if not coeff < 0:
            raise ValueError("conjugate gradients need an SPD operator: coefficient < 0 (-Laplacian, -div(a grad .))")
        if self.order == 4 and hasattr(operator, "field"):
            raise NotImplementedError("order=4 (the compact nine-point scheme) needs constant coefficients: -Laplacian or "
                                      "-Laplacian + shift, not a DiffusionOperator")
        field = operator.field(fine_grid) if hasattr(operator, "field") else None
        self.close()
        self.grid, self.operator = fine_grid, operator
        self._engine = PCGEngine(fine_grid.nx, fine_grid.ny, fine_grid.domain, coeff, self.max_levels, self.cycle_type,
                                 self.pre_smooth_iterations, self.post_smooth_iterations, smoother.kind, smoother.omega,
                                 self.coarse_tolerance, self.coarse_max_iterations, PRECISIONS[self.precision], self.num_cycles,
                                 self.flexible, self.device_id, coarse_direct=self.coarse_direct)
        if field is not None:
            self._engine.set_coefficient(field)
        if self.order != 2:
            self._engine.set_order(self.order)

    def solve(self, grid, operator, rhs, initial_guess=None):
        if self._engine is None or grid.shape != self.grid.shape:
            raise ValueError("PCG solver not properly setup or grid mismatch")
        self._engine.set_shift(getattr(operator, "shift", 0.0))
        rhs = np.asarray(rhs)
        work = np.float32 if rhs.dtype == np.float32 else np.float64
        return self._engine.solve(np.ascontiguousarray(rhs, dtype=work), initial_guess, self.tolerance, self.max_iterations)

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None

    cleanup = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
