"""Semilinear elliptic problems  A u + kappa w(x, y) phi(u) = f  on the device (include/mghip_nl.h): an inexact Newton method
whose iterate, residual and Jacobian diagonal stay on the device, with multigrid-preconditioned conjugate gradients (krylov.py's
loop with a reaction field) as the inner solver.  A is -Laplacian (+ shift) or -div(a grad .); phi is "linear" (u), "cubic"
(u^3), "sinh" or "exp" -- all monotone, so every Jacobian A + diag(kappa w phi'(u)) is symmetric positive definite.
Non-monotone terms (a negative strength or weight) are refused.

SemilinearEngine is the thin owner of one mg_nl; SemilinearSolver has the shape of PCGSolver (setup / solve)."""
import ctypes as C

import numpy as np

from . import _lib
from .engine import _direct_code
from .krylov import PRECISIONS
from .smoothers import GaussSeidelSmoother, IterativeSolver


def _nl_check(rc, handle=None):
    if rc == _lib.MG_OK:
        return
    msg = _lib.load().mg_nl_last_error(handle)
    msg = (msg.decode() if msg else "") or f"mghip error {rc}"
    if rc in (_lib.MG_ERR_INVALID_VALUE, _lib.MG_ERR_STATE):
        raise ValueError(msg)
    if rc == _lib.MG_ERR_ALLOC:
        raise MemoryError(msg)
    raise RuntimeError("mghip: " + msg)


def _checked_weight(weight):
    """the weight field as a float64 array, or ValueError for a negative or non-finite entry"""
    if weight is None:
        return None
    w = np.ascontiguousarray(weight, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError("weight must be a 2-D field")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("weight must be finite and >= 0 everywhere (monotone nonlinearities only)")
    return w


class SemilinearEngine:
    """Owns one mg_nl: the Newton iterates, the inner PCG solver and its preconditioner engine.  The leading arguments are the
    fields of mg_config (the preconditioner's configuration), as for PCGEngine."""

    def __init__(self, nx, ny, domain=(0.0, 1.0, 0.0, 1.0), coeff=-1.0, max_levels=4, cycle="V", pre=2, post=2,
                 smoother=_lib.MG_JACOBI, omega=0.8, coarse_tol=1e-12, coarse_maxit=1000, precision=_lib.MG_PREC_DOUBLE,
                 num_cycles=1, flexible=None, device=0, coarse_direct=None):
        lib = _lib.load()
        if isinstance(cycle, str):
            if cycle not in _lib.CYCLES:
                raise ValueError(f"unknown cycle type {cycle!r}")
            cycle = _lib.CYCLES[cycle]
        cfg = _lib.MgConfig(int(nx), int(ny), float(domain[0]), float(domain[1]), float(domain[2]), float(domain[3]),
                            float(coeff), int(max_levels), int(cycle), int(pre), int(post), int(smoother), float(omega),
                            float(coarse_tol), int(coarse_maxit), int(precision), 1e-6, 4.0, 0, int(device), 0, 0, 2, 1, 0, 2,
                            _direct_code(coarse_direct), 0)
        self.cfg = cfg
        self.nx, self.ny = int(nx), int(ny)
        self._h = C.c_void_p(None)
        self._lib = lib
        _nl_check(lib.mg_nl_create(C.byref(cfg), int(num_cycles), -1 if flexible is None else int(bool(flexible)),
                                   C.byref(self._h)))

    def _check(self, rc):
        _nl_check(rc, self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mg_nl_destroy(self._h)
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
        """A = coeff * div(a grad .) for the eval kernel, the inner operator and the preconditioner (None: constant coefficients)"""
        if a is None:
            self._check(self._lib.mg_nl_set_coefficient(self._h, None, _lib.MG_F64))
            return
        a = _lib.as_c(a)
        if a.shape != (self.nx, self.ny):
            raise ValueError(f"coefficient shape {a.shape} doesn't match grid shape {(self.nx, self.ny)}")
        self._check(self._lib.mg_nl_set_coefficient(self._h, _lib.ptr(a), _lib.dtype_code(a.dtype)))

    def set_shift(self, sigma):
        self._check(self._lib.mg_nl_set_shift(self._h, float(sigma)))

    def set_nonlinearity(self, kind, kappa, weight=None):
        """kind: a name of _lib.NL_KINDS or its code; g(u) = kappa * weight * phi(u)"""
        code = _lib.NL_KINDS[kind] if isinstance(kind, str) else int(kind)
        if weight is None:
            self._check(self._lib.mg_nl_set_nonlinearity(self._h, code, float(kappa), None, _lib.MG_F64))
            return
        w = _lib.as_c(weight)
        if w.shape != (self.nx, self.ny):
            raise ValueError(f"weight shape {w.shape} doesn't match grid shape {(self.nx, self.ny)}")
        self._check(self._lib.mg_nl_set_nonlinearity(self._h, code, float(kappa), _lib.ptr(w), _lib.dtype_code(w.dtype)))

    def set_options(self, forcing="eisenstat_walker", eta=1e-8, gamma=0.9, eta_max=0.1, eta_min=1e-10, max_backtracks=10,
                    max_inner=100):
        opt = _lib.MgNlOptions(_lib.NL_FORCINGS[forcing], int(max_backtracks), int(max_inner), 0, float(eta), float(gamma),
                               float(eta_max), float(eta_min))
        self._check(self._lib.mg_nl_set_options(self._h, C.byref(opt)))

    def solve(self, f, u0=None, tol=1e-8, max_newton=30):
        """host arrays in, host array out (the dtype of f: float32 or float64); the ring of u0 is the Dirichlet data"""
        f = _lib.as_c(f)
        if f.shape != (self.nx, self.ny):
            raise ValueError("semilinear solver not properly setup or grid mismatch")
        u0c = None if u0 is None else np.ascontiguousarray(u0, dtype=f.dtype)
        if u0c is not None and u0c.shape != f.shape:
            raise ValueError("initial guess shape does not match the grid")
        if max_newton < 1:
            raise ValueError("max_newton must be >= 1")
        out = np.empty_like(f)
        norms, steps, etas = ((C.c_double * max_newton)() for _ in range(3))
        inner = (C.c_int * max_newton)()
        nit, conv = C.c_int(0), C.c_int(0)
        stats = _lib.MgNlStats()
        self._check(self._lib.mg_nl_solve(self._h, _lib.ptr(f), None if u0c is None else _lib.ptr(u0c), _lib.ptr(out),
                                          _lib.dtype_code(f.dtype), float(tol), int(max_newton), norms, inner, steps, etas,
                                          max_newton, C.byref(nit), C.byref(conv), C.byref(stats)))
        n = nit.value
        return out, {"newton_iterations": n, "inner_iterations": [inner[i] for i in range(n)],
                     "total_inner_iterations": stats.inner_iterations, "residual_history": [norms[i] for i in range(n)],
                     "step_lengths": [steps[i] for i in range(n)], "forcing_terms": [etas[i] for i in range(n)],
                     "status": _lib.NL_STATUS.get(stats.status, stats.status), "converged": bool(conv.value),
                     "initial_residual": stats.initial_residual, "true_residual": stats.final_residual,
                     "evaluations": stats.evaluations, "solve_seconds": stats.solve_seconds}


class SemilinearSolver:
    """Newton - conjugate gradients - multigrid for  A u + strength * weight * phi(u) = f  on the device, with the Dirichlet
    data on the ring of the initial guess.  Shaped like PCGSolver: setup(fine_grid, operator, ...), solve(f, initial_guess).

    nonlinearity: "linear", "cubic", "sinh" or "exp"; strength >= 0 and weight >= 0 (None: 1) -- the term must be monotone.
    tolerance is absolute, on ||f - N(u)||_h over interior cells (PCGSolver's convention).  precision is the PRECONDITIONER's
    ("double", "single_managed", "mixed"); the Newton and Krylov state is always fp64.  forcing: "eisenstat_walker" (choice 2:
    gamma, eta_max, eta_min) or "fixed" (the constant eta).  info["status"]: "converged", "max_newton", "breakdown" (the inner
    solver broke down before its first step) or "line_search_failed" (no step length down to 2^-max_backtracks reduced the
    residual; the last accepted iterate is returned)."""

    def __init__(self, nonlinearity="sinh", strength=1.0, weight=None, max_levels=4, tolerance=1e-8, precision="double",
                 max_newton=30, forcing="eisenstat_walker", eta=1e-8, gamma=0.9, eta_max=0.1, eta_min=1e-10, max_backtracks=10,
                 max_inner=100, cycle_type="V", pre_smooth_iterations=2, post_smooth_iterations=2, num_cycles=1, flexible=None,
                 device_id=0, coarse_tolerance=1e-12, coarse_max_iterations=1000, coarse_direct=None):
        if nonlinearity not in _lib.NL_KINDS:
            raise ValueError(f"nonlinearity must be one of {sorted(_lib.NL_KINDS)}, not {nonlinearity!r}")
        strength = float(strength)
        if not (strength >= 0.0) or not np.isfinite(strength):
            raise ValueError("strength must be finite and >= 0 (monotone nonlinearities only; Bratu-type terms are out of scope)")
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)} (the preconditioner's; the Newton state is fp64), "
                             f"not {precision!r}")
        if forcing not in _lib.NL_FORCINGS:
            raise ValueError(f"forcing must be one of {sorted(_lib.NL_FORCINGS)}, not {forcing!r}")
        cycle_type = getattr(cycle_type, "value", cycle_type)
        if cycle_type not in _lib.CYCLES:
            raise ValueError(f"unknown cycle type {cycle_type!r}")
        if int(max_newton) < 1 or int(max_inner) < 1 or int(num_cycles) < 1 or int(max_backtracks) < 0:
            raise ValueError("max_newton, max_inner and num_cycles must be >= 1 and max_backtracks >= 0")
        if not (0.0 < eta < 1.0 and 0.0 < gamma <= 1.0 and 0.0 < eta_min <= eta_max < 1.0):
            raise ValueError("forcing terms: 0 < eta < 1, 0 < gamma <= 1, 0 < eta_min <= eta_max < 1")
        if pre_smooth_iterations < 0 or post_smooth_iterations < 0 or pre_smooth_iterations + post_smooth_iterations == 0:
            raise ValueError("the preconditioner needs at least one smoothing sweep")
        self.name = "Newton-PCG"
        self.nonlinearity, self.strength, self.weight = nonlinearity, strength, _checked_weight(weight)
        self.max_levels, self.tolerance, self.precision, self.max_newton = int(max_levels), float(tolerance), precision, int(max_newton)
        self.forcing, self.eta, self.gamma, self.eta_max, self.eta_min = forcing, float(eta), float(gamma), float(eta_max), float(eta_min)
        self.max_backtracks, self.max_inner = int(max_backtracks), int(max_inner)
        self.cycle_type = cycle_type
        self.pre_smooth_iterations, self.post_smooth_iterations = int(pre_smooth_iterations), int(post_smooth_iterations)
        self.num_cycles, self.flexible, self.device_id = int(num_cycles), flexible, device_id
        self.coarse_tolerance, self.coarse_max_iterations, self.coarse_direct = coarse_tolerance, coarse_max_iterations, coarse_direct
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
            raise ValueError("the Newton method's inner solver needs an SPD operator: coefficient < 0 (-Laplacian, -div(a grad .))")
        if self.weight is not None and self.weight.shape != (fine_grid.nx, fine_grid.ny):
            raise ValueError(f"weight shape {self.weight.shape} doesn't match grid shape {(fine_grid.nx, fine_grid.ny)}")
        field = operator.field(fine_grid) if hasattr(operator, "field") else None
        self.close()
        self.grid, self.operator = fine_grid, operator
        self._engine = SemilinearEngine(fine_grid.nx, fine_grid.ny, fine_grid.domain, coeff, self.max_levels, self.cycle_type,
                                        self.pre_smooth_iterations, self.post_smooth_iterations, smoother.kind, smoother.omega,
                                        self.coarse_tolerance, self.coarse_max_iterations, PRECISIONS[self.precision],
                                        self.num_cycles, self.flexible, self.device_id, coarse_direct=self.coarse_direct)
        if field is not None:
            self._engine.set_coefficient(field)
        self._engine.set_shift(getattr(operator, "shift", 0.0))
        self._engine.set_nonlinearity(self.nonlinearity, self.strength, self.weight)
        self._engine.set_options(self.forcing, self.eta, self.gamma, self.eta_max, self.eta_min, self.max_backtracks, self.max_inner)

    def solve(self, f, initial_guess=None):
        if self._engine is None:
            raise ValueError("semilinear solver not properly setup or grid mismatch")
        f = np.asarray(f)
        if f.shape != self.grid.shape:
            raise ValueError("semilinear solver not properly setup or grid mismatch")
        work = np.float32 if f.dtype == np.float32 else np.float64
        return self._engine.solve(np.ascontiguousarray(f, dtype=work), initial_guess, self.tolerance, self.max_newton)

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
