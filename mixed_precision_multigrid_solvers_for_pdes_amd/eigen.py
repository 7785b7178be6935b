"""Device-resident block eigensolver (include/mghip_eig.h): the lowest eigenpairs of -Laplacian or -div(a grad .) with
homogeneous Dirichlet conditions by LOBPCG, preconditioned by the multigrid cycle.  The fp64 block vectors and their Gram
matrices stay on the device; the preconditioner is an engine of its own that may run in fp64, in fp32 on every level but the
coarsest ("single_managed") or in fp32 on the coarser half ("mixed").

EigenEngine is the thin owner of one mg_eig; EigenSolver has the shape of PCGSolver (setup / solve)."""
import ctypes as C

import numpy as np

from . import _lib
from .engine import _direct_code
from .krylov import PRECISIONS
from .smoothers import GaussSeidelSmoother, IterativeSolver

MAX_BLOCK = 16


def _eig_check(rc, handle=None):
    if rc == _lib.MG_OK:
        return
    msg = _lib.load().mg_eig_last_error(handle)
    msg = (msg.decode() if msg else "") or f"mghip error {rc}"
    if rc in (_lib.MG_ERR_INVALID_VALUE, _lib.MG_ERR_STATE):
        raise ValueError(msg)
    if rc == _lib.MG_ERR_ALLOC:
        raise MemoryError(msg)
    raise RuntimeError("mghip: " + msg)


def host_ritz(ga, gb, m):
    """Step 5 of the iteration on host arrays: the lowest m eigenpairs of G_A c = lambda G_B c -> (eigenvalues[m],
    coefficients[n, m]) with C^T G_B C = I; None when G_B is not positive definite."""
    ga, gb = np.ascontiguousarray(ga, dtype=np.float64), np.ascontiguousarray(gb, dtype=np.float64)
    n = ga.shape[0]
    if ga.shape != (n, n) or gb.shape != (n, n):
        raise ValueError("host_ritz takes two square matrices of one size")
    evals, coef = np.empty(int(m)), np.empty((n, int(m)))
    as_pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = _lib.load().mg_eig_host_ritz(n, int(m), as_pd(ga), as_pd(gb), as_pd(evals), as_pd(coef))
    if rc == 1:
        return None
    _eig_check(rc)
    return evals, coef


class EigenEngine:
    """Owns one mg_eig: two blocks of 6 * block_size fp64 columns and the preconditioner engine.  The leading arguments are
    the fields of mg_config (the preconditioner's configuration)."""

    def __init__(self, nx, ny, domain=(0.0, 1.0, 0.0, 1.0), coeff=-1.0, max_levels=4, cycle="V", pre=2, post=2,
                 smoother=_lib.MG_JACOBI, omega=0.8, coarse_tol=1e-12, coarse_maxit=1000, precision=_lib.MG_PREC_DOUBLE,
                 block_size=6, num_cycles=1, device=0, fused=2, tail=True, coarse_direct=None):
        lib = _lib.load()
        if isinstance(cycle, str):
            if cycle not in _lib.CYCLES:
                raise ValueError(f"unknown cycle type {cycle!r}")
            cycle = _lib.CYCLES[cycle]
        cfg = _lib.MgConfig(int(nx), int(ny), float(domain[0]), float(domain[1]), float(domain[2]), float(domain[3]),
                            float(coeff), int(max_levels), int(cycle), int(pre), int(post), int(smoother), float(omega),
                            float(coarse_tol), int(coarse_maxit), int(precision), 1e-6, 4.0, 0, int(device), 0, 0, int(fused),
                            int(tail), 0, 2, _direct_code(coarse_direct), 0)
        self.cfg = cfg
        self.nx, self.ny, self.block_size = int(nx), int(ny), int(block_size)
        self._h = C.c_void_p(None)
        self._lib = lib
        _eig_check(lib.mg_eig_create(C.byref(cfg), int(block_size), int(num_cycles), C.byref(self._h)))

    def _check(self, rc):
        _eig_check(rc, self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mg_eig_destroy(self._h)
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
        """A = coeff * div(a grad .) for the block stencil and the preconditioner (None: constant coefficients)"""
        if a is None:
            self._check(self._lib.mg_eig_set_coefficient(self._h, None, _lib.MG_F64))
            return
        a = _lib.as_c(a)
        if a.shape != (self.nx, self.ny):
            raise ValueError(f"coefficient shape {a.shape} doesn't match grid shape {(self.nx, self.ny)}")
        self._check(self._lib.mg_eig_set_coefficient(self._h, _lib.ptr(a), _lib.dtype_code(a.dtype)))

    def solve(self, x0, nev=None, tol=1e-8, max_iterations=100):
        """x0: (block_size, nx, ny) start vectors (float32 or float64) -> (eigenvalues[nev], vectors[nev, nx, ny], info)"""
        x0 = _lib.as_c(x0)
        m = self.block_size
        if x0.shape != (m, self.nx, self.ny):
            raise ValueError(f"start vectors of shape {x0.shape}: expected {(m, self.nx, self.ny)}")
        nev = m if nev is None else int(nev)
        if not 1 <= nev <= m:
            raise ValueError("the number of eigenpairs must be between 1 and the block size")
        if max_iterations < 0:
            raise ValueError("max_iterations must be >= 0")
        vecs = np.empty((nev, self.nx, self.ny), dtype=x0.dtype)
        evals, resid = (C.c_double * m)(), (C.c_double * m)()
        cap = int(max_iterations) + 1
        hist = (C.c_double * cap)()
        nit, conv = C.c_int(0), C.c_int(0)
        stats = _lib.MgEigStats()
        self._check(self._lib.mg_eig_solve(self._h, nev, _lib.ptr(x0), _lib.dtype_code(x0.dtype), float(tol), int(max_iterations),
                                           evals, _lib.ptr(vecs), resid, hist, cap, C.byref(nit), C.byref(conv), C.byref(stats)))
        n = nit.value
        info = {"iterations": n, "converged": bool(conv.value), "status": _lib.PCG_STATUS.get(stats.status, stats.status),
                "residuals": np.array(resid[:nev]), "residual_history": [hist[i] for i in range(min(n + 1, cap))],
                "restarts": stats.restarts, "solve_seconds": stats.solve_seconds, "precond_seconds": stats.precond_seconds,
                "block_eigenvalues": np.array(evals[:m])}
        return np.array(evals[:nev]), vecs, info

    def time_op(self, op, reps=20):
        """mean milliseconds of one launch: 0 apply, 1 gram (3m x 6m), 2 combine (3m -> 2m), 3 one preconditioner application"""
        ms = C.c_double(0.0)
        self._check(self._lib.mg_eig_time_op(self._h, int(op), int(reps), C.byref(ms)))
        return ms.value


class EigenSolver:
    """The `num_eigenpairs` lowest eigenpairs of A = -Laplacian or -div(a grad .) (zero Dirichlet ring) by LOBPCG with
    `num_cycles` multigrid cycles as preconditioner, on the device.  Shaped like PCGSolver: setup(fine_grid, operator, ...),
    then solve() -> (eigenvalues, vectors, info); a vector v is scaled to Grid.l2_norm(v) == 1, its sign is unspecified.

    precision is the PRECONDITIONER's ("double", "single_managed", "mixed"); the eigenpairs are always fp64.  block_size=None
    iterates on min(16, num_eigenpairs + 2) vectors: the extra ones keep the wanted pairs away from the end of the block."""

    def __init__(self, num_eigenpairs=4, block_size=None, max_levels=4, max_iterations=100, tolerance=1e-8, cycle_type="V",
                 pre_smooth_iterations=2, post_smooth_iterations=2, num_cycles=1, precision="double", seed=0, device_id=0,
                 coarse_tolerance=1e-12, coarse_max_iterations=1000, coarse_direct=None):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)} (the preconditioner's; the eigenpairs are fp64), "
                             f"not {precision!r}")
        cycle_type = getattr(cycle_type, "value", cycle_type)
        if cycle_type not in _lib.CYCLES:
            raise ValueError(f"unknown cycle type {cycle_type!r}")
        if int(num_eigenpairs) < 1:
            raise ValueError("num_eigenpairs must be >= 1")
        if block_size is None:
            block_size = min(MAX_BLOCK, int(num_eigenpairs) + 2)
        if not 1 <= int(block_size) <= MAX_BLOCK:
            raise ValueError(f"block_size must be between 1 and {MAX_BLOCK}")
        if int(num_eigenpairs) > int(block_size):
            raise ValueError("num_eigenpairs must not exceed block_size")
        if int(num_cycles) < 1:
            raise ValueError("num_cycles must be >= 1")
        if int(max_iterations) < 0:
            raise ValueError("max_iterations must be >= 0")
        if pre_smooth_iterations < 0 or post_smooth_iterations < 0 or pre_smooth_iterations + post_smooth_iterations == 0:
            raise ValueError("the preconditioner needs at least one smoothing sweep")
        self.name = "LOBPCG"
        self.num_eigenpairs, self.block_size = int(num_eigenpairs), int(block_size)
        self.max_levels, self.max_iterations, self.tolerance = int(max_levels), int(max_iterations), float(tolerance)
        self.cycle_type = cycle_type
        self.pre_smooth_iterations, self.post_smooth_iterations = int(pre_smooth_iterations), int(post_smooth_iterations)
        self.num_cycles, self.precision, self.seed = int(num_cycles), precision, seed
        self.device_id = device_id
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
            raise ValueError("the eigensolver needs an SPD operator: coefficient < 0 (-Laplacian, -div(a grad .))")
        if getattr(operator, "shift", 0.0):
            raise NotImplementedError("the eigensolver takes no shift: the eigenvalues of A + sigma I are those of A plus sigma")
        field = operator.field(fine_grid) if hasattr(operator, "field") else None
        self.close()
        self.grid, self.operator = fine_grid, operator
        self._engine = EigenEngine(fine_grid.nx, fine_grid.ny, fine_grid.domain, coeff, self.max_levels, self.cycle_type,
                                   self.pre_smooth_iterations, self.post_smooth_iterations, smoother.kind, smoother.omega,
                                   self.coarse_tolerance, self.coarse_max_iterations, PRECISIONS[self.precision],
                                   self.block_size, self.num_cycles, self.device_id, coarse_direct=self.coarse_direct)
        if field is not None:
            self._engine.set_coefficient(field)

    def solve(self, initial_vectors=None):
        if self._engine is None:
            raise ValueError("eigensolver not properly setup")
        m, shape = self.block_size, self.grid.shape
        if initial_vectors is None:
            x0 = np.random.default_rng(self.seed).standard_normal((m,) + tuple(shape))
        else:
            x0 = np.asarray(initial_vectors, dtype=np.float64)
            if x0.shape != (m,) + tuple(shape):
                raise ValueError(f"initial_vectors of shape {x0.shape}: expected {(m,) + tuple(shape)}")
        return self._engine.solve(x0, self.num_eigenpairs, self.tolerance, self.max_iterations)

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
