"""Thin object wrapper of one mg_heat (include/mghip.h, "Time stepping"; include/mghip_heat.h): heat-equation steps whose state stays on the device.

Four state slots (0..3); a step reads one slot (two for BDF2) and writes another.  Fields cross to the host only through
set_slot / get_slot / set_source / set_coefficient, which the object counts (`uploads`, `downloads`, `source_uploads`,
`coefficient_uploads`)."""
import ctypes as C

import numpy as np

from . import _lib

SCHEMES = {"explicit_euler": _lib.MG_HEAT_EXPLICIT_EULER, "implicit_euler": _lib.MG_HEAT_IMPLICIT_EULER,
           "crank_nicolson": _lib.MG_HEAT_CRANK_NICOLSON, "bdf2": _lib.MG_HEAT_BDF2}
NUM_SLOTS = 4
INNER = {"cycle": _lib.MG_HEAT_INNER_CYCLE, "pcg": _lib.MG_HEAT_INNER_PCG}
# the preconditioner's precision of the PCG inner solver (krylov.PRECISIONS); the state and the Krylov vectors are fp64
PRECISIONS = {"double": _lib.MG_PREC_DOUBLE, "single_managed": _lib.MG_PREC_SINGLE_MANAGED, "mixed": _lib.MG_PREC_MIXED_LEVELS}


def scheme_code(scheme):
    """mg_heat_scheme of a name, a TimeSteppingScheme (its value is the name) or a code"""
    name = getattr(scheme, "value", scheme)
    if isinstance(name, str):
        if name not in SCHEMES:
            raise ValueError(f"Unsupported time stepping scheme: {scheme}")
        return SCHEMES[name]
    return int(name)


class DeviceHeatStepper:
    """Owns an mg_heat: the inner solver of (-div(a grad) + lambda) u = f, the slots, the right-hand side, the source and
    the diffusivity field.  inner="cycle": the plain multigrid cycle on an fp64 engine; inner="pcg": conjugate gradients
    preconditioned by `num_cycles` cycles in `precision` ("double", "single_managed", "mixed"; the loop itself is fp64),
    flexible as in PCGEngine (None: auto)."""

    def __init__(self, nx, ny, domain=(0.0, 1.0, 0.0, 1.0), alpha=1.0, max_levels=32, smoother=_lib.MG_JACOBI, omega=0.8,
                 device=0, cycle="V", pre=2, post=2, coarse_tol=1e-12, coarse_maxit=1000, fused=2, tail=True, speculate=True,
                 coarse_direct=None, inner="cycle", precision="double", num_cycles=1, flexible=None):
        from .engine import _direct_code
        if inner not in INNER:                                   # before any device call
            raise ValueError(f"inner must be one of {sorted(INNER)}, not {inner!r}")
        if precision not in PRECISIONS or (inner == "cycle" and precision != "double"):
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)} with inner='pcg' (the preconditioner's) and "
                             f"'double' with inner='cycle', not {precision!r}")
        lib = _lib.load()
        if isinstance(cycle, str):
            if cycle not in _lib.CYCLES:
                raise ValueError(f"unknown cycle type {cycle!r}")
            cycle = _lib.CYCLES[cycle]
        if isinstance(smoother, str):
            from .smoothers import line_kind
            hx, hy = (domain[1] - domain[0]) / (nx - 1), (domain[3] - domain[2]) / (ny - 1)
            smoother = {"jacobi": _lib.MG_JACOBI, "rbgs": _lib.MG_RBGS, "line": line_kind(hx, hy)}[smoother]
        cfg = _lib.MgConfig(int(nx), int(ny), float(domain[0]), float(domain[1]), float(domain[2]), float(domain[3]),
                            -1.0, int(max_levels), int(cycle), int(pre), int(post), int(smoother), float(omega),
                            float(coarse_tol), int(coarse_maxit), PRECISIONS[precision], 1e-6, 4.0, 0, int(device), 0, 0,
                            int(fused), int(tail), 0, (2 if speculate is True else int(speculate)), _direct_code(coarse_direct), 0)
        self.cfg = cfg
        self._h = C.c_void_p(None)
        self._lib = lib
        _lib.check(lib.mg_heat_create_ex(C.byref(cfg), float(alpha), INNER[inner], int(num_cycles),
                                         -1 if flexible is None else int(bool(flexible)), C.byref(self._h)))
        self.nx, self.ny, self.alpha = int(nx), int(ny), float(alpha)
        self.inner, self.precision = inner, precision
        self.uploads = 0          # set_slot calls
        self.downloads = 0        # get_slot calls
        self.source_uploads = 0
        self.coefficient_uploads = 0

    def _check(self, rc):
        if rc == _lib.MG_OK:
            return
        msg = self._lib.mg_heat_last_error(self._h)
        msg = (msg.decode() if msg else "") or f"mghip error {rc}"
        if rc in (_lib.MG_ERR_INVALID_VALUE, _lib.MG_ERR_STATE):
            raise ValueError(msg)
        if rc == _lib.MG_ERR_ALLOC:
            raise MemoryError(msg)
        raise RuntimeError("mghip: " + msg)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mg_heat_destroy(self._h)
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

    def _field(self, a):
        a = _lib.as_c(a)
        if a.shape != (self.nx, self.ny):
            raise ValueError(f"field shape {a.shape} doesn't match grid shape {(self.nx, self.ny)}")
        return a

    def set_slot(self, slot, u):
        u = self._field(u)
        self._check(self._lib.mg_heat_set_slot(self._h, int(slot), _lib.ptr(u), _lib.dtype_code(u.dtype)))
        self.uploads += 1

    def get_slot(self, slot, dtype=np.float64):
        out = np.empty((self.nx, self.ny), dtype=dtype)
        self._check(self._lib.mg_heat_get_slot(self._h, int(slot), _lib.ptr(out), _lib.dtype_code(dtype)))
        self.downloads += 1
        return out

    @staticmethod
    def _dev_args(t):
        return C.c_void_p(t.data_ptr()), int(t.stride(0)), _lib.dtype_code(str(t.dtype).split(".")[-1])

    def set_slot_device(self, slot, t):
        """a 2-D device tensor (nx, ld) whose first ny columns are the field -> slot (no host transfer)"""
        p, ld, dt = self._dev_args(t)
        self._check(self._lib.mg_heat_set_slot_device(self._h, int(slot), p, ld, dt))

    def get_slot_device(self, slot, t):
        p, ld, dt = self._dev_args(t)
        self._check(self._lib.mg_heat_get_slot_device(self._h, int(slot), p, ld, dt))

    def set_source(self, profile):
        """the static source profile S(x, y) on the grid (None: no source)"""
        if profile is None:
            self._check(self._lib.mg_heat_set_source(self._h, None, _lib.MG_F64))
            return
        p = self._field(profile)
        self._check(self._lib.mg_heat_set_source(self._h, _lib.ptr(p), _lib.dtype_code(p.dtype)))
        self.source_uploads += 1

    def set_coefficient(self, a):
        """the diffusivity field a(x, y) > 0 on the grid: du/dt = alpha div(a grad u) + g S (None: back to a == 1)"""
        if a is None:
            self._check(self._lib.mg_heat_set_coefficient(self._h, None, _lib.MG_F64))
            return
        a = self._field(a)
        self._check(self._lib.mg_heat_set_coefficient(self._h, _lib.ptr(a), _lib.dtype_code(a.dtype)))
        self.coefficient_uploads += 1

    def step(self, scheme, dt, src, dst, prev=None, g0=1.0, g1=1.0, edges=None, bc_before_solve=False, tol=1e-10, max_cycles=20):
        """One step from slot `src` (and `prev` for BDF2) into slot `dst`; edges = (left, right, bottom, top) at t + dt or None.
        Returns the step info (mg_heat_step_info)."""
        e4 = None if edges is None else (C.c_double * 4)(*[float(v) for v in edges])
        info = _lib.MgHeatStepInfo()
        self._check(self._lib.mg_heat_step(self._h, scheme_code(scheme), float(dt), int(src), -1 if prev is None else int(prev),
                                           int(dst), float(g0), float(g1), e4, int(bool(bc_before_solve)), float(tol),
                                           int(max_cycles), C.byref(info)))
        return {"lambda": getattr(info, "lambda"), "rhs_norm": info.rhs_norm, "initial_residual": info.initial_residual,
                "final_residual": info.final_residual, "solve_seconds": info.solve_seconds, "cycles": info.cycles,
                "converged": bool(info.converged)}

    def diff_norm(self, a, b):
        """sqrt(sum (slot a - slot b)^2) over all cells: np.linalg.norm of the difference, taken on the device"""
        out = C.c_double(0.0)
        self._check(self._lib.mg_heat_diff_norm(self._h, int(a), int(b), C.byref(out)))
        return out.value
