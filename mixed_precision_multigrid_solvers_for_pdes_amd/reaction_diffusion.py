"""Reaction-diffusion equations with the state resident on the device (include/mghip_rd.h, csrc/mg_rd.hip):

    u_t = alpha div(a grad u) - strength * weight * phi(u) + linear_growth * u + g(t) S(x, y),    Dirichlet data on the ring.

phi is "linear" (u), "cubic" (u^3), "sinh" or "exp": monotone, taken implicitly -- every step is one Newton - conjugate
gradients - multigrid solve (nonlinear.py) on the device.  linear_growth (any sign) is taken explicitly, extrapolated from the
old time levels: Allen-Cahn u_t = eps^2 lap u + u - u^3 is nonlinearity="cubic", strength=1, linear_growth=1 (convex
splitting; implicit Euler then decreases the free energy for every dt).  Schemes: "implicit_euler" (order 1), "crank_nicolson"
(CN-AB2, order 2), "bdf2" (SBDF2, order 2, started with one Crank-Nicolson step).  Fields cross to the host only through
set_state, `state` and the constructor's fields; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib
from .heat_equation import SeparableSource, _on_arrays
from .krylov import PRECISIONS
from .nonlinear import _checked_weight
from .smoothers import GaussSeidelSmoother, IterativeSolver

SCHEMES = _lib.RD_SCHEMES
EDGES = ("left", "right", "bottom", "top")


def _edge_values(boundary):
    """None, four values or {"left": ..} -> None or (left, right, bottom, top), in the heat stepper's order"""
    if boundary is None:
        return None
    if isinstance(boundary, dict):
        unknown = set(boundary) - set(EDGES)
        if unknown:
            raise ValueError(f"unknown edge {sorted(unknown)}: boundary has the keys {EDGES}")
        out = tuple(float(boundary.get(k, 0.0)) for k in EDGES)
    else:
        out = tuple(float(v) for v in boundary)
        if len(out) != 4:
            raise ValueError("boundary is a dict or four values (left, right, bottom, top)")
    if not all(np.isfinite(out)):
        raise ValueError("boundary values must be finite")
    return out


class ReactionDiffusionSolver:
    """One mg_rd on a Grid.  tolerance: every step's Newton solve stops at ||F||_h < tolerance * max(1, ||f||_h); precision is
    the PRECONDITIONER's ("double", "single_managed", "mixed"; the state is fp64).  source: a SeparableSource(profile, factor),
    or an (nx, ny) array (a steady source, g == 1).  conductivity: an (nx, ny) array or a callable a(x, y) > 0.  weight >= 0.
    step() returns the info dict of mg_rd_step_info; energy() the discrete free energy and its three sums.  coarse_direct: as
    MultigridEngine's (None: the default, the coarsest grid of the preconditioner's cycle is solved directly)."""

    def __init__(self, grid, diffusivity, nonlinearity="cubic", strength=1.0, weight=None, linear_growth=0.0, conductivity=None,
                 source=None, scheme="bdf2", max_levels=None, tolerance=1e-8, precision="double", smoother=None, max_newton=30,
                 forcing="eisenstat_walker", coarse_direct=None):
        from .engine import _direct_code
        from .facade import default_max_levels
        # every refusal below happens before the library loads
        self.nx, self.ny = int(grid.nx), int(grid.ny)
        shape = (self.nx, self.ny)
        diffusivity = float(diffusivity)
        if not (np.isfinite(diffusivity) and diffusivity > 0.0):
            raise ValueError("diffusivity must be finite and > 0")
        if nonlinearity not in _lib.NL_KINDS:
            raise ValueError(f"nonlinearity must be one of {sorted(_lib.NL_KINDS)}, not {nonlinearity!r}")
        strength = float(strength)
        if not (strength >= 0.0) or not np.isfinite(strength):
            raise ValueError("strength must be finite and >= 0 (the implicit term is monotone; linear_growth carries a term of "
                             "the other sign explicitly)")
        linear_growth = float(linear_growth)
        if not np.isfinite(linear_growth):
            raise ValueError("linear_growth must be finite")
        if scheme not in SCHEMES:
            raise ValueError(f"scheme must be one of {sorted(SCHEMES)}, not {scheme!r}")
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)} (the preconditioner's; the state is fp64), not {precision!r}")
        if forcing not in _lib.NL_FORCINGS:
            raise ValueError(f"forcing must be one of {sorted(_lib.NL_FORCINGS)}, not {forcing!r}")
        if int(max_newton) < 1:
            raise ValueError("max_newton must be >= 1")
        tolerance = float(tolerance)
        if not (tolerance >= 0.0):
            raise ValueError("tolerance must be >= 0")
        w = _checked_weight(weight)
        if w is not None and w.shape != shape:
            raise ValueError(f"weight shape {w.shape} doesn't match grid shape {shape}")
        a = None
        if conductivity is not None:
            a = _on_arrays(conductivity, grid.X, grid.Y) if callable(conductivity) else np.ascontiguousarray(conductivity, dtype=np.float64)
            if a.shape != shape:
                raise ValueError(f"conductivity shape {a.shape} doesn't match grid shape {shape}")
            if not np.all(np.isfinite(a)) or np.any(a <= 0):
                raise ValueError("conductivity must be finite and > 0 everywhere")
            a = np.ascontiguousarray(a, dtype=np.float64)
        profile, self._factor = None, None
        if isinstance(source, SeparableSource):
            profile, self._factor = _on_arrays(source.profile, grid.X, grid.Y), source.factor
        elif source is not None:
            if callable(source):
                raise ValueError("source must be a SeparableSource(profile, factor) or an (nx, ny) array")
            profile = np.ascontiguousarray(source, dtype=np.float64)
        if profile is not None:
            if profile.shape != shape:
                raise ValueError(f"source shape {profile.shape} doesn't match grid shape {shape}")
            if not np.all(np.isfinite(profile)):
                raise ValueError("source must be finite")
            profile = np.ascontiguousarray(profile, dtype=np.float64)
        if smoother is None:
            smoother = GaussSeidelSmoother(red_black=True)
        if not isinstance(smoother, IterativeSolver) or smoother.kind not in (_lib.MG_JACOBI, _lib.MG_RBGS):
            raise ValueError("smoother must be a JacobiSmoother or a red-black GaussSeidelSmoother (the preconditioner's)")

        self.grid = grid
        self.hx, self.hy = float(grid.hx), float(grid.hy)
        self.diffusivity, self.nonlinearity, self.strength, self.linear_growth = diffusivity, nonlinearity, strength, linear_growth
        self.scheme, self.tolerance, self.max_newton, self.precision = scheme, tolerance, int(max_newton), precision
        levels = default_max_levels(self.nx, self.ny) if max_levels is None else int(max_levels)
        d = grid.domain
        lib = _lib.load()
        cfg = _lib.MgConfig(self.nx, self.ny, float(d[0]), float(d[1]), float(d[2]), float(d[3]), -1.0, levels, _lib.MG_CYCLE_V, 2, 2,
                            int(smoother.kind), float(smoother.omega), 1e-12, 1000, PRECISIONS[precision], 1e-6, 4.0, 0, 0, 0, 0, 2,
                            1, 0, 2, _direct_code(coarse_direct), 0)
        self.cfg = cfg
        self._lib = lib
        self._h = C.c_void_p(None)
        _lib.check(lib.mg_rd_create(C.byref(cfg), diffusivity, 1, -1, C.byref(self._h)))
        try:
            if a is not None:
                self._check(lib.mg_rd_set_coefficient(self._h, _lib.ptr(a), _lib.MG_F64))
            if profile is not None:
                self._check(lib.mg_rd_set_source(self._h, _lib.ptr(profile), _lib.MG_F64))
            self._check(lib.mg_rd_set_reaction(self._h, _lib.NL_KINDS[nonlinearity], strength, None if w is None else _lib.ptr(w),
                                               _lib.MG_F64, linear_growth))
            opt = _lib.MgNlOptions()
            self._check(lib.mg_nl_options_default(C.byref(opt)))
            opt.forcing = _lib.NL_FORCINGS[forcing]
            self._check(lib.mg_rd_set_newton_options(self._h, C.byref(opt)))
        except Exception:
            self.close()
            raise
        self.time, self.steps = 0.0, 0
        self._cur, self._prev = 0, -1          # the slot of u^n and of u^{n-1} (-1: none yet)
        self._prev_dt = None
        self.history = []                      # (dt, newton iterations, inner iterations, converged) per step

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc == _lib.MG_OK:
            return
        msg = self._lib.mg_rd_last_error(self._h)
        msg = (msg.decode() if msg else "") or f"mghip error {rc}"
        if rc in (_lib.MG_ERR_INVALID_VALUE, _lib.MG_ERR_STATE):
            raise ValueError(msg)
        if rc == _lib.MG_ERR_ALLOC:
            raise MemoryError(msg)
        raise RuntimeError("mghip: " + msg)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mg_rd_destroy(self._h)
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

    @staticmethod
    def _dev_args(t):
        return C.c_void_p(t.data_ptr()), int(t.stride(0)), _lib.dtype_code(str(t.dtype).split(".")[-1])

    def get_device(self, t):
        """the current state -> the 2-D device tensor t (nx, ld), no host transfer"""
        p, ld, dt = self._dev_args(t)
        self._check(self._lib.mg_rd_get_slot_device(self._h, self._cur, p, ld, dt))

    def set_device(self, t):
        """the first ny columns of the 2-D device tensor t -> the current state; the multistep history restarts"""
        p, ld, dt = self._dev_args(t)
        self._check(self._lib.mg_rd_set_slot_device(self._h, self._cur, p, ld, dt))
        self._prev, self._prev_dt = -1, None

    # ------------------------------------------------------------------ state
    def set_state(self, u0):
        """u := u0 (its ring is the Dirichlet data); the multistep history and the clock restart"""
        u = _lib.as_c(u0)
        if u.shape != (self.nx, self.ny):
            raise ValueError(f"state shape {u.shape} doesn't match grid shape {(self.nx, self.ny)}")
        self._cur, self._prev, self._prev_dt = 0, -1, None
        self._check(self._lib.mg_rd_set_slot(self._h, 0, _lib.ptr(u), _lib.dtype_code(u.dtype)))
        self.time, self.steps, self.history = 0.0, 0, []

    @property
    def state(self):
        out = np.empty((self.nx, self.ny))
        self._check(self._lib.mg_rd_get_slot(self._h, self._cur, _lib.ptr(out), _lib.MG_F64))
        return out

    def _g(self, t):
        if self._factor is None:
            return 1.0
        return float(self._factor(t))

    # ------------------------------------------------------------------ stepping
    def step(self, dt, boundary=None):
        """One step of self.scheme from the current state; boundary = the Dirichlet values of t + dt (None: the ring stays).
        BDF2 needs the previous level at the same dt: the first step after set_state, and a step whose dt differs from the one
        before it, is Crank-Nicolson."""
        dt = float(dt)
        edge = _edge_values(boundary)
        scheme = SCHEMES[self.scheme]
        if scheme == _lib.MG_HEAT_BDF2 and (self._prev < 0 or self._prev_dt != dt):
            scheme = _lib.MG_HEAT_CRANK_NICOLSON
            prev = -1
        elif scheme == _lib.MG_HEAT_IMPLICIT_EULER:
            prev = -1
        else:
            prev = self._prev if self._prev_dt == dt else -1
        dst = next(k for k in range(4) if k not in (self._cur, self._prev))
        info = _lib.MgRdStepInfo()
        self._check(self._lib.mg_rd_step(self._h, scheme, dt, self._cur, prev, dst, self._g(self.time), self._g(self.time + dt),
                                         None if edge is None else (C.c_double * 4)(*edge), self.tolerance, self.max_newton,
                                         C.byref(info)))
        self._prev, self._cur, self._prev_dt = self._cur, dst, dt
        self.time += dt
        self.steps += 1
        d = {"lambda": getattr(info, "lambda"), "rhs_norm": info.rhs_norm, "initial_residual": info.initial_residual,
             "final_residual": info.final_residual, "solve_seconds": info.solve_seconds,
             "newton_iterations": info.newton_iterations, "inner_iterations": info.inner_iterations,
             "evaluations": info.evaluations, "status": _lib.NL_STATUS.get(info.status, info.status),
             "converged": bool(info.converged), "scheme": {v: k for k, v in SCHEMES.items()}[scheme]}
        self.history.append((dt, d["newton_iterations"], d["inner_iterations"], d["converged"]))
        return d

    def advance(self, t_final, dt, save_interval=None):
        """Fixed-dt steps until self.time reaches t_final (the last one is cut to end there).  Returns (times, states): the
        initial state, every save_interval-th step's and the final one (save_interval None: the initial and the final state).
        RuntimeError at the first step whose Newton solve does not converge."""
        dt = float(dt)
        if not (dt > 0.0 and np.isfinite(dt)):
            raise ValueError("dt must be finite and > 0")
        if save_interval is not None and int(save_interval) < 1:
            raise ValueError("save_interval must be >= 1")
        times, states = [self.time], [self.state]
        n = 0
        while t_final - self.time > 1e-12 * max(1.0, abs(t_final)):
            left = t_final - self.time
            last = dt >= left * (1.0 - 1e-12)
            info = self.step(left if last and abs(left - dt) > 1e-9 * dt else dt)      # a cut step differs from dt: BDF2 restarts
            n += 1
            if last:
                self.time = float(t_final)
            if not info["converged"]:
                raise RuntimeError(f"reaction-diffusion step {self.steps} (t = {self.time:g}) did not converge: Newton status "
                                   f"{info['status']!r}, residual {info['final_residual']:.3e}")
            if last or (save_interval is not None and n % int(save_interval) == 0):
                times.append(self.time)
                states.append(self.state)
        return np.array(times), states

    def energy(self):
        """E = alpha G + hx hy (strength P - linear_growth Q / 2) of the current state, summed on the device"""
        out = (C.c_double * 4)()
        self._check(self._lib.mg_rd_energy(self._h, self._cur, out))
        return {"gradient": out[0], "potential": out[1], "sum_squares": out[2], "energy": out[3], "time": self.time}
