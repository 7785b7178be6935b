"""Time-dependent heat equation  du/dt = alpha Laplace(u) + f(x, y, t)  on top of the multigrid engine
(SURVEY.md section 8f rank 4).  Mirrors applications/heat_equation.py: TimeSteppingScheme, BoundaryType,
BoundaryCondition, HeatEquationConfig, HeatEquationSolver (same constructor, method names, result-dict keys and the
same order of operations inside every step), create_gaussian_initial_condition, create_time_dependent_boundary.

What differs, on purpose:
  * Implicit steps solve  (-Laplace_h + lambda) u = rhs'  (lambda = 1/(alpha dt) or 2/(alpha dt),
    heat_equation.py:209-220, 254-261) with multigrid V-cycles of the SHIFTED operator on the GPU (mg_set_shift).
    The reference builds a CorrectedMultigridSolver (:101-106) but never calls it: its _solve_helmholtz (:459-497)
    runs lexicographic Gauss-Seidel sweeps of the same linear system, and because the residual it tests carries a sign
    error (:474, `rhs - lap + lambda u` for `rhs + lap - lambda u`) the stop test never fires and every step costs
    exactly 100 sweeps.  Both iterate on the same equations from the same initial guess (u_old, boundary ring
    included), so the reference's result is ours up to ITS remaining iteration error (tests/golden/heat.npz).
  * The rhs ring is cleared before the solve: the interior equations never read it, but the engine's norm counts
    r = f on the ring and would never pass the tolerance otherwise.
  * The Laplacian of explicit / Crank-Nicolson steps is evaluated by the HIP residual kernel (same values as
    _compute_laplacian :430-442 up to rounding: a different association of the same five terms).
  * Source terms and boundary data are evaluated on whole coordinate arrays when the callable accepts them (the
    reference loops over points); scalar-only callables fall back to np.vectorize.
  * HeatEquationSolver(device_resident=True) keeps the state on the device between steps (heat_device.DeviceHeatStepper,
    DESIGN.md 5.2): uniform Dirichlet data and a SeparableSource only; it also runs TimeSteppingScheme.BDF2, which the
    reference names (:30) and never implements.
  * Device-resident only: conductivity= turns the equation into  du/dt = alpha div(a(x, y) grad u) + f  (transient conduction
    through a composite; the reference has no counterpart), and inner_solver="pcg" solves the implicit systems by conjugate
    gradients preconditioned with the multigrid cycle (inner_precision: the preconditioner's), which converges on jumping
    coefficients where the plain cycle stalls.
"""
import logging
import time
from dataclasses import dataclass
from enum import Enum
from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np

from . import _lib
from .engine import MultigridEngine
from .grid import Grid
from .operators import LaplacianOperator
from .precision import PrecisionManager

logger = logging.getLogger(__name__)


class TimeSteppingScheme(Enum):                                          # heat_equation.py:25-30
    EXPLICIT_EULER = "explicit_euler"
    IMPLICIT_EULER = "implicit_euler"
    CRANK_NICOLSON = "crank_nicolson"
    BDF2 = "bdf2"


class BoundaryType(Enum):                                                # heat_equation.py:33-38
    DIRICHLET = "dirichlet"
    NEUMANN = "neumann"
    ROBIN = "robin"
    PERIODIC = "periodic"


@dataclass
class BoundaryCondition:                                                 # heat_equation.py:41-53
    boundary_type: BoundaryType
    value: Optional[Callable[[float, float, float], float]] = None      # f(x, y, t)
    alpha: Optional[float] = None                                       # Robin: alpha u + beta du/dn = g
    beta: Optional[float] = None

    def evaluate(self, x, y, t):
        if self.value is None:
            return 0.0
        return self.value(x, y, t)


@dataclass
class HeatEquationConfig:                                                # heat_equation.py:56-72
    thermal_diffusivity: float = 1.0
    initial_condition: Callable[[float, float], float] = None
    source_term: Optional[Callable[[float, float, float], float]] = None
    boundary_conditions: Dict[str, BoundaryCondition] = None

    def __post_init__(self):
        if self.boundary_conditions is None:
            zero = lambda x, y, t: 0.0                                   # noqa: E731
            self.boundary_conditions = {k: BoundaryCondition(BoundaryType.DIRICHLET, zero)
                                        for k in ("left", "right", "bottom", "top")}


def _on_arrays(fn, *args):
    """fn evaluated on broadcast coordinate arrays; callables written for scalars go through np.vectorize."""
    shape = np.broadcast(*[np.asarray(a) for a in args]).shape
    try:
        out = np.asarray(fn(*args), dtype=np.float64)
        if out.shape == shape:
            return out
        if out.shape == ():
            return np.full(shape, float(out))
    except (TypeError, ValueError):        # written for scalars (math.sin(x), `if x < 0.5`, ...): evaluate point by point
        pass
    return np.asarray(np.vectorize(fn, otypes=[np.float64])(*args), dtype=np.float64).reshape(shape)


class SeparableSource:
    """A source term f(x, y, t) = profile(x, y) * factor(t).  A callable like any other source term (the host path evaluates
    it as one); the device-resident path uploads profile(x, y) once and passes factor(t) as a scalar per step."""

    def __init__(self, profile: Callable[[float, float], float], factor: Callable[[float], float]):
        self.profile = profile
        self.factor = factor

    def __call__(self, x, y, t):
        return self.profile(x, y) * self.factor(t)


class HeatEquationSolver:
    """du/dt = alpha Laplace(u) + f  (heat_equation.py:75-600), implicit steps by shifted multigrid on the GPU.
    device_resident=True also takes conductivity= (a callable a(x, y) or an (nx, ny) array: du/dt = alpha div(a grad u) + f),
    inner_solver="multigrid" | "pcg" and, for PCG, inner_precision="double" | "single_managed" | "mixed".  coarse_direct: as
    MultigridEngine's (None: the default, a direct coarsest solve)."""

    def __init__(self, config: HeatEquationConfig, grid: Grid, precision_manager: Optional[PrecisionManager] = None,
                 device_id: int = 0, max_levels: int = 32, smoother: str = "jacobi", device_resident: bool = False,
                 conductivity=None, inner_solver: str = "multigrid", inner_precision: str = "double", coarse_direct=None):
        self.config = config
        self.grid = grid
        self.precision_manager = precision_manager or PrecisionManager()
        if inner_solver not in ("multigrid", "pcg"):
            raise ValueError(f"inner_solver must be 'multigrid' or 'pcg', not {inner_solver!r}")
        self.device_resident = bool(device_resident)
        if not self.device_resident and (conductivity is not None or inner_solver == "pcg"):
            raise ValueError("conductivity= and inner_solver='pcg' need device_resident=True (the host path steps "
                             "du/dt = alpha Laplace(u) + f with the plain multigrid cycle)")
        self.inner_solver, self.inner_precision = inner_solver, inner_precision
        # heat_equation.py:101-106: max_iterations = 20, tolerance = 1e-10 (there for a solver that is never called); the
        # conjugate-gradient loop needs 28-35 iterations on jumping coefficients
        self.mg_max_iterations, self.mg_tolerance = (60 if inner_solver == "pcg" else 20), 1e-10
        if smoother == "line":           # zebra lines along the strongly coupled direction (smoothers.LineRelaxationSmoother)
            from .smoothers import line_kind
            sm, omega = line_kind(grid.hx, grid.hy), 1.0
        else:
            sm, omega = (_lib.MG_JACOBI, 0.8) if smoother == "jacobi" else (_lib.MG_RBGS, 1.0)
        self._x = np.linspace(grid.domain[0], grid.domain[1], grid.nx)   # heat_equation.py:134-135, 449-450, 501-502
        self._y = np.linspace(grid.domain[2], grid.domain[3], grid.ny)
        self.conductivity = None
        if conductivity is not None:
            a = (_on_arrays(conductivity, self._x[:, None], self._y[None, :]) if callable(conductivity)
                 else np.array(conductivity, dtype=np.float64))
            if a.shape != (grid.nx, grid.ny):
                raise ValueError(f"conductivity shape {a.shape} doesn't match grid shape {(grid.nx, grid.ny)}")
            if not np.all(np.isfinite(a)) or not np.all(a > 0):
                raise ValueError("conductivity must be finite and > 0 everywhere")
            self.conductivity = a
        if self.device_resident:
            self._check_device_resident_config()            # before any device call
            from .heat_device import DeviceHeatStepper
            self.stepper = DeviceHeatStepper(grid.nx, grid.ny, tuple(float(v) for v in grid.domain),
                                             config.thermal_diffusivity, max_levels, sm, omega, device=device_id,
                                             inner="pcg" if inner_solver == "pcg" else "cycle",
                                             precision=inner_precision if inner_solver == "pcg" else "double",
                                             coarse_direct=coarse_direct)
            self.mg_solver = None
            self._cur = 0                # slot of the current solution
            self._bdf_prev = None        # (slot of the level before it, the dt that led from there to _cur)
        else:
            self.mg_solver = MultigridEngine(grid.nx, grid.ny, tuple(float(v) for v in grid.domain), -1.0, max_levels, "V",
                                             2, 2, sm, omega, device=device_id, coarse_direct=coarse_direct)
        self.laplacian = LaplacianOperator(coefficient=1.0)
        self.current_time = 0.0
        self.current_solution = None
        self.solution_history, self.time_history, self.dt_history = [], [], []
        self.helmholtz_stats = []        # per implicit solve: (lambda, cycles, final ||r||)
        self.step_converged = []         # per implicit solve of the device-resident path: did it meet the tolerance?
        logger.info(f"Initialized HeatEquationSolver: alpha={config.thermal_diffusivity}")

    # -- initial condition (heat_equation.py:120-153) -----------------------------------------
    def set_initial_condition(self, u0: Optional[np.ndarray] = None) -> np.ndarray:
        if u0 is not None:
            self.current_solution = np.array(u0, dtype=np.float64)
        elif self.config.initial_condition is not None:
            self.current_solution = _on_arrays(self.config.initial_condition, self._x[:, None], self._y[None, :]).copy()
        else:
            self.current_solution = np.zeros((self.grid.nx, self.grid.ny))
        self._apply_boundary_conditions(self.current_solution, 0.0)
        self.current_time = 0.0
        self.solution_history = [self.current_solution.copy()]
        self.time_history = [0.0]
        if self.device_resident:         # the one upload of a run (and the source profile and the conductivity, once each)
            self._cur, self._bdf_prev = 0, None
            self.stepper.set_slot(0, self.current_solution)
            if self.conductivity is not None:
                self.stepper.set_coefficient(self.conductivity)
            src = self.config.source_term
            self.stepper.set_source(None if src is None else _on_arrays(src.profile, self._x[:, None], self._y[None, :]))
        return self.current_solution

    # -- single steps ---------------------------------------------------------------------
    def explicit_euler_step(self, u_old, dt):                            # heat_equation.py:155-185
        if self.device_resident:         # the same step on the stepper's slots (one upload, one download)
            return self._single_time_step(u_old, dt, TimeSteppingScheme.EXPLICIT_EULER)
        h_min = min(self.grid.hx, self.grid.hy)
        dt_stable = h_min**2 / (4 * self.config.thermal_diffusivity)
        if dt > dt_stable:
            logger.warning(f"Time step dt={dt:.2e} exceeds stability limit {dt_stable:.2e}")
        lap_u = self._compute_laplacian(u_old)
        source = self._evaluate_source_term(self.current_time)
        u_new = u_old + dt * (self.config.thermal_diffusivity * lap_u + source)
        self._apply_boundary_conditions(u_new, self.current_time + dt)
        return u_new

    def implicit_euler_step(self, u_old, dt):                            # heat_equation.py:187-225
        if self.device_resident:         # the same step on the stepper's slots (one upload, one download)
            return self._single_time_step(u_old, dt, TimeSteppingScheme.IMPLICIT_EULER)
        alpha = self.config.thermal_diffusivity
        source = self._evaluate_source_term(self.current_time + dt)
        rhs = u_old + dt * source
        self._apply_boundary_conditions_to_rhs(rhs, self.current_time + dt)
        lambda_coeff = 1.0 / (dt * alpha)
        mg_rhs = rhs / (dt * alpha)
        u_new = self._solve_helmholtz(mg_rhs, lambda_coeff, u_old)
        self._apply_boundary_conditions(u_new, self.current_time + dt)
        return u_new

    def crank_nicolson_step(self, u_old, dt):                            # heat_equation.py:227-266
        if self.device_resident:         # the same step on the stepper's slots (one upload, one download)
            return self._single_time_step(u_old, dt, TimeSteppingScheme.CRANK_NICOLSON)
        alpha = self.config.thermal_diffusivity
        lap_u_old = self._compute_laplacian(u_old)
        source_old = self._evaluate_source_term(self.current_time)
        source_new = self._evaluate_source_term(self.current_time + dt)
        rhs = u_old + dt * alpha * lap_u_old / 2 + dt * (source_old + source_new) / 2
        self._apply_boundary_conditions_to_rhs(rhs, self.current_time + dt)
        lambda_coeff = 2.0 / (dt * alpha)
        mg_rhs = 2.0 * rhs / (dt * alpha)
        u_new = self._solve_helmholtz(mg_rhs, lambda_coeff, u_old)
        self._apply_boundary_conditions(u_new, self.current_time + dt)
        return u_new

    def adaptive_time_stepping(self, u_old, dt_initial, error_tolerance=1e-4,
                               scheme=TimeSteppingScheme.CRANK_NICOLSON) -> Tuple[np.ndarray, float]:
        """Step doubling (heat_equation.py:268-330): one step of dt against two of dt/2, Richardson estimate."""
        if self.device_resident:
            self.stepper.set_slot(0, np.ascontiguousarray(u_old, dtype=np.float64))
            self._cur, self._bdf_prev = 0, None
            slot, dt = self._device_adaptive_step(dt_initial, error_tolerance, scheme)
            return self.stepper.get_slot(slot), dt
        dt = dt_initial
        max_iterations = 10
        safety_factor = 0.8
        u_full = u_old
        for _ in range(max_iterations):
            u_full = self._single_time_step(u_old, dt, scheme)
            u_half1 = self._single_time_step(u_old, dt / 2, scheme)
            u_half2 = self._single_time_step(u_half1, dt / 2, scheme)
            if scheme in (TimeSteppingScheme.EXPLICIT_EULER, TimeSteppingScheme.IMPLICIT_EULER):
                error_est = np.linalg.norm(u_half2 - u_full)
                order = 1
            else:
                error_est = np.linalg.norm(u_half2 - u_full) / 3.0
                order = 2
            if error_est < error_tolerance:
                return u_half2, dt
            dt = max(dt / 4, dt * safety_factor * (error_tolerance / error_est) ** (1 / (order + 1)))
        logger.warning(f"Adaptive time stepping failed to converge after {max_iterations} iterations")
        return u_full, dt

    # -- time loop (heat_equation.py:332-417) -----------------------------------------------
    def solve_time_dependent(self, t_final, dt_initial=None, scheme=TimeSteppingScheme.CRANK_NICOLSON, adaptive=True,
                             error_tolerance=1e-4, save_interval=1) -> Dict[str, Any]:
        if self.current_solution is None:
            raise ValueError("Initial condition not set. Call set_initial_condition() first.")
        if self.device_resident:
            return self._device_solve_time_dependent(t_final, dt_initial, scheme, adaptive, error_tolerance, save_interval)
        if dt_initial is None:
            h_min = min(self.grid.hx, self.grid.hy)
            if scheme == TimeSteppingScheme.EXPLICIT_EULER:
                dt_initial = 0.2 * h_min**2 / self.config.thermal_diffusivity
            else:
                dt_initial = 0.1 * h_min
        dt = dt_initial
        step_count = 0
        start_time = time.time()
        while self.current_time < t_final:
            if self.current_time + dt > t_final:
                dt = t_final - self.current_time
            if adaptive and scheme != TimeSteppingScheme.EXPLICIT_EULER:
                u_new, dt = self.adaptive_time_stepping(self.current_solution, dt, error_tolerance, scheme)
            else:
                u_new = self._single_time_step(self.current_solution, dt, scheme)
            self.current_solution = u_new
            self.current_time += dt
            step_count += 1
            if step_count % save_interval == 0:
                self.solution_history.append(u_new.copy())
                self.time_history.append(self.current_time)
                self.dt_history.append(dt)
        solve_time = time.time() - start_time
        return {"solution_history": self.solution_history, "time_history": self.time_history,
                "dt_history": self.dt_history, "final_solution": self.current_solution,
                "final_time": self.current_time, "total_steps": step_count, "solve_time": solve_time,
                "scheme": scheme.value, "adaptive": adaptive}

    def _single_time_step(self, u_old, dt, scheme):                      # heat_equation.py:419-428
        if self.device_resident:         # a host array in, a host array out: one upload, one step on slots, one download
            self.stepper.set_slot(0, np.ascontiguousarray(u_old, dtype=np.float64))
            self._cur, self._bdf_prev = 0, None
            self._device_step(0, 1, dt, scheme, self.current_time)
            return self.stepper.get_slot(1)
        if scheme == TimeSteppingScheme.EXPLICIT_EULER:
            return self.explicit_euler_step(u_old, dt)
        if scheme == TimeSteppingScheme.IMPLICIT_EULER:
            return self.implicit_euler_step(u_old, dt)
        if scheme == TimeSteppingScheme.CRANK_NICOLSON:
            return self.crank_nicolson_step(u_old, dt)
        raise ValueError(f"Unsupported time stepping scheme: {scheme}")

    # -- pieces ---------------------------------------------------------------------------
    def _compute_laplacian(self, u):                                     # heat_equation.py:430-442; boundary 0
        return self.laplacian.apply(self.grid, np.ascontiguousarray(u, dtype=np.float64))

    def _evaluate_source_term(self, t):                                  # heat_equation.py:444-457
        if self.config.source_term is None:
            return np.zeros((self.grid.nx, self.grid.ny))
        return _on_arrays(self.config.source_term, self._x[:, None], self._y[None, :], t)

    def _solve_helmholtz(self, rhs, lambda_coeff, initial_guess):        # replaces heat_equation.py:459-497
        """(-Laplace_h + lambda) u = rhs on the interior, boundary ring of u = that of initial_guess."""
        f = np.array(rhs, dtype=np.float64)
        f[0, :] = f[-1, :] = 0.0
        f[:, 0] = f[:, -1] = 0.0
        eng = self.mg_solver
        eng.set_shift(lambda_coeff)
        scale = max(1.0, float(np.sqrt(self.grid.hx * self.grid.hy * np.sum(f * f))))
        u, info = eng.solve(f, np.ascontiguousarray(initial_guess, dtype=np.float64), self.mg_tolerance * scale,
                            self.mg_max_iterations)
        self.helmholtz_stats.append((lambda_coeff, info["iterations"],
                                     info["residual_history"][-1] if info["iterations"] else info["initial_residual"]))
        return u

    def _edge(self, location):
        x, y = self._x, self._y
        return {"left": (np.s_[0, :], np.s_[1, :], x[0], y), "right": (np.s_[-1, :], np.s_[-2, :], x[-1], y),
                "bottom": (np.s_[:, 0], np.s_[:, 1], x, y[0]), "top": (np.s_[:, -1], np.s_[:, -2], x, y[-1])}[location]

    def _apply_boundary_conditions(self, u, t):                          # heat_equation.py:499-577, same order
        for location in ("left", "right", "bottom", "top"):
            bc = self.config.boundary_conditions.get(location)
            if bc:
                self._apply_single_boundary(u, bc, location, self._x, self._y, t)

    def _apply_single_boundary(self, u, bc, location, x, y, t):
        edge, inner, ex, ey = self._edge(location)
        if bc.boundary_type == BoundaryType.DIRICHLET:
            u[edge] = _on_arrays(bc.evaluate, ex, ey, t)
        elif bc.boundary_type == BoundaryType.NEUMANN:                   # one-sided: u_b = u_inner -/+ h g (:548-562)
            h = min(self.grid.hx, self.grid.hy)
            sign = -1.0 if location in ("left", "bottom") else 1.0
            u[edge] = u[inner] + sign * h * _on_arrays(bc.evaluate, ex, ey, t)
        elif bc.boundary_type == BoundaryType.ROBIN:                     # only 'left' exists in the reference (:570-577)
            if location == "left":
                h = min(self.grid.hx, self.grid.hy)
                g = _on_arrays(bc.evaluate, ex, ey, t)
                u[edge] = (g + bc.beta * u[inner] / h) / (bc.alpha + bc.beta / h)

    def _apply_boundary_conditions_to_rhs(self, rhs, t):                 # heat_equation.py:579-599
        for name, bc in self.config.boundary_conditions.items():
            if bc.boundary_type == BoundaryType.DIRICHLET and name in ("left", "right", "bottom", "top"):
                edge, _, ex, ey = self._edge(name)
                rhs[edge] = _on_arrays(bc.evaluate, ex, ey, t)


    # -- device-resident path: the state lives in the stepper's slots ------------------
    def _check_device_resident_config(self):
        for location in ("left", "right", "bottom", "top"):
            bc = self.config.boundary_conditions.get(location)
            if bc is None or bc.boundary_type != BoundaryType.DIRICHLET:
                raise ValueError(f"device_resident=True needs a Dirichlet condition on every edge ('{location}' is "
                                 f"{'missing' if bc is None else bc.boundary_type.value})")
        src = self.config.source_term
        if src is not None and not isinstance(src, SeparableSource):
            raise ValueError("device_resident=True needs source_term=None or a SeparableSource(profile, factor)")

    def _edge_values(self, t):
        """(left, right, bottom, top) at time t; each edge's Dirichlet value must be spatially uniform"""
        out = []
        for location in ("left", "right", "bottom", "top"):
            _, _, ex, ey = self._edge(location)
            v = _on_arrays(self.config.boundary_conditions[location].evaluate, ex, ey, t)
            if float(np.max(v)) != float(np.min(v)):
                raise ValueError(f"device_resident=True needs a spatially uniform Dirichlet value on the '{location}' edge")
            out.append(float(v.flat[0]))
        return tuple(out)

    def _device_step(self, src, dst, dt, scheme, t, prev=None):
        """one step from slot src at time t into slot dst (BDF2: prev is the slot of the level before src)"""
        if scheme == TimeSteppingScheme.EXPLICIT_EULER:
            h_min = min(self.grid.hx, self.grid.hy)
            a_max = 1.0 if self.conductivity is None else float(np.max(self.conductivity))
            dt_stable = h_min**2 / (4 * self.config.thermal_diffusivity * a_max)
            if dt > dt_stable:
                logger.warning(f"Time step dt={dt:.2e} exceeds stability limit {dt_stable:.2e}")
        elif scheme not in (TimeSteppingScheme.IMPLICIT_EULER, TimeSteppingScheme.CRANK_NICOLSON, TimeSteppingScheme.BDF2):
            raise ValueError(f"Unsupported time stepping scheme: {scheme}")
        if scheme == TimeSteppingScheme.BDF2 and prev is None:
            scheme = TimeSteppingScheme.CRANK_NICOLSON       # the start: self-starting and second order
        factor = self.config.source_term.factor if self.config.source_term is not None else (lambda t: 0.0)
        info = self.stepper.step(scheme, dt, src, dst, prev if scheme == TimeSteppingScheme.BDF2 else None,
                                 float(factor(t)), float(factor(t + dt)), self._edge_values(t + dt), False,
                                 self.mg_tolerance, self.mg_max_iterations)
        if scheme != TimeSteppingScheme.EXPLICIT_EULER:
            self.helmholtz_stats.append((info["lambda"], info["cycles"], info["final_residual"]))
            self.step_converged.append(info["converged"])
        return info

    def _free_slots(self, *used):
        return [k for k in range(4) if k not in used]

    def _device_adaptive_step(self, dt_initial, error_tolerance, scheme):
        """step doubling on slots: old / full / half1 / half2, the error from diff_norm; returns (slot, dt)"""
        if scheme == TimeSteppingScheme.BDF2:
            raise ValueError("adaptive=True is not available with BDF2 (a multistep scheme needs a constant dt)")
        old = self._cur
        full, half1, half2 = self._free_slots(old)
        dt, t = dt_initial, self.current_time
        for _ in range(10):
            self._device_step(old, full, dt, scheme, t)
            self._device_step(old, half1, dt / 2, scheme, t)
            self._device_step(half1, half2, dt / 2, scheme, t)       # the reference's clock stands still inside an attempt (:298-300)
            if scheme in (TimeSteppingScheme.EXPLICIT_EULER, TimeSteppingScheme.IMPLICIT_EULER):
                error_est = self.stepper.diff_norm(half2, full)
                order = 1
            else:
                error_est = self.stepper.diff_norm(half2, full) / 3.0
                order = 2
            if error_est < error_tolerance:
                return half2, dt
            dt = max(dt / 4, dt * 0.8 * (error_tolerance / error_est) ** (1 / (order + 1)))
        logger.warning("Adaptive time stepping failed to converge after 10 iterations")
        return full, dt

    def _device_solve_time_dependent(self, t_final, dt_initial, scheme, adaptive, error_tolerance, save_interval):
        if adaptive and scheme == TimeSteppingScheme.BDF2:
            raise ValueError("adaptive=True is not available with BDF2 (a multistep scheme needs a constant dt)")
        if dt_initial is None:
            h_min = min(self.grid.hx, self.grid.hy)
            if scheme == TimeSteppingScheme.EXPLICIT_EULER:
                dt_initial = 0.2 * h_min**2 / self.config.thermal_diffusivity
                if self.conductivity is not None:
                    dt_initial /= float(np.max(self.conductivity))
            else:
                dt_initial = 0.1 * h_min
        dt = dt_initial
        step_count = 0
        start_time = time.time()
        while self.current_time < t_final:
            if self.current_time + dt > t_final:
                dt = t_final - self.current_time
            if adaptive and scheme != TimeSteppingScheme.EXPLICIT_EULER:
                new, dt = self._device_adaptive_step(dt, error_tolerance, scheme)
                self._bdf_prev = None
            else:
                prev = self._bdf_prev[0] if self._bdf_prev is not None and self._bdf_prev[1] == dt else None
                new = self._free_slots(self._cur, prev)[0]
                self._device_step(self._cur, new, dt, scheme, self.current_time, prev)
                self._bdf_prev = (self._cur, dt)
            self._cur = new
            self.current_time += dt
            step_count += 1
            if step_count % save_interval == 0:
                self.solution_history.append(self.stepper.get_slot(self._cur))
                self.time_history.append(self.current_time)
                self.dt_history.append(dt)
        self.current_solution = self.stepper.get_slot(self._cur)
        solve_time = time.time() - start_time
        return {"solution_history": self.solution_history, "time_history": self.time_history,
                "dt_history": self.dt_history, "final_solution": self.current_solution,
                "final_time": self.current_time, "total_steps": step_count, "solve_time": solve_time,
                "scheme": scheme.value, "adaptive": adaptive}


def create_gaussian_initial_condition(center=(0.5, 0.5), width=0.1, amplitude=1.0):    # heat_equation.py:602-610
    def gaussian(x, y):
        dx = x - center[0]
        dy = y - center[1]
        return amplitude * np.exp(-(dx**2 + dy**2) / (2 * width**2))
    return gaussian


def create_time_dependent_boundary(amplitude=1.0, frequency=1.0):                      # heat_equation.py:613-618
    def time_varying(x, y, t):
        return amplitude * np.sin(2 * np.pi * frequency * t)
    return time_varying
