"""2-D incompressible flow in the vorticity / stream-function form, state resident on the device (include/mghip_flow.h,
csrc/mg_flow.hip):  w_t = J(psi, w) + nu lap w + F,  -lap psi = w,  u = psi_y, v = -psi_x,  psi = 0 on the walls.

Crank-Nicolson for the diffusion, variable-step Adams-Bashforth 2 for the Arakawa Jacobian and the forcing; every step is one
shifted solve for w and one warm-started Poisson solve for psi on the multigrid engine.  At no-slip walls the wall vorticity
(Thom's formula) lags by one step, which is first order in dt there.  Fields cross to the host only through set_vorticity,
set_forcing and the `vorticity` / `stream_function` / `velocity` accessors; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _lib

WALLS = {"free_slip": _lib.MG_FLOW_FREE_SLIP, "no_slip": _lib.MG_FLOW_NO_SLIP}
WALL_SIDES = ("left", "right", "bottom", "top")      # the tangential speeds: v on left / right, u on bottom / top
FIELDS = {"omega": _lib.MG_FLOW_OMEGA, "psi": _lib.MG_FLOW_PSI, "N": _lib.MG_FLOW_N}


def wall_speed_array(wall_speeds):
    """{"top": 1.0, ...} (or a sequence of four) -> (left v, right v, bottom u, top u)"""
    if wall_speeds is None:
        return (0.0, 0.0, 0.0, 0.0)
    if isinstance(wall_speeds, dict):
        unknown = set(wall_speeds) - set(WALL_SIDES)
        if unknown:
            raise ValueError(f"unknown wall {sorted(unknown)}: wall_speeds has the keys {WALL_SIDES}")
        out = tuple(float(wall_speeds.get(k, 0.0)) for k in WALL_SIDES)
    else:
        out = tuple(float(v) for v in wall_speeds)
        if len(out) != 4:
            raise ValueError("wall_speeds is a dict or four values (left, right, bottom, top)")
    if not all(np.isfinite(out)):
        raise ValueError("wall speeds must be finite")
    return out


def _info_dict(info, with_omega=True):
    d = {"psi_rhs_norm": info.psi_rhs_norm, "psi_initial_residual": info.psi_initial_residual,
         "psi_final_residual": info.psi_final_residual, "psi_cycles": info.psi_cycles,
         "psi_converged": bool(info.psi_converged), "seconds": info.seconds}
    if with_omega:
        d.update({"sigma": info.sigma, "lambda": info.sigma, "c0": info.c0, "c1": info.c1, "cfl": info.cfl,
                  "rhs_norm": info.rhs_norm, "initial_residual": info.omega_initial_residual,
                  "final_residual": info.omega_final_residual, "cycles": info.omega_cycles,
                  "converged": bool(info.omega_converged) and bool(info.psi_converged),
                  "omega_converged": bool(info.omega_converged), "omega_cycles": info.omega_cycles,
                  "omega_change": info.omega_change, "solve_seconds": info.seconds})
    return d


class VorticityStreamSolver:
    """Lid-driven cavities and forced box flows on a Grid.

    wall: "no_slip" (Thom's wall vorticity with `wall_speeds`, e.g. {"top": 1.0} for the lid-driven cavity) or "free_slip"
    (w = 0 on the walls).  forcing: F(x, y) on the grid, the curl of a body force (None: none).  tolerance / max_cycles:
    every solve stops at ||r|| < tolerance * max(1, ||f||_h).  The info dict of a step carries the heat stepper's keys for the
    vorticity solve (lambda = sigma = 2/(nu dt), rhs_norm, initial_residual, final_residual, cycles, converged,
    solve_seconds) and psi_* for the stream-function solve, c0, c1, cfl and omega_change = max |w_new - w|.

    Non-finite states: the device maxima propagate NaN, so a step on a state that holds a NaN or an Inf still returns (MG_OK)
    and its cfl, omega_change, norms and residuals are non-finite wherever the field is; no solve of such a step reports
    convergence.  run_to_steady stops at the first step whose omega_change or cfl is not finite and returns converged False,
    diverged True; advance(dt=None) raises FloatingPointError when the velocity maximum is not finite (ValueError when it
    is 0: the fluid is at rest).  set_vorticity with a finite field makes the stepper usable again."""

    def __init__(self, grid, viscosity, wall="no_slip", wall_speeds=None, forcing=None, max_levels=None, tolerance=1e-10,
                 max_cycles=50, cycle="V", pre=2, post=2, smoother="jacobi", omega=0.8, coarse_tol=1e-12, coarse_maxit=1000,
                 coarse_direct=None, device=0):
        from .engine import _direct_code
        from .facade import default_max_levels
        if wall not in WALLS:                                    # before any device call
            raise ValueError(f"wall must be one of {sorted(WALLS)}, not {wall!r}")
        if not (np.isfinite(viscosity) and viscosity > 0.0):
            raise ValueError("viscosity must be finite and > 0")
        speeds = wall_speed_array(wall_speeds)
        if isinstance(cycle, str):
            if cycle not in _lib.CYCLES:
                raise ValueError(f"unknown cycle type {cycle!r}")
            cycle = _lib.CYCLES[cycle]
        if isinstance(smoother, str):
            if smoother not in ("jacobi", "rbgs"):
                raise ValueError(f"smoother must be 'jacobi' or 'rbgs', not {smoother!r}")
            smoother = {"jacobi": _lib.MG_JACOBI, "rbgs": _lib.MG_RBGS}[smoother]
        self.grid = grid
        self.nx, self.ny = int(grid.nx), int(grid.ny)
        self.hx, self.hy = float(grid.hx), float(grid.hy)
        self.viscosity = float(viscosity)
        self.wall, self.wall_speeds = wall, speeds
        self.tolerance, self.max_cycles = float(tolerance), int(max_cycles)
        levels = default_max_levels(self.nx, self.ny) if max_levels is None else int(max_levels)
        d = grid.domain
        lib = _lib.load()
        cfg = _lib.MgConfig(self.nx, self.ny, float(d[0]), float(d[1]), float(d[2]), float(d[3]), -1.0, levels, int(cycle),
                            int(pre), int(post), int(smoother), float(omega), float(coarse_tol), int(coarse_maxit),
                            _lib.MG_PREC_DOUBLE, 1e-6, 4.0, 0, int(device), 0, 0, 2, 1, 0, 2, _direct_code(coarse_direct), 0)
        self.cfg = cfg
        self._lib = lib
        self._h = C.c_void_p(None)
        _lib.check(lib.mg_flow_create(C.byref(cfg), self.viscosity, WALLS[wall], C.byref(self._h)))
        self.time = 0.0
        self.steps = 0
        self.uploads = 0          # fields sent to the device (set_vorticity, set_forcing)
        self.downloads = 0        # fields fetched from it
        self.history = []         # (dt, omega cycles, psi cycles, converged) per step
        self.set_wall_speeds(speeds)
        if forcing is not None:
            self.set_forcing(forcing)
        self.set_vorticity(np.zeros((self.nx, self.ny)))

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc):
        if rc == _lib.MG_OK:
            return
        msg = self._lib.mg_flow_last_error(self._h)
        msg = (msg.decode() if msg else "") or f"mghip error {rc}"
        if rc in (_lib.MG_ERR_INVALID_VALUE, _lib.MG_ERR_STATE):
            raise ValueError(msg)
        if rc == _lib.MG_ERR_ALLOC:
            raise MemoryError(msg)
        raise RuntimeError("mghip: " + msg)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mg_flow_destroy(self._h)
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

    def _get(self, which):
        out = np.empty((self.nx, self.ny))
        self._check(self._lib.mg_flow_get(self._h, FIELDS[which], _lib.ptr(out), _lib.MG_F64))
        self.downloads += 1
        return out

    @staticmethod
    def _dev_args(t):
        return C.c_void_p(t.data_ptr()), int(t.stride(0)), _lib.dtype_code(str(t.dtype).split(".")[-1])

    def get_device(self, which, t):
        """field "omega", "psi" or "N" -> the 2-D device tensor t (nx, ld), no host transfer"""
        p, ld, dt = self._dev_args(t)
        self._check(self._lib.mg_flow_get_device(self._h, FIELDS[which], p, ld, dt))

    def set_device(self, which, t):
        """the first ny columns of the 2-D device tensor t -> field "omega", "psi" or "N" as it is (no solve, no wall update)"""
        p, ld, dt = self._dev_args(t)
        self._check(self._lib.mg_flow_set_device(self._h, FIELDS[which], p, ld, dt))

    # ------------------------------------------------------------------ state
    def set_wall_speeds(self, wall_speeds):
        self.wall_speeds = wall_speed_array(wall_speeds)
        self._check(self._lib.mg_flow_set_walls(self._h, (C.c_double * 4)(*self.wall_speeds)))

    def set_forcing(self, forcing):
        if forcing is None:
            self._check(self._lib.mg_flow_set_forcing(self._h, None, _lib.MG_F64))
            return
        f = self._field(forcing)
        self._check(self._lib.mg_flow_set_forcing(self._h, _lib.ptr(f), _lib.dtype_code(f.dtype)))
        self.uploads += 1

    def set_vorticity(self, w0):
        """w := w0, psi from -lap psi = w0, the wall ring of w from that psi; the multistep history and the clock restart"""
        w = self._field(w0)
        info = _lib.MgFlowStepInfo()
        self._check(self._lib.mg_flow_set_state(self._h, _lib.ptr(w), _lib.dtype_code(w.dtype), self.tolerance, self.max_cycles,
                                                C.byref(info)))
        self.uploads += 1
        self.time, self.steps, self.history = 0.0, 0, []
        return _info_dict(info, with_omega=False)

    # ------------------------------------------------------------------ stepping
    def step(self, dt, tol=None, max_cycles=None):
        info = _lib.MgFlowStepInfo()
        self._check(self._lib.mg_flow_step(self._h, float(dt), self.tolerance if tol is None else float(tol),
                                           self.max_cycles if max_cycles is None else int(max_cycles), C.byref(info)))
        self.time += float(dt)
        self.steps += 1
        d = _info_dict(info)
        self.history.append((float(dt), d["omega_cycles"], d["psi_cycles"], d["converged"]))
        return d

    def velocity_max(self):
        """m = max(|psi_N - psi_S| + |psi_E - psi_W|) of the current psi, taken on the device: cfl = dt m / (2 hx hy)"""
        out = C.c_double(0.0)
        self._check(self._lib.mg_flow_velocity_max(self._h, C.byref(out)))
        return out.value

    def advance(self, t_final, dt=None, cfl=0.5):
        """Step until self.time reaches t_final.  dt=None picks dt = cfl 2 hx hy / m from the device maximum before every step;
        either way the last step is cut so that the run ends at t_final.  Returns the list of step infos."""
        if dt is not None and not dt > 0.0:
            raise ValueError("dt must be > 0")
        if not cfl > 0.0:
            raise ValueError("cfl must be > 0")
        infos = []
        while t_final - self.time > 1e-12 * max(1.0, abs(t_final)):
            if dt is None:
                m = self.velocity_max()
                if not np.isfinite(m):
                    raise FloatingPointError(f"advance(dt=None): the velocity maximum is not finite ({m}): the state has blown up")
                if not m > 0.0:
                    raise ValueError("advance(dt=None): the fluid is at rest (no velocity to take a CFL step from); give dt")
                step = cfl * 2.0 * self.hx * self.hy / m
            else:
                step = float(dt)
            left = t_final - self.time
            last = step >= left * (1.0 - 1e-12)
            infos.append(self.step(left if last else step))
            if last:
                self.time = float(t_final)
        return infos

    def run_to_steady(self, dt, rate_tol=1e-6, max_steps=100000):
        """Fixed-dt steps until max |w_new - w| / dt < rate_tol (taken on the device).  Returns steps, rate, converged,
        diverged, all_solves_converged, omega_cycles and psi_cycles (lists).  The run stops at the first step whose
        omega_change or cfl is not finite: diverged is True then and converged False."""
        rate, wc, pc, ok, diverged = float("inf"), [], [], True, False
        n = 0
        while n < max_steps:
            info = self.step(dt)
            n += 1
            wc.append(info["omega_cycles"]); pc.append(info["psi_cycles"])
            ok = ok and info["converged"]
            rate = info["omega_change"] / dt
            if not (np.isfinite(info["omega_change"]) and np.isfinite(info["cfl"])):
                diverged = True
                break
            if rate < rate_tol:
                break
        return {"steps": n, "rate": rate, "converged": (not diverged) and rate < rate_tol, "diverged": diverged,
                "all_solves_converged": ok, "omega_cycles": wc, "psi_cycles": pc, "time": self.time}

    # ------------------------------------------------------------------ results
    @property
    def vorticity(self):
        return self._get("omega")

    @property
    def stream_function(self):
        return self._get("psi")

    def velocity(self):
        """(u, v) = (psi_y, -psi_x) by central differences of psi on the host.  No through-flow at the walls; no-slip walls carry
        their tangential speeds, free-slip walls the difference across the wall of the odd extension of psi (w = 0 there)"""
        psi = self.stream_function
        u, v = np.zeros_like(psi), np.zeros_like(psi)
        u[1:-1, 1:-1] = (psi[1:-1, 2:] - psi[1:-1, :-2]) / (2 * self.hy)
        v[1:-1, 1:-1] = -(psi[2:, 1:-1] - psi[:-2, 1:-1]) / (2 * self.hx)
        if self.wall == "no_slip":
            v[0, :], v[-1, :], u[:, 0], u[:, -1] = self.wall_speeds
        else:
            v[0, 1:-1] = -(psi[1, 1:-1] - psi[0, 1:-1]) / self.hx
            v[-1, 1:-1] = -(psi[-1, 1:-1] - psi[-2, 1:-1]) / self.hx
            u[1:-1, 0] = (psi[1:-1, 1] - psi[1:-1, 0]) / self.hy
            u[1:-1, -1] = (psi[1:-1, -1] - psi[1:-1, -2]) / self.hy
        return u, v

    def diagnostics(self):
        """kinetic energy 0.5 hx hy sum(psi w) (psi = 0 on the walls) and enstrophy 0.5 hx hy sum(w^2), summed on the device"""
        out = (C.c_double * 2)()
        self._check(self._lib.mg_flow_diagnostics(self._h, out))
        a = 0.5 * self.hx * self.hy
        return {"kinetic_energy": a * out[0], "enstrophy": a * out[1], "time": self.time, "steps": self.steps}
