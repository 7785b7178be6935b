"""NumPy restatement of the device-resident vorticity / stream-function stepper (include/mghip_flow.h, csrc/mg_flow.hip) -- not
a test.

The Jacobian, the right-hand side and the wall formulas are the header's, in the header's association; lap is
oracle.mg_oracle.apply_laplacian(coeff = +1).  A step solves its two Dirichlet problems either with MGOracle (the pinned
cycle, for comparisons at a fixed cycle count or a tolerance) or directly with a sine transform (long runs: a converged
multigrid solve agrees with it to the solve tolerance).  tests/test_flow_cpu.py shows that this file is a correct scheme."""
import numpy as np

from oracle import mg_oracle as O

FREE_SLIP, NO_SLIP = 0, 1
UNIT = (0.0, 1.0, 0.0, 1.0)


def _nb(a):
    """the nine neighbours of the interior cells: E/W = i +- 1, N/S = j +- 1"""
    return dict(C=a[1:-1, 1:-1], E=a[2:, 1:-1], W=a[:-2, 1:-1], N=a[1:-1, 2:], S=a[1:-1, :-2],
                NE=a[2:, 2:], NW=a[:-2, 2:], SE=a[2:, :-2], SW=a[:-2, :-2])


def jacobian(psi, w, hx, hy):
    """Arakawa (1966) J(psi, w) = psi_x w_y - psi_y w_x on interior cells, 0 on the ring, in the header's association"""
    p, q = _nb(psi), _nb(w)
    J1 = (p["E"] - p["W"]) * (q["N"] - q["S"]) - (p["N"] - p["S"]) * (q["E"] - q["W"])
    J2 = ((p["E"] * (q["NE"] - q["SE"]) - p["W"] * (q["NW"] - q["SW"])) - p["N"] * (q["NE"] - q["NW"])) + p["S"] * (q["SE"] - q["SW"])
    J3 = ((p["NE"] * (q["N"] - q["E"]) - p["SW"] * (q["W"] - q["S"])) - p["NW"] * (q["N"] - q["W"])) + p["SE"] * (q["E"] - q["S"])
    out = np.zeros_like(w)
    out[1:-1, 1:-1] = ((J1 + J2) + J3) / (12.0 * hx * hy)
    return out


def jacobian_other_association(psi, w, hx, hy):
    """the same nine-point Jacobian summed in another order and scaled by a reciprocal: how far two correct evaluations lie
    apart in fp64 (the yardstick for grids whose spacings are not exact)"""
    p, q = _nb(psi), _nb(w)
    J3 = p["SE"] * (q["E"] - q["S"]) + (p["NE"] * (q["N"] - q["E"]) - (p["NW"] * (q["N"] - q["W"]) + p["SW"] * (q["W"] - q["S"])))
    J2 = p["S"] * (q["SE"] - q["SW"]) + (p["E"] * (q["NE"] - q["SE"]) - (p["N"] * (q["NE"] - q["NW"]) + p["W"] * (q["NW"] - q["SW"])))
    J1 = (p["E"] - p["W"]) * (q["N"] - q["S"]) - (p["N"] - p["S"]) * (q["E"] - q["W"])
    out = np.zeros_like(w)
    out[1:-1, 1:-1] = (J3 + (J2 + J1)) * (1.0 / (12.0 * hx * hy))
    return out


def velocity_max(psi):
    """m = max(|N(p) - S(p)| + |E(p) - W(p)|) over interior cells: cfl = dt m / (2 hx hy)"""
    p = _nb(psi)
    return float(np.max(np.abs(p["N"] - p["S"]) + np.abs(p["E"] - p["W"])))


def ab2(dt, dt_prev):
    """(c0, c1) of variable-step Adams-Bashforth 2; dt_prev None: the first step"""
    if dt_prev is None:
        return 1.0, 0.0
    r = dt / dt_prev
    return 1.0 + r / 2, -r / 2


def rhs(psi, w, nu, dt, hx, hy, c0=1.0, c1=0.0, n_prev=None, force=None):
    """what mg_dev_flow_rhs stores: (f, N, sum f^2, m)"""
    N = jacobian(psi, w, hx, hy)
    if force is not None:
        N[1:-1, 1:-1] = N[1:-1, 1:-1] + force[1:-1, 1:-1]
    lap = O.apply_laplacian(w, hx, hy, 1.0)
    sigma, k = 2.0 / (nu * dt), 2.0 / nu
    ab = (c0 * N) + (c1 * n_prev) if n_prev is not None else c0 * N
    val = (sigma * w + lap) + k * ab
    f = np.zeros_like(w)
    f[1:-1, 1:-1] = val[1:-1, 1:-1]
    return f, N, float(np.sum(f * f)), velocity_max(psi)


def rhs_other_association(psi, w, nu, dt, hx, hy, c0=1.0, c1=0.0, n_prev=None, force=None):
    """f of `rhs` evaluated another correct way: the other Jacobian, lap with reciprocal spacings (the kernels' form where
    the oracle divides) and the three terms summed from the right"""
    N = jacobian_other_association(psi, w, hx, hy)
    if force is not None:
        N[1:-1, 1:-1] = force[1:-1, 1:-1] + N[1:-1, 1:-1]
    q = _nb(w)
    lap = np.zeros_like(w)
    lap[1:-1, 1:-1] = ((q["E"] + q["W"]) * (1.0 / (hx * hx)) + (q["N"] + q["S"]) * (1.0 / (hy * hy))) - q["C"] * (2.0 / (hx * hx) + 2.0 / (hy * hy))
    sigma, k = 2.0 / (nu * dt), 2.0 / nu
    ab = (c1 * n_prev) + (c0 * N) if n_prev is not None else c0 * N
    return interior(sigma * w + (lap + k * ab))


def wall(w, psi, hx, hy, kind, speeds=(0.0, 0.0, 0.0, 0.0)):
    """the ring of w in place: 0, or Thom's formula with {left v, right v, bottom u, top u}; left, right, bottom, top in this
    order, so corners carry bottom / top"""
    if kind == FREE_SLIP:
        w[0, :] = w[-1, :] = 0.0
        w[:, 0] = w[:, -1] = 0.0
        return w
    vl, vr, ub, ut = speeds
    w[0, :] = (2.0 * (psi[0, :] - psi[1, :])) / (hx * hx) - (2.0 * vl) / hx
    w[-1, :] = (2.0 * (psi[-1, :] - psi[-2, :])) / (hx * hx) + (2.0 * vr) / hx
    w[:, 0] = (2.0 * (psi[:, 0] - psi[:, 1])) / (hy * hy) + (2.0 * ub) / hy
    w[:, -1] = (2.0 * (psi[:, -1] - psi[:, -2])) / (hy * hy) - (2.0 * ut) / hy
    return w


def interior(w):
    """w with a zero ring: the right-hand side of the stream-function solve"""
    g = np.zeros_like(w)
    g[1:-1, 1:-1] = w[1:-1, 1:-1]
    return g


def diag(psi, w):
    """(sum psi w, sum w^2, m) over interior cells"""
    return float(np.sum(psi[1:-1, 1:-1] * w[1:-1, 1:-1])), float(np.sum(w[1:-1, 1:-1] ** 2)), velocity_max(psi)


# ---------------------------------------------------------------------------------------------- the two solvers
class SineSolver:
    """(-lap_h + shift) u = f on interior cells with the Dirichlet ring of `guess`, solved directly: the five-point
    Laplacian is diagonal in the sine basis"""

    def __init__(self, nx, ny, domain=UNIT):
        self.hx, self.hy = O.grid_spacing(nx, ny, domain)
        mx, my = nx - 2, ny - 2
        kx, ky = np.arange(1, mx + 1), np.arange(1, my + 1)
        self.Sx = np.sin(np.pi * np.outer(kx, kx) / (mx + 1))
        self.Sy = np.sin(np.pi * np.outer(ky, ky) / (my + 1))
        self.norm = (2.0 / (mx + 1)) * (2.0 / (my + 1))
        lx = (4.0 / self.hx**2) * np.sin(np.pi * kx / (2 * (mx + 1))) ** 2
        ly = (4.0 / self.hy**2) * np.sin(np.pi * ky / (2 * (my + 1))) ** 2
        self.lam = lx[:, None] + ly[None, :]

    def __call__(self, f, guess, shift):
        b = f[1:-1, 1:-1].copy()
        b[0, :] += guess[0, 1:-1] / self.hx**2
        b[-1, :] += guess[-1, 1:-1] / self.hx**2
        b[:, 0] += guess[1:-1, 0] / self.hy**2
        b[:, -1] += guess[1:-1, -1] / self.hy**2
        hat = self.Sx @ b @ self.Sy
        out = guess.copy()
        out[1:-1, 1:-1] = self.norm * (self.Sx @ (hat / (self.lam + shift)) @ self.Sy)
        return out, {"cycles": 0, "final_residual": 0.0, "converged": True}


class CycleSolver:
    """the pinned oracle's cycle from `guess` to ||r|| < tol max(1, ||f||_h) (tol = 0: exactly max_cycles cycles)"""

    def __init__(self, nx, ny, domain=UNIT, tol=1e-10, max_cycles=50, smoother="jacobi", omega=0.8, max_levels=32, oracle_cls=None):
        self.oracle_cls = oracle_cls                   # None: the pinned MGOracle; or tests/coarse_exact_reference.ExactCoarseOracle
        self.nx, self.ny, self.domain = nx, ny, domain
        self.hx, self.hy = O.grid_spacing(nx, ny, domain)
        self.tol, self.max_cycles = tol, max_cycles
        self.kw = dict(domain=domain, max_levels=max_levels, cycle="V", pre=2, post=2, smoother=smoother, omega=omega)

    def __call__(self, f, guess, shift):
        fnorm = float(np.sqrt(self.hx * self.hy * np.sum(f * f)))
        mgo = (self.oracle_cls or O.MGOracle)(self.nx, self.ny, shift=shift, **self.kw)
        out, info = mgo.solve(f, guess, tol=self.tol * max(1.0, fnorm), max_iterations=self.max_cycles)
        return out, {"cycles": info["iterations"], "final_residual": info["final_residual"], "converged": info["converged"],
                     "rhs_norm": fnorm}


# ---------------------------------------------------------------------------------------------- the stepper
class Flow:
    """state (w, psi, N of the latest step, dt_prev) and the step of mg_flow_step, on either solver"""

    def __init__(self, nx, ny, nu, kind=NO_SLIP, speeds=(0.0, 0.0, 0.0, 0.0), force=None, domain=UNIT, solver=None):
        self.nx, self.ny, self.nu, self.kind, self.speeds, self.force = nx, ny, nu, kind, tuple(speeds), force
        self.hx, self.hy = O.grid_spacing(nx, ny, domain)
        self.solver = solver if solver is not None else SineSolver(nx, ny, domain)
        self.w = np.zeros((nx, ny))
        self.psi = np.zeros((nx, ny))
        self.n_prev, self.dt_prev = None, None
        self.time = 0.0

    def set_state(self, w0):
        """mg_flow_set_state: psi from zero, then the wall ring of w, and no history"""
        self.w = np.array(w0, dtype=np.float64)
        self.psi, info = self.solver(interior(self.w), np.zeros_like(self.w), 0.0)
        wall(self.w, self.psi, self.hx, self.hy, self.kind, self.speeds)
        self.n_prev, self.dt_prev, self.time = None, None, 0.0
        return info

    def step(self, dt):
        c0, c1 = ab2(dt, self.dt_prev)
        f, N, sumsq, m = rhs(self.psi, self.w, self.nu, dt, self.hx, self.hy, c0, c1, self.n_prev, self.force)
        sigma = 2.0 / (self.nu * dt)
        guess = wall(self.w.copy(), self.psi, self.hx, self.hy, self.kind, self.speeds)
        w_new, iw = self.solver(f, guess, sigma)
        change = float(np.max(np.abs(w_new - guess)))
        psi_new, ip = self.solver(interior(w_new), self.psi, 0.0)
        self.w, self.psi, self.n_prev, self.dt_prev = w_new, psi_new, N, dt
        self.time += dt
        return {"sigma": sigma, "c0": c0, "c1": c1, "cfl": dt * m / (2 * self.hx * self.hy),
                "rhs_norm": float(np.sqrt(self.hx * self.hy * sumsq)), "omega": iw, "psi": ip, "omega_change": change}

    def run(self, nsteps, dt):
        return [self.step(dt) for _ in range(nsteps)]


def psi_min(psi, domain=UNIT):
    """(min psi, x, y) on the grid"""
    nx, ny = psi.shape
    i, j = np.unravel_index(np.argmin(psi), psi.shape)
    hx, hy = O.grid_spacing(nx, ny, domain)
    return float(psi[i, j]), domain[0] + i * hx, domain[2] + j * hy
