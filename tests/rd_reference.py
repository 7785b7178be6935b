"""NumPy restatement of the reaction-diffusion stepper (include/mghip_rd.h, csrc/mg_rd.hip) -- not a test: the right-hand sides
in the header's association, the three sums of the free energy term by term, one step with a dense exact Newton method
(nl_reference.newton(inner="dense")), and the closed-form factors of one step on a discrete eigenmode.  What
tests/test_rd_cpu.py pins and tests/test_gpu_rd.py compares the device against."""
import numpy as np

import heat_device_reference as HD
import nl_reference as NL

IMPLICIT, CN, BDF2 = HD.IMPLICIT, HD.CN, HD.BDF2
SCHEME_CODES = {IMPLICIT: 1, CN: 2, BDF2: 3}
lam = HD.lam
set_ring = HD.set_ring


def lap(u, hx, hy, a=None):
    """L_a u on interior cells (0 on the ring) in the kernels' association: times 1/(hx*hx), not divided"""
    return NL.apply_A(u, hx, hy, 1.0, 0.0, a)


def rhs(scheme, kind, u, dt, alpha, hx, hy, kappa=0.0, rho=0.0, u_prev=None, S=None, a=None, w=None, g0=1.0, g1=1.0):
    """what mg_dev_rd_rhs stores: f on interior cells in the header's association, 0 on the ring"""
    sc = np.zeros_like(u) if S is None else S
    dta = dt * alpha
    with np.errstate(over="ignore", invalid="ignore"):
        if scheme == IMPLICIT:
            val = (u + dt * ((g1 * sc) + rho * u)) / dta
        elif scheme == CN:
            h = (2.0 * ((u + (dta * lap(u, hx, hy, a)) / 2) + (dt * ((g0 * sc) + (g1 * sc))) / 2)) / dta
            ka = kappa / alpha
            kw = ka if w is None else ka * w
            E = u if u_prev is None else (3.0 * u - u_prev) / 2
            val = (h + ((2.0 * rho) / alpha) * E) - kw * NL.phi(kind, u)[0]
        elif scheme == BDF2:
            val = ((4.0 * u - u_prev) / (2 * dt * alpha) + (g1 * sc) / alpha) + (rho / alpha) * (2.0 * u - u_prev)
        else:
            raise ValueError(scheme)
    out = np.zeros_like(u)
    out[1:-1, 1:-1] = val[1:-1, 1:-1]
    return out


def Phi(kind, v):
    """the antiderivative of phi in the header's forms (>= 0)"""
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == NL.LINEAR:
            return (v * v) / 2
        if kind == NL.CUBIC:
            return ((v * v) * (v * v)) / 4
        if kind == NL.SINH:
            return np.cosh(v) - 1.0
        if kind == NL.EXP:
            return np.exp(v)
    raise ValueError("kind")


def energy_terms(kind, u, hx, hy, a=None, w=None):
    """(G, P, Q) term by term, each an (nx, ny) array of the cell's own term (0 where the cell has none), in the kernel's
    association: a cell owns the face to its next row and the face to its next column"""
    nx, ny = u.shape
    rx, ry = hy / hx, hx / hy
    tx, ty = np.zeros_like(u), np.zeros_like(u)
    with np.errstate(over="ignore", invalid="ignore"):
        du = u[1:, :] - u[:-1, :]
        dv = u[:, 1:] - u[:, :-1]
        fx, fy = du * du, dv * dv
        if a is not None:
            fx = (0.5 * (a[:-1, :] + a[1:, :])) * fx
            fy = (0.5 * (a[:, :-1] + a[:, 1:])) * fy
        tx[:-1, 1:-1] = (fx * rx)[:, 1:-1]                  # rows 0 .. nx-2, columns 1 .. ny-2
        ty[1:-1, :-1] = (fy * ry)[1:-1, :]                  # rows 1 .. nx-2, columns 0 .. ny-2
        G = 0.5 * (tx + ty)
        P, Q = np.zeros_like(u), np.zeros_like(u)
        ui = u[1:-1, 1:-1]
        P[1:-1, 1:-1] = Phi(kind, ui) if w is None else w[1:-1, 1:-1] * Phi(kind, ui)
        Q[1:-1, 1:-1] = ui * ui
    return G, P, Q


def energy(kind, u, hx, hy, alpha, kappa, rho, a=None, w=None):
    """{G, P, Q, E} with E = alpha G + hx hy (kappa P - rho Q / 2), as mg_rd_energy forms it"""
    import math
    G, P, Q = (math.fsum(t.ravel().tolist()) for t in energy_terms(kind, u, hx, hy, a, w))
    return {"gradient": G, "potential": P, "sum_squares": Q, "energy": alpha * G + (hx * hy) * (kappa * P - (rho * Q) / 2)}


def step(scheme, kind, u, dt, alpha, kappa=0.0, rho=0.0, domain=(0.0, 1.0, 0.0, 1.0), u_prev=None, S=None, a=None, w=None, g0=1.0,
         g1=1.0, edge4=None, tol=1e-10, max_newton=50, inner="dense", oracle_classes=None, **newton_kw):
    """one step with the dense exact Newton method: (u_new, info); the tolerance is tol * max(1, ||f||_h), as the driver's.
    inner="pcg": the driver's own Newton - conjugate gradients - multigrid loop restated (nl_reference.newton) on the hierarchy
    classes `oracle_classes` (None: the pinned pair), with nl_reference.newton's keywords in newton_kw"""
    nx, ny = u.shape
    p = NL.Problem(kind, nx, ny, kappa / alpha, a=a, w=w, coeff=-1.0, sigma=lam(scheme, dt, alpha), domain=domain,
                   oracle_classes=oracle_classes)
    f = rhs(scheme, p.kind, u, dt, alpha, p.hx, p.hy, kappa, rho, u_prev, S, a, w, g0, g1)
    guess = u.copy()
    if edge4 is not None:
        set_ring(guess, edge4)
    fnorm = float(np.sqrt(p.hx * p.hy * np.sum(f * f)))
    out, info = NL.newton(p, f, guess, tol * max(1.0, fnorm), max_newton=max_newton, inner=inner, **newton_kw)
    return out, {"lambda": p.sigma, "rhs_norm": fnorm, "initial_residual": info["initial_residual"],
                 "final_residual": info["true_residual"], "newton_iterations": info["newton_iterations"],
                 "inner_iterations": info["inner_iterations"],
                 "converged": info["converged"]}


def run(scheme, kind, u0, dt, nsteps, alpha, kappa=0.0, rho=0.0, S=None, g=None, t0=0.0, **kw):
    """fixed-dt run from u0: BDF2 starts with one Crank-Nicolson step (E = u), Crank-Nicolson uses the previous level once it
    has one (CN-AB2); g(t) is the source's time factor.  Returns the list of levels."""
    g = g or (lambda t: 1.0)
    levels = [u0]
    for k in range(nsteps):
        t = t0 + k * dt
        prev = levels[-2] if k > 0 else None
        sch = CN if (scheme == BDF2 and k == 0) else scheme
        levels.append(step(sch, kind, levels[-1], dt, alpha, kappa, rho, u_prev=None if sch == IMPLICIT else prev, S=S, g0=g(t),
                           g1=g(t + dt), **kw)[0])
    return levels


def eigenmode(nx, ny, domain=(0.0, 1.0, 0.0, 1.0)):
    """(phi, lam_h): sin(pi x') sin(pi y') on the grid with an exactly zero ring and its eigenvalue under -Laplacian_h"""
    X, Y = NL.mesh(nx, ny, domain)
    lx, ly = domain[1] - domain[0], domain[3] - domain[2]
    hx, hy = lx / (nx - 1), ly / (ny - 1)
    phi = np.sin(np.pi * (X - domain[0]) / lx) * np.sin(np.pi * (Y - domain[2]) / ly)
    phi[0] = phi[-1] = 0.0
    phi[:, 0] = phi[:, -1] = 0.0
    return phi, 4.0 / hx**2 * np.sin(np.pi * hx / (2 * lx)) ** 2 + 4.0 / hy**2 * np.sin(np.pi * hy / (2 * ly)) ** 2


def eigen_factor(scheme, dt, alpha, lam_h, kappa, rho, c=None):
    """linear kind, u = phi, u_prev = c phi (None: no previous level): one step gives factor * phi (section 1 of the header)"""
    d = alpha * lam_h + kappa
    if scheme == IMPLICIT:
        return (1.0 + dt * rho) / (1.0 + dt * d)
    if scheme == CN:
        e = 1.0 if c is None else (3.0 - c) / 2
        return (2.0 / dt - d + 2.0 * rho * e) / (2.0 / dt + d)
    if scheme == BDF2:
        return ((4.0 - c) / (2 * dt) + rho * (2.0 - c)) / (3.0 / (2 * dt) + d)
    raise ValueError(scheme)
