"""NumPy restatement of the semilinear Newton method (include/mghip_nl.h, csrc/mg_nl.hip): the eval kernel with the exact
association the header states, conjugate gradients with a reaction field (the loop of tests/pcg_reference.py, whose pieces it
imports, with A + diag(c) outside and the cycle shifted by c_ref inside), the Newton loop, and a dense exact Newton
(np.linalg.solve, up to 33 x 33).  What tests/test_nl_cpu.py pins and tests/test_gpu_nl.py compares the device against."""
import numpy as np

import pcg_reference as R

LINEAR, CUBIC, SINH, EXP = 0, 1, 2, 3
KINDS = {"linear": LINEAR, "cubic": CUBIC, "sinh": SINH, "exp": EXP}


def phi(kind, v):
    """(phi(v), phi'(v)) in the header's forms"""
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == LINEAR:
            return v, np.ones_like(v)
        if kind == CUBIC:
            vv = v * v
            return vv * v, 3.0 * vv
        if kind == SINH:
            return np.sinh(v), np.cosh(v)
        if kind == EXP:
            e = np.exp(v)
            return e, e
    raise ValueError("kind")


def apply_A(v, hx, hy, coeff, sigma, a=None):
    """A v on interior cells (v carries its ring), 0 on the ring, in the device's association: times 1/(hx*hx), not divided.
    Works on (nx, ny) and on (nx, ny, m) stacks."""
    ihx2, ihy2 = 1.0 / (hx * hx), 1.0 / (hy * hy)
    mid, dn, up, ea, w = v[1:-1, 1:-1], v[2:, 1:-1], v[:-2, 1:-1], v[1:-1, 2:], v[1:-1, :-2]
    out = np.zeros_like(v)
    with np.errstate(over="ignore", invalid="ignore"):
        if a is None:
            diag = 2.0 / (hx * hx) + 2.0 / (hy * hy)
            if sigma != 0.0:
                diag = diag + sigma
            out[1:-1, 1:-1] = coeff * (((dn + up) * ihx2 + (ea + w) * ihy2) - mid * diag)
        else:
            if v.ndim == 3:
                a = a[:, :, None]
            ac = a[1:-1, 1:-1]
            aip, aim = 0.5 * (ac + a[2:, 1:-1]), 0.5 * (ac + a[:-2, 1:-1])
            ajp, ajm = 0.5 * (ac + a[1:-1, 2:]), 0.5 * (ac + a[1:-1, :-2])
            sx = aip * dn + aim * up
            sy = ajp * ea + ajm * w
            D = (aip + aim) * ihx2 + (ajp + ajm) * ihy2
            if sigma != 0.0:
                D = D + sigma
            out[1:-1, 1:-1] = coeff * ((sx * ihx2 + sy * ihy2) - mid * D)
    return out


def evaluate(kind, u, f, hx, hy, coeff, sigma, kappa, a=None, w=None, delta=None, t=1.0):
    """the eval kernel: -> dict(v, F, c, g, sums) with v = u + t delta on interior cells (u on the ring), F = (f - A v) - g,
    g = (kappa w) phi(v), c = (kappa w) phi'(v) on interior cells and 0 on the ring; sums = (sum F^2, sum c)"""
    v = np.array(u, dtype=np.float64)
    if delta is not None:
        v[1:-1, 1:-1] = u[1:-1, 1:-1] + t * delta[1:-1, 1:-1]
    vi = v[1:-1, 1:-1]
    ph, dph = phi(kind, vi)
    kw = kappa if w is None else kappa * w[1:-1, 1:-1]
    F, c, g = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
    with np.errstate(over="ignore", invalid="ignore"):
        g[1:-1, 1:-1] = kw * ph
        F[1:-1, 1:-1] = (f[1:-1, 1:-1] - apply_A(v, hx, hy, coeff, sigma, a)[1:-1, 1:-1]) - g[1:-1, 1:-1]
        c[1:-1, 1:-1] = kw * dph
        sums = (float(np.sum(F * F)), float(np.sum(c)))
    return {"v": v, "F": F, "c": c, "g": g, "sums": sums}


def norm_h(F, hx, hy):
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.sqrt(hx * hy * np.sum(F[1:-1, 1:-1] ** 2)))


class Problem:
    """A u + kappa w phi(u) = f on an (nx, ny) grid of `domain`"""

    def __init__(self, kind, nx, ny, kappa, a=None, w=None, coeff=-1.0, sigma=0.0, domain=(0.0, 1.0, 0.0, 1.0), oracle_classes=None):
        self.oracle_classes = oracle_classes           # what .oracle() builds from (pcg_reference.make_oracle); None: the pinned pair
        self.kind = KINDS[kind] if isinstance(kind, str) else kind
        self.nx, self.ny, self.kappa, self.a, self.w, self.coeff, self.sigma, self.domain = nx, ny, kappa, a, w, coeff, sigma, domain
        self.hx, self.hy = (domain[1] - domain[0]) / (nx - 1), (domain[3] - domain[2]) / (ny - 1)

    def evaluate(self, u, f, delta=None, t=1.0):
        return evaluate(self.kind, u, f, self.hx, self.hy, self.coeff, self.sigma, self.kappa, self.a, self.w, delta, t)

    def N(self, u):
        """N_h(u) = A u + g(u) on interior cells, 0 on the ring (the right-hand side of a manufactured problem)"""
        return -self.evaluate(u, np.zeros_like(u))["F"]

    def norm(self, F):
        return norm_h(F, self.hx, self.hy)

    def oracle(self, shift, pre=2, post=2, smoother="jacobi", omega=0.8):
        return R.make_oracle(self.nx, self.ny, self.a, pre, post, smoother, omega, shift=self.sigma + shift, domain=self.domain,
                             oracle_classes=self.oracle_classes)


def mesh(nx, ny, domain=(0.0, 1.0, 0.0, 1.0)):
    x, y = np.linspace(domain[0], domain[1], nx), np.linspace(domain[2], domain[3], ny)
    return np.meshgrid(x, y, indexing="ij")


def manufactured(nx, ny):
    """u* = 2 sin(pi x) sin(pi y) on the unit square (zero on the ring up to rounding: the ring is set to exactly 0)"""
    X, Y = mesh(nx, ny)
    return R.zero_ring(2.0 * np.sin(np.pi * X) * np.sin(np.pi * Y))


def disc(nx, ny, radius=0.3, inside=1.0, outside=80.0):
    """the Poisson-Boltzmann shape: (a, w) with a = inside / outside the disc and w = 0 / 1"""
    X, Y = mesh(nx, ny)
    out = (X - 0.5) ** 2 + (Y - 0.5) ** 2 > radius ** 2
    return np.where(out, outside, inside), np.where(out, 1.0, 0.0)


# ------------------------------------------------------------------------------------------ conjugate gradients, A + diag(c)
def pcg_react(p, mgo, f, c, u0=None, tol=1e-8, max_iterations=50, flexible=False, pm=None, num_cycles=1):
    """tests/pcg_reference.py's loop for (A + diag(c)) x = f: `mgo` -- built with the shift sigma + c_ref -- is the
    preconditioner only.  The norm is sqrt(hx hy (sum of r^2 over interior cells + sum of f^2 over the ring))."""
    f = np.asarray(f, dtype=np.float64)
    x = np.zeros_like(f) if u0 is None else np.array(u0, dtype=np.float64)
    ring = R.ring_sumsq(f)
    norm = lambda r: float(np.sqrt(p.hx * p.hy * (np.sum(r * r) + ring)))
    op = lambda v: apply_A(v, p.hx, p.hy, p.coeff, p.sigma, p.a) + c * v
    lin = lambda xx: evaluate(LINEAR, xx, f, p.hx, p.hy, p.coeff, p.sigma, 1.0, p.a, c)["F"]       # f - (A x + c x), zero ring
    r = lin(x)
    initial = norm(r)
    hist, status, converged = [], "max_iterations", False
    pd = q = None
    rz = alpha = 0.0
    if initial < tol:
        status, converged = "converged", True
    else:
        for k in range(max_iterations):
            z = R.apply_M(mgo, r, pm, num_cycles)
            rz_new = float(np.sum(r * z))
            if k == 0:
                pd = z.copy()
            else:
                beta = -alpha * float(np.sum(z * q)) / rz if flexible else rz_new / rz
                pd = z + beta * pd
            rz = rz_new
            q = op(pd)
            pq = float(np.sum(pd * q))
            if not (pq > 0.0) or not np.isfinite(pq):
                status = "breakdown"
                break
            alpha = rz / pq
            x = x + alpha * pd
            r = r - alpha * q
            hist.append(norm(r))
            if hist[-1] < tol:
                status, converged = "converged", True
                break
    true = norm(lin(x))
    return x, {"iterations": len(hist), "converged": converged, "residual_history": hist, "true_residual": true,
               "initial_residual": initial, "status": status}


# ------------------------------------------------------------------------------------------ Newton
def jacobian_dense(p, c):
    """A + diag(c) on the interior unknowns as a dense matrix (grids up to 33 x 33)"""
    nx, ny = p.nx, p.ny
    m = (nx - 2) * (ny - 2)
    assert m <= 31 * 31, "the dense Newton is for grids up to 33 x 33"
    E = np.zeros((nx, ny, m))
    E[1:-1, 1:-1, :] = np.eye(m).reshape(nx - 2, ny - 2, m)
    J = apply_A(E, p.hx, p.hy, p.coeff, p.sigma, p.a)[1:-1, 1:-1, :].reshape(m, m)
    return J + np.diag(c[1:-1, 1:-1].ravel())


def forcing_term(k, norm, prev_norm, prev_eta, forcing="eisenstat_walker", eta=1e-8, gamma=0.9, eta_max=0.1, eta_min=1e-10):
    if forcing == "fixed":
        return eta
    if k == 0:
        return eta_max
    q = norm / prev_norm
    e = gamma * (q * q)
    guard = gamma * (prev_eta * prev_eta)
    if guard > 0.1:
        e = max(e, guard)
    return min(max(e, eta_min), eta_max)


def newton(p, f, u0, tol, max_newton=30, inner="pcg", forcing="eisenstat_walker", eta=1e-8, gamma=0.9, eta_max=0.1,
           eta_min=1e-10, max_backtracks=10, max_inner=100, pm=None, pre=2, post=2, smoother="jacobi", omega=0.8):
    """the driver's loop; inner = "pcg" (the restated reaction-field loop, preconditioned by the oracle's cycle with the shift
    sigma + cbar) or "dense" (np.linalg.solve: exact Newton, forcing ignored).  -> (u, info)"""
    u = np.array(u0, dtype=np.float64)
    ev = p.evaluate(u, f)
    norm = p.norm(ev["F"])
    cells = float(p.nx - 2) * float(p.ny - 2)
    initial = norm
    hist, inners, steps, etas, backtracks = [], [], [], [], 0
    prev_norm, prev_eta, status, evals = norm, eta_max, "max_newton", 1
    k = 0
    while True:
        if norm < tol:
            status = "converged"
            break
        if k == max_newton:
            break
        e = forcing_term(k, norm, prev_norm, prev_eta, forcing, eta, gamma, eta_max, eta_min)
        if inner == "dense":
            J = jacobian_dense(p, ev["c"])
            delta = np.zeros_like(u)
            delta[1:-1, 1:-1] = np.linalg.solve(J, ev["F"][1:-1, 1:-1].ravel()).reshape(p.nx - 2, p.ny - 2)
            n_in = 0
        else:
            cbar = ev["sums"][1] / cells
            mgo = p.oracle(cbar, pre, post, smoother, omega)
            delta, pinfo = pcg_react(p, mgo, ev["F"], ev["c"], tol=max(e * norm, 0.1 * tol), max_iterations=max_inner,
                                     flexible=R.default_flexible(smoother, pre, post), pm=pm)
            n_in = pinfo["iterations"]
            if pinfo["status"] == "breakdown" and n_in == 0:
                status = "breakdown"
                break
        t, accepted = 1.0, None
        for _ in range(max_backtracks + 1):
            trial = p.evaluate(u, f, delta, t)
            evals += 1
            tn = p.norm(trial["F"])
            if np.isfinite(tn) and tn <= (1.0 - 1e-4 * t) * norm:
                accepted = trial
                break
            t *= 0.5
            backtracks += 1
        if accepted is None:
            status = "line_search_failed"
            break
        u, ev = accepted["v"], accepted
        prev_norm, prev_eta, norm = norm, e, tn
        hist.append(norm); inners.append(n_in); steps.append(t); etas.append(e)
        k += 1
    return u, {"newton_iterations": k, "inner_iterations": inners, "residual_history": hist, "step_lengths": steps,
               "forcing_terms": etas, "status": status, "converged": status == "converged", "initial_residual": initial,
               "true_residual": norm, "backtracks": backtracks, "evaluations": evals}
