"""NumPy reference of the zebra line smoothers (MG_ZEBRA_X / _Y / _ALT) -- TEST INFRASTRUCTURE ONLY.

Our own design (the reference project has no line relaxation).  One sweep of one direction runs colour 0 then colour 1;
the colour of a line is the parity of its grid index (the fixed j of an X line, the fixed i of a Y line).  For every
line of the colour it solves tridiag(-w, D, -w) x = b with w = 1/h_par^2, c = 1/h_perp^2, D = 2w + 2c + sigma,
b = rhs + c (u_prev_line + u_next_line) plus w * ring value at the two ends, then sets u_line += omega (x - u_line) (omega == 1: u_line = x).
All arithmetic runs in the dtype of `u` (Python-float coefficients are weak scalars)."""
import numpy as np

from oracle import mg_oracle as mo

ZEBRA_X, ZEBRA_Y, ZEBRA_ALT = 3, 4, 5
KINDS = {"zebra_x": ZEBRA_X, "zebra_y": ZEBRA_Y, "zebra_alt": ZEBRA_ALT}


def line_coefficients(direction, hx, hy, sigma=0.0):
    """(w, c, D) of a line along x (ZEBRA_X) or along y (ZEBRA_Y)"""
    h_par, h_perp = (hx, hy) if direction == ZEBRA_X else (hy, hx)
    w, c = 1.0 / (h_par * h_par), 1.0 / (h_perp * h_perp)
    return w, c, 2.0 * w + 2.0 * c + sigma


def thomas(w, D, b):
    """Solve tridiag(-w, D, -w) x = b for every row of b (lines, n); plain Thomas in b's dtype."""
    b = np.asarray(b)
    n = b.shape[-1]
    dt = b.dtype.type
    w, D = dt(w), dt(D)
    piv = np.empty(n, dtype=b.dtype)
    y = np.empty_like(b)
    piv[0] = D
    y[..., 0] = b[..., 0] / piv[0]
    for t in range(1, n):
        piv[t] = D - w * (w / piv[t - 1])
        y[..., t] = (b[..., t] + w * y[..., t - 1]) / piv[t]
    x = np.empty_like(b)
    x[..., n - 1] = y[..., n - 1]
    for t in range(n - 2, -1, -1):
        x[..., t] = y[..., t] + (w / piv[t]) * x[..., t + 1]
    return x


def line_rhs(u, rhs, direction, colour, hx, hy, sigma=0.0):
    """(b, index of the lines): b has one row per line of `colour`, ordered along the line."""
    w, c, _ = line_coefficients(direction, hx, hy, sigma)
    v, f = (u.T, rhs.T) if direction == ZEBRA_X else (u, rhs)          # rows of v are the lines
    idx = np.arange(1, v.shape[0] - 1)
    idx = idx[idx % 2 == colour]
    b = f[idx, 1:-1] + c * (v[idx - 1, 1:-1] + v[idx + 1, 1:-1])
    b[:, 0] += w * v[idx, 0]
    b[:, -1] += w * v[idx, -1]
    return b, idx


def colour_pass(u, rhs, direction, colour, hx, hy, sigma=0.0, omega=1.0, solve=thomas):
    """one colour of one direction, in place on a copy; returns (u_new, x) with x the line solutions"""
    u = u.copy()
    w, c, D = line_coefficients(direction, hx, hy, sigma)
    b, idx = line_rhs(u, rhs, direction, colour, hx, hy, sigma)
    if idx.size == 0:
        return u, b
    x = solve(w, D, b)
    v = u.T if direction == ZEBRA_X else u
    old = v[idx, 1:-1]
    v[idx, 1:-1] = x if omega == 1.0 else old + omega * (x - old)          # omega == 1 stores x itself
    return u, x


def zebra_sweep(u, rhs, kind, hx, hy, sigma=0.0, omega=1.0, nu=1, solve=thomas):
    """nu sweeps of MG_ZEBRA_X / _Y / _ALT (ALT: an X sweep followed by a Y sweep)"""
    dirs = (ZEBRA_X, ZEBRA_Y) if kind == ZEBRA_ALT else (kind,)
    for _ in range(nu):
        for d in dirs:
            for colour in (0, 1):
                u, _ = colour_pass(u, rhs, d, colour, hx, hy, sigma, omega, solve)
    return u


def dense_solve(w, D, b):
    """the same systems by a dense LU (np.linalg.solve), for checking thomas"""
    n = b.shape[-1]
    T = D * np.eye(n) - w * (np.eye(n, k=1) + np.eye(n, k=-1))
    return np.linalg.solve(T.astype(b.dtype), b.T).T


class LineMGOracle(mo.MGOracle):
    """MGOracle whose smoother is one of "zebra_x" | "zebra_y" | "zebra_alt" (anything else: the base class's)."""

    line_solve = staticmethod(thomas)

    def _smooth(self, u, level, nu):
        if self.smoother not in KINDS:
            return super()._smooth(u, level, nu)
        hx, hy = self.h[level]
        return zebra_sweep(u, self.rhs[level], KINDS[self.smoother], hx, hy, self.shift, self.omega, nu, self.line_solve)


def asymptotic_factor(smoother, nx, ny, domain=(0.0, 1.0, 0.0, 1.0), cycles=12, seed=0, **kw):
    """residual reduction factors per cycle of V(2,2) over all levels, random rhs / start with a zero ring"""
    rng = np.random.default_rng(seed)
    rhs, u0 = rng.standard_normal((nx, ny)), rng.standard_normal((nx, ny))
    for a in (rhs, u0):
        a[0, :] = a[-1, :] = 0.0
        a[:, 0] = a[:, -1] = 0.0
    mg = LineMGOracle(nx, ny, domain=domain, max_levels=32, cycle="V", pre=2, post=2, smoother=smoother,
                      omega=kw.pop("omega", 1.0), **kw)
    _, info = mg.solve(rhs, u0, tol=0.0, max_iterations=cycles)
    h = np.array(info["residual_history"])
    return h[1:] / h[:-1]
