"""A plain NumPy restatement of the 3-D multigrid family (include/mghip_3d.h): every operator, the coarsest solve, the cycle, the
solve loop and the defect step, in the header's associations.  Fields are C-ordered (nx, ny, nz) arrays of np.float64 or
np.float32; every scalar that meets a field is first rounded to the field's type, so an fp32 level is computed in fp32 throughout.
NumPy evaluates each ufunc on its own (no fused multiply-add), which is what the library's -ffp-contract=off gives."""
import math

import numpy as np

INT = (slice(1, -1),) * 3


def spacings(shape, domain=(0.0, 1.0, 0.0, 1.0, 0.0, 1.0)):
    return tuple((domain[2 * a + 1] - domain[2 * a]) / (shape[a] - 1) for a in range(3))


def coefs(h, sigma, omega, dtype):
    """ihx2, ihy2, ihz2, diag, w: formed in double, rounded to dtype"""
    hx, hy, hz = (float(x) for x in h)
    ihx2, ihy2, ihz2 = 1.0 / (hx * hx), 1.0 / (hy * hy), 1.0 / (hz * hz)
    diag = ((2.0 * ihx2 + 2.0 * ihy2) + 2.0 * ihz2) + float(sigma)
    T = np.dtype(dtype).type
    return T(ihx2), T(ihy2), T(ihz2), T(diag), T(float(omega) / diag)


def _r_interior(u, f, h, sigma, omega=1.0):
    ihx2, ihy2, ihz2, diag, w = coefs(h, sigma, omega, u.dtype)
    c = u[1:-1, 1:-1, 1:-1]
    nb = ((ihx2 * (u[:-2, 1:-1, 1:-1] + u[2:, 1:-1, 1:-1])) + (ihy2 * (u[1:-1, :-2, 1:-1] + u[1:-1, 2:, 1:-1]))) + \
         (ihz2 * (u[1:-1, 1:-1, :-2] + u[1:-1, 1:-1, 2:]))
    return f[1:-1, 1:-1, 1:-1] - (diag * c - nb), c, w


def residual(u, f, h, sigma=0.0):
    """r = f - A u on interior cells, 0 on the faces"""
    r = np.zeros_like(u)
    r[INT] = _r_interior(u, f, h, sigma)[0]
    return r


def apply(u, h, sigma=0.0):
    """A u on interior cells (0 on the faces)"""
    return -residual(u, np.zeros_like(u), h, sigma)


def jacobi(u, f, h, sigma, omega):
    r, c, w = _r_interior(u, f, h, sigma, omega)
    out = u.copy()
    out[INT] = c + w * r
    return out


def colour_mask(shape, colour, offset=0):
    i, j, k = np.meshgrid(*(np.arange(1, n - 1) for n in shape), indexing="ij")
    return ((i + j + k + offset) & 1) == colour


def colour_pass(u, f, h, sigma, omega, colour, offset=0):
    r, c, w = _r_interior(u, f, h, sigma, omega)
    out = u.copy()
    out[INT] = np.where(colour_mask(u.shape, colour, offset), c + w * r, c)
    return out


def rbgs(u, f, h, sigma, omega, sweeps=1):
    for _ in range(sweeps):
        u = colour_pass(colour_pass(u, f, h, sigma, omega, 0), f, h, sigma, omega, 1)
    return u


def coarse_solve(u, f, h, sigma, sweeps=64):
    return rbgs(u, f, h, sigma, 1.0, sweeps)


def _m(a, b, c):
    T = b.dtype.type
    return T(0.5) * b + T(0.25) * (a + c)


def restrict(r):
    """27-point full weighting onto the interior coarse cells (0 on the coarse faces): along k, then j, then i"""
    p = _m(r[:, :, 1:-2:2], r[:, :, 2:-1:2], r[:, :, 3::2])
    q = _m(p[:, 1:-2:2], p[:, 2:-1:2], p[:, 3::2])
    c = _m(q[1:-2:2], q[2:-1:2], q[3::2])
    out = np.zeros(tuple((n + 1) // 2 for n in r.shape), dtype=r.dtype)
    out[INT] = c
    return out


def interpolate(e):
    """trilinear P e on the whole fine grid: the 1/2 averages along k, then j, then i"""
    T = e.dtype.type
    nxc, nyc, nzc = e.shape
    a = np.empty((nxc, nyc, 2 * nzc - 1), dtype=e.dtype)
    a[:, :, 0::2] = e
    a[:, :, 1::2] = T(0.5) * (e[:, :, :-1] + e[:, :, 1:])
    b = np.empty((nxc, 2 * nyc - 1, 2 * nzc - 1), dtype=e.dtype)
    b[:, 0::2] = a
    b[:, 1::2] = T(0.5) * (a[:, :-1] + a[:, 1:])
    t = np.empty((2 * nxc - 1, 2 * nyc - 1, 2 * nzc - 1), dtype=e.dtype)
    t[0::2] = b
    t[1::2] = T(0.5) * (b[:-1] + b[1:])
    return t


def prolong_add(u, e):
    out = u.copy()
    out[INT] = u[INT] + interpolate(e)[INT]
    return out


def sumsq(x):
    return math.fsum((x.astype(np.float64).ravel() ** 2).tolist())


def norm(r, h):
    """sqrt(hx hy hz sum r^2) over interior cells"""
    return math.sqrt(h[0] * h[1] * h[2] * sumsq(r[INT]))


def hierarchy(shape, max_levels):
    shapes = [tuple(shape)]
    while len(shapes) < max_levels and all(n % 2 == 1 and n >= 5 for n in shapes[-1]):
        shapes.append(tuple((n + 1) // 2 for n in shapes[-1]))
    return shapes


class Config:
    def __init__(self, domain=(0.0, 1.0, 0.0, 1.0, 0.0, 1.0), sigma=0.0, max_levels=10, cycle="V", pre=2, post=2, smoother="jacobi",
                 omega=None, coarse_sweeps=64):
        self.domain, self.sigma, self.max_levels, self.cycle, self.pre, self.post = domain, sigma, max_levels, cycle, pre, post
        self.smoother, self.coarse_sweeps = smoother, coarse_sweeps
        self.omega = (0.8 if smoother == "jacobi" else 1.0) if omega is None else omega


def smooth(u, f, h, cfg, sweeps):
    for _ in range(sweeps):
        u = jacobi(u, f, h, cfg.sigma, cfg.omega) if cfg.smoother == "jacobi" else rbgs(u, f, h, cfg.sigma, cfg.omega)
    return u


def cycle(u, f, cfg, shapes=None, level=0):
    """one cycle on `level`; returns the new iterate"""
    shapes = shapes or hierarchy(u.shape, cfg.max_levels)
    h = spacings(shapes[level], cfg.domain)
    if level == len(shapes) - 1:
        return coarse_solve(u, f, h, cfg.sigma, cfg.coarse_sweeps)
    u = smooth(u, f, h, cfg, cfg.pre)
    fc = restrict(residual(u, f, h, cfg.sigma))
    e = np.zeros(shapes[level + 1], dtype=u.dtype)
    for _ in range(2 if cfg.cycle == "W" else 1):
        e = cycle(e, fc, cfg, shapes, level + 1)
    u = prolong_add(u, e)
    return smooth(u, f, h, cfg, cfg.post)


def residual_norm(u, f, cfg):
    h = spacings(u.shape, cfg.domain)
    return norm(residual(u, f, h, cfg.sigma), h)


def defect_step(u, f, cfg):
    """u, f fp64: r32 = fp32(f - A u), ONE fp32 cycle from zero, u += (double)e"""
    h = spacings(u.shape, cfg.domain)
    r32 = residual(u, f, h, cfg.sigma).astype(np.float32)
    e = cycle(np.zeros(u.shape, dtype=np.float32), r32, cfg)
    out = u.copy()
    out[INT] = u[INT] + e[INT].astype(np.float64)
    return out


def defect_step_with_residual(u, r32, cfg):
    """the defect step's second half with a GIVEN fp32 right-hand side: ONE fp32 cycle for A e = r32 from zero, u += (double)e.
    With r32 = fp32(f - A u) it is defect_step; with the residual of an earlier f or u it models a handle whose cached residual
    was not marked out of date"""
    e = cycle(np.zeros(u.shape, dtype=np.float32), r32, cfg)
    out = u.copy()
    out[INT] = u[INT] + e[INT].astype(np.float64)
    return out


def solve(u, f, cfg, tol, max_iter, defect=False):
    """mg3_solve's loop: returns (u, history, converged)"""
    hist = [residual_norm(u, f, cfg)]
    while not hist[-1] < tol and len(hist) - 1 < max_iter:
        u = defect_step(u, f, cfg) if defect else cycle(u, f, cfg)
        hist.append(residual_norm(u, f, cfg))
    return u, hist, hist[-1] < tol


def mesh(shape, domain=(0.0, 1.0, 0.0, 1.0, 0.0, 1.0)):
    axes = [np.linspace(domain[2 * a], domain[2 * a + 1], shape[a]) for a in range(3)]
    return np.meshgrid(*axes, indexing="ij")
