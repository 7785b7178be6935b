"""NumPy restatement of the fourth-order compact nine-point scheme (include/mghip_ho.h, csrc/mg_ho_kernels.hpp): the right-hand
side average R, the operator A4 and the residual, with exactly the association the kernels use, and the conjugate-gradient
loop of tests/pcg_reference.py with A4 and g = R f swapped in (the preconditioner stays the five-point oracle cycle).  What
tests/test_ho_cpu.py pins and tests/test_gpu_ho.py compares the device against.  Not a test.  Plain Python + NumPy; every
function works on the last two axes, so a stack of fields goes through in one call."""
import numpy as np

import pcg_reference as R


def coefficients(hx, hy, sigma=0.0):
    """(cC, cE, cN, cK) in the forms the host code computes them in"""
    ca = 1.0 / (hx * hx)
    cb = 1.0 / (hy * hy)
    cC = (5.0 / 3.0) * (ca + cb) + sigma * (8.0 / 12.0)
    cE = (cb - 5.0 * ca) / 6.0 + sigma / 12.0
    cN = (ca - 5.0 * cb) / 6.0 + sigma / 12.0
    cK = (ca + cb) / 12.0
    return cC, cE, cN, cK


def _zero_ring(v):
    v = v.copy()
    v[..., 0, :] = v[..., -1, :] = 0
    v[..., :, 0] = v[..., :, -1] = 0
    return v


def rhs_average(f):
    """g = R f on interior cells, the ring of f on the ring"""
    f = np.asarray(f, dtype=np.float64)
    g = f.copy()
    C = f[..., 1:-1, 1:-1]
    dn, up = f[..., 2:, 1:-1], f[..., :-2, 1:-1]
    ea, w = f[..., 1:-1, 2:], f[..., 1:-1, :-2]
    g[..., 1:-1, 1:-1] = (8.0 * C + ((dn + up) + (ea + w))) / 12.0
    return g


def apply_A4(u, hx, hy, coeff=-1.0, sigma=0.0):
    """A4 u on interior cells (the ring of u, corners included, is read), 0 on the ring"""
    u = np.asarray(u, dtype=np.float64)
    cC, cE, cN, cK = coefficients(hx, hy, sigma)
    C = u[..., 1:-1, 1:-1]
    dn, up = u[..., 2:, 1:-1], u[..., :-2, 1:-1]
    ea, w = u[..., 1:-1, 2:], u[..., 1:-1, :-2]
    dn_e, dn_w = u[..., 2:, 2:], u[..., 2:, :-2]
    up_e, up_w = u[..., :-2, 2:], u[..., :-2, :-2]
    out = np.zeros_like(u)
    out[..., 1:-1, 1:-1] = (-coeff) * (((cC * C + cE * (dn + up)) + cN * (ea + w)) - cK * ((dn_e + dn_w) + (up_e + up_w)))
    return out


def residual(x, g, hx, hy, coeff=-1.0, sigma=0.0):
    """g - A4 x on interior cells, 0 on the ring"""
    r = np.zeros_like(np.asarray(g, dtype=np.float64))
    r[..., 1:-1, 1:-1] = (g - apply_A4(x, hx, hy, coeff, sigma))[..., 1:-1, 1:-1]
    return r


def apply_A2(u, hx, hy, coeff=-1.0, sigma=0.0):
    """the five-point operator in the same shape (for the order-2 comparison of the direct solves)"""
    u = np.asarray(u, dtype=np.float64)
    C = u[..., 1:-1, 1:-1]
    out = np.zeros_like(u)
    lap = (u[..., 2:, 1:-1] + u[..., :-2, 1:-1] - 2.0 * C) / (hx * hx) + (u[..., 1:-1, 2:] + u[..., 1:-1, :-2] - 2.0 * C) / (hy * hy)
    out[..., 1:-1, 1:-1] = coeff * (lap - sigma * C)
    return out


def dense_matrix(nx, ny, hx, hy, coeff=-1.0, sigma=0.0, apply=apply_A4):
    """the operator on the (nx - 2)(ny - 2) interior unknowns (zero ring), row-major"""
    n = (nx - 2) * (ny - 2)
    basis = np.zeros((n, nx, ny))
    basis[:, 1:-1, 1:-1] = np.eye(n).reshape(n, nx - 2, ny - 2)
    cols = apply(basis, hx, hy, coeff, sigma)[:, 1:-1, 1:-1].reshape(n, n)
    return np.ascontiguousarray(cols.T)


def manufactured(nx, ny, sigma=0.0):
    """u = e^x sin(2 y + 0.3) on the unit square and f = -Laplace u + sigma u = (3 + sigma) u"""
    x, y = np.linspace(0.0, 1.0, nx), np.linspace(0.0, 1.0, ny)
    X, Y = np.meshgrid(x, y, indexing="ij")
    u = np.exp(X) * np.sin(2.0 * Y + 0.3)
    return u, (3.0 + sigma) * u


def direct_error(nx, ny, sigma=0.0, order=4):
    """max error of a dense direct solve of the manufactured problem (Dirichlet ring from u)"""
    u, f = manufactured(nx, ny, sigma)
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    apply = apply_A4 if order == 4 else apply_A2
    g = rhs_average(f) if order == 4 else f
    ring = u.copy()
    ring[1:-1, 1:-1] = 0.0
    b = (g - apply(ring, hx, hy, -1.0, sigma))[1:-1, 1:-1].ravel()
    sol = np.linalg.solve(dense_matrix(nx, ny, hx, hy, -1.0, sigma, apply), b)
    return float(np.max(np.abs(sol.reshape(nx - 2, ny - 2) - u[1:-1, 1:-1])))


def pcg(mgo, f, u0=None, tol=1e-8, max_iterations=50, flexible=False, pm=None, num_cycles=1):
    """pcg_reference.pcg for A4 u = R f: -> (u, info).  The norm is sqrt(hx hy (sum of r^2 over interior cells)) with
    r = R f - A4 x; the ring of f is data of the scheme and does not enter it."""
    hx, hy = mgo.h[0]
    coeff, sigma = mgo.coeff, mgo.shift
    f = np.asarray(f, dtype=np.float64)
    x = np.zeros_like(f) if u0 is None else np.array(u0, dtype=np.float64)
    g = rhs_average(f)
    norm = lambda r: float(np.sqrt(hx * hy * np.sum(r * r)))
    r = residual(x, g, hx, hy, coeff, sigma)
    initial = norm(r)
    hist, status, converged = [], "max_iterations", False
    p = q = None
    rz = alpha = 0.0
    if initial < tol:
        status, converged = "converged", True
    else:
        for k in range(max_iterations):
            z = R.apply_M(mgo, r, pm, num_cycles)
            rz_new = float(np.sum(r * z))
            if k == 0:
                p = z.copy()
            else:
                beta = -alpha * float(np.sum(z * q)) / rz if flexible else rz_new / rz
                p = _zero_ring(z + beta * p)
            rz = rz_new
            q = apply_A4(p, hx, hy, coeff, sigma)
            pq = float(np.sum(p * q))
            if not (pq > 0.0) or not np.isfinite(pq):
                status = "breakdown"
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * q
            hist.append(norm(r))
            if hist[-1] < tol:
                status, converged = "converged", True
                break
    true = norm(residual(x, g, hx, hy, coeff, sigma))
    return x, {"iterations": len(hist), "converged": converged, "residual_history": hist,
               "final_residual": hist[-1] if hist else initial, "true_residual": true, "initial_residual": initial,
               "status": status, "flexible": bool(flexible), "order": 4}
