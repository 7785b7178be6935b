"""NumPy restatement of the device-resident conjugate-gradient loop (csrc/mg_pcg.hip), built from the pinned oracle
(oracle/mg_oracle.py): A is apply_laplacian / var_residual with f = 0 on a zeroed ring, M is `num_cycles` calls of
MGOracle / VarMGOracle.cycle_once from zero, beta is Fletcher-Reeves or the flexible -alpha (z.q) / (r.z)_old.  What
tests/test_pcg_cpu.py pins and tests/test_gpu_pcg.py compares the device against.  Plain Python + NumPy."""
import numpy as np

from oracle import mg_oracle as O


def zero_ring(v):
    v = v.copy()
    v[0, :] = v[-1, :] = v[:, 0] = v[:, -1] = 0
    return v


def ring_sumsq(f):
    return float(np.sum(f[0, :]**2) + np.sum(f[-1, :]**2) + np.sum(f[1:-1, 0]**2) + np.sum(f[1:-1, -1]**2))


def full_levels(nx, ny):
    """levels down to the coarsest grid the hierarchy rules allow (5 points on the shorter side of a 2^k + 1 grid)"""
    return max(1, int(np.log2(min(nx, ny) - 1)) - 1)


def checkerboard(nx, ny, blocks=8, contrast=1e4):
    x, y = np.linspace(0, 1, nx), np.linspace(0, 1, ny)
    X, Y = np.meshgrid(x, y, indexing="ij")
    a = np.ones((nx, ny))
    a[(np.floor(X * blocks) + np.floor(Y * blocks)) % 2 == 0] = contrast
    return a


def smooth_coefficient(nx, ny):
    x, y = np.linspace(0, 1, nx), np.linspace(0, 1, ny)
    X, Y = np.meshgrid(x, y, indexing="ij")
    return 1 + 0.5 * np.sin(2 * np.pi * X) * np.cos(2 * np.pi * Y)


def random_rhs(nx, ny, seed=0):
    return zero_ring(np.random.default_rng(seed).standard_normal((nx, ny)))


def make_oracle(nx, ny, a=None, pre=1, post=1, smoother="jacobi", omega=0.8, cycle="V", max_levels=None, shift=0.0,
                domain=(0.0, 1.0, 0.0, 1.0), oracle_classes=None):
    """oracle_classes: (constant-coefficient class, variable-coefficient class) to build the hierarchy from -- None: the pinned
    MGOracle / VarMGOracle; tests/coarse_exact_reference.py has the pair with an exact coarsest solve"""
    const_cls, var_cls = oracle_classes or (O.MGOracle, O.VarMGOracle)
    kw = dict(domain=domain, max_levels=max_levels or full_levels(nx, ny), cycle=cycle, pre=pre, post=post, smoother=smoother,
              omega=omega, jacobi_form="vectorized", shift=shift)
    return const_cls(nx, ny, **kw) if a is None else var_cls(np.asarray(a, dtype=np.float64), **kw)


def precision_manager(precision):
    """the oracle's precision manager for a preconditioner precision of PCGSolver"""
    return {"double": None, "single_managed": O.OraclePrecision("single", adaptive=False), "mixed": O.OraclePrecision("mixed")}[precision]


def apply_A(mgo, v):
    """A v on interior cells, 0 on the ring, for v with a zero ring"""
    hx, hy = mgo.h[0]
    if isinstance(mgo, O.VarMGOracle):
        return zero_ring(-O.var_residual(v, np.zeros_like(v), mgo.a_of(0, np.float64), hx, hy, mgo.coeff, mgo.shift))
    return O.apply_laplacian(v, hx, hy, mgo.coeff, mgo.shift)


def residual(mgo, u, f):
    """f - A u with the project's ring convention (r = f on the ring)"""
    hx, hy = mgo.h[0]
    if isinstance(mgo, O.VarMGOracle):
        return O.var_residual(u, f, mgo.a_of(0, np.float64), hx, hy, mgo.coeff, mgo.shift)
    return O.residual(u, f, hx, hy, mgo.coeff, mgo.shift)


def apply_M(mgo, r, pm=None, num_cycles=1):
    mgo.rhs[0] = r.copy()
    u = np.zeros_like(r)
    for _ in range(num_cycles):
        u = mgo.cycle_once(u, 0, pm)
    return np.asarray(u, dtype=np.float64)


def default_flexible(smoother, pre, post):
    return smoother != "jacobi" or pre != post


def pcg(mgo, f, u0=None, tol=1e-8, max_iterations=50, flexible=False, pm=None, num_cycles=1):
    """-> (u, info).  The norm is sqrt(hx hy (sum of r^2 over interior cells + sum of f^2 over the ring)), compared as
    norm < tol; residual_history[k] is the norm after iteration k + 1."""
    hx, hy = mgo.h[0]
    f = np.asarray(f, dtype=np.float64)
    x = np.zeros_like(f) if u0 is None else np.array(u0, dtype=np.float64)
    ring = ring_sumsq(f)
    norm = lambda r: float(np.sqrt(hx * hy * (np.sum(r * r) + ring)))
    r = zero_ring(residual(mgo, x, f))
    initial = norm(r)
    hist, status, converged = [], "max_iterations", False
    p = q = None
    rz = alpha = 0.0
    if initial < tol:
        status, converged = "converged", True
    else:
        for k in range(max_iterations):
            z = apply_M(mgo, r, pm, num_cycles)
            rz_new = float(np.sum(r * z))
            if k == 0:
                p = z.copy()
            else:
                beta = -alpha * float(np.sum(z * q)) / rz if flexible else rz_new / rz
                p = z + beta * p
            rz = rz_new
            q = apply_A(mgo, p)
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
    true = float(O.l2_norm(residual(mgo, x, f), hx, hy))
    return x, {"iterations": len(hist), "converged": converged, "residual_history": hist,
               "final_residual": hist[-1] if hist else initial, "true_residual": true, "initial_residual": initial,
               "status": status, "flexible": bool(flexible)}


def plain_multigrid(mgo, f, tol, max_cycles):
    """cycles of the plain multigrid iteration until ||r|| < tol -> (cycles or None, last norm)"""
    hx, hy = mgo.h[0]
    u = np.zeros_like(f)
    rn = float("inf")
    for it in range(1, max_cycles + 1):
        mgo.rhs[0] = f.copy()
        u = mgo.cycle_once(u, 0)
        rn = float(O.l2_norm(residual(mgo, u, f), hx, hy))
        if not np.isfinite(rn):
            return None, rn
        if rn < tol:
            return it, rn
    return None, rn
