"""NumPy restatement of one device-resident heat step with a diffusivity field,  du/dt = alpha div(a grad u) + g(t) S
(include/mghip_heat.h "Variable diffusivity", "Inner solver"; csrc/mg_heat.hip) -- not a test.

Everything is tests/heat_device_reference.py with the Laplacian replaced by  L_a u = -var_residual(u, 0, a, coeff = +1, shift = 0)
on interior cells (oracle/mg_oracle.py: the engine's variable-coefficient discretisation, faces = arithmetic means); the solve
is VarMGOracle(shift = lambda).solve from the step's initial guess (inner="cycle"), or tests/pcg_reference.pcg on
make_oracle(a = a, shift = lambda) from the same guess (inner="pcg"; pm is the preconditioner's precision manager).
tests/test_heat_var_cpu.py pins this file."""
import os
import sys

import numpy as np

from oracle import mg_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heat_device_reference as R                                                 # noqa: E402
import pcg_reference as P                                                         # noqa: E402

EXPLICIT, IMPLICIT, CN, BDF2 = R.EXPLICIT, R.IMPLICIT, R.CN, R.BDF2


def apply_La(u, a, hx, hy):
    """div(a grad u) on interior cells, 0 on the ring"""
    return P.zero_ring(-O.var_residual(u, np.zeros_like(u), a, hx, hy, 1.0, 0.0))


def rhs_var(scheme, u, dt, alpha, a, hx, hy, u_prev=None, S=None, g0=1.0, g1=1.0):
    """what mg_dev_heat_rhs_var stores: heat_device_reference.rhs with lap = L_a u"""
    S = np.zeros_like(u) if S is None else S
    lap = apply_La(u, a, hx, hy)
    if scheme == EXPLICIT:
        val = u + dt * ((alpha * lap) + g0 * S)
        out = u.copy()
    elif scheme == IMPLICIT:
        val = (u + dt * (g1 * S)) / (dt * alpha)
        out = np.zeros_like(u)
    elif scheme == CN:
        val = (2.0 * ((u + ((dt * alpha) * lap) / 2) + (dt * ((g0 * S) + (g1 * S))) / 2)) / (dt * alpha)
        out = np.zeros_like(u)
    elif scheme == BDF2:
        val = (4.0 * u - u_prev) / (2 * dt * alpha) + (g1 * S) / alpha
        out = np.zeros_like(u)
    else:
        raise ValueError(scheme)
    out[1:-1, 1:-1] = val[1:-1, 1:-1]
    return out


def inner_oracle(a, lm, domain=(0.0, 1.0, 0.0, 1.0), smoother="jacobi", omega=0.8, max_levels=32, oracle_cls=None):
    """the stepper's inner hierarchy: V(2, 2) of -div(a grad) + lambda; oracle_cls: its class (None: the pinned VarMGOracle; or
    tests/coarse_exact_reference.ExactCoarseVarOracle)"""
    return (oracle_cls or O.VarMGOracle)(np.asarray(a, dtype=np.float64), domain=domain, max_levels=max_levels, cycle="V", pre=2, post=2,
                         smoother=smoother, omega=omega, shift=lm)


def step_var(scheme, u, dt, alpha, a, domain=(0.0, 1.0, 0.0, 1.0), u_prev=None, S=None, g0=1.0, g1=1.0, edge4=None,
             bc_before_solve=False, tol=1e-10, max_cycles=20, smoother="jacobi", omega=0.8, max_levels=32, inner="cycle", pm=None,
             flexible=None, oracle_cls=None):
    """one step: (u_new, info) with info = lambda, rhs_norm, final_residual, cycles, converged"""
    nx, ny = u.shape
    hx, hy = O.grid_spacing(nx, ny, domain)
    if scheme == EXPLICIT:
        out = rhs_var(EXPLICIT, u, dt, alpha, a, hx, hy, S=S, g0=g0)
        if edge4 is not None:
            R.set_ring(out, edge4)
        return out, {"lambda": 0.0, "rhs_norm": 0.0, "final_residual": 0.0, "cycles": 0, "converged": True}
    f = rhs_var(scheme, u, dt, alpha, a, hx, hy, u_prev, S, g0, g1)
    lm = R.lam(scheme, dt, alpha)
    guess = u.copy()
    if bc_before_solve:
        R.set_ring(guess, edge4)
    fnorm = float(np.sqrt(hx * hy * np.sum(f * f)))
    mgo = inner_oracle(a, lm, domain, smoother, omega, max_levels, oracle_cls)
    if inner == "cycle":
        out, info = mgo.solve(f, guess, tol=tol * max(1.0, fnorm), max_iterations=max_cycles)
        final, cycles, conv = info["final_residual"], info["iterations"], info["converged"]
    elif inner == "pcg":
        flex = P.default_flexible(smoother, 2, 2) if flexible is None else flexible
        out, info = P.pcg(mgo, f, guess, tol=tol * max(1.0, fnorm), max_iterations=max_cycles, flexible=flex, pm=pm)
        final, cycles, conv = info["final_residual"], info["iterations"], info["converged"]
    else:
        raise ValueError(inner)
    if not bc_before_solve and edge4 is not None:
        R.set_ring(out, edge4)
    return out, {"lambda": lm, "rhs_norm": fnorm, "final_residual": final, "cycles": cycles, "converged": conv}


def dense_operator(a, hx, hy):
    """-L_a on the interior unknowns as a dense matrix (rows and columns in C order of the interior cells); small grids only"""
    nx, ny = a.shape
    n = (nx - 2) * (ny - 2)
    A = np.zeros((n, n))
    e = np.zeros((nx, ny))
    for k in range(n):
        i, j = 1 + k // (ny - 2), 1 + k % (ny - 2)
        e[i, j] = 1.0
        A[:, k] = -apply_La(e, a, hx, hy)[1:-1, 1:-1].ravel()
        e[i, j] = 0.0
    return A


def dense_step(scheme, u, dt, alpha, a, A, hx, hy, u_prev=None, S=None, g0=1.0, g1=1.0):
    """one implicit step with the inner system (A + lambda) u = f solved exactly (homogeneous Dirichlet ring kept from u)"""
    f = rhs_var(scheme, u, dt, alpha, a, hx, hy, u_prev, S, g0, g1)
    lm = R.lam(scheme, dt, alpha)
    b = f[1:-1, 1:-1].copy()
    # the ring of u enters the interior equations through the faces next to the boundary
    ring = u.copy()
    ring[1:-1, 1:-1] = 0.0
    b += apply_La(ring, a, hx, hy)[1:-1, 1:-1]
    out = u.copy()
    out[1:-1, 1:-1] = np.linalg.solve(A + lm * np.eye(A.shape[0]), b.ravel()).reshape(b.shape)
    return out
