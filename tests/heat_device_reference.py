"""NumPy restatement of one device-resident heat step (include/mghip.h "Time stepping", csrc/mg_heat.hip) -- not a test.

The right-hand sides are the header's formulas in the header's association, on oracle.mg_oracle.apply_laplacian; the ring
is written in the host stepper's order; the solve is MGOracle(shift = lambda).solve from the step's initial guess; BDF2 is
started with one Crank-Nicolson step; step doubling is the host stepper's.  tests/test_heat_device_cpu.py pins this file to
oracle.heat_oracle (itself pinned to the reference's outputs) and to tests/golden/heat.npz."""
import os
import sys

import numpy as np

from oracle import mg_oracle as O
from oracle.heat_oracle import HeatOracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from heat_inputs import heat_cases, heat_config                                   # noqa: E402

EXPLICIT, IMPLICIT, CN, BDF2 = "explicit_euler", "implicit_euler", "crank_nicolson", "bdf2"
SCHEME_CODES = {EXPLICIT: 0, IMPLICIT: 1, CN: 2, BDF2: 3}


def lam(scheme, dt, a):
    return {IMPLICIT: 1.0 / (dt * a), CN: 2.0 / (dt * a), BDF2: 3.0 / (2 * dt * a)}[scheme]


def rhs(scheme, u, dt, a, hx, hy, u_prev=None, S=None, g0=1.0, g1=1.0):
    """what mg_dev_heat_rhs stores: f with a zero ring for the implicit schemes, the whole explicit step with the ring of u"""
    S = np.zeros_like(u) if S is None else S
    lap = O.apply_laplacian(u, hx, hy, 1.0)
    if scheme == EXPLICIT:
        val = u + dt * ((a * lap) + g0 * S)
        out = u.copy()
    elif scheme == IMPLICIT:
        val = (u + dt * (g1 * S)) / (dt * a)
        out = np.zeros_like(u)
    elif scheme == CN:
        val = (2.0 * ((u + ((dt * a) * lap) / 2) + (dt * ((g0 * S) + (g1 * S))) / 2)) / (dt * a)
        out = np.zeros_like(u)
    elif scheme == BDF2:
        val = (4.0 * u - u_prev) / (2 * dt * a) + (g1 * S) / a
        out = np.zeros_like(u)
    else:
        raise ValueError(scheme)
    out[1:-1, 1:-1] = val[1:-1, 1:-1]
    return out


def set_ring(u, edge4):
    """left (i = 0), right (i = nx - 1), bottom (j = 0), top (j = ny - 1), in this order: corners carry bottom / top"""
    u[0, :] = edge4[0]
    u[-1, :] = edge4[1]
    u[:, 0] = edge4[2]
    u[:, -1] = edge4[3]
    return u


def step(scheme, u, dt, a, domain=(0.0, 1.0, 0.0, 1.0), u_prev=None, S=None, g0=1.0, g1=1.0, edge4=None, bc_before_solve=False,
         tol=1e-10, max_cycles=20, smoother="jacobi", omega=0.8, max_levels=32, oracle_cls=None):
    """one step: (u_new, info) with info = lambda, rhs_norm, final_residual, cycles; oracle_cls: the hierarchy's class (None: the pinned
    MGOracle, looked up at the call; or tests/coarse_exact_reference.ExactCoarseOracle)"""
    nx, ny = u.shape
    hx, hy = O.grid_spacing(nx, ny, domain)
    if scheme == EXPLICIT:
        out = rhs(EXPLICIT, u, dt, a, hx, hy, S=S, g0=g0)
        if edge4 is not None:
            set_ring(out, edge4)
        return out, {"lambda": 0.0, "rhs_norm": 0.0, "final_residual": 0.0, "cycles": 0}
    f = rhs(scheme, u, dt, a, hx, hy, u_prev, S, g0, g1)
    lm = lam(scheme, dt, a)
    guess = u.copy()
    if bc_before_solve:
        set_ring(guess, edge4)
    fnorm = float(np.sqrt(hx * hy * np.sum(f * f)))
    mgo = (oracle_cls or O.MGOracle)(nx, ny, domain=domain, max_levels=max_levels, cycle="V", pre=2, post=2, smoother=smoother, omega=omega, shift=lm)
    out, info = mgo.solve(f, guess, tol=tol * max(1.0, fnorm), max_iterations=max_cycles)
    if not bc_before_solve and edge4 is not None:
        set_ring(out, edge4)
    return out, {"lambda": lm, "rhs_norm": fnorm, "final_residual": info["final_residual"], "cycles": info["iterations"]}


def bdf2_run(u0, dt, a, nsteps, **kw):
    """fixed-dt BDF2: the first step is Crank-Nicolson (self-starting, second order), the rest BDF2 on the last two levels"""
    levels = [u0]
    for k in range(nsteps):
        if k == 0:
            levels.append(step(CN, levels[-1], dt, a, **kw)[0])
        else:
            levels.append(step(BDF2, levels[-1], dt, a, u_prev=levels[-2], **kw)[0])
    return levels


def adaptive_step(scheme, u, dt, a, error_tolerance, stepper):
    """step doubling (applications/heat_equation.py:268-330); stepper(u, dt) -> u_new, all three steps of an attempt at the
    time of u (the reference's clock stands still inside an attempt)"""
    u_full = u
    for _ in range(10):
        u_full = stepper(u, dt)
        u_half = stepper(stepper(u, dt / 2), dt / 2)
        if scheme in (EXPLICIT, IMPLICIT):
            err, order = np.linalg.norm(u_half - u_full), 1
        else:
            err, order = np.linalg.norm(u_half - u_full) / 3.0, 2
        if err < error_tolerance:
            return u_half, dt
        dt = max(dt / 4, dt * 0.8 * (error_tolerance / err) ** (1 / (order + 1)))
    return u_full, dt


_CONVERGED = {}


def converged_oracle_step(name, k, golden, mod):
    """step k of golden case `name` by HeatOracle(sweeps=20000) -- the reference's relaxation run to convergence -- from the
    golden state u_k; `mod` provides the configuration classes.  20000 sweeps take a minute: computed once per session and
    shared by the tests that compare against it (CPU: the restatement, GPU: the device path)."""
    if (name, k) not in _CONVERGED:
        n, alpha, scheme, _, _, bc_kind, with_source = heat_cases()[name]
        dt = float(golden[f"{name}__dt"])
        conv = HeatOracle(heat_config(mod, alpha, bc_kind, with_source), n, n, sweeps=20000)
        conv.set_initial_condition(golden[f"{name}__u0"])
        conv.t = k * dt
        _CONVERGED[(name, k)] = conv.step(golden[f"{name}__u{k}"].copy(), dt, scheme)
    return _CONVERGED[(name, k)]
