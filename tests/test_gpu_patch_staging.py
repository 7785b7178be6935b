"""Staging of the coarse patch in the register-blocked up legs and the spanning leg (csrc/mg_rb_kernels.hpp PatchStage): all
of a thread's patch loads in one round trip, ahead of the strip loads.  fused = 3 puts the register-blocked legs -- with
speculate = 2 the spanning leg -- on every level, so small grids reach the code; the LDS-tiled two-launch form (fused = 1,
speculate = 1) is the reference: same arithmetic per cell, so the iterates are the same bits; the norm's partial sums run
over other tiles, so histories agree to the last bits only (rtol 1e-12, as in test_gpu_span.py).

Shapes, rectangular on purpose: 161 x 353 (fp64; 6 levels) and 193 x 705 (fp32 working precisions; 7 levels) -- the
smallest grids with an interior workgroup and rim workgroups on all four sides for both the 8 x 8 spanning strip (tile 52 x 112
fp64, 52 x 224 fp32) and the 4 x 8 up leg, patches that hang over every edge of the coarse grid, a partly filled last
staging trip (2244 / 4420 entries on 512 threads, 1188 / 2340 on 256) and at least three levels below the finest."""
import functools

import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib

pytestmark = pytest.mark.gpu

SHAPE64 = (161, 353)
SHAPE32 = (193, 705)
PRECS = [_lib.MG_PREC_DOUBLE, _lib.MG_PREC_SINGLE, _lib.MG_PREC_SINGLE_MANAGED, _lib.MG_PREC_ADAPTIVE]
STAGED = dict(fused=3, speculate=2)          # register-blocked legs + spanning leg on every level
TILED = dict(fused=1, speculate=1)           # LDS-tiled legs, up leg and down leg in two launches


def _shape(prec):
    return SHAPE64 if prec == _lib.MG_PREC_DOUBLE else SHAPE32


def _rhs(nx, ny):
    x = np.linspace(0.0, 1.0, nx); y = np.linspace(0.0, 1.0, ny)
    rng = np.random.default_rng(nx + ny)
    return 2 * np.pi**2 * np.sin(np.pi * x)[:, None] * np.sin(2 * np.pi * y)[None, :] + 0.05 * rng.standard_normal((nx, ny))


def _run(shape, prec, mode, tol, its, u0=None, smoother=_lib.MG_JACOBI, omega=0.8):
    nx, ny = shape
    assert mg.default_max_levels(nx, ny) >= 4            # span_ok: at least three levels below the finest
    eng = mg.MultigridEngine(nx, ny, max_levels=mg.default_max_levels(nx, ny), smoother=smoother, omega=omega, precision=prec, **mode)
    f = _rhs(nx, ny)
    if prec == _lib.MG_PREC_SINGLE:
        f = f.astype(np.float32)
    eng.set_rhs(f)
    eng.set_solution(u0)
    r = eng.iterate(tol, its)
    u = eng.get_solution()
    eng.close()
    return u, r


@functools.lru_cache(maxsize=None)
def _tiled_fixed(prec):
    """the reference of a precision, computed once: three cycles at tol = 0 in the two-launch LDS-tiled form"""
    u, r = _run(_shape(prec), prec, TILED, 0.0, 3)
    u.setflags(write=False)
    return u, r


@pytest.mark.parametrize("prec", PRECS)
def test_fixed_cycles_equal_the_lds_tiled_two_launch_form(prec):
    """tol = 0: the spanning leg does not store the iterate between two cycles (SPAN 2)"""
    u1, r1 = _tiled_fixed(prec)
    u2, r2 = _run(_shape(prec), prec, STAGED, 0.0, 3)
    assert np.array_equal(u1, u2)
    np.testing.assert_allclose(r2["residual_history"], r1["residual_history"], rtol=1e-12)
    assert r1["precision_codes"] == r2["precision_codes"]


@pytest.mark.parametrize("prec", PRECS)
def test_stopping_on_the_tolerance_equals_the_lds_tiled_two_launch_form(prec):
    """a tolerance met at the second or third cycle: the iterate returned is the one the spanning leg stored in between (SPAN 1)"""
    h = _tiled_fixed(prec)[1]["residual_history"]
    tol = 1.5 * h[2]                                      # met by the norm of the third cycle at the latest
    assert h[0] > tol                                     # ... and not by the first
    u1, r1 = _run(_shape(prec), prec, TILED, tol, 8)
    u2, r2 = _run(_shape(prec), prec, STAGED, tol, 8)
    assert r1["converged"] and r2["converged"] and 2 <= r1["iterations"] == r2["iterations"] <= 3
    assert np.array_equal(u1, u2)
    np.testing.assert_allclose(r2["residual_history"], r1["residual_history"], rtol=1e-12)


def test_initial_guess_and_boundary_ring():
    """a non-zero Dirichlet ring and a random initial guess: rim workgroups interpolate next to boundary cells that keep their values"""
    nx, ny = SHAPE64
    x = np.linspace(0.0, 1.0, nx); y = np.linspace(0.0, 1.0, ny)
    u0 = np.random.default_rng(7).standard_normal((nx, ny))
    u0[0, :] = np.sin(3 * y); u0[-1, :] = np.cos(2 * y)
    u0[:, 0] = u0[0, 0] + x * (u0[-1, 0] - u0[0, 0]); u0[:, -1] = u0[0, -1] + x * (u0[-1, -1] - u0[0, -1])
    u1, r1 = _run(SHAPE64, _lib.MG_PREC_DOUBLE, TILED, 0.0, 3, u0=u0)
    u2, r2 = _run(SHAPE64, _lib.MG_PREC_DOUBLE, STAGED, 0.0, 3, u0=u0)
    assert np.array_equal(u1, u2)
    assert np.array_equal(u2[0, :], u0[0, :]) and np.array_equal(u2[-1, :], u0[-1, :])
    assert np.array_equal(u2[:, 0], u0[:, 0]) and np.array_equal(u2[:, -1], u0[:, -1])
    np.testing.assert_allclose(r2["residual_history"], r1["residual_history"], rtol=1e-12)


def test_red_black_gs_patch_footprint():
    """red-black Gauss-Seidel, omega = 1.15: halo 10, five halo lanes per side (HL = 5) -- another tile and patch placement"""
    u1, r1 = _run(SHAPE64, _lib.MG_PREC_DOUBLE, TILED, 0.0, 3, smoother=_lib.MG_RBGS, omega=1.15)
    u2, r2 = _run(SHAPE64, _lib.MG_PREC_DOUBLE, STAGED, 0.0, 3, smoother=_lib.MG_RBGS, omega=1.15)
    assert np.array_equal(u1, u2)
    np.testing.assert_allclose(r2["residual_history"], r1["residual_history"], rtol=1e-12)


def test_variable_coefficient_up_leg():
    """one variable-coefficient V-cycle: the VAR up leg (8 x 4 strip, the patch written behind the loads of the coefficient) against
    the LDS-tiled legs, engines built as in test_gpu_varcoef.py.  The norm of 56833 cells summed in two orders: each sum is
    within (n - 1) eps = 6.3e-12 of the exact one, the square root halves that, so the two norms differ by less than 1e-11."""
    nx, ny = SHAPE64
    rng = np.random.default_rng(nx + ny)
    rhs = _rhs(nx, ny)
    u0 = rng.standard_normal((nx, ny))
    a = np.exp(0.6 * rng.standard_normal((nx, ny)))       # rough, positive: nothing cancels by symmetry
    out = []
    for fused in (3, 1):
        eng = mg.MultigridEngine(nx, ny, max_levels=mg.default_max_levels(nx, ny), cycle="V", smoother=_lib.MG_JACOBI, omega=0.8,
                                 precision=_lib.MG_PREC_DOUBLE, coarse_maxit=60, fused=fused)
        eng.set_coefficient(a)
        out.append(eng.solve(rhs, u0, tol=1e-30, max_iterations=1))
        eng.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_allclose(out[0][1]["residual_history"], out[1][1]["residual_history"], rtol=1e-11)
