"""The CPU half of the reaction-diffusion stepper's tests (tests/test_gpu_rd.py is the GPU half): the NumPy restatement
tests/rd_reference.py is pinned -- its right-hand sides against the heat stepper's with the reaction switched off, one step on
a discrete eigenmode against the closed form, the orders in time, the gradient energy against the operator --, the header
declares the entry points, the bindings match and the library exports them, the build table lists the unit, and the ABI and
ReactionDiffusionSolver refuse bad arguments before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _build, _lib

import heat_device_reference as HD
import heat_var_reference as HV
import nl_reference as NL
import rd_reference as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mghip_rd.h")
SCHEMES = [RD.IMPLICIT, RD.CN, RD.BDF2]


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("scheme", SCHEMES)
def test_rhs_without_reaction_is_the_heat_steppers(scheme):
    """kappa = 0, rho = 0: the heat stepper's right-hand side, bit for bit (17 x 33 on the unit square: 1/hx^2 and 1/hy^2 are
    powers of two, so the kernels' products and the oracle's quotients round alike)"""
    nx, ny, dt, alpha = 17, 33, 0.0137, 0.31
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    rng = np.random.default_rng(5)
    u, up, S = rng.standard_normal((nx, ny)), rng.standard_normal((nx, ny)), rng.standard_normal((nx, ny))
    a = 1.0 + rng.random((nx, ny)) + 20.0 * (rng.random((nx, ny)) > 0.6)
    w = rng.random((nx, ny))
    for src in (None, S):
        for field in (None, a):
            for kind in range(4):
                got = RD.rhs(scheme, kind, u, dt, alpha, hx, hy, 0.0, 0.0, up if scheme == RD.BDF2 else None, src, field, w, 0.7, -1.3)
                if field is None:
                    want = HD.rhs(scheme, u, dt, alpha, hx, hy, up, src, 0.7, -1.3)
                else:
                    want = HV.rhs_var(scheme, u, dt, alpha, field, hx, hy, up, src, 0.7, -1.3)
                np.testing.assert_array_equal(got, want)
    # and the reaction terms do enter
    assert np.any(RD.rhs(scheme, 1, u, dt, alpha, hx, hy, 0.0, 0.5, up) != RD.rhs(scheme, 1, u, dt, alpha, hx, hy, 0.0, 0.0, up))
    assert np.any(RD.rhs(RD.CN, 1, u, dt, alpha, hx, hy, 2.0, 0.0) != RD.rhs(RD.CN, 1, u, dt, alpha, hx, hy, 0.0, 0.0))


@pytest.mark.parametrize("case", [(RD.IMPLICIT, None), (RD.CN, None), (RD.CN, 0.8), (RD.BDF2, 1.15)],
                         ids=["implicit_euler", "cn", "cn_ab2", "bdf2"])
def test_one_step_multiplies_the_eigenmode_by_the_closed_form(case):
    scheme, c = case
    nx, ny, dt, alpha, kappa, rho = 17, 33, 0.02, 0.3, 2.5, 1.75
    phi, lam_h = RD.eigenmode(nx, ny)
    got, info = RD.step(scheme, "linear", phi, dt, alpha, kappa, rho, u_prev=None if c is None else c * phi, tol=1e-12)
    factor = RD.eigen_factor(scheme, dt, alpha, lam_h, kappa, rho, c)
    err = float(np.max(np.abs(got - factor * phi)))
    print(scheme, c, "factor", factor, "error", err, "newton", info["newton_iterations"])
    assert info["converged"] and info["newton_iterations"] == 1
    assert 0.0 < factor < 1.2 and err <= 1e-11
    if scheme == RD.IMPLICIT:
        assert factor == pytest.approx((1 + dt * rho) / (1 + dt * (alpha * lam_h + kappa)), rel=1e-15)


def test_orders_in_time():
    """17 x 17, alpha = 0.05, cubic, kappa = 4, rho = 3, S = sin(pi x) sin(2 pi y), g = cos 3t, u0 = 1.5 sin(pi x) sin(pi y),
    T = 0.5: the max-norm errors of N = 16, 32, 64 steps against BDF2 with 1024"""
    n, alpha, kappa, rho, T = 17, 0.05, 4.0, 3.0, 0.5
    X, Y = NL.mesh(n, n)
    S = np.sin(np.pi * X) * np.sin(2 * np.pi * Y)
    u0 = 1.5 * RD.eigenmode(n, n)[0]
    g = lambda t: float(np.cos(3.0 * t))
    final = lambda scheme, N: RD.run(scheme, "cubic", u0, T / N, N, alpha, kappa, rho, S=S, g=g, tol=1e-13)[-1]
    ref = final(RD.BDF2, 1024)
    for scheme, least in ((RD.IMPLICIT, 1.8), (RD.CN, 3.6), (RD.BDF2, 3.6)):
        errs = [float(np.max(np.abs(final(scheme, N) - ref))) for N in (16, 32, 64)]
        ratios = [errs[0] / errs[1], errs[1] / errs[2]]
        print(scheme, "errors", errs, "ratios", ratios)
        assert min(ratios) >= least, (scheme, errs, ratios)


@pytest.mark.parametrize("var", [False, True], ids=["laplace", "varcoef"])
def test_gradient_energy_is_the_potential_of_the_operator(var):
    """dG/du = -hx hy L_a u on interior cells, for non-zero ring data.  G is quadratic, so the central difference is exact up
    to rounding: |error| <= 4 eps G / step"""
    nx, ny = 9, 12
    hx, hy = 1.0 / (nx - 1), 0.75 / (ny - 1)
    rng = np.random.default_rng(3)
    u = rng.standard_normal((nx, ny))
    a = 1.0 + rng.random((nx, ny)) + 10.0 * (rng.random((nx, ny)) > 0.6) if var else None
    G = lambda v: float(np.sum(RD.energy_terms(0, v, hx, hy, a)[0]))
    want = -hx * hy * RD.lap(u, hx, hy, a)
    step = 1e-3
    bound = 4 * np.finfo(float).eps * G(u) / step + 1e-12 * float(np.max(np.abs(want)))
    for i in range(1, nx - 1):
        for j in range(1, ny - 1):
            e = np.zeros_like(u); e[i, j] = step
            d = (G(u + e) - G(u - e)) / (2 * step)
            assert abs(d - want[i, j]) <= bound, (i, j, d, want[i, j])
    # ring cells enter G (through the faces to interior cells) but corners do not
    e = np.zeros_like(u); e[0, 3] = 1.0
    assert G(u + e) != G(u)
    e = np.zeros_like(u); e[0, 0] = e[-1, -1] = e[0, -1] = e[-1, 0] = 1.0
    assert G(u + e) == G(u)
    # the other two sums, and E
    w = rng.random((nx, ny))
    _, P, Q = RD.energy_terms(1, u, hx, hy, a, w)
    np.testing.assert_array_equal(P[1:-1, 1:-1], w[1:-1, 1:-1] * (((u * u) * (u * u)) / 4)[1:-1, 1:-1])
    np.testing.assert_array_equal(Q[1:-1, 1:-1], (u * u)[1:-1, 1:-1])
    assert not P[0].any() and not Q[:, -1].any()
    for kind in range(4):
        assert np.all(RD.Phi(kind, np.linspace(-3, 3, 41)) >= 0.0)
    E = RD.energy(1, u, hx, hy, 0.3, 2.0, 1.5, a, w)
    assert E["energy"] == pytest.approx(0.3 * E["gradient"] + hx * hy * (2.0 * E["potential"] - 0.75 * E["sum_squares"]), rel=1e-15)


# ------------------------------------------------------------------------------------------ header, bindings, library, build
def test_header_bindings_and_exports():
    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(mg_\w+)\(", text, flags=re.M))
    assert declared == set(_lib.RD_SIGNATURES), declared ^ set(_lib.RD_SIGNATURES)
    for needle in ('#include "mghip_nl.h"', "MG_ERR_INVALID_VALUE", "no FMA contraction", "convex splitting", "Explicit Euler"):
        assert needle in text, needle
    lib = _lib.load()
    for name in _lib.RD_SIGNATURES:
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.MgRdStepInfo) == 64
    assert _lib.RD_SCHEMES == {"implicit_euler": 1, "crank_nicolson": 2, "bdf2": 3}


def test_build_lists_the_rd_unit():
    srcs, hdrs = [os.path.basename(s) for s in _build.SOURCES], [os.path.basename(h) for h in _build.HEADERS]
    assert "mg_rd.hip" in srcs and {"mg_rd_kernels.hpp", "mghip_rd.h"} <= set(hdrs)
    assert all(os.path.exists(p) for p in _build.SOURCES + _build.HEADERS)
    assert set(_build.NOT_INCLUDED) == set(srcs)
    kernel_headers = {h for h in hdrs if h.endswith("_kernels.hpp")} - {"mg_kernels.hpp", "mg_rd_kernels.hpp"}
    assert kernel_headers <= set(_build.NOT_INCLUDED["mg_rd.hip"])              # every other family's kernel header
    assert {"mghip_line.h", "mghip_eig.h", "mghip_ho.h", "mghip_flow.h", "mg_eig_dense.hpp"} <= set(_build.NOT_INCLUDED["mg_rd.hip"])
    assert "mg_kernels.hpp" not in _build.NOT_INCLUDED["mg_rd.hip"] and "mghip_nl.h" not in _build.NOT_INCLUDED["mg_rd.hip"]
    for unit, skip in _build.NOT_INCLUDED.items():
        assert ("mg_rd_kernels.hpp" in skip) == (unit != "mg_rd.hip"), unit
        assert ("mghip_rd.h" in skip) == (unit != "mg_rd.hip"), unit
    for unit in srcs:
        text = open(os.path.join(_build.CSRC, unit)).read()
        assert ('#include "mg_rd_kernels.hpp"' in text) == (unit == "mg_rd.hip"), unit
        assert ("mghip_rd.h" in text) == (unit == "mg_rd.hip"), unit
        for skipped in _build.NOT_INCLUDED[unit]:
            assert '"' + skipped + '"' not in text and "/" + skipped + '"' not in text, (unit, skipped)
    text = open(os.path.join(_build.CSRC, "mg_rd.hip")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["mg_host.hpp", "../../include/mghip_rd.h", "mg_rd_kernels.hpp"]
    assert re.findall(r'#include "([^"]+)"', open(os.path.join(_build.CSRC, "mg_rd_kernels.hpp")).read()) == ["mg_tile.hpp"]
    assert re.findall(r'#include "([^"]+)"', open(os.path.join(_build.CSRC, "mg_tile.hpp")).read()) == ["mg_kernels.hpp"]
    solver_units = {"mg_pcg.hip", "mg_heat.hip", "mg_rd.hip", "mg_nl.hip", "mg_eig.hip", "mg_ho.hip", "mg_flow.hip"}
    assert "mg_tile.hpp" in hdrs
    for unit, skip in _build.NOT_INCLUDED.items():                                # the shared helpers: the solver modules' kernel headers alone
        assert ("mg_tile.hpp" in skip) == (unit not in solver_units), unit
    for name in os.listdir(_build.CSRC):
        text = open(os.path.join(_build.CSRC, name)).read()
        assert ('#include "mg_tile.hpp"' in text) == (name[:-len("_kernels.hpp")] + ".hip" in solver_units and name.endswith("_kernels.hpp")), name
    blob = open(_build.build_library(), "rb").read()
    for kernel in (b"rd_rhs_kernel", b"rd_energy_kernel", b"reduce_rows_kernel"):
        assert kernel in blob, kernel


# ------------------------------------------------------------------------------------------ refusals
BASE = dict(nx=33, ny=33, x0=0.0, x1=1.0, y0=0.0, y1=1.0, coeff=-1.0, max_levels=4, cycle=0, pre=2, post=2, smoother=0,
            omega=0.8, coarse_tol=1e-12, coarse_maxit=1000, precision=_lib.MG_PREC_DOUBLE, switch_threshold=1e-6,
            memory_threshold_gb=4.0, adaptive_reference_rule=0, device=0, profile=0, colour_offset=0, fused=2, tail=1,
            fmg_cycles=0, speculate=2, coarse_direct=0, mixed_split=0)


def test_abi_refuses_before_any_device_work():
    """every refusal that needs no stepper (those of a live stepper -- slots, aliasing, BDF2 without prev -- are in
    tests/test_gpu_rd.py: a stepper needs a device)"""
    lib = _lib.load()
    I = _lib.MG_ERR_INVALID_VALUE
    buf, other = np.zeros((9, 10)), np.zeros((9, 10))
    p, q = _lib.ptr(buf), _lib.ptr(other)
    ok = dict(scheme=2, kind=1, ld=10, alpha=0.5, dt=0.1, kappa=1.0, rho=0.5, prev=None, out=q, scratch=None)

    def rhs(**kw):
        a = dict(ok, **kw)
        return lib.mg_dev_rd_rhs(a["scheme"], a["kind"], 9, 9, a["ld"], 0.1, 0.1, a["alpha"], a["dt"], a["kappa"], a["rho"], p,
                                 a["prev"], None, None, None, 1.0, 1.0, a["out"], a["scratch"], None, None)

    nan, inf = float("nan"), float("inf")
    for bad in (dict(scheme=0), dict(scheme=4), dict(scheme=-1), dict(kind=4), dict(kind=-1), dict(ld=9), dict(alpha=0.0),
                dict(alpha=nan), dict(dt=0.0), dict(dt=-1.0), dict(dt=inf), dict(dt=nan), dict(kappa=-1.0), dict(kappa=nan),
                dict(kappa=inf), dict(rho=nan), dict(rho=inf), dict(scheme=3, scratch=q), dict(out=p, scratch=q), {}):
        assert rhs(**bad) == I, bad                                            # {}: the NULL scratch
    assert b"mg_dev_rd_rhs" in lib.mg_last_error(None)
    assert rhs(scheme=0) == I and b"explicit Euler" in lib.mg_last_error(None)
    energy = lambda kind, ld, u, scratch, sums: lib.mg_dev_rd_energy(kind, 9, 9, ld, 0.1, 0.1, None, None, u, scratch, sums, None)
    assert energy(4, 10, p, q, q) == I and energy(0, 9, p, q, q) == I and energy(0, 10, None, q, q) == I
    assert energy(0, 10, p, None, q) == I and energy(0, 10, p, q, None) == I
    assert b"mg_dev_rd_energy" in lib.mg_last_error(None)
    # calls on a NULL stepper
    info = _lib.MgRdStepInfo()
    out4 = (C.c_double * 4)()
    assert lib.mg_rd_step(None, 1, 0.1, 0, -1, 1, 1.0, 1.0, None, 1e-8, 10, C.byref(info)) == I
    assert lib.mg_rd_set_slot(None, 0, p, _lib.MG_F64) == I and lib.mg_rd_get_slot(None, 0, p, _lib.MG_F64) == I
    assert lib.mg_rd_set_slot_device(None, 0, p, 10, _lib.MG_F64) == I and lib.mg_rd_get_slot_device(None, 0, p, 10, _lib.MG_F64) == I
    assert lib.mg_rd_set_coefficient(None, None, _lib.MG_F64) == I and lib.mg_rd_set_source(None, None, _lib.MG_F64) == I
    assert lib.mg_rd_set_reaction(None, 1, 1.0, None, _lib.MG_F64, 0.0) == I and lib.mg_rd_set_newton_options(None, None) == I
    assert lib.mg_rd_energy(None, 0, out4) == I and lib.mg_rd_diff_norm(None, 0, 1, out4) == I
    assert lib.mg_rd_destroy(None) == _lib.MG_OK
    # creation
    h = C.c_void_p(None)
    assert lib.mg_rd_create(None, 1.0, 1, -1, C.byref(h)) == I and not h.value
    for bad_cfg, alpha in ((dict(), 0.0), (dict(), -1.0), (dict(), nan), (dict(), inf), (dict(coeff=1.0), 1.0), (dict(coeff=-2.0), 1.0),
                           (dict(fmg_cycles=1), 1.0), (dict(precision=_lib.MG_PREC_SINGLE), 1.0),
                           (dict(precision=_lib.MG_PREC_ADAPTIVE), 1.0), (dict(precision=_lib.MG_PREC_DEFECT), 1.0)):
        cfg = _lib.MgConfig(**dict(BASE, **bad_cfg))
        assert lib.mg_rd_create(C.byref(cfg), alpha, 1, -1, C.byref(h)) == I and not h.value, (bad_cfg, alpha)
    assert b"mg_rd_create" in lib.mg_last_error(None)


def test_python_refusals(monkeypatch):
    n = 17
    grid = mg.Grid(n, n)
    loads = []

    def no_load():
        loads.append(1)
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_load)
    R = mg.ReactionDiffusionSolver
    for kw, match in ((dict(diffusivity=0.0), "diffusivity"), (dict(diffusivity=float("nan")), "diffusivity"),
                      (dict(nonlinearity="bratu"), "nonlinearity"), (dict(strength=-1.0), "strength"),
                      (dict(strength=float("inf")), "strength"), (dict(linear_growth=float("nan")), "linear_growth"),
                      (dict(scheme="explicit_euler"), "scheme"), (dict(precision="adaptive"), "precision"),
                      (dict(forcing="constant"), "forcing"), (dict(max_newton=0), "max_newton"),
                      (dict(tolerance=float("nan")), "tolerance"), (dict(weight=np.ones((n, n + 2))), "weight shape"),
                      (dict(weight=-np.ones((n, n))), "weight"), (dict(conductivity=np.zeros((n, n))), "conductivity"),
                      (dict(conductivity=np.ones((n + 1, n))), "conductivity shape"), (dict(source=lambda x, y, t: 1.0), "source"),
                      (dict(source=np.ones((n, 3))), "source shape"), (dict(source=np.full((n, n), np.inf)), "source"),
                      (dict(smoother="jacobi"), "smoother")):
        args = dict(dict(diffusivity=1e-2), **kw)
        with pytest.raises(ValueError, match=match):
            R(grid, **args)
    assert not loads
    assert "ReactionDiffusionSolver" in mg.__all__
