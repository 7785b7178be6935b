"""The vorticity / stream-function stepper without a GPU (tests/test_gpu_flow.py is the GPU half): the header
include/mghip_flow.h, its binding table and the library's exports agree; the build lists the new unit; mg_flow_create and the
mg_dev_flow_* calls refuse what they refuse without looking for a device; and the NumPy restatement tests/flow_reference.py
is a correct scheme: second order in space and time, energy- and enstrophy-conserving, and it reproduces the lid-driven
cavity."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flow_reference as R                                                        # noqa: E402

import mixed_precision_multigrid_solvers_for_pdes_amd as mg                      # noqa: E402
from mixed_precision_multigrid_solvers_for_pdes_amd import _build, _lib          # noqa: E402

ROOT = os.path.dirname(HERE)
FLOW_FUNCTIONS = ["mg_flow_create", "mg_flow_destroy", "mg_flow_last_error", "mg_flow_set_walls", "mg_flow_set_forcing",
                  "mg_flow_set_state", "mg_flow_get", "mg_flow_get_device", "mg_flow_set_device", "mg_flow_step",
                  "mg_flow_diagnostics", "mg_flow_velocity_max", "mg_dev_flow_rhs", "mg_dev_flow_wall", "mg_dev_flow_diag",
                  "mg_dev_flow_interior"]


# ------------------------------------------------------------------ ABI, bindings, build ---------------
def test_flow_header_bindings_and_exports():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mghip_flow.h")).read(), flags=re.S)
    decl = dict(re.findall(r"^\s*(?:const char\*|int)\s+(mg_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.M | re.S))
    assert set(decl) == set(FLOW_FUNCTIONS) == set(_lib.FLOW_SIGNATURES)
    for other in (_lib.SIGNATURES, _lib.HEAT_EXT_SIGNATURES, _lib.LINE_SIGNATURES, _lib.EIG_SIGNATURES, _lib.HO_SIGNATURES):
        assert not set(decl) & set(other)
    lib = _lib.load()
    for name, args in decl.items():
        assert hasattr(lib, name), name
        nargs = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert nargs == len(_lib.FLOW_SIGNATURES[name][1]), (name, nargs)
        assert getattr(lib, name).argtypes == _lib.FLOW_SIGNATURES[name][1]
        assert getattr(lib, name).restype == _lib.FLOW_SIGNATURES[name][0]
    body = re.search(r"typedef struct mg_flow_step_info \{(.*?)\} mg_flow_step_info;", text, flags=re.S).group(1)
    fields = [(t, n.strip()) for t, group in re.findall(r"(double|int32_t)\s+([^;]+);", body) for n in group.split(",")]
    assert [n for _, n in fields] == [f[0] for f in _lib.MgFlowStepInfo._fields_]
    assert [C.c_double if t == "double" else C.c_int32 for t, _ in fields] == [f[1] for f in _lib.MgFlowStepInfo._fields_]
    codes = dict((n, int(v)) for n, v in re.findall(r"(MG_FLOW_[A-Z_]+) = (\d+)", text))
    assert codes == {"MG_FLOW_FREE_SLIP": 0, "MG_FLOW_NO_SLIP": 1, "MG_FLOW_OMEGA": 0, "MG_FLOW_PSI": 1, "MG_FLOW_N": 2}
    for name, value in codes.items():
        assert getattr(_lib, name) == value
    assert (R.FREE_SLIP, R.NO_SLIP) == (_lib.MG_FLOW_FREE_SLIP, _lib.MG_FLOW_NO_SLIP)
    assert '#include "mghip.h"' in text
    main = open(os.path.join(ROOT, "include", "mghip.h")).read()
    assert "mghip_flow" not in main and "mg_flow" not in main and "mg_dev_flow" not in main        # mghip.h itself is unchanged
    assert mg.VorticityStreamSolver is not None and "VorticityStreamSolver" in mg.__all__


def test_build_lists_the_flow_unit():
    srcs, hdrs = [os.path.basename(s) for s in _build.SOURCES], [os.path.basename(h) for h in _build.HEADERS]
    assert "mg_flow.hip" in srcs and {"mg_flow_kernels.hpp", "mghip_flow.h"} <= set(hdrs)
    assert all(os.path.exists(p) for p in _build.SOURCES + _build.HEADERS)
    assert set(_build.NOT_INCLUDED) == set(srcs)
    kernel_headers = {h for h in hdrs if h.endswith("_kernels.hpp")} - {"mg_kernels.hpp", "mg_flow_kernels.hpp"}
    assert kernel_headers <= set(_build.NOT_INCLUDED["mg_flow.hip"])            # every other family's kernel header
    assert {"mghip_line.h", "mghip_eig.h", "mghip_ho.h", "mg_eig_dense.hpp"} <= set(_build.NOT_INCLUDED["mg_flow.hip"])
    assert "mg_kernels.hpp" not in _build.NOT_INCLUDED["mg_flow.hip"]
    for unit, skip in _build.NOT_INCLUDED.items():
        assert ("mg_flow_kernels.hpp" in skip) == (unit != "mg_flow.hip"), unit
        assert ("mghip_flow.h" in skip) == (unit != "mg_flow.hip"), unit
    for unit in srcs:
        text = open(os.path.join(_build.CSRC, unit)).read()
        assert ('#include "mg_flow_kernels.hpp"' in text) == (unit == "mg_flow.hip"), unit
        assert ("mghip_flow.h" in text) == (unit == "mg_flow.hip"), unit
        for skipped in _build.NOT_INCLUDED[unit]:
            assert '"' + skipped + '"' not in text and "/" + skipped + '"' not in text, (unit, skipped)
    text = open(os.path.join(_build.CSRC, "mg_flow.hip")).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["mg_host.hpp", "../../include/mghip_flow.h", "mg_flow_kernels.hpp"]
    blob = open(_build.build_library(), "rb").read()
    for kernel in (b"flow_rhs_kernel", b"flow_wall_kernel", b"flow_diag_kernel"):
        assert kernel in blob, kernel


BASE = dict(nx=33, ny=33, x0=0.0, x1=1.0, y0=0.0, y1=1.0, coeff=-1.0, max_levels=4, cycle=0, pre=2, post=2, smoother=0,
            omega=0.8, coarse_tol=1e-12, coarse_maxit=1000, precision=_lib.MG_PREC_DOUBLE, switch_threshold=1e-6,
            memory_threshold_gb=4.0, adaptive_reference_rule=0, device=0, profile=0, colour_offset=0, fused=2, tail=1,
            fmg_cycles=0, speculate=2, coarse_direct=0, mixed_split=0)


def test_create_refuses_bad_configurations_before_any_device_work():
    lib = _lib.load()
    for bad in (dict(precision=_lib.MG_PREC_SINGLE), dict(precision=_lib.MG_PREC_MIXED_LEVELS), dict(precision=_lib.MG_PREC_ADAPTIVE),
                dict(precision=_lib.MG_PREC_SINGLE_MANAGED), dict(precision=_lib.MG_PREC_DEFECT), dict(coeff=1.0), dict(coeff=-2.0),
                dict(fmg_cycles=1)):
        cfg, h = _lib.MgConfig(**dict(BASE, **bad)), C.c_void_p(None)
        assert lib.mg_flow_create(C.byref(cfg), 0.01, 1, C.byref(h)) == _lib.MG_ERR_INVALID_VALUE, bad
        assert not h.value and b"mg_flow_create" in lib.mg_flow_last_error(None)
    cfg, h = _lib.MgConfig(**BASE), C.c_void_p(None)
    for nu in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.mg_flow_create(C.byref(cfg), nu, 1, C.byref(h)) == _lib.MG_ERR_INVALID_VALUE and not h.value
        assert b"nu" in lib.mg_flow_last_error(None)
    for kind in (-1, 2):
        assert lib.mg_flow_create(C.byref(cfg), 0.01, kind, C.byref(h)) == _lib.MG_ERR_INVALID_VALUE and not h.value
        assert b"wall" in lib.mg_flow_last_error(None)
    assert lib.mg_flow_create(None, 0.01, 1, C.byref(h)) == _lib.MG_ERR_INVALID_VALUE
    assert lib.mg_flow_create(C.byref(cfg), 0.01, 1, None) == _lib.MG_ERR_INVALID_VALUE
    # a valid configuration goes on to look for a device
    rc = lib.mg_flow_create(C.byref(cfg), 0.01, 1, C.byref(h))
    if _lib.device_count() == 0:
        assert rc == _lib.MG_ERR_NO_DEVICE and not h.value
    else:
        assert rc == _lib.MG_OK and h.value
        assert lib.mg_flow_destroy(h) == _lib.MG_OK
    # calls on a NULL stepper are refused, mg_flow_destroy(NULL) is a no-op
    buf, out = np.zeros((3, 3)), (C.c_double * 2)(-3.0, -3.0)
    info = _lib.MgFlowStepInfo()
    assert lib.mg_flow_step(None, 0.1, 1e-10, 20, C.byref(info)) == _lib.MG_ERR_INVALID_VALUE
    assert lib.mg_flow_set_state(None, _lib.ptr(buf), _lib.MG_F64, 1e-10, 20, None) == _lib.MG_ERR_INVALID_VALUE
    assert lib.mg_flow_get(None, 0, _lib.ptr(buf), _lib.MG_F64) == _lib.MG_ERR_INVALID_VALUE
    assert lib.mg_flow_set_forcing(None, None, _lib.MG_F64) == _lib.MG_ERR_INVALID_VALUE
    assert lib.mg_flow_set_walls(None, out) == _lib.MG_ERR_INVALID_VALUE
    assert lib.mg_flow_diagnostics(None, out) == _lib.MG_ERR_INVALID_VALUE and out[0] == -3.0
    assert lib.mg_flow_velocity_max(None, out) == _lib.MG_ERR_INVALID_VALUE and out[0] == -3.0
    assert lib.mg_flow_destroy(None) == _lib.MG_OK


def test_stateless_calls_refuse_bad_arguments_before_any_device_work():
    """every refusal, with pointers that are never followed (host memory: a launch would fault)"""
    lib = _lib.load()
    mem = np.zeros(8 * 128 + 2)            # eight 9 x 10 fields (720 bytes each) 1024 bytes apart
    base = (mem.ctypes.data + 15) // 16 * 16
    p, w, npv, F, f, N, sc, o2 = (C.c_void_p(base + 1024 * k) for k in range(8))
    e4 = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)

    def rhs(nx=9, ny=9, ld=10, hx=0.125, hy=0.125, nu=0.01, dt=0.1, c0=1.5, c1=-0.5, psi=p, om=w, prev=npv, force=F, fo=f, no=N,
            scratch=sc, out=o2):
        rc = lib.mg_dev_flow_rhs(nx, ny, ld, hx, hy, nu, dt, c0, c1, psi, om, prev, force, fo, no, scratch, out, None)
        return rc, lib.mg_last_error(None)

    bad = [dict(psi=None), dict(om=None), dict(fo=None), dict(no=None), dict(scratch=None), dict(nx=2), dict(ny=2), dict(ld=8),
           dict(ld=11), dict(dt=0.0), dict(dt=-0.1), dict(dt=float("nan")), dict(dt=float("inf")), dict(nu=0.0), dict(nu=-1.0),
           dict(nu=float("inf")), dict(hx=0.0), dict(hy=-1.0), dict(c0=float("nan")), dict(c1=float("inf")), dict(fo=p), dict(fo=w),
           dict(no=npv), dict(no=F), dict(fo=N), dict(psi=C.c_void_p(base + 8)), dict(fo=C.c_void_p(base + 4 * 1024 + 8)),
           dict(no=C.c_void_p(base + 9 * 80 - 16))]                                   # N overlaps psi part way
    for kw in bad:
        rc, msg = rhs(**kw)
        assert rc == _lib.MG_ERR_INVALID_VALUE and b"mg_dev_flow_rhs" in msg, kw
    assert b"array of its own" in rhs(fo=w)[1] and b"array of its own" in rhs(fo=N)[1]

    for kw in (dict(nx=2), dict(ny=2), dict(ld=8), dict(ld=11), dict(hx=0.0), dict(hy=float("nan")), dict(kind=2), dict(kind=-1),
               dict(e=None), dict(psi=None), dict(om=None), dict(om=p)):
        a = dict(dict(nx=9, ny=9, ld=10, hx=0.125, hy=0.125, kind=1, e=e4, psi=p, om=w), **kw)
        rc = lib.mg_dev_flow_wall(a["nx"], a["ny"], a["ld"], a["hx"], a["hy"], a["kind"], a["e"], a["psi"], a["om"], None)
        assert rc == _lib.MG_ERR_INVALID_VALUE and b"mg_dev_flow_wall" in lib.mg_last_error(None), kw
    for kw in (dict(nx=2), dict(ny=2), dict(ld=8), dict(ld=11), dict(psi=None), dict(om=None), dict(s=None), dict(o=None),
               dict(psi=C.c_void_p(base + 8))):
        a = dict(dict(nx=9, ny=9, ld=10, psi=p, om=w, s=sc, o=o2), **kw)
        rc = lib.mg_dev_flow_diag(a["nx"], a["ny"], a["ld"], a["psi"], a["om"], a["s"], a["o"], None)
        assert rc == _lib.MG_ERR_INVALID_VALUE and b"mg_dev_flow_diag" in lib.mg_last_error(None), kw
    for kw in (dict(nx=2), dict(ny=2), dict(ld=8), dict(ld=11), dict(w=None), dict(out=None), dict(s=None), dict(out=w), dict(out=npv),
               dict(w=C.c_void_p(base + 1024 + 8))):
        a = dict(dict(nx=9, ny=9, ld=10, w=w, old=npv, out=f, s=sc, o=o2), **kw)
        rc = lib.mg_dev_flow_interior(a["nx"], a["ny"], a["ld"], a["w"], a["old"], a["out"], a["s"], a["o"], None)
        assert rc == _lib.MG_ERR_INVALID_VALUE and b"mg_dev_flow_interior" in lib.mg_last_error(None), kw


def test_solver_refuses_bad_arguments_without_a_device():
    grid = mg.Grid(33, 33)
    with pytest.raises(ValueError, match="wall must be"):
        mg.VorticityStreamSolver(grid, 0.01, wall="partial_slip")
    for nu in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="viscosity"):
            mg.VorticityStreamSolver(grid, nu)
    with pytest.raises(ValueError, match="unknown wall"):
        mg.VorticityStreamSolver(grid, 0.01, wall_speeds={"lid": 1.0})
    with pytest.raises(ValueError, match="finite"):
        mg.VorticityStreamSolver(grid, 0.01, wall_speeds={"top": float("nan")})
    with pytest.raises(ValueError, match="four values"):
        mg.VorticityStreamSolver(grid, 0.01, wall_speeds=(1.0, 2.0))
    with pytest.raises(ValueError, match="cycle"):
        mg.VorticityStreamSolver(grid, 0.01, cycle="X")
    with pytest.raises(ValueError, match="smoother"):
        mg.VorticityStreamSolver(grid, 0.01, smoother="lexgs")
    from mixed_precision_multigrid_solvers_for_pdes_amd.flow import wall_speed_array
    assert wall_speed_array({"top": 1.0, "left": -2.0}) == (-2.0, 0.0, 0.0, 1.0) and wall_speed_array(None) == (0.0,) * 4
    if _lib.device_count() == 0:                      # a configuration the device path serves goes on to the device
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            mg.VorticityStreamSolver(grid, 0.01, wall_speeds={"top": 1.0})


# ------------------------------------------------------------------ the restatement is a correct scheme ---------------
def _two_mode(n):
    """psi* = 0.25 (sin pi x sin pi y + 0.5 sin 2 pi x sin pi y) with w* = -lap psi*, J(psi*, w*) and lap w*, all analytic"""
    x = np.linspace(0.0, 1.0, n)
    X, Y = x[:, None], x[None, :]
    pi = np.pi
    s1, s2, sy, cy = np.sin(pi * X), np.sin(2 * pi * X), np.sin(pi * Y), np.cos(pi * Y)
    c1, c2 = np.cos(pi * X), np.cos(2 * pi * X)
    psi = 0.25 * (s1 * sy + 0.5 * s2 * sy)
    w = 0.25 * (2 * pi**2 * s1 * sy + 2.5 * pi**2 * s2 * sy)
    px, py = 0.25 * (pi * c1 * sy + pi * c2 * sy), 0.25 * (pi * s1 * cy + 0.5 * pi * s2 * cy)
    wx, wy = 0.25 * (2 * pi**3 * c1 * sy + 5 * pi**3 * c2 * sy), 0.25 * (2 * pi**3 * s1 * cy + 2.5 * pi**3 * s2 * cy)
    lapw = -0.25 * (4 * pi**4 * s1 * sy + 12.5 * pi**4 * s2 * sy)
    return psi, w, px * wy - py * wx, lapw


def _ratios(e):
    return [e[k] / e[k + 1] for k in range(len(e) - 1)]


def test_taylor_green_decay_is_second_order():
    """free slip, psi = sin pi x sin pi y decays like exp(-2 pi^2 nu t) (J vanishes); (n - 1)/2 steps to T = 0.25.
    Measured: max psi error 3.12e-3 / 7.79e-4 / 1.95e-4 at 17^2 / 33^2 / 65^2"""
    nu, T, errs = 0.05, 0.25, []
    for n in (17, 33, 65):
        x = np.linspace(0.0, 1.0, n)
        psi0 = np.sin(np.pi * x[:, None]) * np.sin(np.pi * x[None, :])
        fl = R.Flow(n, n, nu, R.FREE_SLIP)
        fl.set_state(2 * np.pi**2 * psi0)
        fl.run((n - 1) // 2, T / ((n - 1) // 2))
        errs.append(float(np.max(np.abs(fl.psi - np.exp(-2 * np.pi**2 * nu * T) * psi0))))
    print("taylor-green errors", errs, _ratios(errs))
    assert all(3.6 <= r <= 4.4 for r in _ratios(errs)), errs


def _forced_error(n, with_jacobian=True):
    nu, T = 0.02, 6.0
    psi, w, J, lapw = _two_mode(n)
    F = (-J if with_jacobian else 0.0) - nu * lapw
    fl = R.Flow(n, n, nu, R.FREE_SLIP, force=F)
    fl.set_state(w)
    steps = int(round(T / (0.5 / (n - 1))))
    fl.run(steps, T / steps)
    return float(np.max(np.abs(fl.psi - psi)))


def test_forced_steady_state_is_second_order_and_sees_the_advection_term():
    """F = -J* - nu lap w* holds the two-mode field steady; dt = h/2 to T = 6 from the exact field.  Measured: max psi error
    6.02e-3 / 1.51e-3 / 3.76e-4; with F = -nu lap w* alone (no Jacobian) 0.103 at every size"""
    errs = [_forced_error(n) for n in (17, 33, 65)]
    print("forced steady errors", errs, _ratios(errs))
    assert all(3.6 <= r <= 4.4 for r in _ratios(errs)), errs
    assert errs[2] < 1e-3
    assert _forced_error(17, with_jacobian=False) > 0.05


def test_temporal_order_is_two():
    """the two-mode field, unforced, nu = 0.02, 33^2, T = 0.1: 4 / 8 / 16 / 32 steps against 256.  Measured max psi error
    8.08e-5, 1.98e-5, 4.88e-6, 1.20e-6"""
    n, nu, T = 33, 0.02, 0.1
    _, w, _, _ = _two_mode(n)

    def run(steps):
        fl = R.Flow(n, n, nu, R.FREE_SLIP)
        fl.set_state(w)
        fl.run(steps, T / steps)
        return fl.psi, fl.w
    ref = run(256)
    out = [run(s) for s in (4, 8, 16, 32)]
    for k, name in ((0, "psi"), (1, "omega")):
        errs = [float(np.max(np.abs(o[k] - ref[k]))) for o in out]
        print("temporal", name, errs, _ratios(errs))
        assert all(3.6 <= r <= 4.4 for r in _ratios(errs)[-2:]), (name, errs)


@pytest.mark.parametrize("shape,domain", [((9, 9), R.UNIT), ((17, 33), R.UNIT), ((12, 7), (0.0, 1.5, -0.2, 0.5))],
                         ids=["9x9", "17x33", "12x7"])
def test_jacobian_conserves_energy_and_enstrophy(shape, domain):
    """sum psi J = 0 for a zero-ring psi and ANY w; sum w J = 0 when the ring of w is zero too (Arakawa 1966): to rounding,
    measured ~1e-17 of sum |psi J|"""
    from oracle import mg_oracle as O
    hx, hy = O.grid_spacing(*shape, domain)
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    psi, w = R.interior(rng.standard_normal(shape)), rng.standard_normal(shape)
    J = R.jacobian(psi, w, hx, hy)
    assert abs(np.sum(psi * J)) <= 1e-13 * np.sum(np.abs(psi * J))
    w0 = R.interior(w)
    J0 = R.jacobian(psi, w0, hx, hy)
    assert abs(np.sum(psi * J0)) <= 1e-13 * np.sum(np.abs(psi * J0))
    assert abs(np.sum(w0 * J0)) <= 1e-13 * np.sum(np.abs(w0 * J0))
    assert np.sum(np.abs(w * J)) > 0 and not J[0, :].any() and not J[:, -1].any()
    # antisymmetry, and the other association is the same Jacobian to rounding
    assert np.max(np.abs(R.jacobian(w, psi, hx, hy) + J)) <= 1e-13 * np.max(np.abs(J))
    assert np.max(np.abs(R.jacobian_other_association(psi, w, hx, hy) - J)) <= 1e-13 * np.max(np.abs(J))


def test_jacobian_is_second_order_accurate():
    errs = []
    for n in (17, 33, 65):
        psi, w, J, _ = _two_mode(n)
        errs.append(float(np.max(np.abs(R.jacobian(psi, w, 1.0 / (n - 1), 1.0 / (n - 1)) - J)[1:-1, 1:-1])))
    assert all(3.6 <= r <= 4.4 for r in _ratios(errs)), errs


@pytest.fixture(scope="module")
def cavities():
    """Re = 100, lid speed 1, dt = h/2 to T = 20 from rest, by direct solves"""
    out = {}
    for n in (33, 65):
        fl = R.Flow(n, n, 0.01, R.NO_SLIP, (0.0, 0.0, 0.0, 1.0))
        fl.set_state(np.zeros((n, n)))
        fl.run(20 * 2 * (n - 1), 0.5 / (n - 1))
        out[n] = fl
    return out


def test_lid_driven_cavity_at_reynolds_100(cavities):
    got33, got65 = R.psi_min(cavities[33].psi), R.psi_min(cavities[65].psi)
    print("cavity psi_min", got33, got65)
    assert abs(got33[0] - (-0.1016214)) < 1e-6 and got33[1:] == (0.625, 0.75)
    assert abs(got65[0] - (-0.1030330)) < 1e-6 and got65[1:] == (0.609375, 0.734375)
    # the primary vortex strengthens towards the literature's ~ -0.1034 under refinement, second order: the difference between
    # the two grids bounds a third of what is left
    assert got65[0] < got33[0] and abs(got65[0] - got33[0]) < 2e-3
    assert abs(cavities[33].time - 20.0) < 1e-9


def test_rectangular_cavity_stays_finite():
    dom = (0.0, 1.0, 0.0, 2.0)
    fl = R.Flow(33, 65, 0.01, R.NO_SLIP, (0.0, 0.0, 0.0, 1.0), domain=dom)
    fl.set_state(np.zeros((33, 65)))
    fl.run(1600, 0.5 / 32)
    assert np.isfinite(fl.psi).all() and np.isfinite(fl.w).all()
    lo = R.psi_min(fl.psi, dom)
    print("rectangular cavity psi_min", lo)
    assert -0.2 < lo[0] < -0.05 and lo[2] > 1.5                   # one primary vortex under the lid


def test_a_converged_cycle_solve_agrees_with_the_direct_solve():
    """five cavity steps at 17^2: the pinned cycle to 1e-12 against the sine transform"""
    n = 17
    runs = []
    for solver in (R.CycleSolver(n, n, tol=1e-12), None):
        fl = R.Flow(n, n, 0.01, R.NO_SLIP, (0.3, -0.2, 0.1, 1.0), solver=solver)
        fl.set_state(np.zeros((n, n)))
        infos = fl.run(5, 0.5 / (n - 1))
        runs.append(fl)
        assert all(i["omega"]["converged"] and i["psi"]["converged"] for i in infos)
    assert np.max(np.abs(runs[0].w - runs[1].w)) < 1e-9 * np.max(np.abs(runs[1].w))
    assert np.max(np.abs(runs[0].psi - runs[1].psi)) < 1e-9 * np.max(np.abs(runs[1].psi))


def test_restatement_rings_wall_order_and_first_step():
    rng = np.random.default_rng(4)
    psi, w, F, Np = (rng.standard_normal((9, 12)) for _ in range(4))
    f, N, ss, m = R.rhs(psi, w, 0.02, 0.01, 0.1, 0.07, 1.25, -0.25, Np, F)
    for a in (f, N):
        assert not a[0, :].any() and not a[-1, :].any() and not a[:, 0].any() and not a[:, -1].any() and a[1:-1, 1:-1].all()
    assert ss == float(np.sum(f * f)) and m > 0
    # c1 = 0 with a history is not the first-step form bit for bit in general, but without N_prev nothing of it is read
    f1, N1, _, _ = R.rhs(psi, w, 0.02, 0.01, 0.1, 0.07, 1.0, 0.0, None, F)
    np.testing.assert_array_equal(N1, N)
    f2, _, _, _ = R.rhs(psi, w, 0.02, 0.01, 0.1, 0.07, 1.0, 0.0, np.full((9, 12), np.nan), F)
    assert np.isfinite(f1).all() and not np.isfinite(f2[1:-1, 1:-1]).any()
    assert R.ab2(0.1, None) == (1.0, 0.0) and R.ab2(0.1, 0.1) == (1.5, -0.5) and R.ab2(0.05, 0.1) == (1.25, -0.25)
    v = R.wall(w.copy(), psi, 0.1, 0.07, R.NO_SLIP, (1.0, 2.0, 3.0, 4.0))
    np.testing.assert_array_equal(v[1:-1, 1:-1], w[1:-1, 1:-1])
    assert v[0, 0] == (2.0 * (psi[0, 0] - psi[0, 1])) / (0.07 * 0.07) + (2.0 * 3.0) / 0.07          # corners: bottom / top
    assert v[-1, -1] == (2.0 * (psi[-1, -1] - psi[-1, -2])) / (0.07 * 0.07) - (2.0 * 4.0) / 0.07
    assert v[0, 5] == (2.0 * (psi[0, 5] - psi[1, 5])) / (0.1 * 0.1) - (2.0 * 1.0) / 0.1
    z = R.wall(w.copy(), psi, 0.1, 0.07, R.FREE_SLIP)
    assert not z[0, :].any() and not z[:, -1].any() and (z[1:-1, 1:-1] == w[1:-1, 1:-1]).all()
