"""NaN and Inf through the reductions, the stop rules and the drivers, on a GPU (DESIGN.md "Special values").

Call by call: one launch per (position, value, field that feeds the reduction) with the positions and values of
tests/special_values.py, against the NumPy restatement of the same call on the same planted field, by same_special (identical
NaN masks, equal bits elsewhere, infinities included); finite sums keep the rule of dev_call_cases.compare_sum.  Every launch
runs twice and must give the same bits.  A planted value is data: every pointer, pitch and extent stays valid.

Drivers: a flow step on a poisoned state against the restatement's step, the cavity that blows up from rest through
run_to_steady, advance on a non-finite velocity maximum, and the handles (mg_handle, mg_flow, ...) after a poisoned solve:
the next clean solve gives the bits of a fresh handle."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib
from oracle import mg_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dev_call_cases as G                                                        # noqa: E402
import flow_reference as R                                                        # noqa: E402
import special_values as SV                                                       # noqa: E402
import test_gpu_flow as F                                                         # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = F.GUARD
FLOW_SHAPES = [(5, 5), (9, 130), (35, 67)]          # sub-tile; more than one workgroup across and an even ny; both ways and an odd ny
SHAPE_IDS = ["%dx%d" % s for s in FLOW_SHAPES]


def _torch():
    import torch
    return torch


def _plant(t, ij, value, row0=GUARD):
    """write `value` at cell ij of the array whose row 0 is row `row0` of the device tensor t; returns the old value"""
    old = t[row0 + ij[0], ij[1]].item()
    t[row0 + ij[0], ij[1]] = value
    return old


def _host_plant(arrs, name, ij, value):
    """the host arrays with `value` at ij of arrs[name] (a pad cell lies outside the array: nothing changes)"""
    out = dict(arrs)
    if SV.in_array(ij, *arrs[name].shape):
        a = arrs[name].copy()
        a[ij] = value
        out[name] = a
    return out


def _same_footprint(got, ref):
    """the non-finite cells agree: NaN for NaN, +Inf for +Inf, -Inf for -Inf (grids whose spacings are not exact: finite cells
    differ in the last bits, which tests/test_gpu_flow.py bounds)"""
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)) and
            np.array_equal(np.isneginf(got), np.isneginf(ref)))


def _plants(nx, ny):
    return [(pname, ij, vname, v) for pname, ij in SV.plant_positions(nx, ny) for vname, v in zip(SV.VALUE_IDS, SV.VALUES)]


# ======================================================================================================================
# 1. the flow kernels
# ======================================================================================================================
@pytest.mark.parametrize("with_force", [False, True], ids=["noforce", "force"])
@pytest.mark.parametrize("with_prev", [False, True], ids=["first", "ab2"])
@pytest.mark.parametrize("shape", FLOW_SHAPES, ids=SHAPE_IDS)
def test_flow_rhs_planted(shape, with_prev, with_force):
    """mg_dev_flow_rhs: psi feeds the velocity maximum m and the footprints of f and N; w, n_prev and force feed sum f^2 and
    the footprints.  Participating cells of m: the four neighbours of interior cells, i.e. everything but the corners (and the
    pad); of the sums: what the restatement's stencils reach from interior cells."""
    lib = _lib.load()
    nx, ny = shape
    hx, hy = O.grid_spacing(nx, ny, F.UNIT)
    ld = F._lib_pitch(ny) + 4
    rng = np.random.default_rng(11 * nx + ny + 2 * with_prev + with_force)
    host = dict(zip(("psi", "w", "n_prev", "force"), (rng.standard_normal(shape) for _ in range(4))))
    nu, dt, c0, c1 = 0.02, 0.01, 1.25, -0.25
    dev = {k: F.Field(a, ld) for k, a in host.items()}
    fo, no = F.Field(np.full(shape, np.nan), ld), F.Field(np.full(shape, np.nan), ld)
    out2, scratch = F._scalars(2), F._scratch(nx, ny)
    fields = ["psi", "w"] + (["n_prev"] if with_prev else []) + (["force"] if with_force else [])
    dyadic = F._dyadic(shape, F.UNIT)

    def launch():
        _lib.check(lib.mg_dev_flow_rhs(nx, ny, ld, hx, hy, nu, dt, c0, c1, dev["psi"].ptr, dev["w"].ptr, dev["n_prev"].ptr if with_prev else None,
                                       dev["force"].ptr if with_force else None, fo.ptr, no.ptr, F._p(scratch), F._p(out2), None))
        _torch().cuda.synchronize()
        return fo.field().copy(), no.field().copy(), out2.cpu().numpy().copy()

    def restate(h):
        with np.errstate(all="ignore"):
            return R.rhs(h["psi"], h["w"], nu, dt, hx, hy, c0, c1, h["n_prev"] if with_prev else None, h["force"] if with_force else None)

    base = launch()
    assert np.isfinite(base[2]).all()
    nonfinite_m = nonfinite_ss = 0
    for name in fields:
        for pname, ij, vname, v in _plants(nx, ny):
            key = (name, pname, vname)
            old = _plant(dev[name].t, ij, v)
            got_f, got_n, (got_ss, got_m) = launch()
            again = launch()
            _plant(dev[name].t, ij, old)
            want_f, want_n, want_ss, want_m = restate(_host_plant(host, name, ij, v))
            assert SV.same_special(got_n, want_n), key
            assert SV.same_special(got_f, want_f) if dyadic else _same_footprint(got_f, want_f), key
            assert SV.same_special(got_m, want_m), (key, got_m, want_m)
            assert SV.same_sum(got_ss, want_ss), (key, got_ss, want_ss)
            for a, b in zip((got_f, got_n, np.array([got_ss, got_m])), again):
                assert SV.same_special(a, b), key                                  # the same bits on every run
            if name != "psi" or SV.is_corner(ij, nx, ny) or pname == "pad":
                assert got_m == base[2][1], key                                    # m reads psi alone, and neither its corners nor the pad
            if not SV.in_array(ij, nx, ny) or (not SV.is_interior(ij, nx, ny) and name in ("n_prev", "force")):
                assert got_ss == base[2][0] and np.array_equal(got_f, base[0]) and np.array_equal(got_n, base[1]), key      # cells no stencil reaches
            nonfinite_m += not math.isfinite(got_m)
            nonfinite_ss += not math.isfinite(got_ss)
    assert nonfinite_m >= 3 * 6 and nonfinite_ss >= 3 * 3 * len(fields)          # the plants did reach the reductions
    assert np.array_equal(launch()[2], base[2])                                  # and the fields are as they were


@pytest.mark.parametrize("shape", FLOW_SHAPES, ids=SHAPE_IDS)
def test_flow_diag_planted(shape):
    """mg_dev_flow_diag: {sum psi w, sum w^2, m}.  The ring of w and the corners of psi do not participate."""
    lib = _lib.load()
    nx, ny = shape
    ld = F._lib_pitch(ny) + 4
    rng = np.random.default_rng(5 * nx + ny)
    host = {"psi": rng.standard_normal(shape), "w": rng.standard_normal(shape)}
    dev = {k: F.Field(a, ld) for k, a in host.items()}
    out3, scratch = F._scalars(3), F._scratch(nx, ny)
    scale = float(np.sum(np.abs(host["psi"][1:-1, 1:-1] * host["w"][1:-1, 1:-1])))

    def launch():
        _lib.check(lib.mg_dev_flow_diag(nx, ny, ld, dev["psi"].ptr, dev["w"].ptr, F._p(scratch), F._p(out3), None))
        _torch().cuda.synchronize()
        return out3.cpu().numpy().copy()

    base = launch()
    assert np.isfinite(base).all()
    seen = 0
    for name in ("psi", "w"):
        for pname, ij, vname, v in _plants(nx, ny):
            key = (name, pname, vname)
            old = _plant(dev[name].t, ij, v)
            got, again = launch(), launch()
            _plant(dev[name].t, ij, old)
            h = _host_plant(host, name, ij, v)
            with np.errstate(all="ignore"):
                e, z, m = R.diag(h["psi"], h["w"])
            if math.isfinite(e):                                                   # a sum of both signs: the bound of tests/test_gpu_flow.py
                assert abs(got[0] - e) <= 1e-13 * scale, (key, got[0], e)
            else:
                assert SV.same_special(got[0], e), (key, got[0], e)
            assert SV.same_sum(got[1], z), (key, got[1], z)
            assert SV.same_special(got[2], m), (key, got[2], m)
            assert SV.same_special(got, again), key
            outside = not SV.in_array(ij, nx, ny) or (name == "w" and not SV.is_interior(ij, nx, ny)) or (name == "psi" and SV.is_corner(ij, nx, ny))
            if outside:
                assert np.array_equal(G.bits(got), G.bits(base)), key
            else:
                seen += not np.isfinite(got).all()
    assert seen >= 3 * 6
    assert np.array_equal(G.bits(launch()), G.bits(base))


@pytest.mark.parametrize("with_old", [False, True], ids=["noold", "old"])
@pytest.mark.parametrize("shape", FLOW_SHAPES, ids=SHAPE_IDS)
def test_flow_interior_planted(shape, with_old):
    """mg_dev_flow_interior: max |w - w_old| runs over ALL cells, ring and corners included, the pad excluded (0 without
    w_old, whatever w holds); sum out^2 over the interior only; out = w with a zero ring."""
    lib = _lib.load()
    nx, ny = shape
    ld = F._lib_pitch(ny) + 4
    rng = np.random.default_rng(7 * nx + ny + with_old)
    host = {"w": rng.standard_normal(shape), "old": rng.standard_normal(shape)}
    dev = {k: F.Field(a, ld) for k, a in host.items()}
    fo, out2, scratch = F.Field(np.full(shape, np.nan), ld), F._scalars(2), F._scratch(nx, ny)

    def launch():
        _lib.check(lib.mg_dev_flow_interior(nx, ny, ld, dev["w"].ptr, dev["old"].ptr if with_old else None, fo.ptr, F._p(scratch), F._p(out2), None))
        _torch().cuda.synchronize()
        return fo.field().copy(), out2.cpu().numpy().copy()

    base = launch()
    assert np.isfinite(base[1]).all()
    seen_max = 0
    for name in ("w", "old") if with_old else ("w",):
        for pname, ij, vname, v in _plants(nx, ny):
            key = (name, pname, vname)
            old = _plant(dev[name].t, ij, v)
            (got, (ss, mx)), again = launch(), launch()
            _plant(dev[name].t, ij, old)
            h = _host_plant(host, name, ij, v)
            want = R.interior(h["w"])
            with np.errstate(all="ignore"):
                want_ss = float(np.sum(want * want))
                want_mx = float(np.max(np.abs(h["w"] - h["old"]))) if with_old else 0.0
            assert SV.same_special(got, want), key
            assert SV.same_sum(ss, want_ss), (key, ss, want_ss)
            assert SV.same_special(mx, want_mx), (key, mx, want_mx)
            assert SV.same_special(got, again[0]) and SV.same_special(np.array([ss, mx]), again[1]), key
            if pname == "pad":
                assert np.array_equal(G.bits(np.array([ss, mx])), G.bits(base[1])), key
            elif with_old:
                assert not math.isfinite(mx), key                                  # every cell of the array feeds the maximum
                seen_max += 1
            if name == "old" or not SV.is_interior(ij, nx, ny):
                assert ss == base[1][0] and np.array_equal(got, base[0]), key
    assert (seen_max >= 3 * 9 * 2) if with_old else (seen_max == 0)


# ======================================================================================================================
# 2. mg_dev_sumsq
# ======================================================================================================================
@pytest.mark.parametrize("dt", G.DT)
@pytest.mark.parametrize("shape", [(9, 10), (33, 66), (65, 131)], ids=lambda s: "%dx%d" % s)
def test_sumsq_planted(shape, dt):
    """inside the window: non-finite as NumPy's sum of the squared fp64-cast cells; outside it (other rows and columns, the pad):
    the bits of the unplanted run"""
    import test_gpu_dev_calls as T
    s = T._env()
    nx, ny = shape
    case = dict(entry="sumsq", dt=dt, nx=nx, ny=ny, pf="lib", seed=3 * nx + ny, id="planted")
    ops = T._ops(case)
    A = G.build_arrays(case, s["dev"])["u"]
    host = A.host()[G.GUARD:G.GUARD + nx, :ny]
    windows = {"full": (0, nx, 0, ny), "interior": (1, nx - 1, 1, ny - 1), "odd": (1, nx - 1, 3, ny - 2), "row": (nx // 2, nx // 2 + 1, 0, ny)}

    def launch(w):
        return float(ops.sumsq(A.view, *w).cpu().numpy()[0])

    inside = 0
    for wname, w in windows.items():
        base = launch(w)
        ref = math.fsum((host[w[0]:w[1], w[2]:w[3]].astype(np.float64) ** 2).ravel().tolist())
        assert math.isfinite(base) and abs(base - ref) <= 1e-12 * ref
        for pname, ij, vname, v in _plants(nx, ny):
            key = (wname, pname, vname)
            old = _plant(A.full, ij, v, G.GUARD)
            got, again = launch(w), launch(w)
            _plant(A.full, ij, old, G.GUARD)
            assert SV.same_special(got, again), key
            if w[0] <= ij[0] < w[1] and w[2] <= ij[1] < w[3]:
                h = host.astype(np.float64)
                h[ij] = v
                with np.errstate(all="ignore"):
                    want = float(np.sum(h[w[0]:w[1], w[2]:w[3]] ** 2))
                assert not math.isfinite(want) and SV.same_special(got, want), (key, got, want)
                inside += 1
            else:
                assert got == base, (key, got, base)
        assert launch(w) == base
    assert inside >= 3 * 12


# ======================================================================================================================
# 3. the flow stepper on poisoned states
# ======================================================================================================================
TOL = 1e-10
SPEEDS = (0.0, 0.0, 0.0, 1.0)


def _cavity(n, nu, max_cycles):
    return mg.VorticityStreamSolver(mg.Grid(n, n), nu, "no_slip", {"top": 1.0}, tolerance=TOL, max_cycles=max_cycles)


def _poison(s, which, ij, value=SV.NAN):
    """plant `value` in a field of the stepper through mg_flow_set_device, which copies the field as it is"""
    t = _torch().empty((s.nx, F._lib_pitch(s.ny)), dtype=_torch().float64, device="cuda")
    s.get_device(which, t)
    t[ij[0], ij[1]] = value
    s.set_device(which, t)


def _nan_pattern(*vals):
    return tuple(math.isnan(v) for v in vals)


@pytest.mark.parametrize("which", ["omega", "psi"])
def test_flow_step_on_a_poisoned_state(which):
    """one NaN in omega or in psi, one step with max_cycles = 4: the step returns (MG_OK) and cfl, rhs_norm, omega_change, the
    residuals and the flags have the restatement's NaN-ness and values"""
    n = 17
    dt = 0.5 / (n - 1)
    w0, _ = F._smooth_state((n, n), np.random.default_rng(3))
    ref = R.Flow(n, n, 0.01, R.NO_SLIP, SPEEDS, solver=R.CycleSolver(n, n, tol=TOL, max_cycles=50))
    ref.set_state(w0)
    ref.step(dt)
    ref.solver = R.CycleSolver(n, n, tol=TOL, max_cycles=4)
    with _cavity(n, 0.01, 50) as s:
        s.set_vorticity(w0)
        assert s.step(dt)["converged"]
        ij = (n // 2, n // 2 + 1)
        _poison(s, which, ij)
        (ref.w if which == "omega" else ref.psi)[ij] = SV.NAN
        m = s.velocity_max()
        assert math.isnan(m) == (which == "psi") == math.isnan(R.velocity_max(ref.psi))
        info = s.step(dt, max_cycles=4)                                          # returns: MG_OK
        with np.errstate(all="ignore"):
            winfo = ref.step(dt)
        got = (info["cfl"], info["rhs_norm"], info["omega_change"], info["final_residual"], info["psi_final_residual"])
        want = (winfo["cfl"], winfo["rhs_norm"], winfo["omega_change"], winfo["omega"]["final_residual"], winfo["psi"]["final_residual"])
        print(which, "device", got, "restatement", want)
        assert _nan_pattern(*got) == _nan_pattern(*want)
        assert math.isnan(info["rhs_norm"]) and math.isnan(info["omega_change"]) and math.isnan(info["cfl"]) == (which == "psi")
        assert math.isnan(info["initial_residual"]) and math.isnan(info["psi_initial_residual"]) and math.isnan(info["psi_rhs_norm"])
        for g, w in zip(got, want):
            if not math.isnan(w):                # two solves to 1e-10 behind it, differenced over h: a check of sanity, not of bits
                np.testing.assert_allclose(g, w, rtol=1e-6)
        assert (info["cycles"], info["psi_cycles"]) == (4, 4) == (winfo["omega"]["cycles"], winfo["psi"]["cycles"])
        assert not info["converged"] and not info["omega_converged"] and not info["psi_converged"]
        assert not winfo["omega"]["converged"] and not winfo["psi"]["converged"]
        assert np.isnan(s.vorticity).any() and np.isnan(s.stream_function).any()
        assert math.isnan(s.velocity_max())


def test_run_to_steady_reports_a_blow_up():
    """the cavity at 17^2, nu = 1e-3, dt = 0.5 (CFL far above 1) from rest: tests/test_special_values_cpu.py shows that the
    restatement is non-finite within 40 steps.  With maxima formed by fmax the NaN state reported omega_change = 0 and this
    returned converged: True."""
    n = 17
    with _cavity(n, 1e-3, 4) as s:
        out = s.run_to_steady(0.5, max_steps=40)
        print("run_to_steady:", {k: out.get(k) for k in ("steps", "rate", "converged", "diverged", "all_solves_converged")})
        assert out["converged"] is False, "run_to_steady reports convergence on a state that has blown up"
        assert out["diverged"] is True
        assert len(s.history) == out["steps"] == s.steps <= 40
        assert not np.isfinite(s.vorticity).all()
    with _cavity(n, 1e-3, 4) as s:                                                # the same steps by hand: where the first non-finite one is
        first = None
        for k in range(1, 41):
            info = s.step(0.5)
            if not (math.isfinite(info["omega_change"]) and math.isfinite(info["cfl"])):
                first = k
                break
        print("first non-finite step", first, "cfl", info["cfl"], "omega_change", info["omega_change"])
        assert first == out["steps"]                                               # it stopped there, not at the cap
    with _cavity(33, 0.01, 50) as s:                                              # a run that does not blow up: the new key is False
        out = s.run_to_steady(0.5 / 32, rate_tol=1e30, max_steps=3)
        assert out["converged"] is True and out["diverged"] is False and out["steps"] == 1


def test_advance_refuses_a_non_finite_velocity_maximum():
    n = 17
    with _cavity(n, 0.01, 50) as s:
        with pytest.raises(ValueError, match="at rest"):
            s.advance(0.1)                                                       # m == 0 stays what it was
        s.step(0.5 / (n - 1))
        _poison(s, "psi", (5, 6))
        before = s.steps
        with pytest.raises(FloatingPointError, match="velocity maximum is not finite"):
            s.advance(s.time + 0.1)
        assert s.steps == before
        _poison(s, "psi", (5, 6), float("inf"))
        with pytest.raises(FloatingPointError, match="velocity maximum is not finite"):
            s.advance(s.time + 0.1)


def test_flow_stepper_is_usable_after_poison():
    """after a poisoned step mg_flow_set_state with a clean field gives the steps of a fresh stepper, bit for bit"""
    n = 17
    dt = 0.5 / (n - 1)
    w0, _ = F._smooth_state((n, n), np.random.default_rng(4))

    def three_steps(s):
        first = s.set_vorticity(w0)
        infos = [s.step(dt), s.step(dt / 2), s.step(dt)]
        keys = ("cfl", "rhs_norm", "omega_change", "initial_residual", "final_residual", "psi_final_residual", "cycles", "psi_cycles", "converged")
        return s.vorticity, s.stream_function, s._get("N"), [first["psi_final_residual"]] + [i[k] for i in infos for k in keys]

    with _cavity(n, 0.01, 50) as fresh:
        want = three_steps(fresh)
    with _cavity(n, 0.01, 50) as s:
        s.set_vorticity(w0)
        s.step(dt)
        _poison(s, "omega", (4, 9))
        _poison(s, "psi", (9, 4), float("inf"))
        info = s.step(dt, max_cycles=4)
        assert not info["converged"] and math.isnan(info["omega_change"])
        s.step(dt, max_cycles=2)                                                 # every field of the stepper is NaN by now
        assert np.isnan(s.vorticity[1:-1, 1:-1]).all() and np.isnan(s._get("N")[1:-1, 1:-1]).all()
        got = three_steps(s)
    for a, b in zip(got[:3], want[:3]):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes()
    assert got[3] == want[3]


# ======================================================================================================================
# 4. mg_handle after a poisoned solve
# ======================================================================================================================
PRECISIONS = {"double": _lib.MG_PREC_DOUBLE, "single": _lib.MG_PREC_SINGLE, "mixed": _lib.MG_PREC_MIXED_LEVELS, "adaptive": _lib.MG_PREC_ADAPTIVE,
              "defect": _lib.MG_PREC_DEFECT}


def _handle(n, precision, speculate):
    from mixed_precision_multigrid_solvers_for_pdes_amd.facade import default_max_levels
    cfg = _lib.MgConfig(n, n, 0.0, 1.0, 0.0, 1.0, -1.0, default_max_levels(n, n), _lib.MG_CYCLE_V, 2, 2, _lib.MG_JACOBI, 0.8, 1e-12, 1000,
                        PRECISIONS[precision], 1e-6, 4.0, 0, 0, 0, 0, 2, 1, 0, speculate, 0, 0)
    h = C.c_void_p(None)
    _lib.check(_lib.load().mg_create(C.byref(cfg), C.byref(h)))
    return h


def _solve(h, rhs, tol, cycles):
    lib = _lib.load()
    u = np.full(rhs.shape, np.nan)
    hist = np.full(cycles, -1.0)
    codes = np.full(cycles, -1, dtype=np.int32)
    n_iter, conv, stats = C.c_int(-1), C.c_int(-1), _lib.MgStats()
    rc = lib.mg_solve(h, _lib.ptr(rhs), None, _lib.ptr(u), _lib.MG_F64, tol, cycles, hist.ctypes.data_as(C.POINTER(C.c_double)), cycles,
                      C.byref(n_iter), C.byref(conv), codes.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(stats))
    return rc, u, hist, codes, n_iter.value, conv.value, stats


@pytest.mark.parametrize("speculate", [0, 2], ids=["plain", "speculate"])
@pytest.mark.parametrize("precision", list(PRECISIONS))
@pytest.mark.parametrize("n", [33, 129])
def test_handle_is_usable_after_a_poisoned_solve(n, precision, speculate):
    """a NaN in the right-hand side, capped at 6 cycles: MG_OK, six NaN norms, converged = 0 (mg_set_rhs validates nothing:
    include/mghip.h); then four clean cycles on the same handle: iterate, history and precision codes of a fresh handle"""
    lib = _lib.load()
    rhs = np.ascontiguousarray(O.sine_rhs(n, n), dtype=np.float64)
    bad = rhs.copy()
    bad[n // 2, n // 3] = SV.NAN
    fresh = _handle(n, precision, speculate)
    try:
        rc, u_want, hist_want, codes_want, it_want, conv_want, _ = _solve(fresh, rhs, 0.0, 4)
        assert rc == _lib.MG_OK and it_want == 4 and np.isfinite(u_want).all() and np.isfinite(hist_want).all()
    finally:
        lib.mg_destroy(fresh)
    h = _handle(n, precision, speculate)
    try:
        rc, u, hist, codes, it, conv, stats = _solve(h, bad, 1e-10, 6)
        print(n, precision, speculate, "poisoned: rc", rc, "cycles", it, "converged", conv, "history", hist, "codes", codes, "switches",
              stats.precision_switches, "initial", stats.initial_residual)
        assert rc == _lib.MG_OK and it == 6 and conv == 0
        assert np.isnan(hist).all() and math.isnan(stats.initial_residual)
        assert stats.precision_switches == 0 and len(set(codes.tolist())) == 1   # no policy decision is taken on a NaN norm
        assert np.isnan(u).any()
        rc, u, hist, codes, it, conv, _ = _solve(h, rhs, 0.0, 4)
        assert rc == _lib.MG_OK and (it, conv) == (it_want, conv_want)
        assert np.array_equal(codes, codes_want), (codes, codes_want)
        assert hist.tobytes() == hist_want.tobytes(), (hist, hist_want)
        assert u.tobytes() == u_want.tobytes()
    finally:
        lib.mg_destroy(h)


# ======================================================================================================================
# 5. the legs: a planted value in u or rhs against NumpyOps -- stored arrays, coarse right-hand side and the norm window
# ======================================================================================================================
def _leg_case(entry, dt, shape, **kw):
    nx, ny = shape
    c = dict(entry=entry, disp="compare", dt=dt, dtc=dt, comp=dt, nx=nx, ny=ny, nxc=(nx + 1) // 2, nyc=(ny + 1) // 2, ci=0, cj=0, pf="lib", pc="min",
             sides=15, sm=0, omega=0.8, poff=0, coeff=-1.0, nsweep=2, nsweep_pre=1, zero_init=0, rect=None, sp="eq",
             window=(nx // 3, nx // 3 + max(1, nx // 2), ny // 4 + 1, ny // 4 + 1 + max(1, ny // 2)), seed=1000 * nx + ny)
    c["hx"], c["hy"], c["dyadic"] = G.SPACINGS["eq"]
    c.update(kw)
    c["id"] = "%s-%s-%dx%d-planted" % (entry, dt, nx, ny)
    return c


def _run_planted(case, plants):
    """the case on the device and through the restatement with `plants` = [(array name, (i, j), value)] written into the inputs"""
    import test_gpu_dev_calls as T
    s = T._env()
    A, Rr = G.build_arrays(case, s["dev"]), G.build_arrays(case, "cpu")
    for name, ij, v in plants:
        A[name].full[G.GUARD + ij[0], ij[1]] = v
        Rr[name].full[G.GUARD + ij[0], ij[1]] = v
    rops = s["Ref"](G.NPDT[case["comp"]])
    with np.errstate(all="ignore"):
        ref_sum = G.invoke(case, rops, Rr)
    before = G.snapshot(A)
    got_sum = G.invoke(case, T._ops(case), A)
    s["torch"].cuda.synchronize()
    return G.snapshot(A), got_sum, G.snapshot(Rr), ref_sum, rops, before


TINY_LEG = (33, 130)
RB_LEG = (1102, 1122)


@pytest.mark.parametrize("name", ["u", "rhs"])
@pytest.mark.parametrize("entry,dt", [("up_leg", "f64"), ("up_leg", "f32"), ("down_leg", "f64"), ("down_leg", "f32")])
def test_small_legs_planted(entry, dt, name):
    """the 8-row family at (33, 130): every position and value in u and in rhs; every stored array and the sum of r^2 over a
    window that some footprints reach and others do not"""
    case = _leg_case(entry, dt, TINY_LEG)
    nx, ny = TINY_LEG
    fam, ti, tj = G.leg_tiles(case)
    nonfinite = finite = 0
    for pname, ij, vname, v in [(p, ij, vn, v) for p, ij in SV.plant_positions(nx, ny, ti, tj) for vn, v in zip(SV.VALUE_IDS, SV.VALUES)]:
        if pname == "pad":
            continue                                     # the restatement's arrays carry the pad too: planted in both, read by neither
        got, got_sum, ref, ref_sum, rops, before = _run_planted(case, [(name, ij, v)])
        G.compare_call(case, got, got_sum, ref, ref_sum, rops, before, special=True)
        again = _run_planted(case, [(name, ij, v)])
        for k in G.OUTPUTS[entry]:
            assert SV.same_special(got[k], again[0][k]), (pname, vname, k)
        if entry == "up_leg":
            assert SV.same_special(got_sum, again[1])
            nonfinite += not math.isfinite(ref_sum)
            finite += math.isfinite(ref_sum)
    if entry == "up_leg":
        assert nonfinite >= 3 and finite >= 3           # footprints inside the window and outside it


def test_pad_of_a_leg_is_not_read():
    """Inf in the pad column of u and rhs (the sentinel NaN is there in every other test): the bits of the unplanted run"""
    for entry in ("up_leg", "down_leg"):
        case = _leg_case(entry, "f64", (33, 131))
        base = _run_planted(case, [])
        got = _run_planted(case, [("u", (16, 131), float("inf")), ("rhs", (17, 131), float("-inf"))])
        specs = G.array_specs(case)
        for k in G.OUTPUTS[entry]:                           # the pad of an output may be stored with its vector: exempt (include/mghip.h)
            onx, ony = specs[k][1], specs[k][2]
            cut = lambda a: G.bits(a[G.GUARD:G.GUARD + onx, :ony])
            assert np.array_equal(cut(got[0][k]), cut(base[0][k])), (entry, k)
        assert got[1] == base[1]


@pytest.mark.parametrize("entry,plants", [
    ("span_leg", [("u", (551, 561), SV.NAN)]), ("span_leg", [("rhs", (400, 700), float("inf"))]), ("span_leg", [("u", (0, 561), SV.NAN)]),
    ("down_leg", [("u", (551, 561), SV.NAN)]), ("down_leg", [("rhs", (1100, 1120), float("-inf"))])],
    ids=["span-u-nan", "span-rhs-inf", "span-ring-nan", "down-u-nan", "down-rhs-inf"])
def test_register_blocked_legs_planted(entry, plants):
    """the spanning leg and one register-blocked down leg at (1102, 1122), fp64"""
    case = _leg_case(entry, "f64", RB_LEG, nsweep_pre=2)
    got, got_sum, ref, ref_sum, rops, before = _run_planted(case, plants)
    G.compare_call(case, got, got_sum, ref, ref_sum, rops, before, special=True)
    if entry == "span_leg":
        print(plants, "sum", got_sum, "reference", ref_sum)
    # the plant did reach what the leg stores: the reference holds non-finite values that are not the sentinel
    assert any(((~np.isfinite(ref[k])) & (G.bits(ref[k]) != G.SENT_BITS[8])).any() for k in G.OUTPUTS[entry])


# ======================================================================================================================
# 6. the Krylov kernels: mg_dev_pcg_dots, mg_dev_pcg_scalars
# ======================================================================================================================
@pytest.mark.parametrize("shape", [(9, 130), (35, 67)], ids=lambda s: "%dx%d" % s)
def test_pcg_dots_planted(shape):
    """r . z and z . q over interior cells: ring and pad excluded (include/mghip.h); each operand separately"""
    import test_gpu_pcg as P
    lib = _lib.load()
    nx, ny = shape
    ld = P._pitches(ny)[0]
    rng = np.random.default_rng(nx + ny)
    host = dict(zip("rzq", (rng.standard_normal(shape) for _ in range(3))))
    dev = {k: P.Field(a, ld) for k, a in host.items()}
    rz, zq, scratch = P._scalar(), P._scalar(), P._scratch(nx, ny)

    def launch(with_q):
        rz.fill_(float("nan")); zq.fill_(float("nan"))
        _lib.check(lib.mg_dev_pcg_dots(nx, ny, ld, dev["r"].ptr, dev["z"].ptr, dev["q"].ptr if with_q else None, P._p(scratch), P._p(rz), P._p(zq), None))
        _torch().cuda.synchronize()
        return np.array([float(rz.cpu()[0]), float(zq.cpu()[0])])

    inner = lambda a, b: float(np.sum(a[1:-1, 1:-1] * b[1:-1, 1:-1]))
    for with_q in (False, True):
        base = launch(with_q)
        hit = 0
        for name in ("r", "z", "q") if with_q else ("r", "z"):
            for pname, ij, vname, v in _plants(nx, ny):
                key = (with_q, name, pname, vname)
                old = _plant(dev[name].t, ij, v, P.GUARD)
                got, again = launch(with_q), launch(with_q)
                _plant(dev[name].t, ij, old, P.GUARD)
                assert SV.same_special(got, again), key
                if not SV.is_interior(ij, nx, ny):
                    assert np.array_equal(G.bits(got), G.bits(base)), key          # ring and pad: the bits of the unplanted run
                    continue
                h = _host_plant(host, name, ij, v)
                with np.errstate(all="ignore"):
                    want = (inner(h["r"], h["z"]), inner(h["z"], h["q"]) if with_q else SV.NAN)
                for g, w, b in zip(got, want, base):
                    if math.isfinite(w):
                        assert g == b, key                                         # the planted operand is not in this product
                    else:
                        assert SV.same_special(g, w), (key, g, w)
                hit += 1
        assert hit >= 3 * 3 * 2


def test_pcg_scalars_breakdown_on_non_finite_partials():
    """a NaN or an Inf anywhere among the partial sums of p . q, or in r . z, sets the breakdown flag and leaves alpha = 0"""
    import test_gpu_pcg as P
    lib = _lib.load()
    torch = _torch()
    RZ, RZ_OLD, ZQ, PQ, ALPHA, BETA, RR, FLAG = range(8)

    def step(op, sc, pa, pb=None):
        ta = torch.tensor(pa, dtype=torch.float64, device="cuda")
        tb = None if pb is None else torch.tensor(pb, dtype=torch.float64, device="cuda")
        _lib.check(lib.mg_dev_pcg_scalars(op, P._p(ta), len(pa), None if tb is None else P._p(tb), 0 if pb is None else len(pb), P._p(sc), None))
        torch.cuda.synchronize()
        return sc.cpu().numpy()

    sc = torch.full((10,), 7.0, dtype=torch.float64, device="cuda")
    for n in (1, 5, 3000):                                   # one partial, a few, more than the workgroup has threads
        for at in sorted({0, n // 2, n - 1}):
            for bad in SV.VALUES:
                pa = [0.5] * n
                pa[at] = bad
                s = step(0, sc, [1.0, 2.0])
                assert s[FLAG] == 0.0 and s[RZ] == 3.0
                s = step(3, sc, pa)                          # p . q
                assert s[FLAG] == 1.0 and s[ALPHA] == 0.0, (n, at, bad)
                assert SV.same_special(float(s[PQ]), float(np.sum(np.array(pa))))
                assert step(4, sc, [1.0])[9] == 1.0          # posted with the norm
                rz = [1.0] * n
                rz[at] = bad
                s = step(0, sc, rz)                          # r . z: the first dots clear the flag and keep the sum as it is
                assert s[FLAG] == 0.0 and not math.isfinite(s[RZ])
                s = step(3, sc, [0.5, 0.25])
                assert s[FLAG] == 1.0 and s[ALPHA] == 0.0 and s[PQ] == 0.75, (n, at, bad)
    s = step(0, sc, [1.0, 2.0])                              # and the block is usable again
    s = step(3, sc, [0.5, 0.25])
    assert s[FLAG] == 0.0 and s[ALPHA] == 4.0


# ======================================================================================================================
# 7. the heat kernels
# ======================================================================================================================
@pytest.mark.parametrize("scheme", ["explicit_euler", "implicit_euler", "crank_nicolson", "bdf2"])
@pytest.mark.parametrize("shape", FLOW_SHAPES, ids=SHAPE_IDS)
def test_heat_rhs_planted(shape, scheme):
    """mg_dev_heat_rhs: the stored field and its sum of squares, a plant in u, u_prev (BDF2) and the source"""
    import heat_device_reference as HR
    import test_gpu_heat_device as HD
    lib = _lib.load()
    nx, ny = shape
    hx, hy = O.grid_spacing(nx, ny, HD.UNIT)
    ld = HD._lib_pitch(ny) + 4
    rng = np.random.default_rng(13 * nx + ny)
    host = dict(zip(("u", "prev", "src"), (rng.standard_normal(shape) for _ in range(3))))
    dev = {k: HD.Field(a, ld) for k, a in host.items()}
    fo, ss, scratch = HD.Field(np.full(shape, np.nan), ld), HD._scalar(), HD._scratch(nx, ny)
    alpha, dt, g0, g1 = 0.7, 0.01, 0.3, 1.25
    dyadic = HD._dyadic(shape, HD.UNIT)

    def launch():
        _lib.check(lib.mg_dev_heat_rhs(HR.SCHEME_CODES[scheme], nx, ny, ld, hx, hy, alpha, dt, dev["u"].ptr, dev["prev"].ptr if scheme == HR.BDF2 else None,
                                       dev["src"].ptr, g0, g1, fo.ptr, HD._p(scratch), HD._p(ss), None))
        _torch().cuda.synchronize()
        return fo.field().copy(), float(ss.cpu()[0])

    base = launch()
    hit = 0
    for name in ("u", "src") + (("prev",) if scheme == HR.BDF2 else ()):
        for pname, ij, vname, v in _plants(nx, ny):
            key = (name, pname, vname)
            old = _plant(dev[name].t, ij, v, HD.GUARD)
            (got, total), again = launch(), launch()
            _plant(dev[name].t, ij, old, HD.GUARD)
            h = _host_plant(host, name, ij, v)
            with np.errstate(all="ignore"):
                want = HR.rhs(scheme, h["u"], dt, alpha, hx, hy, h["prev"], h["src"], g0, g1)
                want_ss = float(np.sum(want * want))
            assert SV.same_special(got, want) if dyadic else _same_footprint(got, want), key
            assert SV.same_sum(total, want_ss, 1e-12), (key, total, want_ss)
            assert SV.same_special(got, again[0]) and SV.same_special(total, again[1]), key
            if pname == "pad":
                assert total == base[1] and np.array_equal(got, base[0]), key
            hit += not math.isfinite(total)
    assert hit >= 3 * 3 * 2


@pytest.mark.parametrize("shape", FLOW_SHAPES, ids=SHAPE_IDS)
def test_heat_diff_sumsq_planted(shape):
    """mg_dev_heat_diff_sumsq: sum (a - b)^2 over ALL cells of the array, the pad excluded"""
    import test_gpu_heat_device as HD
    lib = _lib.load()
    nx, ny = shape
    ld = HD._lib_pitch(ny) + 4
    rng = np.random.default_rng(17 * nx + ny)
    host = {"a": rng.standard_normal(shape), "b": rng.standard_normal(shape)}
    dev = {k: HD.Field(a, ld) for k, a in host.items()}
    ss, scratch = HD._scalar(), HD._scratch(nx, ny)

    def launch():
        _lib.check(lib.mg_dev_heat_diff_sumsq(nx, ny, ld, dev["a"].ptr, dev["b"].ptr, HD._p(scratch), HD._p(ss), None))
        _torch().cuda.synchronize()
        return float(ss.cpu()[0])

    base = launch()
    for name in ("a", "b"):
        for pname, ij, vname, v in _plants(nx, ny):
            old = _plant(dev[name].t, ij, v, HD.GUARD)
            got, again = launch(), launch()
            _plant(dev[name].t, ij, old, HD.GUARD)
            h = _host_plant(host, name, ij, v)
            with np.errstate(all="ignore"):
                want = float(np.sum((h["a"] - h["b"]) ** 2))
            assert SV.same_special(got, again)
            if pname == "pad":
                assert got == base
            else:
                assert not math.isfinite(want) and SV.same_special(got, want), (name, pname, vname, got, want)
    assert launch() == base


# ======================================================================================================================
# 8. the block kernels of the eigensolver
# ======================================================================================================================
@pytest.mark.parametrize("shape", [(17, 17, 3, 5), (40, 37, 6, 12)], ids=["17x17_p3_q5", "40x37_p6_q12"])
def test_eig_gram_planted(shape):
    """G = U^T V over interior cells.  A NaN at an interior cell of column a of u: exactly row a of G is NaN; of column b of v:
    exactly column b.  A NaN or an Inf at a ring or pad cell of one operand: the bits of the unplanted run."""
    import test_gpu_eig as EG
    nx, ny, p, q = shape
    rng = np.random.default_rng(nx + p)
    u, v = rng.standard_normal((p, nx, ny)), rng.standard_normal((q, nx, ny))
    ld = EG._pitches(ny)[0]
    ub, vb = EG.Block(u, ld, outside=1.0), EG.Block(v, ld, outside=1.0)
    base = EG._gram(ub, 0, p, vb, 0, q, nx, ny)
    assert np.isfinite(base).all()
    for blk, ncols, axis in ((ub, p, 0), (vb, q, 1)):
        for col in sorted({0, ncols // 2, ncols - 1}):
            for pname, ij in SV.plant_positions(nx, ny):
                for v_ in SV.VALUES if not SV.is_interior(ij, nx, ny) else SV.VALUES[:1]:
                    old = blk.t[col, EG.GUARD + ij[0], ij[1]].item()
                    blk.t[col, EG.GUARD + ij[0], ij[1]] = v_
                    got, again = EG._gram(ub, 0, p, vb, 0, q, nx, ny), EG._gram(ub, 0, p, vb, 0, q, nx, ny)
                    blk.t[col, EG.GUARD + ij[0], ij[1]] = old
                    key = (axis, col, pname, v_)
                    assert SV.same_special(got, again), key
                    if SV.is_interior(ij, nx, ny):
                        want_nan = np.zeros((p, q), dtype=bool)
                        if axis == 0:
                            want_nan[col, :] = True
                        else:
                            want_nan[:, col] = True
                        assert np.array_equal(np.isnan(got), want_nan), key
                        assert np.array_equal(G.bits(got[~want_nan]), G.bits(base[~want_nan])), key
                    else:
                        assert np.array_equal(G.bits(got), G.bits(base)), key
    assert np.array_equal(G.bits(EG._gram(ub, 0, p, vb, 0, q, nx, ny)), G.bits(base))


def test_eig_residual_planted():
    """r_c = A x_c - lambda_c x_c on interior cells and sum r_c^2, column by column: a plant in column c of x, of ax or in
    lambda_c changes sumsq[c] and column c of r, and nothing else"""
    import test_gpu_eig as EG
    lib = _lib.load()
    nx, ny, ncols = 40, 37, 6
    rng = np.random.default_rng(ncols)
    x, ax = rng.standard_normal((ncols, nx, ny)), rng.standard_normal((ncols, nx, ny))
    lam = 1.0 + 10.0 * rng.random(ncols)
    ld = EG._pitches(ny)[0]
    xb, axb, rb = EG.Block(x, ld, outside=1.0), EG.Block(ax, ld, outside=1.0), EG.Block(x, ld, fill=np.nan)
    lam_d, ss, scratch = EG._dev(lam), EG._dev(np.full(ncols, np.nan)), EG._scratch(nx, ny)

    def launch():
        _lib.check(lib.mg_dev_eig_residual(nx, ny, ld, ncols, xb.stride, xb.ptr(), axb.ptr(), EG._p(lam_d), rb.ptr(), EG._p(scratch), EG._p(ss), None))
        _torch().cuda.synchronize()
        return rb.fields().copy(), ss.cpu().numpy().copy()

    def restate(x_, ax_, lam_):
        with np.errstate(all="ignore"):
            want = np.zeros_like(x_)
            want[:, 1:-1, 1:-1] = ax_[:, 1:-1, 1:-1] - lam_[:, None, None] * x_[:, 1:-1, 1:-1]
            return want, np.einsum("aij,aij->a", want, want)

    base_r, base_ss = launch()
    others = lambda c: [k for k in range(ncols) if k != c]
    for c in (0, 3, ncols - 1):
        plants = [("x", ij, pn, v) for pn, ij in SV.plant_positions(nx, ny) for v in SV.VALUES] + \
                 [("ax", ij, pn, v) for pn, ij in SV.plant_positions(nx, ny) for v in SV.VALUES] + [("lambda", None, "scalar", v) for v in SV.VALUES]
        for name, ij, pname, v in plants:
            key = (c, name, pname, v)
            if name == "lambda":
                old = lam_d[c].item()
                lam_d[c] = v
            else:
                t = (xb if name == "x" else axb).t
                old = t[c, EG.GUARD + ij[0], ij[1]].item()
                t[c, EG.GUARD + ij[0], ij[1]] = v
            (got_r, got_ss), again = launch(), launch()
            if name == "lambda":
                lam_d[c] = old
            else:
                t[c, EG.GUARD + ij[0], ij[1]] = old
            assert SV.same_special(got_r, again[0]) and SV.same_special(got_ss, again[1]), key
            assert np.array_equal(G.bits(got_r[others(c)]), G.bits(base_r[others(c)])) and np.array_equal(G.bits(got_ss[others(c)]), G.bits(base_ss[others(c)])), key
            x2, ax2, lam2 = x.copy(), ax.copy(), lam.copy()
            if name == "lambda":
                lam2[c] = v
            elif SV.in_array(ij, nx, ny):
                (x2 if name == "x" else ax2)[c][ij] = v
            want_r, want_ss = restate(x2, ax2, lam2)
            assert _same_footprint(got_r[c], want_r[c]), key
            if math.isfinite(want_ss[c]):
                assert got_ss[c] == base_ss[c] and np.array_equal(G.bits(got_r[c]), G.bits(base_r[c])), key        # ring and pad: nothing changes
            else:
                assert SV.same_special(float(got_ss[c]), float(want_ss[c])), (key, got_ss[c], want_ss[c])
    got_r, got_ss = launch()
    assert np.array_equal(G.bits(got_r), G.bits(base_r)) and np.array_equal(G.bits(got_ss), G.bits(base_ss))


# ======================================================================================================================
# 9. the residual norms: the fourth-order scheme's (include/mghip_ho.h) and mg_residual_norm on a handle
# ======================================================================================================================
def test_ho_residual_norm_planted():
    import ho_reference as HO
    import test_gpu_ho as TH
    lib = _lib.load()
    nx = ny = 33
    ld = TH._pitch(ny)
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    rng = np.random.default_rng(33)
    host = {"x": rng.standard_normal((nx, ny)), "g": rng.standard_normal((nx, ny))}
    dev = {k: TH.Field(a, ld) for k, a in host.items()}
    fr, rr, scratch = TH.Field(host["x"], ld, fill=TH.SENTINEL), TH._scalar(), TH._scratch(nx, ny)

    def launch():
        _lib.check(lib.mg_dev_ho_residual(nx, ny, ld, hx, hy, -1.0, 0.0, dev["x"].ptr, dev["g"].ptr, fr.ptr, TH._p(scratch), TH._p(rr), None))
        _torch().cuda.synchronize()
        return fr.field().copy() + 0.0, float(rr.cpu()[0])

    base = launch()
    hit = 0
    for name in ("x", "g"):
        for pname, ij, vname, v in _plants(nx, ny):
            key = (name, pname, vname)
            old = _plant(dev[name].t, ij, v, TH.GUARD)
            (got, total), again = launch(), launch()
            _plant(dev[name].t, ij, old, TH.GUARD)
            h = _host_plant(host, name, ij, v)
            with np.errstate(all="ignore"):
                want = HO.residual(h["x"], h["g"], hx, hy, -1.0, 0.0) + 0.0
                want_ss = float(np.sum(want * want))
            assert SV.same_special(got, want), key
            assert SV.same_sum(total, want_ss), (key, total, want_ss)
            assert SV.same_special(got, again[0]) and SV.same_special(total, again[1]), key
            if math.isfinite(want_ss):
                assert total == base[1], key
            hit += not math.isfinite(total)
    assert hit >= 3 * 3 * 2


def test_handle_residual_norm_planted():
    """mg_residual_norm: NaN for a NaN the residual reads -- any cell of f (r = f on the ring), any cell of u but the corners"""
    lib = _lib.load()
    n = 33
    h = _handle(n, "double", 0)
    rng = np.random.default_rng(1)
    f, u = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    hx = 1.0 / (n - 1)

    def norm(f_, u_):
        out = C.c_double(-1.0)
        _lib.check(lib.mg_set_rhs(h, _lib.ptr(np.ascontiguousarray(f_)), _lib.MG_F64), h)
        _lib.check(lib.mg_set_solution(h, _lib.ptr(np.ascontiguousarray(u_)), _lib.MG_F64), h)
        _lib.check(lib.mg_residual_norm(h, C.byref(out)), h)
        return out.value

    try:
        base = norm(f, u)
        assert abs(base - O.l2_norm(O.residual(u, f, hx, hx, -1.0), hx, hx)) <= 1e-12 * base
        for name in ("f", "u"):
            for pname, ij in SV.plant_positions(n, n):
                if not SV.in_array(ij, n, n):
                    continue                                 # host arrays: no pad
                for v in SV.VALUES:
                    arrs = _host_plant({"f": f, "u": u}, name, ij, v)
                    got = norm(arrs["f"], arrs["u"])
                    with np.errstate(all="ignore"):
                        want = float(O.l2_norm(O.residual(arrs["u"], arrs["f"], hx, hx, -1.0), hx, hx))
                    assert not math.isfinite(want) or (name == "u" and SV.is_corner(ij, n, n)), (name, pname)
                    if math.isfinite(want):
                        assert got == base, (name, pname, v)
                    else:
                        assert SV.same_special(got, want), (name, pname, v, got, want)
        assert norm(f, u) == base
    finally:
        lib.mg_destroy(h)


# ======================================================================================================================
# 10. the other drivers after poison: mg_pcg, mg_eig, mg_heat
# ======================================================================================================================
def test_pcg_breaks_down_on_a_nan_and_is_usable_afterwards():
    from mixed_precision_multigrid_solvers_for_pdes_amd.krylov import PCGEngine
    n = 33
    rhs = np.ascontiguousarray(O.sine_rhs(n, n), dtype=np.float64)
    bad = rhs.copy()
    bad[n // 2, n // 3] = SV.NAN
    with PCGEngine(n, n, max_levels=4) as fresh:
        want_x, want = fresh.solve(rhs, tol=1e-9, max_iterations=20)
        assert want["converged"]
    with PCGEngine(n, n, max_levels=4) as s:
        x, info = s.solve(bad, tol=1e-9, max_iterations=20)
        print("pcg poisoned:", {k: info[k] for k in ("status", "iterations", "converged", "initial_residual", "true_residual")})
        assert info["status"] == "breakdown" and not info["converged"] and info["iterations"] == 0
        assert math.isnan(info["initial_residual"]) and math.isnan(info["true_residual"])
        x, info = s.solve(rhs, tol=1e-9, max_iterations=20)
        assert x.tobytes() == want_x.tobytes() and info["residual_history"] == want["residual_history"] and info["status"] == "converged"


def test_eigensolver_refuses_a_nan_start_and_is_usable_afterwards():
    from mixed_precision_multigrid_solvers_for_pdes_amd.eigen import EigenEngine
    n, m = 33, 3
    rng = np.random.default_rng(8)
    x0 = rng.standard_normal((m, n, n))
    bad = x0.copy()
    bad[1, n // 2, n // 2] = SV.NAN
    with EigenEngine(n, n, max_levels=4, block_size=m) as fresh:
        want_ev, want_vec, want = fresh.solve(x0, tol=1e-8, max_iterations=30)
        assert want["converged"]
    with EigenEngine(n, n, max_levels=4, block_size=m) as s:
        # the Gram matrix of the start block has a NaN row: its Cholesky factorisation fails before the first iteration and
        # mg_eig_solve returns its documented MG_ERR_INVALID_VALUE (include/mghip_eig.h) -- no iteration, no convergence
        with pytest.raises(ValueError, match="not finite"):
            s.solve(bad, tol=1e-8, max_iterations=5)
        bad[1, n // 2, n // 2] = float("inf")
        with pytest.raises(ValueError, match="not finite"):
            s.solve(bad, tol=1e-8, max_iterations=5)
        ev, vec, info = s.solve(x0, tol=1e-8, max_iterations=30)
        assert ev.tobytes() == want_ev.tobytes() and vec.tobytes() == want_vec.tobytes() and info["residual_history"] == want["residual_history"]


def test_heat_stepper_is_usable_after_a_nan_slot():
    from mixed_precision_multigrid_solvers_for_pdes_amd.heat_device import DeviceHeatStepper
    n = 33
    rng = np.random.default_rng(2)
    u0 = rng.standard_normal((n, n))
    bad = _torch().zeros((n, F._lib_pitch(n)), dtype=_torch().float64, device="cuda")
    bad[:, :n] = _torch().from_numpy(u0).cuda()
    bad[n // 2, n // 2] = SV.NAN

    def two_steps(s):
        s.set_slot(0, u0)
        a = s.step("crank_nicolson", 1e-3, 0, 1, tol=1e-10, max_cycles=20)
        b = s.step("bdf2", 1e-3, 1, 2, prev=0, tol=1e-10, max_cycles=20)
        keys = ("rhs_norm", "initial_residual", "final_residual", "cycles", "converged")
        return s.get_slot(1), s.get_slot(2), [i[k] for i in (a, b) for k in keys]

    with DeviceHeatStepper(n, n) as fresh:
        want = two_steps(fresh)
        assert want[2][4] and want[2][9]
    with DeviceHeatStepper(n, n) as s:
        s.set_slot_device(3, bad)                            # copies the field as it is
        info = s.step("crank_nicolson", 1e-3, 3, 1, tol=1e-10, max_cycles=4)
        print("heat poisoned:", info)
        assert not info["converged"] and info["cycles"] == 4
        assert math.isnan(info["rhs_norm"]) and math.isnan(info["initial_residual"]) and math.isnan(info["final_residual"])
        assert np.isnan(s.get_slot(1)).any() and math.isnan(s.diff_norm(1, 3))
        got = two_steps(s)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]
