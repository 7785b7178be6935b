"""MG_PREC_DEFECT on the device against tests/defect_reference.py: every outer step restarted from the device's own iterate (norm,
correction, ring, stepping against mg_iterate), the full-multigrid start, the stop rule, the fp64 floor under a shift, and the
shapes at which the grid-stride loops of launch_defect and d_residual_f32in_f64out wrap.

Bars.  Norms: NumPy's fp64 O.l2_norm(O.residual(u_k, ...)) of the DEVICE's iterate at rtol 1e-12 -- no fp32 arithmetic enters it,
so it is what sees a wrong diag, coeff, ihx2 / ihy2 or pitch.  Corrections: 1e-5 max|e_ref| against `step` from the device's own
u_{k-1} (the project's bar for an fp32 cycle under a shift); zebra: ZEBRA_BAR against the fp64 engine's cycle on the same defect.
Rings and the stepping-against-mg_iterate comparison are bit for bit.  DESIGN.md 5.8 holds the measured figures."""
import os
import sys

import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib
from oracle import mg_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import defect_reference as D                                                      # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _np_norm(u, rhs, dom, shift):
    hx, hy = O.grid_spacing(u.shape[0], u.shape[1], dom)
    return float(O.l2_norm(O.residual(u, rhs, hx, hy, -1.0, shift), hx, hy))


def _close(got, ref, what):
    print("%s: %.17g against NumPy's %.17g (%.2e relative)" % (what, got, ref, abs(got - ref) / abs(ref)))
    assert abs(got - ref) <= D.NORM_RTOL * abs(ref), what


def _same_ring(u, u0):
    assert D.ring_of(u).tobytes() == D.ring_of(u0).tobytes()


def _excess(u_new, u_old, e_ref):
    """max|(u_new - u_old) - e_ref| / max|e_ref|, less what the fp64 sum u_old + e rounds away: the device's correction is only
    visible as the difference of two fp64 iterates, each cell of which carries half an ulp of u_new (a loop that has reached the
    fp64 floor adds corrections below that: zebra at shift 4096 does so after two steps)"""
    diff = np.abs((u_new - u_old) - e_ref) - 0.5 * np.spacing(np.abs(u_new))
    return max(0.0, float(np.max(diff))) / float(np.max(np.abs(e_ref)))


def _engine(nx, ny, kw, shift):
    eng = mg.MultigridEngine(nx, ny, **kw)
    if shift:
        eng.set_shift(shift)
    return eng


# ======================================================================================================================
# 1. step by step against the reference
# ======================================================================================================================
@pytest.mark.parametrize("case", D.CASES, ids=[c["id"] for c in D.CASES])
def test_every_outer_step_against_the_reference(case):
    nx, ny, kw = D.engine_kwargs(case)
    dom, shift, K = kw["domain"], case["shift"], D.K_STEPS
    rhs, u0 = D.case_fields(case)
    with _engine(nx, ny, kw, shift) as eng:
        eng.set_rhs(rhs)
        eng.set_solution(u0)
        n_init = eng.residual_norm()
        us, ns = [u0], []
        for _ in range(K):
            eng.cycle(1)
            us.append(eng.get_solution())
            ns.append(eng.residual_norm())
        eng.set_solution(u0)                                         # the same start through mg_iterate
        info = eng.iterate(0.0, K)
        u_it = eng.get_solution()
    # norms: the device's fp64 defect against NumPy's, of the device's own iterates
    _close(n_init, _np_norm(u0, rhs, dom, shift), "initial norm")
    for k in range(K):
        _close(ns[k], _np_norm(us[k + 1], rhs, dom, shift), "norm after step %d" % (k + 1))
    assert ns[-1] < ns[0] < n_init                                   # a converging loop, so a correction is never added twice
    # ring
    for u in us[1:] + [u_it]:
        _same_ring(u, u0)
    # stepping against mg_iterate
    assert info["precision_codes"] == [3] * K and info["iterations"] == K and not info["converged"]
    assert info["initial_residual"] == n_init and info["residual_history"] == ns
    assert u_it.tobytes() == us[-1].tobytes()
    # corrections
    if case["zebra"]:
        nx, ny, kw64 = D.engine_kwargs(case, precision=_lib.MG_PREC_DOUBLE)
        hx, hy = O.grid_spacing(nx, ny, dom)
        worst = 0.0
        with _engine(nx, ny, kw64, shift) as e64:
            for k in range(K):
                r32 = D.zero_ring(O.residual(us[k], rhs, hx, hy, -1.0, shift).astype(F32))
                e64.set_rhs(r32.astype(F64))
                e64.set_solution(None)
                e64.cycle(1)
                ref = e64.get_solution()
                worst = max(worst, _excess(us[k + 1], us[k], ref))
        print("%s: max|e - e_fp64 engine| / max|e_fp64 engine| = %.3g (bar %.3g)" % (case["id"], worst, D.ZEBRA_BAR))
        assert worst <= D.ZEBRA_BAR
        return
    mgo = D.oracle_for(case)
    worst = 0.0
    for k in range(K):
        e_ref, n_ref = D.step(mgo, us[k], rhs)
        worst = max(worst, _excess(us[k + 1], us[k], e_ref))
    print("%s: max|e - e_ref| / max|e_ref| = %.3g (bar %.3g)" % (case["id"], worst, D.E_BAR))
    if case["id"] not in D.NO_CORRECTION_CHECK:
        assert worst <= D.E_BAR
    # The coarsest iteration's stop test counts boundary cells (r = f there): it can only be met on the zero ring the defect pass
    # writes and the injection carries down.  The correction bar cannot see a ring that is not zeroed (the iteration then runs to
    # its cap: 1e-12 max|e|), the sweep count of the last coarsest visit can: the reference's, give or take the one sweep by which
    # a last-bit difference can move the crossing of 1e-12
    cap, dev, ref = kw["coarse_maxit"], info["last_coarse_sweeps"], mgo.coarse_sweeps[-1]
    print("%s: %d sweeps in the last coarsest visit, reference %d, cap %d" % (case["id"], dev, ref, cap))
    assert abs(dev - ref) <= (1 if ref < cap else 0)


# ======================================================================================================================
# 2. the full-multigrid start
# ======================================================================================================================
FMG_SHAPES = {"129x65": (129, 65, D.WIDE, 5), "65": (65, 65, D.UNIT, 5)}
# (shape, cycle, smoother, cycles per level, shift)
FMG_CASES = [("129x65", "V", "J", 1, 0.0), ("129x65", "W", "R", 2, 160.0), ("129x65", "V", "R", 2, 0.0), ("65", "W", "J", 1, 160.0),
             ("65", "V", "R", 1, 0.0), ("65", "W", "R", 2, 0.0), ("65", "V", "J", 2, 160.0)]


def _fmg_setup(shape, cycle, sm, shift):
    nx, ny, dom, levels = FMG_SHAPES[shape]
    kind, code, omega = D.SMOOTHERS[sm]
    kw = dict(domain=dom, max_levels=levels, cycle=cycle, smoother=code, omega=omega, precision=_lib.MG_PREC_DEFECT)
    mgo = O.MGOracle(nx, ny, domain=dom, max_levels=levels, cycle=cycle, smoother=kind, omega=omega, jacobi_form="vectorized", shift=shift)
    rng = np.random.default_rng(nx + 3 * ny)
    rhs = O.sine_rhs(nx, ny, dom) + 0.05 * rng.standard_normal((nx, ny))
    return nx, ny, dom, kw, mgo, rhs, rng


@pytest.mark.parametrize("shape,cycle,sm,c,shift", FMG_CASES)
def test_fmg_start_is_the_walk_on_the_defect_of_the_resident_iterate(shape, cycle, sm, c, shift):
    """mg_fmg under defect correction: u <- u + e, e the full-multigrid walk on A e = f - A u from the zero correction, u the WHOLE
    resident iterate -- a ring-only u (what mg_solve hands it) and one with a non-zero interior alike"""
    nx, ny, dom, kw, mgo, rhs, rng = _fmg_setup(shape, cycle, sm, shift)
    ring_only = D.ring_start(nx, ny, 11)
    full = ring_only + np.pad(0.1 * rng.standard_normal((nx - 2, ny - 2)), 1)
    with _engine(nx, ny, kw, shift) as eng:
        eng.set_rhs(rhs)
        for what, u0 in (("ring-only", ring_only), ("non-zero interior", full)):
            eng.set_solution(u0)
            eng.fmg(c)
            u = eng.get_solution()
            n = eng.residual_norm()
            e_ref = D.fmg_step(mgo, u0, rhs, c)
            ratio = float(np.max(np.abs((u - u0) - e_ref)) / np.max(np.abs(e_ref)))
            print("%s: max|e - e_ref| / max|e_ref| = %.3g" % (what, ratio))
            assert ratio <= D.E_BAR
            _same_ring(u, u0)
            _close(n, _np_norm(u, rhs, dom, shift), "norm after mg_fmg, " + what)
            assert n < 0.5 * _np_norm(u0, rhs, dom, shift)
        # the walk on the defect of the ring alone is another correction: the interior of u0 is part of what FMG sees
        assert np.max(np.abs(D.fmg_step(mgo, ring_only, rhs, c) - e_ref)) > 100 * D.E_BAR * np.max(np.abs(e_ref))


@pytest.mark.parametrize("shape,cycle,sm,shift", [("129x65", "V", "J", 160.0), ("65", "W", "R", 0.0)])
def test_solve_with_an_fmg_start_reports_the_norm_of_the_fmg_iterate(shape, cycle, sm, shift):
    nx, ny, dom, kw, mgo, rhs, _ = _fmg_setup(shape, cycle, sm, shift)
    with _engine(nx, ny, kw, shift) as eng:
        eng.set_rhs(rhs)
        eng.set_solution(None)
        eng.fmg(1)
        u_fmg = eng.get_solution()
    with _engine(nx, ny, dict(kw, fmg_cycles=1), shift) as eng:
        u, info = eng.solve(rhs, None, tol=0.0, max_iterations=2)
    _close(info["initial_residual"], _np_norm(u_fmg, rhs, dom, shift), "initial_residual of solve(fmg_cycles=1)")
    assert info["initial_residual"] < 0.5 * _np_norm(np.zeros_like(rhs), rhs, dom, shift)
    assert info["precision_codes"] == [3, 3]
    _close(info["residual_history"][-1], _np_norm(u, rhs, dom, shift), "final norm")


# ======================================================================================================================
# 3. the stop rule
# ======================================================================================================================
def test_stop_on_tolerance_and_the_converged_flag():
    nx, ny, dom, levels = FMG_SHAPES["129x65"]
    k = 3
    rhs = D.zero_ring(O.sine_rhs(nx, ny, dom) + 0.05 * np.random.default_rng(4).standard_normal((nx, ny)))
    okw = dict(domain=dom, max_levels=levels, cycle="V", smoother="rbgs", omega=1.0)
    _, ref = O.defect_correction(O.MGOracle(nx, ny, **okw), rhs, None, tol=0.0, max_iterations=k + 2)
    h = ref["residual_history"]
    tol = float(np.sqrt(h[k - 1] * h[k]))                            # between entries k and k + 1
    assert h[k] < tol < h[k - 1] and h[k - 1] > 4 * h[k]
    # the reference loop: stops after k + 1 cycles converged, after k unconverged; runs one cycle even above the initial norm
    _, r = O.defect_correction(O.MGOracle(nx, ny, **okw), rhs, None, tol=tol, max_iterations=50)
    assert r["iterations"] == k + 1 and r["converged"]
    _, r = O.defect_correction(O.MGOracle(nx, ny, **okw), rhs, None, tol=tol, max_iterations=k)
    assert r["iterations"] == k and not r["converged"]
    _, r = O.defect_correction(O.MGOracle(nx, ny, **okw), rhs, None, tol=2 * ref["initial_residual"], max_iterations=50)
    assert r["iterations"] == 1 and r["converged"]
    kw = dict(domain=dom, max_levels=levels, cycle="V", smoother=_lib.MG_RBGS, omega=1.0, precision=_lib.MG_PREC_DEFECT)
    with mg.MultigridEngine(nx, ny, **kw) as eng:
        u, info = eng.solve(rhs, None, tol=tol, max_iterations=50)
        print("history", info["residual_history"], "reference", h, "tol", tol)
        assert info["iterations"] == k + 1 and info["converged"]
        assert len(info["residual_history"]) == k + 1 and info["precision_codes"] == [3] * (k + 1)
        np.testing.assert_allclose(info["residual_history"], h[:k + 1], rtol=1e-3)
        _close(info["residual_history"][-1], _np_norm(u, rhs, dom, 0.0), "norm at the stop")
        # the device-resident loop stops the same way
        eng.set_rhs(rhs)
        eng.set_solution(None)
        it = eng.iterate(tol, 50)
        assert it["iterations"] == k + 1 and it["converged"] and it["residual_history"] == info["residual_history"]
        assert eng.get_solution().tobytes() == u.tobytes()
        u, info = eng.solve(rhs, None, tol=tol, max_iterations=k)
        assert info["iterations"] == k and not info["converged"]
        assert len(info["residual_history"]) == k and info["precision_codes"] == [3] * k and info["residual_history"][-1] > tol
        u, info = eng.solve(rhs, None, tol=2 * ref["initial_residual"], max_iterations=50)
        assert info["iterations"] == 1 and info["converged"] and len(info["residual_history"]) == 1
        _close(info["initial_residual"], ref["initial_residual"], "initial norm")


# ======================================================================================================================
# 4. the fp64 floor under a shift
# ======================================================================================================================
def test_defect_correction_reaches_the_fp64_floor_under_a_shift():
    n, shift, steps = 129, 160.0, 14
    rhs = D.zero_ring(O.sine_rhs(n, n) + 0.05 * np.random.default_rng(9).standard_normal((n, n)))
    res = {}
    for name, code in (("double", _lib.MG_PREC_DOUBLE), ("defect", _lib.MG_PREC_DEFECT), ("single", _lib.MG_PREC_SINGLE)):
        with mg.MultigridEngine(n, n, max_levels=mg.default_max_levels(n, n), smoother=_lib.MG_RBGS, omega=1.0, precision=code) as eng:
            eng.set_shift(shift)
            res[name] = eng.solve(rhs, None, tol=0.0, max_iterations=steps)
    floor = {name: float(np.median(r[1]["residual_history"][-5:])) for name, r in res.items()}
    u64 = res["double"][0]
    print("floors", floor, "iterate", float(np.max(np.abs(res["defect"][0] - u64)) / np.max(np.abs(u64))))
    assert floor["defect"] < 3.0 * floor["double"]
    assert np.max(np.abs(res["defect"][0] - u64)) / np.max(np.abs(u64)) < 1e-9
    assert floor["single"] > 3.0 * floor["double"]                   # the case can tell the difference
    assert res["defect"][1]["precision_codes"] == [3] * steps


# ======================================================================================================================
# 5. where the grid-stride loops wrap
# ======================================================================================================================
@pytest.mark.parametrize("name", list(D.WRAP_CASES))
def test_defect_pass_above_the_block_cap(name):
    key, sm = D.WRAP_CASES[name]
    nx, ny = D.wrap_shapes()[key]
    dom = D.wrap_domain(nx, ny)
    _, code, omega = D.SMOOTHERS[sm]
    rhs, u0 = D.integer_rhs(nx, ny, 5), D.ring_start(nx, ny, 6)
    kw = dict(domain=dom, max_levels=D.levels_of(nx, ny), cycle="V", smoother=code, omega=omega, precision=_lib.MG_PREC_DEFECT)
    with mg.MultigridEngine(nx, ny, **kw) as eng:
        eng.set_rhs(rhs)
        eng.set_solution(u0)
        n0 = eng.residual_norm()
        info = eng.iterate(0.0, 1)
        u1 = eng.get_solution()
        n1 = eng.residual_norm()
        eng.set_solution(u0)
        eng.cycle(1)
        u1_cycle = eng.get_solution()
    _close(n0, _np_norm(u0, rhs, dom, 0.0), "initial norm")
    assert info["initial_residual"] == n0
    assert info["residual_history"] == [n1]                          # the updating pass and the plain one: the same bits
    _close(n1, _np_norm(u1, rhs, dom, 0.0), "norm after one step")
    inner = u1[1:-1, 1:-1]
    assert np.array_equal(inner, inner.astype(F32).astype(F64))      # 0 + (double)e: written everywhere, and once
    assert np.count_nonzero(inner) > 0.99 * inner.size
    _same_ring(u1, u0)
    assert u1_cycle.tobytes() == u1.tobytes()
    bound = 2.0 * D.wrap_yardstick(sm)
    print("%s: %d x %d, norm %.6g -> %.6g (factor %.4g, bar %.4g)" % (name, nx, ny, n0, n1, n1 / n0, bound))
    assert n1 <= bound * n0


def test_mixed_precision_residual_above_the_cap_of_grid_for():
    nx, ny = D.wrap_shapes()["residual_mixed"]
    rng = np.random.default_rng(nx + ny)
    u = rng.standard_normal((nx, ny)).astype(F32)
    f = rng.standard_normal((nx, ny)).astype(F32)
    hx, hy = O.grid_spacing(nx, ny)
    r = mg.MixedPrecisionKernels().compute_mixed_precision_residual(u, f, hx, hy)
    assert r.dtype == F64
    np.testing.assert_array_equal(r, O.residual_mixed(u, f, hx, hy))
