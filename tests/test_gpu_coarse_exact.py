"""The engine's DEFAULT coarsest solve (coarse_direct="auto": u = A_c^-1 f from the host's long-double inverse, applied in the
tails) against an EXACT coarse-grid reference, and every solver module under that default.

The suite runs with MG_COARSE_DIRECT=0 (tests/conftest.py): the reference's Gauss-Seidel iteration, bit for bit.  The direct
solve was only ever compared with that iteration at 1e-12 -- the iteration's own distance from an exact solve.  Here the
oracle gets an exact coarsest solve (tests/coarse_exact_reference.py, pinned by tests/test_coarse_exact_cpu.py); everything
around the coarsest solve is bit-for-bit arithmetic, so what is left between device and reference is the direct solve's own
rounding.  Engines are built with coarse_direct="auto" explicitly, never through the environment.

Part A, tier 1: ONE V-cycle from zero (Jacobi 0.8 or red-black 1.0), one visit to the coarsest grid.  The bar is derived:

  (1) The visit.  The device computes x_i = fl(sum_j Minv_ij f_j) in fp64 with Minv = fl64(A_c^-1): a dot product of n terms
      summed in a fixed order, each factor of the inverse carrying one rounding.  |x - A_c^-1 f| <= ((n + 1) u + O(u^2))
      A_c^-1 |f| componentwise with u = eps64 / 2 (A_c is an M-matrix, so A_c^-1 >= 0 and |A_c^-1| |f| = A_c^-1 |f|; the host's
      long-double elimination adds 2^-64-sized terms).  We allow (n + 2) eps64 max(A_c^-1 |f|): twice that.
  (2) Device and reference then round x to the coarsest level's dtype: the two roundings differ by at most one ulp where
      (1) moved x across a rounding boundary: eps_c max|x_ref|.
  (3) Everything after the visit is the same arithmetic on inputs that differ by delta <= (1) + (2).  Bilinear prolongation
      forms convex combinations; a weighted-Jacobi sweep with omega <= 1 and a red-black sweep with omega = 1 of a weakly
      diagonally dominant M-matrix have an iteration matrix of max-norm <= 1; the right-hand sides and pre-smoothed iterates
      are bit-identical.  So no stage expands delta in the max norm.  Each stage rounds its result once more, and results that
      differ by delta may round differently: one more ulp of the stage's result, eps_stage max|u_ref at that stage|, for the
      prolong-add and for each post-sweep on each finer level, with the eps of the dtype the level computes in.

  bar = (n + 2) eps64 max(A_c^-1 |f_c|) + eps_c max|x_ref| + sum_stages eps_stage max|u_ref at that stage|

The reference records every term (coarse_exact_reference._ExactCoarse.visits / .stages).  With an fp32 level above the coarsest
grid the last sum is of size 1e-7: such cases catch a wrong inverse (a missing shift, a wrong face mean, a wrong row), not a
1e-13 one; the fp64 cases catch both.

Part A, tier 2: W- and F-cycles, three cycles, red-black 1.15.  Deviations re-enter later visits and omega > 1 expands them, so
the bar is taken against the two references: max|u_dev - u_exact| <= max(D_iter / 16, floor) with D_iter = max|u_iter - u_exact|
between the pinned iterative oracle and the exact one and floor = 64 eps max|u_ref| in the fine level's dtype.  Which cases
qualify (D_iter >= 32 floors) and why the right-hand side is scaled there: coarse_exact_reference.py, asserted on the CPU.
The residual history gets the matching statement: |h_dev - h_exact| <= max(|h_iter - h_exact| / 16, floor_h) per cycle, where
floor_h = 2 D_max sqrt(area) floor + 1e-12 h_exact: a deviation delta of the iterate moves every entry of r = f - A u by at most
(diagonal + off-diagonal row sum) delta <= 2 D_max delta and so ||r||_h by at most sqrt(area) 2 D_max delta; 1e-12 relative is
the project's bound for sums of r^2 taken in another order (handle_call_cases.NORM_RTOL).

Part B: every solver module's smallest "equals the restatement" case with coarse_direct="auto" on the device and the
exact-coarse oracle inside the module's reference, at the bars the module's own test uses against the iterative reference.
"""
import numpy as np
import pytest

import coarse_exact_reference as R
import eig_reference as ER
import flow_reference as FR
import heat_device_reference as HR
import heat_var_reference as HV
import ho_reference as HO
import nl_reference as NL
import pcg_reference as PR
import rd_reference as RD
import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib
from oracle import mg_oracle as O

pytestmark = pytest.mark.gpu

PREC_CODES = {"double": _lib.MG_PREC_DOUBLE, "single": _lib.MG_PREC_SINGLE, "single_managed": _lib.MG_PREC_SINGLE_MANAGED,
              "mixed": _lib.MG_PREC_MIXED_LEVELS, "adaptive": _lib.MG_PREC_ADAPTIVE}
SMOOTHER_CODES = {"jacobi": _lib.MG_JACOBI, "rbgs": _lib.MG_RBGS}


def _engine(case, coarse_direct="auto", **extra):
    """the engine of a part-A case.  ADAPTIVE with a switch threshold no residual exceeds: its fp64 phase, a double solve."""
    nx, ny, dom, levels = R.ALL_SHAPES[case["shape"]]
    kind, omega = R.SMOOTHERS[case["smoother"]]
    kw = dict(domain=dom, max_levels=levels, cycle=case["cycle"], smoother=SMOOTHER_CODES[kind], omega=omega,
              precision=PREC_CODES[case["prec"]], tail=case["tail"], coarse_direct=coarse_direct)
    if case["prec"] == "adaptive":
        kw["switch_threshold"] = 1e300
    kw.update(extra)
    e = mg.MultigridEngine(nx, ny, **kw)
    a = R.coefficient(case["shape"], case["op"])
    if a is not None:
        e.set_coefficient(a)
    if R.SHIFT[case["op"]] != 0.0:
        e.set_shift(R.SHIFT[case["op"]])
    return e


def _device_cycles(case, coarse_direct="auto", **extra):
    """(iterate in fp64, residual history, sweeps of the last coarsest visit, hierarchy) of the case's cycles from zero"""
    e = _engine(case, coarse_direct, **extra)
    try:
        f = R.case_rhs(case).astype(np.float32 if case["prec"] == "single" else np.float64)
        u, info = e.solve(f, tol=0.0, max_iterations=case["ncycles"])
        assert info["iterations"] == case["ncycles"] and info["precision_switches"] == 0
        return u.astype(np.float64), info["residual_history"], info["last_coarse_sweeps"], list(e.shapes)
    finally:
        e.close()


# ======================================================================================================================
# A, tier 1: one V-cycle, the derived bar
# ======================================================================================================================
@pytest.mark.parametrize("case", R.tier1_cases(), ids=lambda c: c["id"])
def test_one_v_cycle_within_the_derived_first_visit_bound(case):
    u_ref, _, o = R.run_oracle(case)
    u, _, sweeps, shapes = _device_cycles(case)
    assert shapes == o.shapes and shapes[-1] == R.COARSEST[case["shape"]]
    assert sweeps == 0, "the direct solve did not run"
    bar = R.tier1_bar(o)
    err = float(np.max(np.abs(u - u_ref)))
    print("TIER1 %s: err/bar = %.3f (err = %.3g, bar = %.3g = %.3g max|u_ref|)" % (case["id"], err / bar, err, bar, bar / np.max(np.abs(u_ref))))
    assert np.all(np.isfinite(u)) and err <= bar


# ======================================================================================================================
# A, tier 2: W- and F-cycles, three cycles, red-black 1.15: 1/16 of the iteration's distance from the exact solve
# ======================================================================================================================
@pytest.mark.parametrize("case", R.tier2_cases(), ids=lambda c: c["id"])
def test_three_cycles_sixteen_times_closer_to_exact_than_the_iteration(case):
    y = R.yardstick(case)
    assert y["D"] >= 32 * y["floor"]                                   # the condition tests/test_coarse_exact_cpu.py asserts per candidate
    u, hist, sweeps, shapes = _device_cycles(case)
    assert shapes == y["oracle"].shapes and sweeps == 0
    err = float(np.max(np.abs(u - y["u"])))
    print("TIER2 %s: err/D_iter = %.2e, err/floor = %.3f, D_iter/floor = %.3g" % (case["id"], err / y["D"], err / y["floor"], y["D"] / y["floor"]))
    assert np.all(np.isfinite(u)) and err <= max(y["D"] / 16, y["floor"])
    o = y["oracle"]
    hx, hy = o.h[0]
    dom = R.ALL_SHAPES[case["shape"]][2]
    area = (dom[1] - dom[0]) * (dom[3] - dom[2])
    for k, (h, h_ref, h_it) in enumerate(zip(hist, y["hist"], y["hist_iter"])):
        floor_h = 2 * R.diag_max(o) * np.sqrt(area) * y["floor"] + 1e-12 * h_ref
        print("TIER2 %s cycle %d: |h - h_exact| = %.3g, |h_iter - h_exact| = %.3g, floor_h = %.3g" % (case["id"], k, abs(h - h_ref), abs(h_it - h_ref), floor_h))
        assert abs(h - h_ref) <= max(abs(h_it - h_ref) / 16, floor_h)


# ======================================================================================================================
# A: where the direct solve stops applying
# ======================================================================================================================
def _solve(nx, ny, dom, levels, coarse_direct, cyc="W", **kw):
    f = O.sine_rhs(nx, ny, dom) + 0.05 * np.random.default_rng(nx + ny).standard_normal((nx, ny))
    f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = 0.0
    e = mg.MultigridEngine(nx, ny, domain=dom, max_levels=levels, cycle=cyc, smoother=_lib.MG_RBGS, omega=1.0, coarse_direct=coarse_direct, **kw)
    try:
        u, info = e.solve(f, tol=0.0, max_iterations=2)
        return u, info, list(e.shapes)
    finally:
        e.close()


@pytest.mark.parametrize("what,nx,ny,dom,levels,kw", [
    ("10x12: 80 unknowns", 73, 89, R.UNIT, 4, {}),
    ("no tail: nine pre-sweeps are more than the LDS tail plans, and tail=2 rules the register tail out", 33, 33, R.UNIT, 4, dict(pre=9, tail=2)),
    ("no tail: tail=0", 33, 33, R.UNIT, 4, dict(tail=0)),
], ids=["10x12", "pre9-tail2", "tail0"])
def test_default_iterates_where_the_direct_solve_does_not_apply(what, nx, ny, dom, levels, kw):
    """More unknowns than want_direct takes, or a small coarsest grid outside any tail: "auto" must be the iteration, bit for bit
    what coarse_direct=False gives"""
    ua, ia, shapes = _solve(nx, ny, dom, levels, "auto", **kw)
    uf, jf, _ = _solve(nx, ny, dom, levels, False, **kw)
    n = (shapes[-1][0] - 2) * (shapes[-1][1] - 2)
    assert (n > R.direct_unknown_limit()) == what.startswith("10x12") and len(shapes) == levels
    assert ia["last_coarse_sweeps"] > 0 and ia["last_coarse_sweeps"] == jf["last_coarse_sweeps"]
    np.testing.assert_array_equal(ua, uf)
    assert ia["residual_history"] == jf["residual_history"]


def test_the_same_small_grids_are_solved_directly_inside_the_tail():
    """the control of the test above: 33^2 with the default sweeps and tail is direct, and differs from the iteration"""
    ua, ia, _ = _solve(33, 33, R.UNIT, 4, "auto")
    uf, jf, _ = _solve(33, 33, R.UNIT, 4, False)
    assert ia["last_coarse_sweeps"] == 0 and jf["last_coarse_sweeps"] > 0
    assert not np.array_equal(ua, uf)
    assert np.max(np.abs(ua - uf)) <= 1e-12 * np.max(np.abs(uf))
# A non-square coarsest grid of exactly direct_unknown_limit() unknowns that a tail takes exists: 6 x 18 below 21 x 69 under SINGLE
# (coarse_exact_reference.EXTRA_SHAPES); it is a tier-1 case above.


# ======================================================================================================================
# B. every solver module under the default, against its own restatement built on the exact-coarse oracle
# ======================================================================================================================
EXACT = (R.ExactCoarseOracle, R.ExactCoarseVarOracle)
UNIT = R.UNIT


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _jacobi():
    return mg.JacobiSmoother(relaxation_parameter=0.8)


def _differs(a, b):
    """the default really ran: at least one bit apart from the same run with coarse_direct=False"""
    return np.asarray(a).tobytes() != np.asarray(b).tobytes()


# ---- PCG: tests/test_gpu_pcg.py::test_solve_equals_restatement, its smallest constant and its smallest coefficient case
@pytest.mark.parametrize("name,kind,pre,post", [("laplace_v11_65", None, 1, 1), ("checker_v22_65", "checker", 2, 2)])
def test_pcg_under_the_default(name, kind, pre, post):
    n = 65
    a = PR.checkerboard(n, n) if kind else None
    mgo = PR.make_oracle(n, n, a, pre, post, "jacobi", 0.8, oracle_classes=EXACT)
    b = PR.random_rhs(n, n)
    hx, hy = mgo.h[0]
    tol = 1e-10 * float(np.sqrt(hx * hy * np.sum(b * b)))
    want, winfo = PR.pcg(mgo, b, tol=tol, max_iterations=60, flexible=False)
    assert set(mgo.coarse_sweeps) == {0}
    out = {}
    for direct in ("auto", False):
        s = mg.PCGSolver(max_levels=PR.full_levels(n, n), max_iterations=60, tolerance=tol, cycle_type="V", pre_smooth_iterations=pre,
                         post_smooth_iterations=post, coarse_direct=direct)
        s.setup(mg.Grid(n, n), mg.DiffusionOperator(a) if kind else mg.LaplacianOperator(coefficient=-1.0), smoother=_jacobi())
        out[direct] = s.solve(s.grid, s.operator, b)
        s.close()
    got, info = out["auto"]
    print("PARTB pcg %s: iterations %d / %d, max|x - x_ref| / max|x_ref| = %.2e, history max rel diff %.2e" % (
        name, info["iterations"], winfo["iterations"], rel(got, want),
        np.max(np.abs(np.array(info["residual_history"]) / np.array(winfo["residual_history"]) - 1))))
    assert winfo["converged"] and info["converged"] and info["status"] == "converged"
    assert info["iterations"] == winfo["iterations"]
    np.testing.assert_allclose(info["residual_history"], winfo["residual_history"], rtol=1e-10, atol=0)
    assert float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want)))
    np.testing.assert_allclose(info["initial_residual"], winfo["initial_residual"], rtol=1e-12)
    assert _differs(got, out[False][0])


# ---- fourth-order PCG: tests/test_gpu_ho.py::test_solve_of_the_manufactured_problem, 33 x 33 double
def test_fourth_order_pcg_under_the_default():
    n = 33
    u, f = HO.manufactured(n, n, 0.0)
    u0 = u.copy()
    u0[1:-1, 1:-1] = 0.0
    tol = 1e-12 * float(np.sqrt(np.sum(f * f)) / (n - 1))
    mgo = PR.make_oracle(n, n, None, 2, 2, "jacobi", 0.8, oracle_classes=EXACT)
    want, winfo = HO.pcg(mgo, f, u0=u0, tol=tol, max_iterations=60, flexible=False)
    out = {}
    for direct in ("auto", False):
        s = mg.PCGSolver(max_levels=PR.full_levels(n, n), max_iterations=60, tolerance=tol, cycle_type="V", pre_smooth_iterations=2,
                         post_smooth_iterations=2, order=4, coarse_direct=direct)
        s.setup(mg.Grid(n, n), mg.LaplacianOperator(coefficient=-1.0), smoother=_jacobi())
        out[direct] = s.solve(s.grid, s.operator, f, initial_guess=u0)
        s.close()
    got, info = out["auto"]
    print("PARTB ho: iterations %d / %d, max|x - x_ref| / max|x_ref| = %.2e" % (info["iterations"], winfo["iterations"], rel(got, want)))
    assert info["status"] == "converged" and info["order"] == 4 and winfo["converged"]
    assert info["iterations"] == winfo["iterations"]
    np.testing.assert_allclose(info["residual_history"], winfo["residual_history"], rtol=1e-10, atol=0)
    assert float(np.max(np.abs(got - want))) <= 1e-12 * float(np.max(np.abs(want)))
    np.testing.assert_allclose(info["initial_residual"], winfo["initial_residual"], rtol=1e-12)
    assert _differs(got, out[False][0])


# ---- heat: tests/test_gpu_heat_device.py / test_gpu_heat_var.py, the fixed-count step at 33 x 33
def _heat_inputs(n):
    rng = np.random.default_rng(2 * n)
    x = np.linspace(0, 1, n)
    smooth = np.sin(np.pi * x[:, None]) * np.cos(2 * np.pi * x[None, :])
    u = smooth + 0.05 * rng.standard_normal((n, n))
    up = 1.01 * smooth + 0.05 * rng.standard_normal((n, n))
    S = np.cos(np.pi * x[:, None]) * np.sin(np.pi * x[None, :]) + 0.05 * rng.standard_normal((n, n))
    return u, up, S


@pytest.mark.parametrize("inner", ["cycle", "pcg"])
def test_heat_steps_under_the_default(inner):
    """inner="cycle" with constant diffusivity, inner="pcg" with a diffusivity field; implicit Euler, Crank-Nicolson and BDF2, then
    Crank-Nicolson again with another dt: the shift changes with every scheme and dt, so the inverse is rebuilt mid-run"""
    n = 33
    u, up, S = _heat_inputs(n)
    a = PR.smooth_coefficient(n, n) if inner == "pcg" else None
    alpha, g0, g1 = 0.6, 0.8, 0.7
    edges = (0.25, -0.5, 0.75, 1.5)
    steps = [(HR.IMPLICIT, 3e-3, edges, False), (HR.CN, 3e-3, edges, True), (HR.BDF2, 3e-3, None, False), (HR.CN, 7e-3, edges, False)]
    got = {}
    for direct in ("auto", False):
        with mg.DeviceHeatStepper(n, n, UNIT, alpha, 32, "jacobi", 0.8, inner=inner, coarse_direct=direct) as st:
            st.set_slot(0, up); st.set_slot(1, u); st.set_source(S)
            if a is not None:
                st.set_coefficient(a)
            got[direct] = []
            for scheme, dt, e4, before in steps:
                info = st.step(scheme, dt, 1, 2, 0 if scheme == HR.BDF2 else None, g0, g1, e4, before, tol=0.0, max_cycles=3)
                got[direct].append((st.get_slot(2), info))
    for k, (scheme, dt, e4, before) in enumerate(steps):
        kw = dict(u_prev=up, S=S, g0=g0, g1=g1, edge4=e4, bc_before_solve=before, tol=0.0, max_cycles=3, smoother="jacobi", omega=0.8)
        if inner == "cycle":
            want, winfo = HR.step(scheme, u, dt, alpha, oracle_cls=R.ExactCoarseOracle, **kw)
        else:
            want, winfo = HV.step_var(scheme, u, dt, alpha, a, inner="pcg", oracle_cls=R.ExactCoarseVarOracle, **kw)
        x, info = got["auto"][k]
        print("PARTB heat %s step %d (%s, dt %g): rel %.2e, final residual %.6e / %.6e" % (inner, k, scheme, dt, rel(x, want),
                                                                                         info["final_residual"], winfo["final_residual"]))
        assert rel(x, want) <= 1e-12, k
        assert info["cycles"] == 3 == winfo["cycles"] and not info["converged"] and info["lambda"] == winfo["lambda"], k
        np.testing.assert_allclose(info["rhs_norm"], winfo["rhs_norm"], rtol=1e-9)
        if inner == "cycle":
            np.testing.assert_allclose(info["final_residual"], winfo["final_residual"], rtol=1e-9)
        assert _differs(x, got[False][k][0]), k


# ---- semilinear: Newton - PCG - multigrid against the restated loop (nl_reference.newton, inner="pcg"), fixed forcing
def test_semilinear_newton_under_the_default():
    """Newton changes the preconditioner's shift every iteration (sigma + mean(c)): the inverse is rebuilt each time.  Two solves on
    one solver, the second with another right-hand side.  Histories as tests/test_gpu_nl.py holds them (1e-5 above 1e-7 ||F_0||)."""
    n, kind, kappa = 33, "cubic", 3.0
    p = NL.Problem(kind, n, n, kappa, oracle_classes=EXACT)
    us = NL.manufactured(n, n)
    u0 = np.zeros((n, n))
    out = {}
    for direct in ("auto", False):
        s = mg.SemilinearSolver(nonlinearity=kind, strength=kappa, max_levels=PR.full_levels(n, n), tolerance=1e-9, forcing="fixed", eta=1e-8,
                                coarse_direct=direct)
        s.setup(mg.Grid(n, n), mg.LaplacianOperator(coefficient=-1.0), smoother=_jacobi())
        out[direct] = [s.solve(p.N(scale * us), initial_guess=u0) for scale in (1.0, 1.5)]
        s.close()
    for k, scale in enumerate((1.0, 1.5)):
        f = p.N(scale * us)
        want, winfo = NL.newton(p, f, u0, 1e-9, inner="pcg", forcing="fixed", eta=1e-8)
        got, info = out["auto"][k]
        print("PARTB newton solve %d: newton %d / %d, inner %r / %r, history %r / %r, rel %.2e" % (
            k, info["newton_iterations"], winfo["newton_iterations"], list(info["inner_iterations"]), winfo["inner_iterations"],
            info["residual_history"], winfo["residual_history"], rel(got, want)))
        assert info["status"] == "converged" and winfo["converged"]
        assert info["newton_iterations"] == winfo["newton_iterations"]
        assert list(info["inner_iterations"]) == list(winfo["inner_iterations"])
        assert list(info["step_lengths"]) == list(winfo["step_lengths"])
        np.testing.assert_allclose(info["initial_residual"], winfo["initial_residual"], rtol=1e-12)
        for g, x in zip(info["residual_history"], winfo["residual_history"]):
            if x > 1e-7 * winfo["initial_residual"]:
                assert abs(g - x) <= 1e-5 * x
        assert _differs(got, out[False][k][0]), k


# ---- reaction-diffusion: tests/test_gpu_rd.py::test_one_step_against_the_dense_newton at 17 x 17, through the solver class
@pytest.mark.parametrize("scheme", ["implicit_euler", "crank_nicolson", "bdf2"])
def test_reaction_diffusion_step_under_the_default(scheme):
    """one step of each scheme (BDF2: its Crank-Nicolson start, then the BDF2 step) with a jumping conductivity and a weight;
    the reference is the same step by the restated Newton - PCG loop on the exact-coarse hierarchy.  The bars of the existing
    test: ||u - u_ref||_h <= (sum of the two final residuals) / lambda, the same lambda, ||f|| to 1e-12, the same ring."""
    n, kind = 17, "cubic"
    alpha, kappa, rho, dt, tol = 0.3, 2.0, 1.5, 0.01, 1e-10
    rng = np.random.default_rng(n * 4)
    X, Y = NL.mesh(n, n)
    a = np.where((X - 0.5) ** 2 + (Y - 0.5) ** 2 < 0.09, 30.0, 1.0)
    w = rng.random((n, n)) * (rng.random((n, n)) > 0.3)
    S = 3.0 * np.sin(np.pi * X) * np.cos(2 * np.pi * Y)
    u0 = 0.8 * np.sin(2 * np.pi * X) * np.cos(np.pi * Y) + 0.2 * rng.standard_normal((n, n))
    edge4 = (0.3, -0.2, 0.1, 0.45)
    nsteps = 2 if scheme == "bdf2" else 1
    runs = {}
    for direct in ("auto", False):
        with mg.ReactionDiffusionSolver(mg.Grid(n, n), alpha, kind, kappa, w, rho, a, S, scheme, max_levels=3, tolerance=tol, smoother=_jacobi(),
                                        coarse_direct=direct) as s:
            s.set_state(u0)
            runs[direct] = []
            for _ in range(nsteps):
                before = s.state
                info = s.step(dt, edge4)
                runs[direct].append((before, s.state, info))
    levels = [u0]
    for k in range(nsteps):
        before, got, info = runs["auto"][k]
        sch = RD.CN if (scheme == "bdf2" and k == 0) else {"implicit_euler": RD.IMPLICIT, "crank_nicolson": RD.CN, "bdf2": RD.BDF2}[scheme]
        want, ri = RD.step(sch, kind, before, dt, alpha, kappa, rho, u_prev=levels[-2] if sch == RD.BDF2 else None, S=S, a=a, w=w,
                           edge4=edge4, tol=tol, max_newton=30, inner="pcg", oracle_classes=EXACT)
        levels.append(got)
        lam = RD.lam(sch, dt, alpha)
        err = float(np.sqrt(np.sum((got - want)[1:-1, 1:-1] ** 2)) / (n - 1))
        bound = (info["final_residual"] + ri["final_residual"]) / lam
        print("PARTB rd %s step %d: newton %d / %d, inner %r / %r, error %.3e, bound %.3e" % (
            scheme, k, info["newton_iterations"], ri["newton_iterations"], info["inner_iterations"], ri["inner_iterations"], err, bound))
        assert info["converged"] and info["status"] == "converged" and ri["converged"] and info["scheme"] == sch
        assert info["lambda"] == lam and info["rhs_norm"] == pytest.approx(ri["rhs_norm"], rel=1e-12)
        assert info["final_residual"] < tol * max(1.0, info["rhs_norm"])
        for sl in ((0, slice(None)), (-1, slice(None)), (slice(None), 0), (slice(None), -1)):
            assert got[sl].tobytes() == want[sl].tobytes()
        assert err <= bound
        assert info["newton_iterations"] == ri["newton_iterations"] and info["inner_iterations"] == sum(ri["inner_iterations"])
        assert _differs(got, runs[False][k][1]), k


# ---- flow: tests/test_gpu_flow.py::test_steps_equal_restatement_with_a_fixed_cycle_count at 33 x 33, two steps
def test_flow_steps_under_the_default():
    """every step solves a shifted problem (vorticity) and an unshifted one (stream function) on ONE engine: the inverse is
    rebuilt twice per step"""
    n = 33
    speeds = (0.75, -1.25, 0.5, 1.5)
    rng = np.random.default_rng(2 * n)
    x = np.linspace(0, 1, n)
    w0 = 5.0 * np.sin(np.pi * x[:, None]) * np.sin(2 * np.pi * x[None, :]) + 0.05 * rng.standard_normal((n, n))
    F = np.cos(np.pi * x[:, None]) * np.sin(np.pi * x[None, :]) + 0.05 * rng.standard_normal((n, n))
    dt = 0.5 / (n - 1)
    ref = FR.Flow(n, n, 0.02, FR.NO_SLIP, speeds, force=F,
                  solver=FR.CycleSolver(n, n, tol=0.0, max_cycles=3, smoother="jacobi", omega=0.8, oracle_cls=R.ExactCoarseOracle))
    ref.set_state(w0)
    want = [(ref.psi.copy(), ref.w.copy(), None)]
    for step in (dt, dt / 2):
        winfo = ref.step(step)
        want.append((ref.psi.copy(), ref.w.copy(), winfo))
    runs = {}
    for direct in ("auto", False):
        with mg.VorticityStreamSolver(mg.Grid(n, n), 0.02, "no_slip", dict(zip(("left", "right", "bottom", "top"), speeds)), forcing=F,
                                      tolerance=0.0, max_cycles=3, smoother="jacobi", omega=0.8, max_levels=32, coarse_direct=direct) as s:
            s.set_vorticity(w0)
            runs[direct] = [(s.stream_function, s.vorticity, None)]
            for step in (dt, dt / 2):
                info = s.step(step)
                runs[direct].append((s.stream_function, s.vorticity, info))
    for k, ((psi, w, info), (wpsi, ww, winfo)) in enumerate(zip(runs["auto"], want)):
        print("PARTB flow state %d: rel psi %.2e, rel w %.2e" % (k, rel(psi, wpsi), rel(w, ww)))
        assert rel(psi, wpsi) <= 1e-12 and rel(w, ww) <= 1e-12, k
        if info is not None:
            assert info["cycles"] == 3 and info["psi_cycles"] == 3 and not info["converged"], k
            assert info["sigma"] == winfo["sigma"] and info["c0"] == winfo["c0"] and info["c1"] == winfo["c1"], k
            np.testing.assert_allclose(info["rhs_norm"], winfo["rhs_norm"], rtol=1e-9)
            np.testing.assert_allclose(info["final_residual"], winfo["omega"]["final_residual"], rtol=1e-9)
            np.testing.assert_allclose(info["psi_final_residual"], winfo["psi"]["final_residual"], rtol=1e-9)
            np.testing.assert_allclose(info["omega_change"], winfo["omega_change"], rtol=1e-9)
        assert _differs(psi, runs[False][k][0]), k


# ---- eigensolver: tests/test_gpu_eig.py::test_solver_equals_restatement, case "B" and the jumping coefficient "D"
HIST_RTOL = {"B": 1e-3, "D": 2.5e-3}            # tests/test_gpu_eig.py: HIST_RTOL, HIST_TAIL, HIST_TAIL_RTOL, HIST_ATOL
HIST_TAIL, HIST_TAIL_RTOL, HIST_ATOL = 4, {"B": 2.5e-2}, 1e-11


@pytest.mark.parametrize("name", ["B", "D"])
def test_eigensolver_under_the_default(name):
    c = ER.CASES[name]
    wlam, _, winfo = ER.run_case(name, oracle_classes=EXACT)
    out = {}
    for direct in ("auto", False):
        s = mg.EigenSolver(num_eigenpairs=c["k"], block_size=c["m"], max_levels=PR.full_levels(c["nx"], c["ny"]), tolerance=ER.TOL, cycle_type="V",
                           pre_smooth_iterations=c["pre"], post_smooth_iterations=c["post"], precision=c["precision"], coarse_direct=direct)
        a = ER.jump_coefficient(c["nx"], c["ny"]) if c["a"] == "jump" else None
        s.setup(mg.Grid(c["nx"], c["ny"], c["domain"]), mg.DiffusionOperator(a) if a is not None else mg.LaplacianOperator(coefficient=-1.0),
                smoother=_jacobi())
        out[direct] = s.solve()
        s.close()
    lam, vecs, info = out["auto"]
    exact = ER.case_exact(name)
    err = float(np.max(np.abs(lam - exact) / exact))
    h, wh = np.array(info["residual_history"]), np.array(winfo["residual_history"])
    m = min(len(h), len(wh))
    print("PARTB eig %s: iterations %d / %d, eigenvalue error %.2e, history max rel diff %.2e" % (
        name, info["iterations"], winfo["iterations"], err, np.max(np.abs(h[:m] - wh[:m]) / wh[:m])))
    assert info["converged"] and info["status"] == "converged"
    assert abs(info["iterations"] - ER.PINNED_ITERATIONS[name]) <= 1 and abs(winfo["iterations"] - ER.PINNED_ITERATIONS[name]) <= 1
    assert err <= 1e-10 and np.all(info["residuals"] < ER.TOL)
    head = m - HIST_TAIL if name in HIST_TAIL_RTOL else m
    np.testing.assert_allclose(h[:head], wh[:head], rtol=HIST_RTOL[name], atol=HIST_ATOL)
    if head < m:
        np.testing.assert_allclose(h[head:m], wh[head:m], rtol=HIST_TAIL_RTOL[name], atol=HIST_ATOL)
    assert _differs(vecs, out[False][1])
