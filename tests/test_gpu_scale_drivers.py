"""The solver modules' drivers (PCGSolver, SemilinearSolver, DeviceHeatStepper, ReactionDiffusionSolver, EigenSolver,
VorticityStreamSolver) at 1281 x 1281 on the unit square -- handle_call_cases.SHAPES["1281"], the smallest grid on which the
inner engine runs 16-row tiles, register-blocked legs, the spanning leg and the third buffer, and on which the solvers' own
partial buffers leave their floor.  default_max_levels, Jacobi 0.8, V(2,2); fp64 and, where the driver has it, an fp32
preconditioner ("single_managed").

No NumPy restatement of a whole solve runs at this size.  The measure is a closed form of the discrete operator
(tests/scale_edge_cases.py, checked against the restatements at 33 x 33 by tests/test_scale_edges_cpu.py) or an O(N) NumPy
evaluation of the returned field, never a second run of the code under test.  No bound is a number fixed in advance: each is
derived in the test from quantities it computes, every test prints measured / bound, and the ratios measured on an MI355X
stand next to each derivation.

Two rules serve every test:
  * a device norm against the NumPy norm of the same field: c eps (4/hx^2 + 4/hy^2 + shift) max(a) ||u||_h, with c the
    roundings of one stencil evaluation plus the depth of the reduction chain (scale_edge_cases.STENCIL_OPS, REDUCE_DEPTH);
  * an error against a residual: ||u - u*|| <= ||N(u) - N(u*)|| / lambda_min for a strongly monotone N (the linear operators
    included), lambda_min the closed-form smallest eigenvalue (times min(a) with a coefficient).
The issue sketched the steppers' bound as steps x tolerance x ||u0||; the drivers' tolerance is on the residual, relative to
max(1, ||f||_h), not on the error relative to ||u||, so the bound here converts it through 1 / (shift + lambda_min) with
||f|| from the closed form (scale_edge_cases.stepper_bound) -- the only place where the derivation departs from the sketch."""
import numpy as np
import pytest

import mixed_precision_multigrid_solvers_for_pdes_amd as mg
from mixed_precision_multigrid_solvers_for_pdes_amd.facade import default_max_levels
from mixed_precision_multigrid_solvers_for_pdes_amd.heat_device import DeviceHeatStepper

import eig_reference as ER
import flow_reference as FR
import handle_call_cases as HC
import heat_device_reference as HD
import nl_reference as NL
import rd_reference as RD
import scale_edge_cases as S

pytestmark = pytest.mark.gpu

NX, NY, DOMAIN, _ = HC.SHAPES["1281"]
LEVELS = default_max_levels(NX, NY)
HXY = (1.0 / (NX - 1), 1.0 / (NY - 1))
N_CELLS = (NX - 2) * (NY - 2)
PRECISIONS = ["double", "single_managed"]
LAM_MIN = S.lam_min(NX, NY)
SMOOTH, HIGH = (2, 3), (NX - 3, NY - 4)          # a smooth mode and one near the grid's highest frequency
MODES = {"smooth": SMOOTH, "high": HIGH}
STEPS = S.DRIVER_STEPS
STEP_TOL = 1e-10
LIPSCHITZ = 4.0 * (NX - 1) ** 2 + 4.0 * (NY - 1) ** 2          # + twice the shift below: bounds every right-hand side's map


def nh(v):
    return S.norm_h(v, NX, NY)


def _jacobi():
    return mg.JacobiSmoother(relaxation_parameter=0.8)


def _report(what, measured, bound):
    print("%s: measured %.3e bound %.3e ratio %.3g" % (what, measured, bound, measured / bound))
    assert measured <= bound, what


_PROBLEMS = {}


def _problem(kind):
    if kind not in _PROBLEMS:
        _PROBLEMS[kind] = S.pcg_problem(NX, NY, kind)
    return _PROBLEMS[kind]


# ------------------------------------------------------------------------------------------ PCGSolver
# measured / bound on an MI355X (double, single_managed; 6, 27 and 6 iterations):
#   const  true_residual 1.0e-12 0        error 3.3e-4 3.3e-4
#   var    true_residual 1.7e-13 1.7e-13  error 5.1e-5 5.1e-5
#   ho     true_residual 0       8.9e-13  error 7.5e-4 2.3e-4
# (the two norms are sums of 1.6 M squares of like size: they agree to an ulp or two, far inside the cell-by-cell floor)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["const", "var", "ho"])
def test_pcg_solver(kind, precision):
    """u* = low and high sine modes + noise, f = A_h u* in NumPy (order 4: R f = A4 u* mode by mode); the solve stops at
    1e-9 ||f||_h.  info["true_residual"] is the NumPy residual norm of the returned u within the norm rule, and
    ||u - u*||_h <= (||r||_h + 2 floors) / (min(a) lambda_min): r is evaluated in NumPy and f was formed in NumPy, each within
    one floor of its exact value."""
    us, f, a, tol, _ = _problem(kind)
    s = mg.PCGSolver(max_levels=LEVELS, max_iterations=100, tolerance=tol, cycle_type="V", pre_smooth_iterations=2,
                     post_smooth_iterations=2, precision=precision, order=4 if kind == "ho" else 2)
    op = mg.DiffusionOperator(a) if a is not None else mg.LaplacianOperator(coefficient=-1.0)
    s.setup(mg.Grid(NX, NY), op, smoother=_jacobi())
    u, info = s.solve(s.grid, s.operator, f)
    s.close()
    print(kind, precision, "iterations", info["iterations"], "true", info["true_residual"], "tol", tol)
    assert info["status"] == "converged" and info["converged"]
    rnorm = nh(S.np_residual(kind, u, f, a))
    amax, amin = (1.0, 1.0) if a is None else (float(a.max()), float(a.min()))
    floor = S.rounding_floor(NX, NY, kind, 0.0, amax, nh(u))
    _report("%s %s true_residual against NumPy" % (kind, precision), abs(info["true_residual"] - rnorm), floor)
    assert rnorm < tol + floor
    lmin = amin * S.lam_min(NX, NY, 4 if kind == "ho" else 2)
    _report("%s %s error against the residual" % (kind, precision), nh(u - us), (rnorm + 2 * floor) / lmin)


# ------------------------------------------------------------------------------------------ SemilinearSolver
KAPPA = 64.0


def _weight():
    i, j = np.ogrid[:NX, :NY]
    return 0.5 + ((i // 160 + j // 160) % 2).astype(np.float64) + np.zeros((NX, NY))          # 0.5 / 1.5 in blocks


# measured / bound on an MI355X (double, single_managed): linear (3 Newton steps) true_residual 0 1.1e-14, error 8.6e-4 8.6e-4;
# cubic (7 Newton steps) true_residual 8.7e-14 8.7e-14, error 5.5e-2 5.5e-2
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("nonlinearity", ["linear", "cubic"])
def test_semilinear_solver(nonlinearity, precision):
    """N(u) = A u + kappa w phi(u) with f := N(u*) in NumPy.  N is strongly monotone with constant lambda_min (w >= 0,
    phi' >= 0), so ||u - u*||_h <= (||F(u)||_h + 2 floors) / lambda_min with F evaluated in NumPy; info["true_residual"] is that
    ||F(u)||_h within the norm rule (shift: the largest kappa w phi'(u))."""
    us, _, _, _, _ = _problem("const")
    w = _weight()
    kind = NL.KINDS[nonlinearity]
    f = -NL.evaluate(kind, us, np.zeros_like(us), HXY[0], HXY[1], -1.0, 0.0, KAPPA, None, w)["F"]
    tol = S.PCG_REL_TOL * nh(f)
    s = mg.SemilinearSolver(nonlinearity=nonlinearity, strength=KAPPA, weight=w, max_levels=LEVELS, tolerance=tol, precision=precision,
                            cycle_type="V", pre_smooth_iterations=2, post_smooth_iterations=2)
    s.setup(mg.Grid(NX, NY), mg.LaplacianOperator(coefficient=-1.0), smoother=_jacobi())
    u, info = s.solve(f)
    s.close()
    print(nonlinearity, precision, "newton", info["newton_iterations"], "inner", info["total_inner_iterations"], "true", info["true_residual"])
    assert info["status"] == "converged" and info["converged"]
    e = NL.evaluate(kind, u, f, HXY[0], HXY[1], -1.0, 0.0, KAPPA, None, w)
    fnorm = nh(e["F"])
    floor = S.rounding_floor(NX, NY, "const", float(np.max(e["c"])), 1.0, nh(u))
    _report("%s %s true_residual against NumPy" % (nonlinearity, precision), abs(info["true_residual"] - fnorm), floor)
    assert fnorm < tol + floor
    _report("%s %s error against F(u)" % (nonlinearity, precision), nh(u - us), (fnorm + 2 * floor) / LAM_MIN)


# ------------------------------------------------------------------------------------------ DeviceHeatStepper
HEAT_DT, HEAT_ALPHA = 0.01, 1.0


def _stepper_bound(scheme, lam, factors, shift_of, dmin_extra=0.0, rho=0.0):
    """scale_edge_cases.stepper_bound for STEPS steps on a mode of eigenvalue `lam`: ||f_k|| = (lam + shift + dmin_extra) |c_{k+1}|
    ||u0||_h, since f_k is the implicit operator applied to the exact new level"""
    u0n = 0.5                                                   # ||sin sin||_h on the unit square
    shifts = [shift_of(S.heat_scheme_of_step(scheme, k)) for k in range(STEPS)]
    fn = [(lam + shifts[k] + dmin_extra) * abs(factors[k + 1]) * u0n for k in range(STEPS)]
    un = [max(abs(factors[k]), abs(factors[k + 1])) * u0n for k in range(STEPS)]
    carries = [S.carry_of(scheme, k, HEAT_DT, rho, HEAT_ALPHA * LAM_MIN + dmin_extra * HEAT_ALPHA) for k in range(STEPS)]
    return S.stepper_bound(STEP_TOL, shifts, LAM_MIN, fn, un, LIPSCHITZ + 2 * max(shifts) + 4 * abs(rho), carries, NX, NY)


# measured / bound on an MI355X, inner cycle / pcg+single_managed:
#   implicit_euler  smooth 7.2e-4 2.0e-6   high 6.0e-9  4.4e-6
#   crank_nicolson  smooth 6.2e-4 1.7e-5   high 7.5e-6  2.6e-4
#   bdf2            smooth 1.9e-4 1.6e-6   high 1.7e-10 4.5e-5
@pytest.mark.parametrize("inner,precision", [("cycle", "double"), ("pcg", "single_managed")])
@pytest.mark.parametrize("which", ["smooth", "high"])
@pytest.mark.parametrize("scheme", [HD.IMPLICIT, HD.CN, HD.BDF2])
def test_heat_stepper(scheme, which, inner, precision):
    """u0 one sine mode: STEPS steps give c_STEPS u0 with the scheme's amplification factor at lambda_kl (BDF2: its two-term
    recursion after a Crank-Nicolson start).  Bound: scale_edge_cases.stepper_bound, plus twice the distance of the computed
    u0 from the exact eigenvector (scale_edge_cases.mode_defect): that part decays by other factors, none above 1."""
    k, l = MODES[which]
    lam = float(S.lam_kl(NX, NY, k, l))
    u0 = S.mode(NX, NY, k, l)
    c = S.heat_factors(scheme, HEAT_DT, HEAT_ALPHA, lam, STEPS)
    st = DeviceHeatStepper(NX, NY, DOMAIN, alpha=HEAT_ALPHA, max_levels=LEVELS, omega=0.8, inner=inner, precision=precision)
    st.set_slot(0, u0)
    for n in range(STEPS):
        sch = S.heat_scheme_of_step(scheme, n)
        info = st.step(sch, HEAT_DT, n % 4, (n + 1) % 4, prev=(n - 1) % 4 if sch == HD.BDF2 else None, tol=STEP_TOL, max_cycles=40)
        assert info["converged"], (n, info)
    got = st.get_slot(STEPS % 4)
    st.close()
    bound = _stepper_bound(scheme, lam, c, lambda sch: HD.lam(sch, HEAT_DT, HEAT_ALPHA)) + 2 * S.mode_defect(k, l)
    _report("%s %s %s/%s c = %.6e" % (scheme, which, inner, precision, c[-1]), nh(got - c[-1] * u0), bound)
    assert not got[0].any() and not got[-1].any() and not got[:, 0].any() and not got[:, -1].any()


# ------------------------------------------------------------------------------------------ ReactionDiffusionSolver
RD_KAPPA, RD_RHO = 20.0, 5.0


# measured / bound on an MI355X (double, single_managed): implicit_euler smooth 5.1e-7 9.5e-7, high 4.7e-8 1.7e-6;
# crank_nicolson smooth 3.3e-6 3.4e-6, high 7.9e-2 4.0e-6; bdf2 smooth 1.7e-6 1.7e-6, high 1.7e-2 2.3e-6
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", ["smooth", "high"])
@pytest.mark.parametrize("scheme", [RD.IMPLICIT, RD.CN, RD.BDF2])
def test_reaction_diffusion_solver(scheme, which, precision):
    """u_t = alpha lap u - kappa u + rho u on one sine mode, kappa implicit and rho explicit as the module's docstring states:
    the factors are rd_reference.eigen_factor's, step by step.  The implicit operator is -Lap + lambda + kappa / alpha."""
    k, l = MODES[which]
    lam = float(S.lam_kl(NX, NY, k, l))
    u0 = S.mode(NX, NY, k, l)
    c = S.rd_factors(scheme, HEAT_DT, HEAT_ALPHA, lam, RD_KAPPA, RD_RHO, STEPS)
    s = mg.ReactionDiffusionSolver(mg.Grid(NX, NY), HEAT_ALPHA, nonlinearity="linear", strength=RD_KAPPA, linear_growth=RD_RHO,
                                   scheme=scheme, max_levels=LEVELS, tolerance=STEP_TOL, precision=precision, smoother=_jacobi())
    s.set_state(u0)
    for n in range(STEPS):
        info = s.step(HEAT_DT)
        assert info["converged"] and info["scheme"] == S.heat_scheme_of_step(scheme, n), (n, info)
    got = s.state
    s.close()
    bound = _stepper_bound(scheme, lam, c, lambda sch: RD.lam(sch, HEAT_DT, HEAT_ALPHA), dmin_extra=RD_KAPPA / HEAT_ALPHA, rho=RD_RHO)
    bound += 2 * S.mode_defect(k, l)
    _report("%s %s %s c = %.6e" % (scheme, which, precision, c[-1]), nh(got - c[-1] * u0), bound)


# ------------------------------------------------------------------------------------------ EigenSolver
# measured / bound on an MI355X (double, single_managed; 18 iterations): eigenvalues 7.1e-6 8.9e-6, info residuals 3.5e-2 3.5e-2,
# Gram 3.7e-6 5.2e-6
@pytest.mark.parametrize("precision", PRECISIONS)
def test_eigen_solver(precision):
    """six pairs from a block of eight.  For a symmetric matrix an eigenvalue lies within ||A x - lambda x|| / ||x|| of lambda;
    the exact ones are the six smallest lambda_kl in order, and r is evaluated in NumPy (one rounding floor).  The modes are
    orthonormal in Grid.l2_norm's inner product within 2 N eps (the bound of the small-shape Gram test, N eps sum |u||v|, for
    the device's product and for NumPy's), and info["residuals"] = ||r_i|| / (lambda_i ||x_i||) within the norm rule."""
    s = mg.EigenSolver(num_eigenpairs=6, block_size=8, max_levels=LEVELS, tolerance=1e-8, cycle_type="V", pre_smooth_iterations=2,
                       post_smooth_iterations=2, precision=precision)
    s.setup(mg.Grid(NX, NY), mg.LaplacianOperator(coefficient=-1.0), smoother=_jacobi())
    lam, vecs, info = s.solve()
    s.close()
    print(precision, "iterations", info["iterations"], "restarts", info["restarts"], "residuals", info["residuals"])
    assert info["converged"] and info["status"] == "converged"
    exact = ER.exact_dirichlet(NX, NY, DOMAIN, 6)[0]
    worst = {"eigenvalues": 0.0, "residuals": 0.0}
    for i in range(6):
        x = vecs[i]
        assert not x[0].any() and not x[-1].any() and not x[:, 0].any() and not x[:, -1].any()
        r = NL.apply_A(x, HXY[0], HXY[1], -1.0, 0.0) - lam[i] * x
        r[0] = r[-1] = 0.0
        r[:, 0] = r[:, -1] = 0.0
        floor = S.rounding_floor(NX, NY, "const", 0.0, 1.0, nh(x))
        rel = nh(r) / nh(x)
        worst["eigenvalues"] = max(worst["eigenvalues"], abs(lam[i] - exact[i]) / (rel + floor / nh(x) + S.EPS * exact[i]))
        worst["residuals"] = max(worst["residuals"], abs(info["residuals"][i] - rel / lam[i]) / (floor / (nh(x) * lam[i])))
    _report("%s eigenvalues against the residual bound (worst ratio)" % precision, worst["eigenvalues"], 1.0)
    _report("%s info residuals against NumPy (worst ratio)" % precision, worst["residuals"], 1.0)
    flat = vecs.reshape(6, -1)
    gram = HXY[0] * HXY[1] * (flat @ flat.T)
    _report("%s Gram matrix of the modes" % precision, float(np.max(np.abs(gram - np.eye(6)))), 2 * N_CELLS * S.EPS)


# ------------------------------------------------------------------------------------------ VorticityStreamSolver
FLOW_NU, FLOW_DT = 0.05, 0.01


# measured / bound on an MI355X: smooth vorticity 1.1e-2, stream function 1.7e-3; high vorticity 1.3e-4, stream function 7.0e-10
# (on the high mode the bound is the measured Jacobian's: psi = w / lambda holds to the solve tolerance, lambda is 6.5e6)
@pytest.mark.parametrize("which", ["smooth", "high"])
def test_vorticity_stream_solver(which):
    """free slip, no forcing, w0 = lambda_kl psi0 for one sine mode psi0.  Arakawa's J(psi, c psi) is zero by antisymmetry, so
    the Adams-Bashforth term vanishes on the first step (c0 = 1, c1 = 0: tests/flow_reference.py ab2) as on the later ones, and
    every step multiplies w by the Crank-Nicolson factor (1 - nu dt lambda / 2) / (1 + nu dt lambda / 2); psi = w / lambda.
    On the device psi is w / lambda only to the solve tolerance, so J is not exactly 0: its h-norm is evaluated in NumPy from
    the fields of every step and enters the bound as a perturbation (2 / nu) (|c0| ||J_k|| + |c1| ||J_{k-1}||) of f."""
    k, l = MODES[which]
    lam = float(S.lam_kl(NX, NY, k, l))
    psi0 = S.mode(NX, NY, k, l)
    w0 = lam * psi0
    g = S.flow_factor(FLOW_NU, FLOW_DT, lam)
    sigma = 2.0 / (FLOW_NU * FLOW_DT)
    s = mg.VorticityStreamSolver(mg.Grid(NX, NY), FLOW_NU, wall="free_slip", max_levels=LEVELS, tolerance=STEP_TOL, max_cycles=50,
                                 smoother="jacobi", omega=0.8)
    s.set_vorticity(w0)
    jn, extra = [], []
    for n in range(STEPS):
        jn.append(nh(FR.jacobian(s.stream_function, s.vorticity, HXY[0], HXY[1])))
        c0, c1 = FR.ab2(FLOW_DT, FLOW_DT if n else None)
        extra.append((2.0 / FLOW_NU) * (abs(c0) * jn[-1] + (abs(c1) * jn[-2] if n else 0.0)))
        info = s.step(FLOW_DT)
        assert info["converged"] and (info["c0"], info["c1"]) == (c0, c1), (n, info)
    w, psi = s.vorticity, s.stream_function
    s.close()
    wn = nh(w0)
    fn = [(sigma + lam) * abs(g) ** (n + 1) * wn + extra[n] for n in range(STEPS)]
    un = [abs(g) ** n * wn for n in range(STEPS)]
    ew = S.stepper_bound(STEP_TOL, [sigma] * STEPS, LAM_MIN, fn, un, LIPSCHITZ + 2 * sigma, [(1.0, 0.0)] * STEPS, NX, NY, extra)
    print(which, "||J||_h per step", jn, "factor", g)
    ew += 2 * lam * S.mode_defect(k, l)
    _report("%s vorticity" % which, nh(w - g ** STEPS * w0), ew)
    # -lap psi = w_new to the tolerance: psi - g^STEPS psi0 = Lap^-1 (error of w) + the solve's own error
    floor = S.rounding_floor(NX, NY, "const", 0.0, 1.0, nh(psi))
    _report("%s stream function" % which, nh(psi - g ** STEPS * psi0), (ew + STEP_TOL * max(1.0, nh(w)) + floor) / LAM_MIN)
