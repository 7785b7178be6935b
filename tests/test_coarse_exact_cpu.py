"""Pins tests/coarse_exact_reference.py -- the exact coarsest solve the engine's default (coarse_direct="auto") is measured
against in tests/test_gpu_coarse_exact.py -- on the CPU: its matrix is the pinned oracle's operator, its elimination is exact to
long-double rounding, the oracle built on it agrees with the pinned iteration run to convergence, and the tier-2 cases of the
GPU module are those where the iteration (the only yardstick the suite had) stands far enough from the exact solve."""
import numpy as np
import pytest

import coarse_exact_reference as R
from oracle import mg_oracle as O

LD = np.longdouble
U_LD = float(np.finfo(LD).eps) / 2            # unit roundoff of long double: 2^-64 on x86
SMALL = [(5, 5), (9, 5), (5, 9), (7, 4), (10, 10)]


def _spacing(nx, ny):
    return 2.0 / (nx - 1), 1.0 / (ny - 1)      # a 2:1 domain: hx != hy, non-dyadic for 7 x 4 and 10 x 10


def _coef(nx, ny, kind, dtype=np.float64):
    if kind == "const":
        return None
    return np.exp(0.7 * np.random.default_rng(nx * 31 + ny).standard_normal((nx, ny))).astype(dtype)


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("kind", ["const", "var"])
@pytest.mark.parametrize("shift", [0.0, 37.5])
def test_matrix_is_a_symmetric_m_matrix(shape, kind, shift):
    nx, ny = shape
    hx, hy = _spacing(nx, ny)
    A = R.coarse_matrix(nx, ny, hx, hy, shift, _coef(nx, ny, kind))
    n = (nx - 2) * (ny - 2)
    assert A.shape == (n, n) and A.dtype == LD
    np.testing.assert_array_equal(A, A.T)
    off = A - np.diag(np.diag(A))
    assert np.all(np.diag(A) > 0) and np.all(off <= 0)
    # weakly diagonally dominant, strictly with a shift or next to the ring: rounding of the diagonal's sum allowed for
    assert np.all(np.diag(A) + off.sum(axis=1) >= LD(shift) - 8 * U_LD * np.diag(A))


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("kind,dtype", [("const", np.float64), ("var", np.float64), ("var", np.float32)])
@pytest.mark.parametrize("shift", [0.0, 37.5])
def test_matrix_is_the_pinned_oracles_operator(shape, kind, dtype, shift):
    """coarse_matrix @ x == -residual(x, 0) on the interior: the matrix is what oracle/mg_oracle.py's smoothers relax.  The
    oracle evaluates a row in its dtype with at most eight roundings, each of a quantity below |A||x|; the long-double product
    is exact by comparison."""
    nx, ny = shape
    hx, hy = _spacing(nx, ny)
    a = _coef(nx, ny, kind, dtype)
    x = np.zeros((nx, ny), dtype=dtype)
    x[1:-1, 1:-1] = np.random.default_rng(nx + 7 * ny).standard_normal((nx - 2, ny - 2)).astype(dtype)
    zero = np.zeros_like(x)
    if a is None:
        r = O.residual(x, zero, hx, hy, -1.0, shift)
    else:
        r = O.var_residual(x, zero, a, hx, hy, -1.0, shift)
    assert r.dtype == dtype
    A = R.coarse_matrix(nx, ny, hx, hy, shift, a)
    xv = x[1:-1, 1:-1].reshape(-1).astype(LD)
    got, scale = A @ xv, np.abs(A) @ np.abs(xv)
    err = np.abs(got - (-r[1:-1, 1:-1].reshape(-1).astype(LD)))
    assert np.all(err <= 8 * np.finfo(dtype).eps * scale), float(np.max(err / scale))


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("kind", ["const", "var"])
@pytest.mark.parametrize("shift", [0.0, 37.5, 1e4])
def test_exact_solve_residual_is_long_double_rounding(shape, kind, shift):
    """componentwise backward error of the elimination: |b - A x| <= 8 * 2^-64 (|A||x| + |b|).  (No pivot growth for an
    M-matrix; a row of this matrix has at most five entries, the elimination fills it to a band of ny - 2.)"""
    nx, ny = shape
    hx, hy = _spacing(nx, ny)
    A = R.coarse_matrix(nx, ny, hx, hy, shift, _coef(nx, ny, kind))
    b = np.random.default_rng(nx * ny).standard_normal(A.shape[0]).astype(LD)
    x = R.exact_solve(A, b)
    assert x.dtype == LD
    res = np.abs(b - A @ x)
    scale = np.abs(A) @ np.abs(x) + np.abs(b)
    print("max residual / (2^-64 (|A||x| + |b|)) = %.2f" % float(np.max(res / scale) / U_LD))
    assert np.all(res <= 8 * U_LD * scale)
    A0, b0 = A.copy(), b.copy()
    R.exact_solve(A, b)
    assert np.array_equal(A, A0) and np.array_equal(b, b0)           # arguments untouched


def test_exact_solve_pivots():
    A = np.array([[0.0, 2.0, 1.0], [1.0, 1.0, 0.0], [4.0, 0.0, 3.0]])
    x = np.array([1.0, -2.0, 3.0])
    np.testing.assert_allclose(np.asarray(R.exact_solve(A, A @ x), dtype=float), x, rtol=0, atol=1e-18)


@pytest.mark.parametrize("nx,ny,dom,shift", [(33, 33, R.UNIT, 0.0), (65, 33, (0.0, 2.0, 0.0, 1.0), 37.5)])
def test_exact_coarse_oracle_equals_the_iteration_run_to_convergence(nx, ny, dom, shift):
    """V(2,2) Jacobi 0.8, three cycles: the exact-coarse oracle against the pinned oracle with coarse_tol = 0 and 1000 sweeps
    (the iteration at its fixed point): 16 eps max|u|"""
    kw = dict(domain=dom, max_levels=4, cycle="V", smoother="jacobi", omega=0.8, jacobi_form="vectorized", shift=shift)
    it, ex = O.MGOracle(nx, ny, coarse_tol=0.0, coarse_maxit=1000, **kw), R.ExactCoarseOracle(nx, ny, **kw)
    f = O.sine_rhs(nx, ny, dom) + 0.05 * np.random.default_rng(nx).standard_normal((nx, ny))
    f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = 0.0
    ui, ue = np.zeros_like(f), np.zeros_like(f)
    for _ in range(3):
        it.rhs[0], ex.rhs[0] = f.copy(), f.copy()
        ui, ue = it.cycle_once(ui, 0), ex.cycle_once(ue, 0)
    rel = float(np.max(np.abs(ui - ue)) / np.max(np.abs(ue)))
    print("relative distance %.2e" % rel)
    assert rel <= 16 * np.finfo(np.float64).eps
    assert ex.coarse_sweeps == [0, 0, 0] and it.coarse_sweeps == [1000] * 3
    assert [v["n"] for v in ex.visits] == [(ex.shapes[-1][0] - 2) * (ex.shapes[-1][1] - 2)] * 3
    np.testing.assert_array_equal(ue[0, :], 0.0)


def test_exact_coarse_oracle_records_what_the_first_visit_bound_needs():
    """one V(2,2) cycle on four levels: one visit; a prolong-add and two post-sweeps on each of the three finer levels, in the
    dtype each computes in (MIXED: fp32 from level 2 down, the coarsest level in the grid's fp64)"""
    case = next(c for c in R.tier1_cases() if c["id"] == "33-smooth-mixed-VR-tail1")
    u, hist, o = R.run_oracle(case)
    e32, e64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
    assert len(o.visits) == 1 and o.visits[0]["n"] == 9 and o.visits[0]["eps"] == e64
    assert o.visits[0]["amp"] >= o.visits[0]["xmax"] > 0            # A^-1 >= 0 entrywise: A^-1 |f| >= |A^-1 f|
    assert [e for e, _ in o.stages] == [e32] * 3 + [e64] * 6
    assert all(m > 0 for _, m in o.stages) and R.tier1_bar(o) > 0
    # the recording changes nothing: the same cycle with the exact solve alone overridden (no _smooth override, post-sweeps
    # in one call)
    class Plain(O.VarMGOracle):
        def cycle_once(self, v, level=0, pm=None):
            if level != len(self.shapes) - 1:
                return super().cycle_once(v, level, pm)
            nx, ny = self.shapes[level]
            A = R.coarse_matrix(nx, ny, *self.h[level], self.shift, self.a_of(level, v.dtype))
            out = np.zeros_like(v)
            out[1:-1, 1:-1] = R.exact_solve(A, self.rhs[level][1:-1, 1:-1].reshape(-1)).astype(v.dtype).reshape(nx - 2, ny - 2)
            return out
    p = Plain(R.coefficient("33", "smooth"), domain=R.UNIT, max_levels=4, cycle="V", smoother="rbgs", omega=1.0)
    p.rhs[0] = R.case_rhs(case)
    np.testing.assert_array_equal(p.cycle_once(np.zeros((33, 33)), 0, O.OraclePrecision("mixed")).astype(np.float64), u)


def test_direct_unknown_limit_is_read_from_the_engine():
    limit = R.direct_unknown_limit()
    nx, ny = R.COARSEST["73"]
    assert (nx - 2) * (ny - 2) == limit               # the 73^2 case sits exactly on it
    nx, ny = R.COARSEST["21x69"]
    assert (nx - 2) * (ny - 2) == limit and nx != ny  # and so does a non-square one
    assert (10 - 2) * (12 - 2) > limit                # the 10 x 12 grid of the GPU module's "where direct stops" case is past it


def test_case_tables_cover_what_they_claim():
    t1 = R.tier1_cases()
    assert len({c["id"] for c in t1}) == len(t1)
    for shape in R.ALL_SHAPES:
        if shape in R.SHAPES:
            assert {c["op"] for c in t1 if c["shape"] == shape} == set(R.OPERATORS), shape
        o = R.oracle_for(next(c for c in t1 if c["shape"] == shape))[0]
        assert o.shapes[-1] == R.COARSEST[shape] and len(o.shapes) == R.ALL_SHAPES[shape][3]
    for prec in R.PRECISIONS:
        ops = {c["op"] for c in t1 if c["prec"] == prec}
        assert ops & {"smooth", "checker", "smooth+shift"} and ops & {"shift37.5", "shift1e4", "smooth+shift"}, prec
    assert {c["op"] for c in t1 if c["prec"] == "adaptive"} <= {"const", "shift37.5", "shift1e4"}
    for shape in ("33", "129"):
        assert {c["tail"] for c in t1 if c["shape"] == shape} == {1, 2}
    assert {c["smoother"] for c in t1} == {"J", "R"} and {c["cycle"] for c in t1} == {"V"}
    t2 = R.tier2_candidates()
    assert {c["cycle"] for c in t2} == {"W", "F"} and {c["smoother"] for c in t2} == {"R115"}
    assert {c["shape"] for c in t2} == set(R.SHAPES) and {c["op"] for c in t2} == set(R.OPERATORS) - {"shift1e4"}
    assert {c["prec"] for c in t2} == {"double", "mixed", "adaptive"}
    assert R.TIER2_DROPPED <= {c["id"] for c in t2}
    assert 4 * len(R.TIER2_DROPPED) <= len(t2)                       # no more than a quarter dropped
    assert len(R.tier2_cases()) == len(t2) - len(R.TIER2_DROPPED)


@pytest.mark.parametrize("case", R.tier2_candidates(), ids=lambda c: c["id"])
def test_tier2_yardstick(case):
    """D_iter = max|u_iterative_oracle - u_exact_oracle| after three cycles.  A candidate is a tier-2 case of the GPU module iff
    D_iter >= 32 floors (floor = 64 eps max|u_ref|): there max(D_iter / 16, floor) = D_iter / 16 >= 2 floors separates a direct
    solve that is as good as an exact one from one that is no better than the iteration.  The dropped ones are listed in
    coarse_exact_reference.TIER2_DROPPED; this test keeps that list honest both ways."""
    y = R.yardstick(case)
    print("%s: D_iter / floor = %.3g, D_iter / max|u| = %.3g, coarsest sweeps of the iteration %r" %
          (case["id"], y["D"] / y["floor"], y["D"] / np.max(np.abs(y["u"])), y["sweeps"][:3]))
    assert y["oracle"].coarse_sweeps == [0] * len(y["sweeps"]) and all(1 <= s < 1000 for s in y["sweeps"])
    assert y["hist"][0] > y["hist"][1] > y["hist"][2]                # a contracting cycle: deviations are not amplified
    assert (y["D"] >= 32 * y["floor"]) == (case["id"] not in R.TIER2_DROPPED)
