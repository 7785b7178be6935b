"""Stand-in for the reference's `multigrid` package, loaded by facade._load_reference through MG_REFERENCE_SRC.

The reference's CPU solver is not part of this repository, so tests of the facade's use_gpu=False path point
MG_REFERENCE_SRC here.  The stand-in has the module layout and the calls facade.py makes (core.grid.Grid,
operators.laplacian / transfer, solvers.multigrid.MultigridSolver, solvers.iterative / smoothers) and solves with
oracle.mg_oracle, which tests/test_oracle_golden.py pins to the reference's own goldens.  Every argument the facade
passes is forwarded to the oracle, so wrong plumbing shows up as a different history.  Fixed precision only."""
import types

import numpy as np

from oracle import mg_oracle as O


class Grid:
    def __init__(self, nx, ny, domain=(0.0, 1.0, 0.0, 1.0), dtype=np.float64):
        self.nx, self.ny, self.domain, self.dtype = nx, ny, tuple(domain), np.dtype(dtype)


class LaplacianOperator:
    def __init__(self, coefficient=1.0):
        self.coefficient = coefficient


class RestrictionOperator:
    def __init__(self, method="full_weighting"):
        if method != "full_weighting":
            raise NotImplementedError(f"stand-in restriction: {method}")
        self.method = method


class ProlongationOperator:
    def __init__(self, method="bilinear"):
        if method != "bilinear":
            raise NotImplementedError(f"stand-in prolongation: {method}")
        self.method = method


class EnhancedJacobiSolver:
    """NumPy-vectorised weighted Jacobi: the oracle's jacobi_form='vectorized'."""
    kind, form = "jacobi", "vectorized"

    def __init__(self, relaxation_parameter=0.8):
        self.omega = relaxation_parameter


class GaussSeidelSmoother:
    form = "loop"

    def __init__(self, relaxation_parameter=1.0, red_black=False):
        self.omega = relaxation_parameter
        self.kind = "rbgs" if red_black else "lexgs"


class PrecisionManager:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("the stand-in covers the fixed-precision strategies only")


class MultigridSolver:
    def __init__(self, max_levels=4, max_iterations=50, tolerance=1e-8, cycle_type="V", pre_smooth_iterations=2,
                 post_smooth_iterations=2, coarse_tolerance=1e-12, coarse_max_iterations=1000):
        self.max_levels, self.max_iterations, self.tolerance = max_levels, max_iterations, tolerance
        self.cycle_type, self.pre, self.post = cycle_type, pre_smooth_iterations, post_smooth_iterations
        self.coarse_tolerance, self.coarse_max_iterations = coarse_tolerance, coarse_max_iterations
        self.smoother = None

    def setup(self, grid, operator, restriction, prolongation, smoother=None):
        if smoother is None:
            raise NotImplementedError("the stand-in needs an explicit smoother")
        self.smoother = smoother

    def solve(self, grid, operator, rhs, initial_guess=None, precision_manager=None):
        if precision_manager is not None:
            raise NotImplementedError("the stand-in covers the fixed-precision strategies only")
        sm = self.smoother
        mgo = O.MGOracle(grid.nx, grid.ny, grid.domain, dtype=grid.dtype, coeff=operator.coefficient,
                         max_levels=self.max_levels, cycle=self.cycle_type, pre=self.pre, post=self.post,
                         smoother=sm.kind, omega=sm.omega, jacobi_form=sm.form, coarse_tol=self.coarse_tolerance,
                         coarse_maxit=self.coarse_max_iterations)
        return mgo.solve(np.asarray(rhs, dtype=grid.dtype), initial_guess, tol=self.tolerance,
                         max_iterations=self.max_iterations)


core = types.SimpleNamespace(grid=types.SimpleNamespace(Grid=Grid),
                             precision=types.SimpleNamespace(PrecisionManager=PrecisionManager))
operators = types.SimpleNamespace(laplacian=types.SimpleNamespace(LaplacianOperator=LaplacianOperator),
                                  transfer=types.SimpleNamespace(RestrictionOperator=RestrictionOperator,
                                                                 ProlongationOperator=ProlongationOperator))
solvers = types.SimpleNamespace(multigrid=types.SimpleNamespace(MultigridSolver=MultigridSolver),
                                iterative=types.SimpleNamespace(EnhancedJacobiSolver=EnhancedJacobiSolver),
                                smoothers=types.SimpleNamespace(GaussSeidelSmoother=GaussSeidelSmoother))
