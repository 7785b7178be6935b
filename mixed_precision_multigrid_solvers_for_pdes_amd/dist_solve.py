"""The solve loop of the decomposed hierarchy and its precision policies: host logic over one DistributedMultigrid
(distributed.py) per working precision."""
import math


def stagnating(hist):
    """should_promote_precision on the last five residual norms (core/precision.py:189-246; csrc/mg_solve.hip: stagnating)."""
    if len(hist) < 5:
        return False
    r = hist[-5:]
    ratios = [r[i] / r[i - 1] for i in range(1, 5) if r[i - 1] > 0]
    if ratios:
        if sum(ratios) / len(ratios) > 0.9:
            return True
        rel = [abs(r[i] - r[i - 1]) / r[i - 1] for i in range(1, 5) if r[i - 1] > 0]
        if rel and sum(rel) / len(rel) < 1e-3:
            return True
    return all(r[i] >= r[i - 1] * 0.99 for i in range(1, 5))


def fp32_phase_pays(hx, hy, domain, coeff=-1.0, sigma=0.0):
    """csrc/mg_solve.hip fp32_phase_pays: the fp32 residual floor relative to ||r_0|| is at most eps32 diag(A) / lambda_min (a
    property of the grid); with a contraction of ~0.15 per cycle the fp32 phase is good for log(that) / log(0.15) cycles, and
    it is entered only when that is at least two -- its switches cost about one cycle's saving."""
    lx, ly = domain[1] - domain[0], domain[3] - domain[2]
    lam = abs(coeff) * math.pi**2 * (1.0 / (lx * lx) + 1.0 / (ly * ly)) + sigma
    ratio = 2.0**-24 * (2.0 / (hx * hx) + 2.0 / (hy * hy) + sigma) / lam
    return ratio > 0.0 and math.log(ratio) / math.log(0.15) >= 2.0


class AdaptivePolicy:
    """The engine's adaptive rule (csrc/mg_solve.hip: adapt, one-way variant of core/precision.py:270-302) as host logic
    for drivers that hold one solver per precision: start in double, drop to single on a large first residual,
    promote for good when ||r|| < 10 thr or the fp32 iteration stagnates."""

    EPS32 = 2.0 ** -24

    def __init__(self, thr, fp32_pays=True):
        """fp32_pays: the fp32 phase is good for at least two cycles on this grid (fp32_phase_pays); False: stay in double"""
        self.thr, self.phase, self.promoted, self.hist = thr, "f64", False, []
        self.fp32_pays = bool(fp32_pays)
        self.floor = 0.0          # eps32 * diag(A) * ||u||_h: the residual an fp32 iterate can reach (set_floor; 0: not evaluated)
        self.reason = None        # why the fp32 phase ended: "threshold" / "stagnation" / "fp32_floor"; "fp32_skipped": never begun

    def set_floor(self, diag, u_norm_h):
        """after the first fp32 cycle (csrc/mg_solve.hip, measure_fp32_floor): within a factor 2 of this floor another fp32 cycle
        cannot lower the residual, and the policy promotes at once instead of waiting for the stagnation window to fill"""
        self.floor = self.EPS32 * diag * u_norm_h

    def floor_due(self):
        return self.phase == "f32" and not self.promoted and self.floor == 0.0

    def before_cycle(self, rn):
        """-> the precision the coming cycle runs in (the caller moves the iterate when it differs from .phase)"""
        want = self.phase
        if not self.promoted:
            if self.phase == "f64" and rn > 100.0 * self.thr and not self.hist:
                if self.fp32_pays:
                    want = "f32"
                else:
                    self.reason = "fp32_skipped"
            elif self.phase == "f32" and (rn < 10.0 * self.thr or stagnating(self.hist) or 0.0 < self.floor and rn <= 2.0 * self.floor):
                want, self.promoted = "f64", True
                self.reason = "threshold" if rn < 10.0 * self.thr else ("stagnation" if stagnating(self.hist) else "fp32_floor")
        if want != self.phase:
            self.phase = want
            self.hist = []
        return want

    def after_cycle(self, rn):
        self.hist.append(rn)

    def switch_likely(self):
        """Will the norm of the cycle about to run change the precision?  Extrapolated from the last two norms of this
        phase, as the engine does before it queues a speculative front part (csrc/mg_solve.hip, front_would_be_wasted)."""
        if self.floor_due():
            return True                # the floor is evaluated from the iterate the coming cycle leaves and usually ends the phase
        if self.promoted or self.phase != "f32" or len(self.hist) < 2:
            return False
        prev, last = self.hist[-2], self.hist[-1]
        guess = last * (min(1.0, last / prev) if prev > 0 else 1.0)
        return guess < 10.0 * self.thr or stagnating(self.hist + [guess])


class FixedPolicy:
    """One working precision for the whole solve (the interface of AdaptivePolicy)."""

    def __init__(self, name):
        self.phase, self.promoted, self.hist, self.reason = name, True, [], None

    def before_cycle(self, rn):
        return self.phase

    def after_cycle(self, rn):
        self.hist.append(rn)

    def switch_likely(self):
        return False

    def floor_due(self):
        return False


class DecomposedSolve:
    """The loop of mg_iterate (csrc/mg_solve.hip; solvers/multigrid.py:219-246) on the decomposed hierarchy: policy check ->
    cycle -> ||r|| -> record -> absolute stop test, driving one DistributedMultigrid per working precision (they share the
    decomposition; the iterate moves between them with take_iterate_from, the on-device cast of
    PrecisionManager.convert_array).  bench.py --gpus N and DistributedMultigridSolver.solve both run THIS loop.

    solvers: {"f64": DistributedMultigrid, "f32": ...} (one entry for a fixed precision);
    policy:  "fixed" or "adaptive" (AdaptivePolicy with `switch_threshold`)."""

    def __init__(self, solvers, policy="fixed", switch_threshold=1e-6):
        self.solvers = dict(solvers)
        if policy not in ("fixed", "adaptive"):
            raise ValueError(f"Unknown precision policy: {policy}")
        if policy == "adaptive" and set(self.solvers) != {"f32", "f64"}:
            raise ValueError("the adaptive policy switches between an 'f32' and an 'f64' solver")
        self.policy_kind, self.thr = policy, switch_threshold
        self.start = "f64" if "f64" in self.solvers else next(iter(self.solvers))
        self.policy = None
        self.rn = None
        self.switches = 0

    def _new_policy(self):
        if self.policy_kind != "adaptive":
            return FixedPolicy(self.start)
        sv = self.solvers[self.start]
        return AdaptivePolicy(self.thr, fp32_phase_pays(sv.h[0][0], sv.h[0][1], sv.domain, sv.coeff))

    def set_problem(self, rhs_of_block, u0_of_block=None):
        """every precision takes the right-hand side (and the initial guess); a solve starts in `start` (double when there
        is a choice: PrecisionManager's default precision, core/precision.py:26-45).  Returns the initial residual norm."""
        for sv in self.solvers.values():
            sv.set_problem(rhs_of_block, u0_of_block)
        self.policy = self._new_policy()
        self.switches = 0
        self.rn = self.solvers[self.start].residual_norm()
        return self.rn

    @property
    def current(self):
        """the solver that holds the iterate"""
        return self.solvers[self.policy.phase]

    def step(self, tol=0.0):
        """policy check (before the cycle, solvers/multigrid.py:224-227) -> cycle -> norm; returns the new norm"""
        policy, solvers = self.policy, self.solvers
        had = policy.phase
        now = policy.before_cycle(self.rn)
        if now != had:
            solvers[now].take_iterate_from(solvers[had])
            self.switches += 1
        sv = solvers[now]
        # no speculative front part across a precision switch the policy can see coming, nor across the end of the solve
        # (it would run and be dropped): the norm in flight extrapolated from the last two, as front_would_be_wasted does
        ends = False
        if tol > 0.0 and len(policy.hist) >= 2 and policy.hist[-2] > 0:
            ends = policy.hist[-1] * min(1.0, policy.hist[-1] / policy.hist[-2]) < tol
        sv.speculate = not (policy.switch_likely() or ends)
        sv.cycle(0)
        self.rn = sv.residual_norm()
        policy.after_cycle(self.rn)
        if policy.floor_due():
            hx, hy = sv.h[0]
            policy.set_floor(2.0 / (hx * hx) + 2.0 / (hy * hy), math.sqrt(hx * hy * sv.iterate_sumsq()))
        return self.rn

    def run(self, tol, max_iterations):
        """-> (history, phase per cycle, converged): cycles until ||r|| < tol (absolute, solvers/base.py:134)"""
        hist, phases = [], []
        converged = False
        for _ in range(max_iterations):
            rn = self.step(tol)
            hist.append(rn)
            phases.append(self.policy.phase)
            if rn < tol:
                converged = True
                break
        return hist, phases, converged

    def close(self):
        for sv in self.solvers.values():
            sv.close()
