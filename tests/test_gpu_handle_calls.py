"""The handle-bound entry points of include/mghip.h and the state an mg_handle keeps between calls, transition by named
transition (tests/handle_call_cases.py): the device-resident forms (mg_set_rhs_device, mg_update_rhs_device,
mg_zero_solution_device, mg_get_solution_device), mg_set_stream / mg_get_stream, operator changes, mg_time_op and the small
error contracts.

The reference of every comparison is a FRESH handle, created for it, given the same right-hand side and iterate through the
host forms (which the rest of the suite anchors to the oracle and the golden vectors) and destroyed afterwards; one case per
precision policy is anchored to the oracle directly.  Every right-hand side and initial guess carries a random non-zero
boundary ring.  Iterates compare bit for bit; residual norms exactly, or within handle_call_cases.NORM_RTOL where the case
table says so (its docstring has the rule).  Caller-side device arrays sit between guard rows of NaN sentinels, which every
call must leave alone."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dev_call_cases as G  # noqa: E402
import handle_call_cases as H  # noqa: E402

import mixed_precision_multigrid_solvers_for_pdes_amd as mg  # noqa: E402
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib  # noqa: E402
from oracle import mg_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _dev():
    import torch
    torch.cuda.set_device(0)
    return torch, torch.device("cuda", 0)


def _engine(shape, smoother, policy, **extra):
    nx, ny, kw = H.engine_kwargs(shape, smoother, policy, **extra)
    return mg.MultigridEngine(nx, ny, **kw)


def _working(eng, policy):
    """the working precision an adaptive case runs in (mg_set_working_precision)"""
    if H.POLICIES[policy][2] == "f32":
        eng.set_working_precision(F32)


def _rounds_in_f32(policy):
    """the fine right-hand side of these policies lives in fp32 only: an fp64 array must arrive rounded once"""
    return policy in ("single", "single_managed")


def _ids(cases):
    return pytest.mark.parametrize("case", cases, ids=lambda c: c["id"])


def _assert_norm(got, ref, spec, what):
    print("%s: %.17g against %.17g (%s)" % (what, got, ref, "within %g" % H.NORM_RTOL if spec["loose"] else "exact"))
    assert H.norms_agree(got, ref, spec["loose"]), (what, got, ref, spec)


def _assert_hist(got, ref, spec, what):
    assert len(got) == len(ref), (what, got, ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        _assert_norm(a, b, spec, "%s, cycle %d" % (what, k + 1))


# ======================================================================================================================
# A. device forms equal host forms
# ======================================================================================================================
@_ids(H.cases_a())
def test_device_forms_equal_host_forms(case):
    """X: mg_set_rhs_device, mg_zero_solution_device, mg_cycle(2), mg_get_solution_device on caller arrays of either dtype and three
    pitches; Y: mg_set_rhs, mg_set_solution(NULL), mg_cycle(2), mg_get_solution.  The same bits, an array of the other precision
    rounded once exactly as NumPy's astype does.  Above 1100^2 cells mg_iterate(0, 3) takes the place of the cycles: X (ring sum
    unknown) runs the plain loop, Y the speculative one with the spanning leg."""
    torch, dev = _dev()
    policy, shape, smoother = case["policy"], case["shape"], case["smoother"]
    nx, ny = H.SHAPES[shape][:2]
    (rhs,), u0 = H.fields(shape, 11)

    def run(eng):
        if case["large"]:
            return eng.iterate(0.0, 3)["residual_history"]
        eng.cycle(2)
        return None

    for dt in case["dtypes"]:
        npdt = G.NPDT[dt]
        rhs_c = rhs.astype(npdt)                                   # what the caller's array holds
        Y = _engine(shape, smoother, policy)
        Y.set_rhs(rhs_c.astype(F32) if _rounds_in_f32(policy) else rhs_c)
        Y.set_solution(None)
        _working(Y, policy)
        n0_host = Y.residual_norm()
        hist_y = run(Y)
        u_y = Y.get_solution(F64).astype(npdt)                     # an fp32 array of an fp64 iterate: rounded once, by NumPy
        Y.close()

        if not case["large"]:
            # mg_zero_solution_device after an iterate with a non-zero ring: all zero, ring included, and the norm of a fresh
            # handle that was given the zero guess
            Z = _engine(shape, smoother, policy)
            a_rhs = H.dev_array(dev, dt, nx, ny, "lib", rhs)
            torch.cuda.synchronize()
            Z.set_solution(u0)
            Z.set_rhs_device(a_rhs.view)
            _working(Z, policy)
            Z.zero_solution_device()
            assert not Z.get_solution(F64).any()
            n_z = Z.residual_norm()
            Z.close()
            Fr = _engine(shape, smoother, policy)
            Fr.set_rhs_device(a_rhs.view)
            Fr.set_solution(None)
            _working(Fr, policy)
            n_f = Fr.residual_norm()
            Fr.close()
            _assert_norm(n_z, n_f, H.norm_of(case, "zero_same_kind"), "zero iterate, both mg_set_rhs_device")
            _assert_norm(n_z, n0_host, H.norm_of(case, "zero_host"), "zero iterate, against mg_set_rhs")

        for pk in case["pitches"]:
            a_rhs = H.dev_array(dev, dt, nx, ny, pk, rhs)
            outs = [H.dev_array(dev, dt, nx, ny, pk) for _ in range(2)]
            torch.cuda.synchronize()
            before = G.bits(a_rhs.host())
            X = _engine(shape, smoother, policy)
            X.set_rhs_device(a_rhs.view)
            _working(X, policy)
            X.zero_solution_device()
            hist_x = run(X)
            X.get_solution_device(outs[0].view)
            X.get_solution_device(outs[1].view)                    # reading the iterate must not modify the handle
            X.synchronize()
            u_host = X.get_solution(F64).astype(npdt)
            X.close()
            what = "%s, %s caller arrays, %s pitch" % (case["id"], dt, pk)
            np.testing.assert_array_equal(G.bits(a_rhs.host()), before, err_msg=what + ": the caller's rhs array was modified")
            u_x = H.field_of(outs[0])
            np.testing.assert_array_equal(u_x, u_y, err_msg=what)
            np.testing.assert_array_equal(H.field_of(outs[1]), u_x, err_msg=what + ": second mg_get_solution_device")
            np.testing.assert_array_equal(u_host, u_x, err_msg=what + ": mg_get_solution after mg_get_solution_device")
            if case["large"]:
                _assert_hist(hist_x, hist_y, H.norm_of(case, "history"), what)


def _oracle_cycles(policy, rhs, ncyc):
    """(iterate, residual history) of `ncyc` V(2,2) Jacobi-0.8 cycles from the zero guess at 129 x 65 on (0, 2) x (0, 1), by the
    oracle construction the policy's existing cycle tests use"""
    nx, ny, domain, levels = H.SHAPES["129x65"]
    if policy == "defect":
        mgo = O.MGOracle(nx, ny, domain, max_levels=levels, cycle="V", smoother="jacobi", omega=0.8, jacobi_form="vectorized", coarse_maxit=60)
        u, info = O.defect_correction(mgo, rhs, None, tol=0.0, max_iterations=ncyc)
        return u, info["residual_history"]
    dt = F32 if policy == "single" else F64
    norm_dt = F32 if policy in ("single", "single_managed") else F64          # the precision the fine level computes its residual in
    pm = {"mixed": O.OraclePrecision("mixed"), "single_managed": O.OraclePrecision("single", adaptive=False)}.get(policy)
    mgo = O.MGOracle(nx, ny, domain, dtype=dt, max_levels=levels, cycle="V", smoother="jacobi", omega=0.8, jacobi_form="vectorized", coarse_maxit=60)
    f = rhs.astype(dt)
    u = np.zeros_like(f)
    hx, hy = mgo.h[0]
    hist = []
    for _ in range(ncyc):
        mgo.rhs[0] = f.copy()                  # a policy's cycle converts rhs[0] in place on entry
        u = mgo.cycle_once(u, 0, pm)
        # the oracle's residual in the precision the fine level computes it in, its squares summed in fp64 as the norm kernels
        # do (Grid.l2_norm of an fp32 field sums in fp32: 1e-7, the reference's own error, not the engine's)
        r = O.residual(u.astype(norm_dt), f.astype(norm_dt), hx, hy, mgo.coeff)
        hist.append(float(np.sqrt(hx * hy * np.sum(r.astype(F64) ** 2))))
    return u, hist


@pytest.mark.parametrize("policy", H.ANCHOR_POLICIES)
def test_device_forms_anchor_to_the_oracle(policy):
    """So that fresh-handle references are not circular: per precision policy, two cycles through the device forms at 129 x 65 on
    (0, 2) x (0, 1) against the oracle (MGOracle for DOUBLE and SINGLE, O.defect_correction for DEFECT, the precision manager's
    restatement for the others; ADAPTIVE in its fp64 working precision is a double cycle), with the bounds of
    test_random_shapes_cycles: 1e-11 max|u_ref| on the iterate, rtol 1e-8 / atol 1e-11 max|rhs| on the history."""
    torch, dev = _dev()
    nx, ny = H.SHAPES["129x65"][:2]
    (rhs,), _ = H.fields("129x65", 12)
    dt = "f32" if policy == "single" else "f64"
    u_ref, h_ref = _oracle_cycles("double" if policy == "adaptive_f64" else policy, rhs, 2)
    a_rhs, a_out = H.dev_array(dev, dt, nx, ny, "lib", rhs), H.dev_array(dev, dt, nx, ny, "lib")
    torch.cuda.synchronize()
    X = _engine("129x65", "VJ", policy)
    X.set_rhs_device(a_rhs.view)
    X.zero_solution_device()
    hist = []
    for _ in range(2):
        X.cycle(1)
        hist.append(X.residual_norm())
    X.get_solution_device(a_out.view)
    X.synchronize()
    X.close()
    u = H.field_of(a_out).astype(F64)
    u_ref = u_ref.astype(F64)
    print("%s: max |u - u_ref| = %.3g of max |u_ref| = %.3g; history %r against %r" % (policy, np.max(np.abs(u - u_ref)), np.max(np.abs(u_ref)), hist, h_ref))
    assert np.max(np.abs(u - u_ref)) <= 1e-11 * np.max(np.abs(u_ref))
    np.testing.assert_allclose(hist, h_ref, rtol=1e-8, atol=1e-11 * np.max(np.abs(rhs)))


# ======================================================================================================================
# B. mg_update_rhs_device
# ======================================================================================================================
def _device_cycle(eng, a_rhs, a_out, update, first=False):
    """one step of the replicated coarse engine of a decomposed cycle"""
    if first or not update:
        eng.set_rhs_device(a_rhs.view)
    else:
        eng.update_rhs_device(a_rhs.view)
    eng.zero_solution_device()
    eng.cycle(1)
    eng.get_solution_device(a_out.view)
    eng.synchronize()
    return H.field_of(a_out)


@_ids(H.cases_b())
def test_update_rhs_device_equals_set_rhs_device(case):
    """The decomposed cycle in miniature: rhs_k = one fixed non-zero ring + a new random interior.  Handle A takes rhs_0 through
    mg_set_rhs_device and every later one through mg_update_rhs_device (the rings of its coarse right-hand sides are kept); a
    fresh handle B per k takes rhs_k through mg_set_rhs_device.  The same bits for every k."""
    torch, dev = _dev()
    policy, shape, smoother, dt, pk = (case[k] for k in ("policy", "shape", "smoother", "dt", "pitch"))
    nx, ny = H.SHAPES[shape][:2]
    rhs, _ = H.fields(shape, 21, n_rhs=4)
    arrs = [H.dev_array(dev, dt, nx, ny, pk, f) for f in rhs]
    torch.cuda.synchronize()
    A = _engine(shape, smoother, policy)
    got = [_device_cycle(A, arrs[k], H.dev_array(dev, dt, nx, ny, pk), update=True, first=(k == 0)) for k in range(4)]
    A.close()
    for k in range(4):
        B = _engine(shape, smoother, policy)
        ref = _device_cycle(B, arrs[k], H.dev_array(dev, dt, nx, ny, pk), update=False)
        B.close()
        np.testing.assert_array_equal(got[k], ref, err_msg="%s: right-hand side %d" % (case["id"], k))


@pytest.mark.parametrize("shape,smoother", [("129x65", "WR"), ("257", "VJ")])
def test_update_rhs_device_carries_the_rings_of_both_working_precisions(shape, smoother):
    """MG_PREC_ADAPTIVE: the rings are injected per working precision, and mg_update_rhs_device carries both marks.  rhs_0 in
    fp64, then fp32 / fp64 / fp32 with an update and a cycle each; every stage equals a fresh handle that was given that
    right-hand side through mg_set_rhs_device in that working precision."""
    torch, dev = _dev()
    nx, ny = H.SHAPES[shape][:2]
    rhs, _ = H.fields(shape, 22, n_rhs=4)
    arrs = [H.dev_array(dev, "f64", nx, ny, "min", f) for f in rhs]
    torch.cuda.synchronize()
    A = _engine(shape, smoother, "adaptive_f64")
    A.set_rhs_device(arrs[0].view)
    for k, p in ((1, F32), (2, F64), (3, F32)):
        A.set_working_precision(p)
        got = _device_cycle(A, arrs[k], H.dev_array(dev, "f64", nx, ny, "min"), update=True)
        B = _engine(shape, smoother, "adaptive_f64")
        B.set_rhs_device(arrs[k].view)
        B.set_working_precision(p)
        B.zero_solution_device()
        B.cycle(1)
        out = H.dev_array(dev, "f64", nx, ny, "min")
        B.get_solution_device(out.view)
        B.synchronize()
        B.close()
        np.testing.assert_array_equal(got, H.field_of(out), err_msg="stage %d in %s" % (k, np.dtype(p).name))
    A.close()


@pytest.mark.parametrize("policy,shape,smoother", [("double", "129x65", "WR"), ("single_managed", "257", "VJ")])
def test_update_rhs_device_after_a_host_rhs_keeps_its_ring_sums(policy, shape, smoother):
    """mg_set_rhs (ring sums known), mg_update_rhs_device, a cycle: the norm is the up leg's partial sums plus the ring sum of
    the FIRST right-hand side, whose ring the update promises to share."""
    torch, dev = _dev()
    case = next(c for c in H.B_EXTRA if c["kind"] == "host_first")
    nx, ny = H.SHAPES[shape][:2]
    rhs, _ = H.fields(shape, 23, n_rhs=2)
    a1 = H.dev_array(dev, "f64", nx, ny, "lib+16", rhs[1])
    torch.cuda.synchronize()
    A = _engine(shape, smoother, policy)
    A.set_rhs(rhs[0])
    A.update_rhs_device(a1.view)
    A.cycle(1)
    n_a, u_a = A.residual_norm(), A.get_solution(F64)
    A.close()
    B = _engine(shape, smoother, policy)
    B.set_rhs(rhs[1])
    B.cycle(1)
    n_b, u_b = B.residual_norm(), B.get_solution(F64)
    B.close()
    np.testing.assert_array_equal(u_a, u_b)
    _assert_norm(n_a, n_b, H.norm_of(case, "after_update"), "norm after mg_set_rhs + mg_update_rhs_device")


def test_update_rhs_device_before_any_rhs_is_a_state_error():
    torch, dev = _dev()
    nx, ny = H.SHAPES["129x65"][:2]
    (rhs,), _ = H.fields("129x65", 24)
    a = H.dev_array(dev, "f64", nx, ny, "lib", rhs)
    torch.cuda.synchronize()
    A = _engine("129x65", "VJ", "double")
    lib = _lib.load()
    assert lib.mg_update_rhs_device(A._h, C.c_void_p(a.view.data_ptr()), a.ld, _lib.MG_F64) == _lib.MG_ERR_STATE
    assert "before" in _lib.last_error(A._h)
    assert lib.mg_cycle(A._h, 1) == _lib.MG_ERR_STATE              # ... and changed nothing: there is still no right-hand side
    got = _device_cycle(A, a, H.dev_array(dev, "f64", nx, ny, "lib"), update=False)
    A.close()
    B = _engine("129x65", "VJ", "double")
    ref = _device_cycle(B, a, H.dev_array(dev, "f64", nx, ny, "lib"), update=False)
    B.close()
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("policy,shape,smoother", [("double", "129x65", "WR"), ("mixed_split2", "257", "VJ")])
def test_update_rhs_device_through_a_recorded_plan(policy, shape, smoother):
    """The same loop through a recorded single-rank plan without a communicator: MG_PLAN_COARSE_BEGIN with same_ring 0, then 1,
    MG_PLAN_COARSE_CYCLE, MG_PLAN_COARSE_END -- the bits of the eager calls."""
    torch, dev = _dev()
    from mixed_precision_multigrid_solvers_for_pdes_amd import dist_plan
    nx, ny = H.SHAPES[shape][:2]
    rhs, _ = H.fields(shape, 25, n_rhs=4)
    arrs = [H.dev_array(dev, "f64", nx, ny, "min", f) for f in rhs]
    buf, out = H.dev_array(dev, "f64", nx, ny, "min", rhs[0]), H.dev_array(dev, "f64", nx, ny, "min")
    torch.cuda.synchronize()
    A = _engine(shape, smoother, policy)
    plans = []
    for same_ring in (0, 1):
        rec = dist_plan.PlanRecorder()
        rec.emit(_lib.MG_PLAN_COARSE_BEGIN, i=(buf.ld, _lib.MG_F64, same_ring), p=(A._h.value, buf.view))
        rec.emit(_lib.MG_PLAN_COARSE_CYCLE, i=(1,), p=(A._h.value,))
        rec.emit(_lib.MG_PLAN_COARSE_END, i=(out.ld, _lib.MG_F64), p=(A._h.value, out.view))
        plans.append(dist_plan.CyclePlan(rec, None, 0))
    s0 = torch.cuda.current_stream().cuda_stream
    got = []
    for k in range(4):
        buf.full.copy_(arrs[k].full)
        plans[min(k, 1)].run(s0, s0)
        torch.cuda.synchronize()
        got.append(H.field_of(out))
    assert A.get_stream() == s0                                     # the plan queued the handle's work on its compute stream
    A.set_stream(None)
    for p in plans:
        p.close()
    A.close()
    for k in range(4):
        B = _engine(shape, smoother, policy)
        ref = _device_cycle(B, arrs[k], H.dev_array(dev, "f64", nx, ny, "min"), update=False)
        B.close()
        np.testing.assert_array_equal(got[k], ref, err_msg="right-hand side %d" % k)


# ======================================================================================================================
# C. streams
# ======================================================================================================================
def test_set_stream_orders_work_on_the_callers_stream():
    """mg_get_stream names the handle's own stream, the caller's after mg_set_stream(s), the own one again after
    mg_set_stream(use_own).  With the handle on a torch side stream the right-hand side is produced ON that stream by a chain of
    elementwise passes that is still running when mg_set_rhs_device, mg_zero_solution_device, mg_cycle(2) and
    mg_get_solution_device are queued, with no host synchronisation in between: the result equals the own-stream one bit for
    bit.  A handle that ignored the stream would read the array while it is being produced -- a race, which can pass by luck:
    this test can miss such a bug, it cannot report one that is not there."""
    torch, dev = _dev()
    shape = "1281"
    nx, ny = H.SHAPES[shape][:2]
    (rhs,), _ = H.fields(shape, 31)
    S = _engine(shape, "VJ", "double")
    own = S.get_stream()
    assert own != 0
    side = torch.cuda.Stream(device=dev)
    assert side.cuda_stream != own
    a_rhs, a_out = H.dev_array(dev, "f64", nx, ny, "lib"), H.dev_array(dev, "f64", nx, ny, "lib")
    base = torch.from_numpy(rhs).to(dev)
    torch.cuda.synchronize()
    S.set_stream(side.cuda_stream)
    assert S.get_stream() == side.cuda_stream
    with torch.cuda.stream(side):
        t = base.clone()
        for k in range(48):                                         # ~48 passes over 13 MB: still running when the calls below are queued
            t = t * 1.03125 - base * 0.03125 if k % 2 else t + base * 0.5
        t = t * 2.0 ** -12
        a_rhs.view[:, :ny].copy_(t)
        S.set_rhs_device(a_rhs.view)
        S.zero_solution_device()
        S.cycle(2)
        S.get_solution_device(a_out.view)
    side.synchronize()
    u_side = H.field_of(a_out)
    torch.cuda.synchronize()
    R = _engine(shape, "VJ", "double")                               # own stream, the finished array
    b_out = H.dev_array(dev, "f64", nx, ny, "lib")
    torch.cuda.synchronize()
    R.set_rhs_device(a_rhs.view)
    R.zero_solution_device()
    R.cycle(2)
    R.get_solution_device(b_out.view)
    R.synchronize()
    np.testing.assert_array_equal(u_side, H.field_of(b_out))
    # back on its own stream the handle goes on as a fresh one does
    S.set_stream(None)
    assert S.get_stream() == own
    S.cycle(1)
    R.cycle(1)
    u_s, u_r = S.get_solution(F64), R.get_solution(F64)
    S.close()
    R.close()
    np.testing.assert_array_equal(u_s, u_r)
    Fr = _engine(shape, "VJ", "double")
    Fr.set_rhs_device(a_rhs.view)
    Fr.zero_solution_device()
    Fr.cycle(3)
    u_f = Fr.get_solution(F64)
    Fr.close()
    np.testing.assert_array_equal(u_s, u_f)


# ======================================================================================================================
# D. operator changes leave no trace
# ======================================================================================================================
def _standard_tail(eng, u0):
    eng.set_solution(None)
    n0 = eng.residual_norm()
    eng.set_solution(u0)
    r = eng.iterate(0.0, 3)
    return n0, r, eng.get_solution(F64)


@_ids(H.cases_d())
def test_operator_changes_leave_no_trace(case):
    """After each prefix of handle_call_cases.D_PREFIXES (coefficient and shift changes with solves in between, the norm of the
    zero iterate taken under another operator, a full-multigrid start): the norm of the zero iterate, a three-cycle solve from a
    guess with a non-zero ring, its history, initial residual and precision codes equal those of a fresh handle put into the
    same final operator.  Host forms, exact norms.  With the iterated and the direct coarsest solve, tail 1 and 2."""
    policy, shape, smoother = case["policy"], case["shape"], case["smoother"]
    (rhs,), u0 = H.fields(shape, 41)
    coefs = {1: H.coefficient(shape, 42), 2: H.coefficient(shape, 43), None: None}
    settings = H.D_SETTINGS[case["setting"]]
    refs = {}

    def reference(final):
        if final not in refs:
            coef, shift = final
            eng = _engine(shape, smoother, policy, **settings)
            if shift:
                eng.set_shift(shift)
            if coef is not None:
                eng.set_coefficient(coefs[coef])
            eng.set_rhs(rhs)
            refs[final] = _standard_tail(eng, u0)
            eng.close()
        return refs[final]

    failures = []
    for name in case["prefixes"]:
        steps = H.D_PREFIXES[name]
        eng = _engine(shape, smoother, policy, **settings)
        eng.set_rhs(rhs)
        for s in steps:
            if s[0] == "coef":
                eng.set_coefficient(coefs[s[1]])
            elif s[0] == "shift":
                eng.set_shift(s[1])
            elif s[0] == "solve":
                eng.set_solution(None)
                eng.iterate(0.0, 2)
            elif s[0] == "zero_norm":
                eng.set_solution(None)
                eng.residual_norm()
            elif s[0] == "fmg":
                eng.set_solution(u0)
                eng.fmg(1)
                eng.iterate(0.0, 2)
        n0, r, u = _standard_tail(eng, u0)
        eng.close()
        n0_ref, r_ref, u_ref = reference(H.final_operator(steps))
        print("%s: zero-iterate norm %.17g against %.17g; history %r against %r" % (name, n0, n0_ref, r["residual_history"], r_ref["residual_history"]))
        if not H.norms_agree(n0, n0_ref, H.norm_of(case, "zero_norm")["loose"]):
            failures.append("%s: norm of the zero iterate %.17g, a fresh handle's %.17g" % (name, n0, n0_ref))
        if r["residual_history"] != r_ref["residual_history"] or r["initial_residual"] != r_ref["initial_residual"]:
            failures.append("%s: history %r (initial %.17g), a fresh handle's %r (%.17g)" % (
                name, r["residual_history"], r["initial_residual"], r_ref["residual_history"], r_ref["initial_residual"]))
        if r["precision_codes"] != r_ref["precision_codes"]:
            failures.append("%s: precision codes %r, a fresh handle's %r" % (name, r["precision_codes"], r_ref["precision_codes"]))
        if not np.array_equal(u, u_ref):
            failures.append("%s: iterate differs in %d cells, max %.3g" % (name, int((u != u_ref).sum()), float(np.max(np.abs(u - u_ref)))))
    assert not failures, "\n".join(failures)


# ======================================================================================================================
# E. mg_time_op leaves only what it documents
# ======================================================================================================================
def _time_op(eng, op, level, dtype, reps):
    """(status, milliseconds) of the raw call: MG_ERR_STATE is how a handle declines an op / level / dtype"""
    out = C.c_double(0.0)
    rc = eng._lib.mg_time_op(eng._h, int(op), int(level), _lib.dtype_code(dtype), int(reps), C.byref(out))
    return rc, out.value


def _fresh_solve(make, rhs, u0):
    eng = make()
    eng.set_rhs(rhs)
    eng.set_solution(u0)
    r = eng.iterate(0.0, 2)
    u = eng.get_solution(F64)
    eng.close()
    return u, r


def _after_time_op(case, make, rhs, u0, ref, op, level, dtype, reps=2, zero_guess=False):
    """one transition on a handle of its own: mg_time_op, then (suspect 2) the norm against that of a fresh handle loaded with
    the iterate the handle reports, then (suspect 1) a two-cycle solve against the fresh handle's.  Returns the failures."""
    u_ref, r_ref = ref
    tag = "op %d, level %d, %s" % (op, level, np.dtype(dtype).name)
    S = make()
    S.set_rhs(rhs)
    if zero_guess:                        # the zero guess and its cached norm: an op that rewrites the iterate must drop both
        S.set_solution(None)
        S.residual_norm()
    else:
        S.set_solution(u0)
    rc, _ = _time_op(S, op, level, dtype, reps)
    if rc == _lib.MG_ERR_STATE:
        S.close()
        return None
    fails = []
    if rc not in (_lib.MG_OK, _lib.MG_ERR_INVALID_VALUE):
        fails.append("%s: mg_time_op returned %d (%s)" % (tag, rc, _lib.last_error(S._h)))
    tag += "" if rc == _lib.MG_OK else " (refused)"
    n_s = S.residual_norm()
    u_now = S.get_solution(F64)
    Fr = make()
    Fr.set_rhs(rhs)
    Fr.set_solution(u_now)
    n_f = Fr.residual_norm()
    Fr.close()
    spec = H.norm_of(case, "after_op6" if (op == 6 and rc == _lib.MG_OK) else "after_op")
    if not H.norms_agree(n_s, n_f, spec["loose"]):
        fails.append("%s: mg_residual_norm %.17g, but the iterate mg_get_solution returns has %.17g (%s)" % (
            tag, n_s, n_f, "within %g" % H.NORM_RTOL if spec["loose"] else "exact"))
    S.set_solution(u0)
    r = S.iterate(0.0, 2)
    u = S.get_solution(F64)
    S.close()
    if not np.array_equal(u, u_ref):
        fails.append("%s: the next solve differs from a fresh handle's in %d cells, max %.3g" % (tag, int((u != u_ref).sum()), float(np.max(np.abs(u - u_ref)))))
    if r["residual_history"] != r_ref["residual_history"] or r["initial_residual"] != r_ref["initial_residual"]:
        fails.append("%s: history %r, a fresh handle's %r" % (tag, r["residual_history"], r_ref["residual_history"]))
    if r["last_coarse_sweeps"] != r_ref["last_coarse_sweeps"]:
        fails.append("%s: last_coarse_sweeps %d, a fresh handle's %d" % (tag, r["last_coarse_sweeps"], r_ref["last_coarse_sweeps"]))
    return fails


@_ids(H.cases_e())
def test_time_op_leaves_no_trace(case):
    """For every op 0-9, 12, 13 on every level and dtype the handle accepts (mg_time_op does not return MG_ERR_STATE), each on a
    handle of its own with a right-hand side and a guess whose rings are not zero: afterwards mg_residual_norm is the norm of
    the iterate mg_get_solution returns (exact: both take the full-residual kernel; after op 6 on a fused handle the up leg's
    partial sums are valid and the bound is NORM_RTOL), and mg_set_solution(u0) + mg_iterate(0, 2) gives the iterate, history
    and last_coarse_sweeps of a handle that never ran mg_time_op.  An op the handle refuses with MG_ERR_INVALID_VALUE (the
    spanning leg where it does not apply) must leave nothing either."""
    shape = case["shape"]
    (rhs,), u0 = H.fields(shape, 51)

    def make():
        return _engine(shape, case["smoother"], case["policy"], fused=case["fused"], tail=case["tail"], **case["extra"])

    probe = make()
    levels = case["levels"] if case["levels"] is not None else list(range(probe.num_levels))
    probe.close()
    ref = _fresh_solve(make, rhs, u0)
    failures, ran = [], 0
    for op in case["ops"]:
        for level in levels:
            for dtype in (F64, F32):
                fails = _after_time_op(case, make, rhs, u0, ref, op, level, dtype)
                if fails is not None:
                    ran += 1
                    failures += fails
    print("%s: %d transitions ran" % (case["id"], ran))
    assert ran > 0
    assert not failures, "%d of %d transitions left a trace:\n%s" % (len(failures), ran, "\n".join(failures))


@pytest.mark.parametrize("smoother,fused", [("VJ", 1), ("WR", 3)])
def test_time_op_after_the_zero_guess(smoother, fused):
    """The same transitions on the fine level from the zero guess, after mg_residual_norm has cached ||f|| for it: an op that
    rewrites the fine iterate must not leave mg_residual_norm answering from that cache."""
    case = dict(H.E_ZERO, norms=H._e_norms(fused))
    (rhs,), u0 = H.fields("129x65", 53)

    def make():
        return _engine("129x65", smoother, "double", fused=fused)

    ref = _fresh_solve(make, rhs, u0)
    failures, ran = [], 0
    for op in H.E_OPS:
        fails = _after_time_op(case, make, rhs, u0, ref, op, 0, F64, zero_guess=True)
        if fails is not None:
            ran += 1
            failures += fails
    assert ran >= 9
    assert not failures, "\n".join(failures)


def test_time_op_hbm_ops_leave_no_trace():
    """ops 10 and 11 allocate more than 768 MiB by design: each once, on 129 x 65 and level 0 only"""
    case = dict(H.E_HBM, norms=H._e_norms(1))
    (rhs,), u0 = H.fields("129x65", 52)

    def make():
        return _engine("129x65", "VJ", "double", fused=1)

    ref = _fresh_solve(make, rhs, u0)
    failures = []
    for op in (10, 11):
        fails = _after_time_op(case, make, rhs, u0, ref, op, 0, F64, reps=1)
        assert fails is not None
        failures += fails
    assert not failures, "\n".join(failures)


# ======================================================================================================================
# F. small contracts
# ======================================================================================================================
def test_handle_error_and_profile_contracts():
    torch, dev = _dev()
    lib = _lib.load()
    shape = "129x65"
    nx, ny = H.SHAPES[shape][:2]
    (rhs,), u0 = H.fields(shape, 61)

    # before any right-hand side
    e = _engine(shape, "VJ", "double")
    out, hist, nit, conv = C.c_double(0.0), (C.c_double * 2)(), C.c_int(0), C.c_int(0)
    assert lib.mg_cycle(e._h, 1) == _lib.MG_ERR_STATE
    assert lib.mg_fmg(e._h, 1) == _lib.MG_ERR_STATE
    assert lib.mg_residual_norm(e._h, C.byref(out)) == _lib.MG_ERR_STATE
    assert lib.mg_iterate(e._h, 0.0, 2, hist, 2, C.byref(nit), C.byref(conv), None, None) == _lib.MG_ERR_STATE
    assert "before" in _lib.last_error(e._h)

    # device forms: ld < ny, a bad dtype, a NULL array -> MG_ERR_INVALID_VALUE, caller's array and iterate untouched
    e.set_rhs(rhs)
    e.set_solution(u0)
    arr = H.dev_array(dev, "f64", nx, ny, "lib", rhs)
    torch.cuda.synchronize()
    before = G.bits(arr.host())
    p = C.c_void_p(arr.view.data_ptr())
    for fn in (lib.mg_set_rhs_device, lib.mg_update_rhs_device, lib.mg_get_solution_device):
        assert fn(e._h, p, ny - 1, _lib.MG_F64) == _lib.MG_ERR_INVALID_VALUE
        assert fn(e._h, p, arr.ld, 2) == _lib.MG_ERR_INVALID_VALUE
        assert fn(e._h, p, arr.ld, -1) == _lib.MG_ERR_INVALID_VALUE
        assert fn(e._h, None, arr.ld, _lib.MG_F64) == _lib.MG_ERR_INVALID_VALUE
    e.synchronize()
    np.testing.assert_array_equal(G.bits(arr.host()), before)
    np.testing.assert_array_equal(e.get_solution(F64), u0)
    e.cycle(1)
    u1 = e.get_solution(F64)
    e.close()
    f = _engine(shape, "VJ", "double")
    f.set_rhs(rhs)
    f.set_solution(u0)
    f.cycle(1)
    np.testing.assert_array_equal(u1, f.get_solution(F64))         # ... and the right-hand side too

    # mg_set_working_precision on a handle whose precision is fixed
    assert lib.mg_set_working_precision(f._h, _lib.MG_F32) == _lib.MG_ERR_STATE
    f.close()

    # mg_set_coefficient on a defect-correction handle: refused, and the handle still solves the constant problem
    d = _engine(shape, "VJ", "defect")
    u_a, r_a = d.solve(rhs, u0, tol=0.0, max_iterations=2)
    a = H.coefficient(shape, 62)
    assert lib.mg_set_coefficient(d._h, _lib.ptr(a), _lib.MG_F64) == _lib.MG_ERR_INVALID_VALUE
    u_b, r_b = d.solve(rhs, u0, tol=0.0, max_iterations=2)
    d.close()
    np.testing.assert_array_equal(u_a, u_b)
    assert r_a["residual_history"] == r_b["residual_history"]

    # mg_set_shift(-1 / nan / inf): refused, the shift in force stays
    s = _engine(shape, "WR", "double")
    s.set_shift(0.37)
    u_a, r_a = s.solve(rhs, u0, tol=0.0, max_iterations=2)
    for bad in (-1.0, float("nan"), float("inf")):
        assert lib.mg_set_shift(s._h, bad) == _lib.MG_ERR_INVALID_VALUE
    u_b, r_b = s.solve(rhs, u0, tol=0.0, max_iterations=2)
    s.close()
    np.testing.assert_array_equal(u_a, u_b)
    assert r_a["residual_history"] == r_b["residual_history"]
    s = _engine(shape, "WR", "double")
    u_c, _ = s.solve(rhs, u0, tol=0.0, max_iterations=2)
    s.close()
    assert not np.array_equal(u_a, u_c)                              # the shift that stayed is not the zero one

    # profile = 1: the same iterates and history (it only disables speculation), timings that are reset per solve
    res = {}
    for profile in (False, True):
        e = _engine("257", "VJ", "double", profile=profile)
        e.set_rhs(H.fields("257", 63)[0][0])
        e.set_solution(H.fields("257", 63)[1])
        r = e.iterate(0.0, 3)
        res[profile] = (e.get_solution(F64), r, e.level_timings())
        if profile:
            t = res[True][2]
            assert t[0]["smooth_time"] > 0.0
            assert all(v >= 0.0 for lv in t.values() for v in lv.values())
            # zeros again at the start of the next solve: after eight cycles, a solve that ends after ONE (any norm meets its
            # tolerance) reports that one cycle's time, not nine cycles'
            e.iterate(0.0, 8)
            t8 = e.level_timings()[0]["smooth_time"]
            r1 = e.iterate(1e300, 1)
            assert r1["iterations"] == 1 and r1["converged"]
            assert 0.0 < e.level_timings()[0]["smooth_time"] < t8
        else:
            assert all(v == 0.0 for lv in res[False][2].values() for v in lv.values())
        e.close()
    np.testing.assert_array_equal(res[True][0], res[False][0])
    assert res[True][1]["residual_history"] == res[False][1]["residual_history"]
    assert res[True][1]["initial_residual"] == res[False][1]["initial_residual"]
