"""tests/scale_edge_cases.py on the CPU: that every (entry, shape) of the table takes the path it is there for, that its data
makes every sum exact, and that what the scale tests compare the device with is the modules' own references (shown on two
small shapes); then the closed forms tests/test_gpu_scale_drivers.py measures the drivers with, against the NumPy restatements
at 33 x 33."""
import math
import os
import sys

import numpy as np
import pytest

from oracle import mg_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eig_reference as ER                                                        # noqa: E402
import ho_reference as HO                                                         # noqa: E402
import nl_reference as NL                                                         # noqa: E402
import pcg_reference as PR                                                        # noqa: E402
import scale_edge_cases as S                                                      # noqa: E402

C = S.constants()
SHAPES = S.shapes()
NAMES = ["thin", "tall", "sq"]
SMALL = [(34, 67), (70, 131)]          # tests/test_gpu_ho.py: a second tile row and column, a partial last tile, an odd ny
TILE_SUMS = ["pcg_direction", "pcg_direction_react", "ho_direction", "ho_residual", "heat_rhs", "heat_rhs_var", "flow_rhs", "nl_eval",
             "rd_rhs", "rd_energy"]
STREAMS = ["pcg_update", "pcg_dots", "heat_diff_sumsq", "flow_diag", "flow_interior", "eig_combine", "eig_residual"]


def test_constants_are_parsed_and_the_table_is_the_smallest_of_its_kind():
    for key in ("kReduceBlock", "kBlock", "kTI", "kTileRowBytes", "kNumXcd", "kGramWorkgroups"):
        assert C[key] > 0
    R = C["kReduceBlock"]
    if (R, C["kTI"], C["TJ"]) == (1024, 32, 64):          # with today's constants: the shapes and tile counts of the table
        assert SHAPES == {"thin": (65, 65921), "tall": (65921, 65), "sq": (1475, 1471)}
        assert [S.tile_grid(SHAPES[n]) for n in NAMES] == [(3, 1031), (2061, 2), (47, 23)]
        assert [S.tile_grid(SHAPES[n], True) for n in NAMES] == [(2, 1030), (2060, 1), (47, 23)]
    for name in ("thin", "tall"):
        assert S.ntiles(SHAPES[name]) > 2 * R and S.ntiles(SHAPES[name], True) > 2 * R
    assert R < S.ntiles(SHAPES["sq"]) < 2 * R and S.ntiles(SHAPES["sq"]) % C["kNumXcd"] == 1
    assert SHAPES["tall"][1] == C["TJ"] + 1                # a last tile column one cell wide
    assert SHAPES["sq"][0] % C["kTI"] and SHAPES["sq"][1] % C["TJ"]
    for name in NAMES:
        assert S.ntiles(SHAPES[name]) % C["kNumXcd"] and S.ntiles(SHAPES[name], True) % C["kNumXcd"]
        assert 8 * SHAPES[name][0] * SHAPES[name][1] <= 35e6          # 35 MB of cells or less per field


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("entry", S.ENTRIES)
def test_every_case_takes_the_path_it_claims(entry, name):
    shape = SHAPES[name]
    R = C["kReduceBlock"]
    scratch = S.max_partials(*shape)
    for f in S.chain_facts(entry, shape):
        # every set of partials lies inside mg_dev_scratch_bytes
        assert f["sets"] * f["offset"] <= scratch or f["partials"] == 0, (entry, name, f, scratch)
        if f["kind"] == "gram":
            assert f["workgroups"] * f["block"] <= scratch
        elif f["partials"]:
            assert (f["sets"] - 1) * f["offset"] + f["partials"] <= scratch
            assert f["sets"] == 1 or f["offset"] >= f["partials"]          # the sets do not overlap
        if entry in TILE_SUMS:
            assert f["partials"] > (R if name == "sq" else 2 * R) and f["partials"] % C["kNumXcd"] != 0
            if name == "sq":
                assert f["partials"] < 2 * R          # the unrolled loop of the reduce runs for some threads only
            if f["sets"] > 1 and name == "tall":
                assert f["offset"] > 4000
        if entry in ("ho_rhs", "eig_apply"):
            assert f["workgroups"] > R and f["workgroups"] % C["kNumXcd"] != 0
        if entry in STREAMS:
            assert f["chunks"] >= 3 and f["partial_last"], (entry, name, f)
        if entry in S.RING_ENTRIES and name != "sq":
            assert f["chunks"] >= 2 and f["partial_last"]
        if entry.startswith("eig_gram"):
            assert f["chunks"] >= 3 and f["partial_last"] and f["workgroups"] >= 2
    if entry == "rd_energy":
        assert 3 * S.even(S.ntiles(shape)) <= scratch          # the guard of mg_dev_rd_energy holds


def test_scalars_and_weights_are_dyadic():
    for key, v in S.SCALARS.items():
        assert S.is_dyadic(v), key
    hx, hy = S.ho_spacings()
    assert 1.0 / (hx * hx) == 1.0 and 1.0 / (hy * hy) == 11.0
    assert HO.coefficients(hx, hy, 0.0) == (20.0, 1.0, -9.0, 1.0)
    assert 12.0 * S.HX * S.HY == 6.0 and S.FLOW_PEAK % 3 == 0          # the Jacobian's divisor: psi holds multiples of 3
    for n in S.scalar_lengths():
        for k in range(6):
            a = S.partial_array(n, k)
            assert np.all(a == np.rint(a)) and np.all(a >= 1) and a.sum() < 2 ** 53
    R = C["kReduceBlock"]
    assert S.scalar_lengths() == [R - 1, R, R + 1, 2 * R - 1, 2 * R + 1, 3 * R + 21]


def _arrays(d):
    for key, v in d.items():
        if isinstance(v, np.ndarray):
            yield key, v


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("entry", S.ENTRIES)
def test_every_case_is_exact(entry, name):
    """S.case forms every expected sum with exact_dot, which refuses data whose sum could round in some order: building the
    case is the assertion.  Inputs are integers, no cell of a field is 0."""
    if entry == "eig_gram_18x36" and name != "sq":
        # 36 columns of 4.3 M cells: the bound is cells x 3 x 3 < 2^53 whatever the data; the case itself runs on the device test
        assert SHAPES[name][0] * SHAPES[name][1] * 9 < 2 ** 53
        return
    for variant in S.variants(entry):
        c = S.case(entry, SHAPES[name], variant)
        for key, a in _arrays(c["inputs"]):
            assert np.all(a * 8 == np.rint(a * 8)), (entry, key)
            if key not in ("w", "c", "coef", "lam"):          # weights hold zeros on purpose
                assert np.all(interior_or_all(a, c, key) != 0), (entry, key)
        for key, v in c["sums"].items():
            assert np.all(np.abs(np.asarray(v)) < 2.0 ** 53)
        assert c["sums"] or c["fields"]


def interior_or_all(a, c, key):
    # z, p, r, q of the Krylov kernels and the combine inputs carry a zero ring by contract
    return S.interior(a) if key in ("z", "p", "q", "r", "cols") else a


@pytest.mark.parametrize("where,nan", [(0.875, False), (1.0, False), (1.0, True)])
@pytest.mark.parametrize("name", NAMES)
def test_flow_maxima_sit_late_and_a_nan_reaches_only_the_maximum(name, where, nan):
    shape = SHAPES[name]
    n = S.ntiles(shape)
    b, cell = S.late_tile_cell(shape, where)
    assert b >= (0.85 if where < 1 else 0.99) * n - 8
    ti, tj = divmod(S.xcd_remap(b, n), S.tile_grid(shape)[1])
    assert ti * C["kTI"] <= cell[0] < (ti + 1) * C["kTI"] and tj * C["TJ"] <= cell[1] < (tj + 1) * C["TJ"]
    assert sorted(S.xcd_remap(k, n) for k in range(n)) == list(range(n))
    c = S.flow_case("flow_rhs", shape, peak=None if nan else cell, nan=cell if nan else None)
    assert math.isnan(c["maxima"]["m"]) if nan else c["maxima"]["m"] >= 2 * S.FLOW_PEAK
    for entry, rows_from, key in (("flow_diag", 1, "m"), ("flow_interior", 0, "change")):
        f = S.chain_facts(entry, shape)[0]
        wg, chunk, cell = S.late_stream_cell(shape, C["cap_flow_stream"], rows_from, where)
        assert chunk == f["chunks"] - 1 if where == 1.0 else chunk >= 0.8 * f["chunks"] - 1
        c = S.flow_case(entry, shape, peak=None if nan else cell, nan=cell if nan else None)
        assert math.isnan(c["maxima"][key]) if nan else c["maxima"][key] >= S.FLOW_PEAK
        assert all(math.isfinite(v) for v in c["sums"].values())          # built by exact_dot: the NaN enters no sum


@pytest.mark.parametrize("shape", SMALL, ids=["%dx%d" % s for s in SMALL])
def test_the_references_used_at_scale_are_the_modules_own(shape):
    """the cases call pcg_reference, nl_reference, ho_reference, heat_device_reference, heat_var_reference, flow_reference,
    rd_reference and eig_reference directly; what they form themselves -- the operator of the Krylov kernels through
    nl_reference.apply_A, the Gram product as a matrix product, the sums through exact_dot -- equals the references the
    small-shape device tests use"""
    for variant in ("const", "var"):
        c = S.case("pcg_direction", shape, variant)
        p, a = c["fields"]["p"], c["inputs"]["a"]
        if a is None:
            want = O.apply_laplacian(p, S.HX, S.HY, -1.0, S.SIGMA)
        else:
            want = PR.zero_ring(-O.var_residual(p, np.zeros_like(p), a, S.HX, S.HY, -1.0, S.SIGMA))
        assert np.array_equal(c["fields"]["q"], want)
        assert c["sums"]["pq"] == math.fsum((p * want).ravel().tolist())
        r = S.case("pcg_direction_react", shape, variant)
        assert np.array_equal(r["fields"]["q"], PR.zero_ring(want + r["inputs"]["c"] * p))
    c = S.case("eig_apply", shape)
    for col, av in zip(c["inputs"]["cols"], c["fields"]["av"]):
        assert np.array_equal(av, O.apply_laplacian(PR.zero_ring(col), S.HX, S.HY, -1.0, 0.0))
    c = S.case("eig_gram_18x36", shape)
    v = c["inputs"]["v"]
    assert np.array_equal(c["sums"]["G"], ER.gram(S.interior(v[:18]), S.interior(v)))
    c = S.case("eig_combine", shape)
    assert np.array_equal(c["fields"]["out"], ER.mix(c["inputs"]["cols"], c["inputs"]["coef"]))
    c = S.case("ho_residual", shape)
    hx, hy = S.ho_spacings()
    assert np.array_equal(c["fields"]["r"], HO.residual(c["inputs"]["x"], c["inputs"]["g"], hx, hy, -1.0, 0.0))
    # exact_dot is math.fsum (the reference sum of the small-shape tests) wherever it accepts the data
    for entry in ("heat_rhs", "rd_rhs", "nl_eval", "flow_rhs", "ho_direction"):
        for variant in S.variants(entry):
            c = S.case(entry, shape, variant)
            key = {"heat_rhs": "out", "rd_rhs": "out", "nl_eval": "F", "flow_rhs": "f", "ho_direction": None}[entry]
            if key:
                f = c["fields"][key]
                assert next(iter(c["sums"].values())) == math.fsum((f * f).ravel().tolist())
            else:
                assert c["sums"]["pq"] == math.fsum((c["fields"]["p"] * c["fields"]["q"]).ravel().tolist())
    G, P, Q = (S.RD.energy_terms(NL.CUBIC, S.ints(shape, 1), S.HX, S.HY))
    c = S.case("rd_energy", shape, "plain")
    assert [c["sums"][k] for k in "GPQ"] == [math.fsum(t.ravel().tolist()) for t in (G, P, Q)]


def test_exact_dot_refuses_what_could_round():
    with pytest.raises(AssertionError):
        S.exact_dot(np.array([1.0, 0.1]))
    with pytest.raises(AssertionError):
        S.exact_dot(np.full(4, 2.0 ** 30), np.full(4, 2.0 ** 22))
    assert S.exact_dot(np.array([1.5, -0.25]), np.array([2.0, 4.0])) == 2.0


# ============================================================================================== the drivers' closed forms
# tests/test_gpu_scale_drivers.py measures the drivers at 1281 x 1281 with these; here each is the NumPy restatement's answer
# at 33 x 33, to within the bound the driver test derives (scale_edge_cases.stepper_bound, rounding_floor).
import flow_reference as FR                                                       # noqa: E402
import heat_device_reference as HD                                                # noqa: E402
import rd_reference as RD                                                         # noqa: E402

N33 = 33
H33 = 1.0 / (N33 - 1)
DT, ALPHA, STEP_TOL = 0.01, 1.0, 1e-10
MODES33 = [(2, 3), (N33 - 3, N33 - 4)]
LIP33 = 8.0 * (N33 - 1) ** 2


def nh33(v):
    return S.norm_h(v, N33, N33)


def test_discrete_eigenvalues_are_those_of_the_references_operators():
    mgo = PR.make_oracle(N33, N33)
    floor = 16 * S.EPS * 8.0 / H33 ** 2                          # a stencil's roundings on a mode of magnitude <= 1
    for k, l in [(1, 1), (2, 3), (17, 9), (N33 - 3, N33 - 4), (N33 - 2, N33 - 2)]:
        m = S.mode(N33, N33, k, l)
        assert abs(nh33(m) - 0.5) <= 4 * S.EPS
        d = S.mode_defect(k, l)                                   # the computed mode is an eigenvector up to this
        tol = floor + (8.0 / H33 ** 2 + S.lam_kl(N33, N33, k, l)) * d
        assert np.max(np.abs(PR.apply_A(mgo, m) - S.lam_kl(N33, N33, k, l) * m)) <= tol          # eig_reference's operator
        assert np.max(np.abs(HO.apply_A4(m, H33, H33) - S.lam4_kl(N33, N33, k, l) * m)) <= tol
        assert np.max(np.abs(S.interior(HO.rhs_average(m) - S.avg_kl(N33, N33, k, l) * m))) <= 8 * S.EPS + 2 * d
    exact, index = ER.exact_dirichlet(N33, N33, (0.0, 1.0, 0.0, 1.0), 6)
    for lam, (k, l) in zip(exact, index):
        assert abs(lam - S.lam_kl(N33, N33, k, l)) <= 4 * S.EPS * lam
    assert S.lam_min(N33, N33) == pytest.approx(exact[0], rel=1e-14)
    # the nine-point operator's smallest eigenvalue, against the dense matrix of a smaller grid
    dense = np.linalg.eigvalsh(HO.dense_matrix(17, 17, 1 / 16, 1 / 16))
    assert S.lam_min(17, 17, 4) == pytest.approx(dense[0], rel=1e-12)
    assert S.lam_min(17, 17) == pytest.approx(np.linalg.eigvalsh(HO.dense_matrix(17, 17, 1 / 16, 1 / 16, apply=HO.apply_A2))[0], rel=1e-12)


def _bound33(scheme, lam, c, shift_of, kappa=0.0, rho=0.0):
    lmin = S.lam_min(N33, N33)
    shifts = [shift_of(S.heat_scheme_of_step(scheme, k)) for k in range(S.DRIVER_STEPS)]
    fn = [(lam + shifts[k] + kappa / ALPHA) * abs(c[k + 1]) * 0.5 for k in range(S.DRIVER_STEPS)]
    un = [max(abs(c[k]), abs(c[k + 1])) * 0.5 for k in range(S.DRIVER_STEPS)]
    carries = [S.carry_of(scheme, k, DT, rho, ALPHA * lmin + kappa) for k in range(S.DRIVER_STEPS)]
    return S.stepper_bound(STEP_TOL, shifts, lmin, fn, un, LIP33 + 2 * max(shifts) + 4 * abs(rho), carries, N33, N33)


@pytest.mark.parametrize("mode", MODES33, ids=["smooth", "high"])
@pytest.mark.parametrize("scheme", [HD.IMPLICIT, HD.CN, HD.BDF2])
def test_heat_factors_are_the_restatements_steps(scheme, mode):
    lam = float(S.lam_kl(N33, N33, *mode))
    u0 = S.mode(N33, N33, *mode)
    c = S.heat_factors(scheme, DT, ALPHA, lam)
    levels = [u0]
    for k in range(S.DRIVER_STEPS):
        sch = S.heat_scheme_of_step(scheme, k)
        levels.append(HD.step(sch, levels[-1], DT, ALPHA, u_prev=levels[-2] if sch == HD.BDF2 else None, tol=STEP_TOL, max_cycles=40)[0])
    err = nh33(levels[-1] - c[-1] * u0)
    bound = _bound33(scheme, lam, c, lambda sch: HD.lam(sch, DT, ALPHA)) + 2 * S.mode_defect(*mode)
    print(scheme, mode, "factor", c[-1], "error", err, "bound", bound)
    assert err <= bound
    assert abs(c[-1]) <= 1.0 and (scheme != HD.IMPLICIT or c[-1] == pytest.approx((1.0 + DT * ALPHA * lam) ** -S.DRIVER_STEPS))


@pytest.mark.parametrize("mode", MODES33, ids=["smooth", "high"])
@pytest.mark.parametrize("scheme", [RD.IMPLICIT, RD.CN, RD.BDF2])
def test_reaction_diffusion_factors_are_the_restatements_steps(scheme, mode):
    kappa, rho = 20.0, 5.0
    lam = float(S.lam_kl(N33, N33, *mode))
    u0 = S.mode(N33, N33, *mode)
    c = S.rd_factors(scheme, DT, ALPHA, lam, kappa, rho)
    levels = RD.run(scheme, NL.LINEAR, u0, DT, S.DRIVER_STEPS, ALPHA, kappa, rho, tol=STEP_TOL)
    err = nh33(levels[-1] - c[-1] * u0)
    bound = _bound33(scheme, lam, c, lambda sch: RD.lam(sch, DT, ALPHA), kappa, rho) + 2 * S.mode_defect(*mode)
    print(scheme, mode, "factor", c[-1], "error", err, "bound", bound)
    assert err <= bound


@pytest.mark.parametrize("mode", MODES33, ids=["smooth", "high"])
def test_flow_factor_is_the_restatements_step(mode):
    """w0 = lambda psi0 on one mode: the Jacobian vanishes (to the solver's tolerance), the first step has c0 = 1, c1 = 0 and
    takes the same Crank-Nicolson factor as the others"""
    nu, dt = 0.05, 0.01
    lam = float(S.lam_kl(N33, N33, *mode))
    psi0 = S.mode(N33, N33, *mode)
    w0 = lam * psi0
    assert np.max(np.abs(FR.jacobian(psi0, w0, H33, H33))) <= 64 * S.EPS * lam / (H33 * H33)          # antisymmetry, up to rounding
    g = S.flow_factor(nu, dt, lam)
    sigma = 2.0 / (nu * dt)
    fl = FR.Flow(N33, N33, nu, kind=FR.FREE_SLIP, solver=FR.CycleSolver(N33, N33, tol=STEP_TOL, max_cycles=60))
    fl.set_state(w0)
    extra = []
    for k in range(S.DRIVER_STEPS):
        jn = nh33(FR.jacobian(fl.psi, fl.w, H33, H33))
        prev = extra[-1][1] if extra else 0.0
        c0, c1 = FR.ab2(dt, dt if k else None)
        extra.append(((2.0 / nu) * (abs(c0) * jn + abs(c1) * prev), jn))
        info = fl.step(dt)
        assert (info["c0"], info["c1"]) == ((1.0, 0.0) if k == 0 else (1.5, -0.5))
    ex = [e[0] for e in extra]
    wn = nh33(w0)
    lmin = S.lam_min(N33, N33)
    fn = [(sigma + lam) * abs(g) ** (k + 1) * wn + ex[k] for k in range(S.DRIVER_STEPS)]
    un = [abs(g) ** k * wn for k in range(S.DRIVER_STEPS)]
    ew = S.stepper_bound(STEP_TOL, [sigma] * S.DRIVER_STEPS, lmin, fn, un, LIP33 + 2 * sigma, [(1.0, 0.0)] * S.DRIVER_STEPS, N33, N33, ex)
    err = nh33(fl.w - g ** S.DRIVER_STEPS * w0)
    print(mode, "factor", g, "error", err, "bound", ew)
    d = 2 * lam * S.mode_defect(*mode)                          # what is not the mode decays by other factors, all <= 1
    assert err <= ew + d
    floor = S.rounding_floor(N33, N33, "const", 0.0, 1.0, nh33(fl.psi))
    assert nh33(fl.psi - g ** S.DRIVER_STEPS * psi0) <= (ew + d + STEP_TOL * max(1.0, nh33(fl.w)) + floor) / lmin


@pytest.mark.parametrize("kind", ["const", "var", "ho"])
def test_pcg_tolerance_stands_ten_floors_above_rounding(kind):
    """the problems of the driver test, built at its size: the tolerance it asks for is >= 10 x the rounding floor of a residual
    norm of u*, f has a zero ring and u* solves the discrete problem to that floor"""
    n = 1281
    us, f, a, tol, floor = S.pcg_problem(n, n, kind)
    assert tol >= 10 * floor, (tol, floor)
    assert not f[0].any() and not f[-1].any() and not f[:, 0].any() and not f[:, -1].any()
    assert S.norm_h(S.np_residual(kind, us, f, a), n, n) <= floor
    assert a is None or (float(a.min()), float(a.max())) == (1.0, S.PCG_CONTRAST)
