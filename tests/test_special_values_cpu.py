"""The CPU half of the special-value tests (tests/test_gpu_nonfinite.py and tests/test_gpu_range_edges.py are the GPU half):
the helpers of tests/special_values.py themselves, that the finite extreme fields of dev_call_cases.special_cases() do on
the restatement what they are chosen for -- subnormal stored values under `tiny`, at most 1 % non-finite stored cells under
`huge` (a cap on the INPUT choice, not a tolerance) -- and that the flow restatement blows up from rest the way the
driver test expects: non-finite within 40 steps, NaN thereafter, where a maximum formed with fmax would report 0."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dev_call_cases as G  # noqa: E402
import dist_helpers as H  # noqa: E402
import flow_reference as R  # noqa: E402
import special_values as SV  # noqa: E402

Ref = G.make_ref_ops(H.NumpyOps)
SPECIAL = G.special_cases()


# ======================================================================================================================
# 1. the helpers
# ======================================================================================================================
@pytest.mark.parametrize("shape", [(5, 5), (9, 130), (35, 67), (33, 66), (65, 131), (17, 17)])
def test_plant_positions(shape):
    nx, ny = shape
    pos = dict(SV.plant_positions(nx, ny))
    assert len(set(pos.values())) == len(pos)                                      # every cell once
    assert pos["first"] == (1, 1)
    for name in ("first", "last", "centre", "tile0_last", "last_tile_row", "last_tile_col"):
        if name in pos:
            assert SV.is_interior(pos[name], nx, ny), name
    assert (nx - 2, ny - 2) in pos.values() and (nx // 2, ny // 2) in pos.values()
    ti, tj = SV.TILE_I, SV.TILE_J["f64"]              # the last tile starts at a multiple of the extent; it may hold the far ring alone
    assert ("last_tile_row" in pos) == (0 < (nx - 1) // ti * ti <= nx - 2) and ("last_tile_col" in pos) == (0 < (ny - 1) // tj * tj <= ny - 2)
    if "last_tile_row" in pos:
        assert pos["last_tile_row"][0] >= SV.TILE_I and pos["tile0_last"][0] == SV.TILE_I - 1
    if "last_tile_col" in pos:
        assert pos["last_tile_col"][1] >= SV.TILE_J["f64"] and pos["tile0_last"][1] == SV.TILE_J["f64"] - 1
    rings = [pos[k] for k in ("ring_ilo", "ring_ihi", "ring_jlo", "ring_jhi")]
    assert [r[0] for r in rings[:2]] == [0, nx - 1] and [r[1] for r in rings[2:]] == [0, ny - 1]
    for r in rings:
        assert SV.in_array(r, nx, ny) and not SV.is_interior(r, nx, ny) and not SV.is_corner(r, nx, ny)
    assert SV.is_corner(pos["corner_lo"], nx, ny) and SV.is_corner(pos["corner_hi"], nx, ny) and pos["corner_lo"] != pos["corner_hi"]
    assert ("pad" in pos) == bool(ny % 2)
    if ny % 2:
        assert pos["pad"][1] == ny and 1 <= pos["pad"][0] <= nx - 2 and not SV.in_array(pos["pad"], nx, ny)


def test_values_are_canonical():
    assert len(SV.VALUES) == 3 and math.isnan(SV.VALUES[0]) and SV.VALUES[1:] == (math.inf, -math.inf)
    assert int(np.float64(SV.VALUES[0]).view(np.uint64)) == 0x7FF8000000000000 != G.SENT_BITS[8]


def test_same_special():
    nan, inf = SV.NAN, np.inf
    a = np.array([[1.0, nan, inf, -inf, 0.0, 5e-324]])
    assert SV.same_special(a, a.copy())
    other_payload = a.copy()
    other_payload.view(np.uint64)[0, 1] = G.SENT_BITS[8]                           # NaN-ness, not the payload
    assert SV.same_special(a, other_payload)
    for j, v in ((0, nan), (1, 1.0), (1, inf), (2, -inf), (2, 1.7e308), (3, inf), (4, -0.0), (5, 0.0), (5, 1e-323), (0, np.nextafter(1.0, 2.0))):
        b = a.copy()
        b[0, j] = v
        assert not SV.same_special(a, b) and not SV.same_special(b, a), (j, v)
        assert SV.special_mismatch(a, b).sum() == 1
    f = np.array([1.0, nan, inf], dtype=np.float32)
    assert SV.same_special(f, f.copy()) and not SV.same_special(f, np.array([1.0, nan, -inf], dtype=np.float32))
    with pytest.raises(ValueError):
        SV.same_special(f, f.astype(np.float64))
    # scalars
    assert SV.same_special(nan, float("nan")) and SV.same_special(inf, inf) and SV.same_special(2.5, 2.5)
    assert not SV.same_special(nan, 0.0) and not SV.same_special(0.0, nan) and not SV.same_special(inf, -inf)
    assert not SV.same_special(inf, 1.7e308) and not SV.same_special(0.0, -0.0)
    # sums: non-finite by same_special, finite by the rule of compare_sum
    assert SV.same_sum(nan, nan) and SV.same_sum(inf, inf) and not SV.same_sum(0.0, nan) and not SV.same_sum(nan, 1.0)
    assert not SV.same_sum(inf, 1e308) and not SV.same_sum(1e308, inf) and not SV.same_sum(inf, nan)
    assert SV.same_sum(1.0 + 1e-13, 1.0) and not SV.same_sum(1.0 + 1e-11, 1.0) and SV.same_sum(0.0, 0.0)


def test_compare_call_with_special_values():
    """the extended comparison: a NaN for a NaN passes whatever its payload, anything else must have the reference's bits, and a
    cell the reference leaves untouched must still hold the sentinel"""
    case = dict(entry="residual", id="x", dyadic=True, dt="f64", nx=6, ny=7, pf="min")
    ld = G.pitch("min", "f64", 7)
    ref = G.sentinel(np.float64, (6 + 2 * G.GUARD, ld))
    ref[G.GUARD:G.GUARD + 6, :7] = np.arange(42.0).reshape(6, 7)
    ref[G.GUARD + 2, 3], ref[G.GUARD + 3, 3] = SV.NAN, np.inf
    got = ref.copy()
    got.view(np.uint64)[G.GUARD + 2, 3] = 0xFFF8000000000001                       # another NaN
    G.compare_array(case, "r", got, ref, 6, 7, special=True)
    with pytest.raises(AssertionError):
        G.compare_array(case, "r", got, ref, 6, 7)                                 # the plain comparison keeps asking for equal bits
    for i, j, v in ((2, 3, 0.0), (3, 3, -np.inf), (3, 3, SV.NAN), (1, 1, SV.NAN), (4, 4, -0.0 if ref[G.GUARD + 4, 4] == 0 else 0.0)):
        bad = ref.copy()
        bad[G.GUARD + i, j] = v
        with pytest.raises(AssertionError):
            G.compare_array(case, "r", bad, ref, 6, 7, special=True)
    bad = ref.copy()
    bad[G.GUARD + 1, 1] = G.sentinel(np.float64, (1,))[0]                           # untouched where the reference stored
    with pytest.raises(AssertionError):
        G.compare_array(case, "r", bad, ref, 6, 7, special=True)
    G.compare_sum(case, np.inf, np.inf, 5, 1.0, np.float64, special=True)
    G.compare_sum(case, SV.NAN, SV.NAN, 5, 1.0, np.float64, special=True)
    for g, r in ((0.0, SV.NAN), (SV.NAN, 1.0), (np.inf, 1e300), (1e300, np.inf)):
        with pytest.raises(AssertionError):
            G.compare_sum(case, g, r, 5, 1.0, np.float64, special=True)


def test_straddle_values_round_as_documented():
    with np.errstate(over="ignore", under="ignore"):
        as32 = np.array(SV.F32_EDGE_VALUES).astype(np.float32)
    fmax = np.finfo(np.float32).max
    want = [fmax, -fmax, fmax, np.inf, -np.inf, 2.0 ** -149, -2.0 ** -149, 0.0, 2.0 ** -148, -0.0, 0.0]      # 1.5 * 2^-149: a tie, to even
    assert SV.same_special(as32, np.array(want, dtype=np.float32))
    assert SV.ROUNDS_TO_FLT_MAX < SV.ROUNDS_TO_INF == float(np.nextafter(SV.ROUNDS_TO_FLT_MAX, np.inf))
    d = SV.straddle_fill(np.ones((5, 40)))
    for v in SV.F32_EDGE_VALUES:
        assert (d == v).any()
    assert (d == 1.0).sum() > d.size // 2


def test_field_kinds_and_the_unchanged_default():
    """without case["field"] build_arrays gives the bits it always gave; with it, the scale of the narrowest dtype"""
    base = dict(entry="residual_mixed", dt="f32", dtc="f64", nx=9, ny=12, pf="lib", pc="min", seed=77)
    rng = np.random.default_rng(77)
    u = rng.standard_normal((9, 12))
    A = G.build_arrays(base)
    assert np.array_equal(A["u"].host()[G.GUARD:G.GUARD + 9, :12], u.astype(np.float32))
    assert SV.narrowest(base) == "f32" and SV.narrowest(dict(entry="residual", dt="f64", nx=9, ny=12)) == "f64"
    T = G.build_arrays(dict(base, field="tiny"))
    assert np.array_equal(T["u"].host()[G.GUARD:G.GUARD + 9, :12], (u * 2.0 ** -135).astype(np.float32))
    assert SV.is_subnormal(T["u"].host()[G.GUARD:G.GUARD + 9, :12]).all()
    assert np.array_equal(G.bits(T["r"].host()), G.bits(A["r"].host()))            # outputs: the sentinel, as ever
    P = G.build_arrays(dict(entry="residual", dt="f64", nx=40, ny=50, pf="lib", seed=5, field="patches"))["u"].host()[G.GUARD:G.GUARD + 40, :50]
    assert SV.is_subnormal(P).any() and np.abs(P).max() > 1e199 and np.isfinite(P).all()
    var = dict(entry="var_rdiag", dt="f64", nx=9, ny=12, pf="lib", seed=3)
    assert np.array_equal(G.bits(G.build_arrays(dict(var, field="huge"))["a"].host()), G.bits(G.build_arrays(var)["a"].host()))      # coefficients stay


def test_special_case_list():
    ids = [c["id"] for c in SPECIAL]
    assert len(set(ids)) == len(ids)
    default = G.default_cases()
    for name in G.ENTRIES:
        mine = [c for c in SPECIAL if G.entry_name(c) == name and c["field"] in SV.KINDS]
        combos = {(c.get("dt"), c.get("dtc"), c.get("comp")) for c in default if G.entry_name(c) == name and c["disp"] == "compare"}
        assert {(c.get("dt"), c.get("dtc"), c.get("comp")) for c in mine} == combos, name
        assert len(mine) == 3 * len(combos), name
        for combo in combos:
            assert {c["field"] for c in mine if (c.get("dt"), c.get("dtc"), c.get("comp")) == combo} == set(SV.KINDS)
    assert all(c["dyadic"] and c["sp"] in ("eq", "neq") for c in SPECIAL) and {c["sp"] for c in SPECIAL} == {"eq", "neq"}
    assert max(G.cells(c) for c in SPECIAL) == 1102 * 1122
    for c in SPECIAL:
        if c["entry"] in ("down_leg", "up_leg", "span_leg"):
            assert (c["nx"], c["ny"]) in G.SPECIAL_LEG_SHAPES
        else:
            assert (c["nx"], c["ny"]) in G.SPECIAL_OP_SHAPES.values()
    for entry in ("down_leg", "up_leg"):                                           # every family of tile
        assert {G.leg_family(c) for c in SPECIAL if c["entry"] == entry} == {"tiny", "small", "rb"}
    assert {c["entry"] for c in SPECIAL if c["field"] == "straddle"} == {"convert", "restrict", "residual_mixed"}
    # the default list has not moved
    assert all("field" not in c for c in default)


# ======================================================================================================================
# 2. the input choices, on the restatement
# ======================================================================================================================
def _stored(case, ref):
    """the cells the reference stored, of every output, as one fp64 vector (stored: no longer the sentinel)"""
    specs = G.array_specs(case)
    out = []
    for name in G.OUTPUTS[case["entry"]]:
        dt, nx, ny, pk, role = specs[name]
        a = ref[name][G.GUARD:G.GUARD + nx, :ny]
        out.append((a, G.bits(a) != G.SENT_BITS[a.dtype.itemsize]))
    return out


@pytest.mark.parametrize("case", [c for c in SPECIAL if c["field"] in ("tiny", "huge")], ids=lambda c: c["id"])
def test_kinds_do_what_they_are_chosen_for(case):
    ref, ref_sum, rops = G.run_reference(case, Ref)
    stored = _stored(case, ref)
    has_data = any(role in ("in", "inout") for *_, role in G.array_specs(case).values())
    if case["field"] == "huge":
        n = sum(int(m.sum()) for _, m in stored)
        bad = sum(int((~np.isfinite(a[m])).sum()) for a, m in stored)
        print(case["id"], "stored", n, "non-finite", bad, "sum", ref_sum)
        assert bad <= 0.01 * n                                                     # a cap: pick another exponent if a case exceeds it
        if ref_sum is not None:
            assert math.isfinite(ref_sum) and ref_sum > 0.0
    elif has_data and stored:
        # subnormal in the narrowest dtype among the call's arrays, the one the scale is taken from: an fp64 output of fp32
        # inputs (mg_dev_residual_f32in_f64out, an fp32 -> fp64 conversion) holds the subnormal fp32 range as normal doubles
        tiny = float(np.finfo(G.NPDT[SV.narrowest(case)]).tiny)
        sub = sum(int(((a[m] != 0) & (np.abs(a[m].astype(np.float64)) < tiny)).sum()) for a, m in stored)
        print(case["id"], "stored", sum(int(m.sum()) for _, m in stored), "subnormal", sub)
        assert sub >= 1
    else:
        # mg_dev_sumsq stores no cell and mg_dev_var_rdiag reads a coefficient field only, which no kind scales
        assert case["entry"] in ("sumsq", "var_rdiag")
        if ref_sum is not None:
            assert math.isfinite(ref_sum)


# ======================================================================================================================
# 3. the flow restatement blows up from rest: the run the driver test of tests/test_gpu_nonfinite.py repeats on the device
# ======================================================================================================================
@pytest.mark.parametrize("smoother,omega", [("jacobi", 0.8), ("rbgs", 1.0)])
def test_flow_restatement_blows_up_within_forty_steps(smoother, omega):
    n = 17
    ref = R.Flow(n, n, 1e-3, R.NO_SLIP, (0.0, 0.0, 0.0, 1.0), solver=R.CycleSolver(n, n, tol=1e-10, max_cycles=4, smoother=smoother, omega=omega))
    ref.set_state(np.zeros((n, n)))
    first = None
    with np.errstate(all="ignore"):
        for k in range(1, 41):
            info = ref.step(0.5)
            finite = math.isfinite(info["omega_change"]) and math.isfinite(info["cfl"])
            if first is None and not finite:
                first = k
            if first is not None and k >= first + 3:                                # three steps on every interior cell is NaN
                assert math.isnan(info["omega_change"]) and math.isnan(info["cfl"]) and math.isnan(info["rhs_norm"]), k
                assert not info["omega"]["converged"] and not info["psi"]["converged"] and info["omega"]["cycles"] == 4, k
                if k >= first + 5:
                    break                                                          # NaN stays NaN: no need to walk to step 40
    print("first non-finite step", first)
    assert first is not None and first <= 40
    assert np.isnan(ref.w[1:-1, 1:-1]).all() and np.isnan(ref.psi[1:-1, 1:-1]).all()
    # what a maximum formed with fmax reports for that state: a fluid at rest
    p = R._nb(ref.psi)
    assert float(np.fmax.reduce((np.abs(p["N"] - p["S"]) + np.abs(p["E"] - p["W"])).ravel(), initial=0.0)) == 0.0
    assert math.isnan(R.velocity_max(ref.psi))
