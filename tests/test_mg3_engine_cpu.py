"""The CPU half of the 3-D engine's tests (tests/test_gpu_mg3_engine.py and tests/test_gpu_mg3_special.py are the GPU halves): the
case tables of tests/mg3_engine_cases.py are complete (every handle function of the header, every field of mg3_config), the
hierarchy shapes build the levels and take the coarsest path they are chosen for, every knob case is observable on the
restatement, a missed invalidation of the cached fp32 residual cannot hide inside a tolerance, the restatement's solve loop never
stops on a NaN norm, and the special-value cases do on the restatement what they are chosen for."""
import math
import re

import numpy as np
import pytest

import mg3_engine_cases as K
import mg3_reference as R
import special_values as S


# ------------------------------------------------------------------------------------------ completeness
def test_every_handle_function_is_named_by_a_case():
    text = open(K.HEADER).read()
    declared = re.findall(r"^(?:int|const char\*)\s+(mg3_\w+)\(([^;]*)\);", text, flags=re.M | re.S)
    takes_handle = {name for name, args in declared if "mg3_handle" in args}
    assert {"mg3_create", "mg3_destroy", "mg3_solve", "mg3_stream", "mg3_set_rhs_device", "mg3_last_error"} <= takes_handle
    assert len(takes_handle) == 16, sorted(takes_handle)
    named = {e for entries in K.COVERAGE.values() for e in entries}
    assert takes_handle <= named, sorted(takes_handle - named)
    assert named <= {name for name, _ in declared}, sorted(named - {name for name, _ in declared})
    for name, case in K.SEQUENCES.items():
        assert case["stale"] is None or case["stale"] in K.COVERAGE[name], name
    # the six mutators: a missed invalidation in each is modelled by some sequence
    assert {c["stale"] for c in K.SEQUENCES.values()} - {None} == {"mg3_set_rhs", "mg3_set_rhs_device", "mg3_set_solution",
                                                                   "mg3_set_solution_device", "mg3_zero_solution", "mg3_cycle"}


def test_every_config_field_is_moved_off_its_default():
    text = open(K.HEADER).read()
    body = re.search(r"typedef struct mg3_config \{(.*?)\} mg3_config;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in decl.split(",")]
    assert len(fields) == 20 and "coarse_sweeps" in fields and "z1" in fields, fields
    assert set(fields) - {"device", "reserved"} == K.config_fields_moved(), set(fields) ^ K.config_fields_moved()


# ------------------------------------------------------------------------------------------ hierarchies
@pytest.mark.parametrize("name", list(K.HIERARCHIES))
def test_hierarchy_table(name):
    case = K.HIERARCHIES[name]
    levels = R.hierarchy(case["shape"], case["max_levels"])
    assert levels == case["levels"]
    assert ("lds" if max(levels[-1]) <= K.LDS_EXTENT else "colour") == case["coarsest"]
    assert np.prod(case["shape"]) < 40000


def test_hierarchy_table_holds_each_mechanism():
    H = K.HIERARCHIES
    assert K.LDS_EXTENT == 17 and K.T3I == 32
    single = [n for n, c in H.items() if len(c["levels"]) == 1]
    assert {H[n]["coarsest"] for n in single} == {"lds", "colour"}
    assert H["17L1"]["levels"] == [(K.LDS_EXTENT,) * 3] and H["33L2"]["levels"][-1] == (K.LDS_EXTENT,) * 3
    # 2 * 17^3 fp64 values are above the 64 KiB a kernel gets without asking for more dynamic LDS
    assert 2 * K.LDS_EXTENT ** 3 * 8 == 78608 > 65536
    # stopped by max_levels although the coarsest could be coarsened; stopped by an even extent with levels to spare
    for n in ("33L2", "9L2"):
        assert len(H[n]["levels"]) == H[n]["max_levels"] and all(e % 2 == 1 and e >= 5 for e in H[n]["levels"][-1])
    assert len(H["9x9x35"]["levels"]) < H["9x9x35"]["max_levels"] and any(e % 2 == 0 for e in H["9x9x35"]["levels"][-1])
    assert min(H["9x9x35"]["levels"][-1]) >= 5
    # more than one chunk of kT3I interior planes along i on the fine level, and only there
    chunks = {n: -(-(c["shape"][0] - 2) // K.T3I) for n, c in H.items()}
    assert chunks["37x5x5"] == 2 and [n for n, v in chunks.items() if v > 1] == ["37x5x5"]
    hx, hy, hz = R.spacings(H["9x17x33"]["shape"], H["9x17x33"]["domain"])
    assert hx == hy == hz


# ------------------------------------------------------------------------------------------ knobs
@pytest.fixture(scope="module")
def base_runs():
    return {name: K.run_cycles(kw, "single", K.KNOB_CYCLES) for name, kw in K.knob_bases()}


@pytest.mark.parametrize("name,base,changed", K.knob_cases(), ids=[c[0] for c in K.knob_cases()])
def test_knob_case_is_observable(base_runs, name, base, changed):
    """two fp32 cycles with the change against two on the base: an engine that ignored the knob would be off by ten times the
    fp32 tolerance at least"""
    assert [k for k, v in changed.items() if base.get(k) != v] in ([k] for k in changed) or name.endswith("pre3post1")   # one change away
    want = base_runs["-".join(name.split("-")[:2]) + "-base"][-1][0]
    got = K.run_cycles(changed, "single", K.KNOB_CYCLES)[-1][0]
    moved = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)))) / float(np.max(np.abs(want)))
    print(name, "moves the fp32 iterate by", moved)
    assert moved >= K.SENSITIVITY


def test_default_coarse_sweeps_would_hide_the_knob():
    """why the bases do not use the default: at 9^3 with the default levels the coarsest grid has one interior cell, which one
    sweep solves"""
    f, u0 = K.problem((9, 9, 9))
    out = [K.run_cycles(dict(shape=(9, 9, 9), coarse_sweeps=cs), "single", 2, f, u0)[-1][0] for cs in (1, 3, 64)]
    assert out[0].tobytes() == out[1].tobytes() == out[2].tobytes()
    assert K.ref_config(dict(coarse_sweeps=0)).coarse_sweeps == 64 and K.ref_config(dict(coarse_sweeps=-5)).coarse_sweeps == 64
    assert K.ref_config(dict(coarse_sweeps=2)).coarse_sweeps == 2


# ------------------------------------------------------------------------------------------ cached state
def test_simulate_is_the_restatement():
    kw = dict(K.SEQUENCE_BASE, smoother="rbgs")
    fields = K.sequence_fields(kw["shape"])
    cfg = K.ref_config(kw)
    (f1, u1), (f2, u2) = fields[1], fields[2]
    out = K.simulate(K.SEQUENCES["norm-set_rhs-cycle"]["steps"], fields, kw, "defect")
    assert out["u"].tobytes() == R.defect_step(u1, f2, cfg).tobytes() and out["norms"] == [R.residual_norm(u1, f1, cfg)]
    assert out["before_last_cycle"].tobytes() == u1.tobytes() and out["f"].tobytes() == f2.tobytes()
    out = K.simulate(K.PARTNER_SEQUENCES["zero_solution"], fields, kw, "single")
    assert out["u"].tobytes() == R.cycle(np.zeros(kw["shape"], np.float32), f1.astype(np.float32), cfg).tobytes()
    out = K.simulate(K.SEQUENCES["norm-set_solution_device32-cycle"]["steps"], fields, kw, "defect")
    assert out["before_last_cycle"].tobytes() == u2.astype(np.float32).astype(np.float64).tobytes()


@pytest.mark.parametrize("smoother", K.SMOOTHERS)
@pytest.mark.parametrize("name", [n for n, c in K.SEQUENCES.items() if c["stale"]])
def test_a_missed_invalidation_cannot_hide_in_a_tolerance(name, smoother):
    """the defect step taken with the residual of the old f or the old u, against the right one"""
    kw = dict(K.SEQUENCE_BASE, smoother=smoother)
    fields = K.sequence_fields(kw["shape"])
    steps = K.SEQUENCES[name]["steps"]
    right, wrong = (K.simulate(steps, fields, kw, "defect", stale=s)["u"] for s in (False, True))
    gap = float(np.max(np.abs(right - wrong))) / float(np.max(np.abs(right)))
    print(name, smoother, "stale outcome differs by", gap)
    assert gap >= K.STALE_GAP


@pytest.mark.parametrize("name", [n for n, c in K.SEQUENCES.items() if not c["stale"]])
def test_sequences_without_a_mutator_have_nothing_to_invalidate(name):
    kw = dict(K.SEQUENCE_BASE, smoother="jacobi")
    fields = K.sequence_fields(kw["shape"])
    right, wrong = (K.simulate(K.SEQUENCES[name]["steps"], fields, kw, "defect", stale=s) for s in (False, True))
    assert right["u"].tobytes() == wrong["u"].tobytes() and right["norms"] == wrong["norms"]


@pytest.mark.parametrize("sweeps", K.PARTNER_SWEEPS)
def test_partner_sequences_end_on_the_second_iterates_faces(sweeps):
    """the restatement of part d: the faces after the last cycle are those of the iterate set last, and the two iterates' faces
    differ in every cell, so a partner buffer with stale faces shows"""
    kw = dict(K.HIERARCHIES["9L2"], smoother="jacobi", pre=sweeps[0], post=sweeps[1], coarse_sweeps=3)
    kw = {k: v for k, v in kw.items() if k not in ("levels", "coarsest")}
    fields = K.sequence_fields(kw["shape"])
    face = np.ones(kw["shape"], dtype=bool)
    face[R.INT] = False
    assert np.all(fields[1][1][face] != fields[2][1][face]) and np.all(fields[2][1][face] != 0)
    out = K.simulate(K.PARTNER_SEQUENCES["set_solution"], fields, kw, "double")
    assert out["u"][face].tobytes() == fields[2][1][face].tobytes()
    assert out["u"].tobytes() == R.cycle(fields[2][1], fields[1][0], K.ref_config(kw)).tobytes()


# ------------------------------------------------------------------------------------------ the stop rule
def test_solve_with_a_nan_cell_runs_every_cycle_and_never_converges():
    kw = dict(shape=K.HIERARCHIES["9L2"]["shape"], max_levels=2, smoother="rbgs")
    f, u0 = K.problem(kw["shape"])
    f[4, 4, 4] = np.nan
    with np.errstate(all="ignore"):
        u, hist, conv = R.solve(u0, f, K.ref_config(kw), 1e-3, 3)
    assert len(hist) == 4 and all(math.isnan(v) for v in hist) and not conv
    with np.errstate(all="ignore"):
        u, hist, conv = R.solve(u0, f, K.ref_config(kw), math.inf, 3)
    assert len(hist) == 4 and not conv                      # NaN < +inf is false too


# ------------------------------------------------------------------------------------------ special values
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_plant_positions(dtype):
    tk = K.tile_k(dtype)
    big, small = K.special_sweep_shapes(dtype)
    assert big == (35, 18, tk + 2) and small == (5, 5, 5)
    # two workgroups of mg3_sweep_kernel on every axis
    assert -(-(big[0] - 2) // K.T3I) == 2 and -(-big[1] // K.T3J) == 2 and -(-big[2] // tk) == 2
    pos = dict(K.plant_positions(big, dtype))
    assert len(pos) == 18 and len(set(pos.values())) == 18
    assert pos["i_tile0_last"][0] == K.T3I and pos["i_tile1_first"][0] == K.T3I + 1
    assert pos["j_tile0_last"][1] == K.T3J - 1 and pos["j_tile1_first"][1] == K.T3J
    assert pos["k_tile0_last"][2] == tk - 1 and pos["k_tile1_first"][2] == tk
    kinds = {n: (K.is_interior(p, big), K.is_pad(p, big), K.is_corner(p, big)) for n, p in pos.items()}
    assert sum(k[0] for k in kinds.values()) == 9 and kinds["pad"] == (False, True, False)
    assert [n for n, k in kinds.items() if k[2]] == ["corner_lo", "corner_hi"]
    faces = [p for n, p in pos.items() if n.startswith("face_")]
    assert len(faces) == 6 and all(sum(x in (0, m - 1) for x, m in zip(p, big)) == 1 for p in faces)
    for shape in [small] + K.SPECIAL_TRANSFER_SHAPES:
        names = [n for n, _ in K.plant_positions(shape, dtype)]
        assert {"first", "last", "face_i0", "face_k1", "corner_lo", "corner_hi", "pad"} <= set(names)
    assert len(S.VALUES) == 3 and math.isnan(S.VALUES[0]) and S.VALUES[1:] == (math.inf, -math.inf)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_subnormal_scale_gives_subnormal_results(dtype):
    """the restatement's outputs at the scale the GPU test uses are subnormal and not all zero: a kernel that flushed would differ"""
    shape = K.special_sweep_shapes(dtype)[1]
    s = K.SUBNORMAL_SCALE[np.dtype(dtype)]
    rng = np.random.default_rng(61)
    u, f = (rng.standard_normal(shape) * s).astype(dtype), (rng.standard_normal(shape) * s).astype(dtype)
    assert np.all(S.is_subnormal(u) | (u == 0)) and np.count_nonzero(u) > u.size // 2
    h, sigma, omega = K.SPECIAL_H, K.SPECIAL_SIGMA, K.SPECIAL_OMEGA
    outs = {"jacobi": R.jacobi(u, f, h, sigma, omega)[R.INT], "residual": R.residual(u, f, h, sigma)[R.INT],
            "colour": R.colour_pass(u, f, h, sigma, omega, 0)[R.INT], "restrict": R.restrict(u)[R.INT],
            "prolong": R.prolong_add(u, R.restrict(u))[R.INT], "coarse": R.coarse_solve(u, f, h, sigma, 2)[R.INT]}
    for name, out in outs.items():
        sub = S.is_subnormal(out)
        print(np.dtype(dtype).name, name, "subnormal cells", int(sub.sum()), "of", out.size, "zeros", int((out == 0).sum()))
        assert np.all(sub | (out == 0)), name
        assert sub.sum() > out.size // 2, name


def test_huge_fp32_residual_squares_overflow_fp32_only():
    shape = K.special_sweep_shapes(np.float32)[1]
    rng = np.random.default_rng(62)
    u, f = ((rng.standard_normal(shape) * K.HUGE_F32_SCALE).astype(np.float32) for _ in range(2))
    r = R.residual(u, f, K.SPECIAL_H, K.SPECIAL_SIGMA)[R.INT]
    assert np.all(np.isfinite(r))
    with np.errstate(over="ignore"):
        assert np.all(np.isinf(r * r))
    assert math.isfinite(R.sumsq(r)) and R.sumsq(r) > float(np.finfo(np.float32).max)
