"""Case tables for the 3-D engine's tests -- not a test.  Plain Python and NumPy.

HIERARCHIES: the smallest shapes at which each mechanism of mg3_handle's hierarchy exists (single level, the colour-kernel coarsest
solve, the LDS solve at its limit extent, a stop on max_levels or on an even extent, two i-chunks on the fine level).
KNOB_CASES: one change of one mg3_config field away from a base whose coarsest solve is NOT converged, so that every field is
observable; tests/test_mg3_engine_cpu.py checks that each change moves the restatement's iterate by >= SENSITIVITY.
SEQUENCES: lists of handle calls over two right-hand sides and two iterates, with `simulate`, their NumPy model on the restatement
tests/mg3_reference.py (stale=True models a handle that never invalidates its cached fp32 residual).
COVERAGE: case id -> the mg3_* entry points it exercises.  plant_positions / SPECIAL_*: where and what the special-value tests of
the mg3_dev_* kernels plant.  tests/test_gpu_mg3_engine.py and tests/test_gpu_mg3_special.py run the tables on the device."""
import os
import re

import numpy as np

import mg3_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mghip_3d.h")
KERNELS = os.path.join(ROOT, "mixed_precision_multigrid_solvers_for_pdes_amd", "csrc", "mg_3d_kernels.hpp")


def kernel_constant(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(KERNELS).read()).group(1))


T3J, T3ROW, T3I, LDS_EXTENT = (kernel_constant(n) for n in ("kT3J", "kT3RowBytes", "kT3I", "kCoarseLdsExtent"))
UNIT = (0.0, 1.0, 0.0, 1.0, 0.0, 1.0)
EQUAL_DOMAIN = (0.0, 0.25, 0.0, 0.5, 0.0, 1.0)          # 9 x 17 x 33 with equal spacings
SMOOTHERS = ("jacobi", "rbgs")
PRECISIONS = ("double", "single", "defect")
# tests/test_gpu_mg3.py's own: (iterate relative to max|u|, norm relative)
TOLERANCES = {"double": (1e-13, 1e-12), "defect": (1e-13, 1e-12), "single": (1e-5, 1e-5)}


def work_dtype(precision):
    """the type of the iterate and the right-hand side the caller sees"""
    return np.float32 if precision == "single" else np.float64


# ------------------------------------------------------------------------------------------ hierarchies
# id -> shape, max_levels, domain, the levels the engine must build, the coarsest solve's path
HIERARCHIES = {
    "6x7x10": dict(shape=(6, 7, 10), max_levels=10, domain=UNIT, levels=[(6, 7, 10)], coarsest="lds"),
    "4x5x18": dict(shape=(4, 5, 18), max_levels=10, domain=UNIT, levels=[(4, 5, 18)], coarsest="colour"),
    "17L1": dict(shape=(17, 17, 17), max_levels=1, domain=UNIT, levels=[(17, 17, 17)], coarsest="lds"),
    "33L2": dict(shape=(33, 33, 33), max_levels=2, domain=UNIT, levels=[(33, 33, 33), (17, 17, 17)], coarsest="lds"),
    "9L2": dict(shape=(9, 9, 9), max_levels=2, domain=UNIT, levels=[(9, 9, 9), (5, 5, 5)], coarsest="lds"),
    "5x5x35": dict(shape=(5, 5, 35), max_levels=10, domain=UNIT, levels=[(5, 5, 35), (3, 3, 18)], coarsest="colour"),
    "9x9x35": dict(shape=(9, 9, 35), max_levels=10, domain=UNIT, levels=[(9, 9, 35), (5, 5, 18)], coarsest="colour"),
    "37x5x5": dict(shape=(37, 5, 5), max_levels=10, domain=UNIT, levels=[(37, 5, 5), (19, 3, 3)], coarsest="colour"),
    "9x17x33": dict(shape=(9, 17, 33), max_levels=10, domain=EQUAL_DOMAIN, levels=[(9, 17, 33), (5, 9, 17), (3, 5, 9)], coarsest="lds"),
}
# part a runs each hierarchy with these two configurations
HIERARCHY_CYCLES = (dict(cycle="V", smoother="jacobi"), dict(cycle="W", smoother="rbgs"))
HIERARCHY_COARSE_SWEEPS = 3


def problem(shape, seed=5):
    """(f, u0): standard-normal fp64 fields; u0's faces are random and non-zero like its interior"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape), rng.standard_normal(shape)


def engine_kwargs(kw):
    """the keywords of Multigrid3DEngine among a case's (everything but the shape)"""
    return {k: v for k, v in kw.items() if k != "shape"}


def ref_config(kw):
    """the restatement's Config of a case; mg3_config's `coarse_sweeps <= 0: the default, 64` is resolved here"""
    args = {k: v for k, v in kw.items() if k not in ("shape", "precision")}
    if args.get("coarse_sweeps", 64) <= 0:
        args["coarse_sweeps"] = 64
    return R.Config(**args)


# ------------------------------------------------------------------------------------------ knobs
KNOB_BASES = {
    "9L2": dict(shape=(9, 9, 9), max_levels=2, coarse_sweeps=1),
    "5x5x35": dict(shape=(5, 5, 35), max_levels=10, coarse_sweeps=2),
}
SENSITIVITY = 1e-4              # ten times the fp32 tolerance: what a change must move the fp32 iterate by after two cycles
KNOB_CYCLES = 2


def _changes(base_id, base, smoother):
    out = [("pre0", dict(pre=0)), ("post0", dict(post=0)), ("pre3post1", dict(pre=3, post=1)),
           ("omega", dict(omega=0.6 if smoother == "jacobi" else 1.15)),
           ("cs+2", dict(coarse_sweeps=base["coarse_sweeps"] + 2)), ("cs0", dict(coarse_sweeps=0)), ("cs-5", dict(coarse_sweeps=-5)),
           ("sigma3", dict(sigma=3.0)), ("W", dict(cycle="W")), ("domain", dict(domain=(-1.0, 1.0, 0.5, 2.5, 3.0, 5.0)))]
    if base_id == "9L2":
        out.append(("levels10", dict(max_levels=10)))
    return out


def knob_cases():
    """[(id, base keywords, changed keywords)]: every change on every base for both smoothers; the keywords hold the shape and
    everything Multigrid3DEngine / R.Config take but the precision"""
    out = []
    for base_id, base in KNOB_BASES.items():
        for smoother in SMOOTHERS:
            b = dict(base, smoother=smoother)
            for name, change in _changes(base_id, base, smoother):
                out.append(("%s-%s-%s" % (base_id, smoother, name), b, dict(b, **change)))
    return out


def knob_bases():
    return [("%s-%s-base" % (base_id, smoother), dict(base, smoother=smoother)) for base_id, base in KNOB_BASES.items()
            for smoother in SMOOTHERS]


def run_cycles(kw, precision, cycles, f=None, u0=None):
    """the restatement's iterates and norms after each of `cycles` cycles of case `kw` in `precision` -> [(u, norm)]"""
    if f is None:
        f, u0 = problem(kw["shape"])
    dtype = work_dtype(precision)
    cfg = ref_config(kw)
    u, f = u0.astype(dtype), f.astype(dtype)
    out = []
    for _ in range(cycles):
        u = R.defect_step(u, f, cfg) if precision == "defect" else R.cycle(u, f, cfg)
        out.append((u, R.residual_norm(u, f, cfg)))
    return out


# ------------------------------------------------------------------------------------------ state sequences
# A step: ("norm",) ("cycle", n) ("zero",) ("get",) ("get_device",) ("set_rhs", form, k) ("set_solution", form, k); k = 1, 2 picks
# one of the two right-hand sides / iterates; form: "host" (fp64), "host32", "device64", "device32"
FORM_DTYPE = {"host": np.float64, "host32": np.float32, "device64": np.float64, "device32": np.float32}
START = [("set_rhs", "host", 1), ("set_solution", "host", 1)]
SEQUENCE_BASE = dict(shape=(9, 9, 9), max_levels=2, coarse_sweeps=3)

# part c, defect precision.  stale: the mutator whose missed invalidation the sequence would show (None: nothing to invalidate)
SEQUENCES = {
    "norm-set_rhs-cycle": dict(steps=START + [("norm",), ("set_rhs", "host", 2), ("cycle", 1)], stale="mg3_set_rhs"),
    "norm-set_rhs_device-cycle": dict(steps=START + [("norm",), ("set_rhs", "device64", 2), ("cycle", 1)], stale="mg3_set_rhs_device"),
    "norm-set_rhs_device32-cycle": dict(steps=START + [("norm",), ("set_rhs", "device32", 2), ("cycle", 1)], stale="mg3_set_rhs_device"),
    "norm-set_solution-cycle": dict(steps=START + [("norm",), ("set_solution", "host", 2), ("cycle", 1)], stale="mg3_set_solution"),
    "norm-set_solution_device-cycle": dict(steps=START + [("norm",), ("set_solution", "device64", 2), ("cycle", 1)],
                                           stale="mg3_set_solution_device"),
    "norm-set_solution_device32-cycle": dict(steps=START + [("norm",), ("set_solution", "device32", 2), ("cycle", 1)],
                                             stale="mg3_set_solution_device"),
    "norm-zero-cycle": dict(steps=START + [("norm",), ("zero",), ("cycle", 1)], stale="mg3_zero_solution"),
    "norm-cycle-cycle": dict(steps=START + [("norm",), ("cycle", 1), ("cycle", 1)], stale="mg3_cycle"),
    "norm-norm-cycle": dict(steps=START + [("norm",), ("norm",), ("cycle", 1)], stale=None),
    "norm-get-cycle": dict(steps=START + [("norm",), ("get",), ("get_device",), ("cycle", 1)], stale=None),
    "cycle-norm-cycle-norm": dict(steps=START + [("cycle", 1), ("norm",), ("cycle", 1), ("norm",)], stale=None, quiet_twin=True),
}
STALE_GAP = 1e-3                # what a missed invalidation must move the iterate by, relative to max|u|

# part d, double and single: the Jacobi partner must carry the faces of the iterate it is given.  (pre, post) odd and even
PARTNER_SWEEPS = ((2, 1), (2, 2))
PARTNER_SHAPES = ("9L2", "6x7x10")
PARTNER_SEQUENCES = {
    "set_solution": START + [("cycle", 1), ("set_solution", "host", 2), ("cycle", 1)],
    "set_solution_device": START + [("cycle", 1), ("set_solution", "device64", 2), ("cycle", 1)],
    "zero_solution": START + [("cycle", 1), ("zero",), ("cycle", 1)],
}


def sequence_fields(shape):
    """two independent right-hand sides and two iterates with different random non-zero faces -> {1: (f1, u1), 2: (f2, u2)}"""
    return {1: problem(shape, 5), 2: problem(shape, 6)}


def step_entry_points(step):
    kind = step[0]
    if kind in ("set_rhs", "set_solution"):
        return ["mg3_" + kind + ("_device" if step[1].startswith("device") else "")]
    return {"norm": ["mg3_residual_norm"], "cycle": ["mg3_cycle"], "zero": ["mg3_zero_solution"], "get": ["mg3_get_solution"],
            "get_device": ["mg3_get_solution_device", "mg3_synchronize"]}[kind]


def simulate(steps, fields, kw, precision, stale=False):
    """The steps on the restatement.  -> dict(u, f: the final fields in the working type; norms: every norm asked for;
    before_last_cycle: the iterate just before the last "cycle" step).  stale=True (defect only): no step ever marks the fp32
    residual of the last norm or cycle as out of date, the defect step goes on using it."""
    dtype = work_dtype(precision)
    cfg = ref_config(kw)
    u = np.zeros(kw["shape"], dtype=dtype)
    f = None
    r32 = None                          # defect: fp32(f - A u) as last evaluated, None when not current
    norms, before = [], None
    h = R.spacings(kw["shape"], cfg.domain)
    for step in steps:
        kind = step[0]
        if kind == "set_rhs":
            f = fields[step[2]][0].astype(FORM_DTYPE[step[1]]).astype(dtype)
        elif kind == "set_solution":
            u = fields[step[2]][1].astype(FORM_DTYPE[step[1]]).astype(dtype)
        elif kind == "zero":
            u = np.zeros_like(u)
        elif kind == "norm":
            norms.append(R.residual_norm(u, f, cfg))
            r32 = R.residual(u, f, h, cfg.sigma).astype(np.float32)
        elif kind == "cycle":
            before = u.copy()
            for _ in range(step[1]):
                if precision != "defect":
                    u = R.cycle(u, f, cfg)
                else:
                    if r32 is None:
                        r32 = R.residual(u, f, h, cfg.sigma).astype(np.float32)
                    u = R.defect_step_with_residual(u, r32, cfg)
                    if not stale:
                        r32 = None
        if kind in ("set_rhs", "set_solution", "zero") and not stale:
            r32 = None
    return dict(u=u, f=f, norms=norms, before_last_cycle=before)


# ------------------------------------------------------------------------------------------ the other GPU cases, by name
SOLVE_CASES = ("solve-tol-met-at-start", "solve-max_iter-0", "solve-short-history", "solve-null-outputs", "solve-tol-inf", "solve-tol-0",
               "solve-refusals", "solve-nan-rhs", "solve-stats", "no-rhs-refusals", "rhs-device-alone")

# case id -> the mg3_* entry points it exercises (tests/test_mg3_engine_cpu.py: every function of the header that takes a handle)
COVERAGE = {name: sorted({"mg3_create", "mg3_destroy"} | {e for s in case["steps"] for e in step_entry_points(s)})
            for name, case in SEQUENCES.items()}
COVERAGE.update({"partner-" + name: sorted({e for s in steps for e in step_entry_points(s)} | {"mg3_get_solution"})
                 for name, steps in PARTNER_SEQUENCES.items()})
COVERAGE.update({name: ["mg3_solve", "mg3_set_rhs", "mg3_set_solution", "mg3_get_solution"] for name in SOLVE_CASES})
COVERAGE["no-rhs-refusals"] = ["mg3_cycle", "mg3_residual_norm", "mg3_solve", "mg3_last_error"]
COVERAGE["rhs-device-alone"] = ["mg3_set_rhs_device", "mg3_cycle", "mg3_residual_norm", "mg3_solve"]
COVERAGE["hierarchies"] = ["mg3_create", "mg3_num_levels", "mg3_set_rhs", "mg3_set_solution", "mg3_cycle", "mg3_get_solution",
                           "mg3_residual_norm", "mg3_solve", "mg3_destroy"]
COVERAGE["two-handles"] = ["mg3_stream", "mg3_cycle", "mg3_get_solution"]
COVERAGE["getters"] = ["mg3_get_solution", "mg3_get_solution_device", "mg3_synchronize", "mg3_cycle"]
COVERAGE["tensor-refusals"] = ["mg3_set_rhs_device", "mg3_set_solution_device", "mg3_get_solution_device", "mg3_last_error"]
COVERAGE["rhs-faces"] = ["mg3_set_rhs", "mg3_set_rhs_device", "mg3_cycle", "mg3_residual_norm"]


def config_fields_moved():
    """the fields of mg3_config some case moves off make_config's default"""
    moved = {"nx", "ny", "nz"}
    names = {"domain": ("x0", "x1", "y0", "y1", "z0", "z1")}
    for kw in [c for _, _, c in knob_cases()] + [dict(max_levels=h["max_levels"], domain=h["domain"]) for h in HIERARCHIES.values()] + \
            list(HIERARCHY_CYCLES) + [dict(precision=p) for p in PRECISIONS]:
        for k, v in kw.items():
            if k == "shape":
                continue
            default = dict(domain=UNIT, sigma=0.0, max_levels=10, cycle="V", pre=2, post=2, smoother="jacobi", omega=None,
                           coarse_sweeps=64, precision="double")[k]
            if v != default:
                moved.update(names.get(k, (k,)))
    return moved


# ------------------------------------------------------------------------------------------ special values (the mg3_dev_* kernels)
def tile_k(dtype):
    return T3ROW // np.dtype(dtype).itemsize


def special_sweep_shapes(dtype):
    """two tiles of mg3_sweep_kernel on every axis, and the smallest grid with more than one interior cell per axis"""
    return [(T3I + 3, T3J + 2, tile_k(dtype) + 2), (5, 5, 5)]


SPECIAL_TRANSFER_SHAPES = [(2 * T3I + 3, 5, 7), (5, 5, 67)]
SPECIAL_H, SPECIAL_SIGMA, SPECIAL_OMEGA = (0.11, 0.13, 0.09), 0.7, 0.8
SENTINEL = 12345.0                      # the finite fill of guard planes and pad columns where NaN is the thing under test
# u and f are scaled by these powers of two so that every result is subnormal (diag ~ 2^8.5, |r| ~ 2^11 |u|); the huge fp32 scale
# makes r^2 overflow fp32 (|r| ~ 2^101) while r itself and the fp64 square stay finite
SUBNORMAL_SCALE = {np.dtype(np.float32): 2.0 ** -141, np.dtype(np.float64): 2.0 ** -1037}
HUGE_F32_SCALE = 2.0 ** 90


def plant_positions(shape, dtype):
    """[(name, (i, j, k))] where a planted value can be lost: first, last and centre interior cell; the last interior cell of the
    first tile and the first of the second along each axis (chunks of kT3I interior planes from i = 1, tiles of kT3J rows and TK
    columns from 0); a non-corner cell of each face; two opposite corners; a pad column (k = nz, outside the array: device only).
    Cells that coincide on a small grid are listed once."""
    nx, ny, nz = shape
    ci, cj, ck = nx // 2, ny // 2, nz // 2
    tk = tile_k(dtype)
    out = [("first", (1, 1, 1)), ("last", (nx - 2, ny - 2, nz - 2)), ("centre", (ci, cj, ck)),
           ("i_tile0_last", (min(T3I, nx - 2), cj, ck)), ("j_tile0_last", (ci, min(T3J - 1, ny - 2), ck)),
           ("k_tile0_last", (ci, cj, min(tk - 1, nz - 2)))]
    if T3I + 1 <= nx - 2:
        out.append(("i_tile1_first", (T3I + 1, cj, ck)))
    if T3J <= ny - 2:
        out.append(("j_tile1_first", (ci, T3J, ck)))
    if tk <= nz - 2:
        out.append(("k_tile1_first", (ci, cj, tk)))
    out += [("face_i0", (0, cj, ck)), ("face_i1", (nx - 1, cj, ck)), ("face_j0", (ci, 0, ck)), ("face_j1", (ci, ny - 1, ck)),
            ("face_k0", (ci, cj, 0)), ("face_k1", (ci, cj, nz - 1)), ("corner_lo", (0, 0, 0)), ("corner_hi", (nx - 1, ny - 1, nz - 1)),
            ("pad", (ci, cj, nz))]
    seen, uniq = set(), []
    for name, p in out:
        if p not in seen:
            seen.add(p)
            uniq.append((name, p))
    return uniq


def is_interior(p, shape):
    return all(1 <= x <= n - 2 for x, n in zip(p, shape))


def is_pad(p, shape):
    return p[2] >= shape[2]


def is_corner(p, shape):
    return all(x in (0, n - 1) for x, n in zip(p, shape))
