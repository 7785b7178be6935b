"""Case tables and helpers for the handle-bound entry points of include/mghip.h (every function that takes an mg_handle):
what tests/test_gpu_handle_calls.py runs on a device and tests/test_handle_calls_cpu.py checks for completeness.  Plain
Python + NumPy; torch and the engine are imported where a case runs, nothing here touches a GPU by itself.

A case is a dict with an "id", the part of the suite it belongs to ("part": A .. F), the entry points it exercises
("calls") and its residual-norm comparisons ("norms").  A norm comparison names how the SUBJECT handle and the REFERENCE
handle (a fresh one, made for the comparison) received their right-hand side -- "host" (mg_set_rhs) or "device"
(mg_set_rhs_device) --, whether mg_update_rhs_device is part of the sequence, and "loose": compared within NORM_RTOL
instead of exactly.  The rule (norm_is_loose) is checked by the CPU test:

  exact   both handles received their right-hand side through the same kind of entry point, no mg_update_rhs_device:
          the same kernels sum the same cells in the same order;
  loose   otherwise: after mg_set_rhs_device / mg_update_rhs_device the ring sum is unknown, the norm takes the
          full-residual kernel instead of the up leg's partial sums (other tiles: last-bit differences), NORM_RTOL is the
          project's bound for sums of r^2 taken over other tiles;
  loose   (part E only) after mg_time_op(op 6, a whole cycle) on a fused handle: its up leg leaves partial sums, the
          fresh handle that is loaded with the same iterate sums r^2 with the full-residual kernel.
"""
import os
import re

import numpy as np

import dev_call_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mghip.h")
NORM_RTOL = 1e-12
MG_F32, MG_F64 = 0, 1
JACOBI, RBGS = 0, 1
ERR_INVALID, ERR_STATE = -1, -4

# ---- precision policies -----------------------------------------------------------------------------------------------
# name -> (mg_precision_t, engine keywords, working precision set through mg_set_working_precision or None)
POLICIES = {
    "double": (0, {}, None),
    "single": (1, {}, None),
    "single_managed": (4, {}, None),
    "mixed": (2, {}, None),
    "mixed_split2": (2, {"mixed_split": 2}, None),
    "adaptive_f64": (3, {}, None),
    "adaptive_f32": (3, {}, "f32"),
    "defect": (5, {}, None),
}
POLICY_CODES = {"double": 0, "single": 1, "mixed": 2, "adaptive": 3, "single_managed": 4, "defect": 5}     # mg_precision_t
DTYPES = ["f32", "f64"]
PITCHES = ["lib", "min", "lib+16"]

# ---- shapes: the smallest at which each mechanism exists ----------------------------------------------------------------
# (nx, ny, domain, max_levels)
SHAPES = {
    "129x65": (129, 65, (0.0, 2.0, 0.0, 1.0), 5),      # ends in 9 x 5: served by the LDS tail
    "257": (257, 257, (0.0, 1.0, 0.0, 1.0), 7),        # register tail 65^2 .. 5^2
    "33L2": (33, 33, (0.0, 1.0, 0.0, 1.0), 2),         # no tail, the coarse level is the coarsest
    "1281": (1281, 1281, (0.0, 1.0, 0.0, 1.0), 9),     # above 1100^2 cells: register-blocked legs, spanning leg, third buffer
    "2049x641": (2049, 641, (0.0, 1.0, 0.0, 1.0), 8),
}
SMOOTHERS = {"VJ": ("V", JACOBI, 0.8), "WR": ("W", RBGS, 1.0), "VR": ("V", RBGS, 1.0), "WJ": ("W", JACOBI, 0.8)}


def pitch(kind, dt, ny):
    """row pitch in elements: the library's, the least legal one (ny rounded up to 16 bytes), the library's + 16 elements"""
    if kind == "lib+16":
        return G.pitch("lib", dt, ny) + 16
    return G.pitch(kind, dt, ny)


def engine_kwargs(shape, smoother, policy, **extra):
    """(nx, ny, keywords) of MultigridEngine for a case"""
    nx, ny, domain, levels = SHAPES[shape]
    cyc, sm, omega = SMOOTHERS[smoother]
    code, pkw, _ = POLICIES[policy]
    kw = dict(domain=domain, max_levels=levels, cycle=cyc, smoother=sm, omega=omega, precision=code, coarse_maxit=60, tail=1)
    kw.update(pkw)
    kw.update(extra)
    return nx, ny, kw


def fields(shape, seed, n_rhs=1):
    """right-hand sides (one fixed random ring + a new random interior each) and an initial guess, all with a random non-zero
    boundary ring"""
    nx, ny = SHAPES[shape][:2]
    rng = np.random.default_rng(seed)
    ring = rng.standard_normal((nx, ny))
    rhs = []
    for _ in range(n_rhs):
        f = ring.copy()
        f[1:-1, 1:-1] = rng.standard_normal((nx - 2, ny - 2))
        rhs.append(f)
    u0 = rng.standard_normal((nx, ny))
    return rhs, u0


def coefficient(shape, seed):
    nx, ny = SHAPES[shape][:2]
    return np.exp(0.5 * np.random.default_rng(seed).standard_normal((nx, ny)))


# ---- caller-side device arrays: built like those of dev_call_cases (GUARD rows, NaN sentinel in guards and pad columns) ----
def dev_array(device, dt, nx, ny, pitch_kind, data=None):
    """a G.Arr: (GUARD + nx + GUARD, ld) tensor, sentinel everywhere but the (nx, ny) field when `data` is given (cast once
    with astype: the rounding NumPy does)"""
    import torch
    ld = pitch(pitch_kind, dt, ny)
    host = G.sentinel(G.NPDT[dt], (nx + 2 * G.GUARD, ld))
    if data is not None:
        host[G.GUARD:G.GUARD + nx, :ny] = np.asarray(data).astype(G.NPDT[dt])
    return G.Arr(torch, device, host, nx, ny, ld)


def field_of(arr):
    """the (nx, ny) field of a device array after a call.  Guard rows must still hold the sentinel; pad columns are exempt,
    as for every output of the mg_dev_convert cases (dev_call_cases.compare_array)."""
    full = arr.host()
    gb = G.bits(full)
    guards = np.ones(gb.shape[0], dtype=bool)
    guards[G.GUARD:G.GUARD + arr.nx] = False
    bad = gb[guards] != G.SENT_BITS[full.dtype.itemsize]
    assert not bad.any(), "%d guard cells overwritten" % int(bad.sum())
    return full[G.GUARD:G.GUARD + arr.nx, :arr.ny].copy()


def norms_agree(got, ref, loose):
    if loose:
        return abs(got - ref) <= NORM_RTOL * abs(ref)
    return got == ref


def norm_is_loose(part, subject, reference, update, time_op_cycle=False):
    """the rule of the module docstring"""
    return subject != reference or bool(update) or (part == "E" and time_op_cycle)


def _norm(part, name, subject, reference, update=False, time_op_cycle=False):
    return dict(name=name, subject=subject, reference=reference, update=update, time_op_cycle=time_op_cycle,
                loose=norm_is_loose(part, subject, reference, update, time_op_cycle))


def norm_of(case, name):
    return next(n for n in case["norms"] if n["name"] == name)


# ======================================================================================================================
# A. device forms equal host forms
# ======================================================================================================================
A_CALLS = ["mg_set_rhs_device", "mg_zero_solution_device", "mg_get_solution_device", "mg_cycle", "mg_set_rhs", "mg_set_solution",
           "mg_get_solution", "mg_residual_norm", "mg_num_levels", "mg_level_shape"]


def cases_a():
    out = []
    for policy in POLICIES:
        for shape, smoother in (("129x65", "VJ"), ("129x65", "WR"), ("257", "VJ"), ("257", "WR")):
            calls = A_CALLS + (["mg_set_working_precision"] if policy.startswith("adaptive") else [])
            out.append(dict(part="A", id="%s-%s-%s" % (policy, shape, smoother), policy=policy, shape=shape, smoother=smoother,
                            dtypes=DTYPES, pitches=PITCHES, large=False, calls=calls,
                            norms=[_norm("A", "zero_same_kind", "device", "device"), _norm("A", "zero_host", "device", "host")]))
    for policy in ("double", "single_managed"):
        for shape in ("1281", "2049x641"):
            out.append(dict(part="A", id="%s-%s-VJ-iterate" % (policy, shape), policy=policy, shape=shape, smoother="VJ",
                            dtypes=["f64" if policy == "double" else "f32"], pitches=["min"], large=True,
                            calls=A_CALLS + ["mg_iterate"], norms=[_norm("A", "history", "device", "host")]))
    return out


# the oracle anchor: one case per precision policy at 129 x 65 on (0, 2) x (0, 1)
ANCHOR_POLICIES = ["double", "single", "single_managed", "mixed", "adaptive_f64", "defect"]

# ======================================================================================================================
# B. mg_update_rhs_device
# ======================================================================================================================
B_POLICIES = ["double", "single", "single_managed", "mixed_split2"]       # what dist_ops.HipOps.coarse_setup builds
B_CALLS = ["mg_set_rhs_device", "mg_update_rhs_device", "mg_zero_solution_device", "mg_cycle", "mg_get_solution_device"]


def cases_b():
    out = []
    k = 0
    for policy in B_POLICIES:
        for smoother in SMOOTHERS:
            for shape in ("129x65", "257"):
                out.append(dict(part="B", kind="loop", id="%s-%s-%s" % (policy, shape, smoother), policy=policy, shape=shape, smoother=smoother,
                                dt=DTYPES[k % 2], pitch=("min", "lib+16")[(k // 2) % 2], calls=B_CALLS, norms=[]))
                k += 1
    return out


B_EXTRA = [
    dict(part="B", kind="adaptive", id="adaptive-carry", policy="adaptive_f64", dt="f64", calls=B_CALLS + ["mg_set_working_precision"], norms=[]),
    dict(part="B", kind="host_first", id="host-rhs-first", policy="double", dt="f64", calls=["mg_set_rhs", "mg_update_rhs_device", "mg_cycle", "mg_residual_norm"],
         norms=[_norm("B", "after_update", "host", "host", update=True)]),
    dict(part="B", kind="order", id="update-before-any-rhs", calls=["mg_update_rhs_device", "mg_last_error"], norms=[]),
    dict(part="B", kind="plan", id="recorded-plan", calls=B_CALLS + ["mg_set_stream"], norms=[]),
]

# ======================================================================================================================
# C. streams
# ======================================================================================================================
C_CASES = [dict(part="C", id="streams", calls=["mg_set_stream", "mg_get_stream", "mg_synchronize", "mg_set_rhs_device",
                                               "mg_zero_solution_device", "mg_cycle", "mg_get_solution_device"], norms=[])]

# ======================================================================================================================
# D. operator changes leave no trace: host forms, exact norms
# ======================================================================================================================
# a prefix is a list of steps; the final operator is what the last steps leave in force.
#   ("coef", k)  mg_set_coefficient(a_k), k = None: back to the constant operator       ("shift", s)  mg_set_shift(s)
#   ("solve",)   mg_set_solution(NULL) + mg_iterate(0, 2)        ("zero_norm",)  mg_set_solution(NULL) + mg_residual_norm
#   ("fmg",)     mg_set_solution(u0) + mg_fmg(1) + mg_iterate(0, 2)
D_PREFIXES = {
    "coef-solve-const": [("coef", 1), ("solve",), ("coef", None)],
    "coef-solve-coef": [("coef", 1), ("solve",), ("coef", 2)],
    "shift-solve-noshift": [("shift", 0.37), ("solve",), ("shift", 0.0)],
    "shift0.37-solve-shift160": [("shift", 0.37), ("solve",), ("shift", 160.0)],
    "shift160-solve-shift0.37": [("shift", 160.0), ("solve",), ("shift", 0.37)],
    "shift-coef-solve-const": [("shift", 0.37), ("coef", 1), ("solve",), ("coef", None)],
    "zeronorm-const-then-coef": [("zero_norm",), ("coef", 1)],
    "zeronorm-coef-then-const": [("coef", 1), ("zero_norm",), ("coef", None)],
    "fmg-iterate": [("fmg",)],
}
D_SETTINGS = {"iter-tail1": dict(coarse_direct=0, tail=1), "iter-tail2": dict(coarse_direct=0, tail=2),
              "direct-tail1": dict(coarse_direct="auto", tail=1), "direct-tail2": dict(coarse_direct="auto", tail=2)}
D_CALLS = ["mg_set_coefficient", "mg_set_shift", "mg_set_rhs", "mg_set_solution", "mg_get_solution", "mg_iterate", "mg_residual_norm", "mg_fmg"]


def d_prefixes_of(policy):
    """DOUBLE and SINGLE_MANAGED run every prefix, ADAPTIVE those without a coefficient, DEFECT (constant coefficients only,
    and here for the full-multigrid start alone) the last one"""
    if policy == "defect":
        return ["fmg-iterate"]
    if policy.startswith("adaptive"):
        return [k for k, steps in D_PREFIXES.items() if not any(s[0] == "coef" for s in steps)]
    return list(D_PREFIXES)


def final_operator(steps):
    """(coefficient index or None, shift) in force after the steps"""
    coef, shift = None, 0.0
    for s in steps:
        if s[0] == "coef":
            coef = s[1]
        elif s[0] == "shift":
            shift = s[1]
    return coef, shift


def cases_d():
    out = []
    for shape, smoother in (("129x65", "WR"), ("257", "VJ")):
        for policy in ("double", "single_managed", "adaptive_f64", "defect"):
            for setting in D_SETTINGS:
                out.append(dict(part="D", id="%s-%s-%s-%s" % (policy, shape, smoother, setting), policy=policy, shape=shape,
                                smoother=smoother, setting=setting, prefixes=d_prefixes_of(policy), calls=D_CALLS,
                                norms=[_norm("D", "zero_norm", "host", "host"), _norm("D", "history", "host", "host")]))
    return out


# ======================================================================================================================
# E. mg_time_op leaves only what it documents
# ======================================================================================================================
E_OPS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]
E_REWRITES_FINE = (0, 1, 5, 6, 7, 8, 9, 12, 13)       # on level 0 these rewrite the fine iterate (mg_time_op)
E_CALLS = ["mg_time_op", "mg_residual_norm", "mg_get_solution", "mg_set_solution", "mg_set_rhs", "mg_iterate", "mg_num_levels"]


def _e_norms(fused):
    return [_norm("E", "after_op", "host", "host"), _norm("E", "after_op6", "host", "host", time_op_cycle=bool(fused)),
            _norm("E", "history", "host", "host")]


def cases_e():
    out = []
    for shape in ("33L2", "129x65", "257"):
        for fused in (1, 3):
            for tail in (0, 1):
                for policy, smoother in (("double", "VJ"), ("single_managed", "WR")):
                    out.append(dict(part="E", id="%s-fused%d-tail%d-%s-%s" % (shape, fused, tail, policy, smoother), shape=shape, fused=fused,
                                    tail=tail, policy=policy, smoother=smoother, ops=E_OPS, levels=None, extra={}, calls=E_CALLS, norms=_e_norms(fused)))
    for policy, smoother in (("double", "VJ"), ("single_managed", "WR")):      # control: one launch per operator
        out.append(dict(part="E", id="129x65-fused0-%s-%s" % (policy, smoother), shape="129x65", fused=0, tail=0, policy=policy,
                        smoother=smoother, ops=E_OPS, levels=None, extra={}, calls=E_CALLS, norms=_e_norms(0)))
    for smoother in ("VJ", "VR"):      # the span ops: speculate = 2, Jacobi (served) and red-black (mg_time_op refuses, and must leave nothing)
        out.append(dict(part="E", id="1281-span-%s" % smoother, shape="1281", fused=2, tail=1, policy="double", smoother=smoother,
                        ops=[12, 13], levels=[0], extra=dict(speculate=2), calls=E_CALLS, norms=_e_norms(2)))
    return out


E_HBM = dict(part="E", id="hbm-ops-10-11", shape="129x65", calls=["mg_time_op"], norms=[])     # > 768 MiB each by design: once, level 0

E_ZERO = dict(part="E", id="zero-guess-level-0", shape="129x65", calls=["mg_time_op", "mg_set_solution", "mg_residual_norm"], norms=[])

# ======================================================================================================================
# F. small contracts
# ======================================================================================================================
F_CASES = [
    dict(part="F", id="before-any-rhs", calls=["mg_cycle", "mg_fmg", "mg_residual_norm", "mg_iterate", "mg_last_error"], norms=[]),
    dict(part="F", id="device-forms-bad-arguments", calls=["mg_set_rhs_device", "mg_update_rhs_device", "mg_get_solution_device",
                                                           "mg_get_solution", "mg_last_error"], norms=[]),
    dict(part="F", id="working-precision-fixed", calls=["mg_set_working_precision"], norms=[]),
    dict(part="F", id="defect-refuses-coefficient", calls=["mg_set_coefficient", "mg_solve"], norms=[]),
    dict(part="F", id="bad-shift", calls=["mg_set_shift", "mg_solve"], norms=[]),
    dict(part="F", id="profile", calls=["mg_level_timings", "mg_iterate", "mg_set_rhs", "mg_set_solution", "mg_get_solution"],
         norms=[_norm("F", "history", "host", "host")]),
]

# entry points no case needs to name, each with its reason
EXEMPT = {
    "mg_destroy": "implied by every case: every handle a case creates is destroyed (MultigridEngine.close)",
}
IMPLIED = {"mg_create": "implied by every case (not a handle-first function: it returns the handle)"}


def all_cases():
    return cases_a() + cases_b() + B_EXTRA + C_CASES + cases_d() + cases_e() + [E_HBM, E_ZERO] + F_CASES


def handle_functions(header=HEADER):
    """names of the functions of include/mghip.h whose first parameter is `mg_handle*` or `const mg_handle*`"""
    text = open(header).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mg_\w+)\s*\(\s*(?:const\s+)?mg_handle\s*\*", text)))
