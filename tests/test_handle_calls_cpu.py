"""Completeness of tests/handle_call_cases.py, without a GPU: every handle-bound function of include/mghip.h is named by a
case (or exempted with a reason), parts A and B cover the precision policies and both caller dtypes, and the looser norm
bound is used exactly where the rule allows it.  This is what keeps tests/test_gpu_handle_calls.py complete when the ABI
grows."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handle_call_cases as H  # noqa: E402


def test_header_parse_finds_the_handle_functions():
    fns = H.handle_functions()
    for name in ("mg_set_rhs_device", "mg_update_rhs_device", "mg_zero_solution_device", "mg_get_solution_device", "mg_set_stream",
                 "mg_get_stream", "mg_time_op", "mg_last_error", "mg_num_levels", "mg_destroy", "mg_solve", "mg_iterate"):
        assert name in fns, name
    assert "mg_create" not in fns and not any(f.startswith(("mg_dev_", "mg_op_", "mg_plan_", "mg_comm_")) for f in fns)
    assert len(fns) >= 24


def test_every_handle_function_is_named_by_a_case_or_exempt():
    named = set()
    for case in H.all_cases():
        assert case["calls"], case["id"]
        named.update(case["calls"])
    fns = set(H.handle_functions())
    assert named <= fns, "cases name functions the header does not declare: %s" % sorted(named - fns)
    missing = fns - named - set(H.EXEMPT)
    assert not missing, "handle functions of include/mghip.h without a case in tests/handle_call_cases.py: %s" % sorted(missing)
    assert not (set(H.EXEMPT) & named), "exempt and named at once"
    assert len(H.EXEMPT) <= 2 and all(len(reason) > 20 for reason in H.EXEMPT.values())


def test_case_ids_are_unique_per_part():
    seen = set()
    for case in H.all_cases():
        key = (case["part"], case["id"])
        assert key not in seen, key
        seen.add(key)
    assert {c["part"] for c in H.all_cases()} == set("ABCDEF")


def _policy_code(case):
    return H.POLICIES[case["policy"]][0]


def test_parts_a_and_b_cover_the_precision_policies_and_both_dtypes():
    a = H.cases_a()
    assert {_policy_code(c) for c in a} == set(H.POLICY_CODES.values())
    assert {dt for c in a for dt in c["dtypes"]} == {"f32", "f64"}
    assert {p for c in a for p in c["pitches"]} == set(H.PITCHES)
    for policy in H.POLICIES:                          # every policy variant on both shapes, both dtypes, all pitches
        mine = [c for c in a if c["policy"] == policy and not c["large"]]
        assert {c["shape"] for c in mine} == {"129x65", "257"} and {c["smoother"] for c in mine} == {"VJ", "WR"}
        assert all(c["dtypes"] == H.DTYPES and c["pitches"] == H.PITCHES for c in mine)
    assert {(c["policy"], c["shape"]) for c in a if c["large"]} == {(p, s) for p in ("double", "single_managed") for s in ("1281", "2049x641")}
    assert set(H.ANCHOR_POLICIES) <= set(H.POLICIES) and {H.POLICIES[p][0] for p in H.ANCHOR_POLICIES} == set(H.POLICY_CODES.values())
    # B: what the replicated coarse engine is built with (dist_ops.HipOps.coarse_setup) in the loop, the adaptive policy on its own
    b = H.cases_b()
    want = {H.POLICY_CODES[k] for k in ("double", "single", "single_managed", "mixed")}
    assert {_policy_code(c) for c in b} == want
    assert {_policy_code(c) for c in b + [c for c in H.B_EXTRA if "policy" in c]} == want | {H.POLICY_CODES["adaptive"]}
    assert {c["dt"] for c in b} == {"f32", "f64"}
    for policy in H.B_POLICIES:
        mine = [c for c in b if c["policy"] == policy]
        assert {c["smoother"] for c in mine} == set(H.SMOOTHERS) and {c["shape"] for c in mine} == {"129x65", "257"}
        assert all(c["pitch"] != "lib" for c in mine)
    assert {c["kind"] for c in H.B_EXTRA} == {"adaptive", "host_first", "order", "plan"}


def test_the_looser_norm_bound_is_marked_exactly_where_the_rule_allows_it():
    """loose <=> the two handles received their right-hand side through different kinds of entry point, or the sequence holds
    mg_update_rhs_device -- or, in part E, the norm follows mg_time_op(op 6) on a fused handle (the documented exception)"""
    loose, exact = [], []
    for case in H.all_cases():
        for n in case["norms"]:
            assert n["subject"] in ("host", "device") and n["reference"] in ("host", "device")
            rule = n["subject"] != n["reference"] or n["update"]
            if n["time_op_cycle"]:
                assert case["part"] == "E" and case.get("fused", 0) != 0, case["id"]
                rule = True
            if n["update"]:
                assert "mg_update_rhs_device" in case["calls"], case["id"]
            assert n["loose"] == bool(rule), (case["id"], n)
            (loose if n["loose"] else exact).append((case["part"], case["id"], n["name"]))
    assert {p for p, _, _ in loose} == {"A", "B", "E"}                 # mixed kinds (A), an update (B), op 6 (E): nowhere else
    assert all(not n["loose"] for c in H.cases_d() + H.F_CASES for n in c["norms"])      # D and F: host forms, exact
    assert len(exact) > len(loose) > 0


def test_part_d_and_e_tables_cover_what_they_promise():
    d = H.cases_d()
    assert {c["setting"] for c in d} == set(H.D_SETTINGS) and {c["shape"] for c in d} == {"129x65", "257"}
    for c in d:
        if c["policy"].startswith("adaptive"):
            assert c["prefixes"] and not any(s[0] == "coef" for p in c["prefixes"] for s in H.D_PREFIXES[p])
        elif c["policy"] == "defect":
            assert c["prefixes"] == ["fmg-iterate"]
        else:
            assert c["prefixes"] == list(H.D_PREFIXES)
    shifts = {s[1] for steps in H.D_PREFIXES.values() for s in steps if s[0] == "shift"}
    assert {0.37, 160.0, 0.0} <= shifts
    assert H.final_operator(H.D_PREFIXES["shift-coef-solve-const"]) == (None, 0.37)          # the shift stays
    e = H.cases_e()
    assert {c["fused"] for c in e} == {0, 1, 2, 3} and {c["tail"] for c in e} == {0, 1}
    assert {c["shape"] for c in e} == {"33L2", "129x65", "257", "1281"}
    for c in e:
        assert set(c["ops"]) == ({12, 13} if c["shape"] == "1281" else set(H.E_OPS))
    assert set(H.E_OPS) == set(range(10)) | {12, 13}
    assert all(max(H.SHAPES[s][:2]) <= 2049 for s in H.SHAPES)                              # nothing larger
