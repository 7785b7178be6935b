"""Every mg_dev_* kernel entry point at the ends of the finite range: the cases of dev_call_cases.special_cases() -- each entry
and dtype combination of the default list on fields that are subnormal (`tiny`), near overflow (`huge`) or normal with
subnormal, small and large rectangles (`patches`), and fp64 values that straddle what fp32 holds through the conversions --
against the NumPy restatement, through the harness of tests/test_gpu_dev_calls.py.  Dyadic spacings only; every stored
array by special_values.same_special, i.e. bit for bit (a NaN for a NaN), sums by the rule of compare_sum.
tests/test_special_values_cpu.py shows on the restatement that the fields are what they are meant to be."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dev_call_cases as G  # noqa: E402
import test_gpu_dev_calls as T  # noqa: E402

pytestmark = pytest.mark.gpu


def _cases(entry):
    return pytest.mark.parametrize("case", [c for c in G.special_cases() if c["entry"] == entry], ids=lambda c: c["id"])


def _check(case):
    ref, ref_sum, rops = G.run_reference(case, T._env()["Ref"])
    A, before, got, total = T._device_run(case)
    G.compare_call(case, got, total, ref, ref_sum, rops, before, special=True)


@_cases("jacobi")
def test_jacobi(case):
    _check(case)


@_cases("rbgs_colour")
def test_rbgs_colour(case):
    _check(case)


@_cases("residual")
def test_residual(case):
    _check(case)


@_cases("residual_mixed")
def test_residual_f32in_f64out(case):
    _check(case)


@_cases("sumsq")
def test_sumsq(case):
    _check(case)


@_cases("restrict")
def test_restrict_fw(case):
    _check(case)


@_cases("prolong_add")
def test_prolong_add(case):
    _check(case)


@_cases("convert")
def test_convert(case):
    _check(case)


@_cases("inject_ring")
def test_inject_ring(case):
    _check(case)


@_cases("var_rdiag")
def test_var_rdiag(case):
    _check(case)


@_cases("down_leg")
def test_down_leg(case):
    """mg_dev_down_leg and mg_dev_down_leg_var"""
    _check(case)


@_cases("up_leg")
def test_up_leg(case):
    """mg_dev_up_leg and mg_dev_up_leg_var"""
    _check(case)


@_cases("span_leg")
def test_span_leg(case):
    _check(case)
