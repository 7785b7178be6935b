"""The exact-FMA forms of the fp64 register-blocked legs (csrc/mg_rb_kernels.hpp: RowMath, csrc/mg_host.hpp: pow2_stencil) against
the plain forms they replace, bit for bit, in NumPy fp64.

    sweep      plain  nb = a (dn + up) + a (ea + wv);  un = (f + nb) invD;  (1 - w) mid + w un
               fused  un = fma(S, a, f) invD
    residual   plain  f - coeff (((dn + up) a + (ea + wv) a) - mid D)
               fused  fma(-coeff a, fma(mid, -4, S), f)
    with S = (dn + up) + (ea + wv), a = 1 / h^2 = 2^p, D = 4 a, coeff = +-2^k.

NumPy has no fused multiply-add.  On the grids the forms are used on it needs none: a S, (-4) mid and (-coeff a) q are scalings
by powers of two, hence exact products (short of overflow), so fma(x, y, z) IS x * y + z there: the product does not round and
the sum rounds once, as the FMA does.  The last test shows that this stand-in notices a product that does round."""
import numpy as np
import pytest

HS = [2.0 ** -k for k in range(1, 17)]
OMEGAS = [0.8, 2.0 / 3.0, 1.0, 1.15]
COEFFS = [1.0, -1.0, -0.5, 2.0]
CELLS = 20000                      # per (h, field kind)


def fma_exact_product(x, y, z):
    """fma(x, y, z) where x * y is exact (see the module docstring)"""
    return x * y + z


def sweep_plain(mid, dn, up, ea, wv, f, a, invD, om):
    nb = a * (dn + up) + a * (ea + wv)
    un = (f + nb) * invD
    return (1.0 - om) * mid + om * un


def sweep_fused(mid, dn, up, ea, wv, f, a, invD, om):
    un = fma_exact_product((dn + up) + (ea + wv), a, f) * invD
    return (1.0 - om) * mid + om * un


def resid_plain(mid, dn, up, ea, wv, f, a, D, coeff):
    return f - coeff * (((dn + up) * a + (ea + wv) * a) - mid * D)


def resid_fused(mid, dn, up, ea, wv, f, a, coeff):
    return fma_exact_product(-(coeff * a), fma_exact_product(mid, -4.0, (dn + up) + (ea + wv)), f)


def _fields(rng, kind, n):
    """(mid, dn, up, ea, wv, f) of n cells"""
    six = rng.standard_normal((6, n))
    if kind == "wide":             # independent magnitudes from the smallest subnormal to 1e250
        v = six * 10.0 ** rng.uniform(-323.0, 250.0, (6, n))
    elif kind == "subnormal":      # everything at the bottom of the range: sums that are exact, products that scale up
        v = six * 10.0 ** rng.uniform(-323.0, -300.0, (6, n))
    elif kind == "common":         # one scale per cell and neighbours that nearly cancel each other and the centre
        s = 10.0 ** rng.uniform(-310.0, 250.0, n)
        base = rng.standard_normal(n)
        eps = 2.0 ** rng.integers(-52, -1, (6, n)) * rng.integers(-3, 4, (6, n))
        v = (base + base * eps) * s
        v[2] = -v[1] * (1.0 + eps[2])                     # dn + up cancels
        v[0] = 0.25 * ((v[1] + v[2]) + (v[3] + v[4]))     # S - 4 mid cancels
    elif kind == "zeros":          # signed zeros among ordinary values
        v = six.copy()
        z = rng.integers(0, 3, (6, n))
        v[z == 1] = 0.0
        v[z == 2] = -0.0
    else:
        raise KeyError(kind)
    return tuple(np.ascontiguousarray(x) for x in v)


def _mismatches(x, y):
    """cells whose bit patterns differ, among those where either result is finite"""
    look = np.isfinite(x) | np.isfinite(y)
    return int(np.count_nonzero((x.view(np.int64) != y.view(np.int64)) & look))


@pytest.mark.parametrize("kind", ["wide", "subnormal", "common", "zeros"])
def test_fused_forms_give_the_bits_of_the_plain_forms(kind):
    rng = np.random.default_rng({"wide": 11, "subnormal": 12, "common": 13, "zeros": 14}[kind])
    bad_sweep = bad_resid = cells = 0
    with np.errstate(all="ignore"):
        for h in HS:
            a = 1.0 / (h * h)
            D = 2.0 / (h * h) + 2.0 / (h * h)
            invD = 1.0 / D
            assert D == 4.0 * a and np.frexp(a)[0] == 0.5 and np.frexp(invD)[0] == 0.5
            mid, dn, up, ea, wv, f = _fields(rng, kind, CELLS)
            for om in OMEGAS:
                bad_sweep += _mismatches(sweep_plain(mid, dn, up, ea, wv, f, a, invD, om), sweep_fused(mid, dn, up, ea, wv, f, a, invD, om))
            for coeff in COEFFS:
                bad_resid += _mismatches(resid_plain(mid, dn, up, ea, wv, f, a, D, coeff), resid_fused(mid, dn, up, ea, wv, f, a, coeff))
            cells += CELLS
    assert cells == len(HS) * CELLS
    assert bad_sweep == 0 and bad_resid == 0, "%s: %d sweep and %d residual cells differ in %d cells x 4" % (kind, bad_sweep, bad_resid, cells)


def test_the_comparison_notices_a_spacing_that_is_no_power_of_two():
    """a = 1152^2: a S rounds, so the stand-in's x * y + z rounds twice where the plain form rounds three times in other places"""
    rng = np.random.default_rng(15)
    n = 4000
    a = 1152.0 ** 2
    D = 4.0 * a
    mid, dn, up, ea, wv, f = (rng.standard_normal(n) for _ in range(6))
    assert _mismatches(sweep_plain(mid, dn, up, ea, wv, f, a, 1.0 / D, 0.8), sweep_fused(mid, dn, up, ea, wv, f, a, 1.0 / D, 0.8)) > 0
    assert _mismatches(resid_plain(mid, dn, up, ea, wv, f, a, D, -1.0), resid_fused(mid, dn, up, ea, wv, f, a, -1.0)) > 0


def test_scaling_down_breaks_the_identity_in_the_subnormal_range():
    """Why pow2_stencil also asks for a >= 1 and |coeff| a >= 1: a = 1/4 (h = 2) shrinks the sums, a s1 and a s2 round where they
    reach the subnormal range and the plain form no longer equals a rn(s1 + s2).  (A tiny coeff with a >= 1 shrinks only the last
    product, which differs from its FMA on ties alone: excluded as well, too rare to show here.)  tests/test_gpu_pow2_legs.py runs
    both as cases that must keep the plain arithmetic."""
    rng = np.random.default_rng(16)
    a, D = 0.25, 1.0
    assert D == 2.0 / 4.0 + 2.0 / 4.0 and D == 4.0 * a
    with np.errstate(all="ignore"):
        mid, dn, up, ea, wv, f = _fields(rng, "subnormal", 4000)
        assert _mismatches(sweep_plain(mid, dn, up, ea, wv, f, a, 1.0 / D, 0.8), sweep_fused(mid, dn, up, ea, wv, f, a, 1.0 / D, 0.8)) > 0
        assert _mismatches(resid_plain(mid, dn, up, ea, wv, f, a, D, -1.0), resid_fused(mid, dn, up, ea, wv, f, a, -1.0)) > 0
