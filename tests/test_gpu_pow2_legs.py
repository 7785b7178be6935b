"""The fp64 register-blocked legs on grids where they take the exact-FMA forms of RowMath (csrc/mg_host.hpp: pow2_stencil) and on
grids where they must not, through mg_dev_down_leg, mg_dev_up_leg (with and without the norm) and mg_dev_span_leg, against the
NumPy stand-in tests/dist_helpers.NumpyOps (anchored to the oracle by tests/test_dev_calls_cpu.py) -- never against the library.

Shapes: 1153 x 1153 and 1121 x 1185 (coarse 577^2 and 561 x 593), the smallest kind of array the register-blocked family takes
that still has guard-free tiles (the only ones that run the new forms) next to rim tiles (which keep the plain forms) in both
tile shapes, 4 x 8 and 8 x 8 waves x rows.
Taking the new form: hx = hy in {2^-3, 2^-10, 2^-16} with coeff in {-1, 1, -0.5}, two of the nine pairs per leg.  Falling back,
all on every leg: hx = 2^-10 with hy = 2^-9, hx = hy = 1 / 1152, coeff = -0.75, and the two cases that only pow2_stencil's
conditions a >= 1 and |coeff| a >= 1 keep out: hx = hy = 2 (a = 1/4), and coeff = 2^-40 with hx = hy = 2^-3.
Fields: seeded normal values with a patch scaled by 1e-200, one by 1e200 (dyadic spacings), one by 1e-310 (subnormal values:
where hx = hy = 2 took the new form its sums would round differently there), a block of exact zeros and an
untouched (non-zero) ring.  The norm window ends ahead of the 1e200 patch, whose squares are beyond fp64.
Bounds: every stored array bit for bit on dyadic spacings; 5e-14 max(1, max|ref|) on 1 / 1152 (the project's bound for
non-dyadic spacings); the sum of r^2 to 1e-12 relative (its partial sums run over other tiles) -- tests/dev_call_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dev_call_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1153, 1153), (1121, 1185)]
NEW_FORM = [(2.0 ** -3, -1.0), (2.0 ** -10, 1.0), (2.0 ** -16, -0.5), (2.0 ** -3, 1.0), (2.0 ** -10, -0.5), (2.0 ** -16, -1.0),
            (2.0 ** -3, -0.5), (2.0 ** -10, -1.0), (2.0 ** -16, 1.0)]                      # (h, coeff): all nine pairs
FALLBACK = [("neq", 2.0 ** -10, 2.0 ** -9, -1.0, True), ("nd", 1.0 / 1152, 1.0 / 1152, -1.0, False), ("c075", 2.0 ** -10, 2.0 ** -10, -0.75, True),
            ("hbig", 2.0, 2.0, -1.0, True), ("ctiny", 2.0 ** -3, 2.0 ** -3, 2.0 ** -40, True)]
# (name, entry, smoother, omegas, norm window?)
LEGS = [("down-jac", "down_leg", 0, (0.8, 2.0 / 3.0), False), ("down-rb", "down_leg", 1, (1.0, 1.15), False),
        ("up-jac-norm", "up_leg", 0, (2.0 / 3.0, 0.8), True), ("up-jac-plain", "up_leg", 0, (0.8, 2.0 / 3.0), False),
        ("up-rb-norm", "up_leg", 1, (1.15, 1.0), True), ("up-rb-plain", "up_leg", 1, (1.0, 1.15), False),
        ("span-jac", "span_leg", 0, (0.8, 2.0 / 3.0), True)]


def _cases():
    out = []
    for li, (lname, entry, sm, omegas, norm) in enumerate(LEGS):
        combos = [("h%d" % round(-np.log2(h)), h, h, coeff, True) for h, coeff in (NEW_FORM[(li + 4 * m) % 9] for m in range(2))]      # two spacings per leg
        combos += FALLBACK
        for m, (sname, hx, hy, coeff, dyadic) in enumerate(combos):
            k = len(out)
            nx, ny = SHAPES[(li + m) % 2]
            c = dict(entry=entry, disp="compare", dt="f64", dtc="f64", comp="f64", nx=nx, ny=ny, nxc=(nx + 1) // 2, nyc=(ny + 1) // 2, pf="lib", pc="lib",
                     ci=0, cj=0, sides=15, sm=sm, omega=omegas[m % len(omegas)], poff=k % 2, coeff=coeff, hx=hx, hy=hy, dyadic=dyadic,
                     nsweep=1 + (m + li) % 2, nsweep_pre=1 + (k // 2) % 2, zero_init=0, rect=None, seed=4099 * k + 17,
                     window=(1, int(0.55 * nx), 1, ny - 1) if norm else None)
            c["id"] = "%s-%dx%d-%s-c%g-n%d" % (lname, nx, ny, sname, coeff, c["nsweep"])
            out.append(c)
    return out


CASES = _cases()
_STATE = {}


def _env():
    if not _STATE:
        import torch
        import dist_helpers as H
        from mixed_precision_multigrid_solvers_for_pdes_amd import distributed as D
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        _STATE.update(torch=torch, dev=dev, ops=D.HipOps(np.dtype(np.float64), dev), Ref=G.make_ref_ops(H.NumpyOps))
    return _STATE


def _frac(n, lo, hi):
    return slice(int(lo * n), int(hi * n))


def _host_arrays(case):
    """name -> the full host array (guard rows and pad columns hold the NaN sentinel, outputs too)"""
    rng = np.random.default_rng(case["seed"])
    H = {}
    for name, (dt, nx, ny, pk, role) in G.array_specs(case).items():
        ld = G.pitch(pk, dt, ny)
        host = G.sentinel(G.NPDT[dt], (nx + 2 * G.GUARD, ld))
        if role != "out":
            d = rng.standard_normal((nx, ny))
            d[_frac(nx, 0.10, 0.20), _frac(ny, 0.10, 0.30)] *= 1e-200
            # behind the norm window's last row, 0.55 nx; not on 1 / 1152, whose bound scales with max|ref| and would check nothing else
            d[_frac(nx, 0.62, 0.75), _frac(ny, 0.55, 0.80)] *= 1e200 if case["dyadic"] else 1.0
            d[_frac(nx, 0.30, 0.45), _frac(ny, 0.30, 0.50)] = 0.0
            d[_frac(nx, 0.80, 0.90), _frac(ny, 0.10, 0.40)] *= 1e-310
            assert np.all(d[0, :] != 0) and np.all(d[-1, :] != 0) and np.all(d[:, 0] != 0) and np.all(d[:, -1] != 0)      # the ring
            host[G.GUARD:G.GUARD + nx, :ny] = d
        H[name] = (host, nx, ny, ld)
    return H


def _arrays(case, hosts, device):
    torch = _env()["torch"]
    return {name: G.Arr(torch, device, host.copy(), nx, ny, ld) for name, (host, nx, ny, ld) in hosts.items()}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_leg_against_numpy(case):
    s = _env()
    hosts = _host_arrays(case)
    rops = s["Ref"](np.dtype(np.float64))
    R = _arrays(case, hosts, "cpu")
    with np.errstate(all="ignore"):
        ref_sum = G.invoke(case, rops, R)
    ref = G.snapshot(R)
    A = _arrays(case, hosts, s["dev"])
    before = G.snapshot(A)
    got_sum = G.invoke(case, s["ops"], A)
    s["torch"].cuda.synchronize()
    got = G.snapshot(A)
    if case["window"] is not None:
        assert np.isfinite(ref_sum) and ref_sum > 0.0, (case["id"], ref_sum)
        print("%s: sum of r^2 %r, reference %r" % (case["id"], got_sum, ref_sum))
    G.compare_call(case, got, got_sum, ref, ref_sum, rops, before)


def test_the_cases_cover_what_they_should():
    new = {(c["hx"], c["coeff"]) for c in CASES if "-h" in c["id"] and "-hbig-" not in c["id"]}
    assert new == set(NEW_FORM) and len(new) == 9
    for lname, *_ in LEGS:
        mine = [c for c in CASES if c["id"].startswith(lname + "-")]
        assert {c["nsweep"] for c in mine} == {1, 2} and {(c["nx"], c["ny"]) for c in mine} == set(SHAPES), lname
    for sname in ("neq", "nd", "c075", "hbig", "ctiny"):
        assert sum("-%s-" % sname in c["id"] for c in CASES) == len(LEGS), sname
