"""The CPU half of the call-level tests of the mg_dev_* entry points (tests/test_gpu_dev_calls.py is the GPU half):
the NumPy stand-in tests/dist_helpers.NumpyOps is anchored to the pinned oracle (whole grids bit for bit; sub-domains cut out
of a parent array on every cell outside the header's "stale" margin), every case of tests/dev_call_cases.py runs through it, the
case list is shown to notice twelve known kernel mistakes (mutants of the stand-in, compared with the GPU test's own comparison),
and the dispositions of the list are counted."""
import collections
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dev_call_cases as G  # noqa: E402
import dist_helpers as H  # noqa: E402
from oracle import mg_oracle as O  # noqa: E402

Ref = G.make_ref_ops(H.NumpyOps)
SPACINGS = [(1.0 / 32, 1.0 / 32), (1.0 / 64, 1.0 / 16), (0.013, 0.0171)]


def _t(a, pad=3):
    """an array as the padded tensor the ops take"""
    t = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=torch.float32 if a.dtype == np.float32 else torch.float64)
    t.numpy()[:, :a.shape[1]] = a
    return t


def _n(t, shape):
    return t.numpy()[:shape[0], :shape[1]]


def _smooth(kind, u, f, hx, hy, omega, nu):
    return O.jacobi(u, f, hx, hy, omega, nu, "vectorized") if kind == 0 else O.rbgs(u, f, hx, hy, omega, nu)


# ======================================================================================================================
# 1. the stand-in equals the oracle
# ======================================================================================================================
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("sm", [0, 1])
@pytest.mark.parametrize("shape", [(9, 9), (17, 33), (33, 21), (65, 65)])
def test_standin_legs_equal_oracle_composition_on_whole_grids(dtype, sm, shape):
    """sides = 15, zero offsets, full window: down / up / spanning leg == jacobi|rbgs -> residual -> restrict_fw and
    prolong_bilinear -> add -> sweeps -> l2_norm of the oracle, bit for bit"""
    nx, ny = shape
    nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
    rng = np.random.default_rng(nx * 100 + ny + sm)
    for hx, hy in SPACINGS:
        for omega, nsweep in ((0.8, 2), (1.0, 1), (1.15, 0)):
            u, f = rng.standard_normal(shape).astype(dtype), rng.standard_normal(shape).astype(dtype)
            e = rng.standard_normal((nxc, nyc)).astype(dtype)
            ops = H.NumpyOps(dtype)
            # down leg
            out, rc = _t(np.full(shape, 7.0, dtype)), _t(np.full((nxc, nyc), 7.0, dtype))
            ops.down_leg(sm, _t(u), _t(f), out, rc, nx, ny, nxc, nyc, 0, 0, hx, hy, omega, -1.0, nsweep, False, 0)
            v = _smooth(sm, u, f, hx, hy, omega, nsweep)
            r = O.residual(v, f, hx, hy, -1.0)
            np.testing.assert_array_equal(_n(out, shape)[1:], v[1:])
            assert (_n(out, shape)[0] == 7.0).all()
            np.testing.assert_array_equal(_n(rc, (nxc, nyc))[1:-1, 1:-1], O.restrict_fw(r, dtype)[1:-1, 1:-1])
            ring = _n(rc, (nxc, nyc)).copy(); ring[1:-1, 1:-1] = 7.0
            assert (ring == 7.0).all()
            # up leg
            out = _t(np.zeros(shape, dtype))
            s = ops.up_leg(sm, _t(u), _t(f), out, _t(e), nx, ny, nxc, nyc, 0, 0, 15, hx, hy, omega, -1.0, nsweep, 0, (1, nx - 1, 1, ny - 1))
            w = u.copy(); w += O.prolong_bilinear(e, dtype)
            w = _smooth(sm, w, f, hx, hy, omega, nsweep)
            np.testing.assert_array_equal(_n(out, shape)[1:], w[1:])
            rw = O.residual(w, f, hx, hy, -1.0)
            rw[0, :] = rw[-1, :] = 0; rw[:, 0] = rw[:, -1] = 0
            np.testing.assert_allclose(np.sqrt(hx * hy * float(s[0])), float(O.l2_norm(rw, hx, hy)), rtol=1e-13 if dtype == np.float64 else 2e-6)
            wi = O.residual(w, f, hx, hy, -1.0)[1:-1, 1:-1].astype(np.float64)      # the sum itself: fp64 squares of the interior cells
            assert float(s[0]) == float(np.sum(wi * wi))
            # spanning leg = the two compositions in a row
            if nsweep:
                mid, nxt, rc = _t(np.zeros(shape, dtype)), _t(np.zeros(shape, dtype)), _t(np.zeros((nxc, nyc), dtype))
                _n(mid, shape)[0] = w[0]
                ops.span_leg(0, _t(u), _t(f), mid, nxt, _t(e), rc, nx, ny, nxc, nyc, 0, 0, 15, hx, hy, omega, -1.0, nsweep, 2, 0, (1, nx - 1, 1, ny - 1))
                w0 = O.jacobi(u + O.prolong_bilinear(e, dtype), f, hx, hy, omega, nsweep, "vectorized")
                w2 = O.jacobi(w0, f, hx, hy, omega, 2, "vectorized")
                np.testing.assert_array_equal(_n(mid, shape)[1:], w0[1:])
                np.testing.assert_array_equal(_n(nxt, shape)[1:], w2[1:])
                np.testing.assert_array_equal(_n(rc, (nxc, nyc))[1:-1, 1:-1], O.restrict_fw(O.residual(w2, f, hx, hy, -1.0), dtype)[1:-1, 1:-1])


@pytest.mark.parametrize("din", [np.float64, np.float32])
@pytest.mark.parametrize("dout", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(5, 5), (9, 17), (33, 21)])
def test_standin_transfers_equal_oracle_on_whole_grids(din, dout, shape):
    nx, ny = shape
    nxc, nyc = (nx + 1) // 2, (ny + 1) // 2
    rng = np.random.default_rng(nx + 3 * ny)
    fine, e, u = rng.standard_normal(shape).astype(din), rng.standard_normal((nxc, nyc)).astype(din), rng.standard_normal(shape).astype(dout)
    c = _t(np.zeros((nxc, nyc), dout))
    H.NumpyOps(din).restrict(_t(fine), c, nx, ny, nxc, nyc, 15)
    np.testing.assert_array_equal(_n(c, (nxc, nyc)), O.restrict_fw(fine, dout))
    if dout == np.float32 and din == np.float64:
        return                                   # fp32 interpolation of fp64 fields: refused by the library
    tu = _t(u)
    H.NumpyOps(dout).prolong_add(_t(e), tu, nx, ny, nxc, nyc, 15)       # interpolation in the fine grid's dtype (operators/transfer.py:207)
    want = u.copy(); want += O.prolong_bilinear(e, dout)
    np.testing.assert_array_equal(_n(tu, shape), want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_standin_new_entry_points(dtype):
    """fp32-in / fp64-out residual, convert, and the VALUE of the reciprocal diagonal: fl(1 / D) of O._var_update"""
    rng = np.random.default_rng(5)
    shape = (12, 19)
    ops = H.NumpyOps(dtype)
    u, f = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    r = _t(np.zeros(shape))
    ops.residual_mixed(_t(u), _t(f), r, 12, 19, 0.013, 0.02, -1.0)
    np.testing.assert_array_equal(_n(r, shape), O.residual_mixed(u, f, 0.013, 0.02, -1.0))
    x = rng.standard_normal(shape)
    o = _t(np.zeros(shape, np.float32))
    ops.convert(_t(x), o, 12, 19)
    np.testing.assert_array_equal(_n(o, shape), x.astype(np.float32))
    a = np.exp(0.5 * rng.standard_normal(shape)).astype(dtype)
    for sigma in (0.0, 2.5):
        rd = _t(np.full(shape, 9.0, dtype))
        ops.var_rdiag(_t(a), rd, 12, 19, 0.013, 0.02, sigma)
        rd = _n(rd, shape)
        assert rd.dtype == dtype and (rd[0] == 0).all() and (rd[-1] == 0).all() and (rd[:, 0] == 0).all() and (rd[:, -1] == 0).all()
        # one Jacobi step with omega = 1 from u = 0 is f * (1 / D): the factor the oracle's smoother multiplies by
        g = rng.standard_normal(shape).astype(dtype)
        step = O._var_update(np.zeros(shape, dtype), g, a, 0.013, 0.02, 1.0, sigma)
        np.testing.assert_array_equal(step, (g[1:-1, 1:-1] + np.zeros((), dtype)) * rd[1:-1, 1:-1])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("sm", [0, 1])
@pytest.mark.parametrize("cut", [(0, 40, 0, 52), (12, 64, 0, 38), (10, 44, 22, 96), (24, 49, 30, 75), (0, 64, 40, 96)])
def test_standin_on_a_cut_equals_oracle_on_the_parent(dtype, sm, cut):
    """a sub-domain cut out of a 65 x 97 parent (sides, offsets and windows taken from the cut): the stand-in equals the oracle's
    composition on the parent on every cell at least as many cells away from a non-physical edge as the call has stencil stages"""
    NX, NY = 65, 97
    NXC, NYC = 33, 49
    gx0, gx1, gy0, gy1 = cut
    hx, hy = 1.0 / 64, 1.0 / 32
    rng = np.random.default_rng(sum(cut) + sm)
    U, F = rng.standard_normal((NX, NY)).astype(dtype), rng.standard_normal((NX, NY)).astype(dtype)
    E = rng.standard_normal((NXC, NYC)).astype(dtype)
    sides = (1 if gx0 == 0 else 0) | (2 if gx1 == NX - 1 else 0) | (4 if gy0 == 0 else 0) | (8 if gy1 == NY - 1 else 0)
    nx, ny = gx1 - gx0 + 1, gy1 - gy0 + 1
    # coarse block: one coarse cell more than the fine block covers on non-physical low edges (a wider coarse ghost zone)
    cgx0, cgy0 = max(gx0 // 2 - 1, 0), max(gy0 // 2 - 2, 0)
    cgx1, cgy1 = min((gx1 + 1) // 2 + 1, NXC - 1), min((gy1 + 1) // 2, NYC - 1)
    nxc, nyc = cgx1 - cgx0 + 1, cgy1 - cgy0 + 1
    ci, cj = (gx0 - 2 * cgx0) // 2, (gy0 - 2 * cgy0) // 2
    poff = (gx0 + gy0) & 1
    u, f = U[gx0:gx1 + 1, gy0:gy1 + 1].copy(), F[gx0:gx1 + 1, gy0:gy1 + 1].copy()
    e = E[cgx0:cgx1 + 1, cgy0:cgy1 + 1].copy()
    ops = H.NumpyOps(dtype)
    omega, nsweep = (0.8, 2) if sm == 0 else (1.15, 1)
    stages = nsweep * (1 if sm == 0 else 2)            # a red-black sweep is two colour passes: two cells of ghost zone

    def exact(margin):
        """local cells at least `margin` away from every non-physical edge"""
        m = np.ones((nx, ny), dtype=bool)
        if not sides & 1: m[:margin, :] = False
        if not sides & 2: m[nx - margin:, :] = False
        if not sides & 4: m[:, :margin] = False
        if not sides & 8: m[:, ny - margin:] = False
        return m

    # down leg
    V = _smooth(sm, U, F, hx, hy, omega, nsweep)
    RC = O.restrict_fw(O.residual(V, F, hx, hy, -1.0), dtype)
    out, rc = _t(np.zeros((nx, ny), dtype)), _t(np.full((nxc, nyc), np.nan, dtype))
    ops.down_leg(sm, _t(u), _t(f), out, rc, nx, ny, nxc, nyc, ci, cj, hx, hy, omega, -1.0, nsweep, False, poff)
    m = exact(stages); m[0, :] = False
    np.testing.assert_array_equal(_n(out, (nx, ny))[m], V[gx0:gx1 + 1, gy0:gy1 + 1][m])
    m = exact(stages + 2)
    got, n_checked = _n(rc, (nxc, nyc)), 0
    for ic in range(1, nxc - 1):
        for jc in range(1, nyc - 1):
            fi, fj = 2 * (ic - ci), 2 * (jc - cj)
            gi, gj = cgx0 + ic, cgy0 + jc
            if 1 <= fi <= nx - 2 and 1 <= fj <= ny - 2 and m[fi, fj] and 1 <= gi <= NXC - 2 and 1 <= gj <= NYC - 2:
                assert got[ic, jc] == RC[gi, gj], (ic, jc)
                n_checked += 1
            elif not (1 <= fi <= nx - 2 and 1 <= fj <= ny - 2):
                assert np.isnan(got[ic, jc]), (ic, jc)          # no complete fine neighbourhood here: untouched
    assert n_checked > 20
    # up leg, norm over the cells this block would own (two ghost cells more than the stages need)
    W = U.copy(); W += O.prolong_bilinear(E, dtype)
    W = _smooth(sm, W, F, hx, hy, omega, nsweep)
    RW = O.residual(W, F, hx, hy, -1.0)
    g = stages + 2
    win = (0 if sides & 1 else g, nx if sides & 2 else nx - g, 0 if sides & 4 else g, ny if sides & 8 else ny - g)
    out = _t(np.zeros((nx, ny), dtype))
    s = ops.up_leg(sm, _t(u), _t(f), out, _t(e), nx, ny, nxc, nyc, ci, cj, sides, hx, hy, omega, -1.0, nsweep, poff, win)
    m = exact(stages); m[0, :] = False
    np.testing.assert_array_equal(_n(out, (nx, ny))[m], W[gx0:gx1 + 1, gy0:gy1 + 1][m])
    wr = RW[gx0 + max(win[0], 1):gx0 + min(win[1], nx - 1), gy0 + max(win[2], 1):gy0 + min(win[3], ny - 1)].astype(np.float64)
    assert float(s[0]) == float(np.sum(wr * wr))
    # the transfers on the same cut: coarse cell (ic, jc) on fine cell (2 ic, 2 jc), coarse block = what the fine block covers
    nxq, nyq = (nx + 1) // 2, (ny + 1) // 2
    c = _t(np.full((nxq, nyq), np.nan, dtype))
    ops.restrict(_t(f), c, nx, ny, nxq, nyq, sides)
    want = O.restrict_fw(F, dtype)[gx0 // 2:gx0 // 2 + nxq, gy0 // 2:gy0 // 2 + nyq].copy()
    if not sides & 1: want[0, :] = np.nan
    if not sides & 2: want[-1, :] = np.nan
    if not sides & 4: want[:, 0] = np.nan
    if not sides & 8: want[:, -1] = np.nan
    np.testing.assert_array_equal(_n(c, (nxq, nyq)), want)
    eq = E[gx0 // 2:gx0 // 2 + nxq, gy0 // 2:gy0 // 2 + nyq].copy()
    tu = _t(u)
    ops.prolong_add(_t(eq), tu, nx, ny, nxq, nyq, sides)
    W0 = U.copy(); W0 += O.prolong_bilinear(E, dtype)
    want = W0[gx0:gx1 + 1, gy0:gy1 + 1].copy()
    if nx % 2 == 0: want[-1, :] = u[-1, :]          # no coarse partner below the last row / right of the last column: untouched
    if ny % 2 == 0: want[:, -1] = u[:, -1]
    np.testing.assert_array_equal(_n(tu, (nx, ny)), want)
    if sm != 0:
        return
    # the spanning leg: the up leg above, then two more sweeps, residual and full weighting, margins added up
    rops = Ref(dtype)
    mid, nxt, rc = _t(np.zeros((nx, ny), dtype)), _t(np.zeros((nx, ny), dtype)), _t(np.full((nxc, nyc), np.nan, dtype))
    s2 = rops.span_leg(0, _t(u), _t(f), mid, nxt, _t(e), rc, nx, ny, nxc, nyc, ci, cj, sides, hx, hy, omega, -1.0, nsweep, 2, poff, win)
    assert float(s2[0]) == float(np.sum(wr * wr)) or abs(float(s2[0]) - float(np.sum(wr * wr))) <= 1e-12 * float(s2[0])     # fsum against np.sum
    W2 = O.jacobi(W, F, hx, hy, omega, 2, "vectorized")
    RC2 = O.restrict_fw(O.residual(W2, F, hx, hy, -1.0), dtype)
    m = exact(nsweep); m[0, :] = False
    np.testing.assert_array_equal(_n(mid, (nx, ny))[m], W[gx0:gx1 + 1, gy0:gy1 + 1][m])
    m = exact(nsweep + 2); m[0, :] = False
    np.testing.assert_array_equal(_n(nxt, (nx, ny))[m], W2[gx0:gx1 + 1, gy0:gy1 + 1][m])
    m = exact(nsweep + 4)
    got, n_checked = _n(rc, (nxc, nyc)), 0
    for ic in range(1, nxc - 1):
        for jc in range(1, nyc - 1):
            fi, fj = 2 * (ic - ci), 2 * (jc - cj)
            if 1 <= fi <= nx - 2 and 1 <= fj <= ny - 2 and m[fi, fj] and 1 <= cgx0 + ic <= NXC - 2 and 1 <= cgy0 + jc <= NYC - 2:
                assert got[ic, jc] == RC2[cgx0 + ic, cgy0 + jc], (ic, jc)
                n_checked += 1
    assert n_checked > 20


# ======================================================================================================================
# 2. every case runs; the comparison accepts the reference itself
# ======================================================================================================================
_REFS = {}


def _reference(case):
    if case["id"] not in _REFS:
        _REFS[case["id"]] = G.run_reference(case, Ref)
    return _REFS[case["id"]]


@pytest.mark.parametrize("entry", sorted({c["entry"] for c in G.default_cases()}))
def test_every_case_runs_through_the_standin(entry):
    for case in G.cases_of(entry, "compare"):
        keep = G.cells(case) <= 40000
        ref, total, ops = _reference(case) if keep else G.run_reference(case, Ref)
        specs = G.array_specs(case)
        for name in G.OUTPUTS[entry]:
            dt, nx, ny, pk, role = specs[name]
            data = ref[name][G.GUARD:G.GUARD + nx, :ny]
            written = G.bits(data) != G.SENT_BITS[data.dtype.itemsize]
            assert written.any() or name in ("coarse", "rhs_c"), (case["id"], name)       # a 3 x 3 fine array restricts to nothing
            assert np.isfinite(data[written]).all(), (case["id"], name)
        if total is not None:
            assert np.isfinite(total) and total >= 0.0, case["id"]
        G.compare_call(case, ref, total, ref, total, ops)


# ======================================================================================================================
# 3. the list notices known mistakes
# ======================================================================================================================
def _mutants():
    swap = lambda s: (s & ~5) | ((s & 1) << 2) | ((s & 4) >> 2)

    class FarEdgeZerosDropped(Ref):
        def _prolong_field(self, e, a, b, c, d, ci, cj, sides, dtype):
            return super()._prolong_field(e, a, b, c, d, ci, cj, 0, dtype)

    class CiOffByOne(Ref):
        def _prolong_field(self, e, a, b, c, d, ci, cj, sides, dtype):
            return super()._prolong_field(e, a, b, c, d, ci + 1, cj, sides, dtype)

    class CjIgnored(Ref):
        def down_leg(self, sm, u, rhs, out, rhs_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, *a, **kw):
            return super().down_leg(sm, u, rhs, out, rhs_c, lnx, lny, lnxc, lnyc, ci_off, 0, *a, **kw)

    class ColourOffsetIgnored(Ref):
        def _sweeps(self, sm, v, f, hx, hy, omega, nsweep, poff, a=None):
            return super()._sweeps(sm, v, f, hx, hy, omega, nsweep, 0, a)

        def rbgs_colour(self, u, rhs, lnx, lny, hx, hy, omega, colour, offset):
            return super().rbgs_colour(u, rhs, lnx, lny, hx, hy, omega, colour, 0)

    class WindowNotClipped(Ref):
        def _window(self, window, lnx, lny):
            i_lo, i_hi, j_lo, j_hi = window
            return slice(max(i_lo, 0), max(i_hi, i_lo, 0)), slice(max(j_lo, 0), max(j_hi, j_lo, 0))

    class WindowInclusive(Ref):
        def _window(self, window, lnx, lny):
            i_lo, i_hi, j_lo, j_hi = window
            return super()._window((i_lo, i_hi + 1, j_lo, j_hi + 1), lnx, lny)

    class SidesSwapped(Ref):
        def restrict(self, fine, coarse, a, b, c, d, sides):
            return super().restrict(fine, coarse, a, b, c, d, swap(sides))

        def inject_ring(self, fine, coarse, a, b, c, d, sides, ci, cj):
            return super().inject_ring(fine, coarse, a, b, c, d, swap(sides), ci, cj)

    class RingInjectedOnGhostEdge(Ref):
        def inject_ring(self, fine, coarse, a, b, c, d, sides, ci, cj):
            return super().inject_ring(fine, coarse, a, b, c, d, 15, ci, cj)

    class ZeroInitIgnored(Ref):
        def down_leg(self, sm, u, rhs, out, rhs_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, hx, hy, omega, coeff, nsweep, zero_init, *a, **kw):
            return super().down_leg(sm, u, rhs, out, rhs_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, hx, hy, omega, coeff, nsweep, False, *a, **kw)

    class RowZeroWritten(Ref):
        def _store_out(self, o, v):
            o[...] = v

    class IncompleteRestriction(Ref):
        @staticmethod
        def _complete(fi, n):
            return (fi >= 0) & (fi <= n - 2)

    class LastColumnSkipped(Ref):
        """the column next to the pad is never stored"""
        def _store_out(self, o, v):
            keep = o[:, -1].copy()
            super()._store_out(o, v)
            o[:, -1] = keep

        def residual(self, u, f, r, lnx, lny, hx, hy, coeff):
            keep = self._v(r, lnx, lny)[:, -1].copy()
            super().residual(u, f, r, lnx, lny, hx, hy, coeff)
            self._v(r, lnx, lny)[:, -1] = keep

        def convert(self, src, dst, lnx, lny):
            keep = self._v(dst, lnx, lny)[:, -1].copy()
            super().convert(src, dst, lnx, lny)
            self._v(dst, lnx, lny)[:, -1] = keep

        def prolong_add(self, coarse, fine_u, lnxf, lnyf, *a):
            keep = self._v(fine_u, lnxf, lnyf)[:, -1].copy()
            super().prolong_add(coarse, fine_u, lnxf, lnyf, *a)
            self._v(fine_u, lnxf, lnyf)[:, -1] = keep

    return [FarEdgeZerosDropped, CiOffByOne, CjIgnored, ColourOffsetIgnored, WindowNotClipped, WindowInclusive, SidesSwapped,
            RingInjectedOnGhostEdge, ZeroInitIgnored, RowZeroWritten, IncompleteRestriction, LastColumnSkipped]


MUTANTS = _mutants()


def test_there_are_twelve_mutations():
    assert len(MUTANTS) == 12


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_case_list_notices_mutation(mutant):
    """mutant against stand-in, compared with the comparison the GPU test uses: at least one case of the default list fails"""
    caught = []
    for case in sorted(G.default_cases(), key=G.cells):
        if case["disp"] != "compare" or G.cells(case) > 40000:
            continue
        ref, total, ops = _reference(case)
        got, got_total, _ = G.run_reference(case, mutant)
        try:
            G.compare_call(case, got, got_total, ref, total, ops)
        except AssertionError as exc:
            caught.append((case["id"], str(exc)))
            if len(caught) >= 3:
                break
    assert caught, "no case of the default list notices %s: the list is too thin" % mutant.__name__
    for cid, msg in caught:          # the message names entry point, case, output, count, first index, both values, region
        assert cid in msg and "mg_dev_" in msg


# ======================================================================================================================
# 4. dispositions and coverage of the list
# ======================================================================================================================
def test_dispositions_and_coverage():
    cases = G.default_cases()
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    refuse = [c for c in cases if c["disp"] == "refuse"]
    assert 0 < len(refuse) <= len(cases) // 10
    assert len(refuse) == len(G.REFUSALS)
    for c, r in zip(refuse, G.REFUSALS):              # refusals come from the literal table, nowhere else
        assert all(c[k] == v for k, v in r.items()), (c["id"], r)
    n = collections.Counter(G.entry_name(c) for c in cases if c["disp"] == "compare")
    for entry in G.ENTRIES:
        assert n[entry] >= (12 if entry == "span_leg" else 8), (entry, n[entry])
    span = G.cases_of("span_leg", "compare")
    assert 2 * sum(1 for c in span if G.sub_domain(c)) >= len(span)
    for c in span:
        assert G.cells(c) > G.SMALL_CELLS and c["sm"] == 0 and c["dt"] == c["dtc"]
    for entry in ("restrict", "prolong_add", "inject_ring", "up_leg", "span_leg"):
        assert {c["sides"] for c in G.cases_of(entry, "compare")} == set(range(16)), entry
    for entry in ("down_leg", "up_leg", "span_leg"):
        cs = G.cases_of(entry, "compare")
        assert {c["pf"] for c in cs} == set(G.PITCHES) and {c["pc"] for c in cs} == set(G.PITCHES), entry
        assert any(c["pf"] != c["pc"] for c in cs)
        assert {c["sp"] for c in cs} == set(G.SPACINGS), entry
        assert {c["ci"] for c in cs} == {0, 1, 2, 3} and {c["cj"] for c in cs} == {0, 1, 2, 3}, entry
        assert any(c["nxc"] > (c["nx"] + 1) // 2 + c["ci"] for c in cs) and any(c["nxc"] < (c["nx"] + 1) // 2 + c["ci"] for c in cs), entry
    legs = G.cases_of("down_leg", "compare") + G.cases_of("up_leg", "compare")
    assert {G.leg_family(c) for c in legs} == {"tiny", "small", "rb"}
    assert {c["sm"] for c in legs} == {0, 1} and {c["nsweep"] for c in legs} == {0, 1, 2} and {c["poff"] for c in legs} == {0, 1}
    assert {c["zero_init"] for c in G.cases_of("down_leg")} == {0, 1}
    assert {c["omega"] for c in legs} == set(G.OMEGAS)
    assert any(c["coeff"] != -1.0 for c in legs)
    assert {(c["dt"], c["dtc"]) for c in G.cases_of("down_leg", "compare")} == {(a, b) for a in G.DT for b in G.DT}
    for entry in ("prolong_add", "up_leg"):
        assert {(c["dtc"], c["dt"], c["comp"]) for c in G.cases_of(entry, "compare")} == set(G.INTERP_OK), entry
    assert {(c["dt"], c["comp"]) for c in span} == {("f64", "f64"), ("f32", "f32"), ("f32", "f64")}
    for entry in ("restrict", "convert", "inject_ring"):
        assert {(c["dt"], c["dtc"]) for c in G.cases_of(entry)} == {(a, b) for a in G.DT for b in G.DT}, entry
    tags = {c.get("tag") for c in G.cases_of("up_leg", "compare")}
    assert {"full", "sub", "ring", "empty", "none"} <= tags
    assert {"full", "row", "col", "odd", "empty"} <= {c["tag"] for c in G.cases_of("sumsq")}
    # per kernel family of the legs: shapes around the tile extents, elongated arrays, every side mask, every dtype combination
    for fam, ti in (("tiny", 8), ("small", 16)):
        for entry in ("down_leg", "up_leg"):
            cs = [c for c in G.cases_of(entry, "compare") if G.leg_family(c) == fam]
            assert len(cs) >= 20 and sum(1 for c in cs if c.get("var")) >= 6, (fam, entry, len(cs))
            assert {(c["nx"] - 2) % ti for c in cs} >= {0, 1, ti - 1}, (fam, entry)
            assert {(c["ny"] - 1) % 64 for c in cs} >= {0, 1, 63}, (fam, entry)
            assert any(c["nx"] <= 8 and c["ny"] >= 20000 for c in cs) and any(c["ny"] <= 8 and c["nx"] >= 20000 for c in cs), (fam, entry)
        up = [c for c in G.cases_of("up_leg", "compare") if G.leg_family(c) == fam]
        assert {c["sides"] for c in up} == set(range(16)) and {(c["dtc"], c["dt"], c["comp"]) for c in up} == set(G.INTERP_OK), fam
        down = [c for c in G.cases_of("down_leg", "compare") if G.leg_family(c) == fam]
        assert {(c["dt"], c["dtc"]) for c in down} == {(a, b) for a in G.DT for b in G.DT}, fam
    for entry in ("down_leg", "up_leg"):
        cs = [c for c in G.cases_of(entry, "compare") if G.leg_family(c) == "rb"]
        assert len(cs) >= 8 and any(c.get("var") for c in cs), entry
    # the launch split: ghost widths 2 .. 8, as built / a cell larger / a cell smaller, on each family, with variable coefficients
    split = [c for c in G.cases_of("down_leg", "compare") if c["rect"] is not None]
    for fam in ("tiny", "small", "rb"):
        cs = [c for c in split if G.leg_family(c) == fam]
        assert {(c["G"], c["d"]) for c in cs if "G" in c} == {(g, d) for g in range(2, 9) for d in (0, 1, -1)}, fam
        assert {"notile", "whole"} <= {c["tag"] for c in cs}, fam
        assert sum(1 for c in cs if c.get("var") and "G" in c) >= 6 and any(c.get("var") for c in cs if c["tag"] in ("notile", "whole")), fam
        for c in cs:      # large enough for a staged region (at most 64 rows x 256 columns) inside the smallest rectangle
            assert c["nx"] >= 200 and c["ny"] >= 600
    assert len({c["rect_sides"] for c in split}) == 16
    streaming = [c for c in cases if c["dt"] == "f64" and c["nx"] * G.pitch(c.get("pf", "lib"), "f64", c["ny"]) * 8 > G.RB_STREAM_BYTES]
    assert any(c["entry"] == "span_leg" for c in streaming)
    rb = [c for c in span if c["dt"] == "f64"]
    assert any(((c["nx"] - 2 + G.SPAN_TI - 1) // G.SPAN_TI) % G.SPAN_BAND and (c["ny"] - 1) % (G.RB_LANES * 2) in (1, 2) for c in rb)
