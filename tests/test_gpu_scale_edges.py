"""The stateless entry points of the solver modules (mg_dev_pcg_*, mg_dev_ho_*, mg_dev_heat_*, mg_dev_flow_*, mg_dev_nl_eval,
mg_dev_rd_*, mg_dev_eig_*, mg_dev_line_colour) at the shapes of tests/scale_edge_cases.py: more than kReduceBlock and more than
2 kReduceBlock partials, every grid-stride cap passed several times, second and third partial sets thousands of doubles away,
tile counts that are no multiple of kNumXcd, a last tile column one cell wide.

The data is integer-valued and the scalars dyadic (tests/test_scale_edges_cpu.py proves what that gives): every field is compared
bit for bit with the module's own NumPy reference and every sum with ==; there is no tolerance in this file, except in the
line-smoother test, which keeps the rule of tests/test_gpu_line_smoother.py (the Thomas recurrence divides)."""
import ctypes as C
import math

import numpy as np
import pytest

from mixed_precision_multigrid_solvers_for_pdes_amd import _lib

import flow_reference as FR
import heat_device_reference as HD
import line_reference as LR
import nl_reference as NL
import scale_edge_cases as S
from test_gpu_eig import POISON, Block, _dev
from test_gpu_flow import Field as PadField            # outside_untouched(first_free_col): kernels that store whole vectors
from test_gpu_ho import SENTINEL, Field
from test_gpu_line_smoother import Plan, _bits, _row_residual_ratio, _to_device
from test_gpu_line_smoother import _pitch as _line_pitch
from test_gpu_pcg import _direction, _p, _pitches, _same_bits, _scalar, _scratch

pytestmark = pytest.mark.gpu

SHAPES = S.shapes()
NAMES = ["thin", "tall", "sq"]
HX, HY = S.HX, S.HY


def _torch():
    import torch
    return torch


def _sync():
    _torch().cuda.synchronize()


def _nans(n):
    return _torch().full((n,), float("nan"), dtype=_torch().float64, device="cuda")


def _out(shape, ld):
    return Field(np.zeros(shape), ld, fill=SENTINEL)


def _inputs_kept(*fields):
    for f in fields:
        if f is not None:
            assert f.outside_untouched(whole=True), "an input was written"


def _ptr(f):
    return f.ptr if f is not None else None


def _opt(a, ld, cls=Field):
    return cls(a, ld) if a is not None else None


# ------------------------------------------------------------------------------------------ pcg
@pytest.mark.parametrize("variant", S.variants("pcg_direction"))
@pytest.mark.parametrize("name", NAMES)
def test_pcg_direction(name, variant):
    shape = SHAPES[name]
    c = S.case("pcg_direction", shape, variant)
    i = c["inputs"]
    got_p, got_q, pq = _direction(shape[0], shape[1], _pitches(shape[1])[0], HX, HY, S.SIGMA, i["a"], i["z"], i["p"], S.BETA)
    assert _same_bits(got_p, c["fields"]["p"]) and _same_bits(got_q, c["fields"]["q"])
    assert pq == c["sums"]["pq"], (pq, c["sums"]["pq"])


@pytest.mark.parametrize("variant", S.variants("pcg_direction_react"))
@pytest.mark.parametrize("name", NAMES)
def test_pcg_direction_react(name, variant):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("pcg_direction_react", shape, variant)
    i = c["inputs"]
    fz, fp, fa, fc = Field(i["z"], ld), Field(i["p"], ld), _opt(i["a"], ld), Field(i["c"], ld)
    fpo, fq = _out(shape, ld), _out(shape, ld)
    pq, scratch, beta = _scalar(), _scratch(nx, ny), _scalar(S.BETA)
    _lib.check(_lib.load().mg_dev_pcg_direction_react(nx, ny, ld, HX, HY, -1.0, S.SIGMA, _ptr(fa), fc.ptr, fz.ptr, fp.ptr, fpo.ptr,
                                                      fq.ptr, _p(beta), _p(scratch), _p(pq), None))
    _sync()
    _inputs_kept(fz, fp, fa, fc)
    assert fpo.outside_untouched() and fq.outside_untouched()
    assert _same_bits(fpo.field(), c["fields"]["p"]) and _same_bits(fq.field(), c["fields"]["q"])
    assert float(pq.cpu()[0]) == c["sums"]["pq"]


@pytest.mark.parametrize("name", NAMES)
def test_pcg_update(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("pcg_update", shape)
    i = c["inputs"]
    fp, fq, fx, fr = (Field(i[k], ld) for k in "pqxr")
    rr, scratch, alpha = _scalar(), _scratch(nx, ny), _scalar(S.ALPHA)
    _lib.check(_lib.load().mg_dev_pcg_update(nx, ny, ld, _p(alpha), fp.ptr, fq.ptr, fx.ptr, fr.ptr, _p(scratch), _p(rr), None))
    _sync()
    _inputs_kept(fp, fq)
    assert fx.outside_untouched() and fr.outside_untouched()
    assert _same_bits(fx.field(), c["fields"]["x"]) and _same_bits(fr.field(), c["fields"]["r"])
    assert float(rr.cpu()[0]) == c["sums"]["rr"]


@pytest.mark.parametrize("variant", S.variants("pcg_dots"))
@pytest.mark.parametrize("name", NAMES)
def test_pcg_dots(name, variant):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("pcg_dots", shape, variant)
    i = c["inputs"]
    fr, fz, fq = (Field(i[k], ld) for k in "rzq")
    rz, zq, scratch = _scalar(), _scalar(), _scratch(nx, ny)
    flex = variant == "flex"
    _lib.check(_lib.load().mg_dev_pcg_dots(nx, ny, ld, fr.ptr, fz.ptr, fq.ptr if flex else None, _p(scratch), _p(rz), _p(zq), None))
    _sync()
    _inputs_kept(fr, fz, fq)
    assert float(rz.cpu()[0]) == c["sums"]["rz"]
    if flex:
        assert float(zq.cpu()[0]) == c["sums"]["zq"]
    else:
        assert math.isnan(float(zq.cpu()[0]))


@pytest.mark.parametrize("n", S.scalar_lengths())
def test_pcg_scalars(n):
    """every scalar the one-workgroup kernel derives from n partials (first array) and from n partials (second array, the
    flexible beta), against Python's arithmetic on the exact integer sums"""
    lib, torch = _lib.load(), _torch()
    RZ, RZ_OLD, ZQ, PQ, ALPHA, BETA, RR, FLAG = range(8)
    sc = torch.full((10,), 7.0, dtype=torch.float64, device="cuda")

    def step(op, pa, pb=None):
        ta = _dev(pa)
        tb = None if pb is None else _dev(pb)
        _lib.check(lib.mg_dev_pcg_scalars(op, _p(ta), len(pa), None if tb is None else _p(tb), 0 if pb is None else len(pb), _p(sc), None))
        torch.cuda.synchronize()
        return sc.cpu().numpy()

    arrays = [S.partial_array(n, k) for k in range(6)]
    t = [float(int(a.sum())) for a in arrays]
    s = step(0, arrays[0])
    assert s[RZ] == t[0] and s[RZ_OLD] == t[0] and s[FLAG] == 0.0
    s = step(3, arrays[1])
    alpha = t[0] / t[1]
    assert s[PQ] == t[1] and s[ALPHA] == alpha and s[FLAG] == 0.0
    s = step(1, arrays[2])
    assert s[RZ] == t[2] and s[RZ_OLD] == t[0] and s[BETA] == t[2] / t[0]
    s = step(2, arrays[3], arrays[4])                            # na = nb = n
    assert s[RZ] == t[3] and s[RZ_OLD] == t[2] and s[ZQ] == t[4] and s[BETA] == -alpha * t[4] / t[2]
    s = step(2, arrays[3][:5], arrays[4])                        # nb = n alone
    assert s[RZ] == float(arrays[3][:5].sum()) and s[ZQ] == t[4]
    s = step(4, arrays[5])
    assert s[RR] == t[5] and s[8] == t[5] and s[9] == 0.0


# ------------------------------------------------------------------------------------------ ho
@pytest.mark.parametrize("name", NAMES)
def test_ho_direction(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    hx, hy = S.ho_spacings()
    c = S.case("ho_direction", shape)
    fz, fp, fpo, fq = Field(c["inputs"]["z"], ld), Field(c["inputs"]["p"], ld), _out(shape, ld), _out(shape, ld)
    pq, scratch, beta = _scalar(), _scratch(nx, ny), _scalar(S.BETA)
    _lib.check(_lib.load().mg_dev_ho_direction(nx, ny, ld, hx, hy, -1.0, 0.0, fz.ptr, fp.ptr, fpo.ptr, fq.ptr, _p(beta), _p(scratch),
                                               _p(pq), None))
    _sync()
    _inputs_kept(fz, fp)
    assert fpo.outside_untouched() and fq.outside_untouched()
    assert _same_bits(fpo.field(), c["fields"]["p"]) and _same_bits(fq.field(), c["fields"]["q"])
    assert float(pq.cpu()[0]) == c["sums"]["pq"]


@pytest.mark.parametrize("name", NAMES)
def test_ho_rhs_and_residual(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    hx, hy = S.ho_spacings()
    lib = _lib.load()
    c = S.case("ho_rhs", shape)
    ff, fg = Field(c["inputs"]["f"], ld), _out(shape, ld)
    _lib.check(lib.mg_dev_ho_rhs(nx, ny, ld, ff.ptr, fg.ptr, None))
    _sync()
    _inputs_kept(ff)
    assert fg.outside_untouched() and _same_bits(fg.field(), c["fields"]["g"])
    c = S.case("ho_residual", shape)
    fx, fgg, fr = Field(c["inputs"]["x"], ld), Field(c["inputs"]["g"], ld), _out(shape, ld)
    rr, scratch = _scalar(), _scratch(nx, ny)
    _lib.check(lib.mg_dev_ho_residual(nx, ny, ld, hx, hy, -1.0, 0.0, fx.ptr, fgg.ptr, fr.ptr, _p(scratch), _p(rr), None))
    _sync()
    _inputs_kept(fx, fgg)
    assert fr.outside_untouched() and _same_bits(fr.field(), c["fields"]["r"])
    assert float(rr.cpu()[0]) == c["sums"]["rr"]


# ------------------------------------------------------------------------------------------ heat
def _stored(field, want, ny):
    """a kernel that stores whole 16-byte vectors: the field bit for bit, 0 in the pad column of an odd ny, nothing else"""
    assert field.outside_untouched((ny + 1) // 2 * 2)
    assert _same_bits(field.field(), want)
    if ny % 2:
        assert not field.numpy()[2:2 + field.nx, ny].any()


@pytest.mark.parametrize("var", [False, True], ids=["const", "var"])
@pytest.mark.parametrize("scheme", S.variants("heat_rhs"))
@pytest.mark.parametrize("name", NAMES)
def test_heat_rhs(name, scheme, var):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("heat_rhs_var" if var else "heat_rhs", shape, scheme)
    i, h = c["inputs"], S.HEAT
    fu, fp, fs, fa = PadField(i["u"], ld), PadField(i["up"], ld), PadField(i["S"], ld), _opt(i["a"], ld, PadField)
    fo, ss, scratch = PadField(np.full(shape, np.nan), ld), _scalar(), _scratch(nx, ny)
    code = HD.SCHEME_CODES[scheme]
    prev = fp.ptr if scheme == HD.BDF2 else None
    lib = _lib.load()
    if var:
        _lib.check(lib.mg_dev_heat_rhs_var(code, nx, ny, ld, HX, HY, h["alpha"], h["dt"], fu.ptr, prev, fs.ptr, fa.ptr, h["g0"], h["g1"],
                                           fo.ptr, _p(scratch), _p(ss), None))
    else:
        _lib.check(lib.mg_dev_heat_rhs(code, nx, ny, ld, HX, HY, h["alpha"], h["dt"], fu.ptr, prev, fs.ptr, h["g0"], h["g1"], fo.ptr,
                                       _p(scratch), _p(ss), None))
    _sync()
    for f in (fu, fp, fs, fa):
        assert f is None or f.outside_untouched(0)
    _stored(fo, c["fields"]["out"], ny)
    assert float(ss.cpu()[0]) == c["sums"]["sumsq"]


@pytest.mark.parametrize("name", NAMES)
def test_heat_diff_sumsq(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("heat_diff_sumsq", shape)
    fa, fb = PadField(c["inputs"]["a"], ld), PadField(c["inputs"]["b"], ld)
    ss, scratch = _scalar(), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_heat_diff_sumsq(nx, ny, ld, fa.ptr, fb.ptr, _p(scratch), _p(ss), None))
    _sync()
    assert fa.outside_untouched(0) and fb.outside_untouched(0)
    assert float(ss.cpu()[0]) == c["sums"]["sumsq"]


@pytest.mark.parametrize("name", ["thin", "tall"])
def test_heat_ring(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    assert S.chain_facts("heat_ring", shape)[0]["chunks"] >= 2
    c = S.case("heat_ring", shape)
    fu = PadField(c["inputs"]["u"], ld)
    _lib.check(_lib.load().mg_dev_heat_ring(nx, ny, ld, (C.c_double * 4)(*S.EDGE4), fu.ptr, None))
    _sync()
    assert fu.outside_untouched(ny) and _same_bits(fu.field(), c["fields"]["u"])


# ------------------------------------------------------------------------------------------ flow
# where the maximum sits: in the tile / vector at 7/8 of the launch, in the last one, and a NaN in the last one
PLACEMENTS = ["late", "last", "nan"]


def _placement(entry, shape, where):
    frac = 0.875 if where == "late" else 1.0
    if entry == "flow_rhs":
        cell = S.late_tile_cell(shape, frac)[1]
    else:
        cap = S.constants()["cap_flow_stream"]
        wg, chunk, cell = S.late_stream_cell(shape, cap, 1 if entry == "flow_diag" else 0, frac)
        if where != "late":
            assert chunk == S.chain_facts(entry, shape)[0]["chunks"] - 1, "not the last chunk"
    return S.flow_case(entry, shape, peak=None if where == "nan" else cell, nan=cell if where == "nan" else None)


def _same_max(got, want):
    return math.isnan(got) if math.isnan(want) else got == want


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("name", NAMES)
def test_flow_rhs(name, where):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = _placement("flow_rhs", shape, where)
    i, k = c["inputs"], S.FLOW
    assert (where == "nan") == math.isnan(c["maxima"]["m"]) and (where == "nan" or c["maxima"]["m"] >= 2 * S.FLOW_PEAK)
    fp, fw, fn, ff = (PadField(i[n], ld) for n in ("psi", "w", "Np", "F"))
    fo, no = PadField(np.full(shape, np.nan), ld), PadField(np.full(shape, np.nan), ld)
    out2, scratch = _nans(2), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_flow_rhs(nx, ny, ld, HX, HY, k["nu"], k["dt"], k["c0"], k["c1"], fp.ptr, fw.ptr, fn.ptr, ff.ptr, fo.ptr,
                                           no.ptr, _p(scratch), _p(out2), None))
    _sync()
    for f in (fp, fw, fn, ff):
        assert f.outside_untouched(0)
    ss, m = (float(v) for v in out2.cpu())
    assert _same_max(m, c["maxima"]["m"]), (m, c["maxima"]["m"])
    if where != "nan":
        _stored(fo, c["fields"]["f"], ny)
        _stored(no, c["fields"]["N"], ny)
        assert ss == c["sums"]["sumsq"]


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("name", NAMES)
def test_flow_diag(name, where):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = _placement("flow_diag", shape, where)
    assert (where == "nan") == math.isnan(c["maxima"]["m"]) and (where == "nan" or c["maxima"]["m"] >= 2 * S.FLOW_PEAK)
    fp, fw = PadField(c["inputs"]["psi"], ld), PadField(c["inputs"]["w"], ld)
    out3, scratch = _nans(3), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_flow_diag(nx, ny, ld, fp.ptr, fw.ptr, _p(scratch), _p(out3), None))
    _sync()
    assert fp.outside_untouched(0) and fw.outside_untouched(0)
    e, z, m = (float(v) for v in out3.cpu())
    # the NaN sits on the ring of psi: it enters the velocity term of its neighbour and neither sum
    assert e == c["sums"]["e"] and z == c["sums"]["z"] and _same_max(m, c["maxima"]["m"]), (e, z, m, c["sums"], c["maxima"])


@pytest.mark.parametrize("where", PLACEMENTS)
@pytest.mark.parametrize("name", NAMES)
def test_flow_interior(name, where):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = _placement("flow_interior", shape, where)
    assert (where == "nan") == math.isnan(c["maxima"]["change"]) and (where == "nan" or c["maxima"]["change"] == S.FLOW_PEAK)
    fw, fold, fo = PadField(c["inputs"]["w"], ld), PadField(c["inputs"]["old"], ld), PadField(np.full(shape, np.nan), ld)
    out2, scratch = _nans(2), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_flow_interior(nx, ny, ld, fw.ptr, fold.ptr, fo.ptr, _p(scratch), _p(out2), None))
    _sync()
    assert fw.outside_untouched(0) and fold.outside_untouched(0)
    _stored(fo, c["fields"]["out"], ny)
    ss, mx = (float(v) for v in out2.cpu())
    assert ss == c["sums"]["sumsq"] and _same_max(mx, c["maxima"]["change"]), (ss, mx, c["sums"], c["maxima"])


@pytest.mark.parametrize("name", ["thin", "tall"])
def test_flow_wall(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    assert S.chain_facts("flow_wall", shape)[0]["chunks"] >= 2
    c = S.case("flow_wall", shape)
    fp, fw = PadField(c["inputs"]["psi"], ld), PadField(c["inputs"]["w"], ld)
    _lib.check(_lib.load().mg_dev_flow_wall(nx, ny, ld, HX, HY, FR.NO_SLIP, (C.c_double * 4)(*S.SPEEDS), fp.ptr, fw.ptr, None))
    _sync()
    assert fp.outside_untouched(0) and fw.outside_untouched(ny) and _same_bits(fw.field(), c["fields"]["w"])


# ------------------------------------------------------------------------------------------ nl / rd
@pytest.mark.parametrize("kind", S.variants("nl_eval"))
@pytest.mark.parametrize("name", NAMES)
def test_nl_eval(name, kind):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("nl_eval", shape, kind)
    i, n = c["inputs"], S.NLPAR
    fu, fd, ff, fa, fw = (Field(i[k], ld) for k in ("u", "delta", "f", "a", "w"))
    fuo, fF, fc = _out(shape, ld), _out(shape, ld), _out(shape, ld)
    sums, scratch = _nans(2), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_nl_eval(NL.KINDS[kind], nx, ny, ld, HX, HY, n["coeff"], n["sigma"], n["kappa"], fa.ptr, fw.ptr, fu.ptr,
                                          fd.ptr, n["t"], ff.ptr, fuo.ptr, fF.ptr, fc.ptr, _p(scratch), _p(sums), None))
    _sync()
    _inputs_kept(fu, fd, ff, fa, fw)
    for f, key in ((fuo, "v"), (fF, "F"), (fc, "c")):
        assert f.outside_untouched() and _same_bits(f.field(), c["fields"][key]), key
    got = [float(v) for v in sums.cpu()]
    assert got == [c["sums"]["FF"], c["sums"]["c"]], (got, c["sums"])


@pytest.mark.parametrize("name", NAMES)
def test_rd_rhs(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("rd_rhs", shape)
    i, r = c["inputs"], S.RDPAR
    fu, fp, fs, fa, fw = (Field(i[k], ld) for k in ("u", "up", "S", "a", "w"))
    fo, ss, scratch = _out(shape, ld), _scalar(), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_rd_rhs(2, NL.CUBIC, nx, ny, ld, HX, HY, r["alpha"], r["dt"], r["kappa"], r["rho"], fu.ptr, fp.ptr, fs.ptr,
                                         fa.ptr, fw.ptr, r["g0"], r["g1"], fo.ptr, _p(scratch), _p(ss), None))
    _sync()
    _inputs_kept(fu, fp, fs, fa, fw)
    assert fo.outside_untouched() and _same_bits(fo.field(), c["fields"]["out"])
    assert float(ss.cpu()[0]) == c["sums"]["sumsq"]


@pytest.mark.parametrize("variant", S.variants("rd_energy"))
@pytest.mark.parametrize("name", NAMES)
def test_rd_energy(name, variant):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("rd_energy", shape, variant)
    i = c["inputs"]
    fu, fa, fw = Field(i["u"], ld), _opt(i["a"], ld), _opt(i["w"], ld)
    sums, scratch = _nans(3), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_rd_energy(NL.CUBIC, nx, ny, ld, HX, HY, _ptr(fa), _ptr(fw), fu.ptr, _p(scratch), _p(sums), None))
    _sync()
    _inputs_kept(fu, fa, fw)
    got = [float(v) for v in sums.cpu()]
    assert got == [c["sums"]["G"], c["sums"]["P"], c["sums"]["Q"]], (got, c["sums"])


# ------------------------------------------------------------------------------------------ eig
@pytest.mark.parametrize("entry", ["eig_gram_3x5", "eig_gram_18x36"])
@pytest.mark.parametrize("name", NAMES)
def test_eig_gram(name, entry):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    facts = S.chain_facts(entry, shape)[0]
    assert facts["chunks"] >= 3, "a workgroup walks many tiles"
    c = S.case(entry, shape)
    p, q = c["inputs"]["p"], c["inputs"]["q"]
    vb = Block(c["inputs"]["v"], ld, outside=POISON, ring=POISON)
    g, scratch = _nans(p * q), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_eig_gram(nx, ny, ld, vb.stride, p, vb.ptr(0), q, vb.ptr(0), _p(scratch), _p(g), None))
    _sync()
    assert np.array_equal(g.cpu().numpy().reshape(p, q), c["sums"]["G"])


@pytest.mark.parametrize("name", NAMES)
def test_eig_combine(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("eig_combine", shape)
    inb = Block(c["inputs"]["cols"], ld, outside=0.5)
    out = Block(np.zeros((S.COMBINE_Q, nx, ny)), ld, fill=np.nan)
    _lib.check(_lib.load().mg_dev_eig_combine(nx, ny, ld, inb.stride, S.COMBINE_P, inb.ptr(), S.COMBINE_Q, _p(_dev(c["inputs"]["coef"])),
                                              out.ptr(), None))
    _sync()
    assert _same_bits(out.fields(), c["fields"]["out"])
    assert out.untouched(stored_cols=S.nyv_of(ny)) and inb.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_eig_residual(name):
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    c = S.case("eig_residual", shape)
    i = c["inputs"]
    xb, axb, rb = Block(i["x"], ld, outside=POISON), Block(i["ax"], ld, outside=POISON), Block(i["x"], ld, fill=np.nan)
    ss, scratch = _nans(S.EIG_COLS), _scratch(nx, ny)
    _lib.check(_lib.load().mg_dev_eig_residual(nx, ny, ld, S.EIG_COLS, xb.stride, xb.ptr(), axb.ptr(), _p(_dev(i["lam"])), rb.ptr(),
                                               _p(scratch), _p(ss), None))
    _sync()
    assert _same_bits(rb.fields(), c["fields"]["r"])
    assert np.array_equal(ss.cpu().numpy(), c["sums"]["sumsq"])
    assert rb.untouched(stored_cols=S.nyv_of(ny)) and xb.untouched() and axb.untouched()


@pytest.mark.parametrize("name", NAMES)
def test_eig_apply(name):
    """against mg_dev_pcg_direction's q column by column, as the small-shape test does, and against the NumPy operator"""
    shape = SHAPES[name]
    nx, ny = shape
    ld = _pitches(ny)[0]
    lib = _lib.load()
    c = S.case("eig_apply", shape)
    cols = c["inputs"]["cols"]
    vb, avb = Block(cols, ld), Block(cols, ld, fill=np.nan)
    _lib.check(lib.mg_dev_eig_apply(nx, ny, ld, S.EIG_COLS, vb.stride, HX, HY, -1.0, None, vb.ptr(), avb.ptr(), None))
    _sync()
    got = avb.fields()
    assert avb.untouched(stored_cols=ny) and vb.untouched()
    zb = Block(np.stack([S.PR.zero_ring(col) for col in cols]), ld)
    qb, pb = Block(cols, ld, fill=np.nan), Block(cols, ld, fill=np.nan)
    pq, scratch = _nans(1), _scratch(nx, ny)
    for k in range(S.EIG_COLS):
        _lib.check(lib.mg_dev_pcg_direction(nx, ny, ld, HX, HY, -1.0, 0.0, None, zb.ptr(k), None, pb.ptr(k), qb.ptr(k), None, _p(scratch),
                                            _p(pq), None))
    _sync()
    assert _same_bits(got, qb.fields()) and _same_bits(got, c["fields"]["av"])


# ------------------------------------------------------------------------------------------ line
LINE_SHAPES = [SHAPES["sq"], (1025, 4097)]


@pytest.mark.parametrize("direction", [LR.ZEBRA_X, LR.ZEBRA_Y], ids=["x", "y"])
@pytest.mark.parametrize("shape", LINE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_line_colour(shape, direction):
    """many long lines: both colours of one pass (fp64, omega = 1, no shift) under the two bars of
    tests/test_gpu_line_smoother.py: every updated cell satisfies its row of the line system to 8 eps (|T||x| + |b|), and
    max |x - x_ref| <= 8 cond eps max |x_ref| against the reference sweep"""
    torch = _torch()
    nx, ny = shape
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    ld = _line_pitch(np.float64, ny)
    rng = np.random.default_rng(nx + ny)
    u, rhs = rng.standard_normal(shape), rng.standard_normal(shape)
    eps = np.finfo(np.float64).eps
    w, _, D = LR.line_coefficients(direction, hx, hy, 0.0)
    cond = (D + 2 * w) / (D - 2 * w)
    plan = Plan(np.float64, direction, nx, ny, ld, hx, hy, 0.0)
    try:
        cur = u
        for colour in (0, 1):
            du, df = _to_device(cur, ld), _to_device(rhs, ld)
            plan.colour(colour, 1.0, du, df)
            torch.cuda.synchronize()
            full = du.cpu().numpy()
            got = full[:, :ny]
            assert np.all(np.isnan(full[:, ny:])), "pad columns changed"
            ref, xref = LR.colour_pass(cur, rhs, direction, colour, hx, hy, 0.0, 1.0)
            keep = np.ones(shape, bool)                       # the ring and the lines of the other colour
            lines = (np.arange(ny) % 2 == colour) if direction == LR.ZEBRA_X else (np.arange(nx) % 2 == colour)
            if direction == LR.ZEBRA_X:
                keep[1:-1, 1:-1] = ~lines[None, 1:-1]
            else:
                keep[1:-1, 1:-1] = ~lines[1:-1, None]
            assert np.array_equal(_bits(got[keep]), _bits(cur[keep])), "ring / other colour changed"
            ratio = _row_residual_ratio(direction, colour, cur, rhs, got, hx, hy, 0.0)
            err = float(np.max(np.abs(got - ref)))
            bar = 8 * cond * eps * float(np.max(np.abs(xref)))
            print("%dx%d dir %d colour %d: row residual / eps(|T||x|+|b|) %.2f, max|x - x_ref| / bar %.3f" % (nx, ny, direction, colour, ratio, err / bar))
            assert ratio <= 8.0 and err <= bar
            cur = got.copy()
    finally:
        plan.close()
