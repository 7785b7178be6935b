"""Cases for the solver modules' kernels at the shapes where their loops wrap -- not a test.  What tests/test_scale_edges_cpu.py
pins on the CPU and tests/test_gpu_scale_edges.py runs on the device.

Constants.  kReduceBlock, kBlock, kTI, kTileRowBytes, kNumXcd, kGramWorkgroups and the cap of every grid-stride launcher are
parsed from csrc/ (`constants()`), never typed in: the shapes and `chain_facts` follow them.

Shapes.  `thin` (2 kTI + 1 rows), `tall` (TJ + 1 columns: a last tile column one cell wide) and `sq`.  The long side of thin and
tall is (2 kReduceBlock + 12) tiles + 1 cell: more than 2 kReduceBlock partials from tile grids that include the ring rows and
from those that do not, a tile count that is no multiple of kNumXcd in either, and about 8 x the largest grid-stride cap in
vectors.  sq has kReduceBlock < ntiles < 2 kReduceBlock with ntiles % kNumXcd == 1 and a partial tile on both sides.

Data.  Integer-valued fp64 fields (magnitude 1 .. 5 from a position-dependent pattern, seeded signs: no cell is 0) and dyadic
scalars: every operation of every kernel is then exact, a sum is the same number in any order, and the expected sums are
formed in integer arithmetic by `exact_dot`, which also proves the claim (every factor a multiple of 2^-k, the sum of the
absolute products below 2^53 in those units, hence every partial sum of every order representable).  The fields a case expects
come from the modules' own NumPy references (pcg_reference, nl_reference, ho_reference, heat_device_reference,
heat_var_reference, flow_reference, rd_reference, eig_reference): nothing here restates an operator.

The compact nine-point weights hold 5/3, 1/6 and 1/12 of 1/hx^2 and 1/hy^2, which no dyadic spacing makes dyadic; the ho cases
use hx = 1 and an hy with fl(1 / fl(hy hy)) == 11, for which the host's weight formulas give exactly 20, 1, -9 and 1."""
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eig_reference as ER                                                        # noqa: E402
import flow_reference as FR                                                       # noqa: E402
import heat_device_reference as HD                                                # noqa: E402
import heat_var_reference as HV                                                   # noqa: E402
import ho_reference as HO                                                         # noqa: E402
import nl_reference as NL                                                         # noqa: E402
import pcg_reference as PR                                                        # noqa: E402
import rd_reference as RD                                                         # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "mixed_precision_multigrid_solvers_for_pdes_amd", "csrc")


# ---------------------------------------------------------------------------------------------- constants, from the sources
def _text(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _int(text, pattern, what):
    m = re.search(pattern, text)
    assert m, "cannot find %s in the sources" % what
    return int(m.group(1))


_CONSTANTS = {}


def constants():
    if _CONSTANTS:
        return _CONSTANTS
    k, pcg, heat, flow, eig = (_text(n) for n in ("mg_kernels.hpp", "mg_pcg.hip", "mg_heat.hip", "mg_flow.hip", "mg_eig.hip"))
    eigk, launch = _text("mg_eig_kernels.hpp"), _text("mg_launch.hip")
    c = {n: _int(k, r"constexpr int %s = (\d+);" % n, n) for n in ("kReduceBlock", "kBlock", "kTI", "kTileRowBytes", "kNumXcd",
                                                                    "kFusedTISmall", "kFusedTITiny")}
    c["kFusedTI"] = _int(k, r"#define MG_FUSED_TI (\d+)", "MG_FUSED_TI")
    c["TJ"] = c["kTileRowBytes"] // 8
    c["kGramWorkgroups"] = _int(eig, r"constexpr int kGramWorkgroups = (\d+);", "kGramWorkgroups")
    c["kEigKC"] = _int(eigk, r"constexpr int kEigKC = (\d+);", "kEigKC")
    c["cap_pcg_stream"] = _int(pcg, r"(?s)int stream_blocks\(int nx, int nyv\) \{.*?mg::kBlock, (\d+)\)\);", "the cap of pcg stream_blocks")
    c["pcg_dots_second"] = _int(pcg, r"\(double\*\)scratch \+ (\d+), n, zq_dev", "the second set of mg_dev_pcg_dots")
    c["cap_heat_diff"] = _int(heat, r"(?s)int launch_diff\(.*?mg::kBlock, (\d+)\)\);", "the cap of heat launch_diff")
    c["cap_heat_ring"] = _int(heat, r"(?s)void launch_ring\(.*?std::min\((\d+), \(2 \* \(nx \+ ny\)", "the cap of heat launch_ring")
    c["cap_flow_stream"] = _int(flow, r"(?s)int stream_blocks\(long long vecs\) \{.*?mg::kBlock, (\d+)\)\);", "the cap of flow stream_blocks")
    c["cap_flow_wall"] = _int(flow, r"(?s)void launch_wall\(.*?std::min\((\d+), \(2 \* \(nx \+ ny\)", "the cap of flow launch_wall")
    c["cap_eig_combine"] = _int(eig, r"stream_blocks\(\(long long\)nx \* \(nyv / 2\), (\d+)\);", "the cap of eig_combine")
    c["cap_eig_residual"] = _int(eig, r"std::min<size_t>\((\d+), cap / ncols\)", "the cap of eig_residual")
    c["partials_floor"] = _int(launch, r"std::max<long long>\((\d+), ti \* tj\)", "the floor of max_partials")
    c["partials_tj"] = _int(launch, r"const long long tj = \(ny \+ \d+\) / (\d+) \+ 1;", "the tile width of max_partials")
    _CONSTANTS.update(c)
    return _CONSTANTS


def max_partials(nx, ny):
    """mg_launch.hip's max_partials: doubles of mg_dev_scratch_bytes(nx, ny)"""
    c = constants()
    tj = (ny + c["partials_tj"] - 1) // c["partials_tj"] + 1
    ti_min = min(c["kTI"], c["kFusedTI"], c["kFusedTISmall"], c["kFusedTITiny"])
    ti = (nx + ti_min - 1) // ti_min + 1
    return max(c["partials_floor"], ti * tj)


# ---------------------------------------------------------------------------------------------- shapes
LONG_MARGIN = 12         # tiles past 2 kReduceBlock on the long side of thin and tall


def shapes():
    c = constants()
    long_tiles = 2 * c["kReduceBlock"] + LONG_MARGIN
    ti = math.isqrt(2 * c["kReduceBlock"] - 1) + 2          # 47 tile rows ...
    tj = ti // 2                                            # ... x 23 tile columns: kReduceBlock + 57 tiles
    return {"thin": (2 * c["kTI"] + 1, long_tiles * c["kTI"] + 1),
            "tall": (long_tiles * c["kTI"] + 1, c["TJ"] + 1),
            "sq": ((ti - 1) * c["kTI"] + 3, (tj - 1) * c["TJ"] + c["TJ"] - 1)}


def tile_grid(shape, interior_only=False):
    """(tile rows, tile columns) of the LDS-tiled kernels: every solver module's geometry includes the ring rows (i_org = 0);
    the engine's smoothers tile the interior alone (mg_launch.hip make_geom)"""
    c = constants()
    nx, ny = shape
    rows, cols = (nx - 2, ny - 1) if interior_only else (nx, ny)
    return (rows + c["kTI"] - 1) // c["kTI"], (cols + c["TJ"] - 1) // c["TJ"]


def ntiles(shape, interior_only=False):
    a, b = tile_grid(shape, interior_only)
    return a * b


def nyv_of(ny):
    return (ny + 1) // 2 * 2       # the library's pitch is a multiple of 64 doubles: min(ld, roundup(ny, 2)) is the second


def xcd_remap(b, n):
    """mg_kernels.hpp: the tile that workgroup b of n works on"""
    k = constants()["kNumXcd"]
    q, r = divmod(n, k)
    x, idx = b % k, b // k
    base = x * (q + 1) if x < r else r * (q + 1) + (x - r) * q
    return base + idx


def late_tile_cell(shape, fraction):
    """(workgroup, (i, j)): the first interior cell of the tile that the workgroup at `fraction` of an LDS-tiled launch works
    on, walking down from there to the first workgroup whose tile holds one.  fraction = 1 is the last workgroup: its partial is
    the last one a reduction reads"""
    c = constants()
    nx, ny = shape
    n = ntiles(shape)
    tiles_j = tile_grid(shape)[1]
    for b in range(min(n - 1, int(fraction * n)), -1, -1):
        ti, tj = divmod(xcd_remap(b, n), tiles_j)
        i, j = max(1, ti * c["kTI"]), max(1, tj * c["TJ"])
        if i <= nx - 2 and j <= ny - 2:
            return b, (i, j)
    raise AssertionError("no tile with an interior cell")


def late_stream_cell(shape, cap, rows_from, fraction):
    """(workgroup, chunk, (i, j)): a cell of the 16-byte vector at `fraction` of a grid-stride launch over the rows
    rows_from .. nx - 1 - rows_from (fraction = 1: the last vector), which the workgroup takes in its chunk-th pass; with
    rows_from = 1 the cell is an interior one"""
    c = constants()
    nx, ny = shape
    vpr = nyv_of(ny) // 2
    total = (nx - 2 * rows_from) * vpr
    nb = max(1, min((total + c["kBlock"] - 1) // c["kBlock"], cap))
    v = min(total - 1, int(fraction * total))
    if rows_from and (v % vpr) * 2 > ny - 2:
        v -= 1                                                  # the last vector of a row may hold no interior column
    i, j = rows_from + v // vpr, (v % vpr) * 2
    j = max(1, min(j + 1, ny - 2)) if rows_from else min(j, ny - 1)      # the vector's last interior column / its first cell
    return (v // c["kBlock"]) % nb, v // (c["kBlock"] * nb), (i, j)


# ---------------------------------------------------------------------------------------------- chain facts
def _tile_launch(shape, sets=1, offset=None, z=1):
    n = ntiles(shape)
    return dict(kind="tile", workgroups=n * z, partials=n, sets=sets, offset=n if offset is None else offset, chunks=1, partial_last=False)


def _stream_launch(items, cap, per_thread=1, sets=1, offset=None, partials=True):
    c = constants()
    blocks = (items + c["kBlock"] * per_thread - 1) // (c["kBlock"] * per_thread)
    nb = max(1, min(blocks, cap))
    return dict(kind="stream", workgroups=nb, partials=nb if partials else 0, sets=sets, offset=nb if offset is None else offset,
                chunks=(blocks + nb - 1) // nb, partial_last=blocks % nb != 0 or items % c["kBlock"] != 0)


def even(n):
    return (n + 1) & ~1


ENTRIES = ["pcg_direction", "pcg_direction_react", "pcg_update", "pcg_dots", "ho_direction", "ho_rhs", "ho_residual", "heat_rhs",
           "heat_rhs_var", "heat_diff_sumsq", "heat_ring", "flow_rhs", "flow_diag", "flow_interior", "flow_wall", "nl_eval", "rd_rhs",
           "rd_energy", "eig_gram_3x5", "eig_gram_18x36", "eig_combine", "eig_residual", "eig_apply"]
RING_ENTRIES = ("heat_ring", "flow_wall")            # a perimeter of work: they wrap on thin and tall alone
EIG_COLS = 3


def chain_facts(entry, shape):
    """the launches of mg_dev_<entry> on `shape` with the library's pitch, the launchers' formulas restated: per launch the
    workgroup count, the partials per set, the number of sets, the distance between sets and the number of chunks the busiest
    workgroup takes (partial_last: its last pass is not a full one)"""
    c = constants()
    nx, ny = shape
    vecs_all, vecs_in = nx * (nyv_of(ny) // 2), (nx - 2) * (nyv_of(ny) // 2)
    if entry in ("pcg_direction", "pcg_direction_react", "ho_direction", "ho_residual", "heat_rhs", "heat_rhs_var", "rd_rhs"):
        return [_tile_launch(shape)]
    if entry == "ho_rhs":
        return [dict(_tile_launch(shape), partials=0, sets=0)]
    if entry == "eig_apply":
        return [dict(_tile_launch(shape, z=EIG_COLS), partials=0, sets=0)]
    if entry == "pcg_update":
        return [_stream_launch(vecs_in, c["cap_pcg_stream"])]
    if entry == "pcg_dots":
        return [_stream_launch(vecs_in, c["cap_pcg_stream"], sets=2, offset=c["pcg_dots_second"])]
    if entry == "heat_diff_sumsq":
        return [_stream_launch(vecs_all, c["cap_heat_diff"])]
    if entry == "heat_ring":
        return [_stream_launch(2 * (nx + ny), c["cap_heat_ring"], partials=False)]
    if entry == "flow_wall":
        return [_stream_launch(2 * (nx + ny), c["cap_flow_wall"], partials=False)]
    if entry == "flow_rhs":
        return [_tile_launch(shape, sets=2)]
    if entry == "flow_diag":
        return [_stream_launch(vecs_in, c["cap_flow_stream"], sets=3)]
    if entry == "flow_interior":
        return [_stream_launch(vecs_all, c["cap_flow_stream"], sets=2)]
    if entry == "nl_eval":
        return [_tile_launch(shape, sets=2, offset=even(ntiles(shape)))]
    if entry == "rd_energy":
        return [_tile_launch(shape, sets=3, offset=even(ntiles(shape)))]
    if entry.startswith("eig_gram"):
        p, q = (int(v) for v in entry.split("_")[2].split("x"))
        pp, qp = (p + 15) // 16 * 16, (q + 15) // 16 * 16
        tiles = (nx - 2) * ((nyv_of(ny) + c["kEigKC"] - 1) // c["kEigKC"])
        nwg = max(1, min(tiles, c["kGramWorkgroups"], max_partials(nx, ny) // (pp * qp)))
        return [dict(kind="gram", workgroups=nwg, partials=nwg, sets=1, offset=pp * qp, block=pp * qp, chunks=(tiles + nwg - 1) // nwg,
                     partial_last=tiles % nwg != 0)]
    if entry == "eig_combine":
        return [_stream_launch(vecs_all, c["cap_eig_combine"], partials=False)]
    if entry == "eig_residual":
        return [_stream_launch(vecs_all, min(c["cap_eig_residual"], max_partials(nx, ny) // EIG_COLS), sets=EIG_COLS)]
    raise KeyError(entry)


# ---------------------------------------------------------------------------------------------- exact data
def ints(shape, k, span=5, scale=1.0):
    """integer-valued, nowhere 0: magnitude 1 + a position-dependent residue, seeded signs"""
    i, j = np.ogrid[:shape[0], :shape[1]]
    mag = 1 + ((7 + 2 * k) * i + (13 + 6 * k) * j + 3 * k) % span
    sign = 1 - 2 * np.random.default_rng(1000 + k).integers(0, 2, shape)
    return scale * (mag * sign).astype(np.float64)


def positive(shape, k, span=3, lo=1):
    """integers lo .. lo + span - 1 (a coefficient; with lo = 0 a weight with zeros)"""
    i, j = np.ogrid[:shape[0], :shape[1]]
    return (lo + ((3 + k) * i + (5 + 2 * k) * j + k) % span).astype(np.float64) + np.zeros(shape)


def _scaled_ints(a):
    a = np.asarray(a, dtype=np.float64)
    for bits in range(0, 40, 2):
        s = a * 2.0 ** bits
        if np.all(s == np.rint(s)) and float(np.max(np.abs(s), initial=0.0)) < 2.0 ** 31:
            return s.astype(np.int64), bits
    raise AssertionError("not a field of small dyadic numbers")


def exact_dot(a, b=None):
    """sum a b (b None: sum a) as a float, exact; refuses data for which a device sum in some order could round"""
    ia, fa = _scaled_ints(a)
    ib, fb = (np.ones_like(ia), 0) if b is None else _scaled_ints(b)
    prod = ia * ib                                           # below 2^62: exact in int64
    bound = int(np.sum(np.abs(prod).astype(object))) if prod.size < 1 << 10 else int(np.abs(prod).sum())
    assert bound < 2 ** 53, "the absolute sum reaches %g x 2^53 in units of 2^-%d" % (bound / 2.0 ** 53, fa + fb)
    total = int(prod.sum())
    out = total / 2.0 ** (fa + fb)
    assert int(out * 2.0 ** (fa + fb)) == total
    return out


def is_dyadic(x, bits=12):
    return float(x) * 2.0 ** bits == round(float(x) * 2.0 ** bits)


def ho_spacings():
    """hx = 1 and the hy next to sqrt(1/11) with fl(1 / fl(hy hy)) == 11 exactly: 1/hx^2 + 1/hy^2 = 12, so that the host's
    formulas give the weights cC, cE, cN, cK = 20, 1, -9, 1 (tests/test_scale_edges_cpu.py asserts it)"""
    h = math.sqrt(1.0 / 11.0)
    for cand in (h, math.nextafter(h, 0.0), math.nextafter(h, 1.0), math.nextafter(math.nextafter(h, 0.0), 0.0),
                 math.nextafter(math.nextafter(h, 1.0), 1.0)):
        if 1.0 / (cand * cand) == 11.0:
            return 1.0, cand
    raise AssertionError("no double near sqrt(1/11) gives 1/(h h) == 11")


HX, HY = 1.0, 0.5                 # 1/hx^2 = 1, 1/hy^2 = 4, diag = 10: x and y are told apart
SIGMA, BETA, ALPHA = 0.25, -0.5, 0.75
HEAT = dict(alpha=2.0, dt=0.25, g0=0.5, g1=1.5)
FLOW = dict(nu=0.5, dt=0.25, c0=1.5, c1=-0.5)
SPEEDS = (0.75, -1.25, 0.5, 1.5)
EDGE4 = (1.5, -2.25, 3.0, -0.5)
NLPAR = dict(coeff=-1.0, sigma=0.25, kappa=0.5, t=0.5)
RDPAR = dict(alpha=2.0, dt=0.25, kappa=0.5, rho=-1.5, g0=0.5, g1=1.5)
SCALARS = dict(HX=HX, HY=HY, SIGMA=SIGMA, BETA=BETA, ALPHA=ALPHA, **{"heat_" + k: v for k, v in HEAT.items()},
               **{"flow_" + k: v for k, v in FLOW.items()}, **{"nl_" + k: v for k, v in NLPAR.items()},
               **{"rd_" + k: v for k, v in RDPAR.items()}, **{"speed%d" % k: v for k, v in enumerate(SPEEDS)},
               **{"edge%d" % k: v for k, v in enumerate(EDGE4)})


def interior(a):
    return a[..., 1:-1, 1:-1]


# ---------------------------------------------------------------------------------------------- the cases
def case(entry, shape, variant=None):
    """inputs, expected fields (bit for bit) and expected sums (==) of one entry point on one shape.  `variant` selects the
    option set where an entry has more than one (see VARIANTS)."""
    if entry.startswith("eig_gram"):
        return _case_eig_gram(shape, entry)                      # (p, q) is part of the entry's name
    return globals()["_case_" + entry](shape, variant)


VARIANTS = {"pcg_direction": ["const", "var"], "pcg_direction_react": ["const", "var"], "pcg_dots": ["plain", "flex"],
            "heat_rhs": [HD.EXPLICIT, HD.CN, HD.BDF2], "heat_rhs_var": [HD.EXPLICIT, HD.CN, HD.BDF2], "nl_eval": ["linear", "cubic"],
            "rd_energy": ["plain", "aw"]}


def variants(entry):
    return VARIANTS.get(entry, [None])


def _direction(shape, var, react):
    z, p = PR.zero_ring(ints(shape, 1)), PR.zero_ring(ints(shape, 2))
    a = positive(shape, 3) if var else None
    c = positive(shape, 4, lo=0) if react else None
    want_p = PR.zero_ring(z + BETA * p)
    q = NL.apply_A(want_p, HX, HY, -1.0, SIGMA, a)
    if react:
        q = PR.zero_ring(q + c * want_p)
    return dict(inputs=dict(z=z, p=p, a=a, c=c), fields=dict(p=want_p, q=q), sums=dict(pq=exact_dot(want_p, q)))


def _case_pcg_direction(shape, variant):
    return _direction(shape, variant == "var", False)


def _case_pcg_direction_react(shape, variant):
    return _direction(shape, variant == "var", True)


def _case_pcg_update(shape, variant):
    p, q, r = (PR.zero_ring(ints(shape, k)) for k in (1, 2, 3))
    x = ints(shape, 4)
    want_x, want_r = x.copy(), r.copy()
    want_x[1:-1, 1:-1] = x[1:-1, 1:-1] + ALPHA * p[1:-1, 1:-1]
    want_r[1:-1, 1:-1] = r[1:-1, 1:-1] - ALPHA * q[1:-1, 1:-1]
    return dict(inputs=dict(p=p, q=q, r=r, x=x), fields=dict(x=want_x, r=want_r), sums=dict(rr=exact_dot(interior(want_r), interior(want_r))))


def _case_pcg_dots(shape, variant):
    r, z, q = (PR.zero_ring(ints(shape, k)) for k in (1, 2, 3))
    sums = dict(rz=exact_dot(r, z))
    if variant == "flex":
        sums["zq"] = exact_dot(z, q)
    return dict(inputs=dict(r=r, z=z, q=q), fields={}, sums=sums)


def _case_ho_direction(shape, variant):
    hx, hy = ho_spacings()
    z, p = ints(shape, 1), ints(shape, 2)                      # their rings are not read
    want_p = PR.zero_ring(z + BETA * p)
    q = HO.apply_A4(want_p, hx, hy, -1.0, 0.0)
    return dict(inputs=dict(z=z, p=p), fields=dict(p=want_p, q=q), sums=dict(pq=exact_dot(want_p, q)))


def _case_ho_rhs(shape, variant):
    f = ints(shape, 1)
    return dict(inputs=dict(f=f), fields=dict(g=HO.rhs_average(f)), sums={})


def _case_ho_residual(shape, variant):
    hx, hy = ho_spacings()
    x, g = ints(shape, 1), ints(shape, 2)
    r = HO.residual(x, g, hx, hy, -1.0, 0.0)
    return dict(inputs=dict(x=x, g=g), fields=dict(r=r), sums=dict(rr=exact_dot(r, r)))


def _heat(shape, scheme, var):
    u, up, S = ints(shape, 1), ints(shape, 2), ints(shape, 3)
    a = positive(shape, 4) if var else None
    h = HEAT
    if var:
        out = HV.rhs_var(scheme, u, h["dt"], h["alpha"], a, HX, HY, up, S, h["g0"], h["g1"])
    else:
        out = HD.rhs(scheme, u, h["dt"], h["alpha"], HX, HY, up, S, h["g0"], h["g1"])
    return dict(inputs=dict(u=u, up=up, S=S, a=a), fields=dict(out=out), sums=dict(sumsq=exact_dot(out, out)))


def _case_heat_rhs(shape, variant):
    return _heat(shape, variant, False)


def _case_heat_rhs_var(shape, variant):
    return _heat(shape, variant, True)


def _case_heat_diff_sumsq(shape, variant):
    a, b = ints(shape, 1), ints(shape, 2)
    return dict(inputs=dict(a=a, b=b), fields={}, sums=dict(sumsq=exact_dot(a - b, a - b)))


def _case_heat_ring(shape, variant):
    u = ints(shape, 1)
    return dict(inputs=dict(u=u), fields=dict(u=HD.set_ring(u.copy(), EDGE4)), sums={})


def _peak(psi, cell, big):
    """make |N - S| + |E - W| of `cell` the largest by far: +-big on its two y-neighbours (3 | big keeps the Jacobian exact)"""
    i, j = cell
    psi[i, j + 1], psi[i, j - 1] = big, -big
    return psi


FLOW_PEAK = 3000.0


def flow_fields(shape, peak=None, nan=None):
    """(psi, w, N_prev, F); psi in multiples of 3 so that the Jacobian's division by 12 hx hy is exact.  peak / nan: the cell
    whose velocity term is made the maximum / whose northern neighbour is NaN"""
    psi = ints(shape, 1, scale=3.0)
    if peak is not None:
        _peak(psi, peak, FLOW_PEAK)
    if nan is not None:
        psi[nan[0], nan[1] + 1] = np.nan
    return psi, ints(shape, 2), ints(shape, 3), ints(shape, 4)


def _case_flow_rhs(shape, variant, peak=None, nan=None):
    psi, w, Np, F = flow_fields(shape, peak, nan)
    k = FLOW
    f, N, _, m = FR.rhs(psi, w, k["nu"], k["dt"], HX, HY, k["c0"], k["c1"], Np, F)
    # a NaN in psi reaches the Jacobian of its neighbours and with it f and the sum of f^2: only the maximum is pinned then
    return dict(inputs=dict(psi=psi, w=w, Np=Np, F=F), fields=dict(f=f, N=N), sums={} if nan else dict(sumsq=exact_dot(f, f)),
                maxima=dict(m=m))


def _case_flow_diag(shape, variant, peak=None, nan=None):
    psi, w, _, _ = flow_fields(shape, peak, nan)
    return dict(inputs=dict(psi=psi, w=w), fields={}, sums=dict(e=exact_dot(interior(psi), interior(w)), z=exact_dot(interior(w), interior(w))),
                maxima=dict(m=FR.velocity_max(psi)))


def _case_flow_interior(shape, variant, peak=None, nan=None):
    w, old = ints(shape, 2), ints(shape, 3)
    if peak is not None:
        old[peak] = w[peak] + FLOW_PEAK
    if nan is not None:
        old[nan] = np.nan
    out = FR.interior(w)
    return dict(inputs=dict(w=w, old=old), fields=dict(out=out), sums=dict(sumsq=exact_dot(out, out)),
                maxima=dict(change=float(np.max(np.abs(w - old)))))


def _case_flow_wall(shape, variant):
    psi, w = ints(shape, 1), ints(shape, 2)
    return dict(inputs=dict(psi=psi, w=w), fields=dict(w=FR.wall(w.copy(), psi, HX, HY, FR.NO_SLIP, SPEEDS)), sums={})


def _case_nl_eval(shape, variant):
    kind = NL.KINDS[variant]
    u, delta, f = ints(shape, 1), ints(shape, 2), ints(shape, 3)
    a, w = positive(shape, 4), positive(shape, 5, lo=0)
    n = NLPAR
    e = NL.evaluate(kind, u, f, HX, HY, n["coeff"], n["sigma"], n["kappa"], a, w, delta, n["t"])
    return dict(inputs=dict(u=u, delta=delta, f=f, a=a, w=w), fields=dict(v=e["v"], F=e["F"], c=e["c"]),
                sums=dict(FF=exact_dot(e["F"], e["F"]), c=exact_dot(e["c"])))


def _case_rd_rhs(shape, variant):
    u, up, S = ints(shape, 1), ints(shape, 2), ints(shape, 3)
    a, w = positive(shape, 4), positive(shape, 5, lo=0)
    r = RDPAR
    out = RD.rhs(RD.CN, NL.CUBIC, u, r["dt"], r["alpha"], HX, HY, r["kappa"], r["rho"], up, S, a, w, r["g0"], r["g1"])
    return dict(inputs=dict(u=u, up=up, S=S, a=a, w=w), fields=dict(out=out), sums=dict(sumsq=exact_dot(out, out)))


def _case_rd_energy(shape, variant):
    u = ints(shape, 1)
    a, w = (positive(shape, 4), positive(shape, 5, lo=0)) if variant == "aw" else (None, None)
    G, P, Q = RD.energy_terms(NL.CUBIC, u, HX, HY, a, w)
    return dict(inputs=dict(u=u, a=a, w=w), fields={}, sums=dict(G=exact_dot(G), P=exact_dot(P), Q=exact_dot(Q)))


def columns(shape, n, k0):
    """n integer-valued columns (magnitude 1 .. 3, nowhere 0), every one another pattern: the residue of a line through the
    cell picks the magnitude, a seeded bit per row times a seeded bit per column the sign"""
    nx, ny = shape
    i, j = np.arange(nx), np.arange(ny)
    lut = np.array([1, 2, 3, 1, 2], dtype=np.int8)
    out = np.empty((n, nx, ny))
    for k in range(k0, k0 + n):
        rng = np.random.default_rng(2000 + k)
        m = (((7 + 2 * k) * i + k) % 3).astype(np.int8)[:, None] + (((13 + 6 * k) * j) % 3).astype(np.int8)[None, :]
        si, sj = (1 - 2 * rng.integers(0, 2, nx)).astype(np.int8), (1 - 2 * rng.integers(0, 2, ny)).astype(np.int8)
        out[k - k0] = lut[m] * (si[:, None] * sj[None, :])
    return out


def flow_case(entry, shape, peak=None, nan=None):
    """a flow case with the maximum moved to `peak`, or a NaN next to / at `nan`"""
    return globals()["_case_" + entry](shape, None, peak=peak, nan=nan)


# ---- mg_dev_pcg_scalars: synthetic partial arrays around the reduce kernel's strides
def scalar_lengths():
    r = constants()["kReduceBlock"]
    return [r - 1, r, r + 1, 2 * r - 1, 2 * r + 1, 3 * r + 21]


def partial_array(n, k):
    """n positive integers 1 .. 7, no two neighbouring lengths with the same sum"""
    return (1 + ((3 + 2 * k) * np.arange(n) + k) % 7).astype(np.float64)


def gram_exact(u, v):
    """ER.gram's product over interior cells as one matrix product: the same numbers, since every partial sum in any order is
    an integer below 2^53 (cells x max |u| x max |v|)"""
    a = np.ascontiguousarray(interior(u)).reshape(u.shape[0], -1)
    b = a if v is u else np.ascontiguousarray(interior(v)).reshape(v.shape[0], -1)
    amax, bmax = max(float(a.max()), -float(a.min())), max(float(b.max()), -float(b.min()))
    assert a.shape[1] * amax * bmax < 2.0 ** 53
    g = a @ b.T
    assert np.all(g == np.rint(g))
    return g


def _case_eig_gram(shape, entry):
    p, q = (int(t) for t in entry.split("_")[2].split("x"))
    v = columns(shape, q, 10)                       # u: the first p columns of v (one run of columns, staged once)
    return dict(inputs=dict(v=v, p=p, q=q), fields={}, sums=dict(G=gram_exact(v, v)[:p]))


COMBINE_P, COMBINE_Q = 6, 4


def _case_eig_combine(shape, variant):
    cols = np.stack([PR.zero_ring(c) for c in columns(shape, COMBINE_P, 20)])
    coef = (np.arange(COMBINE_P * COMBINE_Q).reshape(COMBINE_P, COMBINE_Q) % 7 - 3) * 0.25 + 0.125
    return dict(inputs=dict(cols=cols, coef=coef), fields=dict(out=ER.mix(cols, coef)), sums={})


def _case_eig_residual(shape, variant):
    x, ax = columns(shape, EIG_COLS, 30), columns(shape, EIG_COLS, 40)
    lam = np.array([1.5, -0.25, 4.0])
    r = np.zeros_like(x)
    r[:, 1:-1, 1:-1] = interior(ax) - lam[:, None, None] * interior(x)
    return dict(inputs=dict(x=x, ax=ax, lam=lam), fields=dict(r=r), sums=dict(sumsq=np.array([exact_dot(c, c) for c in r])))


def _case_eig_apply(shape, variant):
    cols = columns(shape, EIG_COLS, 50)
    want = np.stack([NL.apply_A(PR.zero_ring(c), HX, HY, -1.0, 0.0) for c in cols])
    return dict(inputs=dict(cols=cols), fields=dict(av=want), sums={})


# ============================================================================================== the drivers at 1281^2
# Closed forms of the discrete operators on the unit square: what tests/test_gpu_scale_drivers.py measures the drivers with
# (tests/test_scale_edges_cpu.py checks each against the NumPy restatements at 33 x 33).
EPS = float(np.finfo(np.float64).eps)
# roundings of one stencil evaluation (adds, multiplies and the subtraction from f; the variable-coefficient stencil also forms
# four face means and two diagonal sums; the nine-point one four more neighbours) ...
STENCIL_OPS = {"const": 10, "var": 24, "ho": 18}
# ... and the depth of the reduction chain behind a norm: 4 cells per thread, 6 shuffle steps per wave, 3 adds across the
# waves, and the second stage's per-thread chain (up to 2 x 2 terms at 1281^2), 6 shuffle steps and 15 adds across 16 waves
REDUCE_DEPTH = 4 + 6 + 3 + 4 + 6 + 15
DRIVER_STEPS = 4


def mode(nx, ny, k, l):
    """the discrete sine mode (k, l), with an exactly zero ring"""
    return ER.exact_vector(nx, ny, k, l)


def mode_defect(k, l):
    """how far (in the maximum norm) the computed mode may lie from the exact eigenvector: the arguments k pi i / (n - 1) are
    rounded (three roundings and pi's own, relative 2 eps of an argument up to k pi), so is each sine and their product"""
    return 2.0 * np.pi * (k + l + 1) * EPS


def lam_kl(nx, ny, k, l):
    """its eigenvalue under -Laplacian_h (five-point) on the unit square; k and l may be arrays"""
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    return 4.0 / hx ** 2 * np.sin(k * np.pi * hx / 2) ** 2 + 4.0 / hy ** 2 * np.sin(l * np.pi * hy / 2) ** 2


def lam4_kl(nx, ny, k, l, sigma=0.0):
    """its eigenvalue under the compact nine-point operator A4 (coeff = -1), from the weights of ho_reference.coefficients"""
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    cC, cE, cN, cK = HO.coefficients(hx, hy, sigma)
    cx, cy = np.cos(k * np.pi * hx), np.cos(l * np.pi * hy)
    return cC + 2.0 * cE * cx + 2.0 * cN * cy - 4.0 * cK * cx * cy


def avg_kl(nx, ny, k, l):
    """its eigenvalue under the right-hand-side average R of the compact scheme"""
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    return (8.0 + 2.0 * np.cos(k * np.pi * hx) + 2.0 * np.cos(l * np.pi * hy)) / 12.0


def lam_min(nx, ny, order=2):
    """the smallest eigenvalue of the operator: mode (1, 1) of the five-point one; the minimum over every mode of the nine-point one"""
    if order == 2:
        return float(lam_kl(nx, ny, 1, 1))
    k, l = np.arange(1, nx - 1)[:, None], np.arange(1, ny - 1)[None, :]
    return float(np.min(lam4_kl(nx, ny, k, l)))


def norm_h(v, nx, ny):
    return float(np.sqrt(np.sum(v * v) / ((nx - 1) * (ny - 1))))


def rounding_floor(nx, ny, kind, shift, amax, unorm):
    """c eps (4/hx^2 + 4/hy^2 + shift) max(a) ||u||: how far two correct evaluations of a residual norm of u may lie apart"""
    c = STENCIL_OPS[kind] + REDUCE_DEPTH
    return c * EPS * (4.0 * (nx - 1) ** 2 + 4.0 * (ny - 1) ** 2 + shift) * amax * unorm


PCG_MODES = [(1, 1, 1.0), (3, 2, 0.5), (0.47, 0.7, 0.05), (0.99, 0.99, 0.02)]      # (k, l, amplitude); fractions are of n - 2
PCG_REL_TOL = 1e-9
PCG_CONTRAST = 100.0


def _modes(nx, ny):
    out = []
    for k, l, amp in PCG_MODES:
        k = k if isinstance(k, int) else max(1, int(k * (nx - 2)))
        l = l if isinstance(l, int) else max(1, int(l * (ny - 2)))
        out.append((k, l, amp))
    return out


def pcg_problem(nx, ny, kind):
    """(u*, f, a, tol, floor) for kind "const", "var" (a checkerboard of contrast PCG_CONTRAST) or "ho" (order 4): u* a sum of
    low and high sine modes (plus seeded noise where the operator is applied in NumPy), f with A u* = f (order 4: R f = A4 u*,
    mode by mode), tol = PCG_REL_TOL ||f||_h and the rounding floor of a residual norm of u*"""
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    us = sum(amp * mode(nx, ny, k, l) for k, l, amp in _modes(nx, ny))
    a = None
    if kind == "ho":
        f = sum(amp * float(lam4_kl(nx, ny, k, l) / avg_kl(nx, ny, k, l)) * mode(nx, ny, k, l) for k, l, amp in _modes(nx, ny))
    else:
        us = us + PR.zero_ring(1e-3 * np.random.default_rng(7).standard_normal((nx, ny)))
        a = PR.checkerboard(nx, ny, contrast=PCG_CONTRAST) if kind == "var" else None
        f = NL.apply_A(us, hx, hy, -1.0, 0.0, a)
    amax = 1.0 if a is None else float(np.max(a))
    return us, f, a, PCG_REL_TOL * norm_h(f, nx, ny), rounding_floor(nx, ny, kind, 0.0, amax, norm_h(us, nx, ny))


def np_residual(kind, u, f, a=None, shift=0.0, kappa=0.0, w=None, nl="linear"):
    """f - N(u) on interior cells by the modules' NumPy references"""
    nx, ny = u.shape
    hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    if kind == "ho":
        return HO.residual(u, HO.rhs_average(f), hx, hy, -1.0, shift)
    if kappa:
        return NL.evaluate(NL.KINDS[nl], u, f, hx, hy, -1.0, shift, kappa, a, w)["F"]
    return PR.zero_ring(f - NL.apply_A(u, hx, hy, -1.0, shift, a))


# ---- time steppers on one eigenmode: u_k = c_k u_0
def heat_factors(scheme, dt, alpha, lam, steps=DRIVER_STEPS):
    """[c_0 .. c_steps] of the heat stepper on a mode with eigenvalue lam; BDF2 starts with one Crank-Nicolson step"""
    z = dt * alpha * lam
    c = [1.0]
    for k in range(steps):
        if scheme == HD.IMPLICIT:
            c.append(c[-1] / (1.0 + z))
        elif scheme == HD.CN or k == 0:
            c.append(c[-1] * (1.0 - z / 2) / (1.0 + z / 2))
        else:
            c.append((4.0 * c[-1] - c[-2]) / (3.0 + 2.0 * z))
    return c


def heat_scheme_of_step(scheme, k):
    return HD.CN if scheme == HD.BDF2 and k == 0 else scheme


def rd_factors(scheme, dt, alpha, lam, kappa, rho, steps=DRIVER_STEPS):
    """the same for the reaction-diffusion stepper with the linear kind: rd_reference.eigen_factor step by step (Crank-Nicolson
    extrapolates the explicit term from two levels once it has them; BDF2 starts with one Crank-Nicolson step)"""
    c = [1.0]
    for k in range(steps):
        if scheme == RD.IMPLICIT:
            g = RD.eigen_factor(RD.IMPLICIT, dt, alpha, lam, kappa, rho)
        elif scheme == RD.CN or k == 0:
            g = RD.eigen_factor(RD.CN, dt, alpha, lam, kappa, rho, None if k == 0 else c[-2] / c[-1])
        else:
            g = RD.eigen_factor(RD.BDF2, dt, alpha, lam, kappa, rho, c[-2] / c[-1])
        c.append(c[-1] * g)
    return c


def flow_factor(nu, dt, lam):
    """Crank-Nicolson on the vorticity of an eigenmode: Arakawa's J(psi, c psi) is 0, so the Adams-Bashforth term is 0 on the
    first step (c0 = 1, c1 = 0) as on every other and each step multiplies w by this factor"""
    return (1.0 - nu * dt * lam / 2) / (1.0 + nu * dt * lam / 2)


def carry_of(scheme, k, dt=None, rho=0.0, dmin=0.0):
    """(g1, g2): an error E_k, E_{k-1} in the levels a step reads comes out of the exact step as at most g1 E_k + g2 E_{k-1}.
    Heat (rho = 0): |g| <= 1 on every mode for implicit Euler and Crank-Nicolson, (4, 1) / 3 for BDF2.  With an explicit
    linear term rho u (reaction-diffusion; dmin = alpha lambda_min + kappa bounds the implicit operator from below) the
    numerators grow by the extrapolation's weights times |rho| and the bound is taken at dmin, where it is largest."""
    sch = heat_scheme_of_step(scheme, k)
    r = abs(rho)
    if sch == HD.IMPLICIT:
        return (1.0 if not r else max(1.0, (1.0 + dt * r) / (1.0 + dt * dmin)), 0.0)
    if sch == HD.CN:
        if not r:
            return (1.0, 0.0)
        two = k > 0                                             # a previous level: E = (3 u - u_prev) / 2
        return (max(1.0, (abs(2.0 / dt - dmin) + (3.0 if two else 2.0) * r) / (2.0 / dt + dmin)), (r / (2.0 / dt + dmin)) if two else 0.0)
    if not r:
        return (4.0 / 3.0, 1.0 / 3.0)
    return ((4.0 / (2 * dt) + 2 * r) / (3.0 / (2 * dt) + dmin), (1.0 / (2 * dt) + r) / (3.0 / (2 * dt) + dmin))


def stepper_bound(tol, shifts, lmin, fnorms, unorms, lipschitz, carries, nx, ny, extra=None):
    """E_steps of E_{k+1} <= g1 E_k + g2 E_{k-1} + delta_k (carries[k] = (g1, g2), see carry_of), where step k + 1 adds
    delta_k = (tol max(1, ||f_k|| + L E_k) + floor_k + extra_k) / (shift_k + lambda_min): its solve stops at
    ||r|| < tol max(1, ||f||_h), an error is at most ||r||_h / lambda_min(-Lap_h + shift), ||f|| is the closed form's plus what
    the error so far adds (L bounds the right-hand side's map), floor_k is the rounding floor of a residual norm at that state
    and extra_k a perturbation of f the caller measured (the flow's Jacobian)"""
    E = [0.0, 0.0]
    for k in range(len(fnorms)):
        floor = rounding_floor(nx, ny, "const", shifts[k], 1.0, unorms[k])
        delta = (tol * max(1.0, fnorms[k] + lipschitz * E[-1]) + floor + (extra[k] if extra else 0.0)) / (shifts[k] + lmin)
        E.append(carries[k][0] * E[-1] + carries[k][1] * E[-2] + delta)
    return E[-1]
