"""Call-level cases for every mg_dev_* kernel entry point (include/mghip.h), the driver that runs one case through an
`ops` object (tests/dist_helpers.NumpyOps on CPU tensors, distributed.HipOps on device tensors) and the comparison both
tests/test_dev_calls_cpu.py and tests/test_gpu_dev_calls.py use.  Plain Python + NumPy; torch is imported where tensors
are built, nothing here touches a GPU by itself.

A case is a dict: entry point, dtypes, shapes, pitch kinds, spacings, every integer argument, the seed of its fields and
its disposition -- "compare" or "refuse", decided from the header's rules (REFUSALS below), never from a return code.
MG_FUZZ_SEED shifts the seeded choices, MG_FUZZ_DEV scales the number of seeded extra cases (default list = what CI runs).
"""
import math
import os

import numpy as np

SIDE_ILO, SIDE_IHI, SIDE_JLO, SIDE_JHI = 1, 2, 4, 8
NPDT = {"f32": np.dtype(np.float32), "f64": np.dtype(np.float64)}
ESIZE = {"f32": 4, "f64": 8}
GUARD = 4                      # guard rows before and after every array of a call
BIG = 1 << 30

# ---- the kernels' own geometry (csrc/mg_kernels.hpp, csrc/mg_rb_kernels.hpp, csrc/mg_launch.hip) --------------------------
K_TI = 32                      # kTI: tile rows of the single operators (jacobi / rbgs_colour / residual kernels, TileShape)
TILE_ROW_BYTES = 512           # kTileRowBytes: TJ = 64 fp64 / 128 fp32 columns per LDS tile (TileShape, FusedShape)
FUSED_TI = {"tiny": 8, "small": 16, "large": 32}     # kFusedTITiny / kFusedTISmall / kFusedTI
TINY_CELLS = 520 * 520         # tiny_tiles(): 8-row tiles up to 520^2 cells
SMALL_CELLS = 1100 * 1100      # small_tiles(): 16-row tiles up to 1100^2 cells; use_rb(): register-blocked above
RB_STREAM_BYTES = 100 << 20    # rb_stream(): nx * ld * esize above 100 MB -> streaming hints
RB_LANES = 64 - 2 * 4          # RbShape: HL = 4 halo lanes per side -> TJ = 56 * N columns (112 fp64 / 224 fp32)
SPAN_TI, SPAN_BAND = 8 * 8 - 2 * 6, 4    # spanning leg: 8 waves x 8 rows, halo 6 -> 52 tile rows; tiles numbered down bands of 4 tile rows


def vec(dt):
    return 16 // ESIZE[dt]


def pitch(kind, dt, ny):
    """row pitch in elements: "lib" = mg_pitch_elems (rows on 512-byte boundaries), "min" = the least the header allows
    (ny rounded up to 16 bytes: the pad is shorter than one vector), "mid" = three vectors more than that"""
    es = ESIZE[dt]
    if kind == "lib":
        return (ny * es + 511) // 512 * 512 // es
    mn = (ny * es + 15) // 16 * 16 // es
    return mn if kind == "min" else mn + 3 * vec(dt)


def leg_family(case):
    """the kernel family a leg of this shape runs as (launch_leg_sized: register-blocked above 1100^2 cells, else 8-row tiles
    up to 520^2 cells, else 16-row tiles; the 32-row LDS tiles are never chosen for an mg_dev_* leg)"""
    cells = case["nx"] * case["ny"]
    if cells > SMALL_CELLS:
        return "rb"
    return "tiny" if cells <= TINY_CELLS else "small"


def leg_tiles(case):
    """(family, tile rows, tile columns) of the kernel that stores the `out` arrays of this call"""
    entry, dt = case["entry"], case.get("dt", "f64")
    lds_tj, rb_tj = TILE_ROW_BYTES // ESIZE[dt], RB_LANES * vec(dt)
    if entry == "span_leg":
        return "rb", SPAN_TI, rb_tj
    if entry == "jacobi":        # jacobi_rb: the register-blocked sweeps kernel (4 waves x 8 rows, halo 2) where the arrays stream
        streams = case["nx"] * case["ny"] > SMALL_CELLS and case["nx"] * pitch(case.get("pf", "lib"), dt, case["ny"]) * ESIZE[dt] > RB_STREAM_BYTES
        return ("rb", 4 * 8 - 2 * 2, rb_tj) if streams else ("tile", K_TI, lds_tj)
    fam = leg_family(case)
    if fam != "rb":
        return fam, FUSED_TI[fam], lds_tj
    hs = 2 if case.get("sm") == 1 else 1                               # sweep_halo
    halo = 2 * hs + (2 if entry == "down_leg" else (1 if case.get("window") else 0))
    if case.get("var"):
        rows = 8 * 4                                                   # variable coefficients: 8 waves x 4 rows
    else:
        rows = (8 if (case.get("sm") == 1 and dt == "f64") else 4) * 8  # MG_EXP_RB_W waves x 8 rows
    return fam, rows - 2 * halo, rb_tj


def tile_of(case, i, j):
    """human-readable tile / region of fine cell (i, j) for a failure message"""
    entry, dt = case["entry"], case.get("dt", "f64")
    if entry in ("down_leg", "up_leg", "span_leg"):
        fam, ti, tj = leg_tiles(case)
        nti, ntj = (case["nx"] - 2 + ti - 1) // ti, (case["ny"] - 1 + tj - 1) // tj
        a, b = max(i - 1, 0) // ti, j // tj
        rim = a in (0, nti - 1) or b in (0, ntj - 1)
        return f"{fam} tiles {ti}x{tj}: tile ({a},{b}) of {nti}x{ntj}{' (rim)' if rim else ''}"
    if entry in ("jacobi", "rbgs_colour", "residual"):
        tj = TILE_ROW_BYTES // ESIZE[dt]
        return f"tile ({i // K_TI},{j // tj}) of {K_TI}x{tj} tiles"
    return "vector %d of its row" % (j // vec(case.get("dtc", dt)))


# ---- shapes, chosen against that geometry ---------------------------------------------------------------------------
# smaller than one tile in one or both directions; one short of / exactly / one past a multiple of the tile extent:
# rows nx - 2 = 8 k (8-row tiles: every shape of at most 520^2 cells); columns ny - 1 = 64 k (fp64) / 128 k (fp32); odd and even extents
LEG_SHAPES_TINY = [(3, 3), (3, 4), (4, 3), (5, 9), (9, 10), (10, 11), (11, 64), (17, 65), (18, 66), (19, 128), (26, 129), (33, 130),
                   (6, 257), (66, 7), (130, 200)]
LEG_SHAPES_LONG = [(5, 30001), (30001, 5), (4, 20000)]                 # a few rows x tens of thousands of columns and back
# the 16-row tiles serve 520^2 < cells <= 1100^2 only: rows nx - 2 = 16 k - 1 / 16 k / 16 k + 1 (529, 530, 531), columns
# ny - 1 = 512 +- 1 (a multiple of both 64 and 128), two elongated arrays, one with several tile columns and a 2-cell last one
LEG_SHAPES_SMALL = [(530, 513), (529, 514), (531, 512), (8, 40000), (40000, 8), (546, 643)]
LEG_SHAPES_THRESH = [(520, 520), (521, 520), (1100, 1100)]           # last 8-row shape, first 16-row shape, last LDS-tiled shape
# register-blocked (above 1100^2 cells): tile rows 24-28 (Jacobi legs) / 52 (fp64 red-black, spanning leg), tile columns 112 / 224.
# (1102, 1122): 22 spanning tile rows (not a multiple of the band height 4), last fp64 tile column 1 cell wide ((ny - 1) % 112 = 1);
# (1123, 1103): 22 tile rows, last fp64 column 94, fp32 ((ny - 1) % 224 = 206); (1107, 1123): fp32 last column 2 cells ((1122) % 224 = 2)
RB_SHAPES = [(1101, 1100), (1102, 1122), (1123, 1103), (1107, 1123), (700, 1800), (1800, 700), (2050, 600), (1250, 1011)]
STREAM_SHAPE = (3700, 3600)    # fp64, lib pitch 3648: 3700 * 3648 * 8 B = 103 MiB > rb_stream's threshold
OP_SHAPES = [(3, 3), (4, 5), (33, 64), (34, 65), (35, 66), (32, 129), (66, 130), (7, 20001), (20001, 6), (300, 517)]

SPACINGS = {                   # name -> (hx, hy, dyadic)
    "eq": (1.0 / 32, 1.0 / 32, True),           # dyadic, hx = hy: the diagonal is a power of two (exact reciprocal)
    "neq": (1.0 / 64, 1.0 / 16, True),          # dyadic, hx != hy: true division by the diagonal
    "nd": (0.013, 0.0171, False),               # non-dyadic
}
OMEGAS = [2.0 / 3.0, 0.8, 1.0, 1.15]
PITCHES = ["lib", "min", "mid"]
DT = ["f64", "f32"]
INTERP_OK = [("f64", "f64", "f64"), ("f32", "f32", "f32"), ("f32", "f32", "f64"), ("f32", "f64", "f64"), ("f64", "f32", "f64")]   # (coarse, fine, compute)
# the combinations the header documents as unsupported: fp32 interpolation of fp64 fields; the spanning leg with red-black GS,
# mixed dtypes, or at most 1100^2 cells.  Literal: every "refuse" case of the list comes from here.
REFUSALS = [
    dict(entry="prolong_add", dtc="f64", dt="f64", comp="f32"),
    dict(entry="prolong_add", dtc="f32", dt="f64", comp="f32"),
    dict(entry="prolong_add", dtc="f64", dt="f32", comp="f32"),
    dict(entry="up_leg", dtc="f64", dt="f64", comp="f32"),
    dict(entry="up_leg", dtc="f32", dt="f64", comp="f32"),
    dict(entry="up_leg", dtc="f64", dt="f32", comp="f32", var=True),
    dict(entry="span_leg", sm=1, dt="f64", dtc="f64", comp="f64", nx=1102, ny=1122),
    dict(entry="span_leg", sm=0, dt="f64", dtc="f32", comp="f64", nx=1102, ny=1122),
    dict(entry="span_leg", sm=0, dt="f32", dtc="f64", comp="f64", nx=1102, ny=1122),
    dict(entry="span_leg", sm=0, dt="f64", dtc="f64", comp="f32", nx=1102, ny=1122),
    dict(entry="span_leg", sm=0, dt="f64", dtc="f64", comp="f64", nx=1100, ny=1100),
    dict(entry="span_leg", sm=0, dt="f32", dtc="f32", comp="f32", nx=257, ny=300),
]
ENTRIES = ["jacobi", "rbgs_colour", "residual", "residual_mixed", "sumsq", "restrict", "prolong_add", "convert", "inject_ring",
           "var_rdiag", "down_leg", "down_leg_var", "up_leg", "up_leg_var", "span_leg"]


def entry_name(case):
    """the name of section "Why" of the issue: the *_var legs are entries of their own"""
    return case["entry"] + ("_var" if case.get("var") else "")


def coarse_extent(n, off, how):
    """coarse extent for fine extent n and offset off: "fit" = (n + 1) / 2 + off, "large" two more (coarse cells without a
    complete fine neighbourhood / beyond the fine array), "small" one or two fewer (fine cells without a coarse parent)"""
    base = (n + 1) // 2 + off
    return max(3, {"fit": base, "large": base + 2, "small": base - 1, "smaller": base - 2}[how])


def leg_windows(nx, ny):
    return {"full": (1, nx - 1, 1, ny - 1), "sub": (nx // 3, nx // 3 + max(1, nx // 2), ny // 4 + 1, ny // 4 + 1 + max(1, ny // 2)),
            "ring": (0, nx, 0, ny), "empty": (min(5, nx - 1), min(5, nx - 1), 1, ny - 1)}


SPLIT_SHAPES = [(200, 600), (600, 700), (1102, 1122)]         # 8-row tiles, 16-row tiles, register-blocked


def split_rects(nx, ny, sides, G, d):
    """inner_rect of the launch split: what DistributedMultigrid._down_legs builds for ghost width G (owned cells, -2^30 /
    2^30 on physical sides), the same a cell larger / smaller, one without a whole tile, the whole array"""
    own = (-BIG if sides & SIDE_ILO else G - d, BIG if sides & SIDE_IHI else nx - G + d,
           -BIG if sides & SIDE_JLO else G - d, BIG if sides & SIDE_JHI else ny - G + d)
    return [("own_G%d%+d" % (G, d), own), ("notile", (nx // 2, nx // 2 + 2, ny // 2, ny // 2 + 2)), ("whole", (-BIG, BIG, -BIG, BIG))]


def _cases(seed, scale):
    rng = np.random.default_rng(seed)
    out = []

    def pick(seq):
        return seq[int(rng.integers(0, len(seq)))]

    def add(entry, **kw):
        c = dict(entry=entry, disp="compare", **kw)
        sp = c.setdefault("sp", "eq")
        c["hx"], c["hy"], c["dyadic"] = SPACINGS[sp]
        c["seed"] = 7919 * len(out) + seed
        tag = "-".join(str(c[k]) for k in ("dt", "dtc", "comp", "nx", "ny", "nxc", "nyc", "pf", "pc", "sides", "tag") if k in c)
        c["id"] = "%s%s-%03d-%s" % (entry, "_var" if c.get("var") else "", len(out), tag)
        out.append(c)
        return c

    # ---- single operators on one array shape -----------------------------------------------------------------------
    big_ops = [(1201, 1010)]
    for k, (nx, ny) in enumerate(OP_SHAPES + big_ops):
        for dt in DT:
            pf = PITCHES[(k + (dt == "f32")) % 3]
            sp = ("eq", "neq", "nd")[k % 3]
            add("jacobi", dt=dt, nx=nx, ny=ny, pf=pf, sp=sp, omega=OMEGAS[k % 4])
            add("rbgs_colour", dt=dt, nx=nx, ny=ny, pf=PITCHES[(k + 1) % 3], sp=("neq", "nd", "eq")[k % 3], omega=OMEGAS[(k + 1) % 4],
                colour=k % 2, poff=(k // 2) % 2)
            add("residual", dt=dt, nx=nx, ny=ny, pf=PITCHES[(k + 2) % 3], sp=("nd", "eq", "neq")[k % 3], coeff=(-1.0, 0.37)[k % 2])
            add("var_rdiag", dt=dt, nx=nx, ny=ny, pf=pf, sp=sp, sigma=(0.0, 2.5)[k % 2])
        add("residual_mixed", dt="f32", dtc="f64", nx=nx, ny=ny, pf=PITCHES[k % 3], pc=PITCHES[(k + 1) % 3], sp=("eq", "nd", "neq")[k % 3],
            coeff=(-1.0, 1.5)[k % 2])
        for m, (dti, dto) in enumerate([(a, b) for a in DT for b in DT]):
            if (k + m) % 2 == 0:
                add("convert", dt=dti, dtc=dto, nx=nx, ny=ny, pf=PITCHES[(k + m) % 3], pc=PITCHES[(k + 2 * m + 1) % 3])
    add("jacobi", dt="f64", nx=STREAM_SHAPE[0], ny=STREAM_SHAPE[1], pf="lib", sp="eq", omega=0.8, tag="stream")   # jacobi_rb: the register-blocked sweep

    # ---- sum of squares: windows of any kind -----------------------------------------------------------------------
    for k, (nx, ny) in enumerate([(9, 10), (33, 66), (65, 131), (300, 517), (7, 20001), (2000, 9)]):
        for dt in DT:
            wins = {"full": (0, nx, 0, ny), "row": (nx // 2, nx // 2 + 1, 0, ny), "col": (0, nx, ny // 3, ny // 3 + 1),
                    "odd": (1, nx - 1, 3, ny - 2), "empty": (2, 2, 1, ny - 1), "interior": (1, nx - 1, 1, ny - 1), "oddcol1": (0, nx, 5, 6)}
            for m, (name, w) in enumerate(wins.items()):
                if (k + m) % 2 == 0 or name in ("empty",) and k < 2:
                    add("sumsq", dt=dt, nx=nx, ny=ny, pf=PITCHES[(k + m) % 3], window=w, tag=name)

    # ---- transfers: all 16 side masks, all dtype pairs, coarse extents that fit or fall short ----------------------------
    tshapes = [(5, 5), (9, 12), (17, 33), (34, 65), (65, 130), (130, 67), (7, 4001), (4001, 8), (257, 300), (12, 9), (33, 17), (66, 35),
               (129, 66), (21, 258), (258, 21), (515, 131)]
    for sides in range(16):
        nxf, nyf = tshapes[sides]
        dti, dto = [(a, b) for a in DT for b in DT][sides % 4]
        # restriction: the launcher refuses coarse arrays that reach beyond the fine one, so extents fit or are smaller
        nxc = min(coarse_extent(nxf, 0, ("fit", "small", "fit", "smaller")[sides % 4]), nxf // 2 + 1 if not sides & SIDE_IHI else (nxf + 1) // 2)
        nyc = min(coarse_extent(nyf, 0, ("fit", "fit", "small", "small")[(sides // 4) % 4]), nyf // 2 + 1 if not sides & SIDE_JHI else (nyf + 1) // 2)
        add("restrict", dt=dti, dtc=dto, nx=nxf, ny=nyf, nxc=max(nxc, 2), nyc=max(nyc, 2), pf=PITCHES[sides % 3], pc=PITCHES[(sides // 3) % 3], sides=sides)
        dtc, dtf, comp = INTERP_OK[sides % 5]
        add("prolong_add", dtc=dtc, dt=dtf, comp=comp, nx=nxf, ny=nyf, nxc=coarse_extent(nxf, 0, ("fit", "large", "small", "fit")[sides % 4]),
            nyc=coarse_extent(nyf, 0, ("fit", "small", "large", "fit")[(sides // 2) % 4]), pf=PITCHES[(sides + 1) % 3], pc=PITCHES[(sides // 2) % 3], sides=sides)
        ci, cj = sides % 4, (sides // 4 + sides) % 4
        add("inject_ring", dt=dti, dtc=dto, nx=nxf, ny=nyf, nxc=coarse_extent(nxf, ci, ("fit", "large", "small", "fit")[(sides // 2) % 4]),
            nyc=coarse_extent(nyf, cj, ("large", "fit", "fit", "small")[sides % 4]), pf=PITCHES[(sides + 2) % 3], pc=PITCHES[sides % 3], sides=sides, ci=ci, cj=cj)
    for k in range(8):       # the same transfers at sizes with many vectors per row, both extremes of pitch
        nxf, nyf = [(300, 517), (517, 300), (1025, 260), (64, 2049)][k % 4]
        sides = (15, 0, 5, 10, 6, 9, 3, 12)[k]
        dti, dto = [(a, b) for a in DT for b in DT][(k + 1) % 4]
        add("restrict", dt=dti, dtc=dto, nx=nxf, ny=nyf, nxc=(nxf + 1) // 2, nyc=(nyf + 1) // 2, pf=("min", "lib")[k % 2], pc=("lib", "min")[k % 2], sides=sides)
        dtc, dtf, comp = INTERP_OK[(k + 2) % 5]
        add("prolong_add", dtc=dtc, dt=dtf, comp=comp, nx=nxf, ny=nyf, nxc=(nxf + 1) // 2, nyc=(nyf + 1) // 2, pf=("min", "lib")[k % 2], pc=("min", "mid")[k % 2], sides=sides)

    # ---- fused legs ------------------------------------------------------------------------------------------------
    def leg_common(k, nx, ny, dt, var=False):
        ci, cj = (k % 4, (k // 4 + 1) % 4) if k % 3 else (0, 0)
        hows = ("fit", "large", "small", "fit", "smaller", "large")
        c = dict(dt=dt, nx=nx, ny=ny, ci=ci, cj=cj, nxc=coarse_extent(nx, ci, hows[k % 6]), nyc=coarse_extent(ny, cj, hows[(k // 2 + 1) % 6]),
                 pf=PITCHES[k % 3], pc=PITCHES[(k // 3 + 1) % 3], sm=(k // 2) % 2, omega=OMEGAS[k % 4], poff=(k // 3) % 2,
                 coeff=(-1.0, -1.0, 0.6)[k % 3], sp=("eq", "neq", "nd", "eq")[k % 4])
        if var:
            c["var"] = True
        return c

    small_shapes = LEG_SHAPES_TINY + LEG_SHAPES_LONG + LEG_SHAPES_SMALL + LEG_SHAPES_THRESH
    down_dt = [(a, b) for a in DT for b in DT]
    k = 0
    for rep, shapes in enumerate((small_shapes, small_shapes[::2], RB_SHAPES)):
        for nx, ny in shapes:
            rb = shapes is RB_SHAPES
            for var in ((False, True) if (rep == 0 and nx * ny <= 360000) or (rb and k % 4 == 0) else (False,)):
                dt, dtc = down_dt[(k + rep) % 4]
                c = leg_common(k, nx, ny, dt, var)
                add("down_leg", dtc=dtc, nsweep=(2, 1, 0, 2)[k % 4], zero_init=int(k % 5 == 1), rect=None, **c)
                k += 1
    # the 16-row family with every dtype pair, both operators
    for m, (dt, dtc) in enumerate(down_dt + down_dt):
        c = leg_common(3 * m + 1, *LEG_SHAPES_SMALL[m % 3], dt, m >= 4)
        add("down_leg", dtc=dtc, nsweep=2 - m % 2, zero_init=int(m == 5), rect=None, tag="small16", **c)
    # the launch split: the rectangles DistributedMultigrid._down_legs builds for ghost widths 2 .. 8, each also a cell larger and
    # a cell smaller, one without a whole tile, the whole array -- on an 8-row, a 16-row and a register-blocked shape, every one
    # large enough for select = 1 to find tiles whose staged region lies inside the rectangle
    masks = (0, 15, 5, 10, 9, 6, 1, 14, 7, 8, 2, 13, 4, 11, 3, 12)
    for fam, (nx, ny) in (("tiny", SPLIT_SHAPES[0]), ("small", SPLIT_SHAPES[1]), ("rb", SPLIT_SHAPES[2])):
        m = 0
        for G in range(2, 9):
            for d in (0, 1, -1):
                sides = masks[(m + len(fam)) % 16]
                name, rect = split_rects(nx, ny, sides, G, d)[0]
                dt, dtc = down_dt[m % 4]
                c = leg_common(2 * m + (fam == "small"), nx, ny, dt, m % 3 == 1)
                add("down_leg", dtc=dtc, nsweep=(2, 1)[m % 5 == 4], zero_init=int(m % 7 == 3), rect=rect, rect_sides=sides, G=G, d=d, tag=name, **c)
                m += 1
        for m, which in enumerate((1, 2, 1, 2)):
            name, rect = split_rects(nx, ny, 15, 4, 0)[which]
            dt, dtc = down_dt[m]
            c = leg_common(5 + m, nx, ny, dt, m >= 2)
            add("down_leg", dtc=dtc, nsweep=2, zero_init=0, rect=rect, rect_sides=15, tag=name, **c)
    k = 0
    for rep, shapes in enumerate((small_shapes, small_shapes[1::2], RB_SHAPES)):
        for nx, ny in shapes:
            rb = shapes is RB_SHAPES
            for var in ((False, True) if (rep == 0 and nx * ny <= 360000) or (rb and k % 4 == 1) else (False,)):
                dtc, dt, comp = INTERP_OK[(k + rep) % 5]
                c = leg_common(k + 1, nx, ny, dt, var)
                wname = ("full", "sub", "none", "ring", "empty", "full")[k % 6]
                add("up_leg", dtc=dtc, comp=comp, nsweep=(2, 1, 2, 0)[k % 4], sides=k % 16, window=None if wname == "none" else leg_windows(nx, ny)[wname],
                    tag=wname, **c)
                k += 1
    for sides in range(16):       # every side mask on a shape with several tiles per direction, both families of tile
        nx, ny = ((41, 150), (150, 41))[sides % 2]
        dtc, dt, comp = INTERP_OK[sides % 5]
        c = leg_common(2 * sides + 1, nx, ny, dt)
        add("up_leg", dtc=dtc, comp=comp, nsweep=1 + sides % 2, sides=sides, window=leg_windows(nx, ny)[("full", "sub", "ring")[sides % 3]], tag="sides", **c)

    for sides in range(16):       # ... and on the 16-row tiles, with every interpolation dtype combination and both operators
        nx, ny = LEG_SHAPES_SMALL[sides % 3]
        dtc, dt, comp = INTERP_OK[(sides + 2) % 5]
        c = leg_common(2 * sides + 3, nx, ny, dt, sides % 4 == 3)
        add("up_leg", dtc=dtc, comp=comp, nsweep=1 + sides % 2, sides=sides, window=leg_windows(nx, ny)[("sub", "full", "ring")[sides % 3]], tag="sides16", **c)

    # ---- the spanning leg: register-blocked shapes only; half of the cases carry sub-domain arguments --------------------
    span_dt = [("f64", "f64"), ("f32", "f32"), ("f32", "f64")]       # (field dtype, interpolation dtype)
    k = 0
    for rep in range(2):
        for nx, ny in RB_SHAPES:
            dt, comp = span_dt[k % 3]
            sub = k % 2 == 1
            ci, cj = ((1 + k % 3, (k // 2) % 4) if sub else (0, 0))
            wname = ("full", "sub", "ring", "empty", "sub", "full")[k % 6]
            add("span_leg", dt=dt, dtc=dt, comp=comp, nx=nx, ny=ny, ci=ci, cj=cj, sm=0,
                nxc=coarse_extent(nx, ci, ("fit", "large", "fit", "small")[k % 4] if sub else "fit"),
                nyc=coarse_extent(ny, cj, ("fit", "small", "fit", "large")[k % 4] if sub else "fit"),
                pf=PITCHES[k % 3], pc=PITCHES[(k + 1) % 3], omega=OMEGAS[k % 4], poff=k % 2, coeff=-1.0, sp=("eq", "neq", "nd", "eq")[(k + rep) % 4],
                nsweep=(2, 1, 2, 2)[k % 4], nsweep_pre=(2, 2, 1, 2)[k % 4], sides=(3 * k + 1) % 16 if sub else 15, window=leg_windows(nx, ny)[wname],
                tag=wname + ("-sub" if sub else ""))
            k += 1
    for sides in (1, 3, 5, 7, 9, 11, 13, 6):      # the remaining masks (with the loop above: all 16)
        nx, ny = RB_SHAPES[1 + sides % 3]
        dt, comp = span_dt[sides % 3]
        add("span_leg", dt=dt, dtc=dt, comp=comp, nx=nx, ny=ny, ci=sides % 3, cj=(sides // 3) % 4, sm=0, nxc=coarse_extent(nx, sides % 3, "fit"),
            nyc=coarse_extent(ny, (sides // 3) % 4, "fit"), pf=PITCHES[sides % 3], pc="min", omega=0.8, poff=sides % 2, coeff=-1.0, sp="eq",
            nsweep=2, nsweep_pre=2, sides=sides, window=leg_windows(nx, ny)["sub"], tag="sides-sub")
    nx, ny = STREAM_SHAPE
    add("span_leg", dt="f64", dtc="f64", comp="f64", nx=nx, ny=ny, ci=0, cj=0, sm=0, nxc=coarse_extent(nx, 0, "fit"), nyc=coarse_extent(ny, 0, "fit"),
        pf="lib", pc="lib", omega=0.8, poff=0, coeff=-1.0, sp="eq", nsweep=2, nsweep_pre=2, sides=15, window=leg_windows(nx, ny)["full"], tag="stream")

    # ---- seeded extras (MG_FUZZ_DEV > 1 widens the sweep) -------------------------------------------------------------
    for _ in range(int(24 * max(scale, 0))):
        nx, ny = int(rng.integers(3, 200)), int(rng.integers(3, 400))
        dtc, dt, comp = pick(INTERP_OK)
        kk = int(rng.integers(0, 10000))
        c = leg_common(kk, nx, ny, dt)
        if rng.integers(0, 2):
            add("up_leg", dtc=dtc, comp=comp, nsweep=int(rng.integers(0, 3)), sides=int(rng.integers(0, 16)),
                window=leg_windows(nx, ny)[pick(["full", "sub", "ring", "empty"])], tag="fuzz", **c)
        else:
            add("down_leg", dtc=pick(DT), nsweep=int(rng.integers(0, 3)), zero_init=int(rng.integers(0, 2)), rect=None, tag="fuzz", **c)

    # ---- refusals ----------------------------------------------------------------------------------------------------
    for r in REFUSALS:
        r = dict(r)
        nx, ny = r.pop("nx", 41), r.pop("ny", 66)
        entry = r.pop("entry")
        c = dict(nx=nx, ny=ny, nxc=(nx + 1) // 2, nyc=(ny + 1) // 2, pf="lib", pc="lib", sides=15, ci=0, cj=0, sm=0, omega=0.8, poff=0, coeff=-1.0,
                 nsweep=2, nsweep_pre=2, window=(1, nx - 1, 1, ny - 1), tag="refuse")
        c.update(r)
        add(entry, **c)["disp"] = "refuse"
    return out


# ---- finite extremes (tests/special_values.py, tests/test_gpu_range_edges.py): a list of its own -- the ids and seeds of
# _cases are derived from list position and must not move
SPECIAL_OP_SHAPES = {"f64": (35, 66), "f32": (34, 129)}      # one past the fp64 tile column (64) / at the fp32 one (128)
SPECIAL_LEG_SHAPES = [(33, 130), (530, 513), (1102, 1122)]   # 8-row tiles, 16-row tiles, register-blocked
SPECIAL_KINDS = ("tiny", "huge", "patches")


def _special_case(out, entry, var, dt, dtc, comp, field, k):
    """one case of `entry` with the dtypes given on the field kind `field`; k picks the leg family and the small choices"""
    legs = ("down_leg", "up_leg", "span_leg")
    if entry == "span_leg":
        nx, ny = SPECIAL_LEG_SHAPES[2]
    elif entry in legs:
        nx, ny = SPECIAL_LEG_SHAPES[k % 3]
    else:
        nx, ny = SPECIAL_OP_SHAPES[dt or "f64"]
    c = dict(entry=entry, disp="compare", nx=nx, ny=ny, pf=PITCHES[k % 3], field=field)
    for key, val in (("dt", dt), ("dtc", dtc), ("comp", comp)):
        if val is not None:
            c[key] = val
    if var:
        c["var"] = True
    sp = ("eq", "neq")[len(out) % 2]                      # dyadic spacings only
    c["sp"] = sp
    c["hx"], c["hy"], c["dyadic"] = SPACINGS[sp]
    if entry == "jacobi":
        c.update(omega=OMEGAS[k % 4])
    elif entry == "rbgs_colour":
        c.update(omega=OMEGAS[(k + 1) % 4], colour=k % 2, poff=(k // 2) % 2)
    elif entry == "residual":
        c.update(coeff=(-1.0, 0.37)[k % 2])
    elif entry == "residual_mixed":
        c.update(pc=PITCHES[(k + 1) % 3], coeff=(-1.0, 1.5)[k % 2])
    elif entry == "sumsq":
        c.update(window=((1, nx - 1, 3, ny - 2), (0, nx, 0, ny))[k % 2])
    elif entry == "convert":
        c.update(pc=PITCHES[(k + 1) % 3])
    elif entry == "var_rdiag":
        c.update(sigma=(0.0, 2.5)[k % 2])
    elif entry in ("restrict", "prolong_add", "inject_ring"):
        c.update(nxc=(nx + 1) // 2, nyc=(ny + 1) // 2, pc=PITCHES[(k + 1) % 3], sides=15, ci=0, cj=0)
    elif entry in legs:
        # the norm window of `patches` ends ahead of the large rectangle (rows from 0.62 nx), whose squares may be beyond fp64
        win = (1, int(0.55 * nx), 1, ny - 1) if field == "patches" else (1, nx - 1, 1, ny - 1)
        c.update(nxc=(nx + 1) // 2, nyc=(ny + 1) // 2, ci=0, cj=0, pc=PITCHES[(k + 1) % 3], sm=0 if entry == "span_leg" else k % 2,
                 omega=OMEGAS[k % 4], poff=k % 2, coeff=-1.0, nsweep=2 - (k // 2) % 2, sides=15)
        if entry == "down_leg":
            c.update(zero_init=0, rect=None)
        else:
            c.update(window=win)
        if entry == "span_leg":
            c.update(nsweep_pre=1 + k % 2)
    else:
        raise KeyError(entry)
    c["seed"] = 104729 * len(out) + 31
    c["id"] = "%s%s-%s-%s-%dx%d-%s" % (entry, "_var" if var else "", field, "-".join(x for x in (dt, dtc, comp) if x), nx, ny, sp)
    out.append(c)
    return c


def special_cases():
    """one case per entry of ENTRIES, per dtype combination the default list has for that entry, per kind of finite extreme
    field; then the convert, restrict and residual_mixed cases whose fp64 values straddle what fp32 holds ("straddle")"""
    if "special" in _CACHE:
        return _CACHE["special"]
    combos = {}
    for c in default_cases():
        if c["disp"] == "compare" and c.get("tag") != "fuzz":
            key = (c.get("dt"), c.get("dtc"), c.get("comp"))
            lst = combos.setdefault(entry_name(c), [])
            if key not in lst:
                lst.append(key)
    out = []
    for name in ENTRIES:
        var = name.endswith("_var")
        entry = name[:-4] if var else name
        for m, (dt, dtc, comp) in enumerate(combos[name]):
            for n, field in enumerate(SPECIAL_KINDS):
                _special_case(out, entry, var, dt, dtc, comp, field, m + n)
    _special_case(out, "convert", False, "f64", "f32", None, "straddle", 0)
    _special_case(out, "convert", False, "f32", "f64", None, "straddle", 1)
    _special_case(out, "restrict", False, "f64", "f32", None, "straddle", 2)
    _special_case(out, "restrict", False, "f64", "f64", None, "straddle", 3)
    _special_case(out, "residual_mixed", False, "f32", "f64", None, "straddle", 4)
    _CACHE["special"] = out
    return out


_CACHE = {}


def default_cases():
    key = (int(os.environ.get("MG_FUZZ_SEED", 2024)), float(os.environ.get("MG_FUZZ_DEV", 1)))
    if key not in _CACHE:
        _CACHE[key] = _cases(*key)
    return _CACHE[key]


def cases_of(entry, disp=None):
    return [c for c in default_cases() if c["entry"] == entry and (disp is None or c["disp"] == disp)]


def cells(case):
    return case["nx"] * case["ny"]


def sub_domain(case):
    """a case with sub-domain arguments: ghost edges, coarse offsets or a coarse array that does not fit"""
    return (case.get("sides", 15) != 15 or case.get("ci", 0) or case.get("cj", 0) or case["nxc"] != (case["nx"] + 1) // 2 or
            case["nyc"] != (case["ny"] + 1) // 2)


# ======================================================================================================================
# arrays: every array of a call lives inside a larger allocation with GUARD rows before and after it, filled with a NaN of
# recognisable payload -- a sentinel read as data poisons the result, a sentinel overwritten is a stray store
# ======================================================================================================================
SENT_BITS = {4: 0x7FC0BEEF, 8: 0x7FF80000DEADBEEF}


def sentinel(dtype, shape):
    dtype = np.dtype(dtype)
    u = np.full(shape, SENT_BITS[dtype.itemsize], dtype=np.uint32 if dtype.itemsize == 4 else np.uint64)
    return u.view(dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


class Arr:
    """one array of a call: `full` (GUARD + nx + GUARD, ld) tensor, `view` = its rows GUARD .. GUARD + nx (what the call gets)"""

    def __init__(self, torch, device, host_full, nx, ny, ld):
        self.nx, self.ny, self.ld = nx, ny, ld
        self.full = torch.from_numpy(host_full).to(device)
        self.view = self.full[GUARD:GUARD + nx]

    def host(self):
        return self.full.cpu().numpy().copy()


def array_specs(case):
    """name -> (dtype key, nx, ny, pitch kind, role); role: "in" random data, "coef" rough positive field, "inout" random data the
    call updates, "out" sentinel-filled"""
    e, c = case["entry"], case
    f = (c.get("dt"), c["nx"], c["ny"], c.get("pf", "lib"))
    co = (c.get("dtc"), c.get("nxc"), c.get("nyc"), c.get("pc", "lib"))
    if e == "jacobi":
        s = {"u": f + ("in",), "rhs": f + ("in",), "out": f + ("out",)}
    elif e == "rbgs_colour":
        s = {"u": f + ("inout",), "rhs": f + ("in",)}
    elif e == "residual":
        s = {"u": f + ("in",), "rhs": f + ("in",), "r": f + ("out",)}
    elif e == "residual_mixed":
        s = {"u": f + ("in",), "rhs": f + ("in",), "r": ("f64", c["nx"], c["ny"], c["pc"], "out")}
    elif e == "sumsq":
        s = {"u": f + ("in",)}
    elif e == "convert":
        s = {"u": f + ("in",), "out": (c["dtc"], c["nx"], c["ny"], c["pc"], "out")}
    elif e == "var_rdiag":
        s = {"a": f + ("coef",), "rd": f + ("out",)}
    elif e in ("restrict", "inject_ring"):
        s = {"fine": f + ("in",), "coarse": co + ("out",)}
    elif e == "prolong_add":
        s = {"coarse": co + ("in",), "fine": f + ("inout",)}
    elif e == "down_leg":
        s = {"u": f + ("in",), "rhs": f + ("in",), "out": f + ("out",), "rhs_c": co + ("out",)}
    elif e == "up_leg":
        s = {"u": f + ("in",), "rhs": f + ("in",), "out": f + ("out",), "e_c": co + ("in",)}
    elif e == "span_leg":
        s = {"u": f + ("in",), "rhs": f + ("in",), "out_mid": f + ("out",), "out_next": f + ("out",), "e_c": co + ("in",), "rhs_c": co + ("out",)}
    else:
        raise KeyError(e)
    if c.get("var"):
        s["a"] = f + ("coef",)
        s["rd"] = f + ("out",)
    return s


OUTPUTS = {"jacobi": ["out"], "rbgs_colour": ["u"], "residual": ["r"], "residual_mixed": ["r"], "sumsq": [], "convert": ["out"], "var_rdiag": ["rd"],
           "restrict": ["coarse"], "inject_ring": ["coarse"], "prolong_add": ["fine"], "down_leg": ["out", "rhs_c"], "up_leg": ["out"],
           "span_leg": ["out_mid", "out_next", "rhs_c"]}
# entries whose `out` arrays a sweep kernel stores tile by tile: rows 1 .., and the far edge (row nx - 1, column ny - 1) only where
# the last tile reaches it: include/mghip.h leaves those cells open (the fixed edge value, or what the caller left there)
SWEEP_OUTPUTS = {"jacobi": ["out"], "down_leg": ["out"], "up_leg": ["out"], "span_leg": ["out_mid", "out_next"]}


def build_arrays(case, device="cpu"):
    """the arrays of a call.  case["field"] (optional; tests/special_values.py): a kind of FIELD_KINDS scales the seeded data of
    every `in` / `inout` array by the scale of the narrowest dtype among the call's arrays, "straddle" writes fp64 values
    around the ends of the fp32 range over part of it; coefficient fields stay as they are"""
    import torch
    rng = np.random.default_rng(case["seed"])
    field = case.get("field")
    if field:
        import special_values as SV
        narrow = SV.narrowest(case)
    A = {}
    for name, (dt, nx, ny, pk, role) in array_specs(case).items():
        ld = pitch(pk, dt, ny)
        host = sentinel(NPDT[dt], (nx + 2 * GUARD, ld))
        if role != "out":
            data = rng.standard_normal((nx, ny))
            if field and role != "coef":
                data = SV.straddle_fill(data) if field == "straddle" else SV.apply_field(field, data, narrow)
                with np.errstate(over="ignore", under="ignore"):
                    host[GUARD:GUARD + nx, :ny] = data.astype(NPDT[dt])
            else:
                host[GUARD:GUARD + nx, :ny] = (np.exp(0.5 * data) if role == "coef" else data).astype(NPDT[dt])
        A[name] = Arr(torch, device, host, nx, ny, ld)
    return A


def invoke(case, ops, A, select=0, out_mid=True, rdiag_ready=False):
    """run the case's call through `ops`; returns the sum of squares (float) where the call has one"""
    c, e = case, case["entry"]
    v = {k: a.view for k, a in A.items()}
    nx, ny, hx, hy = c["nx"], c["ny"], c["hx"], c["hy"]
    kw = {}
    if c.get("var"):
        if not rdiag_ready:
            ops.var_rdiag(v["a"], v["rd"], nx, ny, hx, hy, 0.0)
        kw = dict(acoef=v["a"], rdiag=v["rd"])
    res = None
    if e == "jacobi":
        ops.jacobi(v["u"], v["rhs"], v["out"], nx, ny, hx, hy, c["omega"])
    elif e == "rbgs_colour":
        ops.rbgs_colour(v["u"], v["rhs"], nx, ny, hx, hy, c["omega"], c["colour"], c["poff"])
    elif e == "residual":
        ops.residual(v["u"], v["rhs"], v["r"], nx, ny, hx, hy, c["coeff"])
    elif e == "residual_mixed":
        ops.residual_mixed(v["u"], v["rhs"], v["r"], nx, ny, hx, hy, c["coeff"])
    elif e == "sumsq":
        res = ops.sumsq(v["u"], *c["window"])
    elif e == "convert":
        ops.convert(v["u"], v["out"], nx, ny)
    elif e == "var_rdiag":
        ops.var_rdiag(v["a"], v["rd"], nx, ny, hx, hy, c["sigma"])
    elif e == "restrict":
        ops.restrict(v["fine"], v["coarse"], nx, ny, c["nxc"], c["nyc"], c["sides"])
    elif e == "inject_ring":
        ops.inject_ring(v["fine"], v["coarse"], nx, ny, c["nxc"], c["nyc"], c["sides"], c["ci"], c["cj"])
    elif e == "prolong_add":
        ops.prolong_add(v["coarse"], v["fine"], nx, ny, c["nxc"], c["nyc"], c["sides"])
    elif e == "down_leg":
        ops.down_leg(c["sm"], v["u"], v["rhs"], v["out"], v["rhs_c"], nx, ny, c["nxc"], c["nyc"], c["ci"], c["cj"], hx, hy, c["omega"], c["coeff"],
                     c["nsweep"], bool(c["zero_init"]), c["poff"], select, c["rect"] if select else None, **kw)
    elif e == "up_leg":
        res = ops.up_leg(c["sm"], v["u"], v["rhs"], v["out"], v["e_c"], nx, ny, c["nxc"], c["nyc"], c["ci"], c["cj"], c["sides"], hx, hy, c["omega"],
                         c["coeff"], c["nsweep"], c["poff"], c["window"], **kw)
    elif e == "span_leg":
        res = ops.span_leg(c["sm"], v["u"], v["rhs"], v["out_mid"] if out_mid else None, v["out_next"], v["e_c"], v["rhs_c"], nx, ny, c["nxc"], c["nyc"],
                           c["ci"], c["cj"], c["sides"], hx, hy, c["omega"], c["coeff"], c["nsweep"], c["nsweep_pre"], c["poff"], c["window"])
    else:
        raise KeyError(e)
    return None if res is None else float(res.cpu().numpy()[0])


def snapshot(A):
    return {k: a.host() for k, a in A.items()}


def make_ref_ops(base):
    """the reference form of a NumpyOps class: exactly rounded sums (math.fsum of the squared fp64-cast cells), the window's
    cell count and largest value remembered for the sum's bound, and a spanning leg that serves out_mid = NULL"""
    import torch

    class RefOps(base):
        whole = False
        last_window = (0, 0.0)

        def _sum_of_squares(self, w):
            self.last_window = (int(w.size), float(np.max(np.abs(w))) if w.size else 0.0)
            return math.fsum((w * w).ravel().tolist())

        def _store_out(self, o, v):
            if self.whole:
                o[...] = v
                return
            super()._store_out(o, v)

        def span_leg(self, sm, u, rhs, out_mid, out_next, e_c, rhs_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, sides, hx, hy, omega, coeff,
                     nsweep_post, nsweep_pre, poff, window):
            # the iterate between the two halves never leaves the kernel: every edge of it is the fixed value u + P e
            mid = torch.zeros((lnx, lny), dtype=u.dtype)
            self.whole = True
            try:
                res = self.up_leg(sm, u, rhs, mid, e_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, sides, hx, hy, omega, coeff, nsweep_post, poff, window)
            finally:
                self.whole = False
            self.last_mid = mid.numpy().copy()
            self.down_leg(sm, mid, rhs, out_next, rhs_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, hx, hy, omega, coeff, nsweep_pre, False, poff)
            if out_mid is not None:
                self._store_out(self._v(out_mid, lnx, lny), self.last_mid)
            return res
    return RefOps


def run_reference(case, ops_cls):
    """the case through a NumpyOps class on CPU tensors: (arrays after the call, sum or None, ops)"""
    ops = ops_cls(NPDT[case.get("comp") or case.get("dt") or "f64"])
    A = build_arrays(case, "cpu")
    with np.errstate(all="ignore"):
        s = invoke(case, ops, A)
    return snapshot(A), s, ops


def tau_of(case, dtype, ref_max):
    """the project's bound for non-dyadic spacings (tests/test_gpu_fuzz.py): 5e-14 (fp64) / 2e-5 (fp32) times max(1, max|ref|)"""
    return (5e-14 if np.dtype(dtype) == np.float64 else 2e-5) * max(1.0, ref_max)


def _fail(case, name, bad, got, ref, what):
    idx = np.argwhere(bad)
    i, j = (int(x) for x in idx[0])
    raise AssertionError("mg_dev_%s case %s: output %s %s in %d cells; first (%d, %d): got %r (bits %#x), expected %r (bits %#x); %s" % (
        entry_name(case), case["id"], name, what, len(idx), i, j, got[i, j], int(bits(got)[i, j]), ref[i, j], int(bits(ref)[i, j]), tile_of(case, i, j)))


def compare_array(case, name, got_full, ref_full, nx, ny, exact=None, tol_dtype=None, far_edge_open=False, special=False):
    """one output, guards included.  Bit for bit on dyadic spacings (sentinels included: a cell the reference leaves untouched
    must still hold the sentinel), within tau otherwise; pad columns are exempt; guard rows must be untouched.
    tol_dtype: the dtype whose bound applies where it is not the array's own (the down leg's coarse rhs is rounded in the fine
    level's dtype and in its own: an fp64 array of fp32-rounded values, or an fp32 rounding of fp64 values that a last-bit
    difference can flip).
    special (exact comparisons only): the data may hold non-finite values -- special_values.same_special: the cells that hold
    the sentinel are the same, the NaN masks are identical and every other cell, infinities included, has equal bits."""
    sent = SENT_BITS[got_full.dtype.itemsize]
    gb = bits(got_full)
    guards = np.ones(gb.shape[0], dtype=bool)
    guards[GUARD:GUARD + nx] = False
    bad = gb[guards] != sent
    if bad.any():
        r, j = (int(x) for x in np.argwhere(bad)[0])
        rows = np.flatnonzero(guards)
        raise AssertionError("mg_dev_%s case %s: output %s: %d guard cells overwritten; first at row %d (array rows 0..%d), column %d" % (
            entry_name(case), case["id"], name, int(bad.sum()), int(rows[r]) - GUARD, nx - 1, j))
    got, ref = got_full[GUARD:GUARD + nx, :ny], ref_full[GUARD:GUARD + nx, :ny]
    g, r = bits(got), bits(ref)
    free = np.zeros(got.shape, dtype=bool)
    if far_edge_open:               # unstored far-edge cells still hold the sentinel; stored ones must hold the reference's bits
        free[-1, :] = True
        free[:, -1] = True
        free &= (g == sent)
    exact = case["dyadic"] if exact is None else exact
    if exact:
        if special:
            import special_values as SV
            bad = (((g == sent) != (r == sent)) | SV.special_mismatch(got, ref)) & ~free
        else:
            bad = (g != r) & ~free
        if bad.any():
            _fail(case, name, bad, got, ref, "differs")
        return
    rs, gs = (r == sent), (g == sent)
    bad = (rs != gs) & ~free
    if bad.any():
        _fail(case, name, bad, got, ref, "written / unwritten cells differ")
    val = ~rs & ~gs
    tau = tau_of(case, tol_dtype or got.dtype, float(np.max(np.abs(ref[val].astype(np.float64)))) if val.any() else 0.0)
    with np.errstate(invalid="ignore"):
        bad = val & ~(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= tau)
    if bad.any():
        _fail(case, name, bad, got, ref, "differs by more than %.3g" % tau)


def compare_sum(case, got, ref, n_w, w_max, field_dtype, exact=None, special=False):
    """sums: relative 1e-12 on dyadic spacings (partial sums run over other tiles); otherwise the per-cell bound tau carried
    through the sum by Cauchy-Schwarz, |S - S_ref| <= 2 sqrt(S_ref n_w) tau + n_w tau^2, plus the same 1e-12 S_ref.  An empty
    window gives exactly 0.0."""
    exact = case["dyadic"] if exact is None else exact
    if special and not (math.isfinite(got) and math.isfinite(ref)):      # NaN where the reference's is, the same infinity
        import special_values as SV
        assert SV.same_special(got, ref), "mg_dev_%s case %s: sum of squares %r, reference %r" % (entry_name(case), case["id"], got, ref)
        return
    if n_w == 0:
        assert got == 0.0 and ref == 0.0, "mg_dev_%s case %s: sum over an empty window is %r (reference %r)" % (entry_name(case), case["id"], got, ref)
        return
    bound = 1e-12 * ref
    if not exact:
        tau = tau_of(case, field_dtype, w_max)
        bound += 2.0 * math.sqrt(ref * n_w) * tau + n_w * tau * tau
    assert abs(got - ref) <= bound, "mg_dev_%s case %s: sum of squares %r, reference %r: differs by %.3g > %.3g (window of %d cells)" % (
        entry_name(case), case["id"], got, ref, abs(got - ref), bound, n_w)


def compare_call(case, got, got_sum, ref, ref_sum, ref_ops, before=None, special=False):
    """every output of one call against the reference; `before`: snapshot taken before the call (inputs must be unchanged);
    special: by special_values.same_special (data that may hold non-finite values; dyadic spacings)"""
    e = case["entry"]
    specs = array_specs(case)
    exact = True if e in ("restrict", "inject_ring", "prolong_add", "convert", "sumsq") else None
    for name in OUTPUTS[e]:
        dt, nx, ny, pk, role = specs[name]
        # the coarse rhs is rounded in the fine level's dtype and again in its own: the looser of the two bounds
        loose = np.dtype(np.float32) if name == "rhs_c" and "f32" in (case["dt"], case["dtc"]) else None
        compare_array(case, name, got[name], ref[name], nx, ny, exact, loose, name in SWEEP_OUTPUTS.get(e, ()), special)
    if before is not None:
        for name, (dt, nx, ny, pk, role) in specs.items():
            if name not in OUTPUTS[e] and not (case.get("var") and name == "rd"):
                assert np.array_equal(bits(got[name]), bits(before[name])), "mg_dev_%s case %s: input %s was modified" % (entry_name(case), case["id"], name)
    if ref_sum is not None or got_sum is not None:
        n_w, w_max = ref_ops.last_window
        compare_sum(case, got_sum, ref_sum, n_w, w_max, NPDT[case["dt"]], exact, special)
