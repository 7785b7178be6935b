"""Special values for the kernel and driver tests -- not a test.

Where a NaN or an Inf is planted (plant_positions, VALUES), how two results that may hold non-finite values are compared
(same_special: identical NaN masks, equal bits everywhere else, infinities included), and the three kinds of finite
extreme field the call-level cases of tests/dev_call_cases.py run on (FIELD_KINDS: `tiny`, `huge`, `patches`).
tests/test_special_values_cpu.py checks the helpers and that the kinds do what they are chosen for on the restatement:
subnormal outputs under `tiny`, (almost) no overflow under `huge`.  Plain NumPy."""
import math

import numpy as np

import dev_call_cases as G

NAN = float(np.uint64(0x7FF8000000000000).view(np.float64))      # the canonical quiet NaN, never the sentinel's payload
VALUES = (NAN, float("inf"), float("-inf"))
VALUE_IDS = ("nan", "+inf", "-inf")

# tile extents of the single operators and of the flow kernels (TileShape: kTI rows, 512 bytes of columns)
TILE_I = G.K_TI
TILE_J = {"f64": G.TILE_ROW_BYTES // G.ESIZE["f64"], "f32": G.TILE_ROW_BYTES // G.ESIZE["f32"]}


def plant_positions(nx, ny, tile_i=TILE_I, tile_j=TILE_J["f64"]):
    """[(name, (i, j))]: where a kernel that tiles an (nx, ny) array in tile_i x tile_j tiles can lose a planted value.
    Interior: first, last, centre, the last interior cell of the first tile, the first interior cell of the last tile in
    each direction (where there is more than one tile).  Not interior: a non-corner ring cell on each side, two opposite
    corners and, where ny is odd, the pad column ny of a middle row (outside the array: only a device buffer has it).
    Cells that coincide on a small array are listed once, under their first name."""
    out = [("first", (1, 1)), ("last", (nx - 2, ny - 2)), ("centre", (nx // 2, ny // 2)),
           ("tile0_last", (min(tile_i - 1, nx - 2), min(tile_j - 1, ny - 2)))]
    ti0, tj0 = (nx - 1) // tile_i * tile_i, (ny - 1) // tile_j * tile_j
    if 0 < ti0 <= nx - 2:                       # a last tile that holds the far ring alone has no interior cell
        out.append(("last_tile_row", (ti0, max(1, ny // 3))))
    if 0 < tj0 <= ny - 2:
        out.append(("last_tile_col", (max(1, nx // 3), tj0)))
    out += [("ring_ilo", (0, ny // 2)), ("ring_ihi", (nx - 1, ny // 2)), ("ring_jlo", (nx // 2, 0)), ("ring_jhi", (nx // 2, ny - 1)),
            ("corner_lo", (0, 0)), ("corner_hi", (nx - 1, ny - 1))]
    if ny % 2:
        out.append(("pad", (nx // 2, ny)))
    seen, uniq = set(), []
    for name, ij in out:
        if ij not in seen:
            seen.add(ij)
            uniq.append((name, ij))
    return uniq


def is_interior(ij, nx, ny):
    return 1 <= ij[0] <= nx - 2 and 1 <= ij[1] <= ny - 2


def is_corner(ij, nx, ny):
    return ij[0] in (0, nx - 1) and ij[1] in (0, ny - 1)


def in_array(ij, nx, ny):
    return 0 <= ij[0] < nx and 0 <= ij[1] < ny


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def special_mismatch(got, ref):
    """boolean array: True where got and ref differ -- one is a NaN and the other is not, or neither is and the bits differ
    (so +Inf / -Inf, +0 / -0 and every finite value, subnormal ones included, must agree bit for bit)"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype != ref.dtype or got.shape != ref.shape:
        raise ValueError("same_special compares arrays of one dtype and shape: %s %s, %s %s" % (got.dtype, got.shape, ref.dtype, ref.shape))
    gn, rn = np.isnan(got), np.isnan(ref)
    return (gn != rn) | (~gn & ~rn & (_bits(got) != _bits(ref)))


def same_special(got, ref):
    """True only if the NaN masks are identical and all remaining cells, infinities included, have equal bits.  Python
    floats and NumPy scalars are taken as fp64."""
    if np.ndim(got) == 0 and np.ndim(ref) == 0 and not isinstance(got, np.generic):
        got, ref = np.float64(got), np.float64(ref)
    return not bool(np.any(special_mismatch(got, ref)))


def same_sum(got, ref, rel=1e-12):
    """a sum against the restatement's: same_special where either is non-finite; for finite sums the rule of
    dev_call_cases.compare_sum on dyadic spacings (relative 1e-12: partial sums run over other tiles)"""
    got, ref = float(got), float(ref)
    if not (math.isfinite(got) and math.isfinite(ref)):
        return same_special(got, ref)
    return abs(got - ref) <= rel * abs(ref)


# ---- finite extremes -------------------------------------------------------------------------------------------------
# kind -> {narrowest dtype among the call's arrays: scale(s)}.  Powers of two (exact in both formats) except the fp64
# patches, which follow tests/test_gpu_pow2_legs.py.  With an fp64 scale on a call that has an fp32 array everything would
# round to 0 or Inf and the case would prove nothing, hence the narrowest dtype decides.
FIELD_KINDS = {
    "tiny": {"f32": 2.0 ** -135, "f64": 2.0 ** -1040},
    "huge": {"f32": 2.0 ** 90, "f64": 2.0 ** 400},
    # (subnormal, small, large) factors of three rectangles of an otherwise normal field
    "patches": {"f32": (2.0 ** -140, 2.0 ** -20, 2.0 ** 80), "f64": (1e-310, 1e-200, 1e200)},
}
KINDS = tuple(FIELD_KINDS)


def narrowest(case):
    """"f32" if any array of the call is fp32, else "f64" """
    return "f32" if any(spec[0] == "f32" for spec in G.array_specs(case).values()) else "f64"


def _frac(n, lo, hi):
    return slice(int(lo * n), int(hi * n))


def patch_slices(nx, ny):
    """the rectangles of `patches`, as fractions of the array (tests/test_gpu_pow2_legs.py::_host_arrays): subnormal, small, large"""
    return ((_frac(nx, 0.80, 0.90), _frac(ny, 0.10, 0.40)), (_frac(nx, 0.10, 0.20), _frac(ny, 0.10, 0.30)),
            (_frac(nx, 0.62, 0.75), _frac(ny, 0.55, 0.80)))


def apply_field(kind, data, narrow):
    """the fp64 standard-normal `data` of one `in` / `inout` array, scaled for `kind` (still fp64: the caller rounds it)"""
    s = FIELD_KINDS[kind][narrow]
    if kind != "patches":
        return data * s
    out = data.copy()
    for (si, sj), f in zip(patch_slices(*data.shape), s):
        out[si, sj] *= f
    return out


def is_subnormal(a):
    a = np.asarray(a)
    tiny = np.finfo(a.dtype).tiny
    return (a != 0) & (np.abs(a) < tiny)


# ---- fp64 values that straddle what fp32 holds -----------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
# the largest double that still rounds to FLT_MAX: one ulp(double) below the midpoint FLT_MAX + 2^103 (the tie rounds to even,
# which is 2^128 = Inf)
ROUNDS_TO_FLT_MAX = float(np.nextafter(np.float64(FLT_MAX) + 2.0 ** 103, 0.0))
ROUNDS_TO_INF = float(np.float64(FLT_MAX) + 2.0 ** 103)
F32_EDGE_VALUES = (FLT_MAX, -FLT_MAX, ROUNDS_TO_FLT_MAX, ROUNDS_TO_INF, -ROUNDS_TO_INF, 2.0 ** -149, -2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -149,
                   -0.0, 0.0)


def straddle_fill(data):
    """`data` (fp64, 2-D) with F32_EDGE_VALUES written over every 7th cell of the flattened array, in turn: next to random fill"""
    out = data.copy()
    flat = out.reshape(-1)
    idx = np.arange(3, flat.size, 7)
    flat[idx] = np.resize(np.array(F32_EDGE_VALUES), idx.size)
    return out
