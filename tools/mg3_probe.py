#!/usr/bin/env python3
"""Kernel and cycle times of the 3-D multigrid family (needs a GPU).

At 257^3 and 513^3 (or the sizes given on the command line), in fp64 and fp32: device-event times of each mg3_dev_* kernel and
of one whole V(2,2) weighted-Jacobi cycle of the engine, after a warm-up, as the median over `--reps` windows of `--launches`
launches each.  Each kernel time is printed with the words per cell the kernel must move (the least traffic of the algorithm,
computed from the shape: the table below), the bandwidth that gives, and its fraction of the 8 TB/s HBM peak -- the bound of all
of these kernels is bytes, not operations.  The yardstick in the tree is the 2-D Jacobi sweep from HBM, 0.61-0.67 of peak
(README).  A 257^3 fp32 field (68 MB) fits the 256 MB last-level cache, so its figures are not HBM figures; 513^3 fields do not
fit.  Writes what it prints to --out (default profiles/mg3_times.txt).

    kernel                     words per cell it must move
    Jacobi sweep               3        (u, f in; out)
    colour pass                2.5      (u in; half of f in; half of u out)
    residual                   3        (u, f in; r out)
    residual, sum only         2        (u, f in)
    restriction                1 + 1/8  (r in; coarse f out)
    prolong-add                2 + 1/8  (u in and out; coarse e in)
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mixed_precision_multigrid_solvers_for_pdes_amd as mg          # noqa: E402
from mixed_precision_multigrid_solvers_for_pdes_amd import _build, _lib      # noqa: E402
from mixed_precision_multigrid_solvers_for_pdes_amd.engine3d import check3   # noqa: E402

import torch                                                         # noqa: E402

PEAK = 8.0e12
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def timed(fn, launches, reps, warm=3):
    """median, min, max seconds per launch over `reps` windows of `launches` launches on torch's current stream"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / launches)
    return statistics.median(out), min(out), max(out)


def kernels(n, dtype, launches, reps):
    lib = _lib.load()
    code = _lib.dtype_code("float64" if dtype == torch.float64 else "float32")
    es = 8 if dtype == torch.float64 else 4
    ld = C.c_int(0)
    _lib.check(lib.mg_pitch_elems(code, n, C.byref(ld)))
    ld = ld.value
    nc = (n + 1) // 2
    ldc = C.c_int(0)
    _lib.check(lib.mg_pitch_elems(code, nc, C.byref(ldc)))
    ldc = ldc.value
    gen = torch.Generator(device="cuda").manual_seed(1)
    u, f, out = (torch.randn((n, n, ld), dtype=dtype, device="cuda", generator=gen) for _ in range(3))
    e, fc = (torch.randn((nc, nc, ldc), dtype=dtype, device="cuda", generator=gen) * 1e-3 for _ in range(2))
    nbytes = C.c_int64(0)
    check3(lib.mg3_dev_scratch_bytes(n, n, n, C.byref(nbytes)))
    scratch = torch.zeros(nbytes.value // 8 + 2, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    h = 1.0 / (n - 1)
    cells = float(n) ** 3
    runs = [
        ("jacobi", 3.0, lambda: check3(lib.mg3_dev_jacobi(code, n, n, n, ld, h, h, h, 0.0, 0.8, p(u), p(f), p(out), st))),
        ("colour pass", 2.5, lambda: check3(lib.mg3_dev_rbgs_colour(code, n, n, n, ld, h, h, h, 0.0, 1.0, 0, 0, p(out), p(f), st))),
        ("residual", 3.0, lambda: check3(lib.mg3_dev_residual(code, code, n, n, n, ld, ld, h, h, h, 0.0, p(u), p(f), p(out), None, None, st))),
        ("residual, sum only", 2.0, lambda: check3(lib.mg3_dev_residual(code, code, n, n, n, ld, ld, h, h, h, 0.0, p(u), p(f), None, p(scratch),
                                                                        p(scratch[-1:]), st))),
        ("restriction", 1.125, lambda: check3(lib.mg3_dev_restrict(code, n, n, n, ld, ldc, p(u), p(fc), st))),
        ("prolong-add", 2.125, lambda: check3(lib.mg3_dev_prolong_add(code, n, n, n, ld, ldc, p(e), p(out), st))),
    ]
    for name, words, fn in runs:
        med, lo, hi = timed(fn, launches, reps)
        bw = words * cells * es / med
        say(f"{n}^3 {'fp64' if es == 8 else 'fp32'} {name:20s} {med * 1e6:10.1f} us  (min {lo * 1e6:.1f}, max {hi * 1e6:.1f})  "
            f"{words:5.3f} words/cell  {bw / 1e12:6.3f} TB/s  {bw / PEAK:5.3f} of peak")


def cycle(n, precision, launches, reps):
    with mg.Multigrid3DEngine(n, n, n, max_levels=10, cycle="V", pre=2, post=2, smoother="jacobi", omega=0.8, precision=precision) as eng:
        gen = torch.Generator(device="cuda").manual_seed(2)
        f = torch.randn((n, n, n + 1), dtype=torch.float32, device="cuda", generator=gen)
        eng.set_rhs(f)
        eng.set_solution(None)
        stream = C.c_void_p(None)
        check3(_lib.load().mg3_stream(eng._h, C.byref(stream)))
        ext = torch.cuda.ExternalStream(stream.value)
        with torch.cuda.stream(ext):
            med, lo, hi = timed(lambda: eng.cycle(1), launches, reps)
        norm = eng.residual_norm()
        # per cycle on the fine level: 4 Jacobi sweeps (3 words), the residual (3), the restriction's read (1), the prolong-add (2);
        # the coarser levels add 1/7 of that
        words = (4 * 3 + 3 + 1 + 2) * 8.0 / 7.0
        es = 8 if precision == "double" else 4
        bw = words * float(n) ** 3 * es / med
        say(f"{n}^3 {precision:6s} V(2,2) Jacobi cycle, {eng.num_levels} levels {med * 1e3:9.3f} ms  (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})  "
            f"{words:5.2f} words/cell  {bw / 1e12:6.3f} TB/s  {bw / PEAK:5.3f} of peak   residual norm after {norm:.3e}  "
            f"device bytes {eng.device_bytes / 2**30:.2f} GiB")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sizes", nargs="*", type=int, default=[257, 513])
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mg3_times.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mg3_probe needs a GPU: nothing here is measured without one")
    say(f"mg3_probe: libmghip {_build.source_hash()}, {torch.cuda.get_device_name(0)}; median of {args.reps} windows of {args.launches} "
        f"launches, device events; peak = 8 TB/s; words = the least the kernel must move")
    for n in args.sizes:
        for dtype in (torch.float64, torch.float32):
            kernels(n, dtype, args.launches, args.reps)
        for precision in ("double", "single"):
            cycle(n, precision, max(2, args.launches // 2), args.reps)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
