#!/usr/bin/env python3
"""Time to solution of the device-resident conjugate-gradient loop against the plain multigrid iteration (needs a GPU).

At 1025^2 and 4097^2 (or the sizes given on the command line), for -Laplacian with the sine right-hand side and for
-div(a grad .) with the 8 x 8 checkerboard coefficient (contrast 1e4), V(2,2) weighted Jacobi 0.8:
  * PCGEngine.solve_device to tol = 1e-8 ||r_0|| with a double and a single_managed preconditioner: iterations, seconds;
  * MultigridEngine.iterate (mg_iterate) to the same tolerance, at most 100 cycles, non-convergence reported;
alternating the two in one process after a warm-up, the median of `--reps` solves each.  Then hipEvent times of the three
field kernels of the loop with the bytes they move.  Writes what it prints to --out (default profiles/pcg_times.txt)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mixed_precision_multigrid_solvers_for_pdes_amd as mg          # noqa: E402
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib      # noqa: E402

import torch                                                         # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def checkerboard(n, blocks=8, contrast=1e4):
    x = np.linspace(0, 1, n)
    X, Y = np.meshgrid(x, x, indexing="ij")
    a = np.ones((n, n))
    a[(np.floor(X * blocks) + np.floor(Y * blocks)) % 2 == 0] = contrast
    return a


def sine_rhs(n):
    x = np.linspace(0, 1, n)
    f = 2 * np.pi**2 * np.sin(np.pi * x)[:, None] * np.sin(np.pi * x)[None, :]
    f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = 0
    return f


def solves(n, a, reps):
    levels = mg.default_max_levels(n, n)
    b = sine_rhs(n)
    tol = 1e-8 * float(np.sqrt(np.sum(b * b)) / (n - 1))
    kw = dict(max_levels=levels, cycle="V", pre=2, post=2, smoother=_lib.MG_JACOBI, omega=0.8)
    plain = mg.MultigridEngine(n, n, precision=_lib.MG_PREC_DOUBLE, **kw)
    pcg = {p: mg.PCGEngine(n, n, precision=code, **kw) for p, code in (("double", _lib.MG_PREC_DOUBLE), ("single_managed", _lib.MG_PREC_SINGLE_MANAGED))}
    if a is not None:
        plain.set_coefficient(a)
        for e in pcg.values():
            e.set_coefficient(a)
    rhs_t = torch.from_numpy(b).cuda()
    x_t = torch.zeros_like(rhs_t)
    plain.set_rhs(b)

    def run_plain():
        plain.set_solution(None)
        r = plain.iterate(tol, 100)
        return r["solve_seconds"], r["iterations"], r["converged"], r["residual_history"][-1]

    def run_pcg(p):
        x_t.zero_()
        torch.cuda.synchronize()
        r = pcg[p].solve_device(rhs_t, x_t, tol, 100)
        return r["solve_seconds"], r["iterations"], r["converged"], r["true_residual"], r["precond_seconds"], r["status"]

    run_plain()
    for p in pcg:
        run_pcg(p)                                                     # warm-up
    res = {"plain": [], "double": [], "single_managed": []}
    for _ in range(reps):                                              # alternate: drift hits all three alike
        res["plain"].append(run_plain())
        for p in pcg:
            res[p].append(run_pcg(p))
    t = statistics.median(r[0] for r in res["plain"])
    last = res["plain"][-1]
    say(f"  mg_iterate fp64          : {last[1]:3d} cycles     {'converged' if last[2] else 'NOT converged'}  ||r|| / tol {last[3] / tol:9.3g}"
        f"  {t * 1e3:8.3f} ms")
    for p in pcg:
        t = statistics.median(r[0] for r in res[p])
        tp = statistics.median(r[4] for r in res[p])
        last = res[p][-1]
        say(f"  PCG, M {p:15s}: {last[1]:3d} iterations {last[5]:14s} true ||r|| / tol {last[3] / tol:6.3g}  {t * 1e3:8.3f} ms"
            f"  (preconditioner {tp * 1e3:7.3f} ms)")
    plain.close()
    for e in pcg.values():
        e.close()


def kernels(n, reps=20):
    lib = _lib.load()
    ld = C.c_int(0)
    _lib.check(lib.mg_pitch_elems(_lib.MG_F64, n, C.byref(ld)))
    ld = ld.value
    nbytes = C.c_int64(0)
    _lib.check(lib.mg_dev_scratch_bytes(n, n, C.byref(nbytes)))
    f = lambda: torch.zeros((n, ld), dtype=torch.float64, device="cuda")
    z, p0, p1, q, x, r, a = (f() for _ in range(7))
    for t in (z, p0, x, r):
        t[1:-1, 1:n - 1] = torch.randn((n - 2, n - 2), dtype=torch.float64, device="cuda")
    a[:, :n] = 1.0
    scratch = torch.zeros(nbytes.value // 8, dtype=torch.float64, device="cuda")
    sc = torch.tensor([0.25, 1e-3, 0.0], dtype=torch.float64, device="cuda")     # beta, alpha, sink
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)
    h = 1.0 / (n - 1)
    calls = {
        "direction       (4 words)": (4, lambda: lib.mg_dev_pcg_direction(n, n, ld, h, h, -1.0, 0.0, None, P(z), P(p0), P(p1), P(q), P(sc), P(scratch), P(sc, 2), st)),
        "direction, var  (5 words)": (5, lambda: lib.mg_dev_pcg_direction(n, n, ld, h, h, -1.0, 0.0, P(a), P(z), P(p0), P(p1), P(q), P(sc), P(scratch), P(sc, 2), st)),
        "update          (6 words)": (6, lambda: lib.mg_dev_pcg_update(n, n, ld, P(sc, 1), P(p0), P(q), P(x), P(r), P(scratch), P(sc, 2), st)),
        "dots            (2 words)": (2, lambda: lib.mg_dev_pcg_dots(n, n, ld, P(r), P(z), None, P(scratch), P(sc, 2), P(sc, 2), st)),
        "dots, flexible  (3 words)": (3, lambda: lib.mg_dev_pcg_dots(n, n, ld, P(r), P(z), P(q), P(scratch), P(sc, 2), P(sc, 2), st)),
    }
    for name, (words, call) in calls.items():
        for _ in range(3):
            _lib.check(call())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            _lib.check(call())
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / reps
        say(f"  {name}: {us:8.1f} us per call (with its one-workgroup reduction)  {words * 8 * n * n / us * 1e-6:7.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1025, 4097])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pcg_times.txt"))
    args = ap.parse_args()
    say(f"pcg_probe: V(2,2) Jacobi 0.8, tol = 1e-8 ||r_0||, median of {args.reps} alternating solves, build {mg._build.source_hash()}")
    for n in args.sizes:
        for name, a in (("-Laplacian, sine rhs", None), ("-div(a grad .), checkerboard 8 x 8, contrast 1e4", checkerboard(n))):
            say(f"{n}^2  {name}")
            solves(n, a, args.reps)
        say(f"{n}^2  field kernels")
        kernels(n)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
