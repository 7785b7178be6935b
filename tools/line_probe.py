#!/usr/bin/env python3
"""Time per full zebra line sweep (both colours) against the red-black Gauss-Seidel sweep, and the user-visible gain on an
anisotropic grid.  python3 tools/line_probe.py [--reps 20] [--rounds 5] [--limit 600] [--out profiles/line_times.txt]

One measuring process, started under `timeout` so that a hang ends it.  Per shape (1025^2, 4097^2, 513 x 8193), dtype and
direction: mg_line_time_sweep (hipEvents around `reps` sweeps after two warm-up sweeps, arrays of pseudo-random data the call
allocates), `rounds` times interleaved with mg_time_op op 1 -- the red-black sweep on a handle of the same shape -- in the
same process; median and minimum of the rounds.  Then cycles to ||r|| < 1e-9 and the solve's device time on 513 x 4097 over
the unit square (the 33 x 257 aspect ratio at a size where launches no longer dominate), line cycle against red-black cycle.
Arrays up to 4097^2 fp64 (134 MB each) fit the 256 MiB Infinity Cache pairwise or not at all: the table says which."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1025, 1025), (4097, 4097), (513, 8193)]


def measure(args):
    import numpy as np
    from mixed_precision_multigrid_solvers_for_pdes_amd import _lib
    from mixed_precision_multigrid_solvers_for_pdes_amd.engine import MultigridEngine
    so = _lib.load()
    lines = ["# zebra line sweep vs red-black sweep, ms per full sweep: median (min) of %d rounds x %d reps; build %s" %
             (args.rounds, args.reps, __import__("mixed_precision_multigrid_solvers_for_pdes_amd")._build.source_hash()),
             "%-12s %-4s %-22s %-22s %-22s %-8s %-8s" % ("shape", "dt", "rbgs", "zebra_x", "zebra_y", "x/rbgs", "y/rbgs")]
    for nx, ny in SHAPES:
        for dt, prec in ((np.float64, _lib.MG_PREC_DOUBLE), (np.float32, _lib.MG_PREC_SINGLE)):
            code = _lib.dtype_code(dt)
            ld = C.c_int(0)
            _lib.check(so.mg_pitch_elems(code, ny, C.byref(ld)))
            hx, hy = 1.0 / (nx - 1), 1.0 / (ny - 1)
            plans = {}
            for name, d in (("x", _lib.MG_ZEBRA_X), ("y", _lib.MG_ZEBRA_Y)):
                plans[name] = C.c_void_p(None)
                _lib.check(so.mg_line_plan_create(code, d, nx, ny, ld.value, hx, hy, 0.0, C.byref(plans[name])))
            times = {"rbgs": [], "x": [], "y": []}
            with MultigridEngine(nx, ny, max_levels=2, smoother=_lib.MG_RBGS, omega=1.0, precision=prec, fused=0) as eng:
                rng = np.random.default_rng(0)
                eng.set_rhs(rng.standard_normal((nx, ny)).astype(dt))
                eng.set_solution(rng.standard_normal((nx, ny)).astype(dt))
                for _ in range(args.rounds):
                    times["rbgs"].append(eng.time_op("rbgs", 0, dt, args.reps))
                    for name in ("x", "y"):
                        out = C.c_double(0.0)
                        _lib.check(so.mg_line_time_sweep(plans[name], args.reps, C.byref(out)))
                        times[name].append(out.value)
            for p in plans.values():
                so.mg_line_plan_destroy(p)
            med = {k: statistics.median(v) for k, v in times.items()}
            cell = {k: "%.4f (%.4f)" % (med[k], min(times[k])) for k in times}
            lines.append("%-12s %-4s %-22s %-22s %-22s %-8.2f %-8.2f" % ("%dx%d" % (nx, ny), np.dtype(dt).name[-2:], cell["rbgs"], cell["x"],
                                                                       cell["y"], med["x"] / med["rbgs"], med["y"] / med["rbgs"]))
            print(lines[-1], flush=True)
    nx, ny = 513, 4097
    rng = np.random.default_rng(1)
    rhs, u0 = rng.standard_normal((nx, ny)), rng.standard_normal((nx, ny))
    for a in (rhs, u0):
        a[0, :] = a[-1, :] = 0.0
        a[:, 0] = a[:, -1] = 0.0
    lines.append("# 513x4097 on the unit square, V(2,2), all levels, fp64: cycles to ||r|| < 1e-9 (at most 60) and the solve's seconds")
    for name, sm in (("zebra_y", _lib.MG_ZEBRA_Y), ("rbgs", _lib.MG_RBGS)):
        with MultigridEngine(nx, ny, max_levels=32, smoother=sm, omega=1.0) as eng:
            eng.solve(rhs, u0, tol=1e-9, max_iterations=2)                    # warm-up
            _, info = eng.solve(rhs, u0, tol=1e-9, max_iterations=60)
        lines.append("%-8s cycles %3d converged %-5s final %.3e solve_seconds %.4f" % (name, info["iterations"], info["converged"],
                                                                                    info["residual_history"][-1], info["solve_seconds"]))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds the measuring process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
           "--rounds", str(args.rounds)] + (["--out", args.out] if args.out else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
