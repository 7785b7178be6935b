#!/usr/bin/env python3
"""Per-step wall time of the vorticity / stream-function stepper, the cycles of its two solves, and the hipEvent time of
flow_rhs_kernel.  python3 tools/flow_probe.py [--sizes 1025 4097] [--steps 10] [--warmup 3] [--out profiles/flow_times.txt]

The lid-driven cavity at Re = 1000 from rest, dt = h/2, solves to 1e-10.  The step figure is the wall time of `steps` steps
closed by one diagnostics() call (which synchronises).  The kernel figure is flow_rhs_kernel<N_prev, no forcing>: 5 words per
cell (psi, w, N_prev in; f, N out), timed over back-to-back launches on ONE set of arrays: where the five fit the 256 MiB
Infinity Cache (1025^2: 42 MB) the rate is a cache figure and the line says so; only a larger set (4097^2: 672 MB) streams
from HBM."""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mixed_precision_multigrid_solvers_for_pdes_amd as mg          # noqa: E402
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib      # noqa: E402

PEAK_TBS = 8.0
INFINITY_CACHE_BYTES = 256 << 20


def cavity_steps(n, steps, warmup):
    g = mg.Grid(n, n)
    with mg.VorticityStreamSolver(g, 1e-3, "no_slip", {"top": 1.0}, tolerance=1e-10, max_cycles=50) as s:
        dt = 0.5 * g.hx
        for _ in range(warmup):
            s.step(dt)
        s.diagnostics()
        t0 = time.perf_counter()
        infos = [s.step(dt) for _ in range(steps)]
        s.diagnostics()
        t = (time.perf_counter() - t0) / steps
    return t, [i["omega_cycles"] for i in infos], [i["psi_cycles"] for i in infos], all(i["converged"] for i in infos)


def rhs_kernel_time(n, reps=50):
    import torch
    lib = _lib.load()
    ld = C.c_int(0)
    _lib.check(lib.mg_pitch_elems(_lib.MG_F64, n, C.byref(ld)))
    nb = C.c_int64(0)
    _lib.check(lib.mg_dev_scratch_bytes(n, n, C.byref(nb)))
    psi, w, prev = (torch.rand((n, ld.value), dtype=torch.float64, device="cuda") for _ in range(3))
    f, N = torch.zeros_like(psi), torch.zeros_like(psi)
    scratch = torch.zeros(nb.value // 8, dtype=torch.float64, device="cuda")
    h = 1.0 / (n - 1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                        # noqa: E731

    def launch():
        _lib.check(lib.mg_dev_flow_rhs(n, n, ld.value, h, h, 1e-3, 0.5 * h, 1.5, -0.5, p(psi), p(w), p(prev), None, p(f), p(N),
                                       p(scratch), None, st))
    for _ in range(5):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps, 5 * 8 * n * ld.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1025, 4097])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flow_times.txt"))
    a = ap.parse_args()
    lines = [f"tools/flow_probe.py --steps {a.steps} --warmup {a.warmup}: lid-driven cavity, Re = 1000, from rest, dt = h/2, tol 1e-10; "
             "wall time per step; cycles per solve in brackets"]
    for n in a.sizes:
        t, wc, pc, ok = cavity_steps(n, a.steps, a.warmup)
        row = f"{n}^2 step {t * 1e3:9.3f} ms   vorticity solve {wc}   stream-function solve {pc}   all converged: {ok}"
        lines.append(row)
        print(row, flush=True)
        tk, working_set = rhs_kernel_time(n)
        tbs = 5 * 8 * n * n / tk / 1e12
        where = ("HBM" if working_set > INFINITY_CACHE_BYTES else
                 f"NOT an HBM figure: the {working_set / 2**20:.0f} MiB working set stays in the 256 MiB Infinity Cache")
        row = (f"{n}^2 flow_rhs_kernel<N_prev, no forcing> {tk * 1e6:8.1f} us (hipEvent, 50 launches)  5 words / cell  "
               f"{tbs:5.2f} TB/s  {tbs / PEAK_TBS:5.2f} of the {PEAK_TBS:g} TB/s HBM peak ({where})")
        lines.append(row)
        print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
