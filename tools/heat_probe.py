#!/usr/bin/env python3
"""Per-step wall time of the heat stepper, device-resident against the host path, in one process; and the hipEvent time of
heat_rhs_kernel.  python3 tools/heat_probe.py [--sizes 1025 4097] [--steps 10] [--warmup 2] [--out profiles/heat_times.txt]

Crank-Nicolson and BDF2, no source, zero Dirichlet data, dt = 0.1 h.  The device figure is
the wall time of `steps` steps on slots closed by one diff_norm (which synchronises); the host figure the wall time of `steps`
calls of HeatEquationSolver._single_time_step on host arrays (device_resident=False: upload, cycles, download, NumPy around
them).  The host path has no BDF2.  The kernel figure is Crank-Nicolson without a source: 2 words per cell (u in, f out),
timed over back-to-back launches on ONE pair of arrays: where the pair fits the 256 MiB Infinity Cache (1025^2: 18 MB) the
rate is a cache figure and the line says so; only a larger pair (4097^2: 273 MB) streams from HBM."""
import argparse
import ctypes as C
import os
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mixed_precision_multigrid_solvers_for_pdes_amd as mg          # noqa: E402
from mixed_precision_multigrid_solvers_for_pdes_amd import _lib      # noqa: E402
from mixed_precision_multigrid_solvers_for_pdes_amd import heat_equation as H   # noqa: E402

PEAK_TBS = 8.0
INFINITY_CACHE_BYTES = 256 << 20


def device_steps(n, scheme, steps, warmup):
    g = mg.Grid(n, n)
    hs = H.HeatEquationSolver(H.HeatEquationConfig(thermal_diffusivity=1.0, initial_condition=H.create_gaussian_initial_condition()),
                              g, device_resident=True)
    hs.set_initial_condition()
    dt = 0.1 * g.hx
    cur, prev, cycles = 0, None, []

    def advance(k):
        nonlocal cur, prev
        new = hs._free_slots(cur, prev)[0]
        info = hs._device_step(cur, new, dt, scheme, k * dt, prev)
        cycles.append(info["cycles"])
        prev, cur = cur, new

    for k in range(warmup):
        advance(k)
    hs.stepper.diff_norm(cur, cur)
    del cycles[:]
    t0 = time.perf_counter()
    for k in range(warmup, warmup + steps):
        advance(k)
    hs.stepper.diff_norm(cur, cur)
    t = (time.perf_counter() - t0) / steps
    hs.stepper.close()
    return t, cycles


def host_steps(n, scheme, steps, warmup):
    g = mg.Grid(n, n)
    hs = H.HeatEquationSolver(H.HeatEquationConfig(thermal_diffusivity=1.0, initial_condition=H.create_gaussian_initial_condition()), g)
    u = hs.set_initial_condition()
    dt = 0.1 * g.hx
    for _ in range(warmup):
        u = hs._single_time_step(u, dt, scheme)
    n0 = len(hs.helmholtz_stats)
    t0 = time.perf_counter()
    for _ in range(steps):
        u = hs._single_time_step(u, dt, scheme)
    t = (time.perf_counter() - t0) / steps
    cycles = [c for _, c, _ in hs.helmholtz_stats[n0:]]
    hs.mg_solver.close()
    return t, cycles


def rhs_kernel_time(n, reps=50):
    import torch
    lib = _lib.load()
    ld = C.c_int(0)
    _lib.check(lib.mg_pitch_elems(_lib.MG_F64, n, C.byref(ld)))
    nb = C.c_int64(0)
    _lib.check(lib.mg_dev_scratch_bytes(n, n, C.byref(nb)))
    u = torch.rand((n, ld.value), dtype=torch.float64, device="cuda")
    out = torch.zeros_like(u)
    scratch = torch.zeros(nb.value // 8, dtype=torch.float64, device="cuda")
    h = 1.0 / (n - 1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        _lib.check(lib.mg_dev_heat_rhs(_lib.MG_HEAT_CRANK_NICOLSON, n, n, ld.value, h, h, 1.0, 0.1 * h, C.c_void_p(u.data_ptr()), None, None,
                                       0.0, 0.0, C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), None, st))
    for _ in range(5):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps, 2 * 8 * n * ld.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1025, 4097])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "heat_times.txt"))
    a = ap.parse_args()
    lines = [f"tools/heat_probe.py --steps {a.steps} --warmup {a.warmup}: wall time per step (dt = 0.1 h, tol 1e-10, <= 20 cycles); cycles per step in brackets"]
    for n in a.sizes:
        for scheme in (H.TimeSteppingScheme.CRANK_NICOLSON, H.TimeSteppingScheme.BDF2):
            td, cd = device_steps(n, scheme, a.steps, a.warmup)
            row = f"{n}^2 {scheme.value:15s} device-resident {td * 1e3:9.3f} ms {cd}"
            if scheme == H.TimeSteppingScheme.CRANK_NICOLSON:
                th, ch = host_steps(n, scheme, a.steps, a.warmup)
                row += f"   host path {th * 1e3:9.3f} ms {ch}   host / device {th / td:6.2f} x"
            else:
                row += "   host path: no BDF2"
            lines.append(row)
            print(row, flush=True)
        tk, working_set = rhs_kernel_time(n)
        tbs = 2 * 8 * n * n / tk / 1e12
        where = ("HBM" if working_set > INFINITY_CACHE_BYTES else
                 f"NOT an HBM figure: the {working_set / 2**20:.0f} MiB working set stays in the 256 MiB Infinity Cache")
        row = (f"{n}^2 heat_rhs_kernel<crank_nicolson, no source> {tk * 1e6:8.1f} us (hipEvent, 50 launches)  2 words / cell  "
               f"{tbs:5.2f} TB/s  {tbs / PEAK_TBS:5.2f} of the {PEAK_TBS:g} TB/s HBM peak ({where})")
        lines.append(row)
        print(row, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
