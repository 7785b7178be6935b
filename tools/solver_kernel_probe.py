#!/usr/bin/env python3
"""hipEvent times of the LDS-tiled kernels of the solver modules, each through its stateless mg_dev_* entry point (needs a GPU).

    python3 tools/solver_kernel_probe.py [sizes ...] [--only substring] [--json run.json]
    python3 tools/solver_kernel_probe.py --compare parentA.json headA.json parentB.json headB.json [--out profiles/solver_kernel_times.txt]

A run warms every case up, then takes the hipEvent time of 50 launches (each with its one-workgroup reduction where the entry
point has one), `--reps` times over, and prints the median and the min - max of those repeats.  The library is the one
MGHIP_LIBRARY names (default: the built one), so two builds are compared by alternating runs of this tool in one job, each its
own process.  --compare pools the repeats of the runs it is given (even positions: parent, odd: head), writes both sets of
numbers and fails (exit 1) where a head median exceeds the parent median by more than the parent's own min - max spread."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = 50


def cases(lib, torch, n):
    from mixed_precision_multigrid_solvers_for_pdes_amd import _lib
    ld = C.c_int(0)
    _lib.check(lib.mg_pitch_elems(_lib.MG_F64, n, C.byref(ld)))
    ld = ld.value
    nbytes = C.c_int64(0)
    _lib.check(lib.mg_dev_scratch_bytes(n, n, C.byref(nbytes)))
    gen = torch.Generator(device="cuda").manual_seed(1234)

    def field(ring=False, cols=1):
        t = torch.zeros((cols * n, ld), dtype=torch.float64, device="cuda")
        v = t.view(cols, n, ld)
        if ring:
            v[:, :, :n] = 0.1 * torch.randn((cols, n, n), dtype=torch.float64, device="cuda", generator=gen)
        else:
            v[:, 1:-1, 1:n - 1] = 0.1 * torch.randn((cols, n - 2, n - 2), dtype=torch.float64, device="cuda", generator=gen)
        return t

    a = field(ring=True)
    a[:, :n] = 1.0 + a[:, :n].abs()
    u, up, z, p0, f, w = field(ring=True), field(ring=True), field(), field(), field(), field(ring=True)
    o0, o1, o2 = field(), field(), field()
    v4, av4 = field(cols=4), field(cols=4)
    scratch = torch.zeros(nbytes.value // 8, dtype=torch.float64, device="cuda")
    sc = torch.tensor([0.25, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda")     # beta, then the sums' sink
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)
    h = 1.0 / (n - 1)
    S = P(scratch), P(sc, 1), st
    CN, CUBIC = 2, 1
    return {
        "pcg_direction": lambda: lib.mg_dev_pcg_direction(n, n, ld, h, h, -1.0, 0.0, None, P(z), P(p0), P(o0), P(o1), P(sc), *S),
        "pcg_direction var": lambda: lib.mg_dev_pcg_direction(n, n, ld, h, h, -1.0, 0.0, P(a), P(z), P(p0), P(o0), P(o1), P(sc), *S),
        "heat_rhs CN": lambda: lib.mg_dev_heat_rhs_var(CN, n, n, ld, h, h, 0.5, 1e-3, P(u), None, None, None, 1.0, 1.0, P(o0), *S),
        "heat_rhs CN var": lambda: lib.mg_dev_heat_rhs_var(CN, n, n, ld, h, h, 0.5, 1e-3, P(u), None, None, P(a), 1.0, 1.0, P(o0), *S),
        "rd_rhs CN cubic": lambda: lib.mg_dev_rd_rhs(CN, CUBIC, n, n, ld, h, h, 0.5, 1e-3, 1.0, 0.5, P(u), P(up), None, None, None, 1.0, 1.0, P(o0), *S),
        "rd_energy": lambda: lib.mg_dev_rd_energy(CUBIC, n, n, ld, h, h, None, None, P(u), *S),
        "nl_eval cubic": lambda: lib.mg_dev_nl_eval(CUBIC, n, n, ld, h, h, -1.0, 0.0, 1.0, None, None, P(u), P(z), 0.5, P(f), P(o0), P(o1), P(o2), *S),
        "nl_eval cubic var": lambda: lib.mg_dev_nl_eval(CUBIC, n, n, ld, h, h, -1.0, 0.0, 1.0, P(a), None, P(u), P(z), 0.5, P(f), P(o0), P(o1), P(o2), *S),
        "eig_apply 4 cols": lambda: lib.mg_dev_eig_apply(n, n, ld, 4, n * ld, h, h, -1.0, None, P(v4), P(av4), st),
        "ho_direction": lambda: lib.mg_dev_ho_direction(n, n, ld, h, h, -1.0, 0.0, P(z), P(p0), P(o0), P(o1), P(sc), *S),
        "ho_residual": lambda: lib.mg_dev_ho_residual(n, n, ld, h, h, -1.0, 0.0, P(u), P(f), P(o0), *S),
        "ho_rhs": lambda: lib.mg_dev_ho_rhs(n, n, ld, P(f), P(o0), st),
        "flow_rhs": lambda: lib.mg_dev_flow_rhs(n, n, ld, h, h, 1e-3, 1e-3, 1.5, -0.5, P(u), P(w), P(f), None, P(o0), P(o1), *S),
    }, (a, u, up, z, p0, f, w, o0, o1, o2, v4, av4, scratch, sc)


def measure(sizes, reps, only=""):
    sys.path.insert(0, ROOT)
    import hashlib
    from mixed_precision_multigrid_solvers_for_pdes_amd import _lib
    import torch
    lib = _lib.load()
    path = _lib.library_path()
    result = {"library": os.path.basename(path), "build": hashlib.sha1(open(path, "rb").read()).hexdigest()[:12], "times_us": {}}
    print(f"solver_kernel_probe: {LAUNCHES} launches per repeat, {reps} repeats, library {result['library']}", flush=True)
    for n in sizes:
        calls, keep = cases(lib, torch, n)
        for name, call in calls.items():
            if only not in name:
                continue
            for _ in range(3):
                _lib.check(call())
            torch.cuda.synchronize()
            us = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LAUNCHES):
                    _lib.check(call())
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
            result["times_us"][f"{n}^2 {name}"] = us
            print(f"  {n:5d}^2 {name:20s}: median {statistics.median(us):9.2f} us  min {min(us):9.2f}  max {max(us):9.2f}", flush=True)
        del calls, keep
    return result


def compare(paths, out):
    runs = [json.load(open(p)) for p in paths]
    pooled = [{}, {}]
    for i, r in enumerate(runs):
        for k, us in r["times_us"].items():
            pooled[i % 2].setdefault(k, []).extend(us)
    lines = [f"solver_kernel_probe --compare: us per launch, {LAUNCHES} launches per repeat; pooled repeats of the alternating runs "
             f"{', '.join(os.path.basename(p) for p in paths)} (parent {runs[0]['library']} {runs[0]['build']}, head {runs[1]['library']} {runs[1]['build']})",
             "accept: head median <= parent median + (parent max - parent min)", "",
             f"{'kernel':30s} {'parent median':>13s} {'min':>9s} {'max':>9s} | {'head median':>11s} {'min':>9s} {'max':>9s} | {'head/parent':>11s}"]
    worst, failed = (0.0, ""), []
    for k in pooled[0]:
        p, h = pooled[0][k], pooled[1][k]
        pm, hm = statistics.median(p), statistics.median(h)
        ok = hm <= pm + (max(p) - min(p))
        worst = max(worst, (hm / pm, k))
        if not ok:
            failed.append(k)
        lines.append(f"{k:30s} {pm:13.2f} {min(p):9.2f} {max(p):9.2f} | {hm:11.2f} {min(h):9.2f} {max(h):9.2f} | {hm / pm:11.4f}{'' if ok else '  OVER'}")
    lines += ["", f"worst head/parent ratio of medians: {worst[0]:.4f} ({worst[1]})", f"over the parent's spread: {', '.join(failed) if failed else 'none'}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as fh:
        fh.write(text)
    return 1 if failed else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1025, 4097])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="", help="only the cases whose name contains this")
    ap.add_argument("--json")
    ap.add_argument("--compare", nargs="+")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_kernel_times.txt"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare, args.out))
    result = measure(args.sizes, args.reps, args.only)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh)


if __name__ == "__main__":
    main()
