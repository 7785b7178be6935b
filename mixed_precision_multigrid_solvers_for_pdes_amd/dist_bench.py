"""bench.py --gpus N (N > 1): weak scaling of the decomposed solver, 4097^2 points per GPU, and the plan self-check that
runs before its clock starts."""
import importlib
import json
import os
import sys
import time

import numpy as np

from . import _lib
from .dist_layout import process_grid, sine_rhs_block
from .dist_ops import HipOps
from .dist_solve import DecomposedSolve
from .distributed import DistributedMultigrid


def _first_difference(a, b):
    """(i, j) of the first element where two equally shaped tensors differ bitwise, or None"""
    import torch
    ne = (a.view(torch.int64 if a.element_size() == 8 else torch.int32) != b.view(torch.int64 if b.element_size() == 8 else torch.int32))
    idx = torch.nonzero(ne)
    return None if idx.numel() == 0 else tuple(int(v) for v in idx[0])


def plan_selfcheck(sv, set_problem, dist):
    """Before the clock: one cycle through the Python driver and the same cycle replayed from the recorded plan, from the
    same start, must leave the same iterate BIT FOR BIT on every rank and the same norm.  Returns a dict for the bench line;
    mismatch = {"rank", "first_diff", ...} on the ranks that differ (the caller aborts non-zero)."""
    torch = sv.torch
    if not sv.native:
        return {"ran": False, "reason": "python driver only (no native plan on this backend / mode)"}
    (r, d), = sv.doms.items()
    b = d.blk[0]
    was = sv.native
    set_problem(sv)
    sv.native = False
    sv.cycle(0)
    n_py = sv.residual_norm()
    u_py = d.u[0][:b.lnx, :b.lny].clone()
    sv.native = was
    set_problem(sv)
    sv.cycle(0)                       # records (first time) or replays
    sv.residual_norm()
    if sv.native:                     # the recording did not fall back: this one is a replay for certain
        set_problem(sv)
        replays_before = sv.native_cycles
        sv.cycle(0)
        n_na = sv.residual_norm()
        replayed = sv.native_cycles == replays_before + 1
        u_na = d.u[0][:b.lnx, :b.lny]
        diff = _first_difference(u_py, u_na)
        bad = (diff is not None) or not (n_py == n_na)
    else:
        replayed, diff, bad, n_na = False, None, False, n_py
    flag = torch.tensor([1 if bad else 0], dtype=torch.int32, device=u_py.device)
    if dist is not None:
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
    res = {"ran": True, "replayed": bool(replayed), "bit_identical": not bool(int(flag.item())), "norm_python": n_py, "norm_native": n_na}
    if bad:
        res["mismatch"] = {"rank": r, "block": [b.gx0, b.gy0, b.lnx, b.lny], "first_diff": diff}
    return res


def bench_main(args, rank, local_rank, world):
    """bench.py --gpus N (N > 1): BASELINE config 3's workload per GPU (4097^2, adaptive fp32 -> fp64, V(2,2) weighted
    Jacobi) on a px x py block decomposition -- weak scaling of the N = 1 bench line.  The precision policy is the
    engine's (core/precision.py:270-302 with the one-way promotion): start in double, drop to single while
    ||r|| > 100 thr, promote for good once ||r|| < 10 thr; it switches between two solvers that share the decomposition
    (DecomposedSolve: the loop DistributedMultigridSolver.solve runs too).

    Before the clock starts the run checks itself: every rank of the communicator is counted (`ranks_seen`), one cycle is
    run through the Python driver and replayed from the recorded plan from the same start and the two iterates are compared
    bit for bit (`selfcheck`; a mismatch prints the first differing block and exits non-zero).  After the timed region three
    diagnostic cycles are bracketed with timing events per phase (`phases_ms_per_cycle`: legs, halo copies, send/recv groups
    incl. the wait for the peers, coarse all-gather, replicated engine, all-reduce).  A rank whose plan times out
    (MG_PLAN_TIMEOUT_S) reports and leaves with os._exit -- it never synchronises on the stuck streams again.

    Test hook (tests/test_distributed_cpu.py): MG_DIST_BACKEND=gloo with MG_BENCH_OPS=module:Class runs the same driver
    on CPU tensors with a stand-in kernel provider; without it the kernels are libmghip's and a GPU is required."""
    import torch
    import torch.distributed as dist
    if world != args.gpus:
        raise RuntimeError(f"bench.py --gpus {args.gpus} under a launcher that started {world} ranks (WORLD_SIZE)")
    # rehearsal knobs (one-GPU box): MG_DIST_BACKEND=gloo MG_DIST_SAME_DEVICE=1 runs every rank on cuda:0 over gloo
    backend = os.environ.get("MG_DIST_BACKEND", "nccl")
    ops_spec = os.environ.get("MG_BENCH_OPS") if backend == "gloo" else None
    on_gpu = ops_spec is None
    if os.environ.get("MG_DIST_SAME_DEVICE") == "1":
        local_rank = 0
    if on_gpu:
        assert torch.cuda.is_available(), "bench.py --gpus N needs MI355X devices (no CPU fallback)"
        torch.cuda.set_device(local_rank)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group(backend)
    try:
        return _bench_ranks(args, rank, local_rank, world, backend, ops_spec, on_gpu)
    except _lib.PlanTimeout as exc:
        # the RCCL work of the stuck cycle is still queued: any synchronisation (torch.cuda.synchronize, mg_destroy, hipFree,
        # destroy_process_group) would hang on it.  Report and leave; the launcher tears the other ranks down.
        sys.stderr.write(f"bench.py rank {rank}: {exc}\n")
        sys.stderr.flush()
        os._exit(3)


def _bench_ranks(args, rank, local_rank, world, backend, ops_spec, on_gpu):
    import torch
    import torch.distributed as dist
    px, py = process_grid(world)
    m = args.n - 1
    NX, NY = px * m + 1, py * m + 1
    # unit cells: the domain grows with the process grid so that hx = hy = 1/(n-1) as on one GPU
    domain = (0.0, float(px), 0.0, float(py))
    thr = 1e-6                                                    # BASELINE config 3: switch_threshold
    if on_gpu:
        dev = torch.device("cuda", local_rank)
        providers = (("f32", HipOps(np.float32, dev, managed_single=True)), ("f64", HipOps(np.float64, dev)))
    else:
        modname, cls = ops_spec.split(":")
        factory = getattr(importlib.import_module(modname), cls)
        providers = (("f32", factory(np.float32)), ("f64", factory(np.float64)))
    sync = torch.cuda.synchronize if on_gpu else (lambda: None)
    solvers = {}
    # MG_DIST_NATIVE=0: the Python driver every cycle (default: recorded cycle plans wherever they apply)
    native = "auto" if os.environ.get("MG_DIST_NATIVE", "1") != "0" else False
    for name, ops in providers:
        solvers[name] = DistributedMultigrid(NX, NY, px, py, [rank], ops, dist, domain=domain, smoother="jacobi", omega=0.8,
                                             cycle="V", pre=2, post=2, agglomerate_at=getattr(args, "agglomerate_at", 1025),
                                             native=native)
    loop = DecomposedSolve(solvers, "adaptive", thr)
    rhs_of = lambda b: sine_rhs_block(b, domain)

    # ---- who is here: every rank adds one, over torch.distributed and (native plans) over the library's own communicator ----
    seen = torch.ones(1, dtype=torch.int32, device="cuda" if (on_gpu and backend == "nccl") else "cpu")
    dist.all_reduce(seen)
    ranks_seen = int(seen.item())
    who = [None] * world
    dist.all_gather_object(who, {"rank": rank, "device": (torch.cuda.current_device() if on_gpu else "cpu"), "pid": os.getpid()})

    # ---- untimed set-up: the plan self-check builds both cycle plans (and the library's RCCL communicator) -------------------
    checks = {}
    for name, sv in solvers.items():
        checks[name] = plan_selfcheck(sv, lambda s: s.set_problem(rhs_of), dist)
    failed = [c for c in checks.values() if c.get("ran") and not c["bit_identical"]]
    if failed:
        for name, c in checks.items():
            if "mismatch" in c:
                sys.stderr.write(f"bench.py rank {rank}: native replay != Python driver ({name}): {json.dumps(c['mismatch'])}\n")
        sys.stderr.flush()
        sync()
        dist.barrier()
        for x in solvers.values():
            x.close()
        dist.destroy_process_group()
        return 4
    comm_ranks = None
    for sv in solvers.values():
        if sv._comm is not None:
            comm_ranks = sv._comm.ranks()[0]
    for sv in solvers.values():           # the Python-driver fallback needs its warm-up too
        if not sv.native:
            sv.set_problem(rhs_of)
            sv.cycle(0)
            sv.residual_norm()

    K, W = args.steps, args.warmup
    loop.set_problem(rhs_of)
    for _ in range(W):
        loop.step()
    r0 = loop.set_problem(rhs_of)
    hist, phases = [], []
    for sv in solvers.values():
        sv.exchanges = 0
        sv.native_cycles = 0
    dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(K):
        hist.append(loop.step())
        phases.append(loop.policy.phase)
    sync()
    dist.barrier()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], dtype=torch.float64, device="cuda" if (on_gpu and backend == "nccl") else "cpu")
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    exchanges = sum(x.exchanges for x in solvers.values()) / max(1, K)
    native_cycles = sum(x.native_cycles for x in solvers.values())
    # iterations to tolerance / the plateau of the reference's absolute norm (untimed continuation of the same solve)
    long_hist = list(hist)
    for _ in range(max(0, 40 - K)):
        long_hist.append(loop.step())
    tail = sorted(long_hist[-5:])
    floor = tail[len(tail) // 2]
    first = lambda vals, t: next((k + 1 for k, v in enumerate(vals) if v < t), None)
    # ---- per-phase device times: three more cycles of the dominant precision, every phase bracketed by timing events ------
    dom = "f64" if phases.count("f64") >= phases.count("f32") else "f32"
    sv = solvers[dom]
    sv.profile_phases(True)
    ncyc = 3
    for _ in range(ncyc):
        sv.cycle(0)
        sv.residual_norm()
    ph = sv.collect_phase_times()
    sv.profile_phases(False)
    phases_ms = {k: v / ncyc for k, v in ph.items()}
    # roofline leg (rank 0): the dominant kernel of the timed region -- the level-0 up leg (prolongation + 2 sweeps +
    # norm) of the precision that ran most cycles -- on this rank's block, timed with events on its own stream
    b0, leg = sv.level0_up_leg(rank)
    reps = 20 if on_gpu else 1
    leg()
    if on_gpu:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(reps):
            leg()
        ev1.record()
        torch.cuda.synchronize()
        ms_leg = ev0.elapsed_time(ev1) / reps
    else:
        t1 = time.perf_counter()
        leg()
        ms_leg = (time.perf_counter() - t1) * 1e3
    w = 8 if dom == "f64" else 4
    moved, unfused = 3.25 * w * b0.lnx * b0.lny, 10.25 * w * b0.lnx * b0.lny
    if rank == 0:
        value = NX * NY * K / dt / 1e6
        s0 = solvers["f64"]
        gbs = moved / (ms_leg * 1e-3) / 1e9
        print(json.dumps({
            "metric": "MDoF/s per V-cycle on 2D Poisson", "value": value, "unit": "MDoF/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": dt / K * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32->f64 (adaptive)", "data": "synthetic",
            "config": {"workload": f"2D Poisson {NX}x{NY} adaptive fp32->fp64 (switch_threshold={thr:g}), V(2,2) weighted-Jacobi "
                                   f"omega=0.8, {px}x{py} block decomposition ({args.n}^2 per GPU), RCCL halo exchange ({s0.mode} legs, "
                                   f"ghost width {s0.G}), {s0.L} levels ({s0.Ld} distributed, rest replicated after all-gather)",
                       "grid": [NX, NY], "levels": s0.L, "cycle": "V(2,2)", "smoother": "jacobi",
                       "parallelism": f"dd{px}x{py}", "backend": backend if on_gpu else f"{backend} (CPU rehearsal, {ops_spec})"},
            "cycles_fp32": phases.count("f32"), "cycles_fp64": phases.count("f64"),
            "residual_initial": r0, "residual_first": hist[0], "residual_last": hist[-1],
            "iterations": K, "iterations_to_1e-10_absolute": first(long_hist, 1e-10),
            "iterations_to_1e-10_relative": first([v / r0 for v in long_hist], 1e-10),
            "iterations_to_1e-9_absolute": first(long_hist, 1e-9),
            "residual_floor": floor, "iterations_to_floor": first(long_hist, 2.0 * floor),
            "roofline": {"bound": "hbm", "kernel": f"fused up leg ({'rb_leg_kernel' if b0.lnx * b0.lny > 1100 * 1100 else 'fused_jacobi_kernel'}) {dom} on the local {b0.lnx}x{b0.lny} block (rank 0, level 0)",
                         "achieved": gbs, "peak": 8000.0, "unit": "GB/s", "frac": gbs / 8000.0, "traffic": None, "launch_ms": ms_leg,
                         "bytes_per_launch": moved, "unfused_equivalent_bytes": unfused,
                         "unfused_equivalent_gbs": unfused / (ms_leg * 1e-3) / 1e9,
                         "note": "achieved = bytes the launch must move (3.25 words per cell of the local block, ghost zone "
                                 "included) / launch time; unfused_equivalent_* prices the same work as one launch per operator "
                                 "(SURVEY 8d)"},
            "exchanges_per_cycle": exchanges,
            "ranks_seen": ranks_seen, "rank_devices": who,
            "driver": {"native_plan_cycles": native_cycles, "python_cycles": K - native_cycles,
                       "fallback": next((x.native_failure for x in solvers.values() if x.native_failure), None),
                       "rccl_comm_ranks": comm_ranks,
                       # level-0 up legs of cycle k + down legs of cycle k + 1 as one launch per block (MG_DIST_SPAN=0: two)
                       "spanning_scheme": {name: bool(x._span_usable()) for name, x in solvers.items()},
                       "rccl_multi_rank_replay": ("exercised in this run" if (native_cycles > 0 and world > 1 and backend == "nccl") else
                                                  "not exercised (no multi-rank RCCL plan ran here)"),
                       "selfcheck": checks},
            "phases_ms_per_cycle": dict(phases_ms, precision=dom, cycles=ncyc, rank=0,
                                        source=("timing events inside mg_plan_run" if sv.native else
                                                ("timing events around the Python driver's phases" if on_gpu else "wall clock (CPU rehearsal)"))),
            "note": "distributed levels: communication-avoiding fused legs (two launches and about one halo exchange per "
                    "level and cycle); a cycle is recorded once through the Python driver and then replayed from C++ -- one "
                    "mg_plan_run per cycle enqueues the kernels, the RCCL send/recv groups, the coarse all-gather and the "
                    "norm all-reduce on two HIP streams (MG_DIST_NATIVE=0: torch.distributed P2P from Python every cycle); "
                    "the replicated coarse hierarchy runs on the fused single-GPU engine; same precision policy as the "
                    "N = 1 line; multi-rank RCCL replay has never run before the first real multi-GPU run: `driver` says which "
                    "path this run took and `selfcheck` that replay and Python driver agreed bit for bit before the clock",
        }), flush=True)
    for x in solvers.values():
        x.close()
    if on_gpu:
        from . import dist_plan
        dist_plan.shutdown()
    dist.destroy_process_group()
    return 0
