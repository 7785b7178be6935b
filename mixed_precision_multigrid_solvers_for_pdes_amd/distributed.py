"""Block domain decomposition of the multigrid hierarchy over the GPUs of one node.

One process per GPU (torch.distributed; backend "nccl" is RCCL over xGMI on ROCm, "gloo" on CPU for the
tests).  The reference has no communication backend at all (gpu/multi_gpu.py:540-607 solves
sub-domains independently, gpu/multi_gpu_solver.py:90-185 copies slices between CuPy devices); what is
kept from it is the partitioning idea (2-D blocks with a 1-cell overlap, gpu/multi_gpu.py:386-476,
gpu/multi_gpu_solver.py:30-64) -- the algorithm here is the SAME V/W-cycle as the single-GPU engine,
decomposition-invariant by construction:

  * the global vertex grid (NX, NY) is cut at indices c_k = k (NX-1)/px (even on every distributed
    level); rank (rx, ry) stores global rows c_rx .. c_rx+1 + 1: its owned cells plus a 1-cell ring
    that is either the physical boundary or a ghost copy of the neighbour's edge.  Local cell (0,0) has
    an even global index, so coarse cell (ic, jc) sits on local fine cell (2ic, 2jc) on every rank and
    the red/black colouring is the global one;
  * mode "fused" (default; communication-avoiding): every rank keeps a ghost ZONE of G cells and runs the same
    two fused kernels per level as the single-GPU engine (down leg: 2 sweeps + residual + restriction; up leg:
    prolongation + 2 sweeps [+ norm]) on its whole local array, recomputing inside the ghost zone what the
    neighbour computes too; each Jacobi sweep / GS colour pass / residual / transfer invalidates one more ghost
    cell from the outside; G = 7 (weighted Jacobi) and G = 13 (red-black GS) are the smallest odd widths for
    which the owned cells stay exact through every V / W / F visit (GHOST_FUSED below).
    Exchanges per cycle: the fine iterate once (G rows / columns per neighbour) and each coarse right-hand side
    once -- L_d + 1 exchanges instead of 5 L_d, each a few hundred KB instead of 16 KB, and two launches per level;
  * mode "per_operator": 1-cell ghost ring, one launch per operator (the kernels pass the ring through); every
    sweep (every colour) is followed by a halo exchange of u; the residual gets one exchange (with corners)
    before full-weighting restriction; prolongation interpolates the ghost ring from the exchanged coarse ghost
    values, so no exchange is needed after the correction;
  * below `agglomerate_at` points per direction the remaining coarse hierarchy is solved redundantly on
    every GPU by the single-GPU engine after one all-gather of the coarse right-hand side: no broadcast
    back, no latency-bound tiny halo messages;
  * ||r|| is an all-reduce of one fp64 partial sum per rank over exactly the cells each rank owns.

Messages are G rows / columns (118 KB at 4097^2 fp32, G = 7; 16-32 KB per 1-cell ring in per-operator mode):
latency-bound, each neighbour pair on its own xGMI link.  Fields live in torch tensors (device memory, streams); the arithmetic is libmghip's
device-pointer entry points (mg_dev_*).  `ops` and `comm` are injected so that the decomposition logic
runs unchanged (a) on CPU under gloo with a NumPy stand-in for the kernels (tests) and (b) with several
virtual ranks in one process on one GPU (tests), besides (c) the real thing.
"""
import collections
import contextlib
import math
import os
import time

import numpy as np

from . import _lib
from .dist_layout import (SIDE_ILO, SIDE_IHI, SIDE_JLO, SIDE_JHI, GHOST_FUSED, Block, distributed_levels,      # noqa: F401
                          hierarchy_shapes, process_grid, sine_rhs_block)
from .dist_ops import HipOps                                                                                   # noqa: F401
from .dist_solve import AdaptivePolicy, DecomposedSolve, FixedPolicy, fp32_phase_pays, stagnating              # noqa: F401


class _Dom:
    """Per-rank state: one Block per distributed level and its fields."""


# What the fused legs of one block on one level are launched with (DistributedMultigrid._leg)
_Leg = collections.namedtuple("_Leg", "b bc ci cj e target poff win kw")


class _Phase:
    """`with solver._ph(name):` -- adds the time of the enclosed work to solver.phase_times[name] when profiling is on"""

    def __init__(self, owner, name):
        self.o, self.name = owner, name

    def __enter__(self):
        o = self.o
        self.on = o.phase_times is not None
        if not self.on:
            return self
        self.cuda = bool(getattr(o.ops, "supports_overlap", False))        # device kernels: stream-ordered timing events
        if self.cuda:
            self.e0 = o.torch.cuda.Event(enable_timing=True)
            self.e0.record()
        else:
            self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        if not self.on:
            return False
        o = self.o
        if self.cuda:
            e1 = o.torch.cuda.Event(enable_timing=True)
            e1.record()
            o._phase_events.append((self.name, self.e0, e1))
        else:
            o.phase_times[self.name] += (time.perf_counter() - self.t0) * 1e3
        return False


class DistributedMultigrid:
    """V/W/F-cycle on a px x py block decomposition.

    ranks:  the rank ids this PROCESS computes (one under torch.distributed; all of them for the
            in-process virtual-rank mode used by the single-GPU test).
    ops:    kernel provider (HipOps, or the tests' NumPy stand-in).
    dist:   torch.distributed module (initialised) or None for the in-process mode.
    mode:   "fused" (ghost zone of 7 cells for weighted Jacobi, 13 for red-black GS; two fused launches and ~one
            exchange per level; pre, post <= 2) or "per_operator" (1-cell ghost ring, one launch and one exchange per
            operator; any sweep count).  "auto" picks "fused" whenever it applies.
    """

    def __init__(self, NX, NY, px, py, ranks, ops, dist=None, domain=(0.0, 1.0, 0.0, 1.0), coeff=-1.0,
                 max_levels=None, cycle="V", pre=2, post=2, smoother="jacobi", omega=0.8, coarse_tol=1e-12,
                 coarse_maxit=1000, agglomerate_at=1025, mode="auto", overlap=True, native="auto", span="auto"):
        """span: run the level-0 up leg of cycle k and the down leg of cycle k + 1 as ONE launch (ops.span_leg) whenever the
        next cycle's front part is queued ahead of the norm anyway (`speculate`): "auto" with native plans (MG_DIST_SPAN=0
        turns it off), True also in the eager driver (tests), False never.  Weighted Jacobi, constant coefficients, level 0
        and level 1 in one dtype, blocks the kernel serves (ops.span_ok); same iterates bit for bit.
        native: replay the cycle from a recorded plan (dist_plan.py; one C call per cycle).  "auto": whenever the
        kernels are the device ones, the mode is "fused" and the ranks talk over RCCL (or live in this process).
        Precision: every level in ops.np_dtype, or -- with an `ops` built for per-level mixed precision (ops.mixed:
        PrecisionManager('mixed'), core/precision.py:337-357) -- level l >= L // 2 in fp32 and the rest, like the
        coarsest level, in fp64, decomposed and replicated levels alike."""
        from .facade import default_max_levels
        self.NX, self.NY, self.px, self.py = NX, NY, px, py
        self.ops, self.dist = ops, dist
        self.torch = ops.torch
        self.domain, self.coeff = domain, coeff
        self.cycle_type, self.pre, self.post = cycle, pre, post
        if smoother in ("line", "line_x", "line_y", "line_alternating", "zebra_x", "zebra_y", "zebra_alt"):
            raise NotImplementedError("the decomposed (multi-GPU) solver has no line smoothers: a line would cross "
                                      "sub-domains")                  # before any device work
        if smoother not in ("jacobi", "rbgs"):
            raise ValueError(f"Unknown smoother: {smoother}")
        if mode not in ("auto", "fused", "per_operator"):
            raise ValueError(f"Unknown mode: {mode}")
        can_fuse = pre <= 2 and post <= 2 and hasattr(ops, "down_leg")
        if mode == "fused" and not can_fuse:
            raise ValueError("mode 'fused' needs pre, post <= 2")
        self.mode = "fused" if (mode in ("auto", "fused") and can_fuse) else "per_operator"
        self.G = GHOST_FUSED[smoother] if self.mode == "fused" else 1
        self.smoother, self.omega = smoother, omega
        self.smk = _lib.MG_JACOBI if smoother == "jacobi" else _lib.MG_RBGS
        self.shapes = hierarchy_shapes(NX, NY, max_levels or default_max_levels(NX, NY))
        self.L = len(self.shapes)
        self.Ld = distributed_levels(self.shapes, px, py, agglomerate_at, self.G) if px * py > 1 else 0
        self.h = [((domain[1] - domain[0]) / (a - 1), (domain[3] - domain[2]) / (b - 1)) for a, b in self.shapes]
        # precision of every level (see the docstring); the coarsest level is never converted (solvers/multigrid.py:270-272)
        self.mixed = bool(getattr(ops, "mixed", False))
        self.split = self.L // 2
        self.ldt = [np.dtype(np.float32) if (self.mixed and l >= self.split and l != self.L - 1) else
                    (np.dtype(np.float64) if self.mixed else np.dtype(ops.np_dtype)) for l in range(self.L)]
        self.var = False                        # variable-coefficient operator (set_coefficient)
        self.ranks = list(ranks)
        self.doms = {}
        self.exchanges = 0                      # halo exchanges issued (statistics)
        for r in self.ranks:
            rx, ry = divmod(r, py)
            d = _Dom()
            d.rank, d.rx, d.ry = r, rx, ry
            d.blk = [Block(a, b, px, py, rx, ry, self.G) for (a, b) in self.shapes[:self.Ld + 1]]
            d.u, d.t, d.rhs, d.r, d.a, d.rd = [], [], [], [], [], []
            d.s = [None] * self.Ld                 # level 0 only: third buffer of the spanning leg, allocated on first use
            for l in range(self.Ld):
                b = d.blk[l]
                d.u.append(ops.alloc(b.lnx, b.lny, self.ldt[l]))
                d.t.append(ops.alloc(b.lnx, b.lny, self.ldt[l]) if (smoother == "jacobi" or self.mode == "fused") else None)
                d.rhs.append(ops.alloc(b.lnx, b.lny, self.ldt[l]))
                d.r.append(ops.alloc(b.lnx, b.lny, self.ldt[l]) if self.mode == "per_operator" else None)
                d.a.append(None)
                d.rd.append(None)
            # the agglomeration level: a local coarse buffer (restriction target / prolongation source)
            if self.Ld > 0:
                b = d.blk[self.Ld]
                d.rc = ops.alloc(b.lnx, b.lny, self.ldt[self.Ld])   # restricted rhs (its boundary ring is written once per rhs in fused mode)
                d.ec = ops.alloc(b.lnx, b.lny, self.ldt[self.Ld])   # this rank's piece of the replicated correction
                d.zc = None                                          # zero correction for the level-1 block (variable-coefficient norm)
            d.ring_sumsq = None
            self.doms[r] = d
        NXa, NYa = self.shapes[self.Ld]
        self.rhs_a = ops.alloc(NXa, NYa, self.ldt[self.Ld])
        self.e_a = ops.alloc(NXa, NYa, self.ldt[self.Ld])
        ops.coarse_setup(NXa, NYa, domain, dict(coeff=coeff, levels=self.L - self.Ld, cycle=cycle, pre=pre, post=post,
                                                smoother=self.smk, omega=omega, coarse_tol=coarse_tol, coarse_maxit=coarse_maxit,
                                                mixed_split=self.split - self.Ld))
        # gather buffers: exclusive blocks padded to the largest block
        if self.Ld > 0:
            blocks = [Block(NXa, NYa, px, py, rx, ry, self.G) for rx in range(px) for ry in range(py)]
            self.gmx = max(b.i_hi - b.i_lo for b in blocks)
            self.gmy = max(b.j_hi - b.j_lo for b in blocks)
        self._last_norm_parts = None
        self._stage_p2p = None                   # decided at the first exchange (see _p2p)
        # exchange / compute overlap on a second stream (device kernels only)
        self.overlap = bool(overlap) and self.mode == "fused" and getattr(ops, "supports_overlap", False)
        if self.overlap:
            torch = self.torch
            from . import dist_plan
            # ONE communication stream per process and device: the solvers of a process share the RCCL communicator, and every
            # RCCL call on a communicator must reach it from one stream (dist_plan.shared_comm_stream)
            self._comm_stream = dist_plan.shared_comm_stream(getattr(ops, "device", torch.device("cuda", torch.cuda.current_device())))
            self._ev_a, self._ev_b = torch.cuda.Event(), torch.cuda.Event()
            self._ev_c, self._ev_d = torch.cuda.Event(), torch.cuda.Event()      # spanning mode: the level-0 exchange beside the lower levels
        # native replay of the cycle (dist_plan.py)
        plan_ok = (self.mode == "fused" and getattr(ops, "plan_capable", False) and self.Ld > 0 and
                   (dist is None or dist.get_backend() == "nccl"))
        if native not in ("auto", True, False):
            raise ValueError(f"Unknown native setting: {native}")
        if native is True and not plan_ok:
            raise ValueError("native cycle plans need the device kernels, mode 'fused' and RCCL (or in-process ranks)")
        self.native = plan_ok if native == "auto" else bool(native)
        self.native_required = native is True
        if span not in ("auto", True, False):
            raise ValueError(f"Unknown span setting: {span}")
        self.span = (self.native and os.environ.get("MG_DIST_SPAN", "1") != "0") if span == "auto" else bool(span)
        self._pre = None                         # spanning mode: the level-0 buffer ("t" / "s") holding the queued front part's pre-smoothed iterate
        self._sp_plans = {}                      # ... its recorded plans: ("mid", src) -> (legs + norm, lower levels), ("back", src) -> plan
        self._norm_plan = None                   # the plan whose RESULT (sum of r^2) is in flight
        self._plan_x = {}                        # plan -> halo exchanges it issues (statistics; the plain scheme's are all in its front part)
        self._plan_kind = None                   # which scheme self._plan belongs to: "plain" (front | back) or "span"
        self._plan_failure = None                # why a part recorded in this cycle has no plan (_record_part -> _plans_agreed)
        self.native_failure = None               # why "auto" fell back to the Python driver, if it did
        self._rec = None                         # PlanRecorder while the first cycle is being recorded
        self._plan = None
        self._plan_state = None
        self._comm = None
        self._bufs = {}                          # persistent staging buffers (pack / unpack / gather)
        self._norm_value = None                  # sum of r^2 the last native cycle returned
        self._plan_back = None                   # the plan is kept as two: front (level-0 down legs and below) / back (up legs, norm)
        self._front_queued = False               # the front part of the COMING cycle is already on the streams
        self._norm_pending = False               # the back part's sum of r^2 is still on its way to the host
        self.speculate = True                    # queue the next cycle's front part before waiting for the norm
        self.native_cycles = 0
        # per-phase times of the cycle (diagnostics, profile_phases / collect_phase_times)
        self.phase_times = None
        self._phase_events = []

    # ---- per-phase times (diagnostics) -----------------------------------------------------------
    def profile_phases(self, enable=True):
        """Bracket the phases of the coming cycles -- fused legs, halo copies, send/recv groups (incl. the wait for the
        peers), the coarse all-gather, the replicated engine, the norm all-reduce -- with timers: timing events on the stream a
        phase runs on for device tensors (inside the C++ plan executor when cycles are replayed natively), wall clock for the
        CPU stand-in.  For diagnostic cycles outside a timed region; collect_phase_times() returns milliseconds per phase."""
        self.phase_times = {n: 0.0 for n in _lib.PLAN_PHASE_NAMES} if enable else None
        self._phase_events = []
        for pl in self._all_plans():
            pl.profile(enable)

    def collect_phase_times(self):
        if self.phase_times is None:
            return {}
        if self._phase_events:
            self.torch.cuda.synchronize()
            for name, e0, e1 in self._phase_events:
                self.phase_times[name] += e0.elapsed_time(e1)
            self._phase_events = []
        for pl in self._all_plans():
            pl.phase_times(self.phase_times)
        out = dict(self.phase_times)
        for k in self.phase_times:
            self.phase_times[k] = 0.0
        return out

    def _ph(self, name):
        return _Phase(self, name)

    # ---- primitives the plan recorder sees ------------------------------------------------------
    def _copy(self, dst, src):
        dst.copy_(src)
        if self._rec is not None:
            self._rec.copy2d(dst, src)

    def _buf(self, key, shape, dtype, device, zero=False):
        """staging buffer that lives as long as the solver (a recorded plan holds its pointer)"""
        t = self._bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = (self.torch.zeros if zero else self.torch.empty)(tuple(shape), dtype=dtype, device=device)
            self._bufs[key] = t
        return t

    def _add(self, a, b):
        out = a + b
        if self._rec is not None:
            self._rec.add(out, a, b)
        return out

    # ---- neighbours ----------------------------------------------------------------------
    def _nbr(self, d, dx, dy):
        rx, ry = d.rx + dx, d.ry + dy
        if 0 <= rx < self.px and 0 <= ry < self.py:
            return rx * self.py + ry
        return None

    def _p2p(self, sends, recvs):
        """sends/recvs: lists of (peer_rank, tensor): batched isend/irecv (RCCL send/recv, one group per phase)."""
        if self.dist is None or not (sends or recvs):
            return
        if self._rec is not None:
            self._rec.group(sends, recvs)
        if self._stage_p2p is None:
            # gloo moves device tensors with host-side memcpy on their raw pointers, unordered against the HIP streams
            # that produce / consume them (rehearsals on a one-GPU box): stage through host tensors, synchronously.
            # nccl (= RCCL) send/recv are enqueued on the current stream and need nothing of the kind.
            self._stage_p2p = (self.dist.get_backend() == "gloo") and any(t.is_cuda for _, t in sends + recvs)
        if self._stage_p2p:
            self.torch.cuda.current_stream().synchronize()
            hs = [(p, t.cpu()) for p, t in sends]
            hr = [(p, self.torch.empty(t.shape, dtype=t.dtype), t) for p, t in recvs]
            ops = [self.dist.P2POp(self.dist.isend, t, p) for p, t in hs] + \
                  [self.dist.P2POp(self.dist.irecv, h, p) for p, h, _ in hr]
            for req in self.dist.batch_isend_irecv(ops):
                req.wait()
            for _, h, t in hr:
                t.copy_(h)
            return
        ops = [self.dist.P2POp(self.dist.isend, t, p) for p, t in sends] + \
              [self.dist.P2POp(self.dist.irecv, t, p) for p, t in recvs]
        for req in self.dist.batch_isend_irecv(ops):
            req.wait()

    def exchange(self, name, l, corners=False):
        """Fill the ghost zone (G cells wide) of field `name` on level l from the neighbours' owned cells next to the cut,
        in ONE communication step: whole rows to the row neighbours (contiguous memory, no packing), packed columns over
        the full local height to the column neighbours, packed G x G corners to the diagonal neighbours.  Rows and columns
        carry stale data where they cross the receiver's corner regions; the corner blocks are unpacked last."""
        G = self.G
        self.exchanges += 1
        fields = {r: (getattr(d, name)[l] if isinstance(getattr(d, name), list) else getattr(d, name)) for r, d in self.doms.items()}

        def rows_of(b, dx, ghost):       # the G rows next to the cut towards dx: the ghost rows, or the owned rows beside them
            if ghost:
                return slice(b.oi_lo - G, b.oi_lo) if dx < 0 else slice(b.oi_hi + 1, b.oi_hi + 1 + G)
            return slice(b.oi_lo, b.oi_lo + G) if dx < 0 else slice(b.oi_hi - G + 1, b.oi_hi + 1)

        def cols_of(b, dy, ghost):
            if ghost:
                return slice(b.oj_lo - G, b.oj_lo) if dy < 0 else slice(b.oj_hi + 1, b.oj_hi + 1 + G)
            return slice(b.oj_lo, b.oj_lo + G) if dy < 0 else slice(b.oj_hi - G + 1, b.oj_hi + 1)

        sends, recvs = [], []
        # in-process neighbours: copies, grouped so that runs of them do not touch each other (the plan executor launches such
        # a run as one kernel): all rows, all columns, then the corners (they overwrite what rows and columns left there)
        local = {"row": [], "col": [], "corner": []}
        unpack = {"col": [], "corner": []}
        for r, d in self.doms.items():
            b, t = d.blk[l], fields[r]
            for dx in (-1, 0, +1):
                for dy in (-1, 0, +1):
                    if dx == 0 and dy == 0:
                        continue
                    p = self._nbr(d, dx, dy)
                    if p is None:
                        continue
                    pb = self.doms[p].blk[l] if p in self.doms else None
                    if dy == 0:                                   # row neighbour
                        if pb is not None:
                            local["row"].append((t[rows_of(b, dx, True), :b.lny], fields[p][rows_of(pb, -dx, False), :pb.lny]))
                        else:
                            sends.append((p, t[rows_of(b, dx, False)]))      # whole padded rows: one contiguous chunk
                            recvs.append((p, t[rows_of(b, dx, True)]))
                    elif dx == 0:                                 # column neighbour
                        if pb is not None:
                            local["col"].append((t[:b.lnx, cols_of(b, dy, True)], fields[p][:pb.lnx, cols_of(pb, -dy, False)]))
                        else:
                            sbuf = self._buf(("pack", name, l, r, dy), (b.lnx, G), t.dtype, t.device)
                            rbuf = self._buf(("unpack", name, l, r, dy), (b.lnx, G), t.dtype, t.device)
                            self._copy(sbuf, t[:b.lnx, cols_of(b, dy, False)])
                            sends.append((p, sbuf))
                            recvs.append((p, rbuf))
                            unpack["col"].append((t[:b.lnx, cols_of(b, dy, True)], rbuf))
                    else:                                         # diagonal neighbour: the G x G corner
                        dst = t[rows_of(b, dx, True), cols_of(b, dy, True)]
                        if pb is not None:
                            local["corner"].append((dst, fields[p][rows_of(pb, -dx, False), cols_of(pb, -dy, False)]))
                        else:
                            sbuf = self._buf(("cpack", name, l, r, dx, dy), (G, G), t.dtype, t.device)
                            rbuf = self._buf(("cunpack", name, l, r, dx, dy), (G, G), t.dtype, t.device)
                            self._copy(sbuf, t[rows_of(b, dx, False), cols_of(b, dy, False)])
                            sends.append((p, sbuf))
                            recvs.append((p, rbuf))
                            unpack["corner"].append((dst, rbuf))
        with self._ph("halo_copy"):
            for dst, src in local["row"] + local["col"]:
                self._copy(dst, src)
        with self._ph("halo_exchange"):
            self._p2p(sends, recvs)
        with self._ph("halo_copy"):
            for dst, src in unpack["col"] + local["corner"] + unpack["corner"]:
                self._copy(dst, src)

    def allreduce_sum(self, parts):
        """parts: {rank: 1-element fp64 tensor}.  Returns the global sum as a Python float."""
        total = None
        with self._ph("allreduce"):
            for r in self.ranks:
                total = parts[r] if total is None else self._add(total, parts[r])
            if self.dist is not None:
                self.dist.all_reduce(total)
                if self._rec is not None:
                    self._rec.allreduce(total)
        if self._rec is not None:
            self._rec.result(total)
        return float(total.item())

    # ---- agglomeration -----------------------------------------------------------------------
    def _gather_coarse_rhs(self):
        """All ranks end up with the whole coarse right-hand side (exclusive blocks tile the grid)."""
        torch = self.torch
        La = self.Ld
        NXa, NYa = self.shapes[La]
        if self.dist is None:
            for r, d in self.doms.items():
                b = d.blk[La]
                self._copy(self.rhs_a[b.gx0 + b.i_lo:b.gx0 + b.i_hi, b.gy0 + b.j_lo:b.gy0 + b.j_hi], d.rc[b.i_lo:b.i_hi, b.j_lo:b.j_hi])
            return
        (r, d), = self.doms.items()
        b = d.blk[La]
        P = self.px * self.py
        mine = self._buf(("gather", "mine"), (self.gmx, self.gmy), d.rc.dtype, d.rc.device, zero=True)   # the padding stays zero
        every = self._buf(("gather", "all"), (P, self.gmx, self.gmy), d.rc.dtype, d.rc.device)
        self._copy(mine[:b.i_hi - b.i_lo, :b.j_hi - b.j_lo], d.rc[b.i_lo:b.i_hi, b.j_lo:b.j_hi])
        self.dist.all_gather(list(every.unbind(0)), mine)
        if self._rec is not None:
            self._rec.allgather(mine, every)
        for q in range(P):
            qb = Block(NXa, NYa, self.px, self.py, *divmod(q, self.py), self.G)
            self._copy(self.rhs_a[qb.gx0 + qb.i_lo:qb.gx0 + qb.i_hi, qb.gy0 + qb.j_lo:qb.gy0 + qb.j_hi],
                       every[q, :qb.i_hi - qb.i_lo, :qb.j_hi - qb.j_lo])

    def _replicated_cycle(self, l):
        """Coarse tail: gather the coarse rhs, run the remaining levels on the single-GPU engine (on every GPU),
        take this rank's piece of the correction (ghost zone included: it is global data)."""
        with self._ph("coarse_allgather"):
            self._gather_coarse_rhs()
        with self._ph("replicated_engine"):
            if self.mode == "fused" and getattr(self.ops, "plan_capable", False):
                self.ops.coarse_begin(self.rhs_a, same_ring=True)      # the ring went in with set_problem
            else:
                self.ops.coarse_begin(self.rhs_a)
            for _ in range(self._reps(l)):
                self.ops.coarse_cycle()
            self.ops.coarse_end(self.e_a)
        with self._ph("halo_copy"):
            for d in self.doms.values():
                bc = d.blk[l + 1]
                self._copy(d.ec[:bc.lnx, :bc.lny], self.e_a[bc.gx0:bc.gx0 + bc.lnx, bc.gy0:bc.gy0 + bc.lny])

    # ---- the cycle (solvers/multigrid.py:253-337) ------------------------------------------------
    def _reps(self, l):
        if self.cycle_type == "V":
            return 1
        if self.cycle_type == "W":
            return 2
        return max(1, 2 ** (self.L - l - 2))

    def smooth(self, l, nu):
        hx, hy = self.h[l]
        for _ in range(nu):
            if self.smoother == "jacobi":
                for d in self.doms.values():
                    b = d.blk[l]
                    self.ops.jacobi(d.u[l], d.rhs[l], d.t[l], b.lnx, b.lny, hx, hy, self.omega)
                    d.u[l], d.t[l] = d.t[l], d.u[l]
                self.exchange("u", l)
            else:
                for colour in (0, 1):
                    for d in self.doms.values():
                        b = d.blk[l]
                        self.ops.rbgs_colour(d.u[l], d.rhs[l], b.lnx, b.lny, hx, hy, self.omega, colour,
                                             (b.gx0 + b.gy0) & 1)
                    self.exchange("u", l)

    def cycle(self, l=0, zero_u=False):
        if self.Ld == 0:                      # nothing distributed: the replicated engine is the whole solver
            raise RuntimeError("single-block problems go through MultigridEngine")
        self._last_norm_parts = None
        self._norm_value = None
        spanning = l == 0 and not zero_u and self._span_usable()
        if self.native and l == 0 and not zero_u:
            return self._cycle_native_span() if spanning else self._cycle_native()
        if spanning:
            if self._norm_pending or self._front_queued:      # native cycles came before: start from their iterate
                self._settle()
            return self._cycle_span_eager()
        # an eager cycle after native ones: collect a norm still in flight and forget a queued front part -- it was computed
        # from the iterate this cycle is about to replace
        self._settle()
        if self.mode == "fused":
            return self._cycle_fused(l, zero_u)
        return self._cycle_per_operator(l)

    # ---- native replay (dist_plan.py) --------------------------------------------------------------
    def _pointer_state(self):
        return tuple((d.u[l].data_ptr(), d.t[l].data_ptr(), d.rhs[l].data_ptr(), 0 if d.a[l] is None else d.a[l].data_ptr(),
                      0 if d.rd[l] is None else d.rd[l].data_ptr(), 0 if d.s[l] is None else d.s[l].data_ptr())
                     for d in self.doms.values() for l in range(self.Ld)) + \
            tuple(0 if d.ring_sumsq is None else d.ring_sumsq.data_ptr() for d in self.doms.values()) + (self.var,)

    def _all_plans(self):
        out = [q for q in (self._plan, self._plan_back) if q is not None]
        for pair in self._sp_plans.values():
            out.extend(q for q in pair if q is not None)
        return out

    def _drop_plan(self):
        plans = self._all_plans()
        if plans:
            self.torch.cuda.synchronize()
            for q in plans:
                q.close()
        self._plan = self._plan_back = self._norm_plan = None
        self._sp_plans = {}
        self._plan_x = {}
        self._plan_state = None
        self._front_queued = self._norm_pending = False
        self._pre = None

    def _settle(self):
        """Before the iterate is replaced (new problem / coefficient / iterate): collect a norm still in flight and forget a
        front part queued for a cycle that will not come."""
        if self._norm_pending:
            self._norm_value = (self._norm_plan or self._plan_back).wait()
            self._norm_pending = False
        self._front_queued = False
        self._pre = None                         # spanning mode: u holds the iterate, whatever t / s were being prepared for

    def _record_part(self, fn, split=False):
        """run `fn` through the Python driver with a recorder attached -> CyclePlan, or with `split` the pair (front, back) cut
        at the recorder's mark_split; None, and self._plan_failure, if the replay cannot be built"""
        from . import dist_plan
        device = next(iter(self.doms.values())).u[0].device
        before = self.exchanges
        rec = self._rec = self.ops.rec = dist_plan.PlanRecorder()
        try:
            fn()
        finally:
            self._rec = self.ops.rec = None
        cut = rec.split if rec.split is not None else len(rec.ops)
        plans = []
        try:
            if self.dist is not None and self._comm is None:
                self._comm = dist_plan.shared_comm(self.dist, device.index or 0)
            for lo, hi in (((0, cut), (cut, None)) if split else ((0, None),)):
                plans.append(dist_plan.CyclePlan(rec, self._comm, device.index or 0, lo, hi))
        except Exception as exc:                 # the work is done; only the replay is missing (all ranks agree on it in _plans_agreed)
            for q in plans:
                q.close()
            self._plan_failure = exc
            return None
        for k, q in enumerate(plans):            # a back part -- up legs and the norm -- exchanges nothing
            self._plan_x[q] = 0 if k else self.exchanges - before
            if self.phase_times is not None:
                q.profile(True)
        return tuple(plans) if split else plans[0]

    def _plans_agreed(self):
        """After a cycle that recorded: a rank that could not build a plan takes every rank back to the Python driver -- agreed on
        through torch.distributed (every rank records in the same cycle), so nobody replays alone.  -> every rank holds its
        plans; otherwise raises (native=True) or drops the plans -- and with them a queued front part: the eager driver starts
        from the iterate in u -- and leaves the reason in native_failure."""
        failure, self._plan_failure = self._plan_failure, None
        if self.dist is not None:
            device = next(iter(self.doms.values())).u[0].device
            flag = self.torch.tensor([0 if failure is None else 1], dtype=self.torch.int32, device=device)
            self.dist.all_reduce(flag, op=self.dist.ReduceOp.MAX)
            if int(flag.item()) and failure is None:
                failure = RuntimeError("another rank could not build its cycle plan")
        if failure is None:
            return True
        if self.native_required:
            raise failure
        self._drop_plan()
        self.native = False
        self.native_failure = repr(failure)
        return False

    def _plan_streams(self):
        """(compute, communication) stream handles a plan is enqueued on"""
        compute = self.torch.cuda.current_stream().cuda_stream
        return compute, (self._comm_stream.cuda_stream if self.overlap else compute)

    def _run_plan(self, plan):
        plan.run_async(*self._plan_streams())
        self.exchanges += self._plan_x[plan]

    def _cycle_native_span(self):
        """The spanning scheme with recorded plans: front F (u -> t, lower levels), and per source buffer a mid pair (spanning
        legs + norm | exchange + lower levels) and a back plan (up legs + norm).  Each is recorded from the Python driver the
        first time its turn comes (that cycle runs eagerly) and replayed afterwards; the norm travels behind the legs' plan."""
        if self._plan is not None and self._plan_kind != "span":      # plans of the two-launch scheme
            self._settle()
            self._drop_plan()
        self._ensure_third()
        state = self._pointer_state()
        if (self._plan is not None or self._sp_plans) and self._plan_state != state:
            self._settle()
            self._drop_plan()
        if self._norm_pending:                   # nobody asked for the previous cycle's norm
            (self._norm_plan or self._plan_back).wait()
            self._norm_pending = False
        replayed = True
        if self._pre is None:
            if self._plan is None:
                self._plan = self._record_part(lambda: (self._sp_front("t"), self._sp_lower("t")))
                self._plan_state, self._plan_kind = state, "span"
                replayed = False
            else:
                self._run_plan(self._plan)
            self._pre = "t"
        src = self._pre
        dst = ("s" if src == "t" else "t") if self.speculate else None
        key = ("mid" if dst else "back", src)
        plans = self._sp_plans.get(key)
        if plans is None:
            def legs():
                self._sp_legs(src, dst)
                self._norm_value = self.allreduce_sum(self._last_norm_parts)
            first = self._record_part(legs)
            self._last_norm_parts = None
            second = self._record_part(lambda: self._sp_lower(dst)) if dst else None
            self._sp_plans[key] = (first, second)
            replayed = False
        else:
            for q in plans:
                if q is not None:
                    self._run_plan(q)
            self._norm_plan, self._norm_pending = plans[0], True
        self._pre = dst
        if not replayed and not self._plans_agreed():
            return
        self._front_queued = self._pre is not None
        if replayed:
            self.native_cycles += 1

    def _cycle_native(self):
        """The first cycle (and the first after anything moved a field to another buffer) runs through the Python driver
        with a recorder attached; every other one is a single mg_plan_run.  Either way the sum of r^2 over the grid comes
        back with the cycle (the eager path computes it lazily in residual_norm())."""
        state = self._pointer_state()
        if self._plan is not None and (self._plan_state != state or self._plan_kind == "span"):
            self._settle()
            self._drop_plan()
        self._plan_kind = "plain"
        if self._plan is None:
            def whole():
                self._cycle_fused(0, False)
                self._norm_value = self.allreduce_sum(self._last_norm_parts)
                if self._pointer_state() != state:
                    raise RuntimeError("a cycle must leave every field in the buffer it started in")
            self._plan, self._plan_back = self._record_part(whole, split=True) or (None, None)      # front | back part
            self._last_norm_parts = None
            self._plan_state = state
            self._plans_agreed()
            return
        if self._norm_pending:                   # nobody asked for the previous cycle's norm
            self._plan_back.wait()
            self._norm_pending = False
        compute, comm = self._plan_streams()
        if not self._front_queued:
            self._plan.run_async(compute, comm)
        self._plan_back.run_async(compute, comm)
        self._norm_pending = True
        # the front part of the NEXT cycle goes onto the streams before anybody waits for this cycle's norm: it reads the
        # iterate this cycle leaves and writes only the other buffers, so a solve that ends here just leaves it unused
        self._front_queued = bool(self.speculate)
        if self._front_queued:
            self._plan.run_async(compute, comm)
        self.native_cycles += 1
        self.exchanges += self._plan_x[self._plan]          # per cycle, whenever its front part was queued

    def _leg(self, d, l):
        """What block `d`'s legs on level l are launched with: the block and its coarse block, the coarse offsets, the correction
        source `e` and the restriction `target` (the agglomeration buffers below the last distributed level), the colour of
        local (0, 0), the norm window (owned cells inside the local array), the variable-coefficient keywords."""
        b, bc = d.blk[l], d.blk[l + 1]
        ci, cj = b.coarse_offsets(bc)
        last = (l + 1 == self.Ld)
        return _Leg(b, bc, ci, cj, d.ec if last else d.u[l + 1], d.rc if last else d.rhs[l + 1], (b.gx0 + b.gy0) & 1,
                    (max(b.i_lo, 1), min(b.i_hi, b.lnx - 1), max(b.j_lo, 1), min(b.j_hi, b.lny - 1)),
                    {"acoef": d.a[l], "rdiag": d.rd[l]} if self.var else {})

    def _up_leg(self, d, l, src, out, norm, e=None, nsweep=None):
        """The up leg of block `d` on level l: out = sweeps(src + P e), e the correction from below and `post` sweeps unless
        given; `norm`: also the sum of r^2 over the owned cells (device tensor)."""
        g = self._leg(d, l)
        b, bc = g.b, g.bc
        return self.ops.up_leg(self.smk, src, d.rhs[l], out, g.e if e is None else e, b.lnx, b.lny, bc.lnx, bc.lny, g.ci, g.cj, b.sides,
                               self.h[l][0], self.h[l][1], self.omega, self.coeff, self.post if nsweep is None else nsweep, g.poff,
                               g.win if norm else None, **g.kw)

    def level0_up_leg(self, rank):
        """-> (block, launch): launch() runs the level-0 up leg of `rank`'s block once, u -> t with the norm; the iterate stays
        in u.  The dominant kernel of a cycle on its own, for timing (dist_bench's roofline leg)."""
        self._settle()
        d = self.doms[rank]
        return d.blk[0], lambda: self._up_leg(d, 0, d.u[0], d.t[0], True)

    @contextlib.contextmanager
    def _beside(self, k, fork, done):
        """`with self._beside(k, fork, done):` the enclosed work runs on the communication stream, after what the compute stream
        holds so far (torch event `fork`, plan event k) and beside what it is given next; `done` (plan event k + 1) marks its
        end, for _join."""
        torch, rec = self.torch, self._rec
        fork.record(torch.cuda.current_stream())
        if rec is not None:
            rec.event_record(k)
            rec.stream = 1
            rec.stream_wait(k)
        with torch.cuda.stream(self._comm_stream):
            self._comm_stream.wait_event(fork)
            yield
            done.record(self._comm_stream)
        if rec is not None:
            rec.event_record(k + 1)
            rec.stream = 0

    def _join(self, k, done):
        """the compute stream waits for the side branch that ended with `done` (plan event k)"""
        self.torch.cuda.current_stream().wait_event(done)
        if self._rec is not None:
            self._rec.stream_wait(k)

    def _down_legs(self, l, zero_u, pending, out=None):
        """The down legs of level l on every local block: u -> `out` (rank -> array; default the ping-pong partner t), the
        restricted residual -> the level below.  `pending`: fields of this level whose ghost zones the legs wait for; with
        overlap the exchange runs on the communication stream beside the tiles that read no ghost data."""
        hx, hy = self.h[l]
        big = 1 << 30

        def down(select):
            for r, d in self.doms.items():
                g = self._leg(d, l)
                b, bc = g.b, g.bc
                # select 1 / 2: tiles inside / outside the cells whose values do not come out of an exchange (owned cells and
                # physical boundary)
                inner = (-big if b.sides & SIDE_ILO else b.oi_lo, big if b.sides & SIDE_IHI else b.oi_hi + 1,
                         -big if b.sides & SIDE_JLO else b.oj_lo, big if b.sides & SIDE_JHI else b.oj_hi + 1) if select else None
                with self._ph("legs"):
                    self.ops.down_leg(self.smk, d.u[l], d.rhs[l], d.t[l] if out is None else out[r], g.target, b.lnx, b.lny, bc.lnx, bc.lny,
                                      g.ci, g.cj, hx, hy, self.omega, self.coeff, self.pre, zero_u, g.poff, select, inner, **g.kw)

        if pending and self.overlap:
            # tiles that read no ghost data run on the compute stream while the exchange runs on the comm stream
            with self._beside(0, self._ev_a, self._ev_b):
                for name in pending:
                    self.exchange(name, l)
            down(1)
            self._join(1, self._ev_b)
            down(2)
        else:
            for name in pending:
                self.exchange(name, l)
            down(0)

    # ---- level 0 with a spanning leg ------------------------------------------------------------------------------------
    # Three level-0 arrays per block: u ALWAYS holds the iterate of the last completed cycle; t and s take turns holding the
    # pre-smoothed iterate of the cycle in flight (self._pre names the one that does).  front: u -> t (down legs);
    # mid: src -> u (iterate of this cycle) and -> the other one (pre-smoothed iterate of the next), one launch; back: src -> u
    # (up legs).  Every part ends with the level-0 ghost zones of what it just wrote on their way (beside the lower levels), so
    # that the part that follows -- mid or back -- reads m = 7 exact ghost cells: post sweeps leave 4, the norm reads owned
    # cells, pre sweeps leave 2, residual 1, full weighting of the owned coarse cells needs 1.
    def _f0(self, d, name):
        return d.u[0] if name == "u" else (d.t[0] if name == "t" else d.s[0])

    def _span_usable(self):
        if not (self.span and self.mode == "fused" and self.smoother == "jacobi" and not self.var and self.Ld >= 1 and
                1 <= self.pre <= 2 and 1 <= self.post <= 2 and hasattr(self.ops, "span_leg") and self.ldt[0] == self.ldt[1]):
            return False
        for d in self.doms.values():
            b = d.blk[0]
            if not self.ops.span_ok(self.smk, d.u[0], d.ec if self.Ld == 1 else d.u[1], b.lnx, b.lny):
                return False
        return True

    def _ensure_third(self):
        for d in self.doms.values():
            if d.s[0] is None:
                b = d.blk[0]
                d.s[0] = self.ops.alloc(b.lnx, b.lny, self.ldt[0])
                d.s[0].copy_(d.u[0])               # the outermost ring (Dirichlet values on physical edges) is never written by a leg

    def _sp_front(self, dst):
        self._down_legs(0, False, ["u"], out={r: self._f0(d, dst) for r, d in self.doms.items()})

    def _sp_lower(self, xname):
        """everything below level 0 of one cycle, the halo exchange of the level-0 array `xname` beside it"""
        if self.overlap:
            with self._beside(2, self._ev_c, self._ev_d):
                self.exchange(xname, 0)
        else:
            self.exchange(xname, 0)
        if self.Ld == 1:
            self._replicated_cycle(0)
        else:
            for k in range(self._reps(0)):
                self._cycle_fused(1, k == 0, k == 0)
        if self.overlap:
            self._join(3, self._ev_d)

    def _sp_legs(self, src, dst):
        """dst None: the up legs src -> u (back part); else the spanning legs src -> u and dst (mid part).  Sets the norm parts."""
        hx, hy = self.h[0]
        parts = {}
        for r, d in self.doms.items():
            with self._ph("legs"):
                if dst is None:
                    res = self._up_leg(d, 0, self._f0(d, src), d.u[0], True)
                else:
                    g = self._leg(d, 0)
                    b, bc = g.b, g.bc
                    res = self.ops.span_leg(self.smk, self._f0(d, src), d.rhs[0], d.u[0], self._f0(d, dst), g.e, g.target,
                                            b.lnx, b.lny, bc.lnx, bc.lny, g.ci, g.cj, b.sides, hx, hy, self.omega, self.coeff, self.post,
                                            self.pre, g.poff, g.win)
            parts[r] = self._add(res, d.ring_sumsq)
        self._last_norm_parts = parts

    def _cycle_span_eager(self):
        """one cycle of the spanning scheme through the Python driver (the order of operations the plans replay)"""
        self._ensure_third()
        if self._pre is None:
            self._sp_front("t")
            self._sp_lower("t")
            self._pre = "t"
        if self.speculate:                           # the next cycle's front part goes out with this cycle's back part
            dst = "s" if self._pre == "t" else "t"
            self._sp_legs(self._pre, dst)
            parts = self._last_norm_parts
            self._sp_lower(dst)
            self._last_norm_parts = parts
            self._pre = dst
        else:
            self._sp_legs(self._pre, None)
            self._pre = None

    def _cycle_fused(self, l, zero_u, first_visit_rhs=False):
        """Two launches and (at most) two exchanges per level.  Validity bookkeeping (m = cells of the ghost zone that
        are exact, counted from the owned cells outwards; G = 7): after an exchange m = 7; the down leg's two sweeps
        leave the iterate exact on m = 5, its restriction is exact on all owned coarse cells; the correction that
        comes back from below is exact on m_c >= 3 coarse cells = 6 fine cells, so after the up leg (prolongation,
        two sweeps) m = min(5, 6) - 2 = 3 >= 0, and the norm (one more cell) only reads exact values."""
        last = (l + 1 == self.Ld)
        # What this level's down leg is waiting for: the iterate's ghost zone (level 0 every cycle; coarser levels only
        # when re-visited by a W / F cycle) and, below level 0, the ghost zone of the rhs the level above just produced.
        pending = []
        if not zero_u:
            pending.append("u")
        if l > 0 and first_visit_rhs:
            pending.append("rhs")

        self._down_legs(l, zero_u, pending)
        for d in self.doms.values():
            d.u[l], d.t[l] = d.t[l], d.u[l]
        if last:
            self._replicated_cycle(l)
        else:
            for k in range(self._reps(l)):
                self._cycle_fused(l + 1, k == 0, k == 0)
        want_norm = (l == 0)
        if l == 0 and self._rec is not None:
            self._rec.mark_split()               # what follows -- the level-0 up legs and the norm -- is the back part
        parts = {}
        for r, d in self.doms.items():
            with self._ph("legs"):
                res = self._up_leg(d, l, d.u[l], d.t[l], want_norm)
            d.u[l], d.t[l] = d.t[l], d.u[l]
            if want_norm:
                parts[r] = self._add(res, d.ring_sumsq)
        if want_norm:
            self._last_norm_parts = parts

    def _cycle_per_operator(self, l):
        if self.var:
            raise NotImplementedError("the variable-coefficient operator runs on the fused legs (pre, post <= 2)")
        hx, hy = self.h[l]
        if self.pre > 0:
            self.smooth(l, self.pre)
        for d in self.doms.values():
            b = d.blk[l]
            self.ops.residual(d.u[l], d.rhs[l], d.r[l], b.lnx, b.lny, hx, hy, self.coeff)
        self.exchange("r", l, corners=True)
        for d in self.doms.values():
            g = self._leg(d, l)
            self.ops.restrict(d.r[l], g.target, g.b.lnx, g.b.lny, g.bc.lnx, g.bc.lny, g.bc.sides)
        if l + 1 == self.Ld:
            self._replicated_cycle(l)
        else:
            for d in self.doms.values():
                d.u[l + 1].zero_()
            for _ in range(self._reps(l)):
                self._cycle_per_operator(l + 1)
        for d in self.doms.values():
            g = self._leg(d, l)
            self.ops.prolong_add(g.e, d.u[l], g.b.lnx, g.b.lny, g.bc.lnx, g.bc.lny, g.b.sides)
        if self.post > 0:
            self.smooth(l, self.post)

    # ---- fields in / out -------------------------------------------------------------------------
    def set_coefficient(self, a_at):
        """Variable-coefficient operator A = coeff * div(a grad .) (BASELINE config 5; not in the reference).
        a_at(ix, iy) -> 2-D array of the vertex values of a at GLOBAL FINE-grid indices (1-D integer arrays ix, iy).
        Level l takes every 2^l-th fine vertex (injection, the single-GPU engine's rule), so every rank fills its blocks
        of every level -- ghost zones included -- from the function alone: no exchange.  None: constant coefficients."""
        torch = self.torch
        self._settle()
        if a_at is None:
            self.var = False
            self.ops.coarse_coefficient(None)
            return
        if self.mode != "fused":
            raise NotImplementedError("the variable-coefficient operator runs on the fused legs (pre, post <= 2)")
        for d in self.doms.values():
            for l in range(self.Ld):
                b = d.blk[l]
                vals = np.asarray(a_at((b.gx0 + np.arange(b.lnx)) << l, (b.gy0 + np.arange(b.lny)) << l))
                if d.a[l] is None:
                    d.a[l] = self.ops.alloc(b.lnx, b.lny, self.ldt[l])
                    d.rd[l] = self.ops.alloc(b.lnx, b.lny, self.ldt[l])
                d.a[l][:b.lnx, :b.lny] = torch.as_tensor(np.ascontiguousarray(vals, dtype=self.ldt[l])).to(d.a[l].device)
                # the reciprocal diagonal of the block (ghost zone included: it only needs the block's own coefficient values)
                self.ops.var_rdiag(d.a[l], d.rd[l], b.lnx, b.lny, self.h[l][0], self.h[l][1])
        NXa, NYa = self.shapes[self.Ld]
        self.ops.coarse_coefficient(np.ascontiguousarray(a_at(np.arange(NXa) << self.Ld, np.arange(NYa) << self.Ld), dtype=np.float64))
        self.var = True
        self._last_norm_parts = None
        self._norm_value = None

    def set_problem(self, rhs_of_block, u0_of_block=None):
        """rhs_of_block(block) -> (lnx, lny) array of f on that block (ghost zone and boundary included)."""
        torch = self.torch
        self._settle()
        for d in self.doms.values():
            b = d.blk[0]
            d.rhs[0][:b.lnx, :b.lny] = torch.as_tensor(np.ascontiguousarray(rhs_of_block(b), dtype=self.ldt[0])).to(d.rhs[0].device)
            d.u[0].zero_()
            if u0_of_block is not None:
                d.u[0][:b.lnx, :b.lny] = torch.as_tensor(np.ascontiguousarray(u0_of_block(b), dtype=self.ldt[0])).to(d.u[0].device)
            if d.t[0] is not None:
                d.t[0].copy_(d.u[0])
            if d.s[0] is not None:
                d.s[0].copy_(d.u[0])
            if self.mode == "fused":
                # boundary ring of every coarse rhs = injected ring of f (r = f on boundary cells), once per rhs;
                # sum of f^2 over the physical boundary cells of the exclusive window, for the norm
                for l in range(self.Ld):
                    g = self._leg(d, l)
                    self.ops.inject_ring(d.rhs[l], g.target, g.b.lnx, g.b.lny, g.bc.lnx, g.bc.lny, g.b.sides, g.ci, g.cj)
                i_lo, i_hi = self._leg(d, 0).win[:2]
                ring = torch.zeros(1, dtype=torch.float64, device=d.rhs[0].device)
                if b.sides & SIDE_ILO:
                    ring = ring + self.ops.sumsq(d.rhs[0], 0, 1, b.j_lo, b.j_hi)
                if b.sides & SIDE_IHI:
                    ring = ring + self.ops.sumsq(d.rhs[0], b.lnx - 1, b.lnx, b.j_lo, b.j_hi)
                if b.sides & SIDE_JLO:
                    ring = ring + self.ops.sumsq(d.rhs[0], i_lo, i_hi, 0, 1)
                if b.sides & SIDE_JHI:
                    ring = ring + self.ops.sumsq(d.rhs[0], i_lo, i_hi, b.lny - 1, b.lny)
                if d.ring_sumsq is None:
                    d.ring_sumsq = ring
                else:
                    d.ring_sumsq.copy_(ring)           # same buffer: a recorded plan holds its pointer
        if self.mode == "fused" and self.Ld > 0 and getattr(self.ops, "plan_capable", False):
            # the boundary ring of the gathered coarse rhs is final now (its interior is rewritten every cycle): the
            # replicated engine takes it -- and the rings of its own coarser levels -- once per problem
            self._gather_coarse_rhs()
            self.ops.coarse_begin(self.rhs_a, same_ring=False)
        self._last_norm_parts = None
        self._norm_value = None

    def residual_norm(self):
        hx, hy = self.h[0]
        if self._norm_pending:
            self._norm_value = (self._norm_plan or self._plan_back).wait()
            self._norm_pending = False
        if self._norm_value is not None:            # a native cycle brought the sum back with it
            return math.sqrt(hx * hy * self._norm_value)
        if self._last_norm_parts is not None:       # the up leg of the last cycle already summed r^2 over the owned cells
            return math.sqrt(hx * hy * self.allreduce_sum(self._last_norm_parts))
        if self.mode == "fused":
            self.exchange("u", 0)
        parts = {}
        if self.var:
            # no stand-alone variable-coefficient residual on device arrays: an up leg without sweeps on a zero correction
            # (out = u + P 0 = u, then sum r^2 over the owned cells)
            for r, d in self.doms.items():
                if d.zc is None:
                    bc = d.blk[1]
                    d.zc = self.ops.alloc(bc.lnx, bc.lny, self.ldt[1])
                res = self._up_leg(d, 0, d.u[0], d.t[0], True, e=d.zc, nsweep=0)
                d.t[0].copy_(d.u[0])
                parts[r] = res + d.ring_sumsq
            return math.sqrt(hx * hy * self.allreduce_sum(parts))
        for r, d in self.doms.items():
            b = d.blk[0]
            tmp = d.r[0] if d.r[0] is not None else d.t[0]
            self.ops.residual(d.u[0], d.rhs[0], tmp, b.lnx, b.lny, hx, hy, self.coeff)
            parts[r] = self.ops.sumsq(tmp, b.i_lo, b.i_hi, b.j_lo, b.j_hi)
            if d.r[0] is None:                       # t doubled as scratch: restore its boundary ring / contents
                tmp.copy_(d.u[0])
        return math.sqrt(hx * hy * self.allreduce_sum(parts))

    def iterate_sumsq(self):
        """sum of u^2 over the whole grid (every rank its exclusive window), as a Python float on every rank"""
        self._settle()
        parts = {}
        for r, d in self.doms.items():
            b = d.blk[0]
            parts[r] = self.ops.sumsq(d.u[0], b.i_lo, b.i_hi, b.j_lo, b.j_hi)
        return self.allreduce_sum(parts)

    def take_iterate_from(self, other):
        """The fine iterate of `other` (same decomposition, another working precision) becomes this solver's iterate:
        the on-device cast of PrecisionManager.convert_array (core/precision.py:106-134), ghost zone included."""
        self._settle()
        for r, d in self.doms.items():
            b = d.blk[0]
            d.u[0][:b.lnx, :b.lny].copy_(other.doms[r].u[0][:b.lnx, :b.lny])      # torch casts on the device; pitches differ
            if d.t[0] is not None:
                # the ping-pong partner only needs the outermost ring (Dirichlet values on physical edges; the legs rewrite
                # everything inside it)
                u, t = d.u[0], d.t[0]
                for t in (d.t[0], d.s[0]):
                    if t is not None:
                        t[0, :b.lny].copy_(u[0, :b.lny]); t[b.lnx - 1, :b.lny].copy_(u[b.lnx - 1, :b.lny])
                        t[:b.lnx, 0].copy_(u[:b.lnx, 0]); t[:b.lnx, b.lny - 1].copy_(u[:b.lnx, b.lny - 1])
        self._last_norm_parts = None
        self._norm_value = None

    def local_solution(self, rank):
        d = self.doms[rank]
        b = d.blk[0]
        return b, d.u[0][:b.lnx, :b.lny].cpu().numpy()

    def close(self):
        self._drop_plan()
        self._comm = None                        # shared per process: dist_plan.shutdown() destroys it
        self.ops.close()


def __getattr__(name):
    """distributed.bench_main & co.: the benchmark lives in dist_bench, which imports this module -- resolved on first use"""
    if name in ("bench_main", "plan_selfcheck", "_bench_ranks", "_first_difference"):
        from . import dist_bench
        return getattr(dist_bench, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
