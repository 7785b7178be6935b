"""libmghip's device-pointer entry points (mg_dev_*) on torch tensors: the kernel provider of the decomposed driver
(distributed.py).  The tests' NumPy stand-in implements the same interface."""
import ctypes as C

import numpy as np

from . import _lib


class HipOps:
    """mg_dev_* on CUDA tensors.  A field is a 2-D tensor (lnx, ld) whose first lny columns are the data; its precision
    is the tensor's dtype (levels of one hierarchy may differ: per-level mixed precision)."""

    def __init__(self, dtype, device, managed_single=False, mixed=False):
        """dtype: the default field precision (`alloc` without a dtype).
        managed_single (fp32 fields only): the reference's PrecisionManager('single') layout on a float64 Grid --
        interpolation in fp64 and the coarsest level solved in fp64 (otherwise an fp32 coarsest solve can never
        meet the 1e-12 tolerance and burns its 1000 sweeps on every visit, exactly like Grid(dtype=float32) does).
        mixed: PrecisionManager('mixed') on a float64 Grid (core/precision.py:337-357): the caller allocates coarse
        levels in fp32; interpolation runs in fp64 (the grid dtype)."""
        import torch
        self.torch = torch
        self.lib = _lib.load()
        self.np_dtype = np.dtype(dtype)
        self.dt = _lib.dtype_code(dtype)
        self.managed = bool(managed_single) and self.dt == _lib.MG_F32
        self.mixed = bool(mixed)
        self.comp_dt = _lib.MG_F64 if (self.managed or self.mixed) else self.dt
        self.tdtype = torch.float32 if self.dt == _lib.MG_F32 else torch.float64
        self.device = device
        self.scratch = torch.zeros(2048, dtype=torch.float64, device=device)          # grown per field shape (_scratch_for)
        self.acc = torch.zeros(1, dtype=torch.float64, device=device)
        self._engine = None
        self._coarse_ring_valid = False # the replicated engine holds the boundary ring of the current problem's coarse rhs
        self.rec = None                 # dist_plan.PlanRecorder while a cycle is being recorded

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _scratch_for(self, lnx, lny):
        """Partial-sum scratch of at least mg_dev_scratch_bytes(lnx, lny) (the library writes one fp64 per workgroup)."""
        nbytes = C.c_int64(0)
        _lib.check(self.lib.mg_dev_scratch_bytes(int(lnx), int(lny), C.byref(nbytes)))
        if self.scratch.numel() * 8 < nbytes.value:
            self.scratch = self.torch.zeros(nbytes.value // 8, dtype=self.torch.float64, device=self.device)
        return self._p(self.scratch)

    def _code(self, t):
        return _lib.MG_F32 if t.dtype == self.torch.float32 else _lib.MG_F64

    def alloc(self, lnx, lny, dtype=None):
        code = self.dt if dtype is None else _lib.dtype_code(dtype)
        ld = C.c_int(0)
        _lib.check(self.lib.mg_pitch_elems(code, lny, C.byref(ld)))
        return self.torch.zeros((lnx, ld.value), dtype=self.torch.float32 if code == _lib.MG_F32 else self.torch.float64,
                                device=self.device)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr())

    def jacobi(self, u, rhs, out, lnx, lny, hx, hy, omega):
        _lib.check(self.lib.mg_dev_jacobi(self._code(u), lnx, lny, u.stride(0), hx, hy, omega, self._p(u), self._p(rhs),
                                          self._p(out), self._stream()))

    def rbgs_colour(self, u, rhs, lnx, lny, hx, hy, omega, colour, offset):
        _lib.check(self.lib.mg_dev_rbgs_colour(self._code(u), lnx, lny, u.stride(0), hx, hy, omega, colour, offset,
                                               self._p(u), self._p(rhs), self._stream()))

    def residual(self, u, f, r, lnx, lny, hx, hy, coeff):
        _lib.check(self.lib.mg_dev_residual(self._code(u), lnx, lny, u.stride(0), hx, hy, coeff, self._p(u), self._p(f),
                                            self._p(r), self._stream()))

    def sumsq(self, field, i_lo, i_hi, j_lo, j_hi):
        """fp64 sum of squares of the window as a 1-element device tensor."""
        _lib.check(self.lib.mg_dev_sumsq(self._code(field), field.stride(0), i_lo, i_hi, j_lo, j_hi, self._p(field),
                                         self._scratch_for(i_hi, j_hi), self._p(self.acc), self._stream()))
        return self.acc.clone()

    def restrict(self, fine, coarse, lnxf, lnyf, lnxc, lnyc, sides):
        _lib.check(self.lib.mg_dev_restrict_fw(self._code(fine), self._code(coarse), lnxf, lnyf, fine.stride(0), lnxc, lnyc,
                                               coarse.stride(0), sides, self._p(fine), self._p(coarse), self._stream()))

    def prolong_add(self, coarse, fine_u, lnxf, lnyf, lnxc, lnyc, sides):
        _lib.check(self.lib.mg_dev_prolong_add(self._code(coarse), self._code(fine_u), self.comp_dt, lnxf, lnyf, fine_u.stride(0),
                                               lnxc, lnyc, coarse.stride(0), sides, self._p(coarse), self._p(fine_u), self._stream()))

    # fused legs (mode "fused"): the single-GPU engine's kernels on the local array with its ghost zone
    supports_overlap = True
    plan_capable = True               # cycles can be recorded into a native plan (dist_plan.py)

    def var_rdiag(self, a, rd, lnx, lny, hx, hy, sigma=0.0):
        """reciprocal diagonal of -div(a grad .) on this array (mg_dev_var_rdiag): what the variable-coefficient sweeps multiply by"""
        _lib.check(self.lib.mg_dev_var_rdiag(self._code(a), lnx, lny, a.stride(0), hx, hy, float(sigma), self._p(a), self._p(rd), self._stream()))

    def down_leg(self, sm, u, rhs, out, rhs_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, hx, hy, omega, coeff, nsweep, zero_init, poff,
                 select=0, inner=None, acoef=None, rdiag=None):
        """select: 0 all tiles; 1 only tiles that need nothing outside `inner` = (i_lo, i_hi, j_lo, j_hi); 2 the others.
        acoef / rdiag: vertex values of the diffusion coefficient on this array and its reciprocal diagonal (var_rdiag);
        None: constant-coefficient operator."""
        rect = (C.c_int * 4)(*inner) if inner is not None else None
        _lib.check(self.lib.mg_dev_down_leg_var(sm, self._code(rhs), self._code(rhs_c), lnx, lny, rhs.stride(0), lnxc, lnyc,
                                                rhs_c.stride(0), ci_off, cj_off, hx, hy, omega, coeff, nsweep, int(zero_init), poff,
                                                None if zero_init else self._p(u), self._p(rhs), self._p(out), self._p(rhs_c),
                                                self._stream(), int(select), rect, None if acoef is None else self._p(acoef),
                                                None if rdiag is None else self._p(rdiag)))
        if self.rec is not None:
            clamp = lambda v: max(-(1 << 30), min(1 << 30, int(v)))
            self.rec.emit(_lib.MG_PLAN_DOWN_LEG,
                          i=(sm, self._code(rhs), self._code(rhs_c), lnx, lny, rhs.stride(0), lnxc, lnyc, rhs_c.stride(0), ci_off, cj_off,
                             nsweep, int(zero_init), poff, int(select), int(inner is not None)) + tuple(clamp(v) for v in (inner or (0, 0, 0, 0))),
                          d=(hx, hy, omega, coeff), p=(None if zero_init else u, rhs, out, rhs_c, acoef, rdiag))

    def up_leg(self, sm, u, rhs, out, e_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, sides, hx, hy, omega, coeff, nsweep, poff,
               window=None, acoef=None, rdiag=None):
        """out = sweeps(u + P e_c); with `window` = (i_lo, i_hi, j_lo, j_hi) also returns sum r^2 over it (device tensor)."""
        w = window or (0, 0, 0, 0)
        res = self.torch.empty(1, dtype=self.torch.float64, device=self.device) if window is not None else self.acc
        self._scratch_for(lnx, lny)
        _lib.check(self.lib.mg_dev_up_leg_var(sm, self._code(u), self._code(e_c), self.comp_dt, lnx, lny, u.stride(0), lnxc, lnyc,
                                              e_c.stride(0), ci_off, cj_off, sides, hx, hy, omega, coeff, nsweep, poff, self._p(u),
                                              self._p(rhs), self._p(out), self._p(e_c), int(window is not None), w[0], w[1], w[2],
                                              w[3], self._p(self.scratch), self._p(res), self._stream(),
                                              None if acoef is None else self._p(acoef), None if rdiag is None else self._p(rdiag)))
        if self.rec is not None:
            self.rec.emit(_lib.MG_PLAN_UP_LEG,
                          i=(sm, self._code(u), self._code(e_c), self.comp_dt, lnx, lny, u.stride(0), lnxc, lnyc, e_c.stride(0), ci_off,
                             cj_off, sides, nsweep, poff, int(window is not None)) + tuple(w),
                          d=(hx, hy, omega, coeff), p=(u, rhs, out, e_c, self.scratch, res, acoef, rdiag))
        return res if window is not None else None

    def span_ok(self, sm, u, e_c, lnx, lny):
        """the spanning leg serves this block (weighted Jacobi, one dtype, above ~1100^2 cells: include/mghip.h)"""
        return bool(self.lib.mg_dev_span_leg_ok(sm, self._code(u), self._code(e_c), self.comp_dt, lnx, lny))

    def span_leg(self, sm, u, rhs, out_mid, out_next, e_c, rhs_c, lnx, lny, lnxc, lnyc, ci_off, cj_off, sides, hx, hy, omega, coeff,
                 nsweep_post, nsweep_pre, poff, window):
        """up_leg of cycle k (u -> out_mid, sum r^2 over `window`) and down_leg of cycle k + 1 (-> out_next, rhs_c) in one
        launch (mg_dev_span_leg); returns the sum as a device tensor"""
        res = self.torch.empty(1, dtype=self.torch.float64, device=self.device)
        self._scratch_for(lnx, lny)
        w = window
        _lib.check(self.lib.mg_dev_span_leg(sm, self._code(u), self._code(e_c), self.comp_dt, lnx, lny, u.stride(0), lnxc, lnyc,
                                            e_c.stride(0), ci_off, cj_off, sides, hx, hy, omega, coeff, nsweep_post, nsweep_pre, poff,
                                            self._p(u), self._p(rhs), self._p(out_mid), self._p(out_next), self._p(e_c), self._p(rhs_c),
                                            w[0], w[1], w[2], w[3], self._p(self.scratch), self._p(res), self._stream()))
        if self.rec is not None:
            self.rec.emit(_lib.MG_PLAN_SPAN_LEG,
                          i=(sm, self._code(u), self._code(e_c), self.comp_dt, lnx, lny, u.stride(0), lnxc, lnyc, e_c.stride(0), ci_off,
                             cj_off, sides, nsweep_post, nsweep_pre, poff) + tuple(w),
                          d=(hx, hy, omega, coeff), p=(u, rhs, out_mid, out_next, e_c, rhs_c, self.scratch, res))
        return res

    def inject_ring(self, fine, coarse, lnxf, lnyf, lnxc, lnyc, sides, ci_off, cj_off):
        _lib.check(self.lib.mg_dev_inject_ring(self._code(fine), self._code(coarse), lnxf, lnyf, fine.stride(0), lnxc, lnyc,
                                               coarse.stride(0), sides, ci_off, cj_off, self._p(fine), self._p(coarse), self._stream()))

    # replicated coarse hierarchy = the single-GPU engine on this GPU, queued on the same stream
    def coarse_setup(self, NX, NY, domain, cfg):
        """cfg["mixed_split"] (per-level mixed only): first fp32 level counted from the agglomeration level; <= 0 means
        every level of the replicated part but the coarsest is fp32."""
        from .engine import MultigridEngine
        split = 0
        if self.mixed:
            split = int(cfg.get("mixed_split", 0))
            prec = _lib.MG_PREC_MIXED_LEVELS if split > 0 else _lib.MG_PREC_SINGLE_MANAGED
        elif self.dt == _lib.MG_F32:
            prec = _lib.MG_PREC_SINGLE_MANAGED if self.managed else _lib.MG_PREC_SINGLE
        else:
            prec = _lib.MG_PREC_DOUBLE
        self._engine = MultigridEngine(NX, NY, domain, cfg["coeff"], cfg["levels"], cfg["cycle"], cfg["pre"], cfg["post"],
                                       cfg["smoother"], cfg["omega"], cfg["coarse_tol"], cfg["coarse_maxit"], prec,
                                       device=self.device.index or 0, mixed_split=max(split, 0))
        self._engine.set_stream(self._stream())

    def coarse_coefficient(self, a_host):
        """vertex values of the diffusion coefficient on the agglomeration level (host array; None: constant)"""
        self._engine.set_coefficient(a_host)

    def coarse_begin(self, rhs_global, same_ring=False):
        """same_ring: the boundary ring of rhs_global equals that of the previous call (the coarse right-hand side of a
        decomposed cycle: its ring is the injected ring of f, the same cycle after cycle) -- the replicated engine keeps the
        rings of its coarser levels instead of injecting them again (mg_update_rhs_device)."""
        e = self._engine
        same_ring = bool(same_ring) and self._coarse_ring_valid
        e.set_stream(self._stream())
        (e.update_rhs_device if same_ring else e.set_rhs_device)(rhs_global)
        self._coarse_ring_valid = True
        e.zero_solution_device()
        if self.rec is not None:
            self.rec.emit(_lib.MG_PLAN_COARSE_BEGIN, i=(rhs_global.stride(0), self._code(rhs_global), int(same_ring)), p=(e._h.value, rhs_global))

    def coarse_cycle(self):
        self._engine.cycle(1)
        if self.rec is not None:
            self.rec.emit(_lib.MG_PLAN_COARSE_CYCLE, i=(1,), p=(self._engine._h.value,))

    def coarse_end(self, out_global):
        self._engine.get_solution_device(out_global)
        if self.rec is not None:
            self.rec.emit(_lib.MG_PLAN_COARSE_END, i=(out_global.stride(0), self._code(out_global)), p=(self._engine._h.value, out_global))

    def close(self):
        if self._engine is not None:
            self.torch.cuda.synchronize()
            self._engine.close()
            self._engine = None
