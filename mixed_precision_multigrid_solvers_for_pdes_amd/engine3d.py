"""Multigrid3DEngine: owns an mg3_handle (include/mghip_3d.h), the device-resident 3-D hierarchy, as MultigridEngine owns the 2-D
one.  Host arrays are (nx, ny, nz), C order, of either dtype; torch device tensors go through the `_device` forms."""
import ctypes as C

import numpy as np

from . import _lib

SMOOTHERS = {"jacobi": _lib.MG_JACOBI, "rbgs": _lib.MG_RBGS, "red_black": _lib.MG_RBGS, "gauss_seidel": _lib.MG_RBGS}


def check3(rc, handle=None):
    """a status of the mg3_ family -> the exception _lib.check raises for it (the message is mg3_last_error's)"""
    if rc == _lib.MG_OK:
        return
    lib = _lib.load()
    msg = lib.mg3_last_error(handle) or lib.mg3_last_error(None)
    msg = (msg.decode() if msg else "") or f"mghip error {rc}"
    if rc in (_lib.MG_ERR_INVALID_VALUE, _lib.MG_ERR_STATE):
        raise ValueError(msg)
    if rc == _lib.MG_ERR_ALLOC:
        raise MemoryError(msg)
    if rc == _lib.MG_ERR_NO_DEVICE:
        raise RuntimeError("mghip: no usable HIP device (the multigrid path has no CPU fallback): " + msg)
    raise RuntimeError("mghip: " + msg)


def make_config(nx, ny, nz, domain=(0.0, 1.0, 0.0, 1.0, 0.0, 1.0), sigma=0.0, max_levels=10, cycle="V", pre=2, post=2,
                smoother="jacobi", omega=None, coarse_sweeps=64, precision="double", device=0):
    """an Mg3Config from keywords; omega None: 0.8 for Jacobi, 1 for red-black"""
    if isinstance(cycle, str):
        if cycle not in ("V", "W"):
            raise ValueError(f"unknown cycle type {cycle!r}: the 3-D engine runs V and W cycles")
        cycle = _lib.CYCLES[cycle]
    if isinstance(smoother, str):
        if smoother not in SMOOTHERS:
            raise ValueError(f"unknown smoother {smoother!r}: the 3-D engine has 'jacobi' and 'rbgs'")
        smoother = SMOOTHERS[smoother]
    if isinstance(precision, str):
        if precision not in _lib.MG3_PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}: 'double', 'single' or 'defect'")
        precision = _lib.MG3_PRECISIONS[precision]
    if len(tuple(domain)) != 6:
        raise ValueError("a 3-D domain holds six numbers (x0, x1, y0, y1, z0, z1)")
    if omega is None:
        omega = 0.8 if smoother == _lib.MG_JACOBI else 1.0
    return _lib.Mg3Config(int(nx), int(ny), int(nz), int(max_levels), *(float(v) for v in domain), float(sigma), float(omega),
                          int(cycle), int(pre), int(post), int(smoother), int(coarse_sweeps), int(precision), int(device), 0)


def device_bytes(cfg):
    """the bytes mg3_create allocates on the device for `cfg` (no device needed)"""
    out = C.c_int64(0)
    check3(_lib.load().mg3_device_bytes(C.byref(cfg), C.byref(out)))
    return out.value


class Multigrid3DEngine:
    """Owns a device-resident 3-D multigrid hierarchy.  The keywords are the fields of mg3_config."""

    def __init__(self, nx, ny, nz, **kw):
        lib = _lib.load()
        self.cfg = make_config(nx, ny, nz, **kw)
        self._h = C.c_void_p(None)
        check3(lib.mg3_create(C.byref(self.cfg), C.byref(self._h)))
        self._lib = lib
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        n = C.c_int(0)
        self._check(lib.mg3_num_levels(self._h, C.byref(n)))
        self.num_levels = n.value
        self.last_stats = None

    def _check(self, rc):
        check3(rc, self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mg3_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- fields: NumPy arrays, or torch device tensors (nx, ny, ld) whose first nz columns are the field ----
    @staticmethod
    def _is_tensor(a):
        return hasattr(a, "data_ptr")

    def _dev_args(self, t):
        if t.dim() != 3 or t.shape[0] != self.nx or t.shape[1] != self.ny or t.shape[2] < self.nz or t.stride(2) != 1 or \
                t.stride(0) != self.ny * t.stride(1):
            raise ValueError(f"a device field is an (nx, ny, >= nz) tensor with unit stride along k and a plane stride of ny rows, "
                             f"got shape {tuple(t.shape)} strides {tuple(t.stride())}")
        import torch
        torch.cuda.current_stream(t.device).synchronize()          # the handle queues on a stream of its own
        return C.c_void_p(t.data_ptr()), int(t.stride(1)), _lib.dtype_code(str(t.dtype).split(".")[-1])

    def _host(self, a):
        a = _lib.as_c(a)
        if a.shape != (self.nx, self.ny, self.nz):
            raise ValueError(f"Field shape {a.shape} doesn't match grid shape {(self.nx, self.ny, self.nz)}")
        return a

    def set_rhs(self, f):
        if self._is_tensor(f):
            self._check(self._lib.mg3_set_rhs_device(self._h, *self._dev_args(f)))
        else:
            f = self._host(f)
            self._check(self._lib.mg3_set_rhs(self._h, _lib.ptr(f), _lib.dtype_code(f.dtype)))

    def set_solution(self, u0=None):
        if u0 is None:
            self._check(self._lib.mg3_zero_solution(self._h))
        elif self._is_tensor(u0):
            self._check(self._lib.mg3_set_solution_device(self._h, *self._dev_args(u0)))
        else:
            u0 = self._host(u0)
            self._check(self._lib.mg3_set_solution(self._h, _lib.ptr(u0), _lib.dtype_code(u0.dtype)))

    def solution(self, out=None, dtype=np.float64):
        """the iterate: a new NumPy array of `dtype`, or into the device tensor `out` (waits for the handle's stream)"""
        if out is not None and self._is_tensor(out):
            self._check(self._lib.mg3_get_solution_device(self._h, *self._dev_args(out)))
            self.synchronize()
            return out
        res = np.empty((self.nx, self.ny, self.nz), dtype=dtype)
        self._check(self._lib.mg3_get_solution(self._h, _lib.ptr(res), _lib.dtype_code(dtype)))
        return res

    def cycle(self, n=1):
        self._check(self._lib.mg3_cycle(self._h, int(n)))

    def residual_norm(self):
        out = C.c_double(0.0)
        self._check(self._lib.mg3_residual_norm(self._h, C.byref(out)))
        return out.value

    def synchronize(self):
        self._check(self._lib.mg3_synchronize(self._h))

    def solve(self, tol, max_iter=100):
        """cycles until the residual norm is below `tol` (absolute) or max_iter is reached -> (history, converged)"""
        hist = (C.c_double * (int(max_iter) + 1))()
        n, conv, stats = C.c_int(0), C.c_int(0), _lib.Mg3Stats()
        self._check(self._lib.mg3_solve(self._h, float(tol), int(max_iter), hist, int(max_iter) + 1, C.byref(n), C.byref(conv),
                                        C.byref(stats)))
        self.last_stats = stats
        return [hist[k] for k in range(n.value + 1)], bool(conv.value)

    @property
    def device_bytes(self):
        return device_bytes(self.cfg)
