"""Grid metadata in three dimensions (host side): Grid's constructor, attributes, coarsen / refine rules and messages with a
third axis.  X, Y, Z are built on first use.  The l2 norm is summed on the device (mg3_dev_norm, include/mghip_3d.h)."""
import ctypes as C

import numpy as np

from . import _lib


class Grid3D:
    def __init__(self, nx, ny, nz, domain=(0.0, 1.0, 0.0, 1.0, 0.0, 1.0), dtype=np.float64):
        if nx < 3 or ny < 3 or nz < 3:
            raise ValueError("Grid must have at least 3 points in each direction")
        if len(tuple(domain)) != 6:
            raise ValueError("a 3-D domain holds six numbers (x0, x1, y0, y1, z0, z1)")
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.domain = tuple(domain)
        self.dtype = dtype
        self.hx = (domain[1] - domain[0]) / (nx - 1)
        self.hy = (domain[3] - domain[2]) / (ny - 1)
        self.hz = (domain[5] - domain[4]) / (nz - 1)
        self.h = min(self.hx, self.hy, self.hz)
        self.x = np.linspace(domain[0], domain[1], nx, dtype=dtype)
        self.y = np.linspace(domain[2], domain[3], ny, dtype=dtype)
        self.z = np.linspace(domain[4], domain[5], nz, dtype=dtype)
        self._mesh3 = None

    def _mesh(self):
        if self._mesh3 is None:
            self._mesh3 = np.meshgrid(self.x, self.y, self.z, indexing="ij")
        return self._mesh3

    @property
    def X(self):
        return self._mesh()[0]

    @property
    def Y(self):
        return self._mesh()[1]

    @property
    def Z(self):
        return self._mesh()[2]

    @property
    def shape(self):
        return (self.nx, self.ny, self.nz)

    @property
    def size(self):
        return self.nx * self.ny * self.nz

    def interior_slice(self):
        return (slice(1, -1), slice(1, -1), slice(1, -1))

    def coarsen(self):
        if (self.nx - 1) % 2 != 0 or (self.ny - 1) % 2 != 0 or (self.nz - 1) % 2 != 0:
            raise ValueError("Cannot coarsen grid: need even number of interior points")
        return Grid3D((self.nx - 1) // 2 + 1, (self.ny - 1) // 2 + 1, (self.nz - 1) // 2 + 1, self.domain, self.dtype)

    def refine(self):
        return Grid3D(2 * (self.nx - 1) + 1, 2 * (self.ny - 1) + 1, 2 * (self.nz - 1) + 1, self.domain, self.dtype)

    def l2_norm(self, field):
        """sqrt(hx*hy*hz*sum(field^2)) over all cells: fixed-order reduction on the device, fp64 accumulation"""
        import torch
        f = _lib.as_c(field)
        if f.shape != self.shape:
            raise ValueError(f"Field shape {f.shape} doesn't match grid shape {self.shape}")
        lib = _lib.load()
        ld = self.nz + (self.nz & 1)
        dev = torch.zeros((self.nx, self.ny, ld), dtype=torch.float64 if f.dtype == np.float64 else torch.float32, device="cuda")
        dev[:, :, :self.nz] = torch.from_numpy(f).to("cuda")
        nbytes = C.c_int64(0)
        _lib.check(lib.mg3_dev_scratch_bytes(self.nx, self.ny, self.nz, C.byref(nbytes)))
        scratch = torch.zeros(nbytes.value // 8 + 1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _lib.check(lib.mg3_dev_norm(_lib.dtype_code(f.dtype), self.nx, self.ny, self.nz, ld, C.c_void_p(dev.data_ptr()),
                                    C.c_void_p(scratch.data_ptr()), C.c_void_p(scratch[-1:].data_ptr()), None))
        torch.cuda.synchronize()
        return float(np.sqrt(self.hx * self.hy * self.hz * float(scratch[-1].item())))

    def max_norm(self, field):
        return float(np.max(np.abs(field)))

    def __repr__(self):
        return f"Grid3D(nx={self.nx}, ny={self.ny}, nz={self.nz}, domain={self.domain}, dtype={self.dtype})"

    __str__ = __repr__
