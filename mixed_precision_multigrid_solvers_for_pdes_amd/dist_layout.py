"""Index bookkeeping of the block decomposition (pure Python, no device): level shapes, the process grid, one rank's block of
one level, the number of levels that stay distributed, the ghost widths of the fused mode.  distributed.py explains the
decomposition these describe."""
import math

import numpy as np

SIDE_ILO, SIDE_IHI, SIDE_JLO, SIDE_JHI = 1, 2, 4, 8


def hierarchy_shapes(nx, ny, max_levels):
    """Global level shapes by the reference's rule (solvers/multigrid.py:153-171)."""
    shapes = [(nx, ny)]
    for _ in range(1, max_levels):
        a, b = shapes[-1]
        if (a - 1) % 2 or (b - 1) % 2:
            break
        c = ((a - 1) // 2 + 1, (b - 1) // 2 + 1)
        if c[0] < 5 or c[1] < 5:
            break
        shapes.append(c)
    return shapes


def process_grid(world):
    """px x py with px >= py, as square as possible (1, 2x1, 2x2, 4x2)."""
    py = int(math.sqrt(world))
    while world % py:
        py -= 1
    return world // py, py


class Block:
    """One rank's block of one level: owned cells, a ghost zone of `G` cells towards every neighbour, the physical
    boundary row/column where the block touches the domain boundary.  Local (0, 0) has an even global index."""

    def __init__(self, NX, NY, px, py, rx, ry, G=1):
        mx, my = (NX - 1) // px, (NY - 1) // py
        self.NX, self.NY, self.G = NX, NY, G
        self.gx0 = 0 if rx == 0 else rx * mx - (G - 1)              # global index of local (0, 0)
        self.gy0 = 0 if ry == 0 else ry * my - (G - 1)
        gx1 = NX - 1 if rx == px - 1 else (rx + 1) * mx + G          # global index of the last local row
        gy1 = NY - 1 if ry == py - 1 else (ry + 1) * my + G
        self.lnx, self.lny = gx1 - self.gx0 + 1, gy1 - self.gy0 + 1
        self.sides = ((SIDE_ILO if rx == 0 else 0) | (SIDE_IHI if rx == px - 1 else 0) |
                      (SIDE_JLO if ry == 0 else 0) | (SIDE_JHI if ry == py - 1 else 0))
        # owned interior cells (local indices, inclusive)
        self.oi_lo = rx * mx + 1 - self.gx0
        self.oi_hi = (NX - 2 if rx == px - 1 else (rx + 1) * mx) - self.gx0
        self.oj_lo = ry * my + 1 - self.gy0
        self.oj_hi = (NY - 2 if ry == py - 1 else (ry + 1) * my) - self.gy0
        # exclusive window: owned cells plus the adjacent physical boundary cells (a disjoint cover of the grid)
        self.i_lo = 0 if rx == 0 else self.oi_lo
        self.i_hi = self.lnx if rx == px - 1 else self.oi_hi + 1
        self.j_lo = 0 if ry == 0 else self.oj_lo
        self.j_hi = self.lny if ry == py - 1 else self.oj_hi + 1

    def coarse_offsets(self, coarse):
        """(ci_off, cj_off): coarse local (ic, jc) sits on fine local (2 (ic - ci_off), 2 (jc - cj_off))."""
        return (self.gx0 - 2 * coarse.gx0) // 2, (self.gy0 - 2 * coarse.gy0) // 2


def distributed_levels(shapes, px, py, agglomerate_at, G=1):
    """Number of leading levels that stay distributed.  A level is distributed while its cuts are even
    (so the next level lines up), its blocks own at least max(4, G + 1) rows/cols -- and those of the level below
    at least G, whose ghost zone the correction is cut out for -- and it is larger than `agglomerate_at` points in
    some direction; at least one level is always left for the replicated part."""
    n = 0
    need = max(4, G + 1)
    for (NX, NY) in shapes[:-1]:
        if (NX - 1) % px or (NY - 1) % py:
            break
        mx, my = (NX - 1) // px, (NY - 1) // py
        if (px > 1 and (mx % 2 or mx < need or mx // 2 < G)) or (py > 1 and (my % 2 or my < need or my // 2 < G)):
            break
        if max(NX, NY) <= agglomerate_at:
            break
        n += 1
    return n


# Ghost width of the fused mode: the smallest odd G for which the owned cells stay exact through every fused visit.
# With s = halo cells a leg's two sweeps consume (Jacobi 2, red-black GS 4: one per colour pass), m exact ghost cells
# after the up leg of a level and m_c on the level below: m = min(G - s, 2 m_c - 1) - s; the recursion must reproduce
# itself (m_c = m) and leave m >= 1 for the norm: Jacobi m = 3, G = 7; red-black GS m = 5, G = 13.
GHOST_FUSED = {"jacobi": 7, "rbgs": 13}


def sine_rhs_block(b, domain=(0.0, 1.0, 0.0, 1.0)):
    """f = 2 pi^2 sin(pi x) sin(pi y) on one block, from GLOBAL indices (identical bits on every rank count)."""
    x = np.linspace(domain[0], domain[1], b.NX)[b.gx0:b.gx0 + b.lnx]
    y = np.linspace(domain[2], domain[3], b.NY)[b.gy0:b.gy0 + b.lny]
    return 2 * np.pi**2 * np.sin(np.pi * x)[:, None] * np.sin(np.pi * y)[None, :]
