"""Helpers shared by the GPU suites of the fluid + scalar step over row slabs (tests/test_gpu_ade_slabs.py, _iwalls_slabs,
_open_slabs, _kbc_slabs and the slab tests of test_gpu_ade_scalar_bc.py and test_gpu_ade_buoyancy.py): the one chain
emulator (Chain), the edges of a slab, the test body of interior walls, what a view holds, the carry of an open table, the
start state on the global lattice, and the write-set check of a part.  Which entry point a suite goes through stays the
suite's choice: it hands Chain an `advance` and the write-set check a launcher, both built on tests/ade_calls.py."""
import ctypes as ct

import numpy as np
import torch

import pylbm
from ade_util import (SENTINEL, W, alloc, assert_write_set, bits, cut_slab, geom, initial_state, owned, poisoned,
                      to_lattice)
from gpu_util import dev
from pylbm import _ptr

FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
HALO = pylbm.EDGE_HALO
NO_FLUX = pylbm.ADE_SCALAR_NO_FLUX
ROW_NEG, COL_NEG = pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_NEG


def slab_bc(gbc, r0, r1, Rg, closed=False):
    """the edges of the slab of global rows [r0, r1): HALO at a seam (every row edge of a closed ring), the global
    domain's at a chain end and on the columns"""
    return pylbm.Bc(row_lo=HALO if (closed or r0 > 0) else gbc.row_lo, row_hi=HALO if (closed or r1 < Rg) else gbc.row_hi,
                    col_lo=gbc.col_lo, col_hi=gbc.col_hi)


def global_state(oracle, Rg, C, seed=0, w=W, **kw):
    """(geometry, [f, g]): ade_util.initial_state as the pre-collision lattices of the global box (dense, ghost 0)"""
    gg = geom(Rg, C, 0)
    return gg, [to_lattice(a, gg) for a in initial_state(oracle, Rg, C, seed, w, **kw)]


def assert_finite(lats, g, what):
    for k, t in enumerate(lats):
        assert bool(torch.isfinite(owned(t, g)).all()), f"{what}: the yardstick's lattice {k} is not finite"


# ---- tables and views ----------------------------------------------------------------------------------------------------
def body_segments(R):
    """the test body on a lattice of R rows: a column wall at column 20 through ALL rows (a wall node on every seam row
    and in every band) and the row walls at rows 5 and 29, columns 20..30, that fit: (r0, c0, dr, dc, n, slots)"""
    return [(0, 20, 1, 0, R, COL_NEG)] + [(r, 20, 0, 1, 11, ROW_NEG) for r in (5, 29) if r < R]


def body_table(lib, R, C, rule=(NO_FLUX, 0.0), finalize=True):
    t = pylbm.AdeInteriorWalls(lib, R, C)
    for r0, c0, dr, dc, n, slots in body_segments(R):
        t.add(r0, c0, dr, dc, n, slots, slots, *rule)
    return t.finalize() if finalize else t


def bands_hold_nodes(table, E):
    """every band of a part launch with E edge rows holds a node of the (slab-local) table or view"""
    rows = {n["r"] for n in table.nodes()}
    R = table.R
    return all(any(a <= r < b for r in rows) for a, b in ((0, E), (E, R - E), (R - E, R)))


def first_index(table, row0):
    """the index in the parent of the first node of a view that starts at row0"""
    return sum(1 for n in table.nodes() if n["r"] < row0)


def carry_like(table, seed=None):
    """a carry of the open table: SENTINEL, or (seed) velocities of a few per cent"""
    if table is None:
        return None
    n = table.carry_len()
    if seed is None:
        t = torch.zeros(n, dtype=torch.float64, device=dev())
        bits(t).fill_(SENTINEL)
        return t
    return torch.from_numpy(0.03 * np.random.default_rng(seed).standard_normal(n)).to(dev())


# ---- the chain -----------------------------------------------------------------------------------------------------------
class Chain:
    """slabs of the given heights of one global box, every slab in turn on this GPU: advance(slab, dst, src, e) -- the
    suite's FRAME + INNER with e = min(E, (R - 1) // 2) edge rows -- then the single-step halo of BOTH lattices by
    lbm_halo_pack -> lbm_halo_unpack across every seam (the wrap-around one of a closed ring included; the last slab of
    an open chain and a chain of one slab exchange nothing).

    A slab is a dict: g (ghost 1, row pitch `pitch`), bc (slab_bc of gbc), r0, r1, lat = [time level][f, g] cut from the
    global post-collision pair `post` (cut_slab: ghost rows wrapped on a closed ring, poisoned beyond a wall), cur (the
    time level it is at), and whatever per_slab(k, r0, r1, bc) returns for it -- sliced descriptors, views, carries."""

    def __init__(self, lib, gg, post, heights, closed, gbc, advance, pitch=0, per_slab=None):
        self.lib, self.closed, self.n, self.advance = lib, closed, len(heights), advance
        self.r0 = np.concatenate([[0], np.cumsum(heights)]).tolist()
        self.slabs = []
        for k in range(self.n):
            a, b = self.r0[k], self.r0[k + 1]
            cut = [cut_slab(p, gg, a, b, pitch, closed) for p in post]
            g = cut[0][0]
            s = dict(g=g, bc=slab_bc(gbc, a, b, gg.R, closed), r0=a, r1=b, cur=0,
                     lat=[[cut[0][1], cut[1][1]], [alloc(g), alloc(g)]])
            if per_slab is not None:
                s.update(per_slab(k, a, b, s["bc"]))
            self.slabs.append(s)
        self.msg = lib.raw.lbm_halo_rows(1) * gg.C
        self.cur = 0

    def step(self, E):
        lib, cur = self.lib, self.cur
        for s in self.slabs:
            self.advance(s, s["lat"][cur ^ 1], s["lat"][cur], min(E, (s["g"].R - 1) // 2))
        n = self.n
        for k in range(n):
            if (not self.closed and k == n - 1) or n == 1:
                continue
            a, b = self.slabs[k], self.slabs[(k + 1) % n]  # slab a's high edge meets slab b's low edge
            for j in range(2):
                down = torch.empty(self.msg, dtype=torch.float64, device=dev())
                up = torch.empty(self.msg, dtype=torch.float64, device=dev())
                lib.halo_pack(_ptr(down), _ptr(a["lat"][cur ^ 1][j]), ct.byref(a["g"]), 1, 1, None)
                lib.halo_pack(_ptr(up), _ptr(b["lat"][cur ^ 1][j]), ct.byref(b["g"]), 1, 0, None)
                lib.halo_unpack(_ptr(b["lat"][cur ^ 1][j]), _ptr(down), ct.byref(b["g"]), 1, 0, None)
                lib.halo_unpack(_ptr(a["lat"][cur ^ 1][j]), _ptr(up), ct.byref(a["g"]), 1, 1, None)
        self.cur ^= 1
        for s in self.slabs:
            s["cur"] = self.cur

    def gather(self, j):
        """lattice j of the whole box: the slabs' owned rows, [9, Rg, C]"""
        return torch.cat([owned(s["lat"][self.cur][j], s["g"]) for s in self.slabs], dim=1)

    def close(self):
        for s in self.slabs:
            for v in s.values():
                if hasattr(v, "close"):
                    v.close()


class OneSlabRing:
    """a ring of one rank in this process, not closed: a chain of one slab -- nothing travels, both parts run on `main`"""

    def __init__(self, lib, sg):
        self.lib, self.ring, ident = lib, ct.c_void_p(), (ct.c_ubyte * 128)()
        lib.ring_unique_id(ident)
        lib.ring_create(ct.byref(self.ring), ident, 0, 1, ct.byref(sg), 0)

    def __enter__(self):
        return self.ring

    def __exit__(self, *exc):
        self.lib.ring_destroy(self.ring)


# ---- the write set of a part ---------------------------------------------------------------------------------------------
def assert_part_write_sets(launch, g, want, E, what, also=None):
    """launch(dst, which) runs ONE part into the lattices dst.  Into NaN-poisoned lattices -- ghost rows, row padding and
    plane padding included -- each part alone writes exactly its rows of both lattices in all 9 planes
    (ade_util.assert_write_set), and every written double is the one of `want`, where FRAME + INNER ran together.
    also(which, rows, what): the suite's further checks of that part (a carry)"""
    R = g.R
    for which, name, rows in ((FRAME, "FRAME", list(range(E)) + list(range(R - E, R))), (INNER, "INNER", list(range(E, R - E)))):
        dst = (poisoned(g), poisoned(g))
        torch.cuda.synchronize()
        launch(dst, which)
        torch.cuda.synchronize()
        expect = torch.zeros(9 * g.plane_stride, dtype=torch.bool, device=dev())
        owned(expect, g)[:, rows] = True
        for k in range(2):
            assert_write_set(dst[k], g, rows, f"{name} {what} lattice {k}")
            diff = torch.nonzero(expect & (bits(dst[k]) != bits(want[k])))
            assert diff.numel() == 0, f"{name} {what} lattice {k}: {diff.shape[0]} written doubles differ from FRAME + INNER"
        if also is not None:
            also(which, rows, f"{name} {what}")
