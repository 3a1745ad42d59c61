"""GPU suite, interior walls of the fluid + scalar step over row slabs and the ring: lbm_ade_iwalls_slab (the slab view of a
table), lbm_ade_stream_collide_part_w (k_ade_iwalls_ranges behind each part's dispatch), lbm_ring_ade_step_w and
slab_ring_ade --rectangle.

The yardstick is one block in the SAME form: lbm_ade_stream_collide_w on the global lattice with the global table (pinned
to the reference's loop bit for bit in tests/test_gpu_ade_iwalls.py).  Every comparison is bitwise, so there are no
tolerances -- except the scalar mass of the sealed seam, whose bound is that of test_a_sealed_wall_seals.

The body, on a global 48 x 64 lattice: a column wall at column 20 through ALL rows (COL_NEG for f and g) and row walls at
rows 5 and 29, columns 20..30 (ROW_NEG): 68 nodes, 34 in each of the views [0, 24), [24, 48), [12, 36).  The column wall
puts a node on the first and last row of every slab and into every FRAME and INNER band for any E; each test asserts that
each band it exercises holds a table node (bands_hold_nodes), so that none passes by testing nothing."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
from ade_util import (GBC, GUO, SENTINEL, W, alloc, assert_bits, bits, buoyancy, cut_slab, geom, owned, params,  # noqa: E402
                      random_lattice, to_lattice)
from gpu_util import dev  # noqa: E402
from proc_util import last_json, run_driver, run_ranks  # noqa: E402
from pylbm import _ptr  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
BB, SP, HALO, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO, pylbm.EDGE_PERIODIC
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_POS, ROW_NEG, COL_NEG = pylbm.ADE_FACE_ROW_POS, pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_NEG
RG, CG = 48, 64


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


def _ref(x):
    return ct.byref(x) if x is not None else None


def _h(t):
    return t.h if t is not None else None


# ---- the body and the calls under test -----------------------------------------------------------------------------------
def body_segments(R):
    """the test body on a lattice of R rows: (r0, c0, dr, dc, n, slots) -- the row walls that fit into R rows"""
    return [(0, 20, 1, 0, R, COL_NEG)] + [(r, 20, 0, 1, 11, ROW_NEG) for r in (5, 29) if r < R]


def body_table(lib, R, C, rule=(NO_FLUX, 0.0), finalize=True):
    t = pylbm.AdeInteriorWalls(lib, R, C)
    for r0, c0, dr, dc, n, slots in body_segments(R):
        t.add(r0, c0, dr, dc, n, slots, slots, *rule)
    return t.finalize() if finalize else t


def bands_hold_nodes(table, E):
    """every band of a part launch with E edge rows holds a node of the (slab-local) table"""
    rows = {n["r"] for n in table.nodes()}
    R = table.R
    return all(any(a <= r < b for r in rows) for a, b in ((0, E), (E, R - E), (R - E, R)))


def full_w(lib, g, bc, prm, fo, go, sbc=None, by=None, table=None, moments=None):
    """the yardstick: lbm_ade_stream_collide_w on one block"""
    fn, gn = alloc(g), alloc(g)
    m = [_ptr(t) for t in moments] if moments else [None, None, None]
    lib.ade_stream_collide_w(_ptr(fn), _ptr(gn), _ptr(fo), _ptr(go), ct.byref(g), ct.byref(bc), ct.byref(prm[0]),
                             ct.byref(prm[1]), _ref(sbc), _ref(by), _h(table), 0, g.R, *m, None)
    return fn, gn


def part_w(lib, g, bc, prm, dst, src, which, E, sbc=None, by=None, table=None, moments=None, stream=None):
    m = [_ptr(t) for t in moments] if moments else [None, None, None]
    lib.ade_stream_collide_part_w(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), ct.byref(g), ct.byref(bc),
                                  ct.byref(prm[0]), ct.byref(prm[1]), _ref(sbc), _ref(by), _h(table), which, E, *m,
                                  pylbm._stream(stream))


def part_b(lib, g, bc, prm, dst, src, which, E, sbc=None, by=None):
    lib.ade_stream_collide_part_b(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), ct.byref(g), ct.byref(bc),
                                  ct.byref(prm[0]), ct.byref(prm[1]), _ref(sbc), _ref(by), which, E, None, None, None, None)


def slab_bc(gbc, r0, r1, Rg, closed=False):
    return pylbm.Bc(row_lo=HALO if (closed or r0 > 0) else gbc.row_lo, row_hi=HALO if (closed or r1 < Rg) else gbc.row_hi,
                    col_lo=gbc.col_lo, col_hi=gbc.col_hi)


# ---- 1. FRAME + INNER with a view == the one-block step on the global lattice --------------------------------------------
CASES = {"no_flux": ((NO_FLUX, 0.0), False), "absorbing": ((FIXED, 0.0), False), "fixed_row_lo_buoyant": ((FIXED, 1e-3), True)}


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("C,pitch", [(CG, 0), (1040, 1056)], ids=["48x64", "48x1040_padded"])
def test_frame_plus_inner_with_a_view_is_the_one_block_step(lib, form, case, C, pitch):
    rule, driven = CASES[case]
    prm = params(form)
    by = buoyancy((2e-2, -1e-2), 1.0, GUO) if driven else None      # random_lattice: C ~ 1.0 .. 1.05
    gsbc = pylbm.AdeScalarBC(row_lo=1.02) if driven else None        # a FIXED domain edge beside the table's FIXED slots
    gg = geom(RG, C, 0, pitch)
    src = (random_lattice(gg, 11 + C), random_lattice(gg, 12 + C))
    table = body_table(lib, RG, C, rule)
    assert table.count() == 68
    twin = body_table(lib, RG, C, rule, finalize=False)
    want = full_w(lib, gg, GBC, prm, *src, sbc=gsbc, by=by, table=table)
    plain = full_w(lib, gg, GBC, prm, *src, sbc=gsbc, by=by)
    assert not torch.equal(bits(want[1]), bits(plain[1]))  # the body is felt
    for r0, r1 in ((0, 24), (24, 48), (12, 36)):
        view = table.slab(r0, r1 - r0)
        other = twin.slab(r0, r1 - r0)
        assert view.count() == 34 and view.nodes() == other.nodes()  # a finalized parent gives the unfinalized one's view
        other.close()
        view.finalize()
        bc = slab_bc(GBC, r0, r1, RG)
        sbc = gsbc if (driven and r0 == 0) else None  # a FIXED row acts where the slab keeps that edge
        slab = [cut_slab(s, gg, r0, r1, pitch) for s in src]
        sg = slab[0][0]
        for E in (1, 3, 8):
            assert bands_hold_nodes(view, E)
            dst = (alloc(sg), alloc(sg))
            part_w(lib, sg, bc, prm, dst, (slab[0][1], slab[1][1]), FRAME, E, sbc, by, view)
            part_w(lib, sg, bc, prm, dst, (slab[0][1], slab[1][1]), INNER, E, sbc, by, view)
            torch.cuda.synchronize()
            for k in range(2):
                assert_bits(owned(dst[k], sg), owned(want[k], gg)[:, r0:r1], f"{case} C={C} slab [{r0}, {r1}) E={E} lattice {k}")
        view.close()
    twin.close()
    table.close()


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_the_moment_outputs_of_wall_nodes_are_the_one_block_steps(lib, form):
    """ghost 0, periodic rows (what both entry points accept): rho, u, C of FRAME + INNER == lbm_ade_stream_collide_w's"""
    R, C, E = 24, CG, 3
    g, prm, bc = geom(R, C, 0), params(form), pylbm.Bc(col_lo=BB, col_hi=SP)
    table = body_table(lib, R, C, (FIXED, 1e-3))
    assert bands_hold_nodes(table, E)
    src = (random_lattice(g, 3), random_lattice(g, 4))

    def moments():
        m = [torch.zeros(n * R * C, dtype=torch.float64, device=dev()) for n in (1, 2, 1)]
        for t in m:
            bits(t).fill_(SENTINEL)
        return m

    mw, mp, mplain = moments(), moments(), moments()
    want = full_w(lib, g, bc, prm, *src, table=table, moments=mw)
    full_w(lib, g, bc, prm, *src, moments=mplain)
    dst = (alloc(g), alloc(g))
    for which in (FRAME, INNER):
        part_w(lib, g, bc, prm, dst, src, which, E, table=table, moments=mp)
    torch.cuda.synchronize()
    for k in range(2):
        assert_bits(owned(dst[k], g), owned(want[k], g), f"lattice {k}")
    for k, name in enumerate(("rho", "u", "C")):
        assert_bits(mp[k], mw[k], name)
    assert not torch.equal(bits(mw[2]), bits(mplain[2]))  # the wall nodes' C is the table's, not the plain step's
    table.close()


# ---- 2. NULL and empty table == _part_b ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_null_and_empty_tables_are_part_b(lib, form):
    R, C, E = 24, CG, 3
    prm = params(form)
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO, col_lo=BB, col_hi=SP)
    sbc, by = pylbm.AdeScalarBC(row_lo=1.02, col_hi=0.0), buoyancy((2e-2, -1e-2), 1.0, GUO)
    g = geom(R, C, 1, C + 6)
    src = (random_lattice(g, 1), random_lattice(g, 2))
    empty = pylbm.AdeInteriorWalls(lib, R, C).finalize()
    view = pylbm.AdeInteriorWalls(lib, 48, C).add(40, 3, 0, 1, 5, ROW_NEG, ROW_NEG).slab(0, R).finalize()  # no node in its rows
    assert view.count() == 0
    for drive in (None, by):
        outs = []
        for t in ("b", None, empty, view):
            dst = (alloc(g), alloc(g))
            for d in dst:
                bits(d).fill_(SENTINEL)
            for which in (FRAME, INNER):
                if t == "b":
                    part_b(lib, g, bc, prm, dst, src, which, E, sbc, drive)
                else:
                    part_w(lib, g, bc, prm, dst, src, which, E, sbc, drive, t)
            torch.cuda.synchronize()
            outs.append(dst)
        for i, what in ((1, "NULL"), (2, "empty"), (3, "empty view")):
            for k in range(2):
                assert_bits(outs[i][k], outs[0][k], f"{what} table, lattice {k}")  # the whole allocation, padding included
    empty.close()
    view.close()


# ---- 3. write sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,E", [(24, 64, 1), (24, 64, 8), (33, 96, 5)])
@pytest.mark.parametrize("walls", [0, 1])
def test_each_part_alone_with_the_table_writes_exactly_its_rows(lib, R, C, E, walls):
    """NaN-poisoned destinations, ghost rows and row / plane padding included: each part (its dispatch and its wall pass)
    changes exactly its rows -- so FRAME leaves INNER's wall nodes unwritten and the reverse -- and every written double is
    the one of FRAME + INNER together; the wall nodes' are the table's, not the plain step's"""
    prm = params(FAST)
    bc = pylbm.Bc(row_lo=BB if walls else HALO, row_hi=HALO, col_lo=BB if walls else PER, col_hi=SP if walls else PER)
    g = geom(R, C, 1, C + 10)
    table = body_table(lib, R, C, (FIXED, 1e-3))  # built for the slab, not viewed
    assert bands_hold_nodes(table, E)
    src = (random_lattice(g, R), random_lattice(g, C))
    want, plain = [alloc(g), alloc(g)], [alloc(g), alloc(g)]
    for which in (FRAME, INNER):
        part_w(lib, g, bc, prm, want, src, which, E, table=table)
        part_b(lib, g, bc, prm, plain, src, which, E)
    torch.cuda.synchronize()
    wall_rows = sorted({n["r"] for n in table.nodes()})
    for k in range(2):
        differs = (bits(owned(want[k], g)) != bits(owned(plain[k], g))).any(dim=0).any(dim=1)
        assert differs.tolist() == [r in wall_rows for r in range(R)], (k, differs.tolist())
    for which, rows in ((FRAME, list(range(E)) + list(range(R - E, R))), (INNER, list(range(E, R - E)))):
        dst = (alloc(g), alloc(g))
        for d in dst:
            bits(d).fill_(SENTINEL)
        torch.cuda.synchronize()
        part_w(lib, g, bc, prm, dst, src, which, E, table=table)
        torch.cuda.synchronize()
        expect = torch.zeros(9 * g.plane_stride, dtype=torch.bool, device=dev())
        owned(expect, g)[:, rows] = True
        for k in range(2):
            changed = bits(dst[k]) != SENTINEL
            wrong = torch.nonzero(changed != expect)
            what = f"{'FRAME' if which == FRAME else 'INNER'} R={R} C={C} E={E} walls={walls} lattice {k}"
            assert wrong.numel() == 0, f"{what}: {wrong.shape[0]} doubles wrong, first flat index {int(wrong[0, 0])} " \
                                       f"({'missed' if bool(expect[int(wrong[0, 0])]) else 'over-written'})"
            diff = torch.nonzero(expect & (bits(dst[k]) != bits(want[k])))
            assert diff.numel() == 0, f"{what}: {diff.shape[0]} written doubles differ from the full call"
    table.close()


# ---- 4. chains and rings of slabs in one process -------------------------------------------------------------------------
def global_state(oracle, Rg, C, seed=0, w=W):
    """pre-collision f, g of the global box (dense SoA, ghost 0): a shear wave with noise, the scalar a Gaussian blob"""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(Rg, dtype=float), np.arange(C, dtype=float), indexing="ij")
    u = np.zeros((Rg, C, 2))
    u[..., 1] = 0.03 * np.sin(2 * np.pi * r / Rg)
    u += 0.005 * rng.standard_normal((Rg, C, 2))
    rho = 1 + 0.01 * rng.standard_normal((Rg, C))
    f = oracle.equilibrium(u, rho) * (1 + 0.005 * rng.standard_normal((Rg, C, 9)))
    s = 0.15 * min(Rg, C)
    conc = 1e-3 * np.exp(-((r - 0.4 * Rg) ** 2 + (c - 0.55 * C) ** 2) / (2 * s * s))
    gg = geom(Rg, C, 0)
    return gg, [to_lattice(a, gg) for a in (f, oracle.equilibrium(u + np.asarray(w), conc))]


def one_block(lib, gg, pre, gbc, prm, steps, table):
    """lbm_ade_collide + `steps` x lbm_ade_stream_collide_w on the global lattice: (post-collision state, after steps)"""
    post = [alloc(gg), alloc(gg)]
    lib.ade_collide(_ptr(post[0]), _ptr(post[1]), _ptr(pre[0]), _ptr(pre[1]), ct.byref(gg), ct.byref(gbc),
                    ct.byref(prm[0]), ct.byref(prm[1]), None, None, None, None)
    cur = [t.clone() for t in post]
    for _ in range(steps):
        cur = list(full_w(lib, gg, gbc, prm, *cur, table=table))
    torch.cuda.synchronize()
    return post, cur


class Chain:
    """slabs of the given heights of one global box, every slab in turn on this GPU: FRAME + INNER through
    lbm_ade_stream_collide_part_w with the slab's view of the global table, then the single-step halo of BOTH lattices by
    lbm_halo_pack -> lbm_halo_unpack (tests/test_gpu_ade_slabs.py's Chain with a table)"""

    def __init__(self, lib, gg, post, heights, closed, gbc, prm, table):
        self.lib, self.prm, self.closed, self.n = lib, prm, closed, len(heights)
        self.r0 = np.concatenate([[0], np.cumsum(heights)]).tolist()
        self.slabs = []
        for k in range(self.n):
            a, b = self.r0[k], self.r0[k + 1]
            cut = [cut_slab(p, gg, a, b, 0, closed) for p in post]
            g = cut[0][0]
            view = table.slab(a, b - a).finalize() if table is not None else None
            self.slabs.append(dict(g=g, bc=slab_bc(gbc, a, b, gg.R, closed), view=view,
                                   lat=[[cut[0][1], cut[1][1]], [alloc(g), alloc(g)]]))
        self.msg = lib.raw.lbm_halo_rows(1) * gg.C
        self.cur = 0

    def step(self, E):
        lib, cur = self.lib, self.cur
        for s in self.slabs:
            e = min(E, (s["g"].R - 1) // 2)
            for which in (FRAME, INNER):
                part_w(lib, s["g"], s["bc"], self.prm, s["lat"][cur ^ 1], s["lat"][cur], which, e, table=s["view"])
        n = self.n
        for k in range(n):
            if not self.closed and k == n - 1:
                continue
            a, b = self.slabs[k], self.slabs[(k + 1) % n]
            for j in range(2):
                down = torch.empty(self.msg, dtype=torch.float64, device=dev())
                up = torch.empty(self.msg, dtype=torch.float64, device=dev())
                lib.halo_pack(_ptr(down), _ptr(a["lat"][cur ^ 1][j]), ct.byref(a["g"]), 1, 1, None)
                lib.halo_pack(_ptr(up), _ptr(b["lat"][cur ^ 1][j]), ct.byref(b["g"]), 1, 0, None)
                lib.halo_unpack(_ptr(b["lat"][cur ^ 1][j]), _ptr(down), ct.byref(b["g"]), 1, 0, None)
                lib.halo_unpack(_ptr(a["lat"][cur ^ 1][j]), _ptr(up), ct.byref(a["g"]), 1, 1, None)
        self.cur ^= 1

    def gather(self, j):
        return torch.cat([owned(s["lat"][self.cur][j], s["g"]) for s in self.slabs], dim=1)

    def close(self):
        for s in self.slabs:
            if s["view"] is not None:
                s["view"].close()


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
@pytest.mark.parametrize("heights", [(24, 24), (16, 20, 12)])
def test_emulated_chain_with_the_body_equals_one_block(lib, oracle, form, closed, heights):
    """20 steps; on the closed ring (a periodic box) the column wall also crosses the wrap-around seam"""
    prm, gbc = params(form), (pylbm.Bc.periodic() if closed else GBC)
    E, steps = 4, 20
    gg, pre = global_state(oracle, RG, CG)
    table = body_table(lib, RG, CG, (FIXED, 1e-3))
    post, want = one_block(lib, gg, pre, gbc, prm, steps, table)
    _, plain = one_block(lib, gg, pre, gbc, prm, steps, None)
    assert not torch.equal(bits(want[0]), bits(plain[0])) and not torch.equal(bits(want[1]), bits(plain[1]))
    ch = Chain(lib, gg, post, heights, closed, gbc, prm, table)
    assert all(bands_hold_nodes(s["view"], min(E, (s["g"].R - 1) // 2)) for s in ch.slabs)
    for _ in range(steps):
        ch.step(E)
    torch.cuda.synchronize()
    for j in range(2):
        assert_bits(ch.gather(j), owned(want[j], gg), f"{len(heights)} slabs {heights} closed={closed} lattice {j}")
    ch.close()
    table.close()


# ---- 5. real rank processes (tests/ade_ring_rank.py, entry "walls") ------------------------------------------------------
@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
def test_ring_of_rank_processes_with_the_body_equals_one_block(lib, oracle, tmp_path, closed):
    """two ranks, lbm_ring_ade_step_w: the wall pass of the FRAME rows runs before the pack -- enqueued behind it, the
    neighbour would receive a wall node's un-fixed populations and its rows beside the seam would differ from one block"""
    n, R, C, steps, E, form = 2, 24, CG, 11, 4, FAST
    rule = (FIXED, 1e-3)
    prm, gbc = params(form), (pylbm.Bc.periodic() if closed else GBC)
    gg, pre = global_state(oracle, R * n, C, seed=2)
    table = body_table(lib, R * n, C, rule)
    for k in range(n):
        view = table.slab(k * R, R)
        assert bands_hold_nodes(view, E)
        view.close()
    _, want = one_block(lib, gg, pre, gbc, prm, steps, table)
    _, plain = one_block(lib, gg, pre, gbc, prm, steps, None)
    assert not torch.equal(bits(want[1]), bits(plain[1]))
    cfg = dict(R=R, C=C, steps=steps, edge_rows=E, closed=int(closed), form=form, bc=bytes(gbc).hex(), w=list(W),
               entry="walls", segments=body_segments(R * n), g_mode=rule[0], conc=rule[1])
    outs = run_ranks(lib, tmp_path, "ade_ring_rank.py", n, cfg,
                     dict(f0=owned(pre[0], gg).cpu().numpy(), g0=owned(pre[1], gg).cpu().numpy()), timeout=240)
    for j, key in enumerate(("f", "g")):
        got = np.concatenate([o[key] for o in outs], axis=1)
        ref = owned(want[j], gg).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"{n} ranks closed={closed}: {key} differs"
    assert [int(o["nodes"]) for o in outs] == [34, 34]
    table.close()


# ---- 6. a chain of one slab in this process ------------------------------------------------------------------------------
def test_ring_step_w_on_a_chain_of_one_slab_is_the_one_block_step(lib):
    """a ring of one rank, not closed: its rows keep their walls, nothing travels, both parts and both wall passes run on
    the caller's stream.  lbm_ring_ade_step_w with the body, a FIXED row, a FIXED profile column and buoyancy ==
    lbm_ade_stream_collide_w on the same block after 3 steps, bit for bit"""
    R, C, E, steps = 34, 64, 2, 3
    prm = params(FAST)
    by = pylbm.AdeBuoyancy((2e-2, -1e-2), 1.0, 0.5, (3.0, 9.0))  # random_lattice: C ~ 1.0 .. 1.05
    prof = torch.from_numpy(np.linspace(0.9, 1.1, R)).to(dev())
    sbc = pylbm.AdeScalarBC(row_lo=1.02, col_lo=(0.0, prof), col_hi=0.0)
    table = body_table(lib, R, C, (FIXED, 1.01))
    assert bands_hold_nodes(table, E)
    gg = geom(R, C, 0)
    want = [random_lattice(gg, 1), random_lattice(gg, 2)]
    plain = want
    cut = [cut_slab(t, gg, 0, R, 0) for t in want]  # ghost rows poisoned: beyond a wall nothing may read them
    sg = cut[0][0]
    lat = [[cut[0][1], cut[1][1]], [alloc(sg), alloc(sg)]]
    for _ in range(steps):
        want = full_w(lib, gg, GBC, prm, *want, sbc=sbc, by=by, table=table)
        plain = full_w(lib, gg, GBC, prm, *plain, sbc=sbc, by=by)
    ring, ident = ct.c_void_p(), (ct.c_ubyte * 128)()
    lib.ring_unique_id(ident)
    lib.ring_create(ct.byref(ring), ident, 0, 1, ct.byref(sg), 0)
    try:
        for k in range(steps):
            src, dst = lat[k & 1], lat[(k & 1) ^ 1]
            lib.ring_ade_step_w(ring, _ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), ct.byref(GBC),
                                ct.byref(prm[0]), ct.byref(prm[1]), ct.byref(sbc), ct.byref(by), table.h, E, None)
        torch.cuda.synchronize()
    finally:
        lib.ring_destroy(ring)
    for j in range(2):
        assert_bits(owned(lat[steps & 1][j], sg), owned(want[j], gg), f"lattice {j}")
        assert not torch.equal(bits(owned(want[j], gg)), bits(owned(plain[j], gg)))
    table.close()


# ---- 7. a sealed wall on a seam ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_a_sealed_wall_on_a_seam_seals(lib, oracle, form):
    """rows BOUNCE_BACK, fluid at rest, w = 0, two slabs of 12 rows; a full-width pair on the seam -- ROW_NEG on the last
    row of slab 0, ROW_POS on the first row of slab 1, NO_FLUX; the scalar starts above the pair only: after 200 steps C
    and g in slab 1 are exactly 0.0 at every node -- and are not without the table.  The mass above is conserved to
    rounding; the bound is test_a_sealed_wall_seals's, fixed before measuring: 200 steps x about 20 roundings per
    population and step x 2^-53 = 4.4e-13 if every rounding erred the same way, so 1e-12 relative"""
    heights, C, k, steps = (12, 12), 32, 11, 200
    Rg = sum(heights)
    prm, gbc = params(form, w=(0.0, 0.0)), pylbm.Bc(row_lo=BB, row_hi=BB)
    u = np.zeros((Rg, C, 2))
    conc = np.zeros((Rg, C))
    conc[:k + 1] = 1e-3 * (1.0 + 0.5 * np.cos(2 * np.pi * np.arange(C) / C))[None, :]
    gg = geom(Rg, C, 0)
    pre = [to_lattice(a, gg) for a in (oracle.equilibrium(u, np.ones((Rg, C))), oracle.equilibrium(u, conc))]
    post, _ = one_block(lib, gg, pre, gbc, prm, 0, None)
    table = pylbm.AdeInteriorWalls(lib, Rg, C).add(k, 0, 0, 1, C, ROW_NEG, ROW_NEG).add(k + 1, 0, 0, 1, C, ROW_POS, ROW_POS)
    table.finalize()
    out = {}
    for name, t in (("sealed", table), ("open", None)):
        ch = Chain(lib, gg, post, heights, False, gbc, prm, t)
        if t is not None:  # E = 2: the pair lies in the FRAME bands of both slabs
            assert [s["view"].count() for s in ch.slabs] == [C, C]
            assert {n["r"] for n in ch.slabs[0]["view"].nodes()} == {11} and {n["r"] for n in ch.slabs[1]["view"].nodes()} == {0}
        for _ in range(steps):
            ch.step(2)
        torch.cuda.synchronize()
        out[name] = ch.gather(1).cpu().numpy()  # [9, Rg, C]
        ch.close()
    sealed_C, open_C = out["sealed"].sum(axis=0), out["open"].sum(axis=0)
    assert np.all(out["sealed"][:, k + 1:] == 0.0) and np.all(sealed_C[k + 1:] == 0.0)
    assert np.all(sealed_C[:k + 1] > 0.0)
    assert np.all(open_C[k + 1:k + 4] > 0.0)
    assert abs(sealed_C.sum() - conc.sum()) <= 1e-12 * conc.sum()
    table.close()


# ---- 8. the driver -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fast", "ref"])
def test_slab_ring_ade_driver_emulated_chain_of_four_with_the_rectangle(form):
    line = last_json(run_driver("slab_ring_ade", "--emulate", 4, "--rows", 48, "--cols", 200, "--steps", 9, "--warmup", 2,
                                "--edge-rows", 8, "--walls", 1, "--rectangle", 1, "--form", form, "--check", 1, timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["slabs"] == 4
    assert line["interior_wall_nodes"] > 0
    per_slab = line["interior_wall_nodes_per_slab"]
    assert len(per_slab) == 4 and sum(per_slab) == line["interior_wall_nodes"]
    assert sum(1 for n in per_slab if n > 0) >= 2 and per_slab[2] > 0 and per_slab[3] > 0  # the body crosses the seam 2 | 3


def test_slab_ring_ade_driver_self_ring_with_the_rectangle(tmp_path):
    """one forked rank with walls: a chain of one slab through lbm_ring_ade_step_w == one block bit for bit"""
    line = last_json(run_driver("slab_ring_ade", "--spawn", 1, "--rows", 96, "--cols", 256, "--steps", 5, "--warmup", 1,
                                "--edge-rows", 16, "--walls", 1, "--rectangle", 1, "--check", 1, "--id-file", tmp_path / "id",
                                timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["n_gpus"] == 1 and line["interior_wall_nodes"] > 0


def test_slab_ring_ade_driver_refuses_the_rectangle_without_walls():
    r = run_driver("slab_ring_ade", "--emulate", 2, "--rows", 48, "--cols", 64, "--rectangle", 1, timeout=60, check=False)
    assert r.returncode != 0
    assert "--rectangle 1 needs --walls 1" in r.stderr
