"""CPU suite, open boundaries of the fluid + scalar step over row slabs: lbm_ade_open_slab (the slab view of an open table),
its accessors, and the host refusals of the entry points that take a view (lbm_ade_stream_collide_part_o) or refuse one
(lbm_ade_stream_collide_o, lbm_ade_collide_o).  Host only: no view is finalized here -- only a non-empty finalize touches the
device -- and every refusal tested is made before any device call.

The expected view is restated here from the parent's resolved nodes: node i of the view is node i0 + i of the parent at
r - row0; a g source keeps its column and takes, of its global row modulo the parent's rows, the slab-local row in [-1, R]
nearest to the slot's plain pull row; a source with no such row is unreachable and reported at the plain pull source."""
import ctypes as ct
import re

import pytest

import pylbm

BB, SP, PER, HALO = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_PERIODIC, pylbm.EDGE_HALO
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
O_BB, O_SROW, O_SCOL, O_ABB, O_ABBX = (pylbm.ADE_OPEN_BOUNCE_BACK, pylbm.ADE_OPEN_SPECULAR_ROW, pylbm.ADE_OPEN_SPECULAR_COL,
                                       pylbm.ADE_OPEN_ABB, pylbm.ADE_OPEN_ABB_EXTRAPOLATED)
LBM_ERR_INVALID = -1
CX = [0, 1, 0, -1, 0, 1, -1, -1, 1]
CY = [0, 0, 1, 0, -1, 1, 1, -1, -1]
ALL = 0xFF
RG, CG = 48, 64
VIEWS = ((0, 24), (24, 48), (12, 36))
SYMBOLS = ["lbm_ade_open_slab", "lbm_ade_open_unreachable", "lbm_ade_stream_collide_part_o", "lbm_ring_ade_collide_o",
           "lbm_ring_ade_step_o", "lbm_ade_part_launches"]


@pytest.fixture(scope="module")
def lib():
    return pylbm.Lib()


def _refused(lib, rc, name, msg):
    err = lib.raw.lbm_last_error_string().decode()
    assert rc == LBM_ERR_INVALID, (name, rc, err)
    assert err.startswith(name + ":") and re.search(msg, err), (name, err)


def channel(lib, R=RG, C=CG):
    return pylbm.AdeOpenBoundary(lib, R, C).channel(0.03, 1e-3, 10)


def every_rule(lib, R=RG, C=CG):
    """every kind of f rule, both g rules and two copies, on nodes of several rows; the extrapolation neighbours lie in
    the node's own row"""
    t = pylbm.AdeOpenBoundary(lib, R, C)
    t.add_f(2, 3, 1, 0, R - 4, 0x0F, O_BB)
    t.add_f(0, 10, 0, 1, 8, 0x91, O_SROW)
    t.add_f(5, C - 1, 1, 0, 30, 0xC8, O_SCOL)
    t.add_f(1, 0, 1, 0, R - 2, ALL, O_ABB, (0.0, 0.02))
    t.add_f(0, C - 2, 1, 0, R, ALL, O_ABBX, (1.5, -0.5), (0, -1))
    t.add_g(3, 7, 1, 1, 20, 0x33, NO_FLUX)
    t.add_g(1, 0, 1, 0, R - 2, ALL, FIXED, 1e-3)
    t.add_g_copy(0, 0, 0, 1, C, (1, 0))
    t.add_g_copy(20, 30, 1, 0, 10, (0, -1))
    return t


def expected_view(parent_nodes, Rg, C, row0, R):
    out = []
    for n in parent_nodes:
        if not row0 <= n["r"] < row0 + R:
            continue
        r = n["r"] - row0
        src, unreachable = [], 0
        for q, (sr, sc) in enumerate(n["g_src"]):
            pull = r - CX[q]
            cands = [x for x in (sr - row0 - Rg, sr - row0, sr - row0 + Rg) if -1 <= x <= R]
            if cands:
                src.append((min(cands, key=lambda x: abs(x - pull)), sc))
            else:
                unreachable |= 1 << q
                src.append((pull, (n["c"] - CY[q]) % C))
        out.append(dict(r=r, c=n["c"], f_rule=n["f_rule"], g_rule=n["g_rule"], g_src=src, unreachable=unreachable))
    return out


def test_symbols_are_declared_and_exported(lib):
    declared = set(pylbm.declared_symbols())
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib.raw, name), name


@pytest.mark.parametrize("make", [channel, every_rule], ids=["channel", "every_rule_kind"])
def test_views_partition_the_parent(lib, make):
    table = make(lib)
    parent = table.nodes()
    assert all(n["unreachable"] == 0 for n in parent)
    counts = {}
    ghost_rows = set()
    for r0, r1 in VIEWS:
        view = table.slab(r0, r1 - r0)
        got = view.nodes()
        counts[r0, r1] = view.count()
        assert view.carry_len() == 2 * view.count() == 2 * len(got)
        assert got == expected_view(parent, RG, CG, r0, r1 - r0), (r0, r1)
        assert [(n["r"], n["c"]) for n in got] == sorted((n["r"], n["c"]) for n in got)  # the parent's order is (r, c) order
        ghost_rows |= {sr for n in got for sr, _ in n["g_src"] if sr in (-1, r1 - r0)}
        for i in (0, view.count() - 1):  # the C accessor agrees with the mask the binding reports
            assert lib.raw.lbm_ade_open_unreachable(view.h, i) == got[i]["unreachable"]
        view.close()
    assert counts[0, 24] + counts[24, 48] == table.count() == len(parent)
    assert counts[12, 36] == sum(1 for n in parent if 12 <= n["r"] < 36) > 0
    assert ghost_rows == {-1, 24}  # sources in both ghost rows are reported there
    table.close()


def test_the_channel_view_of_the_last_slab_marks_the_wrap_around_readers(lib):
    """the lid's copy g*(0, .) = g*(1, .): the parent lists the readers in global row R_g - 1, whose redirected slots (c_x =
    -1) pull global row 1 -- two rows beyond the slab's last row: unreachable, reported at the plain pull source, row R"""
    table = channel(lib)
    view = table.slab(24, 24)
    last = [n for n in view.nodes() if n["r"] == 23]
    assert len(last) == CG
    for n in last:
        assert n["unreachable"] == (1 << 3) | (1 << 6) | (1 << 7), n
        for q in (3, 6, 7):
            assert n["g_src"][q] == (24, (n["c"] - CY[q]) % CG)
    assert all(n["unreachable"] == 0 for n in view.nodes() if n["r"] < 23)
    top = table.slab(0, 24)
    assert all(n["unreachable"] == 0 for n in top.nodes())
    assert all(n["g_src"][0] == (1, n["c"]) for n in top.nodes() if n["r"] == 0)  # the lid's copy stays inside slab 0
    for t in (view, top, table):
        t.close()


def test_a_whole_box_view_reports_the_wrapped_sources_in_the_ghost_rows(lib):
    table = channel(lib)
    view = table.slab(0, RG)
    got = view.nodes()
    assert len(got) == table.count() and all(n["unreachable"] == 0 for n in got)
    n0 = next(n for n in got if n["r"] == 0 and n["c"] == 5)
    assert n0["g_src"][1] == (-1, 5)  # global row R_g - 1, which wrap_row wraps on a ghost = 0 geometry
    last = next(n for n in got if n["r"] == RG - 1 and n["c"] == 5)
    assert last["g_src"][3] == (1, 5)  # the lid's copy, reachable in the whole box
    view.close()
    table.close()


def test_an_empty_finalized_parent_and_an_unfinalized_one_give_the_same_view(lib):
    a = pylbm.AdeOpenBoundary(lib, RG, CG).finalize()  # empty: no device call
    b = pylbm.AdeOpenBoundary(lib, RG, CG)
    va, vb = a.slab(12, 24), b.slab(12, 24)
    assert va.count() == vb.count() == 0 and va.carry_len() == 0 and va.nodes() == vb.nodes() == []
    va.finalize()  # an empty view makes no device call either
    for t in (va, vb, a, b):
        t.close()


def test_a_copy_from_one_row_across_a_seam_reads_the_ghost_row(lib):
    table = pylbm.AdeOpenBoundary(lib, RG, CG).add_g_copy(24, 5, 0, 1, 10, (-1, 0))
    lower = table.slab(24, 24)
    own = {n["c"]: n for n in lower.nodes() if n["r"] == 0}
    for c in range(5, 15):
        assert own[c]["g_src"][0] == (-1, c) and own[c]["unreachable"] == 0
    upper = table.slab(0, 24)
    for n in upper.nodes():  # the readers above the seam pull the copied row from their own last row
        assert n["r"] == 23 and n["unreachable"] == 0
        if 6 <= n["c"] <= 13:  # all three sources below are copied nodes
            assert all(sr in (22, 23) for sr, _ in n["g_src"])
    assert upper.count() > 0
    for t in (lower, upper, table):
        t.close()


@pytest.mark.parametrize("chained", [False, True], ids=["two_rows_away", "second_copy_after_first"])
def test_a_source_two_rows_across_a_seam_is_marked_unreachable(lib, chained):
    table = pylbm.AdeOpenBoundary(lib, RG, CG)
    if chained:  # row 23 <- row 22, then row 24 <- row 23: the second copy sees the first and ends two rows away
        table.add_g_copy(23, 5, 0, 1, 10, (-1, 0)).add_g_copy(24, 5, 0, 1, 10, (-1, 0))
    else:
        table.add_g_copy(24, 5, 0, 1, 10, (-2, 0))
    assert next(n for n in table.nodes() if (n["r"], n["c"]) == (24, 7))["g_src"][0] == (22, 7)
    view = table.slab(24, 24)
    n = next(n for n in view.nodes() if (n["r"], n["c"]) == (0, 7))
    assert n["unreachable"] & 1 and n["g_src"][0] == (0, 7)  # marked, and pointed at the plain source: the node itself
    reader = next(n for n in view.nodes() if (n["r"], n["c"]) == (1, 7))
    assert reader["unreachable"] == (1 << 1) | (1 << 5) | (1 << 8) and reader["g_src"][1] == (0, 7)
    view.close()
    table.close()


def test_an_extrapolation_neighbour_outside_the_view_is_refused_and_the_node_named(lib):
    table = pylbm.AdeOpenBoundary(lib, RG, CG).add_f(24, 5, 0, 1, 3, ALL, O_ABBX, (1.5, -0.5), (-1, 0))
    h = ct.c_void_p()
    _refused(lib, lib.raw.lbm_ade_open_slab(ct.byref(h), table.h, 24, 24), "lbm_ade_open_slab",
             r"node \(24, 5\), f slot 1: its extrapolation neighbour \(23, 5\) lies outside rows \[24, 48\)")
    assert not h
    view = table.slab(12, 24)  # both rows inside: fine
    assert view.count() == 6
    view.close()
    table.close()


def test_bad_arguments_are_refused(lib):
    table = channel(lib)
    h = ct.c_void_p()
    slab = lib.raw.lbm_ade_open_slab
    _refused(lib, slab(None, table.h, 0, 24), "lbm_ade_open_slab", "NULL argument")
    _refused(lib, slab(ct.byref(h), None, 0, 24), "lbm_ade_open_slab", "NULL argument")
    _refused(lib, slab(ct.byref(h), table.h, -1, 24), "lbm_ade_open_slab", "row0=-1 must not be negative")
    _refused(lib, slab(ct.byref(h), table.h, 0, 0), "lbm_ade_open_slab", "R=0 must be at least 1")
    _refused(lib, slab(ct.byref(h), table.h, 25, 24), "lbm_ade_open_slab", r"rows \[25, 49\) beyond the 48 rows of the table")
    assert not h
    view = table.slab(0, 24)
    _refused(lib, slab(ct.byref(h), view.h, 0, 12), "lbm_ade_open_slab", "itself a slab view")
    assert lib.raw.lbm_ade_open_unreachable(None, 0) == 0 and lib.raw.lbm_ade_open_unreachable(view.h, -1) == 0
    view.close()
    table.close()


def test_a_view_takes_no_segments(lib):
    table = channel(lib)
    view = table.slab(0, 24)
    n = view.count()
    msg = "slab view .*it takes no segments"
    _refused(lib, lib.raw.lbm_ade_open_add_f(view.h, 2, 2, 0, 1, 1, ct.c_uint(1), O_BB, ct.c_double(0), ct.c_double(0), 0, 0),
             "lbm_ade_open_add_f", msg)
    _refused(lib, lib.raw.lbm_ade_open_add_g(view.h, 2, 2, 0, 1, 1, ct.c_uint(1), NO_FLUX, ct.c_double(0)), "lbm_ade_open_add_g", msg)
    _refused(lib, lib.raw.lbm_ade_open_add_g_copy(view.h, 2, 2, 0, 1, 1, 1, 0), "lbm_ade_open_add_g_copy", msg)
    _refused(lib, lib.raw.lbm_ade_open_add_channel(view.h, ct.c_double(0.03), ct.c_double(1e-3), 5), "lbm_ade_open_add_channel", msg)
    assert view.count() == n
    view.close()
    table.close()


def test_each_kind_of_table_is_refused_by_the_other_kind_of_entry_point(lib):
    """the kind is checked before the finalized state, and both before any device call"""
    table = channel(lib)
    view = table.slab(0, 24)
    fl, sc = pylbm.BgkParams(1.2, 0), pylbm.AdeParams(1.7, (3e-3, 3e-3))
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO)
    g1, gg = pylbm.Geom(24, CG, 1), pylbm.Geom(RG, CG, 0)
    raw = lib.raw
    rc = raw.lbm_ade_stream_collide_part_o(None, None, None, None, ct.byref(g1), ct.byref(bc), ct.byref(fl), ct.byref(sc), None,
                                           None, None, table.h, None, None, pylbm.ADE_PART_FRAME, 2, None, None, None, None)
    _refused(lib, rc, "lbm_ade_stream_collide_part_o", "not a slab view.*lbm_ade_open_slab")
    gbc = pylbm.Bc(row_hi=BB)
    rc = raw.lbm_ade_stream_collide_o(None, None, None, None, ct.byref(gg), ct.byref(gbc), ct.byref(fl), ct.byref(sc), None, None,
                                      None, view.h, None, None, 0, RG, None, None, None, None)
    _refused(lib, rc, "lbm_ade_stream_collide_o", "is a slab view.*lbm_ade_stream_collide_part_o")
    rc = raw.lbm_ade_collide_o(None, None, None, None, ct.byref(gg), ct.byref(gbc), ct.byref(fl), ct.byref(sc), None, None, view.h,
                               None, None, None, None, None)
    _refused(lib, rc, "lbm_ade_collide_o", "is a slab view.*lbm_ring_ade_collide_o")
    # the right kind, not finalized: the next refusal
    rc = raw.lbm_ade_stream_collide_part_o(None, None, None, None, ct.byref(g1), ct.byref(bc), ct.byref(fl), ct.byref(sc), None,
                                           None, None, view.h, None, None, pylbm.ADE_PART_FRAME, 2, None, None, None, None)
    _refused(lib, rc, "lbm_ade_stream_collide_part_o", "the table is not finalized")
    # a NULL view is lbm_ade_stream_collide_part_w itself: past validation to the NULL lattices
    rc = raw.lbm_ade_stream_collide_part_o(None, None, None, None, ct.byref(g1), ct.byref(bc), ct.byref(fl), ct.byref(sc), None,
                                           None, None, None, None, None, pylbm.ADE_PART_FRAME, 2, None, None, None, None)
    _refused(lib, rc, "lbm_ade_stream_collide_part_o", "NULL lattice")
    assert raw.lbm_ade_part_launches() == 0  # nothing was enqueued by any of this
    view.close()
    table.close()
