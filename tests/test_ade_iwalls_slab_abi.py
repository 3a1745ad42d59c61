"""CPU suite, interior walls over row slabs: the slab view of a table (lbm_ade_iwalls_slab, pylbm.AdeInteriorWalls.slab)
and the host-side refusals of the entry points that take a slab-local table (lbm_ade_stream_collide_part_w).  The view
builder makes no device call, so everything here runs without a GPU: the nodes are read back through
lbm_ade_iwalls_count / lbm_ade_iwalls_node.

The body is the one of tests/test_gpu_ade_iwalls_slabs.py, on a global 48 x 64 lattice: a column wall at column 20
through all 48 rows (COL_NEG) and row walls at rows 5 and 29, columns 20..30 (ROW_NEG) -- 48 + 11 + 11 - 2 = 68 nodes."""
import ctypes as ct
import re

import pytest

import pylbm

NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_POS, ROW_NEG, COL_POS, COL_NEG = (pylbm.ADE_FACE_ROW_POS, pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_POS,
                                      pylbm.ADE_FACE_COL_NEG)
LBM_ERR_INVALID = -1
RG, C = 48, 64


@pytest.fixture(scope="module")
def lib():
    return pylbm.Lib()


def body(lib, g_mode=FIXED, conc=1e-3):
    """the test body, not finalized; FIXED so that the FIXED slots and conc of a node are carried too"""
    t = pylbm.AdeInteriorWalls(lib, RG, C)
    t.add(0, 20, 1, 0, RG, COL_NEG, COL_NEG, g_mode, conc)
    for r in (5, 29):
        t.add(r, 20, 0, 1, 11, ROW_NEG, ROW_NEG, g_mode, conc)
    return t


def _refused(lib, rc, name, msg):
    err = lib.raw.lbm_last_error_string().decode()
    assert rc == LBM_ERR_INVALID, (name, rc, err)
    assert err.startswith(name + ":") and re.search(msg, err), (name, err)


def test_symbols_are_declared_and_exported(lib):
    declared = set(pylbm.declared_symbols())
    for name in ("lbm_ade_iwalls_slab", "lbm_ade_stream_collide_part_w", "lbm_ring_ade_step_w"):
        assert name in declared and hasattr(lib.raw, name), name
    assert "lbm_ring_ade_collide_w" not in declared  # collide-only applies no wall rule: lbm_ring_ade_collide_b serves


def test_the_body_and_its_three_views_hold_the_counted_nodes(lib):
    t = body(lib)
    assert t.count() == 68
    for row0 in (0, 24, 12):
        v = t.slab(row0, 24)
        assert v.count() == 34, (row0, v.count())
        assert (v.R, v.C) == (24, C)
        v.close()
    assert t.count() == 68  # the parent is not modified
    t.close()


@pytest.mark.parametrize("row0,R", [(0, 24), (24, 24), (12, 24), (0, 48), (47, 1), (5, 1), (6, 23)])
def test_every_view_node_is_the_parents_node_with_the_row_shifted(lib, row0, R):
    t = body(lib)
    want = [dict(n, r=n["r"] - row0) for n in t.nodes() if row0 <= n["r"] < row0 + R]
    v = t.slab(row0, R)
    got = v.nodes()
    assert got == want  # field for field (f, g, FIXED slots, conc), in the parent's order
    assert got == sorted(got, key=lambda n: (n["r"], n["c"]))
    # a corner node of the body carries both facings and the FIXED slots of both segments
    if row0 <= 5 < row0 + R:
        corner = [n for n in got if (n["r"], n["c"]) == (5 - row0, 20)][0]
        assert corner["f_slots"] == COL_NEG | ROW_NEG and corner["g_fixed_slots"] == COL_NEG | ROW_NEG
        assert corner["conc"] == 1e-3
    v.close()
    t.close()


@pytest.mark.parametrize("heights", [(24, 24), (16, 20, 12), (1, 47)])
def test_views_that_tile_the_parent_partition_its_nodes(lib, heights):
    t = body(lib, NO_FLUX, 0.0)
    assert sum(heights) == RG
    row0, joined = 0, []
    for R in heights:
        v = t.slab(row0, R)
        joined += [dict(n, r=n["r"] + row0) for n in v.nodes()]
        v.close()
        row0 += R
    assert joined == t.nodes()
    t.close()


def test_a_view_is_an_ordinary_table_of_its_own(lib):
    t = body(lib)
    v = t.slab(24, 24)   # global rows 24..47: the column wall and the row wall of global row 29 = local row 5
    t.close()            # the view owns its nodes
    assert v.count() == 34
    v.add(10, 40, 0, 1, 3, ROW_POS, ROW_POS)   # further nodes, in the view's coordinates
    assert v.count() == 37
    v.add(5, 25, 0, 1, 1, 0, ROW_NEG, FIXED, 1e-3)  # the same rule on an inherited node merges
    assert v.count() == 37
    # the clash rules hold against inherited nodes: another mode on a g slot, another FIXED conc
    rc = lib.raw.lbm_ade_iwalls_add(v.h, 5, 25, 0, 1, 1, ct.c_uint(0), ct.c_uint(ROW_NEG), NO_FLUX, ct.c_double(0.0))
    _refused(lib, rc, "lbm_ade_iwalls_add", r"node \(5, 25\): g slot \d named with two modes")
    rc = lib.raw.lbm_ade_iwalls_add(v.h, 7, 20, 0, 1, 1, ct.c_uint(0), ct.c_uint(COL_POS), FIXED, ct.c_double(2e-3))
    _refused(lib, rc, "lbm_ade_iwalls_add", r"node \(7, 20\): FIXED conc=0.002 differs from the conc=0.001")
    # the view is 24 x 64: row 24 is outside it
    rc = lib.raw.lbm_ade_iwalls_add(v.h, 24, 0, 0, 1, 1, ct.c_uint(ROW_POS), ct.c_uint(0), NO_FLUX, ct.c_double(0.0))
    _refused(lib, rc, "lbm_ade_iwalls_add", r"node \(24, 0\) outside the 24 x 64 lattice")
    assert v.count() == 37
    v.close()


def test_a_view_without_nodes_is_an_empty_table(lib):
    t = pylbm.AdeInteriorWalls(lib, RG, C).add(5, 20, 0, 1, 11, ROW_NEG, ROW_NEG)
    v = t.slab(6, 42)
    assert v.count() == 0
    v.finalize()  # an empty finalize makes no device call
    v.close()
    t.close()


def test_slab_refuses_bad_arguments_on_the_host(lib):
    t = body(lib)
    h, name = ct.c_void_p(), "lbm_ade_iwalls_slab"
    _refused(lib, lib.raw.lbm_ade_iwalls_slab(None, t.h, 0, 24), name, "NULL argument")
    _refused(lib, lib.raw.lbm_ade_iwalls_slab(ct.byref(h), None, 0, 24), name, "NULL argument")
    _refused(lib, lib.raw.lbm_ade_iwalls_slab(ct.byref(h), t.h, -1, 24), name, r"row0=-1 must not be negative")
    _refused(lib, lib.raw.lbm_ade_iwalls_slab(ct.byref(h), t.h, 0, 0), name, r"R=0 must be at least 1")
    _refused(lib, lib.raw.lbm_ade_iwalls_slab(ct.byref(h), t.h, 0, -5), name, r"R=-5 must be at least 1")
    _refused(lib, lib.raw.lbm_ade_iwalls_slab(ct.byref(h), t.h, 25, 24), name, r"rows \[25, 49\) beyond the 48 rows")
    _refused(lib, lib.raw.lbm_ade_iwalls_slab(ct.byref(h), t.h, 48, 1), name, r"rows \[48, 49\) beyond the 48 rows")
    _refused(lib, lib.raw.lbm_ade_iwalls_slab(ct.byref(h), t.h, 2 ** 31 - 1, 2 ** 31 - 1), name, r"beyond the 48 rows")
    assert not h
    with pytest.raises(pylbm.LbmError, match="lbm_ade_iwalls_slab"):
        t.slab(40, 9)
    t.close()


def _part_w(lib, g, table, part=pylbm.ADE_PART_FRAME, E=2):
    fl, sc, bc = pylbm.BgkParams(1.2, 0), pylbm.AdeParams(1.7, (0.0, 0.0)), pylbm.Bc()
    return lib.raw.lbm_ade_stream_collide_part_w(None, None, None, None, ct.byref(g), ct.byref(bc), ct.byref(fl), ct.byref(sc),
                                                 None, None, table, part, E, None, None, None, None)


def test_part_w_refuses_an_unfinalized_or_misfit_table_on_the_host(lib):
    name = "lbm_ade_stream_collide_part_w"
    t = body(lib)
    v = t.slab(0, 24)
    _refused(lib, _part_w(lib, pylbm.Geom(24, C, 0), v.h), name, "interior walls: the table is not finalized")
    empty = pylbm.AdeInteriorWalls(lib, 24, C).finalize()
    _refused(lib, _part_w(lib, pylbm.Geom(48, C, 0), empty.h), name,
             r"interior walls: the table is for a 24 x 64 lattice, the call for 48 x 64")
    # a fitting (empty) table and NULL pass the table check: the call reaches the NULL-lattice refusal
    _refused(lib, _part_w(lib, pylbm.Geom(24, C, 0), empty.h), name, "NULL lattice")
    _refused(lib, _part_w(lib, pylbm.Geom(24, C, 0), None), name, "NULL lattice")
    for x in (empty, v, t):
        x.close()
