"""CPU suite, interior walls of the fluid + scalar solver (lbm_ade_iwalls, lbm_ade_stream_collide_w,
lbm_ade_solver_set_walls; pylbm.AdeInteriorWalls): exported and declared, plain C99, every refusal of the table builder
and of the calls that take a table made on the host with LBM_ERR_INVALID and a message before any device call, the merged
table of the reference's rectangle (test/rectangle_sedimentation_test.cpp:184-196, :220-232) and of a closed box, and a
supported call past validation to the NULL-lattice refusal (no GPU needed: only a non-empty finalize touches the device)."""
import ctypes as ct
import math
import os
import re
import subprocess

import pytest

import pylbm

SYMBOLS = ["lbm_ade_iwalls_create", "lbm_ade_iwalls_add", "lbm_ade_iwalls_count", "lbm_ade_iwalls_node",
           "lbm_ade_iwalls_finalize", "lbm_ade_iwalls_destroy", "lbm_ade_stream_collide_w", "lbm_ade_solver_set_walls"]
BB, SP, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_PERIODIC
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_POS, ROW_NEG, COL_POS, COL_NEG = (pylbm.ADE_FACE_ROW_POS, pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_POS,
                                      pylbm.ADE_FACE_COL_NEG)
LBM_ERR_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CX = [0, 1, 0, -1, 0, 1, -1, -1, 1]  # icx / icy of d2q9.hpp: icx is the row component
CY = [0, 0, 1, 0, -1, 1, 1, -1, -1]


@pytest.fixture(scope="module")
def lib():
    return pylbm.Lib()


def mask(*slots):
    return sum(1 << (s - 1) for s in slots)


def test_symbols_are_declared_and_exported_and_the_masks_follow_the_lattice(lib):
    declared = set(pylbm.declared_symbols())
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib.raw, name), name
    assert lib.raw.lbm_abi_version() == 1
    assert (ROW_POS, ROW_NEG, COL_POS, COL_NEG) == (0x91, 0x64, 0x32, 0xC8)
    # a facing names the populations that arrive from the wall's side: c_s points to the fluid
    assert ROW_POS == mask(*[s for s in range(1, 9) if CX[s] == 1]) and ROW_NEG == mask(*[s for s in range(1, 9) if CX[s] == -1])
    assert COL_POS == mask(*[s for s in range(1, 9) if CY[s] == 1]) and COL_NEG == mask(*[s for s in range(1, 9) if CY[s] == -1])
    txt = open(os.path.join(ROOT, "include", "lbm_hip.h")).read()
    for name, v in (("ROW_POS", ROW_POS), ("ROW_NEG", ROW_NEG), ("COL_POS", COL_POS), ("COL_NEG", COL_NEG)):
        assert re.search(rf"#define LBM_ADE_FACE_{name} 0x{v:02X}u?\b", txt), name


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "iwalls_c99.c"
    src.write_text('#include "lbm_hip.h"\n'
                   'int main(void){ lbm_ade_iwalls* t = 0; int r, c; unsigned f, g, gf; double conc;\n'
                   '  if (lbm_ade_solver_set_walls(0, 0) != LBM_ERR_INVALID) return 2;\n'
                   '  if (lbm_ade_iwalls_create(&t, 24, 32) != LBM_OK) return 3;\n'
                   '  if (lbm_ade_iwalls_add(t, -7, 10, 0, 1, 7, LBM_ADE_FACE_ROW_NEG, LBM_ADE_FACE_ROW_NEG,\n'
                   '                         LBM_ADE_SCALAR_FIXED, 0.0) != LBM_OK) return 4;\n'
                   '  if (lbm_ade_iwalls_count(t) != 7) return 5;\n'
                   '  if (lbm_ade_iwalls_node(t, 0, &r, &c, &f, &g, &gf, &conc) != LBM_OK || r != 17 || c != 10) return 6;\n'
                   '  if (f != 0x64u || g != 0x64u || gf != 0x64u || conc != 0.0) return 7;\n'
                   '  if (lbm_ade_stream_collide_w(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, t, 0, 0, 0, 0, 0, 0) != LBM_ERR_INVALID) return 8;\n'
                   '  if (lbm_ade_iwalls_destroy(t) != LBM_OK) return 9;\n'
                   '  return lbm_abi_version() == 1 ? 0 : 1; }\n')
    libdir = os.path.join(ROOT, "lattice-boltzmann-method_amd", "lib")
    exe = tmp_path / "iwalls_c99"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-L", libdir, "-llbm_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


# ---- the table builder's refusals ---------------------------------------------------------------------------------------
def _refused(lib, rc, name, msg):
    err = lib.raw.lbm_last_error_string().decode()
    assert rc == LBM_ERR_INVALID, (name, rc, err)
    assert err.startswith(name + ":") and re.search(msg, err), (name, err)


def _add(lib, t, r0, c0, dr, dc, n, f_slots, g_slots, g_mode=NO_FLUX, conc=0.0):
    h = t.h if isinstance(t, pylbm.AdeInteriorWalls) else t
    return lib.raw.lbm_ade_iwalls_add(h, r0, c0, dr, dc, n, ct.c_uint(f_slots), ct.c_uint(g_slots), g_mode, ct.c_double(conc))


def test_create_refuses_a_null_out_and_a_non_positive_size(lib):
    _refused(lib, lib.raw.lbm_ade_iwalls_create(None, 8, 8), "lbm_ade_iwalls_create", "NULL argument")
    h = ct.c_void_p()
    for R, C in ((0, 8), (8, 0), (-3, 8)):
        _refused(lib, lib.raw.lbm_ade_iwalls_create(ct.byref(h), R, C), "lbm_ade_iwalls_create", f"R={R} C={C} must be positive")
        assert not h


def test_a_null_table_is_refused_by_every_entry_that_needs_one(lib):
    _refused(lib, _add(lib, None, 0, 0, 0, 1, 1, ROW_POS, 0), "lbm_ade_iwalls_add", "NULL table")
    _refused(lib, lib.raw.lbm_ade_iwalls_finalize(None), "lbm_ade_iwalls_finalize", "NULL table")
    _refused(lib, lib.raw.lbm_ade_iwalls_node(None, 0, None, None, None, None, None, None), "lbm_ade_iwalls_node", "NULL table")
    assert lib.raw.lbm_ade_iwalls_count(None) == 0
    assert lib.raw.lbm_ade_iwalls_destroy(None) == 0
    _refused(lib, lib.raw.lbm_ade_solver_set_walls(None, None), "lbm_ade_solver_set_walls", "NULL solver")


ADD_REFUSALS = [
    ((24, 0, 0, 1, 1, ROW_POS, 0), r"node \(24, 0\) outside the 24 x 32 lattice"),
    ((0, 32, 1, 0, 1, ROW_POS, 0), r"node \(0, 32\) outside the 24 x 32 lattice"),
    ((-25, 0, 0, 1, 1, ROW_POS, 0), r"node \(-1, 0\) outside the 24 x 32 lattice"),
    ((20, 0, 1, 0, 5, COL_POS, 0), r"node \(24, 0\) outside the 24 x 32 lattice"),     # the far end leaves
    ((3, 30, 0, 1, 3, ROW_POS, 0), r"node \(3, 32\) outside the 24 x 32 lattice"),
    ((3, 1, 0, -1, 3, ROW_POS, 0), r"node \(3, -1\) outside the 24 x 32 lattice"),
    ((3, 3, 0, 1, 2, 0x100, 0), r"f_slots=0x100 g_slots=0x0 above 0xFF"),
    ((3, 3, 0, 1, 2, 0, 0x1FF), r"f_slots=0x0 g_slots=0x1ff above 0xFF"),
    ((3, 3, 0, 1, 2, 0, 0), r"f_slots and g_slots are both 0"),
    ((3, 3, 0, 1, 2, ROW_POS, ROW_POS, 2), r"g_mode=2 \(LBM_ADE_SCALAR_NO_FLUX or LBM_ADE_SCALAR_FIXED\)"),
    ((3, 3, 0, 1, 2, ROW_POS, ROW_POS, -1), r"g_mode=-1"),
    ((3, 3, 0, 1, 2, ROW_POS, ROW_POS, FIXED, math.nan), r"conc=nan must be finite"),
    ((3, 3, 0, 1, 2, ROW_POS, ROW_POS, FIXED, math.inf), r"conc=inf must be finite"),
    ((3, 3, 0, 1, 2, ROW_POS, ROW_POS, NO_FLUX, -math.inf), r"conc=-inf must be finite"),
    ((3, 3, 0, 1, 0, ROW_POS, 0), r"n=0 must be at least 1"),
    ((3, 3, 0, 0, 2, ROW_POS, 0), r"step \(dr, dc\)=\(0, 0\)"),
    ((3, 3, 2, 0, 2, ROW_POS, 0), r"step \(dr, dc\)=\(2, 0\)"),
]


@pytest.mark.parametrize("case", range(len(ADD_REFUSALS)))
def test_add_refuses_on_the_host_and_adds_nothing(lib, case):
    args, msg = ADD_REFUSALS[case]
    t = pylbm.AdeInteriorWalls(lib, 24, 32)
    _refused(lib, _add(lib, t, *args), "lbm_ade_iwalls_add", msg)
    assert t.count() == 0
    t.close()


def test_a_slot_with_two_modes_and_a_node_with_two_concentrations_are_refused_naming_the_node(lib):
    t = pylbm.AdeInteriorWalls(lib, 24, 32)
    t.add(5, 4, 0, 1, 6, ROW_NEG, ROW_NEG, FIXED, 1e-3)
    before = t.nodes()
    # the crossing segment clashes at its third node: nothing of it is added
    _refused(lib, _add(lib, t, 3, 6, 1, 0, 5, 0, mask(7), NO_FLUX), "lbm_ade_iwalls_add",
             r"node \(5, 6\): g slot 7 named with two modes")
    _refused(lib, _add(lib, t, 3, 6, 1, 0, 5, COL_NEG, COL_NEG, FIXED, 2e-3), "lbm_ade_iwalls_add",
             r"node \(5, 6\): FIXED conc=0.002 differs from the conc=0.001")
    assert t.nodes() == before
    t.add(8, 4, 0, 1, 2, 0, mask(2), NO_FLUX)
    _refused(lib, _add(lib, t, 8, 5, 0, 1, 1, 0, mask(2, 5), FIXED, 0.0), "lbm_ade_iwalls_add",
             r"node \(8, 5\): g slot 2 named with two modes")
    # what merges: other slots of the same node in the other mode, the same conc again, f slots with any g mode
    t.add(3, 6, 1, 0, 5, COL_NEG, mask(4, 8), FIXED, 1e-3)
    t.add(5, 6, 0, 1, 1, ROW_POS, mask(1), NO_FLUX, 7.0)  # a NO_FLUX segment's conc is not the node's
    node = [n for n in t.nodes() if (n["r"], n["c"]) == (5, 6)][0]
    assert node == dict(r=5, c=6, f_slots=ROW_NEG | COL_NEG | ROW_POS, g_slots=ROW_NEG | mask(4, 8, 1),
                        g_fixed_slots=ROW_NEG | mask(4, 8), conc=1e-3)
    t.close()


def test_the_table_is_immutable_after_finalize_and_unusable_before(lib):
    fl, sc = pylbm.BgkParams(1.2, 0), pylbm.AdeParams(1.7, (3e-3, 3e-3))
    g = pylbm.Geom(24, 32, 0)

    def step(t, geom=g):
        return lib.raw.lbm_ade_stream_collide_w(None, None, None, None, ct.byref(geom), None, ct.byref(fl), ct.byref(sc),
                                                None, None, t.h if t is not None else None, 0, geom.R, None, None, None, None)

    t = pylbm.AdeInteriorWalls(lib, 24, 32)
    _refused(lib, step(t), "lbm_ade_stream_collide_w", "interior walls: the table is not finalized")
    t.finalize()  # empty: no device call
    _refused(lib, _add(lib, t, 3, 3, 0, 1, 2, ROW_POS, 0), "lbm_ade_iwalls_add", "the table is finalized")
    _refused(lib, lib.raw.lbm_ade_iwalls_finalize(t.h), "lbm_ade_iwalls_finalize", "finalized already")
    assert t.count() == 0 and t.nodes() == []
    _refused(lib, lib.raw.lbm_ade_iwalls_node(t.h, 0, None, None, None, None, None, None), "lbm_ade_iwalls_node",
             r"node 0 outside \[0, 0\)")
    # a table built for another lattice
    for geom in (pylbm.Geom(24, 34, 0), pylbm.Geom(26, 32, 0)):
        _refused(lib, step(t, geom), "lbm_ade_stream_collide_w",
                 rf"interior walls: the table is for a 24 x 32 lattice, the call for {geom.R} x {geom.C}")
    # everything the passive call refuses comes first or beside it, still on the host
    _refused(lib, step(t, pylbm.Geom(24, 31, 0)), "lbm_ade_stream_collide_w", "C=31 must be even")
    t.close()


def test_a_supported_call_passes_validation_without_a_gpu(lib):
    """NULL, and an empty finalized table, with and without walls, FIXED edges and buoyancy, in every form: up to the
    existing NULL-lattice refusal"""
    g = pylbm.Geom(24, 32, 0)
    empty = pylbm.AdeInteriorWalls(lib, 24, 32).finalize()
    wall_bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=SP, col_hi=BB)
    for t in (None, empty):
        for bc, sbc in ((None, None), (wall_bc, None), (wall_bc, pylbm.AdeScalarBC(row_lo=1e-3, col_hi=0.0))):
            for by in (None, pylbm.AdeBuoyancy((1e-4, -2e-4), 0.5)):
                for form in (pylbm.FORM_DEFAULT, pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED):
                    fl, sc = pylbm.BgkParams(1.2, 0, form=form), pylbm.AdeParams(1.7, (3e-3, 3e-3), form=form)
                    rc = lib.raw.lbm_ade_stream_collide_w(None, None, None, None, ct.byref(g), ct.byref(bc) if bc else None,
                                                          ct.byref(fl), ct.byref(sc), ct.byref(sbc) if sbc else None,
                                                          ct.byref(by) if by else None, t.h if t else None, 0, g.R, None,
                                                          None, None, None)
                    _refused(lib, rc, "lbm_ade_stream_collide_w", "NULL lattice")
    empty.close()


# ---- merged tables ------------------------------------------------------------------------------------------------------
def reference_rectangle(lib, R, C, r_top, c_first, c_second, g_mode=FIXED, conc=0.0):
    """the rectangle as the driver adds it: first wall, ceiling, second wall; f stops one row short of the last row
    (:186-188, :194-196: Slice(R23 + 1, -1)), g's first wall runs through it (:222-224: Slice(R23 + 1, None)) with slot 7 of
    its foot left to the bottom wall, which the driver applies last (:234-236)"""
    t = pylbm.AdeInteriorWalls(lib, R, C)
    top = r_top + R if r_top < 0 else r_top
    n_side = (R - 1) - (top + 1)
    t.add(r_top + 1, c_first, 1, 0, n_side, COL_NEG, COL_NEG, g_mode, conc)
    t.add(-1, c_first, 1, 0, 1, 0, COL_NEG & ~mask(7), g_mode, conc)
    t.add(r_top, c_first, 0, 1, c_second - c_first + 1, ROW_NEG, ROW_NEG, g_mode, conc)
    t.add(r_top + 1, c_second, 1, 0, n_side, COL_POS, COL_POS, g_mode, conc)
    return t


def test_the_reference_rectangle_merges_to_its_eighteen_nodes(lib):
    t = reference_rectangle(lib, 24, 32, -7, 10, 16)
    assert lib.raw.lbm_ade_iwalls_count(t.h) == 18
    nodes = t.nodes()
    assert [(n["r"], n["c"]) for n in nodes] == sorted((n["r"], n["c"]) for n in nodes)  # sorted by (r, c)
    by_rc = {(n["r"], n["c"]): n for n in nodes}
    assert sorted(by_rc) == sorted([(17, c) for c in range(10, 17)] + [(r, c) for r in range(18, 23) for c in (10, 16)] + [(23, 10)])

    def entry(r, c, f, g):
        return dict(r=r, c=c, f_slots=f, g_slots=g, g_fixed_slots=g, conc=0.0)

    assert by_rc[(17, 10)] == entry(17, 10, ROW_NEG, ROW_NEG)          # the ceiling (its corner is the ceiling's alone)
    assert by_rc[(17, 16)] == entry(17, 16, ROW_NEG, ROW_NEG)
    assert by_rc[(18, 10)] == entry(18, 10, COL_NEG, COL_NEG)          # the first wall
    assert by_rc[(22, 16)] == entry(22, 16, COL_POS, COL_POS)          # the second wall
    assert by_rc[(23, 10)] == entry(23, 10, 0, mask(4, 8))             # g's foot: slot 7 is the bottom wall's
    assert (23, 16) not in by_rc
    # the raw accessor, every output optional
    r, c, gf = ct.c_int(), ct.c_int(), ct.c_uint()
    assert lib.raw.lbm_ade_iwalls_node(t.h, 17, ct.byref(r), ct.byref(c), None, None, ct.byref(gf), None) == 0
    assert (r.value, c.value, gf.value) == (23, 10, 0x88)
    # a body that holds a concentration: the same masks, FIXED at conc; NO_FLUX: no fixed slots
    held = reference_rectangle(lib, 24, 32, -7, 10, 16, FIXED, 1e-3).nodes()
    assert [dict(n, conc=0.0) for n in held] == nodes and all(n["conc"] == 1e-3 for n in held)
    sealed = reference_rectangle(lib, 24, 32, -7, 10, 16, NO_FLUX).nodes()
    assert [dict(n, g_fixed_slots=n["g_slots"]) for n in sealed] == nodes and all(n["g_fixed_slots"] == 0 for n in sealed)
    t.close()


def test_a_closed_box_has_corners_with_the_union_of_two_facings(lib):
    t = pylbm.AdeInteriorWalls(lib, 30, 42).add_box(5, 9, 11, 20, FIXED, 2e-3)
    by_rc = {(n["r"], n["c"]): n for n in t.nodes()}
    assert len(by_rc) == 2 * 10 + 2 * 3
    corners = {(5, 11): ROW_NEG | COL_NEG, (5, 20): ROW_NEG | COL_POS, (9, 11): ROW_POS | COL_NEG, (9, 20): ROW_POS | COL_POS}
    for rc, m in corners.items():
        assert bin(m).count("1") == 5
        assert by_rc[rc] == dict(r=rc[0], c=rc[1], f_slots=m, g_slots=m, g_fixed_slots=m, conc=2e-3)
    assert by_rc[(5, 15)]["f_slots"] == ROW_NEG and by_rc[(9, 15)]["f_slots"] == ROW_POS
    assert by_rc[(7, 11)]["g_slots"] == COL_NEG and by_rc[(7, 20)]["g_slots"] == COL_POS
    assert (7, 15) not in by_rc  # the inside is not in the table
    t.close()
