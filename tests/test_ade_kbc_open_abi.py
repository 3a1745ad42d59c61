"""CPU suite, open boundaries and the wall exchange of the fluid + scalar step with the fluid by model
(lbm_ade_open_collide_m, lbm_ade_open_stream_collide_m, lbm_ade_solver_set_open_m, lbm_ade_wallx_rows_m,
lbm_ade_solver_wall_exchange_m): the entries are exported and declared, their names stay outside the closed family of
tests/ade_calls.py, each refuses on the host before any device call -- under its own name with a KBC fluid, under its
sibling's with model = BGK -- and the header still compiles as C99.  Without a device only an EMPTY open table can be
finalized: the refusals that need listed nodes (the carry, the row range, the overlap rule) and those that need a context
are tests/test_gpu_ade_kbc_open.py's."""
import ctypes as ct
import os
import re
import subprocess

import pytest

import ade_calls
import pylbm

SYMBOLS = ["lbm_ade_open_collide_m", "lbm_ade_open_stream_collide_m", "lbm_ade_solver_set_open_m", "lbm_ade_wallx_rows_m",
           "lbm_ade_solver_wall_exchange_m"]
SIBLINGS = {"lbm_ade_open_collide_m": "lbm_ade_collide_o", "lbm_ade_open_stream_collide_m": "lbm_ade_stream_collide_o",
            "lbm_ade_solver_set_open_m": "lbm_ade_solver_set_open", "lbm_ade_wallx_rows_m": "lbm_ade_wallx_rows",
            "lbm_ade_solver_wall_exchange_m": "lbm_ade_solver_wall_exchange"}
REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = pylbm.Geom(16, 16, 0)
SCALAR = pylbm.AdeParams(1.7, (3e-3, -2e-3))
HOST_CHECK_ROWS = 307  # the refusals drivers/ade_kbc_host_check.cpp checks: 226 before the open-boundary section


@pytest.fixture(scope="module")
def lib():
    return pylbm.Lib()


def kbc(s2=1.9, form=pylbm.FORM_DEFAULT):
    return pylbm.AdeFluid(pylbm.KbcParams(s2, form))


def bgk(omega=1.2, form=pylbm.FORM_DEFAULT):
    return pylbm.AdeFluid(pylbm.BgkParams(omega, 0, form=form))


def ref(x):
    return ct.byref(x) if x is not None else None


def handle(t):
    return t.h if t is not None else None


def open_collide_m(lib, fluid, g=G, bc=None, scalar=SCALAR, sbc=None, buoy=None, table=None, lattices=(None,) * 4, carry_out=None):
    lib.ade_open_collide_m(*lattices, ref(g), ref(bc), ref(fluid), ref(scalar), ref(sbc), ref(buoy), handle(table), carry_out,
                           None, None, None, None)


def open_step_m(lib, fluid, g=G, bc=None, scalar=SCALAR, sbc=None, buoy=None, walls=None, table=None, lattices=(None,) * 4,
                carry=(None, None), rows=None):
    r0, r1 = rows if rows is not None else (0, g.R)
    lib.ade_open_stream_collide_m(*lattices, ref(g), ref(bc), ref(fluid), ref(scalar), ref(sbc), ref(buoy), handle(walls),
                                  handle(table), *carry, r0, r1, None, None, None, None)


def wallx_rows_m(lib, fluid, g=G, bc=None, scalar=SCALAR, sbc=None, buoy=None, walls=None, buffers=(None,) * 3, table_rows=16,
                 rows=None):
    r0, r1 = rows if rows is not None else (0, g.R)
    lib.ade_wallx_rows_m(buffers[0], table_rows, 0, buffers[1], buffers[2], ref(g), ref(bc), ref(fluid), ref(scalar), ref(sbc),
                         ref(buoy), handle(walls), None, r0, r1, None)


RAW = {"lbm_ade_open_collide_m": open_collide_m, "lbm_ade_open_stream_collide_m": open_step_m, "lbm_ade_wallx_rows_m": wallx_rows_m}


def every_entry(lib, msg, fluid, bgk_model=False, only=RAW, **kw):
    """the three raw entries refuse with `msg` under their own name -- under the sibling's with model = BGK"""
    for name in only:
        said = SIBLINGS[name] if bgk_model else name
        with pytest.raises(pylbm.LbmError, match=rf"{name} -> -1: {said}: .*{msg}"):
            RAW[name](lib, fluid, **kw)


def test_symbols_are_declared_and_exported(lib):
    declared = set(pylbm.declared_symbols())
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(lib.raw, name), name


def test_the_new_names_stay_outside_the_closed_family(lib):
    """tests/test_ade_calls.py pins the prototypes tests/ade_calls.py reads from the header to a literal table"""
    pattern = re.compile(r"lbm_(?:ring_)?ade_(?:collide|stream_collide|step)\w*")
    for name in SYMBOLS:
        assert not pattern.fullmatch(name), name
        assert name not in ade_calls.PROTOTYPES, name
    for name in ("lbm_ade_collide_o", "lbm_ade_stream_collide_o"):  # (the siblings are in it)
        assert name in ade_calls.PROTOTYPES


def test_parameter_lists_are_the_siblings_with_the_fluid_by_model():
    txt = re.sub(r"/\*.*?\*/", "", open(pylbm.HEADER).read(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(lbm_ade_\w+)\s*\(([^)]*)\)\s*;", txt))
    for new, old in SIBLINGS.items():
        a, b = [" ".join(protos[k].split()) for k in (new, old)]
        assert a == b.replace("const lbm_bgk_params* fluid", "const lbm_ade_fluid* fluid"), (new, a, b)


def test_null_fluid_and_unknown_model(lib):
    every_entry(lib, "NULL fluid", None)
    every_entry(lib, "fluid model=7", pylbm.AdeFluid(pylbm.KbcParams(1.6), model=7))


@pytest.mark.parametrize("s2", [0.0, 2.5, -1.0])
def test_s2_outside_its_range(lib, s2):
    every_entry(lib, r"KBC fluid: s2=\S+ outside \(0, 2\]", kbc(s2))


def test_what_the_m_and_mb_calls_refuse(lib):
    """pressure rows, a form mismatch, non-finite buoyancy fields -- naming the feature and the model -- and the checks the
    step shares with the BGK fluid, under the new names"""
    every_entry(lib, "pressure rows .* with a KBC fluid", kbc(), bc=pylbm.Bc(pressure_rows=1))
    every_entry(lib, "KBC fluid: form=7", kbc(form=7))
    every_entry(lib, "KBC fluid form=1 differs from the scalar form=2", kbc(form=REF), scalar=pylbm.AdeParams(1.7, (0.0, 0.0), form=FAST))
    for field, word in (("beta_r", "beta"), ("beta_c", "beta"), ("c_ref", "c_ref"), ("u_shift", "u_shift"), ("guo_a", "guo"),
                        ("guo_b", "guo")):
        by = pylbm.AdeBuoyancy((1e-2, -5e-3), 0.4)
        setattr(by, field, float("nan") if field != "c_ref" else float("inf"))
        every_entry(lib, f"buoyancy {word}=.* must be finite", kbc(), buoy=by)
    every_entry(lib, "C=15 must be even", kbc(), g=pylbm.Geom(16, 15, 0))
    every_entry(lib, "omega_g=2", kbc(), scalar=pylbm.AdeParams(2.0, (0.0, 0.0)))
    every_entry(lib, "NULL scalar params", kbc(), scalar=None)
    every_entry(lib, "scalar edge row_lo: FIXED on a PERIODIC", kbc(), sbc=pylbm.AdeScalarBC(row_lo=1e-3))
    every_entry(lib, "ghost=2", kbc(), g=pylbm.Geom(16, 16, 2), only=["lbm_ade_open_collide_m", "lbm_ade_open_stream_collide_m"])
    walls = pylbm.AdeInteriorWalls(lib, 16, 16).add(3, 3, 0, 1, 2, 0x0F, 0)  # not finalized
    every_entry(lib, "interior walls: the table is not finalized", kbc(), walls=walls,
                only=["lbm_ade_open_stream_collide_m", "lbm_ade_wallx_rows_m"])
    walls.close()


def test_what_the_o_calls_refuse_without_a_listed_node(lib):
    """an unfinalized table, a table for another lattice, a slab view; past the table the lattices, the moments, the range"""
    only = ["lbm_ade_open_collide_m", "lbm_ade_open_stream_collide_m"]
    raw = pylbm.AdeOpenBoundary(lib, 16, 16).channel(0.03, 1e-3, 4)  # not finalized: finalize uploads
    every_entry(lib, "open boundaries: the table is not finalized", kbc(), table=raw, only=only)
    view = raw.slab(0, 16)
    every_entry(lib, r"open boundaries: the table is a slab view \(lbm_ade_open_slab\)", kbc(), table=view, only=only)
    small = pylbm.AdeOpenBoundary(lib, 6, 8).finalize()  # empty: no device call
    every_entry(lib, "open boundaries: the table is for a 6 x 8 lattice, the call for 16 x 16", kbc(), table=small, only=only)
    empty = pylbm.AdeOpenBoundary(lib, 16, 16).finalize()
    for table in (None, empty):  # NULL's: no carry is asked for, the call is stopped at its lattices
        every_entry(lib, "NULL lattice", kbc(), table=table, only=only)
    one, two, three, four = [(ct.c_double * 4)() for _ in range(4)]
    with pytest.raises(pylbm.LbmError, match="lbm_ade_open_stream_collide_m: aliased lattices"):
        open_step_m(lib, kbc(), lattices=(one, one, two, two))
    with pytest.raises(pylbm.LbmError, match=r"lbm_ade_open_stream_collide_m: row range \[5, 3\) outside \[0, 16\)"):
        open_step_m(lib, kbc(), lattices=(one, two, three, four), rows=(5, 3))
    for t in (view, raw, small, empty):
        t.close()


def test_the_exchange_s_own_arguments(lib):
    one, two, three = [(ct.c_double * 4)() for _ in range(3)]
    with pytest.raises(pylbm.LbmError, match=r"lbm_ade_wallx_rows_m: NULL argument \(table, fo, go\)"):
        wallx_rows_m(lib, kbc())
    with pytest.raises(pylbm.LbmError, match="lbm_ade_wallx_rows_m: "):
        wallx_rows_m(lib, kbc(), buffers=(one, two, three), rows=(5, 3))
    with pytest.raises(pylbm.LbmError, match=r"lbm_ade_wallx_rows_m: table_row0=0 \+ rows \[0, 16\) do not fit table_rows=4"):
        wallx_rows_m(lib, kbc(), buffers=(one, two, three), table_rows=4)
    out = (ct.c_double * pylbm.WALLX_NQ)()
    with pytest.raises(pylbm.LbmError, match=r"NULL argument \(solver, out_host\)"):
        lib.ade_solver_wall_exchange_m(None, None, 0, 16, out, None)
    with pytest.raises(pylbm.LbmError, match="NULL solver"):
        lib.ade_solver_set_open_m(None, None)


def test_model_bgk_reports_under_the_sibling_s_name(lib):
    every_entry(lib, "omega=2 outside", bgk(2.0), bgk_model=True)
    every_entry(lib, "incompressible=1", pylbm.AdeFluid(pylbm.BgkParams(1.2, 1)), bgk_model=True)
    raw = pylbm.AdeOpenBoundary(lib, 16, 16).channel(0.03, 1e-3, 4)
    every_entry(lib, "open boundaries: the table is not finalized", bgk(), bgk_model=True, table=raw,
                only=["lbm_ade_open_collide_m", "lbm_ade_open_stream_collide_m"])
    raw.close()
    every_entry(lib, "NULL lattice", bgk(), bgk_model=True, only=["lbm_ade_open_collide_m", "lbm_ade_open_stream_collide_m"])
    every_entry(lib, r"NULL argument \(table, fo, go\)", bgk(), bgk_model=True, only=["lbm_ade_wallx_rows_m"])
    fl = bgk()
    fl.kbc = pylbm.KbcParams(-3.0, 9)  # not read with model = BGK
    every_entry(lib, "NULL lattice", fl, bgk_model=True, only=["lbm_ade_open_stream_collide_m"])


def test_header_is_plain_c99_and_every_entry_refuses_nulls(tmp_path):
    src = tmp_path / "ade_kbc_open_c99.c"
    src.write_text('#include "lbm_hip.h"\n'
                   'int main(void){ double out[LBM_WALLX_NQ]; int bad = 0;\n'
                   '  bad += lbm_ade_open_collide_m(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != LBM_ERR_INVALID;\n'
                   '  bad += lbm_ade_open_stream_collide_m(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != LBM_ERR_INVALID;\n'
                   '  bad += lbm_ade_solver_set_open_m(0, 0) != LBM_ERR_INVALID;\n'
                   '  bad += lbm_ade_wallx_rows_m(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) != LBM_ERR_INVALID;\n'
                   '  bad += lbm_ade_solver_wall_exchange_m(0, 0, 0, 0, out, 0) != LBM_ERR_INVALID;\n'
                   '  return bad; }\n')
    libdir = os.path.join(ROOT, "lattice-boltzmann-method_amd", "lib")
    exe = tmp_path / "ade_kbc_open_c99"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L",
                           libdir, "-llbm_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_host_check_program_counts_the_new_rows():
    """drivers/ade_kbc_host_check.cpp, the stand-alone program `make san` runs under ASan + UBSan, here in the ordinary
    build: the refusals of the new entries from C++, and WHICH fault a call with two faults reports -- for model = BGK word
    for word what lbm_ade_collide_o, lbm_ade_stream_collide_o and lbm_ade_wallx_rows report"""
    exe = os.path.join(ROOT, "lattice-boltzmann-method_amd", "drivers", "bin", "ade_kbc_host_check")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) refusals checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) == HOST_CHECK_ROWS, r.stdout
