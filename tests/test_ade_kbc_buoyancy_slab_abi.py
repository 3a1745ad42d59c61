"""CPU suite, the forced KBC collision (buoyancy) over row slabs and the ring: lbm_ade_slab_stream_collide_mb,
lbm_ring_ade_slab_collide_mb and lbm_ring_ade_slab_step_mb are declared, exported and bound, their parameter lists are
pinned to a literal table, the header compiles as C99, and every host refusal comes with its message under the new name
before any device call -- NULL arguments, a non-finite field of the descriptor, and everything the `_m` slab entries refuse.
model = BGK answers under the names of lbm_ade_stream_collide_part_w / lbm_ring_ade_collide_b / lbm_ring_ade_step_w.  The
ring's entries need a ring, and a ring needs a device: what they refuse before they look at the ring is here, the rest in
tests/test_gpu_ade_kbc_buoyancy_slabs.py."""
import ctypes as ct
import os
import re
import subprocess

import pytest

import pylbm
from ade_calls import ref as _ref
from ade_kbc_buoyancy_slab_calls import PROTOTYPES

PART, RING_COLLIDE, RING_STEP = "lbm_ade_slab_stream_collide_mb", "lbm_ring_ade_slab_collide_mb", "lbm_ring_ade_slab_step_mb"
REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
HALO, BB = pylbm.EDGE_HALO, pylbm.EDGE_BOUNCE_BACK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

G0 = pylbm.Geom(16, 16, 0)
G1 = pylbm.Geom(16, 16, 1)
SEAMS = pylbm.Bc(row_lo=HALO, row_hi=HALO)
SCALAR = pylbm.AdeParams(1.7, (3e-3, 3e-3))
BY = pylbm.AdeBuoyancy((1e-2, -5e-3), 0.4)

# the parameter lists, literally: the `_m` sibling's with `buoy` after `sbc`
PINNED = {
    PART: ["fn", "gn", "fo", "go", "g", "bc", "fluid", "scalar", "sbc", "buoy", "iwalls", "part", "edge_rows", "rho", "u", "conc", "s"],
    RING_COLLIDE: ["rg", "fp", "gp", "f", "g_in", "bc", "fluid", "scalar", "sbc", "buoy", "main"],
    RING_STEP: ["rg", "fn", "gn", "fo", "go", "bc", "fluid", "scalar", "sbc", "buoy", "iwalls", "edge_rows", "main"],
}


@pytest.fixture(scope="module")
def lib():
    return pylbm.Lib()


@pytest.fixture(scope="module")
def lattices():
    """four distinct 16-byte aligned host buffers: every call here is refused before a lattice is read"""
    bufs = [(ct.c_double * 8)() for _ in range(4)]
    ptrs = [(ct.addressof(b) + 15) & ~15 for b in bufs]
    return bufs, ptrs


def kbc(s2=1.6, form=pylbm.FORM_DEFAULT):
    return pylbm.AdeFluid(pylbm.KbcParams(s2, form))


def part_mb(lib, lat, g, bc, fluid, scalar, part=FRAME, E=1, sbc=None, by=BY, table=None, rho=None):
    lib.ade_slab_stream_collide_mb(*lat, _ref(g), _ref(bc), _ref(fluid), _ref(scalar), _ref(sbc), _ref(by),
                                   table.h if table is not None else None, part, E, rho, None, None, None)


def refused(lib, lattices, msg, g=G1, bc=SEAMS, fluid=None, scalar=SCALAR, **kw):
    with pytest.raises(pylbm.LbmError, match=msg):
        part_mb(lib, lattices[1], g, bc, fluid, scalar, **kw)


def test_symbols_are_declared_exported_and_bound(lib):
    declared = set(pylbm.declared_symbols())
    for name, n in ((PART, 17), (RING_COLLIDE, 11), (RING_STEP, 13)):
        assert name in declared, name
        assert hasattr(lib.raw, name), name
        fn = getattr(lib.raw, name)
        assert fn.argtypes is not None and fn.restype is ct.c_int, name
        assert len(fn.argtypes) == n, name
    assert lib.raw.lbm_ade_slab_stream_collide_mb.argtypes[11:13] == [ct.c_int, ct.c_int]  # part, edge_rows
    assert lib.raw.lbm_ring_ade_slab_step_mb.argtypes[11] is ct.c_int                        # edge_rows


def test_parameter_lists_are_the_pinned_ones():
    assert PROTOTYPES == PINNED


def test_parameter_lists_are_the_m_siblings_with_buoy_after_sbc():
    import ade_calls
    for name, sibling in ((PART, "lbm_ade_stream_collide_part_m"), (RING_COLLIDE, "lbm_ring_ade_collide_m"),
                          (RING_STEP, "lbm_ring_ade_step_m")):
        want = list(ade_calls.PROTOTYPES[sibling])
        want.insert(want.index("sbc") + 1, "buoy")
        assert PINNED[name] == want, name
        assert name not in ade_calls.PROTOTYPES  # the pinned table of that module stays what it is


def test_abi_version_stays_one(lib):
    assert lib.raw.lbm_abi_version() == 1


def test_null_fluid_and_unknown_model(lib, lattices):
    refused(lib, lattices, rf"-> -1: {PART}: NULL fluid \(lbm_ade_fluid\)", fluid=None)
    refused(lib, lattices, f"{PART}: fluid model=7", fluid=pylbm.AdeFluid(pylbm.KbcParams(1.6), model=7))


@pytest.mark.parametrize("field,by,msg", [
    ("beta_r", pylbm.AdeBuoyancy((NAN, 0.0), 0.5), r"buoyancy beta=\(nan, 0\) must be finite"),
    ("beta_c", pylbm.AdeBuoyancy((1e-2, INF), 0.5), r"buoyancy beta=\(0\.01, inf\) must be finite"),
    ("c_ref", pylbm.AdeBuoyancy((1e-2, 0.0), NAN), r"buoyancy c_ref=nan must be finite"),
    ("u_shift", pylbm.AdeBuoyancy((1e-2, 0.0), 0.5, -INF), r"buoyancy u_shift=-inf must be finite"),
    ("guo", pylbm.AdeBuoyancy((1e-2, 0.0), 0.5, 1.0, (NAN, 1.0)), r"buoyancy guo=\(nan, 1\) must be finite"),
])
def test_a_non_finite_field_is_refused_by_name_in_all_three(lib, lattices, field, by, msg):
    p, sc, fl = lattices[1], ct.byref(SCALAR), ct.byref(kbc())
    refused(lib, lattices, f"-> -1: {PART}: {msg}", fluid=kbc(), by=by)
    with pytest.raises(pylbm.LbmError, match=f"-> -1: {RING_COLLIDE}: {msg}"):  # before the ring is looked at
        lib.ring_ade_slab_collide_mb(None, *p, None, fl, sc, None, ct.byref(by), None)
    with pytest.raises(pylbm.LbmError, match=f"-> -1: {RING_STEP}: {msg}"):
        lib.ring_ade_slab_step_mb(None, *p, None, fl, sc, None, ct.byref(by), None, 1, None)


def test_a_non_finite_field_is_refused_with_a_zero_beta_too(lib, lattices):
    refused(lib, lattices, f"{PART}: buoyancy c_ref=inf must be finite", fluid=kbc(), by=pylbm.AdeBuoyancy((0.0, 0.0), INF))


@pytest.mark.parametrize("s2", [0.0, 2.5, -1.0])
def test_s2_outside_its_range(lib, lattices, s2):
    refused(lib, lattices, rf"{PART}: KBC fluid: s2=\S+ outside \(0, 2\]", fluid=kbc(s2))


def test_a_fluid_form_that_differs_from_the_scalars(lib, lattices):
    refused(lib, lattices, f"{PART}: KBC fluid form=1 differs from the scalar form=2", fluid=kbc(form=REF),
            scalar=pylbm.AdeParams(1.7, (0.0, 0.0), form=FAST))
    refused(lib, lattices, "KBC fluid form=2 differs from the scalar form=0", fluid=kbc(form=FAST),
            scalar=pylbm.AdeParams(1.7, (0.0, 0.0)))
    refused(lib, lattices, "KBC fluid: form=7", fluid=kbc(form=7))


def test_pressure_rows_are_refused_by_name(lib, lattices):
    refused(lib, lattices, f"{PART}: pressure rows .* with a KBC fluid",
            bc=pylbm.Bc(row_lo=HALO, row_hi=HALO, pressure_rows=1), fluid=kbc())


def test_a_wrong_part_and_the_edge_rows(lib, lattices):
    refused(lib, lattices, rf"{PART}: part=5 \(LBM_ADE_PART_FRAME or LBM_ADE_PART_INNER\)", fluid=kbc(), part=5)
    refused(lib, lattices, "edge_rows=0: need 1 <= edge_rows", fluid=kbc(), E=0)
    refused(lib, lattices, f"{PART}: edge_rows=8: need 1 <= edge_rows and 2 x edge_rows < R=16", fluid=kbc(), E=8)
    refused(lib, lattices, "edge_rows=8", fluid=kbc(), E=8, part=INNER)


def test_the_geometry_of_a_slab(lib, lattices):
    refused(lib, lattices, "row edge mode HALO needs ghost rows", g=G0, bc=SEAMS, fluid=kbc())
    refused(lib, lattices, "row edge mode PERIODIC given", g=G1, bc=pylbm.Bc.periodic(), fluid=kbc())
    refused(lib, lattices, "row edge mode PERIODIC given", g=G1, bc=None, fluid=kbc())
    for g, bc in ((G1, SEAMS), (G1, pylbm.Bc(row_lo=BB, row_hi=HALO)), (pylbm.Geom(16, 16, 2), SEAMS),
                  (G0, pylbm.Bc.periodic()), (G0, pylbm.Bc(row_lo=BB, row_hi=BB))):
        refused(lib, lattices, "part=5", g=g, bc=bc, fluid=kbc(), part=5)
    refused(lib, lattices, "_slab_stream_collide_mb: C=15 must be even", g=pylbm.Geom(16, 15, 1), fluid=kbc())
    refused(lib, lattices, "_slab_stream_collide_mb: ghost=16 must be 0..15", g=pylbm.Geom(16, 16, 16), fluid=kbc())
    refused(lib, lattices, f"{PART}: NULL geometry", g=None, fluid=kbc())
    refused(lib, lattices, f"{PART}: NULL scalar params", fluid=kbc(), scalar=None)
    refused(lib, lattices, "_slab_stream_collide_mb: scalar edge row_lo: FIXED on a HALO", fluid=kbc(), sbc=pylbm.AdeScalarBC(row_lo=1e-3))


def test_lattice_and_moment_arguments(lib, lattices):
    """with NULL, zero and non-zero beta the first refusal of a call with nothing wrong but a lattice is the lattice's"""
    p = lattices[1]
    for by in (None, pylbm.AdeBuoyancy((0.0, 0.0), 0.3), BY):
        with pytest.raises(pylbm.LbmError, match=f"{PART}: NULL lattice"):
            part_mb(lib, [None, p[1], p[2], p[3]], G1, SEAMS, kbc(), SCALAR, by=by)
    with pytest.raises(pylbm.LbmError, match="_slab_stream_collide_mb: aliased lattices"):
        part_mb(lib, [p[0], p[0], p[2], p[3]], G1, SEAMS, kbc(), SCALAR)
    with pytest.raises(pylbm.LbmError, match="_slab_stream_collide_mb: lattices must be 16-byte aligned"):
        part_mb(lib, [p[0] + 8, p[1], p[2], p[3]], G1, SEAMS, kbc(), SCALAR)
    with pytest.raises(pylbm.LbmError, match="rho, u and conc"):
        part_mb(lib, p, G1, SEAMS, kbc(), SCALAR, rho=p[0])


def test_buoyancy_on_a_slab_is_no_longer_refused(lib, lattices):
    """the refusal no public call could reach is gone: a buoyant call on a slab with nothing else wrong gets as far as its
    part, in every form"""
    for form in (pylbm.FORM_DEFAULT, REF, FAST):
        refused(lib, lattices, f"{PART}: part=5", fluid=kbc(form=form), scalar=pylbm.AdeParams(1.7, (0.0, 0.0), form=form), part=5)
    src = open(os.path.join(ROOT, "lattice-boltzmann-method_amd", "csrc", "capi_ade.hip")).read()
    assert "buoyancy on a slab is not supported" not in src


def test_an_unfinalized_table_and_a_table_of_the_wrong_shape(lib, lattices):
    t = pylbm.AdeInteriorWalls(lib, 16, 16)  # empty: no device call at finalize
    refused(lib, lattices, "_slab_stream_collide_mb: interior walls: the table is not finalized", fluid=kbc(), table=t)
    t.close()
    t = pylbm.AdeInteriorWalls(lib, 12, 16).finalize()
    refused(lib, lattices, "interior walls: the table is for a 12 x 16 lattice, the call for 16 x 16", fluid=kbc(), table=t)
    t.close()


def test_the_order_of_checks(lib, lattices):
    """calls with two faults report the first: the fluid's own parameters, the scalar's walls, the geometry, the descriptor,
    the table, the form, the lattices, the part"""
    bad_by = pylbm.AdeBuoyancy((NAN, 0.0), 0.5)
    refused(lib, lattices, "s2=2.5 outside", fluid=kbc(2.5), by=bad_by)
    refused(lib, lattices, "C=15 must be even", g=pylbm.Geom(16, 15, 1), fluid=kbc(), by=bad_by)
    refused(lib, lattices, "buoyancy beta", fluid=kbc(form=REF), scalar=pylbm.AdeParams(1.7, (0.0, 0.0), form=FAST), by=bad_by)
    refused(lib, lattices, "buoyancy beta", fluid=kbc(), by=bad_by, part=5)
    refused(lib, lattices, "differs from the scalar form", fluid=kbc(form=REF), scalar=pylbm.AdeParams(1.7, (0.0, 0.0), form=FAST), part=5)
    p = lattices[1]
    with pytest.raises(pylbm.LbmError, match="NULL lattice"):
        part_mb(lib, [None, p[1], p[2], p[3]], G1, SEAMS, kbc(), SCALAR, part=5)


def test_model_bgk_is_part_w(lib, lattices):
    """a bad descriptor, bad BGK parameters, a bad part and a bad geometry give lbm_ade_stream_collide_part_w's message; the
    kbc member is not read"""
    fl = pylbm.AdeFluid(pylbm.BgkParams(1.2, 0))
    w = "-> -1: lbm_ade_stream_collide_part_w: "
    refused(lib, lattices, w + r"buoyancy beta=\(nan, 0\) must be finite", fluid=fl, by=pylbm.AdeBuoyancy((NAN, 0.0), 0.5))
    for bad, msg in ((pylbm.BgkParams(2.0, 0), "omega=2 outside"), (pylbm.BgkParams(1.2, 1), "incompressible=1")):
        refused(lib, lattices, w + msg, fluid=pylbm.AdeFluid(bad))
    fl.kbc = pylbm.KbcParams(-3.0, 9)
    refused(lib, lattices, w + "part=5", fluid=fl, part=5)
    refused(lib, lattices, w + "edge_rows=8", fluid=fl, E=8)
    refused(lib, lattices, w + "row edge mode HALO needs ghost rows", g=G0, fluid=fl)


def test_the_ring_entries_look_at_the_fluid_then_the_descriptor_then_their_arguments(lib, lattices):
    p = lattices[1]
    sc, by = ct.byref(SCALAR), ct.byref(BY)
    with pytest.raises(pylbm.LbmError, match=f"{RING_COLLIDE}: NULL fluid"):
        lib.ring_ade_slab_collide_mb(None, *p, None, None, sc, None, by, None)
    with pytest.raises(pylbm.LbmError, match=f"{RING_STEP}: NULL fluid"):
        lib.ring_ade_slab_step_mb(None, *p, None, None, sc, None, by, None, 1, None)
    bad = pylbm.AdeFluid(pylbm.KbcParams(1.6), model=7)
    with pytest.raises(pylbm.LbmError, match=f"{RING_STEP}: fluid model=7"):
        lib.ring_ade_slab_step_mb(None, *p, None, ct.byref(bad), sc, None, by, None, 1, None)
    for b in (None, by):
        with pytest.raises(pylbm.LbmError, match=f"{RING_COLLIDE}: NULL argument"):
            lib.ring_ade_slab_collide_mb(None, *p, None, ct.byref(kbc()), sc, None, b, None)
        with pytest.raises(pylbm.LbmError, match=f"{RING_STEP}: NULL argument"):
            lib.ring_ade_slab_step_mb(None, *p, None, ct.byref(kbc()), sc, None, b, None, 1, None)
    fl = pylbm.AdeFluid(pylbm.BgkParams(1.2, 0))  # model = BGK: the entries it forwards to answer
    with pytest.raises(pylbm.LbmError, match="lbm_ring_ade_collide_b: NULL argument"):
        lib.ring_ade_slab_collide_mb(None, *p, None, ct.byref(fl), sc, None, by, None)
    with pytest.raises(pylbm.LbmError, match="lbm_ring_ade_step_w: NULL argument"):
        lib.ring_ade_slab_step_mb(None, *p, None, ct.byref(fl), sc, None, by, None, 1, None)
    nan_by = pylbm.AdeBuoyancy((NAN, 0.0), 0.5)
    with pytest.raises(pylbm.LbmError, match=r"lbm_ring_ade_step_w: buoyancy beta=\(nan, 0\)"):
        lib.ring_ade_slab_step_mb(None, *p, None, ct.byref(fl), sc, None, ct.byref(nan_by), None, 1, None)


def test_header_with_the_new_prototypes_is_plain_c99(tmp_path):
    src = tmp_path / "ade_kbc_buoyancy_slab_c99.c"
    src.write_text('#include "lbm_hip.h"\n'
                   'int main(void){ lbm_ade_fluid fl; lbm_ade_params p = {1.0, 0.0, 0.0, LBM_FORM_DEFAULT};\n'
                   '  lbm_ade_buoyancy b = {1e-3, 0.0, 0.5, 1.0, 0.0, 0.0};\n'
                   '  lbm_geom g = {16, 16, 1, 0, 0}; double a[2] = {0}, c[2] = {0}, d[2] = {0}, e[2] = {0};\n'
                   '  fl.model = LBM_MODEL_KBC; fl.kbc.s2 = 0.0; fl.kbc.form = LBM_FORM_DEFAULT;\n'
                   '  if (lbm_ade_slab_stream_collide_mb(a, c, d, e, &g, 0, &fl, &p, 0, &b, 0, LBM_ADE_PART_FRAME, 1, 0, 0, 0, 0)\n'
                   '      != LBM_ERR_INVALID) return 1;\n'
                   '  if (lbm_ring_ade_slab_collide_mb(0, a, c, d, e, 0, 0, &p, 0, &b, 0) != LBM_ERR_INVALID) return 2;\n'
                   '  return lbm_ring_ade_slab_step_mb(0, a, c, d, e, 0, 0, &p, 0, &b, 0, 1, 0) == LBM_ERR_INVALID ? 0 : 3; }\n')
    libdir = os.path.join(ROOT, "lattice-boltzmann-method_amd", "lib")
    exe = tmp_path / "ade_kbc_buoyancy_slab_c99"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-L", libdir, "-llbm_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0


def test_the_extended_host_check_program_passes():
    """the ORDINARY build of drivers/ade_kbc_host_check with its rows for the three entries: 226 refusals in all, 66 of them
    for these entries, 15 of those calls with two faults that pin which one is reported; the sanitizer build of the same
    source is `make san`'s and is not run here"""
    exe = os.path.join(ROOT, "lattice-boltzmann-method_amd", "drivers", "bin", "ade_kbc_host_check")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) refusals checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 226, r.stdout
    assert "lbm_ade_slab_stream_collide_mb" in open(os.path.join(ROOT, "lattice-boltzmann-method_amd", "drivers",
                                                                 "ade_kbc_host_check.cpp")).read()
