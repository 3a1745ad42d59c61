"""The stated accuracy of the default two-phase step -- the one-launch fused step (lbm_cg_step_fused, inner form 102) -- per
node and per output, in units in the last place against the 80-bit yardstick of tests/exact_cg.py, on lattices of edge
states (interfaces on the wall row, on the copy columns and on a tile corner, exact steps, exactly absent colours, noise
up to 0.1, six parameter points).  The bar is the error of the two-pass reference-order kernels on the same nodes -- which
are bitwise the oracle's loop body -- not a tolerance chosen in advance; tests/test_gpu_cg.py bounds the same step by an
L2 norm over smooth fields, which a kernel that is wrong on a few nodes passes.

Per parameter point and lattice, through the C ABI with the driver's boundary set, one step each:
  a. reference order (lbm_cg_stream_moments + lbm_cg_stream_collide): populations and the five fields bitwise equal to
     orc_cg_step_from_post;
  b. fused: everything finite; with add_source = 0 an exactly absent colour stays nine exact zeros; and for each of the
     four classes (populations, rho_k / u, psi, s_nu) median, 99th percentile and maximum of the per-node error at most
     MARGIN x the same statistic of the two-pass GPU result.  MARGIN is that of tests/test_gpu_collision_accuracy.py: a
     margin over the reference, not over the code under test;
  c. kernel forms, on 80 x 200 of two parameter points: the 16 x 32 inner kernel ("cg_big" = 0), the FRAME + INNER parts
     with edge_rows = 3 and the row-padded lattice write the bits of the default -- with b. that carries the bound to
     every kernel form a solver step can launch.
  d. the opt-in inner kernels (the walking block; in an EXPERIMENTS build the strip kernels and the walking tile) write the
     bits of the default on the same lattice, whose inner rectangle holds nodes inside the blend band.
The lattices: 37 x 45 (no inner rectangle: every tile through the boundary gather, inner form 0) and 80 x 200 (3 x 2 tiles
of 16 x 64 inside, a 16 x 32 tile column and a partial one in the frame: inner form 102), the latter also with row_pitch =
208; all with the plane padding of ade_util.geom, every double outside the owned nodes SENTINEL before and after.
Nodes the yardstick marks ill-conditioned (exact_cg: the colour gradient cancels) are left out of the population
statistics only; the generator has none.  The measured table goes to profiles/cg_accuracy.txt.

Measured on MI355X (18 runs of a. and b.): the worst fused / two-pass ratio of a statistic is 1.24 for the populations,
0.85 for rho_k / u, 1.06 for psi and 1.00 for s_nu.  Before this test the s_nu ratio was 2.45: its maximum missed the bar
at density-ratio-100 37x45 (86.09 units fused, 35.08 two-pass) and static-droplet 37x45 (4.34 | 2.54).  The term: inside
the blend band |psi| <= delta the slope of s_nu(psi) -- up to 2 (s_1 - omega_b) / delta = 30 -- multiplies the error psi
inherits from the rounding of rho_r and rho_b, in both forms alike, on some twenty nodes per lattice.  The fused kernels
now take psi there from compensated sums (cg_snu_node, csrc/cg_fused.hpp): s_nu maximum 0.94 ... 2.38 units on all 18
runs, against up to 107 in the reference order.  profiles/cg_accuracy.txt has both tables and the benchmark."""
import ctypes as ct
import os

import numpy as np
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import exact_cg as xg  # noqa: E402
import pylbm  # noqa: E402
from ade_util import SENTINEL, assert_bits, assert_write_set, bits, from_lattice, geom, owned, poisoned  # noqa: E402
from gpu_util import bits_equal, dev, ulp_diff  # noqa: E402
from pylbm import _ptr  # noqa: E402
from test_exact_cg import as_classes, oracle_params  # noqa: E402
from test_gpu_collision_accuracy import MARGIN  # noqa: E402

REPORT = os.path.join(ROOT, "profiles", "cg_accuracy.txt")
CASES = xg.cases()
LAYOUTS = {"37x45": ("37x45", 0), "80x200": ("80x200", 0), "80x200-pitch208": ("80x200", 208)}   # lattice, row pitch (0: dense)
INNER_FORM = {"37x45": 0, "80x200": 102}
FIELDS = (("rho_r", 1), ("rho_b", 1), ("u", 2), ("psi", 1), ("s_nu", 1))
_rows = {}


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if len(_rows) != len(CASES) * len(LAYOUTS):   # a full run only
        return
    lines = ["per case and lattice, per class: two-pass | fused"]   # (no commit id: a re-run on the same kernels rewrites the same bytes)
    for (name, layout), (ref, fast) in _rows.items():
        lines.append("%-20s %-16s %s" % (name, layout, "   ".join("%s %s | %s" % (cls, xg.fmt(ref[cls]), xg.fmt(fast[cls]))
                                                                  for cls in xg.CLASSES)))
    lines.append("worst fused / two-pass ratio of a statistic, per class: " + "   ".join(
        "%s %.2f" % (cls, max(f[cls][k] / r[cls][k] for r, f in _rows.values() for k in range(3) if r[cls][k] > 0))
        for cls in xg.CLASSES))
    try:
        xg.write_report(REPORT, "MI355X", lines)
    except OSError:
        pass


def gpu_params(case):
    return pylbm.cg_params(red=tuple(case.red), blue=tuple(case.blue), sigma=case.sigma, gravity=case.g_r, delta=case.delta,
                           gravity_c=case.g_c, add_source=case.add_source)


def default_bc(lib):
    bc = pylbm.Bc()
    lib.raw.lbm_cg_default_bc(ct.byref(bc))
    return bc


def to_lattice(a, g):
    """[R, C, 9] -> the owned nodes of a flat lattice that is SENTINEL everywhere else"""
    t = poisoned(g)
    owned(t, g)[:] = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(dev())
    return t


def field_outputs(g):
    """the five dense field outputs, every double SENTINEL"""
    out = {}
    for name, n in FIELDS:
        out[name] = torch.zeros(n * g.R * g.C, dtype=torch.float64, device=dev())
        bits(out[name]).fill_(SENTINEL)
    return out


def step(lib, case, g, p, form, edge_rows=3):
    """one step from the post-collision populations p = (p_r, p_b) [R, C, 9] on lattices of geometry g; form: "two_pass",
    "fused" or "parts" (FRAME on a second stream beside INNER).  Returns (pn_r, pn_b device lattices, the fields as device
    tensors) after checking that exactly the owned nodes and every field value were written and the inputs are untouched"""
    bc, prm = default_bc(lib), gpu_params(case)
    src = [to_lattice(a, g) for a in p]
    keep = [t.clone() for t in src]
    dst = [poisoned(g), poisoned(g)]
    f = field_outputs(g)
    gp, bp, pp = ct.byref(g), ct.byref(bc), ct.byref(prm)
    if form == "two_pass":
        lib.cg_stream_moments(_ptr(f["rho_r"]), _ptr(f["rho_b"]), _ptr(f["u"]), _ptr(src[0]), _ptr(src[1]), gp, bp, pp, None)
        lib.cg_stream_collide(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), _ptr(f["rho_r"]), _ptr(f["rho_b"]),
                              _ptr(f["u"]), gp, bp, pp, 0, g.R, _ptr(f["psi"]), _ptr(f["s_nu"]), None)
    elif form == "fused":
        lib.cg_step_fused(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), gp, bp, pp, 0, g.R, _ptr(f["rho_r"]),
                          _ptr(f["rho_b"]), _ptr(f["u"]), _ptr(f["psi"]), _ptr(f["s_nu"]), None)
    else:
        second = torch.cuda.Stream()
        torch.cuda.synchronize()
        for part, stream in ((pylbm.CG_PART_FRAME, ct.c_void_p(second.cuda_stream)), (pylbm.CG_PART_INNER, None)):
            lib.cg_step_fused_part(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), gp, bp, pp, part, edge_rows,
                                   _ptr(f["rho_r"]), _ptr(f["rho_b"]), _ptr(f["u"]), _ptr(f["psi"]), _ptr(f["s_nu"]), stream)
    torch.cuda.synchronize()
    what = f"{case.name} {g.R}x{g.C} pitch {g.row_pitch} {form}"
    for k in range(2):
        assert_write_set(dst[k], g, slice(None), f"{what}: output lattice {k}")
        assert_bits(src[k], keep[k], f"{what}: input lattice {k}")
    for name, t in f.items():
        assert not bool((bits(t) == SENTINEL).any()), f"{what}: field {name} not fully written"
    return dst, f


def host(g, dst, f):
    """the device outputs in the reference's shapes, as test_exact_cg.as_classes takes them"""
    s = dict(col_r=from_lattice(dst[0], g), col_b=from_lattice(dst[1], g))
    for name, n in FIELDS:
        a = f[name].cpu().numpy()
        s[name] = a.reshape(g.R, g.C) if n == 1 else np.ascontiguousarray(a.reshape(2, g.R, g.C).transpose(1, 2, 0))
    return s


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_units_in_the_last_place(lib, oracle, case, layout):
    """a. and b. of the module docstring.  Measured on MI355X: profiles/cg_accuracy.txt."""
    lattice, pitch = LAYOUTS[layout]
    R, C = xg.LATTICES[lattice]
    g = geom(R, C, 0, pitch)
    p, exact = xg.case_data(case, lattice)
    assert np.mean(exact.ill) <= xg.CAP
    want = oracle.cg_step_from_post(oracle_params(case, lattice), *p)
    absent = [np.asarray(exact.mom[..., k] == 0) for k in range(2)]
    assert all(np.mean(a) > 0.05 for a in absent)
    measured = {}
    for form in ("two_pass", "fused"):
        s = host(g, *step(lib, case, g, p, form))
        assert all(np.all(np.isfinite(v)) for v in s.values()), f"{form}: non-finite output"
        if form == "two_pass":
            for k in ("col_r", "col_b", "rho_r", "rho_b", "u", "psi", "s_nu"):
                assert bits_equal(s[k], want[k]), (k, ulp_diff(s[k], want[k]))
        else:
            assert lib.raw.lbm_cg_last_inner_form() == INNER_FORM[lattice]
        if not case.add_source:   # an exactly absent colour stays nine exact zeros
            for k, name in enumerate(("col_r", "col_b")):
                assert np.all(s[name][absent[k]] == 0) and np.all(s[("rho_r", "rho_b")[k]][absent[k]] == 0), (form, name)
        measured[form] = xg.measure(as_classes(s), exact)
        print("%-20s %-16s %-8s %s" % (case.name, layout, form, xg.fmt_row(measured[form])))
    ref, fast = measured["two_pass"], measured["fused"]
    _rows[(case.name, layout)] = (ref, fast)
    for cls in xg.CLASSES:
        assert np.all(np.isfinite(ref[cls] + fast[cls]))
        for stat, rv, fv in zip(("median", "99 %", "maximum"), ref[cls], fast[cls]):
            assert fv <= MARGIN * rv, f"{cls} {stat}: fused {fv:.3f} units > {MARGIN} x two-pass {rv:.3f}"


FORM_CASES = [c for c in CASES if c.name in ("shipped-toml", "density-ratio-100")]


@pytest.mark.parametrize("case", FORM_CASES, ids=[c.name for c in FORM_CASES])
def test_every_kernel_form_writes_the_bits_of_the_default(lib, case):
    """c. of the module docstring"""
    assert len(FORM_CASES) == 2
    lattice = "80x200"
    R, C = xg.LATTICES[lattice]
    g = geom(R, C, 0)
    p, _ = xg.case_data(case, lattice)
    want = step(lib, case, g, p, "fused")
    assert lib.raw.lbm_cg_last_inner_form() == 102

    def same(got, what):
        for k in range(2):
            assert_bits(got[0][k], want[0][k], f"{case.name} {what}: output lattice {k}")
        for name in want[1]:
            assert_bits(got[1][name], want[1][name], f"{case.name} {what}: field {name}")

    try:
        lib.set_tuning(b"cg_big", 0)
        small = step(lib, case, g, p, "fused")
        assert lib.raw.lbm_cg_last_inner_form() == 0
    finally:
        lib.set_tuning(b"cg_big", -1)
    same(small, "16 x 32 inner kernel")
    same(step(lib, case, g, p, "parts", edge_rows=3), "FRAME + INNER, edge_rows = 3")
    wide = geom(R, C, 0, 208)
    padded = step(lib, case, wide, p, "fused")
    assert lib.raw.lbm_cg_last_inner_form() == 102
    for k in range(2):
        assert bits_equal(from_lattice(padded[0][k], wide), from_lattice(want[0][k], g)), (case.name, "row_pitch = 208", k)
    for name in want[1]:
        assert_bits(padded[1][name], want[1][name], f"{case.name} row_pitch = 208: field {name}")


# tuning of the opt-in inner kernels, as tests/test_gpu_cg.py sets it: the walking block of the default build, and the strip
# kernels and the walking tile of an EXPERIMENTS build
OPT_IN = [dict(cg_big=0, cg_strip2=41, cg_rows2=16, cg_split=1), dict(cg_big=0, cg_strip2=42, cg_rows2=9, cg_split=1)]
OPT_IN_EXPERIMENTS = ([dict(cg_big=10, cg_walk_rows=16)]
                      + [dict(cg_big=0, cg_strip=s, cg_rows=16, cg_split=1) for s in (1, 2, 4)]
                      + [dict(cg_big=0, cg_strip2=s, cg_rows2=16, cg_split=1) for s in (11, 21, 31)])


@pytest.mark.parametrize("case", FORM_CASES, ids=[c.name for c in FORM_CASES])
def test_opt_in_kernels_take_the_same_psi_in_the_blend_band(lib, case):
    """Every other inner kernel writes the bits of the default on the edge-state lattice too -- where, unlike on the smooth
    states of tests/test_gpu_cg.py, dozens of nodes lie inside the blend band and take psi from the compensated sums
    (cg_snu_node / cg_psi_node, csrc/cg_fused.hpp): the walking block, and in an EXPERIMENTS build the strip kernels and
    the walking tile.  A form the geometry does not admit falls back to the tile kernel; the walking block must run."""
    lattice = "80x200"
    R, C = xg.LATTICES[lattice]
    g = geom(R, C, 0)
    p, exact = xg.case_data(case, lattice)
    psi = np.asarray(exact.psi[16:64, 32:160, 0], dtype=np.float64)
    assert np.sum(np.abs(psi) <= case.delta) >= 20, "the inner rectangle holds band nodes"
    want = step(lib, case, g, p, "fused")
    ran = set()
    for knobs in OPT_IN + (OPT_IN_EXPERIMENTS if lib.raw.lbm_build_has_experiments() else []):
        try:
            for k, v in knobs.items():
                lib.set_tuning(k.encode(), v)
            got = step(lib, case, g, p, "fused")
            ran.add(lib.raw.lbm_cg_last_inner_form())
        finally:
            for k in knobs:
                lib.set_tuning(k.encode(), -1)
        for k in range(2):
            assert_bits(got[0][k], want[0][k], f"{case.name} {knobs}: output lattice {k}")
        for name in want[1]:
            assert_bits(got[1][name], want[1][name], f"{case.name} {knobs}: field {name}")
    assert 41 in ran, ran
    if lib.raw.lbm_build_has_experiments():
        assert len(ran - {0, 41, 42, 102}) >= 2, ran
