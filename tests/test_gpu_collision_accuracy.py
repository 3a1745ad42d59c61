"""The stated accuracy of the reassociated (default) collisions: BgkFastModel, the BGK stand-in for the delta form,
KbcFastModel and AdeFastModel, per population and per moment, in units in the last place against the 80-bit yardstick of
tests/exact_collide.py -- and the bar is the reference-order kernel's own error on the same nodes (itself bitwise equal
to the oracle, which is pinned to the unmodified reference), not a tolerance chosen in advance.

Per class (one parameter point of a call, exact_collide.cases) and per lattice, through the collide-only entry points
with `form` in the parameter struct and bc = NULL:
  a. reference order: populations and moments bitwise equal to the oracle -- at omega = 1, s2 = 2, rho 0.2 .. 5 and
     Mach 0.25 too;
  b. reassociated: everything finite, and median, 99th percentile and maximum of the per-node error each at most 1.5 x
     the same statistic of the reference-order GPU result, separately for the populations (f*, g*) and the moments
     (rho, u, C).  Both forms are chains of correctly rounded operations whose medians and 99th percentiles differ by
     about +-15 % on 20 000 nodes; the reassociated ones take a reciprocal (rcp_f64, d2q9.hpp) where the reference
     divides.  The margin is over the reference, not over the code under test;
  c. hot path: one stream+collide call on the inverse-streamed state writes exactly the bits of the collide-only call,
     in both forms -- the multi-step windows are tied to single steps bitwise elsewhere, so the unit bound reaches the
     kernels the benchmark runs.
The lattices: 7 x 6 (fewer nodes than one workgroup) and 48 x 430 = 20 640 nodes (no multiple of 256) with row_pitch =
C + 2 and the plane padding of ade_util.geom; every double outside the owned nodes is SENTINEL before and after.
Nodes with C = 0 exactly (all nine g_q = 0; 4 % by the generator) must give nine zeros and conc = 0 in both forms and
are left out of the unit statistics, where their unit is 0: the only carve-out.
The measured table goes to profiles/collision_accuracy.txt."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import exact_collide as xc  # noqa: E402
from collide_reference import reference_order  # noqa: E402
import pylbm  # noqa: E402
from ade_util import (SENTINEL, assert_bits, assert_write_set, bits, from_lattice, geom, moment_fields, owned,  # noqa: E402
                      poisoned)
from gpu_util import bits_equal, dev, ulp_diff  # noqa: E402
from pylbm import _ptr  # noqa: E402

REPORT = os.path.join(ROOT, "profiles", "collision_accuracy.txt")
CASES = xc.cases()
LATTICES = {"7x6": (7, 6, 0), "48x430": (48, 430, 432)}   # R, C, row pitch (0: dense)
FORMS = {"reference_order": pylbm.FORM_REFERENCE_ORDER, "reassociated": pylbm.FORM_REASSOCIATED}
MARGIN = 1.5
_rows = {}


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if len(_rows) != len(CASES) * len(LATTICES):   # a full run only
        return
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                timeout=10).stdout.strip() or "unknown"
    except (OSError, subprocess.SubprocessError):
        commit = "unknown"
    lines = [f"tree on commit {commit}; per class and lattice: reference order | reassociated"]
    for (name, lat), (ref, fast) in _rows.items():
        lines.append("%-44s %-7s pop %s | %s   mom %s | %s" % (name, lat, xc.fmt(ref[0]), xc.fmt(fast[0]), xc.fmt(ref[1]),
                                                              xc.fmt(fast[1])))
    try:
        xc.write_section(REPORT, "MI355X", lines)
    except OSError:
        pass


def to_lattice(a, g):
    """[R C, 9] nodes -> the owned nodes of a flat lattice that is SENTINEL everywhere else"""
    t = poisoned(g)
    owned(t, g)[:] = torch.from_numpy(np.ascontiguousarray(a.reshape(g.R, g.C, 9).transpose(2, 0, 1))).to(dev())
    return t


def params(case, form):
    """(fluid parameters, scalar parameters or None) of a case in a form"""
    if case.cls.endswith("kbc"):
        fluid = pylbm.KbcParams(case.fluid, form=form)
    else:
        fluid = pylbm.BgkParams(case.fluid, 0, case.delta_form, form=form)
    return fluid, (pylbm.AdeParams(case.omega_g, case.w, form=form) if case.cls.startswith("ade") else None)


def call(lib, case, form, g, src, dst, mom, streamed):
    """the collide-only entry point of the case's model (streamed: its stream+collide on all rows), bc = NULL"""
    fluid, scalar = params(case, form)
    gp, m = ct.byref(g), [_ptr(t) for t in mom]
    rows = (0, g.R) if streamed else ()
    if case.cls == "bgk":
        fn = lib.bgk_stream_collide if streamed else lib.bgk_collide
        fn(_ptr(dst[0]), _ptr(src[0]), gp, None, ct.byref(fluid), *rows, *m, None)
    elif case.cls == "kbc":
        fn = lib.kbc_stream_collide if streamed else lib.kbc_collide
        fn(_ptr(dst[0]), _ptr(src[0]), gp, None, ct.byref(fluid), *rows, *m, None)
    elif case.cls == "ade_bgk":
        fn = lib.ade_stream_collide if streamed else lib.ade_collide
        fn(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), gp, None, ct.byref(fluid), ct.byref(scalar), *rows, *m, None)
    else:
        fl = pylbm.AdeFluid(fluid)
        if streamed:
            lib.ade_stream_collide_m(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), gp, None, ct.byref(fl),
                                     ct.byref(scalar), None, None, *rows, *m, None)
        else:
            lib.ade_collide_m(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), gp, None, ct.byref(fl),
                              ct.byref(scalar), None, *m, None)
    torch.cuda.synchronize()


def run(lib, case, form, g, nodes, streamed=False):
    """one call on the pre-collision nodes [[R C, 9], ...] (f, then g); returns the device outputs (lattices, moments)
    after checking that exactly the owned nodes were written and the inputs are untouched"""
    pre = [np.ascontiguousarray(a).reshape(g.R, g.C, 9) for a in nodes]
    if streamed:   # the inverse-streamed state: p_old_q(r, c) = F_q(r + cx_q, c + cy_q), wrapped
        pre = [np.stack([np.roll(a[..., q], (-xc.CX[q], -xc.CY[q]), axis=(0, 1)) for q in range(9)], axis=-1) for a in pre]
    src = [to_lattice(a.reshape(-1, 9), g) for a in pre]
    keep = [t.clone() for t in src]
    dst = [poisoned(g) for _ in src]
    mom = moment_fields(g)[:1 + len(src)]   # rho, u (and C)
    call(lib, case, form, g, src, dst, mom, streamed)
    what = f"{case.name} {g.R}x{g.C} form {form}" + (" streamed" if streamed else "")
    for k, t in enumerate(dst):
        assert_write_set(t, g, slice(None), f"{what}: output lattice {k}")
        assert_bits(src[k], keep[k], f"{what}: input lattice {k}")
    for k, t in enumerate(mom):
        assert not bool((bits(t) == SENTINEL).any()), f"{what}: moment field {k} not fully written"
    return dst, mom


def host(g, dst, mom):
    """(pop [n, 9 or 18], mom [n, 3 or 4]) of the device outputs"""
    n = g.R * g.C
    pop = np.concatenate([from_lattice(t, g).reshape(n, 9) for t in dst], axis=1)
    cols = [mom[0].cpu().numpy().reshape(n, 1), mom[1].cpu().numpy().reshape(2, n).T]
    if len(mom) == 3:
        cols.append(mom[2].cpu().numpy().reshape(n, 1))
    return pop, np.concatenate(cols, axis=1)


@pytest.mark.parametrize("lattice", list(LATTICES))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_units_in_the_last_place(lib, oracle, case, lattice):
    """a. and b. of the module docstring.  Measured on MI355X: profiles/collision_accuracy.txt."""
    R, C, pitch = LATTICES[lattice]
    g = geom(R, C, 0, pitch)
    n = R * C
    st, exact = xc.case_data(case)
    st = {k: v[:n] for k, v in st.items()}
    exact = xc.Exact(*[a[:n] for a in exact])
    nodes = [st["f"]] + ([st["g"]] if "g" in st else [])
    keep = None
    if "zero_c" in st:
        keep = ~st["zero_c"]
        assert 0 < np.sum(st["zero_c"]) <= 0.05 * n
    want_pop, want_mom = reference_order(oracle, case, st)
    measured = {}
    for name, form in FORMS.items():
        pop, mom = host(g, *run(lib, case, form, g, nodes))
        assert np.all(np.isfinite(pop)) and np.all(np.isfinite(mom)), f"{name}: non-finite output"
        if keep is not None:   # C = 0 exactly: nine zeros and conc = 0
            assert np.all(pop[~keep, 9:] == 0) and np.all(mom[~keep, 3] == 0), f"{name}: C = 0 nodes"
        if name == "reference_order":
            assert bits_equal(pop, want_pop), ("populations", ulp_diff(pop, want_pop))
            assert bits_equal(mom, want_mom), ("moments", ulp_diff(mom, want_mom))
        measured[name] = xc.measure(pop, mom, exact, keep)
        print("%-44s %-7s %-15s pop %s   mom %s" % (case.name, lattice, name, xc.fmt(measured[name][0]),
                                                    xc.fmt(measured[name][1])))
    ref, fast = measured["reference_order"], measured["reassociated"]
    _rows[(case.name, lattice)] = (ref, fast)
    assert np.all(np.isfinite(ref[0] + ref[1] + fast[0] + fast[1]))
    for what, r, f in (("populations", ref[0], fast[0]), ("moments", ref[1], fast[1])):
        for stat, rv, fv in zip(("median", "99 %", "maximum"), r, f):
            assert fv <= MARGIN * rv, f"{what} {stat}: reassociated {fv:.3f} units > {MARGIN} x reference order {rv:.3f}"


HOT = [c for c in CASES if c.name in ("bgk-omega1.999-delta0", "bgk-omega1.0-delta1", f"kbc-s2_{xc.S2_SHEAR:.6g}", "kbc-s2_2",
                                      "ade_bgk-1.2-omega_g1.999-w0.003", "ade_kbc-2-omega_g0.6-w0.003")]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", HOT, ids=[c.name for c in HOT])
def test_hot_path_writes_the_bits_of_collide_only(lib, case, form):
    """c. of the module docstring on a periodic dense 48 x 512 lattice (the vector kernels of the single step: C even and
    >= 64): lbm_bgk_stream_collide, lbm_kbc_stream_collide, lbm_ade_stream_collide and lbm_ade_stream_collide_m with a KBC
    fluid.  No other test compares a single step with the collide-only call bit for bit in the reassociated form."""
    assert len(HOT) == 6
    R, C = 48, 512
    g = geom(R, C, 0)
    st = xc.states(case.cls, R * C, case.seed + 1000, case.w or (0.0, 0.0))
    nodes = [st["f"]] + ([st["g"]] if "g" in st else [])
    want = run(lib, case, FORMS[form], g, nodes)
    got = run(lib, case, FORMS[form], g, nodes, streamed=True)
    for k, (a, b) in enumerate(zip(got[0] + got[1], want[0] + want[1])):
        assert_bits(a, b, f"{case.name} {form}: output {k} of the streamed call against collide-only")
