"""GPU suite, the fluid + scalar step with the entropic KBC collision as the fluid (lbm_ade_fluid; lbm_ade_collide_m,
lbm_ade_stream_collide_m, lbm_ade_solver_create_m; ade_kbc.hpp k_ade_kbc_stream_collide).

The yardstick is `oracle_loop` of tests/ade_kbc_util.py: one driver iteration composed on the CPU from the oracle's
kbc::collide on the populations' own moments and the scalar half and wall rules of tests/ade_util.py; it never calls the
library under test, is computed once per case (yardstick(), cached, read-only) and is asserted finite wherever it is used
-- the start states are off equilibrium (ade_util.initial_state), since KBC's gamma is 0/0 on a lattice at equilibrium.
Bitwise means equal bit patterns.  The only tolerances: the reassociated form against the reference order, relative L2
<= 1e-12 after 20 steps (the bound tests/test_gpu_kbc.py states for the reassociated KBC collision at <= 20 steps), and
the scalar mass, 1e-12 relative (the bound of test_scalar_mass_is_conserved in tests/test_gpu_ade.py).
Shapes: 6 x 8, 96 x 70 and 48 x 1040 at a row pitch of 1056 (three 512-column tiles per row), unless a test names another."""
import ctypes as ct
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ade_calls  # noqa: E402
import ade_kbc_util as kbc  # noqa: E402
import diag_reference as ref  # noqa: E402
import pylbm  # noqa: E402
from ade_slab_util import body_table  # noqa: E402
from ade_util import (GBC, W, Body, alloc, assert_bits, assert_state_bits, assert_write_set, bits, build_sbc,  # noqa: E402
                      geom, initial_state, moment_fields, owned, poisoned, random_lattice, to_lattice)
from ade_util import params as bgk_params  # noqa: E402
from gpu_util import bits_equal, dev  # noqa: E402
from proc_util import run_driver  # noqa: E402
from pylbm import _ptr  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FORMS = {"reference_order": REF, "reassociated": FAST}
BB, SP = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_NEG, COL_NEG = pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_NEG
S2, OMEGA_G = kbc.S2, kbc.OMEGA_G
SHAPES = {"6x8": (6, 8, 0), "96x70": (96, 70, 0), "48x1040_padded": (48, 1040, 1056)}
EDGES = {"periodic": pylbm.Bc(), "bounce_back_columns": pylbm.Bc(col_lo=BB, col_hi=BB),
         "bounce_back_rows_specular_columns": pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=SP, col_hi=SP), "box": GBC}
ITERATIONS = (1, 2, 20)


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(autouse=True)
def _default_knobs_afterwards(lib):
    yield
    lib.reset_tuning()


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _yardstick(R, C, edges, fixed_key, iterations):
    from pyoracle import Oracle
    orc = Oracle()
    f0, g0 = initial_state(orc, R, C, seed=R * C)
    fixed = fixed_spec(EDGES[edges], R, C) if fixed_key else {}
    fixed_np = {k: (v[1] if isinstance(v, tuple) else np.full(C if k.startswith("row") else R, float(v))) for k, v in fixed.items()}
    out, f, g, done = {0: _frozen(dict(f=f0, g=g0))}, f0, g0, 0
    for n in iterations:
        st = kbc.oracle_loop(orc, f, g, S2, OMEGA_G, W, n - done, EDGES[edges], fixed_np)
        assert kbc.finite(st), f"the yardstick is not finite after {n} iterations"
        f, g, done = st["f"], st["g"], n
        out[n] = _frozen(st)
    return out


def yardstick(R, C, edges, fixed=False, iterations=ITERATIONS):
    """{0: the start state (f, g), n: the state after n driver iterations (f, g, rho, u, C)}, computed once, read-only"""
    return _yardstick(R, C, edges, fixed, tuple(iterations))


def fixed_spec(bc, R, C):
    """FIXED on every wall edge of bc, constants and profiles mixed, corners included"""
    spec, rows = {}, bc.row_lo == BB
    if rows:
        spec["row_lo"] = 7e-4
        spec["row_hi"] = ("profile", np.linspace(2e-4, 1.2e-3, C))
    if bc.col_lo in (BB, SP):
        spec["col_lo"] = ("profile", np.linspace(1.5e-3, 3e-4, R)) if rows else 2e-3
        spec["col_hi"] = 0.0 if rows else ("profile", np.linspace(1e-4, 9e-4, R))
    return spec


def solver(lib, R, C, form, bc=None, s2=S2, **kw):
    return pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(s2, form), pylbm.AdeParams(OMEGA_G, W, form=form), bc=bc, **kw)


def post_collision(oracle, state, g):
    """the post-collision pair of a pre-collision state as device lattices, and the moments a raw step writes for it"""
    c = kbc.collide(oracle, state["f"], state["g"], S2, OMEGA_G, W)
    m = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev()) for a in (c["rho"], c["u"].transpose(2, 0, 1), c["C"])]
    return (to_lattice(c["fc"], g), to_lattice(c["gc"], g)), m


def raw_steps(lib, g, bc, prm, src, steps, sbc=None, table=None, with_moments=True):
    cur, m = src, (moment_fields(g) if with_moments else None)
    for _ in range(steps):
        cur = ade_calls.full_step(lib, "_m", g, bc, prm, *cur, sbc=sbc, iwalls=table, moments=m)
    torch.cuda.synchronize()
    return cur, m


def assert_same_run(got, want, what):
    for k, name in enumerate("fg"):
        assert_bits(got[0][k], want[0][k], f"{what}: {name}")
    if got[1] is not None:
        for k, name in enumerate(("rho", "u", "C")):
            assert_bits(got[1][k], want[1][k], f"{what}: {name}")


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


# ---- 1. the reference order is the yardstick ------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", ["periodic", "bounce_back_columns", "bounce_back_rows_specular_columns"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reference_order_is_the_yardstick(lib, oracle, shape, edges):
    """after 1, 2 and 20 iterations, f, g, rho, u, C bit for bit: the raw step on the (padded) lattice from the
    yardstick's own post-collision state, and the context from the pre-collision state (its collide-only first
    iteration, its fused steps, the lazily streamed level of get_state)"""
    R, C, pitch = SHAPES[shape]
    bc, yard = EDGES[edges], yardstick(R, C, edges)
    g, prm = geom(R, C, 0, pitch), kbc.params(REF)
    cur, _ = post_collision(oracle, yard[0], g)
    m, done = moment_fields(g), 0
    sv = solver(lib, R, C, REF, bc)
    try:
        sv.set_state(yard[0]["f"], yard[0]["g"])
        for n in ITERATIONS:
            for _ in range(n - done):
                cur = ade_calls.full_step(lib, "_m", g, bc, prm, *cur, moments=m)
            sv.step(n - done)
            done = n
            torch.cuda.synchronize()
            assert_same_run((cur, m), post_collision(oracle, yard[n], g), f"{shape} {edges}: {n} raw steps")
            assert_state_bits(sv.get_state(), yard[n], f"{shape} {edges}: context after {n} iterations")
    finally:
        sv.close()


# ---- 2. the fluid is the existing KBC fluid -------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("edges", ["periodic", "box"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_fluid_half_is_lbm_kbc_stream_collide(lib, shape, edges, form):
    """f of lbm_ade_stream_collide_m == lbm_kbc_stream_collide on the same lattice, edges and form, and its rho, u"""
    R, C, pitch = SHAPES[shape]
    g, bc = geom(R, C, 0, pitch), EDGES[edges]
    fo, go = random_lattice(g, 21), random_lattice(g, 22)
    m = moment_fields(g)
    fn, _ = ade_calls.full_step(lib, "_m", g, bc, kbc.params(FORMS[form]), fo, go, moments=m)
    want, rho, u = alloc(g), torch.zeros(R * C, dtype=torch.float64, device=dev()), torch.zeros(2 * R * C, dtype=torch.float64, device=dev())
    prm = pylbm.KbcParams(S2, FORMS[form])
    lib.kbc_stream_collide(_ptr(want), _ptr(fo), ct.byref(g), ct.byref(bc), ct.byref(prm), 0, R, _ptr(rho), _ptr(u), None)
    torch.cuda.synchronize()
    assert_bits(fn, want, f"{shape} {edges} {form}: f")
    assert_bits(m[0], rho, f"{shape} {edges} {form}: rho")
    assert_bits(m[1], u, f"{shape} {edges} {form}: u")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("edges", ["periodic", "bounce_back_columns"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_twenty_steps_leave_the_f_of_the_kbc_solver(lib, shape, edges, form):
    """AdeSolver.get_state()["f"] == Solver(model = KBC).get_f() from the same start: the scalar is passive"""
    R, C, _ = SHAPES[shape]
    start = yardstick(R, C, edges)[0]
    sv = solver(lib, R, C, FORMS[form], EDGES[edges])
    fl = pylbm.Solver(lib, pylbm.MODEL_KBC, R, C, pylbm.KbcParams(S2, FORMS[form]), bc=EDGES[edges])
    try:
        sv.set_state(start["f"], start["g"])
        fl.set_f(start["f"])
        sv.step(20)
        fl.step(20)
        assert bits_equal(sv.get_state()["f"], fl.get_f())
    finally:
        sv.close()
        fl.close()


# ---- 3. model = BGK through the `_m` entry points is the existing entry points ---------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_model_bgk_is_the_existing_call(lib, oracle, form):
    R, C, pitch = SHAPES["48x1040_padded"]
    g, prm = geom(R, C, 0, pitch), bgk_params(FORMS[form])
    fluid = pylbm.AdeFluid(prm[0])
    sbc, _ = build_sbc(fixed_spec(GBC, R, C), R, C)
    table = body_table(lib, R, C, (FIXED, 2e-3))
    fo, go = random_lattice(g, 31), random_lattice(g, 32)
    want_m, got_m = moment_fields(g), moment_fields(g)
    want = ade_calls.full_step(lib, "_w", g, GBC, prm, fo, go, sbc=sbc, iwalls=table, moments=want_m)
    got = ade_calls.full_step(lib, "_m", g, GBC, (fluid, prm[1]), fo, go, sbc=sbc, iwalls=table, moments=got_m)
    torch.cuda.synchronize()
    assert_same_run((got, got_m), (want, want_m), f"{form}: lbm_ade_stream_collide_m against _w")
    cw, cg, cm_w, cm_g = (alloc(g), alloc(g)), (alloc(g), alloc(g)), moment_fields(g), moment_fields(g)
    ade_calls.collide(lib, "_b", g, GBC, prm, cw, (fo, go), sbc=sbc, moments=cm_w)
    ade_calls.collide(lib, "_m", g, GBC, (fluid, prm[1]), cg, (fo, go), sbc=sbc, moments=cm_g)
    torch.cuda.synchronize()
    assert_same_run((cg, cm_g), (cw, cm_w), f"{form}: lbm_ade_collide_m against _b")
    table.close()
    # the context: the same state and the same launch count
    R, C, _ = SHAPES["96x70"]
    f0, g0 = initial_state(oracle, R, C, seed=5)
    states, launches = [], []
    for fl in (prm[0], fluid):
        sv = pylbm.AdeSolver(lib, R, C, fl, prm[1], bc=GBC)
        sv.set_state(f0, g0)
        sv.step(7)
        states.append(sv.get_state())
        launches.append(sv.launches())
        sv.close()
    assert_state_bits(states[1], states[0], f"{form}: lbm_ade_solver_create_m against lbm_ade_solver_create")
    assert launches[0] == launches[1] == 1 + 6 * 2


# ---- 4. the reassociated form against the reference order ------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reassociated_form_agrees_with_the_reference_order(lib, shape):
    """relative L2 <= 1e-12 on f and on g after 20 steps.  Measured on MI355X, the largest of the three shapes: f 1.1e-15,
    g 2.1e-15."""
    R, C, _ = SHAPES[shape]
    start, got = yardstick(R, C, "periodic")[0], {}
    for name, form in FORMS.items():
        sv = solver(lib, R, C, form)
        sv.set_state(start["f"], start["g"])
        sv.step(20)
        got[name] = sv.get_state()
        sv.close()
    errs = {k: rel_l2(got["reassociated"][k], got["reference_order"][k]) for k in ("f", "g")}
    print(f"{shape}: reassociated against reference order after 20 steps, relative L2:", errs)
    assert not bits_equal(got["reassociated"]["f"], got["reference_order"]["f"])  # the two forms are different code
    assert max(errs.values()) <= 1e-12, errs


# ---- 5. launch variants ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("edges", ["periodic", "box"])
def test_every_launch_variant(lib, oracle, edges, form):
    """48 x 1040: all four `nt` settings x grid_cap 0, 1, 7 (three tiles per row: the stride of 1 and 7 workgroups walks
    across rows), with the moment outputs and with them NULL: two steps, each bit for bit the default launch, which in
    the reference order is the yardstick"""
    R, C, pitch = SHAPES["48x1040_padded"]
    g, bc, prm = geom(R, C, 0, pitch), EDGES[edges], kbc.params(FORMS[form])
    yard = yardstick(R, C, edges)
    src, _ = post_collision(oracle, yard[0], g)
    base = raw_steps(lib, g, bc, prm, src, 2)
    if FORMS[form] == REF:
        assert_same_run(base, post_collision(oracle, yard[2], g), f"{edges}: default launch against the yardstick")
    for with_moments in (True, False):
        for nt in (0, 1, 2, 3):
            for cap in (0, 1, 7):
                lib.set_tuning(b"nt", nt)
                lib.set_tuning(b"grid_cap", cap)
                got = raw_steps(lib, g, bc, prm, src, 2, with_moments=with_moments)
                assert_same_run(got, base, f"{edges} {form} nt={nt} grid_cap={cap} moments={with_moments}")


@pytest.mark.parametrize("edges", ["periodic", "box"])
@pytest.mark.parametrize("R,C", [(1, 8), (2, 8), (6, 2), (1, 2)])
def test_the_smallest_shapes(lib, R, C, edges):
    """R = 1 (a row is its own neighbour and both wall rows at once), R = 2, C = 2 (a row's only pair is its first and its
    last): 9 iterations through the context; reference order == the yardstick bit for bit, the reassociated form within
    1e-12 relative L2 of it on f and g"""
    yard = yardstick(R, C, edges, iterations=(9,))
    for name, form in FORMS.items():
        sv = solver(lib, R, C, form, EDGES[edges])
        sv.set_state(yard[0]["f"], yard[0]["g"])
        sv.step(9)
        got = sv.get_state()
        sv.close()
        if form == REF:
            assert_state_bits(got, yard[9], f"{R}x{C} {edges}")
        else:
            errs = {k: rel_l2(got[k], yard[9][k]) for k in ("f", "g")}
            print(f"{R}x{C} {edges}: reassociated against the yardstick after 9 steps, relative L2:", errs)
            assert max(errs.values()) <= 1e-12, errs


# ---- 6. the scalar's FIXED walls and the interior-wall table ---------------------------------------------------------------
@pytest.mark.parametrize("edges", ["bounce_back_columns", "bounce_back_rows_specular_columns", "box"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fixed_scalar_walls_are_the_yardstick(lib, shape, edges):
    """every wall edge FIXED, constants and profiles, corners included: 8 iterations in the reference order, bit for bit"""
    R, C, _ = SHAPES[shape]
    bc = EDGES[edges]
    yard = yardstick(R, C, edges, fixed=True, iterations=(8,))
    plain = yardstick(R, C, edges, iterations=(8,)) if shape == "6x8" else None
    sbc, _ = build_sbc(fixed_spec(bc, R, C), R, C)
    sv = solver(lib, R, C, REF, bc, scalar_bc=sbc)
    try:
        sv.set_state(yard[0]["f"], yard[0]["g"])
        sv.step(8)
        assert_state_bits(sv.get_state(), yard[8], f"{shape} {edges} FIXED")
    finally:
        sv.close()
    if plain is not None:
        assert not bits_equal(plain[8]["g"], yard[8]["g"])  # the walls are felt


BODY_R, BODY_C = 48, 64
BODY_BC = pylbm.Bc(row_lo=BB)


def body_numpy(rule):
    seg = [((slice(None), 20), COL_NEG), ((5, slice(20, 31)), ROW_NEG), ((29, slice(20, 31)), ROW_NEG)]
    return Body(seg, seg, *rule)


@pytest.mark.parametrize("case", ["no_flux", "absorbing", "fixed"])
def test_interior_walls_are_the_yardstick(lib, oracle, case):
    """the 68-node body on 48 x 64 under a bounce-back first row (the column wall stands on it), its g slots NO_FLUX,
    absorbing (FIXED at 0) or FIXED at 2e-3 beside a FIXED first row: 8 iterations in the reference order, bit for bit"""
    R, C = BODY_R, BODY_C
    rule = {"no_flux": (NO_FLUX, 0.0), "absorbing": (FIXED, 0.0), "fixed": (FIXED, 2e-3)}[case]
    spec = {"row_lo": 7e-4} if case == "fixed" else {}
    sbc, fixed = build_sbc(spec, R, C) if spec else (None, {})
    f0, g0 = initial_state(oracle, R, C, seed=11)
    want = kbc.oracle_loop(oracle, f0, g0, S2, OMEGA_G, W, 8, BODY_BC, fixed, body_numpy(rule))
    plain = kbc.oracle_loop(oracle, f0, g0, S2, OMEGA_G, W, 8, BODY_BC, fixed, Body([], []))
    assert kbc.finite(want) and not bits_equal(want["g"], plain["g"])
    table = body_table(lib, R, C, rule)
    assert table.count() == 68
    sv = solver(lib, R, C, REF, BODY_BC, scalar_bc=sbc, walls=table)
    try:
        sv.set_state(f0, g0)
        sv.step(8)
        assert sv.launches() == 1 + 7 * 3  # interior, edge pass, table pass
        assert_state_bits(sv.get_state(), want, f"body {case}")
    finally:
        sv.close()
        table.close()


# ---- 7. write sets ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape,rows", [("6x8", (2, 5)), ("48x1040_padded", (7, 19)), ("48x1040_padded", (0, 48))])
def test_a_row_range_writes_exactly_its_rows(lib, shape, rows, form):
    """NaN-poisoned targets, walls all round, the body's table, grid_cap = 7: rows [row_begin, row_end) of both lattices
    (no padding, no other row) and of the three moment fields, each double the full launch's"""
    R, C, pitch = SHAPES[shape]
    g, prm = geom(R, C, 0, pitch), kbc.params(FORMS[form])
    table = body_table(lib, R, C, (FIXED, 2e-3)) if R >= 48 else None
    src = random_lattice(g, 41), random_lattice(g, 42)
    want_m = moment_fields(g)
    want = ade_calls.full_step(lib, "_m", g, GBC, prm, *src, iwalls=table, moments=want_m)
    lib.set_tuning(b"grid_cap", 7)
    dst, m = (poisoned(g), poisoned(g)), moment_fields(g)
    ade_calls.step_into(lib, "_m", g, GBC, prm, dst, src, rows, iwalls=table, moments=m)
    torch.cuda.synchronize()
    span = list(range(*rows))
    for k, name in enumerate("fg"):
        assert_write_set(dst[k], g, span, f"{shape} rows {rows} {form}: {name}")
        assert_bits(owned(dst[k], g)[:, span], owned(want[k], g)[:, span], f"{shape} rows {rows} {form}: {name}")
    for t, w, planes, name in zip(m, want_m, (1, 2, 1), ("rho", "u", "C")):
        t, w = t.view(planes, R, C), w.view(planes, R, C)
        written = bits(t) != moment_sentinel()
        expect = torch.zeros_like(written)
        expect[:, span] = True
        assert torch.equal(written, expect), f"{shape} rows {rows} {form}: write set of {name}"
        assert_bits(t[:, span], w[:, span], f"{shape} rows {rows} {form}: {name}")
    if table is not None:
        table.close()


def moment_sentinel():
    from ade_util import SENTINEL
    return SENTINEL


# ---- 8. the context --------------------------------------------------------------------------------------------------------
def test_launches_per_step_and_graph_replay(lib):
    """one launch per step on a periodic box, two with wall edges (+1 for the collide-only first iteration); ten steps
    captured on a created stream and replayed == ten direct steps, bit for bit"""
    R, C, _ = SHAPES["96x70"]
    start = yardstick(R, C, "box")[0]
    for edges, per_step in (("periodic", 1), ("box", 2)):
        sv = solver(lib, R, C, pylbm.FORM_DEFAULT, EDGES[edges])
        sv.set_state(start["f"], start["g"])
        sv.step(11)
        assert sv.launches() == 1 + 10 * per_step
        if edges == "box":
            want = sv.get_state()
        sv.close()
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        sv = solver(lib, R, C, pylbm.FORM_DEFAULT, GBC, stream=st.value)
        sv.set_state(start["f"], start["g"])
        sv.step(1)  # the collide-only first iteration, direct
        sv.sync()
        lib.graph_begin_capture(st)
        sv.step(10)
        lib.graph_end_capture(st, ct.byref(graph))
        lib.graph_launch(graph, 1, st)
        lib.stream_sync(st)
        assert_state_bits(sv.get_state(), want, "graph replay")
        sv.close()
    finally:
        if graph:
            lib.graph_destroy(graph)
        lib.stream_destroy(st)


def moments_table(s, profile=None):
    return ref.row_table(s["rho"], np.ascontiguousarray(s["u"][..., 0]), np.ascontiguousarray(s["u"][..., 1]), s["C"], profile)


def test_diag_is_the_fold_of_get_state(lib):
    R, C, _ = SHAPES["96x70"]
    start = yardstick(R, C, "box")[0]
    sbc, _ = build_sbc({"row_lo": 1e-3, "col_hi": 0.0}, R, C)
    sv = solver(lib, R, C, pylbm.FORM_DEFAULT, GBC, scalar_bc=sbc)
    try:
        sv.set_state(start["f"], start["g"])
        profile = 0.01 * np.random.default_rng(9).standard_normal(C)
        pd = torch.tensor(profile, dtype=torch.float64, device=dev())
        for n in (0, 1, 12):  # the state as given, after the collide-only iteration, after fused steps
            sv.step(n)
            s = sv.get_state()
            want = moments_table(s, profile)
            for a, b in ((0, R), (R // 3, R - R // 4)):
                got, table = sv.diag(profile=pd, row_begin=a, row_end=b, table=True)
                assert ref.bits_equal(got, ref.fold_table(want, a, b)), f"after {n} more steps, rows [{a}, {b})"
                assert ref.bits_equal(table[:, a:b], want[:, a:b])
                assert got[ref.NONFINITE] == 0.0
    finally:
        sv.close()


def test_run_until_stops_where_the_host_loop_stops(lib):
    """the watched value is the mean of C over a row range of the streamed state; the rule fires at the same step with
    the same last value as a host loop over get_state"""
    R, C = 24, 70
    start = yardstick(R, C, "periodic", iterations=())[0]
    bc = pylbm.Bc(row_lo=BB, row_hi=BB)
    rule = dict(quantity=pylbm.DIAG_SUM_C, interval=10, offset=3, tolerance=1e-9, old_value=1.0, row_begin=2, row_end=20)

    def make():
        sv = solver(lib, R, C, pylbm.FORM_DEFAULT, bc)
        sv.set_state(start["f"], start["g"])
        return sv

    sv = make()
    try:
        got = sv.run_until(pylbm.Converge(**rule), 47)
    finally:
        sv.close()
    sv = make()
    try:
        t, old, last, conv = 0, 1.0, 1.0, False
        while t < 47:
            if t > 0 and t % 10 == 3:
                last = ref.fold_table(moments_table(sv.get_state()), 2, 20)[ref.SUM_C] / (18.0 * C)
                if abs(last / old - 1.0) < 1e-9:
                    conv = True
                    break
                old = last
            n = min(t - t % 10 + 3 + (10 if t % 10 >= 3 else 0), 47) - t
            sv.step(n)
            t += n
    finally:
        sv.close()
    assert got[0] == t and got[1] == conv and np.float64(got[2]).view(np.uint64) == np.float64(last).view(np.uint64)


def test_what_a_kbc_context_refuses(lib, oracle):
    """buoyancy with a non-zero beta, a non-empty open table and the wall exchange: LBM_ERR_INVALID, the message names the
    feature and the model; beta = (0, 0) and an empty table are the passive step and pass"""
    R, C = 16, 16
    sv = solver(lib, R, C, pylbm.FORM_DEFAULT, pylbm.Bc(row_hi=BB))
    empty = pylbm.AdeOpenBoundary(lib, R, C).finalize()
    channel = pylbm.AdeOpenBoundary(lib, R, C).channel(0.02, 1e-3, 4).finalize()
    try:
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_set_buoyancy: buoyancy .* KBC fluid"):
            sv.set_buoyancy(pylbm.AdeBuoyancy((1e-3, 0.0), 0.0))
        sv.set_buoyancy(pylbm.AdeBuoyancy((0.0, 0.0), 0.5))
        sv.set_buoyancy(None)
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_set_open: open boundaries .* KBC fluid"):
            sv.set_open(channel)
        sv.set_open(empty)
        sv.set_open(None)
        f0, g0 = initial_state(oracle, R, C, seed=2)
        sv.set_state(f0, g0)
        sv.step(2)
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_wall_exchange: the wall exchange .* KBC fluid"):
            sv.wall_exchange()
        assert sv.launches() == 1 + 2  # the refusals enqueued nothing and the passive setters changed no launch
    finally:
        sv.close()
        empty.close()
        channel.close()


# ---- 9. physics ------------------------------------------------------------------------------------------------------------
def test_dye_in_the_under_resolved_double_shear_layer(lib, oracle):
    """64 x 64 double shear layer (Oracle.kbc_shear_init, the reference driver's start: eval_equilibrium with the u^2 terms
    left out) at nu = 1.7e-4 with a Gaussian blob of dye, 500 steps in the default form: nothing non-finite, and the scalar
    mass SUM_C conserved to 1e-12 relative -- the bound of test_scalar_mass_is_conserved (tests/test_gpu_ade.py)"""
    R = C = 64
    s2 = 1.0 / (0.5 + 3 * 1.7e-4)
    m0, m1 = oracle.kbc_shear_init(R, C)
    f0 = oracle.kbc_equilibrium(m0, m1, use_zero_u2=True)
    r, c = np.meshgrid(np.arange(R, dtype=float), np.arange(C, dtype=float), indexing="ij")
    conc = 1e-3 * np.exp(-((r - 0.5 * R) ** 2 + (c - 0.5 * C) ** 2) / (2 * 6.0 ** 2))
    g0 = oracle.equilibrium(m1 + np.asarray(W), conc)
    sv = solver(lib, R, C, pylbm.FORM_DEFAULT, s2=s2)
    try:
        sv.set_state(f0, g0)
        before = sv.diag()
        sv.step(500)
        after = sv.diag()
        s = sv.get_state()
    finally:
        sv.close()
    print(f"double shear layer, 500 steps: SUM_C {before[ref.SUM_C]!r} -> {after[ref.SUM_C]!r}, "
          f"relative change {abs(after[ref.SUM_C] / before[ref.SUM_C] - 1):.3e}; max |u| {np.abs(s['u']).max():.4f}")
    assert before[ref.NONFINITE] == 0.0 and after[ref.NONFINITE] == 0.0
    assert np.all(np.isfinite(s["f"])) and np.all(np.isfinite(s["g"]))
    assert abs(after[ref.SUM_C] - before[ref.SUM_C]) <= 1e-12 * before[ref.SUM_C]
    assert not bits_equal(s["C"], conc)  # the dye has moved


# ---- 10. the driver --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walls", ["0", "2"])
def test_passive_scalar_box_driver_with_a_kbc_fluid_equals_pylbm(lib, tmp_path, walls):
    """the C++ facade (lbm::AdeSolver::kbc) in drivers/passive_scalar_box --fluid kbc: its dumps == pylbm.AdeSolver with a
    KbcParams on the driver's own initial state, bit for bit; --buoyancy and --exchange fail with the library's message"""
    R, C, steps, om_g, wr, wc, s2 = 72, 90, 40, 1.6, 2e-3, 3e-3, 1.9
    pre = tmp_path / "psb"
    r = run_driver("passive_scalar_box", R, C, steps, 1.1, om_g, wr, wc, "--dump", pre, "--walls", walls, "--fluid", "kbc",
                   "--s2", s2, timeout=300)
    out = dict(line.split("=", 1) for line in r.stdout.split() if "=" in line)
    assert int(out["steps"]) == steps and int(out["launches"]) == 1 + (steps - 1) * (2 if walls == "2" else 1)

    def load(k, shape):
        return np.fromfile(f"{pre}-{k}.f64").reshape(shape)

    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=BB) if walls == "2" else None
    sv = pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(s2), pylbm.AdeParams(om_g, (wr, wc)), bc=bc)
    sv.set_state(load("f0", (R, C, 9)), load("g0", (R, C, 9)))
    sv.step(steps)
    got = sv.get_state()
    sv.close()
    want = dict(f=load("f", (R, C, 9)), g=load("g", (R, C, 9)), rho=load("rho", (R, C)), u=load("u", (R, C, 2)), C=load("C", (R, C)))
    assert all(np.all(np.isfinite(v)) for v in want.values())
    assert_state_bits(got, want, "driver vs pylbm")
    if walls == "2":
        for extra, msg in ((("--buoyancy", "1e-3,0,0"), "lbm_ade_solver_set_buoyancy: buoyancy"),
                           (("--rectangle", "-20,30,40", "--exchange", "1"), "lbm_ade_solver_wall_exchange: the wall exchange")):
            bad = run_driver("passive_scalar_box", R, C, 2, 1.1, om_g, wr, wc, "--walls", 2, "--fluid", "kbc", "--s2", s2, *extra,
                             timeout=300, check=False)
            assert bad.returncode == 3 and msg in bad.stderr and "KBC fluid" in bad.stderr, bad.stderr
