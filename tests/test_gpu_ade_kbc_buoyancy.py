"""GPU suite, buoyancy of the fluid + scalar step with the entropic KBC collision as the fluid: the forced KBC collision
(lbm_ade_collide_mb, lbm_ade_stream_collide_mb, lbm_ade_solver_set_buoyancy_m; pylbm.AdeSolver.set_buoyancy_m; the
rayleigh_benard driver; ade_kbc.hpp k_ade_kbc_stream_collide_buoyant and the BUOYANT one-node kernels with KbcModel).

The yardstick is `oracle_loop` of tests/ade_kbc_buoyancy_util.py: tests/ade_kbc_util.collide with m1 replaced by
u0 + u_shift F -- the oracle's kbc::collide on the moments the driver HOLDS, F from calc_rho(g), the scalar on the shifted
u -- and tests/ade_util.stream for walls, FIXED edges and the body.  It never calls the library under test, is computed
once per case (cached, read-only) and is asserted finite wherever it is used.  Bitwise means equal bit patterns.  The
start states are ade_util.initial_state with the scalar scaled to C in [0, 1] (ade_util.buoyant_initial_state), beta of
order 1e-2: shifts of ~1e-3 to 1e-2, far above rounding."""
import ctypes as ct
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ade_calls  # noqa: E402
import ade_kbc_buoyancy_util as yb  # noqa: E402
import ade_kbc_util as kbc  # noqa: E402
import diag_reference as ref  # noqa: E402
import pylbm  # noqa: E402
from ade_slab_util import body_table  # noqa: E402
from ade_util import (GBC, Body, alloc, assert_bits, assert_state_bits, assert_write_set, bits,  # noqa: E402
                      buoyant_initial_state, from_lattice, geom, moment_fields, owned, poisoned, to_lattice)
from gpu_util import bits_equal, dev  # noqa: E402
from proc_util import last_json, run_driver  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
BB, SP = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_NEG, COL_NEG = pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_NEG
S2, OMEGA_G, W = kbc.S2, kbc.OMEGA_G, (3e-3, -2e-3)
BETA, C_REF = (1.2e-2, -8e-3), 0.4
BY = pylbm.AdeBuoyancy(BETA, C_REF)  # u_shift = 1
SHAPES = {"2x2": (2, 2), "3x2": (3, 2), "16x16": (16, 16), "3x1040": (3, 1040)}  # 1040: three 512-column tiles per row
EDGES = {"periodic": pylbm.Bc(), "walls": GBC}  # GBC: bounce-back rows, a bounce-back and a specular column
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


def fixed_spec(R, C):
    """every wall edge of GBC FIXED, constants and profiles mixed, corners included; values of the order of C"""
    return {"row_lo": 0.7, "row_hi": ("profile", np.linspace(0.2, 1.2, C)), "col_lo": ("profile", np.linspace(1.5, 0.3, R)),
            "col_hi": 0.0}


def fixed_numpy(spec, R, C):
    return {k: (v[1] if isinstance(v, tuple) else np.full(C if k.startswith("row") else R, float(v))) for k, v in spec.items()}


def device_sbc(spec):
    """pylbm.AdeScalarBC of a spec (the profiles uploaded and kept alive by the descriptor)"""
    return pylbm.AdeScalarBC(**{k: ((0.0, torch.from_numpy(np.ascontiguousarray(v[1])).to(dev())) if isinstance(v, tuple) else v)
                                for k, v in spec.items()})


@functools.lru_cache(maxsize=None)
def _yardstick(R, C, edges, iterations):
    from pyoracle import Oracle
    orc = Oracle()
    f0, g0 = buoyant_initial_state(orc, R, C, seed=R * C, w=W)
    fixed = fixed_numpy(fixed_spec(R, C), R, C) if edges == "walls" else {}
    out, f, g, done = {0: _frozen(dict(f=f0, g=g0))}, f0, g0, 0
    for n in iterations:
        st = yb.oracle_loop(orc, f, g, S2, OMEGA_G, W, n - done, BY, EDGES[edges], fixed)
        assert yb.finite(st), f"the yardstick is not finite after {n} iterations"
        f, g, done = st["f"], st["g"], n
        out[n] = _frozen(st)
    return out


def yardstick(R, C, edges, iterations=ITERATIONS):
    """{0: the start state (f, g), n: the state after n driver iterations (f, g, rho, u, C)}, computed once, read-only"""
    return _yardstick(R, C, edges, tuple(iterations))


def solver(lib, R, C, form=REF, bc=None, by=BY, s2=S2, omega_g=OMEGA_G, w=W, **kw):
    return pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(s2, form), pylbm.AdeParams(omega_g, w, form=form), bc=bc, buoyancy=by, **kw)


def run(lib, R, C, start, steps, **kw):
    sv = solver(lib, R, C, **kw)
    try:
        sv.set_state(start["f"], start["g"])
        sv.step(steps)
        return sv.get_state(), sv.launches()
    finally:
        sv.close()


# ---- 1. bit for bit against the yardstick ----------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", list(EDGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_context_is_the_yardstick(lib, shape, edges):
    """f, g and get_state's rho, u, C after 1, 2 and 20 iterations: a periodic box; walls all round (bounce-back rows, a
    bounce-back and a specular column) with every edge of the scalar FIXED.  Every compared state is finite"""
    R, C = SHAPES[shape]
    yard = yardstick(R, C, edges)
    sbc = device_sbc(fixed_spec(R, C)) if edges == "walls" else None
    sv, done = solver(lib, R, C, bc=EDGES[edges], scalar_bc=sbc), 0
    try:
        sv.set_state(yard[0]["f"], yard[0]["g"])
        for n in ITERATIONS:
            sv.step(n - done)
            done = n
            got = sv.get_state()
            assert yb.finite(got), f"{shape} {edges}: non-finite after {n} iterations"
            assert_state_bits(got, yard[n], f"{shape} {edges}: after {n} iterations")
        assert sv.launches() == 1 + 19 * (2 if edges == "walls" else 1)
    finally:
        sv.close()
    passive = kbc.oracle_loop(_oracle(), yard[0]["f"], yard[0]["g"], S2, OMEGA_G, W, 2, EDGES[edges])
    assert not bits_equal(passive["f"], yard[2]["f"])  # the scalar does push on the fluid


@functools.lru_cache(maxsize=None)
def _oracle():
    from pyoracle import Oracle
    return Oracle()


BODY_R, BODY_C, BODY_BC = 48, 64, pylbm.Bc(row_lo=BB)


def body_numpy(rule):
    seg = [((slice(None), 20), COL_NEG), ((5, slice(20, 31)), ROW_NEG), ((29, slice(20, 31)), ROW_NEG)]
    return Body(seg, seg, *rule)


@pytest.mark.parametrize("case", ["no_flux", "fixed"])
def test_the_interior_wall_body_is_the_yardstick(lib, oracle, case):
    """the body of the KBC suite on 48 x 64 under a bounce-back first row, its g slots NO_FLUX, or FIXED at 0.6 beside a
    FIXED first row: 1, 2 and 20 iterations, bit for bit; three launches per step"""
    R, C = BODY_R, BODY_C
    rule = {"no_flux": (NO_FLUX, 0.0), "fixed": (FIXED, 0.6)}[case]
    spec = {"row_lo": 0.7} if case == "fixed" else {}
    f0, g0 = buoyant_initial_state(oracle, R, C, seed=11, w=W)
    table = body_table(lib, R, C, rule)
    sv = solver(lib, R, C, bc=BODY_BC, scalar_bc=device_sbc(spec) if spec else None, walls=table)
    try:
        sv.set_state(f0, g0)
        want, done = dict(f=f0, g=g0), 0
        for n in ITERATIONS:
            want = yb.oracle_loop(oracle, want["f"], want["g"], S2, OMEGA_G, W, n - done, BY, BODY_BC, fixed_numpy(spec, R, C),
                                  body_numpy(rule))
            assert yb.finite(want)
            sv.step(n - done)
            done = n
            assert_state_bits(sv.get_state(), want, f"body {case} after {n} iterations")
        assert sv.launches() == 1 + 19 * 3  # interior, edge pass, table pass
    finally:
        sv.close()
        table.close()
    plain = yb.oracle_loop(oracle, f0, g0, S2, OMEGA_G, W, 20, BY, BODY_BC, fixed_numpy(spec, R, C), Body([], []))
    assert not bits_equal(want["g"], plain["g"])  # the body is felt


@pytest.mark.parametrize("edges", list(EDGES))
def test_every_launch_variant(lib, edges):
    """3 x 1040: all four `nt` settings x grid_cap 1 and 7 (three tiles per row: the stride of 1 and 7 workgroups walks
    across rows): three iterations, each bit for bit the default launch, which is the yardstick"""
    R, C = SHAPES["3x1040"]
    yard = yardstick(R, C, edges, iterations=(3,))
    kw = dict(bc=EDGES[edges], scalar_bc=device_sbc(fixed_spec(R, C)) if edges == "walls" else None)
    base, _ = run(lib, R, C, yard[0], 3, **kw)
    assert yb.finite(base)
    assert_state_bits(base, yard[3], f"{edges}: default launch against the yardstick")
    for nt in (0, 1, 2, 3):
        for cap in (1, 7):
            lib.set_tuning(b"nt", nt)
            lib.set_tuning(b"grid_cap", cap)
            got, _ = run(lib, R, C, yard[0], 3, **kw)
            assert_state_bits(got, base, f"{edges} nt={nt} grid_cap={cap}")


# ---- 2. the raw calls ------------------------------------------------------------------------------------------------------
def raw_collide(lib, g, bc, prm, src, **kw):
    dst = alloc(g), alloc(g)
    ade_calls.collide(lib, "_mb", g, bc, prm, dst, src, buoy=BY, **kw)
    return dst


def raw_step_into(lib, g, bc, prm, dst, src, **kw):
    ade_calls.step_into(lib, "_mb", g, bc, prm, dst, src, buoy=BY, **kw)


def assert_raw(what, g, lat, m, want):
    torch.cuda.synchronize()
    R, C = g.R, g.C
    assert bits_equal(from_lattice(lat[0], g), want["fc"]), what + ": f"
    assert bits_equal(from_lattice(lat[1], g), want["gc"]), what + ": g"
    assert bits_equal(m[0].view(R, C).cpu().numpy(), want["rho"]), what + ": rho"
    assert bits_equal(m[1].view(2, R, C).cpu().numpy().transpose(1, 2, 0), want["u"]), what + ": u is not the shifted velocity"
    assert bits_equal(m[2].view(R, C).cpu().numpy(), want["C"]), what + ": C"


@pytest.mark.parametrize("edges", list(EDGES))
@pytest.mark.parametrize("R,C,pitch", [(16, 16, 0), (3, 1040, 1056)])
def test_raw_calls_write_the_shifted_velocity(lib, oracle, R, C, pitch, edges):
    """lbm_ade_collide_mb on the pre-collision state == the yardstick's collision half (the collide-only first iteration),
    lbm_ade_stream_collide_mb from it == the collision half of the streamed state; their moments: rho, the SHIFTED u, C.
    The form of the parameters is REASSOCIATED: a buoyant step runs the reference order whatever it says"""
    g, bc, prm = geom(R, C, 0, pitch), EDGES[edges], kbc.params(FAST, w=W)
    spec = fixed_spec(R, C) if edges == "walls" else {}
    sbc = device_sbc(spec) if spec else None
    f0, g0 = buoyant_initial_state(oracle, R, C, seed=21, w=W)
    c0 = yb.collide(oracle, f0, g0, S2, OMEGA_G, W, BY)
    f1, g1 = yb.stream(oracle, bc, fixed_numpy(spec, R, C), c0["fc"], c0["gc"], W)
    c1 = yb.collide(oracle, f1, g1, S2, OMEGA_G, W, BY)
    assert not bits_equal(c0["u"], oracle.calc_u(f0, c0["rho"]))  # the shift is there
    m = moment_fields(g)
    post = raw_collide(lib, g, bc, prm, (to_lattice(f0, g), to_lattice(g0, g)), sbc=sbc, moments=m)
    assert_raw("lbm_ade_collide_mb", g, post, m, c0)
    nxt, m = (alloc(g), alloc(g)), moment_fields(g)
    raw_step_into(lib, g, bc, prm, nxt, post, sbc=sbc, moments=m)
    assert_raw("lbm_ade_stream_collide_mb", g, nxt, m, c1)


@pytest.mark.parametrize("shape,pitch,rows", [("16x16", 0, (5, 11)), ("3x1040", 1056, (1, 2)), ("3x1040", 1056, (0, 3))])
def test_a_row_range_writes_exactly_its_rows(lib, oracle, shape, pitch, rows):
    """sentinel-poisoned targets, walls all round with FIXED edges, the body's column wall as a table, grid_cap = 7: rows
    [row_begin, row_end) of both lattices (no padding, no other row) and of the three moment fields, each double the full
    launch's"""
    R, C = SHAPES[shape]
    g, prm = geom(R, C, 0, pitch), kbc.params(REF, w=W)
    sbc = device_sbc(fixed_spec(R, C))
    table = pylbm.AdeInteriorWalls(lib, R, C).add(0, 6, 1, 0, R, COL_NEG, COL_NEG, FIXED, 0.6).finalize()
    f0, g0 = buoyant_initial_state(oracle, R, C, seed=41, w=W)
    src = to_lattice(f0, g), to_lattice(g0, g)
    want, want_m = (alloc(g), alloc(g)), moment_fields(g)
    raw_step_into(lib, g, GBC, prm, want, src, sbc=sbc, iwalls=table, moments=want_m)
    lib.set_tuning(b"grid_cap", 7)
    dst, m = (poisoned(g), poisoned(g)), moment_fields(g)
    raw_step_into(lib, g, GBC, prm, dst, src, sbc=sbc, iwalls=table, rows=rows, moments=m)
    torch.cuda.synchronize()
    span = list(range(*rows))
    for k, name in enumerate("fg"):
        assert_write_set(dst[k], g, span, f"{shape} rows {rows}: {name}")
        assert_bits(owned(dst[k], g)[:, span], owned(want[k], g)[:, span], f"{shape} rows {rows}: {name}")
    from ade_util import SENTINEL
    for t, w_, planes, name in zip(m, want_m, (1, 2, 1), ("rho", "u", "C")):
        t, w_ = t.view(planes, R, C), w_.view(planes, R, C)
        expect = torch.zeros_like(t, dtype=torch.bool)
        expect[:, span] = True
        assert torch.equal(bits(t) != SENTINEL, expect), f"{shape} rows {rows}: write set of {name}"
        assert_bits(t[:, span], w_[:, span], f"{shape} rows {rows}: {name}")
    table.close()


# ---- 3. the momentum input -------------------------------------------------------------------------------------------------
def test_momentum_input_is_rho_u_shift_f_per_step(lib, oracle):
    """periodic 16 x 16, uniform C = 0.6, c_ref = 0.5, beta = (1e-2, -5e-3), u_shift = 1: a collision adds rho u_shift F
    to each node's momentum and streaming on a periodic box moves it, so AdeSolver.diag's momentum sums grow per step by
    sum rho u_shift F of the state before the step (rho, C of get_state) -- to 1e-12 relative over 50 steps; the mass is
    unchanged to 1e-13; guo_a, guo_b are not read: (3, 9) and (1/3, 1/9) give the same bits"""
    R = C = 16
    beta, c_ref = (1e-2, -5e-3), 0.5
    f0, _ = buoyant_initial_state(oracle, R, C, seed=7, w=W)
    rho0 = oracle.calc_rho(f0)
    g0 = oracle.equilibrium(oracle.calc_u(f0, rho0) + np.asarray(W), np.full((R, C), 0.6))
    states = []
    for guo in ((3.0, 9.0), (1.0 / 3.0, 1.0 / 9.0)):
        sv = solver(lib, R, C, by=pylbm.AdeBuoyancy(beta, c_ref, 1.0, guo))
        try:
            sv.set_state(f0, g0)
            first = sv.diag()
            added = np.zeros(2)
            for _ in range(50):
                s = sv.get_state()
                added += [float(np.sum(s["rho"] * (beta[k] * (s["C"] - c_ref)))) for k in range(2)]
                sv.step(1)
            last = sv.diag()
            states.append(sv.get_state())
        finally:
            sv.close()
        got = np.array([last[ref.SUM_MR] - first[ref.SUM_MR], last[ref.SUM_MC] - first[ref.SUM_MC]])
        print(f"guo={guo}: momentum grown by {got!r}, sum of rho u_shift F {added!r}, relative {np.abs(got / added - 1)!r}; "
              f"mass {first[ref.SUM_RHO]!r} -> {last[ref.SUM_RHO]!r}")
        assert last[ref.NONFINITE] == 0.0
        assert np.all(np.abs(got - added) <= 1e-12 * np.abs(added)), (got, added)
        assert abs(last[ref.SUM_RHO] - first[ref.SUM_RHO]) <= 1e-13 * first[ref.SUM_RHO]
    assert_state_bits(states[1], states[0], "guo (1/3, 1/9) against (3, 9)")


# ---- 4. zero beta, NULL and the form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
@pytest.mark.parametrize("edges", list(EDGES))
def test_zero_beta_and_null_are_the_passive_context(lib, form, edges):
    R, C = 16, 16
    start = yardstick(R, C, edges)[0]
    sbc = device_sbc(fixed_spec(R, C)) if edges == "walls" else None
    runs = {}
    for key, by in (("plain", "unset"), ("null", None), ("zero", pylbm.AdeBuoyancy((0.0, 0.0), 0.3, 0.5, (3.0, 9.0))), ("buoyant", BY)):
        sv = solver(lib, R, C, form, bc=EDGES[edges], by=None, scalar_bc=sbc)
        try:
            if by != "unset":
                sv.set_buoyancy_m(by)
            sv.set_state(start["f"], start["g"])
            sv.step(11)
            runs[key] = (sv.get_state(), sv.launches())
        finally:
            sv.close()
    for key in ("null", "zero"):
        assert_state_bits(runs[key][0], runs["plain"][0], key)
        assert runs[key][1] == runs["plain"][1]
    assert runs["buoyant"][1] == runs["plain"][1] == 1 + 10 * (2 if edges == "walls" else 1)  # buoyancy adds no launch
    assert not bits_equal(runs["buoyant"][0]["f"], runs["plain"][0]["f"])


@pytest.mark.parametrize("edges", list(EDGES))
def test_a_buoyant_step_runs_the_reference_order_whatever_the_form(lib, edges):
    R, C = 16, 16
    yard = yardstick(R, C, edges)
    sbc = device_sbc(fixed_spec(R, C)) if edges == "walls" else None
    for form in (FAST, pylbm.FORM_DEFAULT):
        got, _ = run(lib, R, C, yard[0], 20, form=form, bc=EDGES[edges], scalar_bc=sbc)
        assert_state_bits(got, yard[20], f"{edges} form={form}")


# ---- 5. set_buoyancy_m -----------------------------------------------------------------------------------------------------
def test_set_buoyancy_m_on_a_bgk_context_is_set_buoyancy(lib):
    R, C = 16, 16
    start = yardstick(R, C, "walls")[0]
    by = pylbm.AdeBuoyancy(BETA, C_REF, 0.5, (3.0, 9.0))
    states = []
    for setter in ("set_buoyancy", "set_buoyancy_m"):
        sv = pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(1.2, 0), pylbm.AdeParams(OMEGA_G, W), bc=GBC,
                             scalar_bc=device_sbc(fixed_spec(R, C)))
        try:
            getattr(sv, setter)(by)
            sv.set_state(start["f"], start["g"])
            sv.step(20)
            states.append((sv.get_state(), sv.launches()))
        finally:
            sv.close()
    assert_state_bits(states[1][0], states[0][0], "set_buoyancy_m against set_buoyancy on a BGK context")
    assert states[0][1] == states[1][1]


def test_what_stays_refused_on_a_buoyant_kbc_context(lib):
    """lbm_ade_solver_set_buoyancy keeps its refusal and message; a non-empty open table and the wall exchange stay refused"""
    R, C = 16, 16
    start = yardstick(R, C, "periodic")[0]
    sv = solver(lib, R, C, pylbm.FORM_DEFAULT, bc=pylbm.Bc(row_hi=BB))
    channel = pylbm.AdeOpenBoundary(lib, R, C).channel(0.02, 1e-3, 4).finalize()
    try:
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_set_buoyancy: buoyancy .* KBC fluid"):
            sv.set_buoyancy(pylbm.AdeBuoyancy((1e-3, 0.0), 0.0))
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_set_open: open boundaries .* KBC fluid"):
            sv.set_open(channel)
        sv.set_state(start["f"], start["g"])
        sv.step(2)
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_wall_exchange: the wall exchange .* KBC fluid"):
            sv.wall_exchange()
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_set_buoyancy_m: buoyancy c_ref=nan must be finite"):
            sv.set_buoyancy_m(pylbm.AdeBuoyancy((1e-3, 0.0), float("nan")))
        assert sv.launches() == 1 + 2  # the refusals enqueued nothing
        assert sv.diag()[ref.NONFINITE] == 0.0
    finally:
        sv.close()
        channel.close()


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------
def test_graph_replay_keeps_the_buoyancy_of_its_capture(lib, oracle):
    """launch counts: 1 per step on a periodic box, +1 with wall edges, +1 with a non-empty table; 10 steps captured and
    replayed 3 times == 30 plain steps, bit for bit, with set_buoyancy_m between the replays changing nothing the graph
    does (the descriptor travels by value in the kernel arguments)"""
    R, C = BODY_R, BODY_C
    f0, g0 = buoyant_initial_state(oracle, R, C, seed=17, w=W)
    start = dict(f=f0, g=g0)
    table = body_table(lib, R, C, (FIXED, 0.6))
    try:
        for kw, per_step in ((dict(), 1), (dict(bc=BODY_BC), 2), (dict(bc=BODY_BC, walls=table), 3)):
            want, launches = run(lib, R, C, start, 31, **kw)
            assert launches == 1 + 30 * per_step
        assert yb.finite(want)
        st, graph = ct.c_void_p(), ct.c_void_p()
        lib.stream_create(ct.byref(st))
        try:
            sv = solver(lib, R, C, bc=BODY_BC, walls=table, stream=st.value)
            sv.set_state(f0, g0)
            sv.step(1)  # the collide-only first iteration, direct
            sv.sync()
            lib.graph_begin_capture(st)
            sv.step(10)
            lib.graph_end_capture(st, ct.byref(graph))
            lib.graph_launch(graph, 1, st)
            lib.stream_sync(st)
            sv.set_buoyancy_m(pylbm.AdeBuoyancy((0.5, 0.5), 0.0))  # not what the graph holds
            lib.graph_launch(graph, 1, st)
            sv.set_buoyancy_m(None)
            lib.graph_launch(graph, 1, st)
            lib.stream_sync(st)
            assert_state_bits(sv.get_state(), want, "three replays of ten steps")  # get_state does not read the buoyancy
            sv.close()
        finally:
            if graph:
                lib.graph_destroy(graph)
            lib.stream_destroy(st)
    finally:
        table.close()


# ---- 7. vertical slot, conduction regime -----------------------------------------------------------------------------------
def test_vertical_slot_conduction_regime_converges_to_the_cubic_profile(lib, oracle):
    """the setup of tests/test_gpu_ade_buoyancy.py with a KBC fluid: periodic rows, bounce-back columns with the scalar
    FIXED at 0 / 1, c_ref = 0.5, beta = (1e-4, 0), w = 0, s2 = 1.0, omega_g = 1.2, u_shift = 1, R = 8; linear C, physical
    velocity u0 + F / 2 against u_r(x) = -(beta / nu)(x^3 / 6L - x^2 / 4 + x L / 12) after 6 C^2 / nu steps.
    The CPU yardstick of exactly this scheme (ade_kbc_buoyancy_util.oracle_loop) gives relative L2 errors 8.153e-3 at
    C = 16 and 2.042e-3 at C = 32, order 1.998, C linear to 7e-15 and 4e-14, nothing non-finite (the BGK fluid with Guo's
    coefficients: 8.15e-3 and 2.04e-3); the device gives the same figures.  Asserted, the bounds of that file: the error at 32 <= 2.5e-3, the observed order >= 1.9, C linear
    to 1e-12, u identical across the rows; and a non-finite count of 0"""
    errs = {}
    for C in (16, 32):
        f0, g0, n = yb.slot_initial(oracle, 8, C)
        sv = solver(lib, 8, C, bc=pylbm.Bc(col_lo=BB, col_hi=BB), by=pylbm.AdeBuoyancy((yb.SLOT_BETA, 0.0), 0.5, 1.0),
                    s2=yb.SLOT_S2, omega_g=yb.SLOT_OMEGA_G, w=(0.0, 0.0), scalar_bc=pylbm.AdeScalarBC(col_lo=0.0, col_hi=1.0))
        try:
            sv.set_state(f0, g0)
            sv.step(n)
            assert sv.diag()[ref.NONFINITE] == 0.0
            errs[C] = yb.slot_errors(sv.get_state(), C)
        finally:
            sv.close()
    order = float(np.log2(errs[16][0] / errs[32][0]))
    print(f"vertical slot, KBC: rel L2 error {errs[16][0]:.3e} at C=16, {errs[32][0]:.3e} at C=32, order {order:.3f}; "
          f"C off linear by {errs[16][1]:.1e}, {errs[32][1]:.1e}")
    assert errs[16][2] and errs[32][2], "u or C differs across the rows"
    assert errs[32][0] <= 2.5e-3, errs
    assert order >= 1.9, (errs, order)
    assert max(errs[16][1], errs[32][1]) <= 1e-12, errs


# ---- 8. Rayleigh-Benard onset ----------------------------------------------------------------------------------------------
def test_rayleigh_benard_onset(lib, oracle):
    """the setup of tests/test_gpu_ade_buoyancy.py with a KBC fluid: R = 24, C = 48, bounce-back rows, periodic columns, the
    scalar FIXED at 1 below and 0 above, c_ref = 0.5, beta = (Ra nu^2 / R^3, 0), s2 = omega_g = 1.4, u_shift = 1; conduction
    profile plus 1e-3 sin cos; sigma T = 1/2 ln(E(2T) / E(T)), E = sum u_c^2, T = 8063.
    The CPU yardstick (ade_kbc_buoyancy_util.oracle_loop) gives sigma T = -1.546 at Ra = 1500 and +1.932 at 1950, zero crossing
    at Ra_c = 1700.0 (-0.45 % off 1707.76; the BGK fluid with Guo's coefficients: 1727, +1.1 %): inside 3 %, so the bound
    against theory holds and no comparison against the yardstick's own Ra_c is needed; the device gives the same figures.  Asserted: decay at 1500, growth at 1950, the interpolated Ra_c
    within 3 % of 1707.76 -- the bound the BGK test states"""
    assert yb.RB_T == 8063
    f0, g0 = yb.rb_initial(oracle)
    sigma = {}
    for Ra in (1500.0, 1950.0):
        sv = solver(lib, yb.RB_R, yb.RB_C, bc=pylbm.Bc(row_lo=BB, row_hi=BB), by=pylbm.AdeBuoyancy((yb.rb_beta(Ra), 0.0), 0.5, 1.0),
                    s2=yb.RB_S2, omega_g=yb.RB_S2, w=(0.0, 0.0), scalar_bc=pylbm.AdeScalarBC(row_lo=1.0, row_hi=0.0))
        try:
            sv.set_state(f0, g0)
            e = []
            for _ in range(2):
                sv.step(yb.RB_T)
                e.append(float(np.sum(sv.get_state()["u"][..., 1] ** 2)))
            assert sv.diag()[ref.NONFINITE] == 0.0
        finally:
            sv.close()
        sigma[Ra] = yb.rb_sigma(*e)
    ra_c = yb.rb_ra_c(sigma[1500.0], sigma[1950.0])
    print(f"Rayleigh-Benard, KBC: sigma T = {sigma[1500.0]:.3f} at Ra = 1500, {sigma[1950.0]:.3f} at Ra = 1950, Ra_c = {ra_c:.1f}")
    assert sigma[1500.0] < 0.0, sigma
    assert sigma[1950.0] > 0.0, sigma
    assert abs(ra_c - yb.RA_THEORY) <= 0.03 * yb.RA_THEORY, ra_c


# ---- 9. the driver ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fluid", ["kbc", "bgk"])
def test_rayleigh_benard_driver_equals_pylbm(lib, tmp_path, fluid):
    """drivers/rayleigh_benard --dump on 24 x 48 for 40 steps == pylbm.AdeSolver on the driver's own initial state, bit for
    bit: --fluid kbc through set_buoyancy_m (the forced KBC collision), --fluid bgk through set_buoyancy; the JSON line's
    non-finite count is 0"""
    R, C, steps, rate, om_g, Ra = 24, 48, 40, 1.4, 1.3, 5000.0
    pre = tmp_path / "rb"
    r = run_driver("rayleigh_benard", "--fluid", fluid, "--rows", R, "--cols", C, "--steps", steps,
                   "--s2" if fluid == "kbc" else "--omega", rate, "--omega-g", om_g, "--ra", Ra, "--dump", pre, timeout=300)
    line = last_json(r)
    assert line["steps"] == steps and line["nonfinite"] == 0 and line["fluid"] == fluid
    assert line["launches"] == 1 + (steps - 1) * 2

    def load(k, shape):
        return np.fromfile(f"{pre}-{k}.f64").reshape(shape)

    assert (line["u_shift"], line["guo"]) == ((1.0, [1.0 / 3.0, 1.0 / 9.0]) if fluid == "kbc" else (0.5, [3.0, 9.0]))
    by = pylbm.AdeBuoyancy((line["beta"], 0.0), 0.5, line["u_shift"], tuple(line["guo"]))
    sv = pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(rate) if fluid == "kbc" else pylbm.BgkParams(rate, 0),
                         pylbm.AdeParams(om_g, (0.0, 0.0)), bc=pylbm.Bc(row_lo=BB, row_hi=BB),
                         scalar_bc=pylbm.AdeScalarBC(row_lo=1.0, row_hi=0.0))
    try:
        (sv.set_buoyancy_m if fluid == "kbc" else sv.set_buoyancy)(by)
        sv.set_state(load("f0", (R, C, 9)), load("g0", (R, C, 9)))
        sv.step(steps)
        got = sv.get_state()
        d = sv.diag()
    finally:
        sv.close()
    want = dict(f=load("f", (R, C, 9)), g=load("g", (R, C, 9)), rho=load("rho", (R, C)), u=load("u", (R, C, 2)), C=load("C", (R, C)))
    assert yb.finite(want)
    assert_state_bits(got, want, f"driver --fluid {fluid} vs pylbm")
    assert line["max_u"] == float(np.sqrt(d[ref.MAX_U2]))
    assert not bits_equal(want["u"], np.zeros((R, C, 2)))  # the perturbation has set the fluid in motion
