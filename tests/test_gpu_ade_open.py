"""GPU suite, open boundaries of the fluid + scalar solver (lbm_ade_open: lbm_ade_stream_collide_o, lbm_ade_collide_o,
lbm_ade_solver_set_open; pylbm.AdeOpenBoundary).

Two yardsticks, neither of which calls the library under test: the CPU oracle's whole sediment loop (Oracle.sed_steps,
test/rectangle_sedimentation_test.cpp:106-237) and, for every rule alone and combined, tests/ade_open_util.py -- the
driver's sequential index assignments in numpy on the oracle's solver:: primitives.  Bitwise means equal bit patterns;
the reassociated form is held to 1e-10 relative."""
import ctypes as ct
import json
import os

import numpy as np
import pytest
from conftest import relerr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
import ade_calls  # noqa: E402
import ade_open_util as aou  # noqa: E402
import ade_util as ade  # noqa: E402
from ade_open_util import ABB, ABB_X, ALL, BB_RULE, SPEC_COL, SPEC_ROW, Segments, mask  # noqa: E402
from ade_util import SENTINEL, Body  # noqa: E402
from gpu_util import bits_equal, dev  # noqa: E402
from proc_util import PKG, run_driver  # noqa: E402
from pylbm import _ptr  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
BB, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_PERIODIC
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_NEG, COL_POS, COL_NEG = pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_POS, pylbm.ADE_FACE_COL_NEG
W = (3e-3, 3e-3)
OMEGA, OMEGA_G = 1.2, 1.7
BETA, C_REF = (2e-3, -1.5e-3), 0.4
LBM_ERR_INVALID = -1
SHAPES = [(2, 2, 0), (3, 4, 0), (6, 8, 0), (48, 1040, 1048)]  # R, C, row pitch (0: dense)
SHAPE_IDS = ["2x2", "3x4", "6x8", "48x1040_pitch1048"]
BOTTOM = pylbm.Bc(row_hi=BB)


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


# ---- the rectangle of the driver, as table and as index assignments (tests/test_gpu_ade_iwalls.py) ------------------------
def rectangle_body(R, r_top, c1, c2):
    top = r_top + R
    f_side, g_first = slice(top + 1, R - 1), slice(top + 1, R)
    f_seg = [((f_side, c1), COL_NEG), ((top, slice(c1, c2 + 1)), ROW_NEG), ((f_side, c2), COL_POS)]
    g_seg = [((g_first, c1), COL_NEG), ((top, slice(c1, c2 + 1)), ROW_NEG), ((f_side, c2), COL_POS)]
    return Body(f_seg, g_seg, FIXED, 0.0)


def rectangle_table(lib, R, C, r_top, c1, c2):
    """absorbing at C_w = -0.0: -g*[q] + 2 G_q (-0.0) is the driver's `-g_coll` bit for bit, the sign of an exact zero
    included (at +0.0 a population that is exactly +0 comes back as +0, the driver's as -0)"""
    ABSORB = -0.0
    t = pylbm.AdeInteriorWalls(lib, R, C)
    n_side = (R - 1) - (r_top + R + 1)
    if n_side > 0:
        t.add(r_top + 1, c1, 1, 0, n_side, COL_NEG, COL_NEG, FIXED, ABSORB)
        t.add(r_top + 1, c2, 1, 0, n_side, COL_POS, COL_POS, FIXED, ABSORB)
    t.add(-1, c1, 1, 0, 1, 0, COL_NEG & ~(1 << 6), FIXED, ABSORB)  # g's foot; slot 7 is the bottom wall's
    t.add(r_top, c1, 0, 1, c2 - c1 + 1, ROW_NEG, ROW_NEG, FIXED, ABSORB)
    return t.finalize()


# ---- running the library ------------------------------------------------------------------------------------------------
def solver(lib, R, C, form=REF, bc=None, sbc=None, by=None, walls=None, table=None, stream=None, omega_g=OMEGA_G, w=W):
    return pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(OMEGA, 0, form=form), pylbm.AdeParams(omega_g, w, form=form), bc=bc,
                           stream=stream, scalar_bc=sbc, buoyancy=by, walls=walls, open=table)


def run(lib, f0, g0, steps, **kw):
    sv = solver(lib, f0.shape[0], f0.shape[1], **kw)
    sv.set_state(f0, g0)
    sv.step(steps)
    out, launches = sv.get_state(), sv.launches()
    sv.close()
    return out, launches


def carry_buffer(table, extra=0):
    t = torch.zeros(table.carry_len() + extra, dtype=torch.float64, device=dev())
    ade.bits(t).fill_(SENTINEL)
    return t


def raw_collide(lib, g, bc, prm, dst, src, table, carry_out, **kw):
    ade_calls.collide(lib, "_o", g, bc, prm, dst, src, open=table, carry_out=carry_out, **kw)


def raw_step(lib, g, bc, prm, dst, src, table, carry_in, carry_out, **kw):
    ade_calls.step_into(lib, "_o", g, bc, prm, dst, src, open=table, carry_in=carry_in, carry_out=carry_out, **kw)


def raw_run(lib, g, bc, prm, f0, g0, n, table, sbc=None, by=None, walls=None):
    """the collide-only iteration and n streamed steps through the raw entry points, every target poisoned first:
    the post-collision pair, the carry and the moments of the last step"""
    src = (ade.to_lattice(f0, g), ade.to_lattice(g0, g))
    cin, moments = carry_buffer(table), None
    dst = (ade.poisoned(g), ade.poisoned(g))
    raw_collide(lib, g, bc, prm, dst, src, table, cin, sbc=sbc, buoy=by)
    for _ in range(n):
        src, dst, cout, moments = dst, (ade.poisoned(g), ade.poisoned(g)), carry_buffer(table), ade.moment_fields(g)
        raw_step(lib, g, bc, prm, dst, src, table, cin, cout, sbc=sbc, buoy=by, iwalls=walls, moments=moments)
        cin = cout
    torch.cuda.synchronize()
    return dst, cin, moments


def check_raw(lib, orc, shape, segs, n=3, bc=None, sbc_spec=None, by=None, body=None, walls=None, seed=3, form=REF):
    """n streamed steps through the raw entry points against the yardstick: lattices, carry and moments bit for bit in the
    reference order, within 1e-10 in the reassociated form; returns the yardstick's state"""
    R, C, pitch = shape
    g = ade.geom(R, C, 0, pitch)
    bc = bc if bc is not None else pylbm.Bc()
    sbc, fixed = ade.build_sbc(sbc_spec, R, C) if sbc_spec else (None, {})
    f0, g0 = ade.buoyant_initial_state(orc, R, C, seed) if by else ade.initial_state(orc, R, C, seed=seed)
    table = segs.table(lib)
    (fn, gn), carry, moments = raw_run(lib, g, bc, ade.params(form), f0, g0, n, table, sbc, by, walls)
    want = aou.loop(orc, segs, f0, g0, OMEGA, OMEGA_G, W, n, bc, fixed, body, by)
    c = ade.collide(orc, want["f"], want["g"], OMEGA, OMEGA_G, W, by)
    got = dict(fc=ade.from_lattice(fn, g), gc=ade.from_lattice(gn, g), carry=carry.cpu().numpy(),
               rho=moments[0].cpu().numpy().reshape(R, C), u=moments[1].cpu().numpy().reshape(2, R, C).transpose(1, 2, 0),
               C=moments[2].cpu().numpy().reshape(R, C))
    ref = dict(fc=c["fc"], gc=c["gc"], carry=aou.carry_of(table, want["u"]), rho=c["rho"], u=c["u"], C=c["C"])
    for k in ref:
        if form == REF:
            assert bits_equal(got[k], ref[k]), f"{shape} {k}: max |d| = {np.max(np.abs(got[k] - ref[k]))}"
        else:
            assert relerr(got[k], ref[k]) <= 1e-10, (shape, k, relerr(got[k], ref[k]))
    ade.assert_write_set(fn, g, slice(0, R), "f")
    ade.assert_write_set(gn, g, slice(0, R), "g")
    table.close()
    return want


# ---- 1. the whole driver loop against the CPU oracle ------------------------------------------------------------------------
SED = dict(X=160, Y=256, omega=1.2, u_in=0.03)


@pytest.fixture(scope="module")
def sed(oracle):
    """the oracle's loop after 1 iteration (the hand-over state) and 1, 2, 5, 40 iterations later -- computed once"""
    X, Y, om, u_in = SED["X"], SED["Y"], SED["omega"], SED["u_in"]
    start = oracle.sed_steps(X, Y, om, u_in, 1)
    states, cur, done = {}, start, 0
    for n in (1, 2, 5, 40):
        cur = oracle.sed_steps(X, Y, om, u_in, n - done, state=cur)
        states[n], done = cur, n
    return start, states


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_the_sedimentation_loop_is_the_oracles_bit_for_bit(lib, sed, form):
    X, Y, om, u_in = SED["X"], SED["Y"], SED["omega"], SED["u_in"]
    start, states = sed
    assert states[40]["C"].max() > 5e-4 and all(np.isfinite(states[40][k]).all() for k in states[40])  # not a dead field
    table = pylbm.AdeOpenBoundary(lib, X, Y).channel(u_in).finalize()
    walls = rectangle_table(lib, X, Y, -151, 200, 250)  # the oracle's hard-coded R23, C28, C38
    sv = solver(lib, X, Y, form, BOTTOM, walls=walls, table=table, omega_g=om)
    sv.set_state(start["f"], start["g"])
    done = 0
    for n in (1, 2, 5, 40):
        sv.step(n - done)
        done = n
        got = sv.get_state()
        if form == REF:
            ade.assert_state_bits(got, states[n], f"sedimentation loop, {n} iterations after the hand-over")
        else:
            errs = {k: relerr(got[k], states[n][k]) for k in ("f", "g", "rho", "u", "C")}
            print(f"reassociated vs oracle after {n} iterations:", errs)
            assert max(errs.values()) <= 1e-10, (n, errs)
    # collide-only + its carry launch, then interior + edge pass + open pass + interior-wall pass
    assert sv.launches() == 2 + 4 * 39
    sv.close()
    table.close()
    walls.close()


def test_the_yardstick_is_the_oracles_loop_as_well(oracle, sed):
    """the numpy restatement against Oracle.sed_steps: what the other tests are held to is the driver's loop"""
    X, Y, om, u_in = SED["X"], SED["Y"], SED["omega"], SED["u_in"]
    start, states = sed
    want = aou.loop(oracle, aou.channel(X, Y, u_in), start["f"], start["g"], om, om, W, 2, BOTTOM, {},
                    rectangle_body(X, -151, 200, 250))
    ade.assert_state_bits(want, states[2], "numpy yardstick vs oracle")


# ---- 2. each rule alone and combined, against the numpy yardstick -----------------------------------------------------------
def columns(R, C, g_rules=True):
    """an ABB inlet on column 0 and an extrapolated outlet on column C-1, all rows, all eight slots"""
    s = Segments(R, C)
    s.f(0, 0, 1, 0, R, ALL, ABB, (2e-3, 0.03))
    s.f(0, C - 1, 1, 0, R, ALL, ABB_X, (1.5, -0.5), (0, -1))
    if g_rules:
        s.g(0, 0, 1, 0, R, ALL, FIXED, 1e-3)
    return s


def copies(R, C, s=None):
    s = s or Segments(R, C)
    s.copy(0, 0, 0, 1, C, (1, 0))
    s.copy(0, C - 1, 1, 0, R, (0, -1))  # all rows: its corner reads the first copy's result
    return s


def corners(R, C):
    """columns, then rows: every corner node is named by two segments, for f and for g"""
    s = columns(R, C)
    s.f(0, 0, 0, 1, C, mask(1, 5, 8), SPEC_ROW)
    s.f(R - 1, 0, 0, 1, C, mask(3, 6, 7), BB_RULE)
    s.g(0, 0, 0, 1, C, mask(1, 5, 8), NO_FLUX)
    s.g(R - 1, 0, 0, 1, C, mask(3, 6, 7), FIXED, 5e-4)
    return s


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_inlet_and_outlet_without_copies(lib, oracle, shape):
    R, C, _ = shape
    want = check_raw(lib, oracle, shape, columns(R, C))
    plain = ade.oracle_loop(oracle, *ade.initial_state(oracle, R, C, seed=3), OMEGA, OMEGA_G, W, 3)
    assert not bits_equal(plain["f"], want["f"]) and not bits_equal(plain["g"], want["g"])  # the rules are felt


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_copies_only_on_a_periodic_box(lib, oracle, shape):
    R, C, _ = shape
    want = check_raw(lib, oracle, shape, copies(R, C))
    plain = ade.oracle_loop(oracle, *ade.initial_state(oracle, R, C, seed=3), OMEGA, OMEGA_G, W, 3)
    assert bits_equal(plain["f"], want["f"]) and not bits_equal(plain["g"], want["g"])  # f has no copy


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_both_specular_rows_and_a_specular_column(lib, oracle, shape):
    R, C, _ = shape
    s = Segments(R, C).f(0, 0, 0, 1, C, mask(1, 5, 8), SPEC_ROW).f(R - 1, 0, 0, 1, C, mask(3, 6, 7), SPEC_ROW)
    s.f(0, 0, 1, 0, R, mask(2, 5, 6), SPEC_COL)
    check_raw(lib, oracle, shape, s)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_segment_added_later_wins_at_all_four_corners(lib, oracle, shape):
    R, C, _ = shape
    s = corners(R, C)
    a = check_raw(lib, oracle, shape, s)
    b = check_raw(lib, oracle, shape, s.reversed_rules())
    assert not bits_equal(a["f"], b["f"]) and not bits_equal(a["g"], b["g"])  # the order is felt


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_with_a_fixed_domain_row_and_copies(lib, oracle, shape, form):
    R, C, _ = shape
    bc = pylbm.Bc(row_lo=BB, row_hi=BB)
    check_raw(lib, oracle, shape, copies(R, C, columns(R, C)), bc=bc, sbc_spec={"row_lo": 7e-4}, form=form)


@pytest.mark.parametrize("variant", [ade.REFERENCE, ade.GUO], ids=["reference", "guo"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_buoyant_with_both_coefficient_sets(lib, oracle, shape, variant):
    R, C, _ = shape
    check_raw(lib, oracle, shape, copies(R, C, corners(R, C)), by=ade.buoyancy(BETA, C_REF, variant), seed=5)


@pytest.mark.parametrize("shape", SHAPES[2:], ids=SHAPE_IDS[2:])
def test_with_a_body_whose_foot_is_the_allowed_overlap(lib, oracle, shape):
    """the channel with the rectangle standing on the bottom wall: its foot (R-1, c1) reads the redirected row 0 in slots
    3, 6, 7 -- the bounce-back row's -- and carries no open rule"""
    R, C, _ = shape
    r_top, c1, c2 = -4, C // 2 - 1, C // 2 + 1
    walls = rectangle_table(lib, R, C, r_top, c1, c2)
    check_raw(lib, oracle, shape, aou.channel(R, C, 0.03, 1e-3, 3), bc=BOTTOM, body=rectangle_body(R, r_top, c1, c2), walls=walls)
    walls.close()


# ---- 3. NULL and the empty table; launches ----------------------------------------------------------------------------------
def test_null_and_the_empty_table_are_the_walled_step_and_a_table_costs_one_launch_a_step(lib, oracle):
    R, C = 24, 32
    g, prm = ade.geom(R, C, 0, 40), ade.params(pylbm.FORM_DEFAULT)
    f0, g0 = ade.initial_state(oracle, R, C, seed=4)
    fo, go = ade.to_lattice(f0, g), ade.to_lattice(g0, g)
    walls = rectangle_table(lib, R, C, -7, 10, 16)
    empty = pylbm.AdeOpenBoundary(lib, R, C).finalize()
    want = ade_calls.full_step(lib, "_w", g, BOTTOM, prm, fo, go, iwalls=walls)
    for table in (None, empty):
        dst = (ade.alloc(g), ade.alloc(g))
        raw_step(lib, g, BOTTOM, prm, dst, (fo, go), table, None, None, iwalls=walls)  # no carry asked for
        ade.assert_bits(dst[0], want[0], "f")
        ade.assert_bits(dst[1], want[1], "g")
    launches = {}
    table = aou.channel(R, C, 0.03, 1e-3, 5).table(lib)
    for name, t in (("none", None), ("empty", empty), ("table", table)):
        for steps in (1, 8):
            launches[name, steps] = run(lib, f0, g0, steps, form=pylbm.FORM_DEFAULT, bc=BOTTOM, table=t)[1]
    assert launches["none", 1] == launches["empty", 1] == 1 and launches["none", 8] == launches["empty", 8] == 1 + 2 * 7
    assert launches["table", 8] - launches["table", 1] == 3 * 7  # interior + edge pass + the open pass
    for t in (walls, empty, table):
        t.close()


# ---- 4. the write set -------------------------------------------------------------------------------------------------------
def test_the_step_writes_its_nodes_and_its_carry_and_nothing_else(lib, oracle):
    R, C = 12, 16
    g, prm = ade.geom(R, C, 0, 24), ade.params(REF)
    f0, g0 = ade.initial_state(oracle, R, C, seed=6)
    table = aou.channel(R, C, 0.03, 1e-3, 4).table(lib)
    n = table.carry_len()
    assert n == 2 * table.count() > 0
    src = (ade.to_lattice(f0, g), ade.to_lattice(g0, g))
    cin = torch.from_numpy(np.random.default_rng(1).normal(0.0, 0.01, n)).to(dev())
    keep = [t.clone() for t in (*src, cin)]
    dst, cout, moments = (ade.poisoned(g), ade.poisoned(g)), carry_buffer(table, extra=32), ade.moment_fields(g)
    raw_step(lib, g, BOTTOM, prm, dst, src, table, cin, cout, moments=moments)
    torch.cuda.synchronize()
    for t, what in zip(dst, "fg"):
        ade.assert_write_set(t, g, slice(0, R), what)
    written = ade.bits(cout) != SENTINEL
    assert bool(written[:n].all()) and not bool(written[n:].any())
    for m in moments:
        assert bool((ade.bits(m) != SENTINEL).all())
    for t, k in zip((*src, cin), keep):
        ade.assert_bits(t, k, "an input of the step")
    # the collide-only call writes the same carry entries and no others
    cout2 = carry_buffer(table, extra=32)
    raw_collide(lib, g, BOTTOM, prm, (ade.poisoned(g), ade.poisoned(g)), src, table, cout2)
    torch.cuda.synchronize()
    written = ade.bits(cout2) != SENTINEL
    assert bool(written[:n].all()) and not bool(written[n:].any())
    want = aou.carry_of(table, aou.calc_u(oracle, f0))
    assert bits_equal(cout2[:n].cpu().numpy(), want)
    table.close()


# ---- 5. the host's refusals that need a finalized, non-empty table ------------------------------------------------------------
def _refused(lib, call, name, msg):
    with pytest.raises(pylbm.LbmError, match=msg) as e:
        call()
    assert f"lbm_{name} -> {LBM_ERR_INVALID}: lbm_{name}:" in str(e.value)


def test_carry_row_range_and_overlap_refusals_name_what_is_wrong(lib, oracle):
    R, C = 12, 16
    g, prm = ade.geom(R, C, 0), ade.params(REF)
    f0, g0 = ade.initial_state(oracle, R, C, seed=6)
    src, dst = (ade.to_lattice(f0, g), ade.to_lattice(g0, g)), (ade.poisoned(g), ade.poisoned(g))
    table = aou.channel(R, C, 0.03, 1e-3, 4).table(lib)
    a, b = carry_buffer(table), carry_buffer(table)
    step = "ade_stream_collide_o"
    _refused(lib, lambda: raw_step(lib, g, BOTTOM, prm, dst, src, table, None, b), step, "NULL carry with a table of 75 nodes")
    _refused(lib, lambda: raw_step(lib, g, BOTTOM, prm, dst, src, table, a, None), step, "NULL carry")
    _refused(lib, lambda: raw_step(lib, g, BOTTOM, prm, dst, src, table, a, a), step, "carry_in and carry_out alias")
    _refused(lib, lambda: raw_collide(lib, g, BOTTOM, prm, dst, src, table, None), "ade_collide_o", "NULL carry")
    _refused(lib, lambda: raw_step(lib, g, BOTTOM, prm, dst, src, table, a, b, rows=(0, R - 1)), step,
             r"row range \[0, 11\): the whole block \[0, 12\) only")
    _refused(lib, lambda: raw_step(lib, ade.geom(R, C + 2, 0), BOTTOM, prm, dst, src, table, a, b), step,
             "the table is for a 12 x 16 lattice, the call for 12 x 18")
    # a node of both tables with an open rule
    walls = pylbm.AdeInteriorWalls(lib, R, C).add(5, C - 1, 1, 0, 2, COL_NEG, 0).finalize()
    _refused(lib, lambda: raw_step(lib, g, BOTTOM, prm, dst, src, table, a, b, iwalls=walls), step,
             r"node \(5, 15\) carries an open-boundary rule and is in the interior-wall table")
    walls.close()
    # a node of both tables without a rule, reading a redirected node where no wall replaces the slot
    walls = pylbm.AdeInteriorWalls(lib, R, C).add(1, 5, 0, 1, 1, ROW_NEG, 0).finalize()
    _refused(lib, lambda: raw_step(lib, g, BOTTOM, prm, dst, src, table, a, b, iwalls=walls), step,
             r"node \(1, 5\) is in the interior-wall table and its g slot \d is redirected")
    walls.close()
    # the foot on the bottom wall is allowed -- but only while that row is a wall
    walls = pylbm.AdeInteriorWalls(lib, R, C).add(-1, 5, 0, 1, 1, 0, mask(4, 8), FIXED, 0.0).finalize()
    raw_step(lib, g, BOTTOM, prm, dst, src, table, a, b, iwalls=walls)
    _refused(lib, lambda: raw_step(lib, g, pylbm.Bc(), prm, dst, src, table, a, b, iwalls=walls), step,
             r"node \(11, 5\) is in the interior-wall table and its g slot 3 is redirected")
    torch.cuda.synchronize()
    walls.close()
    # the context takes a new table on a pre-collision state only
    sv = solver(lib, R, C, bc=BOTTOM)
    sv.set_state(f0, g0)
    sv.step(2)
    _refused(lib, lambda: sv.set_open(table), "ade_solver_set_open", "the state is post-collision")
    sv.set_state(f0, g0)
    sv.set_open(table)
    sv.close()
    table.close()


# ---- 6. entry points agree ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, pylbm.FORM_DEFAULT], ids=["reference_order", "default_form"])
def test_the_context_is_the_raw_entry_points_bit_for_bit(lib, oracle, form):
    R, C, n = 24, 32, 6
    f0, g0 = ade.initial_state(oracle, R, C, seed=8)
    table = aou.channel(R, C, 0.03, 1e-3, 5).table(lib)
    walls = rectangle_table(lib, R, C, -7, 10, 16)
    sv = solver(lib, R, C, form, BOTTOM, walls=walls, table=table)
    sv.set_state(f0, g0)
    sv.step(1 + n)
    sv.sync()
    fc, gc, _, _, cg = sv.lattices()
    g = pylbm.Geom(R, C, 0, cg.plane_stride, cg.row_pitch)  # the raw run on the context's own padded geometry
    (fn, gn), _, _ = raw_run(lib, g, BOTTOM, ade.params(form), f0, g0, n, table, walls=walls)
    for got, want, what in ((fc, fn, "f"), (gc, gn, "g")):
        mine = ade.alloc(g)
        lib.lattice_copy_rows(_ptr(mine), ct.byref(g), 0, _ptr(got), ct.byref(g), 0, R, None)
        torch.cuda.synchronize()
        ade.assert_bits(ade.owned(mine, g), ade.owned(want, g), what)
    sv.close()
    table.close()
    walls.close()


def test_get_state_in_the_middle_of_a_run_does_not_change_the_following_steps(lib, oracle):
    R, C = 24, 32
    f0, g0 = ade.initial_state(oracle, R, C, seed=9)
    segs = aou.channel(R, C, 0.03, 1e-3, 5)
    table = segs.table(lib)
    sv = solver(lib, R, C, REF, BOTTOM, table=table)
    sv.set_state(f0, g0)
    sv.step(3)
    mid = sv.get_state()
    sv.step(4)
    end = sv.get_state()
    sv.close()
    ade.assert_state_bits(mid, aou.loop(oracle, segs, f0, g0, OMEGA, OMEGA_G, W, 3, BOTTOM), "mid-run state")
    ade.assert_state_bits(end, run(lib, f0, g0, 7, bc=BOTTOM, table=table)[0], "the run with a get_state in it")
    ade.assert_state_bits(end, aou.loop(oracle, segs, f0, g0, OMEGA, OMEGA_G, W, 7, BOTTOM), "end state")
    table.close()


def test_a_captured_graph_of_an_even_number_of_steps_replays_the_eager_run(lib, oracle):
    R, C = 24, 32
    f0, g0 = ade.initial_state(oracle, R, C, seed=10)
    table = aou.channel(R, C, 0.03, 1e-3, 5).table(lib)
    kw = dict(form=pylbm.FORM_DEFAULT, bc=BOTTOM, table=table)
    want1, _ = run(lib, f0, g0, 11, **kw)
    want2, _ = run(lib, f0, g0, 21, **kw)
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        sv = solver(lib, R, C, stream=st.value, **kw)
        sv.set_state(f0, g0)
        sv.step(1)
        sv.sync()
        lib.graph_begin_capture(st)
        sv.step(10)  # even: lattices and carries are back where the capture found them
        lib.graph_end_capture(st, ct.byref(graph))
        for want in (want1, want2):
            lib.graph_launch(graph, 1, st)
            lib.stream_sync(st)
            ade.assert_state_bits(sv.get_state(), want, "replay")
        sv.close()
    finally:
        if graph:
            lib.graph_destroy(graph)
        lib.stream_destroy(st)
    table.close()


# ---- 7. a known answer, independent of the yardstick ------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, pylbm.FORM_DEFAULT], ids=["reference_order", "default_form"])
def test_a_uniform_stream_stays_uniform(lib, oracle, form):
    """rho = 1, u = (0, u0) between an ABB inlet at (0, u0), an extrapolated outlet and two specular rows: the
    anti-bounce-back of an equilibrium at rho_w = 1 returns the opposite equilibrium exactly, the extrapolation of a
    uniform u is u, a specular row mirrors a state that is even in c_x -- only rounding remains.  200 steps, 16 x 32."""
    R, C, u0 = 16, 32, 0.05
    s = Segments(R, C)
    s.f(0, 0, 1, 0, R, ALL, ABB, (0.0, u0)).f(0, C - 1, 1, 0, R, ALL, ABB_X, (1.5, -0.5), (0, -1))
    s.f(0, 0, 0, 1, C, mask(1, 5, 8), SPEC_ROW).f(R - 1, 0, 0, 1, C, mask(3, 6, 7), SPEC_ROW)
    table = s.table(lib)
    u = np.zeros((R, C, 2))
    u[..., 1] = u0
    f0 = oracle.equilibrium(u, np.ones((R, C)))
    g0 = oracle.equilibrium(u + np.asarray(W), np.full((R, C), 1e-3))
    out, _ = run(lib, f0, g0, 200, form=form, table=table)
    err_u, err_rho = np.abs(out["u"] - u).max(), np.abs(out["rho"] - 1.0).max()
    print(f"uniform stream after 200 steps: |u - u0| = {err_u:.3e} ({err_u / u0:.3e} of u0), |rho - 1| = {err_rho:.3e}")
    assert err_u <= 1e-13 * u0 and err_rho <= 1e-13
    table.close()


# ---- 8. the driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [0, 1])
def test_rectangle_sedimentation_driver_fused_vs_oracle(tmp_path, oracle, fast):
    """drivers/rectangle_sedimentation_test --fused 1 on the 540 x 420 lattice of tests/test_gpu_drivers.py, 60 steps: one
    iteration at operator level, 59 fused; equal bit patterns in the reference operation order, 1e-10 reassociated"""
    toml = open(os.path.join(PKG, "examples", "parameters.toml")).read()
    toml = toml.replace("characteristic_velocity = 0.5", "characteristic_velocity = 0.03")
    toml = toml.replace("lattice_spacing = 2.0E-5", "lattice_spacing = 1.0E-4")
    (tmp_path / "sed.toml").write_text(toml)
    lp = json.loads(run_driver("params_dump", tmp_path / "sed.toml", timeout=60).stdout)["lattice"]
    X, Y, steps = lp["X"], lp["Y"], 60
    assert (X, Y) == (540, 420) and lp["u"] < 0.06
    r = run_driver("rectangle_sedimentation_test", tmp_path / "sed.toml", "--steps", steps, "--dump", tmp_path / "sed",
                   "--fused", 1, "--time", 1, timeout=300, tune=f"bgk_fast={fast}")
    assert f"(fused, {steps - 1} steps, {2 + 4 * (steps - 2)} launches)" in r.stdout, r.stdout[-500:]
    want = oracle.sed_steps(X, Y, lp["omega"], lp["u"], steps)
    assert want["C"].max() > 5e-4 and np.isfinite(want["f"]).all()
    shapes = dict(f=(X, Y, 9), g=(X, Y, 9), rho=(X, Y), u=(X, Y, 2), C=(X, Y))
    got = {k: np.fromfile(tmp_path / f"sed-{k}.f64").reshape(shp) for k, shp in shapes.items()}
    if fast:
        errs = {k: relerr(got[k], want[k]) for k in shapes}
        print("fused driver, reassociated, vs oracle after 60 steps:", errs)
        assert max(errs.values()) <= 1e-10, errs
    else:
        ade.assert_state_bits(got, want, "fused driver vs oracle after 60 steps")
