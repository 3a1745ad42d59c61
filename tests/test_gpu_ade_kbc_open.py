"""GPU suite, open boundaries and the wall exchange of the fluid + scalar step with a KBC fluid: lbm_ade_open_collide_m,
lbm_ade_open_stream_collide_m, lbm_ade_solver_set_open_m, lbm_ade_wallx_rows_m, lbm_ade_solver_wall_exchange_m
(pylbm.AdeSolver.set_open_m / wall_exchange_m; capi_ade_kbc_open.hip) and the driver sedimentation_channel.

The yardstick is tests/ade_kbc_open_util.py: the driver's iteration composed on the CPU from the KBC collisions of
tests/ade_kbc_util.py / ade_kbc_buoyancy_util.py, the open stream of tests/ade_open_util.py and the exchange definition of
tests/ade_exchange_reference.py.  It never calls the library under test, is computed once per case (cached, read-only) and
is asserted finite before anything is compared with it: every start state is off equilibrium (ade_util.initial_state),
since KBC's gamma is 0/0 on a lattice at equilibrium, and equal NaNs are equal bits.  Bitwise means equal bit patterns.
The only tolerances: the reassociated / default form against the reference order, relative L2 <= 1e-12 on f and on g after
20 steps (the bound tests/test_gpu_ade_kbc.py states for the KBC forms at <= 20 steps), and the wall exchange in the default
form, 1e-10 of the largest value after 100 steps (the bound of tests/test_gpu_ade_wall_exchange.py).
s2 = 1.9, w = (3e-3, -2e-3), u_in = 0.03; buoyant: beta = (1.2e-2, -8e-3), c_ref = 0.4, u_shift = 1.
Shapes of the channel: 4 x 4 (every node is listed or beside a listed one), 16 x 16, 5 x 1040 at a row pitch of 1056 (odd
rows, more than four workgroups of listed nodes in one dispatch); a hand-built table on 6 x 8.  The chain of slabs is 16 +
20 + 12 rows x 64 columns, the lattice of the 68-node body of tests/ade_slab_util.py (it stands in columns 20..30)."""
import ctypes as ct
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ade_calls  # noqa: E402
import ade_exchange_reference as xref  # noqa: E402
import ade_kbc_buoyancy_slab_calls as mb  # noqa: E402
import ade_kbc_open_util as yo  # noqa: E402
import ade_kbc_util as kbc  # noqa: E402
import ade_open_util as aou  # noqa: E402
import ade_util as ade  # noqa: E402
import pylbm  # noqa: E402
from ade_kbc_open_util import OMEGA_G, S2, U_IN, W  # noqa: E402
from ade_open_util import ABB, ABB_X, ALL, BB_RULE, SPEC_COL, SPEC_ROW, Segments, mask  # noqa: E402
from ade_slab_util import Chain, assert_finite, body_table  # noqa: E402
from ade_util import GBC, SENTINEL  # noqa: E402
from gpu_util import bits_equal, dev  # noqa: E402
from proc_util import key_values, run_driver  # noqa: E402
from pylbm import _ptr  # noqa: E402

REF, FAST, DEFAULT = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED, pylbm.FORM_DEFAULT
BB = pylbm.EDGE_BOUNCE_BACK
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_NEG, COL_POS, COL_NEG = pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_POS, pylbm.ADE_FACE_COL_NEG
NQ = pylbm.WALLX_NQ
BOTTOM = pylbm.Bc(row_hi=BB)
ROWS_BB = pylbm.Bc(row_lo=BB, row_hi=BB)
SHAPES = {"4x4": (4, 4, 0), "16x16": (16, 16, 0), "5x1040": (5, 1040, 1056), "6x8": (6, 8, 0)}
ITERATIONS = (1, 2, 20)
FLUIDS = pytest.mark.parametrize("buoyant", [False, True], ids=["passive", "buoyant"])


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(autouse=True)
def _default_knobs_afterwards(lib):
    yield
    lib.reset_tuning()


# ---- the cases: an open table, the domain's edges, the scalar's FIXED row, a body ------------------------------------------
def rectangle(lib, R, C, r_top, c1, c2, side=(NO_FLUX, 0.0), top=(FIXED, 1e-3)):
    """the driver's rectangle standing on the last row: two side walls (f stops one row short of the last row; the first
    wall's g runs through it, slot 7 of the foot left to the bottom wall) and a ceiling, each with its own scalar rule"""
    t = pylbm.AdeInteriorWalls(lib, R, C)
    first = r_top + R + 1
    if R - 1 - first > 0:
        t.add(first, c1, 1, 0, R - 1 - first, COL_NEG, COL_NEG, *side)
        t.add(first, c2, 1, 0, R - 1 - first, COL_POS, COL_POS, *side)
    t.add(-1, c1, 1, 0, 1, 0, COL_NEG & ~(1 << 6), *side)
    t.add(r_top, c1, 0, 1, c2 - c1 + 1, ROW_NEG, ROW_NEG, *top)
    return t.finalize()


BODY = {"16x16": (-6, 6, 9), "5x1040": (-3, 500, 540)}  # r_top, c_first, c_second: clear of the redirected row 0


def hand_table(R, C):
    """every f rule, both g rules and two chained copies on a periodic box: an ABB inlet with a FIXED scalar on column 0,
    an outlet extrapolating from the DIAGONAL neighbour (r + 1, c - 1) on column C-1 above the last row, a specular first
    row, a bounce-back last row with a NO_FLUX scalar, a specular column inside, and the copies row 0 <- row 1, then
    column C-1 <- column C-2 over all rows (its corner reads the first copy's result)"""
    s = Segments(R, C)
    s.copy(0, 0, 0, 1, C, (1, 0)).copy(0, C - 1, 1, 0, R, (0, -1))
    s.f(0, 0, 1, 0, R, ALL, ABB, (2e-3, U_IN))
    s.f(0, C - 1, 1, 0, R - 1, ALL, ABB_X, (1.5, -0.5), (1, -1))
    s.f(0, 1, 0, 1, C - 2, mask(1, 5, 8), SPEC_ROW)
    s.f(R - 1, 1, 0, 1, C - 2, mask(3, 6, 7), BB_RULE)
    s.f(2, 3, 1, 0, 2, mask(2, 5, 6), SPEC_COL)
    s.g(0, 0, 1, 0, R, ALL, FIXED, 1e-3)
    s.g(R - 1, 1, 0, 1, C - 2, mask(3, 6, 7), NO_FLUX)
    return s


CASES = ("channel", "fixed_row", "body", "hand")


def case_of(lib, case, shape):
    """(segments, domain edges, FIXED spec of the scalar's rows, interior walls or None) of a case"""
    R, C, _ = SHAPES[shape]
    if case == "hand":
        return hand_table(R, C), pylbm.Bc(), {}, None
    segs = aou.channel(R, C, U_IN, yo.CONC_W, max(2, R // 2))
    spec = {"row_hi": ("profile", np.linspace(2e-4, 1.2e-3, C))} if case == "fixed_row" else {}
    return segs, BOTTOM, spec, (rectangle(lib, R, C, *BODY[shape]) if case == "body" else None)


def start_state(oracle, R, C, buoyant):
    f, g = (ade.buoyant_initial_state if buoyant else ade.initial_state)(oracle, R, C, seed=R * C + 1, w=W)
    return f, g


_YARD = {}


def yardstick(lib, oracle, case, shape, buoyant, iterations=ITERATIONS):
    """{0: the start state, n: the state after n iterations}, computed once per case, read-only, finite (yo.loop asserts)"""
    key = (case, shape, buoyant, tuple(iterations))
    if key not in _YARD:
        R, C, _ = SHAPES[shape]
        segs, bc, spec, walls = case_of(lib, case, shape)
        fixed = ade.build_sbc(spec, R, C)[1] if spec else {}
        nodes = walls.nodes() if walls is not None else None
        f, g = start_state(oracle, R, C, buoyant)
        out, done = {0: dict(f=f, g=g)}, 0
        for n in iterations:
            st = yo.loop(oracle, segs, f, g, n - done, bc, fixed, nodes, yo.buoyancy() if buoyant else None)
            f, g, done = st["f"], st["g"], n
            out[n] = st
        for st in out.values():
            for v in st.values():
                v.setflags(write=False)
        if walls is not None:
            walls.close()
        _YARD[key] = out
    return _YARD[key]


# ---- running the library ---------------------------------------------------------------------------------------------------
def params(form=REF, model="kbc"):
    if model == "kbc":
        return kbc.params(form, s2=S2, w=W)
    return pylbm.AdeFluid(pylbm.BgkParams(1.2, 0, form=form)), pylbm.AdeParams(OMEGA_G, W, form=form)


def ref_(x):
    return ct.byref(x) if x is not None else None


def handle(t):
    return t.h if t is not None else None


def open_collide_m(lib, g, bc, prm, dst, src, table, carry_out, sbc=None, by=None, moments=None, stream=None):
    m = moments if moments is not None else (None, None, None)
    lib.ade_open_collide_m(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), ct.byref(g), ct.byref(bc), ct.byref(prm[0]),
                           ct.byref(prm[1]), ref_(sbc), ref_(by), handle(table), _ptr(carry_out), *[_ptr(t) for t in m],
                           pylbm._stream(stream))


def open_step_m(lib, g, bc, prm, dst, src, table, carry_in, carry_out, sbc=None, by=None, walls=None, moments=None, rows=None,
                stream=None):
    m = moments if moments is not None else (None, None, None)
    r0, r1 = rows if rows is not None else (0, g.R)
    lib.ade_open_stream_collide_m(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), ct.byref(g), ct.byref(bc),
                                  ct.byref(prm[0]), ct.byref(prm[1]), ref_(sbc), ref_(by), handle(walls), handle(table),
                                  _ptr(carry_in), _ptr(carry_out), int(r0), int(r1), *[_ptr(t) for t in m], pylbm._stream(stream))


def box4(region):
    return (ct.c_int * 4)(*region) if region is not None else None


def wallx_rows_m(lib, out, table_rows, row0, g, bc, prm, fo, go, walls, sbc=None, by=None, region=None, rows=None, stream=None):
    r0, r1 = rows if rows is not None else (0, g.R)
    lib.ade_wallx_rows_m(_ptr(out), int(table_rows), int(row0), _ptr(fo), _ptr(go), ct.byref(g), ct.byref(bc), ct.byref(prm[0]),
                         ct.byref(prm[1]), ref_(sbc), ref_(by), handle(walls), box4(region), int(r0), int(r1),
                         pylbm._stream(stream))


def raw_exchange_m(lib, g, bc, prm, fo, go, walls, **kw):
    """(values, row table) of one block through lbm_ade_wallx_rows_m + lbm_ade_wallx_fold"""
    tab = torch.zeros(NQ * g.R, dtype=torch.float64, device=dev())
    ade.bits(tab).fill_(SENTINEL)
    out = torch.zeros(NQ, dtype=torch.float64, device=dev())
    wallx_rows_m(lib, tab, g.R, 0, g, bc, prm, fo, go, walls, **kw)
    lib.ade_wallx_fold(_ptr(out), _ptr(tab), g.R, 0, g.R, None)
    torch.cuda.synchronize()
    return out.cpu().numpy(), tab.cpu().numpy().reshape(NQ, g.R)


def carry_buffer(table, extra=0):
    t = torch.zeros((table.carry_len() if table is not None else 0) + extra, dtype=torch.float64, device=dev())
    ade.bits(t).fill_(SENTINEL)
    return t


def solver(lib, R, C, form=REF, bc=None, sbc=None, by=None, walls=None, table=None, stream=None, model="kbc"):
    fluid, scalar = params(form, model)
    return pylbm.AdeSolver(lib, R, C, fluid, scalar, bc=bc, stream=stream, scalar_bc=sbc, buoyancy=by, walls=walls, open=table)


def moments_np(m, R, C):
    return dict(rho=m[0].cpu().numpy().reshape(R, C), u=m[1].cpu().numpy().reshape(2, R, C).transpose(1, 2, 0),
                C=m[2].cpu().numpy().reshape(R, C))


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


def assert_np_bits(got, want, what):
    assert bits_equal(got, want), f"{what}: max |d| = {np.max(np.abs(np.asarray(got) - np.asarray(want)))}"


# ---- 1. bitwise in the reference order -------------------------------------------------------------------------------------
RUNS = [(c, s) for c in ("channel", "fixed_row") for s in ("4x4", "16x16", "5x1040")] + [("body", "16x16"), ("body", "5x1040"),
                                                                                        ("hand", "6x8")]


@FLUIDS
@pytest.mark.parametrize("case,shape", RUNS, ids=[f"{c}-{s}" for c, s in RUNS])
def test_raw_calls_and_context_are_the_yardstick_bit_for_bit(lib, oracle, case, shape, buoyant):
    """reference order, after 1, 2 and 20 iterations.  Raw: lbm_ade_open_collide_m, then lbm_ade_open_stream_collide_m step by
    step into poisoned targets -- the post-collision pair, the moments (the shifted u of a buoyant step) and carry_out (the
    unshifted u of the fixed-up f).  Context: set_open_m, step, get_state (the unshifted u)."""
    R, C, pitch = SHAPES[shape]
    yard = yardstick(lib, oracle, case, shape, buoyant)
    segs, bc, spec, walls = case_of(lib, case, shape)
    sbc = ade.build_sbc(spec, R, C)[0] if spec else None
    by = yo.buoyancy() if buoyant else None
    table = segs.table(lib)
    g, prm = ade.geom(R, C, 0, pitch), params(REF)
    src = (ade.to_lattice(yard[0]["f"], g), ade.to_lattice(yard[0]["g"], g))
    cin, dst = carry_buffer(table), (ade.poisoned(g), ade.poisoned(g))
    open_collide_m(lib, g, bc, prm, dst, src, table, cin, sbc=sbc, by=by)
    torch.cuda.synchronize()
    assert_np_bits(cin.cpu().numpy(), aou.carry_of(table, aou.calc_u(oracle, yard[0]["f"])), "the collide-only call's carry")
    for n in range(1, max(ITERATIONS) + 1):
        src, dst, cout, m = dst, (ade.poisoned(g), ade.poisoned(g)), carry_buffer(table), ade.moment_fields(g)
        open_step_m(lib, g, bc, prm, dst, src, table, cin, cout, sbc=sbc, by=by, walls=walls, moments=m)
        cin = cout
        if n not in ITERATIONS:
            continue
        torch.cuda.synchronize()
        c = yo.collide(oracle, yard[n]["f"], yard[n]["g"], by)
        assert yo.finite(c)
        got = dict(fc=ade.from_lattice(dst[0], g), gc=ade.from_lattice(dst[1], g), carry=cout.cpu().numpy(), **moments_np(m, R, C))
        want = dict(fc=c["fc"], gc=c["gc"], carry=aou.carry_of(table, yard[n]["u"]), rho=c["rho"], u=c["u"], C=c["C"])
        for k in want:
            assert_np_bits(got[k], want[k], f"raw, {case} {shape} after {n} steps: {k}")
        for t, name in zip(dst, "fg"):
            ade.assert_write_set(t, g, slice(0, R), name)
    sv = solver(lib, R, C, REF, bc, sbc, by, walls, table)
    sv.set_state(yard[0]["f"], yard[0]["g"])
    done = 0
    for n in ITERATIONS:
        sv.step(n - done)
        done = n
        ade.assert_state_bits(sv.get_state(), yard[n], f"context, {case} {shape} after {n} iterations")
    sv.close()
    plain = kbc.oracle_loop(oracle, yard[0]["f"], yard[0]["g"], S2, OMEGA_G, W, 2, bc) if not buoyant else None
    if plain is not None:  # the table is felt
        assert not bits_equal(plain["f"], yard[2]["f"]) and not bits_equal(plain["g"], yard[2]["g"])
    table.close()
    if walls is not None:
        walls.close()


def test_every_launch_variant(lib, oracle):
    """5 x 1040 with the body: all four `nt` settings x grid_cap 0, 1, 7, two raw steps with moments and carries: each bit
    for bit the default launch, which is the yardstick"""
    case, shape = "body", "5x1040"
    R, C, pitch = SHAPES[shape]
    yard = yardstick(lib, oracle, case, shape, False)
    segs, bc, _, walls = case_of(lib, case, shape)
    table, g, prm = segs.table(lib), ade.geom(R, C, 0, pitch), params(REF)
    src = (ade.to_lattice(yard[0]["f"], g), ade.to_lattice(yard[0]["g"], g))

    def two_steps():
        c0, post = carry_buffer(table), (ade.alloc(g), ade.alloc(g))
        open_collide_m(lib, g, bc, prm, post, src, table, c0)
        cur, cin = post, c0
        for _ in range(2):
            dst, cout, m = (ade.poisoned(g), ade.poisoned(g)), carry_buffer(table), ade.moment_fields(g)
            open_step_m(lib, g, bc, prm, dst, cur, table, cin, cout, walls=walls, moments=m)
            cur, cin = dst, cout
        torch.cuda.synchronize()
        return [*cur, cin, *m]

    base = two_steps()
    c = yo.collide(oracle, yard[2]["f"], yard[2]["g"])
    assert_np_bits(ade.from_lattice(base[0], g), c["fc"], "default launch against the yardstick: f")
    assert_np_bits(ade.from_lattice(base[1], g), c["gc"], "default launch against the yardstick: g")
    for nt in (0, 1, 2, 3):
        for cap in (0, 1, 7):
            lib.set_tuning(b"nt", nt)
            lib.set_tuning(b"grid_cap", cap)
            for k, (got, want) in enumerate(zip(two_steps(), base)):
                ade.assert_bits(got, want, f"nt={nt} grid_cap={cap}: output {k}")
    table.close()
    walls.close()


# ---- 2. the reassociated and the default form against the reference order ---------------------------------------------------
@pytest.mark.parametrize("case,shape", [("channel", "16x16"), ("body", "5x1040"), ("hand", "6x8")])
def test_other_forms_agree_with_the_reference_order(lib, oracle, case, shape):
    """20 steps through the context: relative L2 on f and on g <= 1e-12 (the bound of tests/test_gpu_ade_kbc.py for the KBC
    forms at <= 20 steps); a buoyant step in the default form IS the reference-order step"""
    R, C, _ = SHAPES[shape]
    segs, bc, _, walls = case_of(lib, case, shape)
    table = segs.table(lib)
    for buoyant in (False, True):
        yard = yardstick(lib, oracle, case, shape, buoyant)
        for name, form in (("reassociated", FAST), ("default", DEFAULT)):
            sv = solver(lib, R, C, form, bc, None, yo.buoyancy() if buoyant else None, walls, table)
            sv.set_state(yard[0]["f"], yard[0]["g"])
            sv.step(20)
            got = sv.get_state()
            sv.close()
            if buoyant:
                ade.assert_state_bits(got, yard[20], f"{case} {shape}, buoyant, {name} form")
                continue
            errs = {k: rel_l2(got[k], yard[20][k]) for k in "fg"}
            print(f"{case} {shape} {name} form vs reference order after 20 steps: relative L2 {errs}")
            assert np.all(np.isfinite(got["f"])) and np.all(np.isfinite(got["g"]))
            assert max(errs.values()) <= 1e-12, errs
    table.close()
    if walls is not None:
        walls.close()


# ---- 3. identities -----------------------------------------------------------------------------------------------------------
@FLUIDS
@pytest.mark.parametrize("form", [REF, DEFAULT], ids=["reference_order", "default_form"])
def test_null_and_the_empty_table_are_the_mb_calls(lib, oracle, form, buoyant):
    """lbm_ade_collide_mb / lbm_ade_stream_collide_mb bit for bit, no carry asked for; the same launches on a context"""
    R, C = 16, 16
    g, prm, by = ade.geom(R, C, 0, 24), params(form), (yo.buoyancy() if buoyant else None)
    f0, g0 = start_state(oracle, R, C, buoyant)
    walls = rectangle(lib, R, C, *BODY["16x16"])
    empty = pylbm.AdeOpenBoundary(lib, R, C).finalize()
    pre = (ade.to_lattice(f0, g), ade.to_lattice(g0, g))
    post, mw = (ade.alloc(g), ade.alloc(g)), ade.moment_fields(g)
    ade_calls.collide(lib, "_mb", g, BOTTOM, prm, post, pre, buoy=by, moments=mw)
    want_m = ade.moment_fields(g)
    want = ade_calls.full_step(lib, "_mb", g, BOTTOM, prm, *post, buoy=by, iwalls=walls, moments=want_m)
    torch.cuda.synchronize()
    assert_finite(want, g, "the _mb step")
    for table in (None, empty):
        dst, m = (ade.alloc(g), ade.alloc(g)), ade.moment_fields(g)
        open_collide_m(lib, g, BOTTOM, prm, dst, pre, table, None, by=by, moments=m)
        for got, ref in zip((*dst, *m), (*post, *mw)):
            ade.assert_bits(got, ref, "collide-only")
        dst, m = (ade.alloc(g), ade.alloc(g)), ade.moment_fields(g)
        open_step_m(lib, g, BOTTOM, prm, dst, post, table, None, None, by=by, walls=walls, moments=m)
        for got, ref in zip((*dst, *m), (*want, *want_m)):
            ade.assert_bits(got, ref, "step")
    launches = []
    for table in ("none", None, empty):
        sv = solver(lib, R, C, form, BOTTOM, None, by, walls)
        if table != "none":
            sv.set_open_m(table)
        sv.set_state(f0, g0)
        sv.step(5)
        launches.append(sv.launches())
        sv.close()
    assert launches == [1 + 3 * 4] * 3  # collide-only; interior + edge pass + interior walls
    empty.close()
    walls.close()


@pytest.mark.parametrize("buoyant", [False, True], ids=["passive", "buoyant"])
def test_model_bgk_through_the_new_calls_is_the_bgk_calls(lib, oracle, buoyant):
    """lbm_ade_collide_o, lbm_ade_stream_collide_o, lbm_ade_wallx_rows and, on a BGK context, set_open and wall_exchange:
    the same bits and the same launches"""
    R, C = 16, 16
    g, prm_m = ade.geom(R, C, 0, 24), params(DEFAULT, "bgk")
    prm = (prm_m[0].bgk, prm_m[1])
    by = ade.buoyancy((2e-3, -1.5e-3), 0.4, ade.GUO) if buoyant else None
    f0, g0 = start_state(oracle, R, C, buoyant)
    walls = rectangle(lib, R, C, *BODY["16x16"])
    table = aou.channel(R, C, U_IN, yo.CONC_W, 8).table(lib)
    pre = (ade.to_lattice(f0, g), ade.to_lattice(g0, g))
    a, b = [(ade.alloc(g), ade.alloc(g)) for _ in range(2)]
    ca, cb = carry_buffer(table), carry_buffer(table)
    ade_calls.collide(lib, "_o", g, BOTTOM, prm, a, pre, buoy=by, open=table, carry_out=ca)
    open_collide_m(lib, g, BOTTOM, prm_m, b, pre, table, cb, by=by)
    for got, want in zip((*b, cb), (*a, ca)):
        ade.assert_bits(got, want, "collide-only")
    a2, b2 = [(ade.alloc(g), ade.alloc(g)) for _ in range(2)]
    ca2, cb2, ma, mb_ = carry_buffer(table), carry_buffer(table), ade.moment_fields(g), ade.moment_fields(g)
    ade_calls.step_into(lib, "_o", g, BOTTOM, prm, a2, a, buoy=by, iwalls=walls, open=table, carry_in=ca, carry_out=ca2, moments=ma)
    open_step_m(lib, g, BOTTOM, prm_m, b2, a, table, ca, cb2, by=by, walls=walls, moments=mb_)
    torch.cuda.synchronize()
    assert_finite(a2, g, "the _o step")
    for got, want in zip((*b2, cb2, *mb_), (*a2, ca2, *ma)):
        ade.assert_bits(got, want, "step")
    tabs = [torch.zeros(NQ * R, dtype=torch.float64, device=dev()) for _ in range(2)]
    lib.ade_wallx_rows(_ptr(tabs[0]), R, 0, _ptr(a2[0]), _ptr(a2[1]), ct.byref(g), ct.byref(BOTTOM), ct.byref(prm[0]),
                       ct.byref(prm[1]), None, ref_(by), walls.h, None, 0, R, None)
    wallx_rows_m(lib, tabs[1], R, 0, g, BOTTOM, prm_m, a2[0], a2[1], walls, by=by)
    torch.cuda.synchronize()
    ade.assert_bits(tabs[1], tabs[0], "wall exchange rows")
    assert float(tabs[0].view(NQ, R)[pylbm.WALLX_NODES].sum()) == walls.count()
    out = []
    for new in (False, True):
        sv = pylbm.AdeSolver(lib, R, C, prm_m[0] if new else prm[0], prm[1], bc=BOTTOM, walls=walls)
        (sv.set_buoyancy_m if new else sv.set_buoyancy)(by)
        (sv.set_open_m if new else sv.set_open)(table)
        sv.set_state(f0, g0)
        sv.step(6)
        out.append((sv.get_state(), (sv.wall_exchange_m if new else sv.wall_exchange)(table=True), sv.launches()))
        sv.close()
    ade.assert_state_bits(out[1][0], out[0][0], "context state")
    assert_np_bits(out[1][1][0], out[0][1][0], "context wall exchange")
    assert_np_bits(out[1][1][1], out[0][1][1], "context wall exchange row table")
    assert out[1][2] == out[0][2] == 2 + 4 * 5
    table.close()
    walls.close()


# ---- 4. write set and launches -----------------------------------------------------------------------------------------------
@FLUIDS
def test_the_open_pass_writes_its_nodes_and_its_carry_and_one_launch(lib, oracle, buoyant):
    """the step with the table against the step without: every double of fn, gn and the moments outside the listed nodes is
    the table-less step's (the open pass writes listed nodes only), carry_out is written for exactly the listed nodes, no
    input changes; the collide-only call writes the same carry entries.  On a context a table costs one launch per step and
    one for the collide-only iteration"""
    R, C = 12, 16
    g, prm, by = ade.geom(R, C, 0, 24), params(REF), (yo.buoyancy() if buoyant else None)
    f0, g0 = start_state(oracle, R, C, buoyant)
    table = aou.channel(R, C, U_IN, yo.CONC_W, 4).table(lib)
    n = table.carry_len()
    assert n == 2 * table.count() > 0
    listed = torch.zeros(R, C, dtype=torch.bool, device=dev())
    for nd in table.nodes():
        listed[nd["r"], nd["c"]] = True
    assert not bool(listed.all())
    src = (ade.to_lattice(f0, g), ade.to_lattice(g0, g))
    cin = torch.from_numpy(np.random.default_rng(1).normal(0.0, 0.01, n)).to(dev())
    keep = [t.clone() for t in (*src, cin)]
    plain, mp = (ade.poisoned(g), ade.poisoned(g)), ade.moment_fields(g)
    open_step_m(lib, g, BOTTOM, prm, plain, src, None, None, None, by=by, moments=mp)
    dst, cout, m = (ade.poisoned(g), ade.poisoned(g)), carry_buffer(table, extra=32), ade.moment_fields(g)
    open_step_m(lib, g, BOTTOM, prm, dst, src, table, cin, cout, by=by, moments=m)
    torch.cuda.synchronize()
    for t, p, what in zip(dst, plain, "fg"):
        ade.assert_write_set(t, g, slice(0, R), what)
        differs = (ade.bits(ade.owned(t, g)) != ade.bits(ade.owned(p, g))).any(dim=0)
        assert bool(differs.any()) and not bool((differs & ~listed).any()), f"{what}: changed outside the listed nodes"
    for t, p, planes in zip(m, mp, (1, 2, 1)):
        differs = (ade.bits(t).view(planes, R, C) != ade.bits(p).view(planes, R, C)).any(dim=0)
        assert not bool((differs & ~listed).any()) and bool((ade.bits(t) != SENTINEL).all())
    written = ade.bits(cout) != SENTINEL
    assert bool(written[:n].all()) and not bool(written[n:].any())
    for t, k in zip((*src, cin), keep):
        ade.assert_bits(t, k, "an input of the step")
    cout2 = carry_buffer(table, extra=32)
    open_collide_m(lib, g, BOTTOM, prm, (ade.poisoned(g), ade.poisoned(g)), src, table, cout2, by=by)
    torch.cuda.synchronize()
    written = ade.bits(cout2) != SENTINEL
    assert bool(written[:n].all()) and not bool(written[n:].any())
    assert_np_bits(cout2[:n].cpu().numpy(), aou.carry_of(table, aou.calc_u(oracle, f0)), "the collide-only call's carry")
    launches = {}
    for name, t in (("none", None), ("table", table)):
        for steps in (1, 8):
            sv = solver(lib, R, C, DEFAULT, BOTTOM, None, by, None, t)
            sv.set_state(f0, g0)
            sv.step(steps)
            launches[name, steps] = sv.launches()
            sv.close()
    assert launches["none", 1] == 1 and launches["none", 8] == 1 + 2 * 7
    assert launches["table", 1] == 2 and launches["table", 8] == 2 + 3 * 7  # interior + edge pass + the open pass
    table.close()


# ---- 5. graph ---------------------------------------------------------------------------------------------------------------
def test_a_captured_graph_keeps_the_table_and_the_descriptor_of_its_capture(lib, oracle):
    """a buoyant context's steps captured (an even number: lattices and carries end where they began) and replayed after
    the context was given another descriptor and the caller's table variable names another table: the eager runs"""
    R, C = 24, 32
    f0, g0 = start_state(oracle, R, C, True)
    table = aou.channel(R, C, U_IN, yo.CONC_W, 5).table(lib)
    other_table = aou.channel(R, C, 0.05, 5e-4, 9).table(lib)
    walls = rectangle(lib, R, C, -7, 10, 16)
    want = []
    for steps in (11, 21):
        sv = solver(lib, R, C, DEFAULT, BOTTOM, None, yo.buoyancy(), walls, table)
        sv.set_state(f0, g0)
        sv.step(steps)
        want.append(sv.get_state())
        sv.close()
    assert yo.finite(want[1]) and not bits_equal(want[0]["f"], want[1]["f"])
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        by = yo.buoyancy()
        sv = solver(lib, R, C, DEFAULT, BOTTOM, None, by, walls, table, stream=st.value)
        sv.set_state(f0, g0)
        sv.step(1)
        sv.sync()
        before = sv.launches()
        lib.graph_begin_capture(st)
        sv.step(10)
        lib.graph_end_capture(st, ct.byref(graph))
        assert sv.launches() - before == 4 * 10  # the captured steps are counted: interior, edge, open, interior walls
        by.beta_r, by.beta_c, by.c_ref = -3e-2, 2e-2, 0.1
        sv.set_buoyancy_m(by)  # the context's descriptor changes: the graph holds the one of its capture
        captured, table = table, other_table  # ... and so does what the caller calls its table
        for k in range(2):
            lib.graph_launch(graph, 1, st)
            lib.stream_sync(st)
            ade.assert_state_bits(sv.get_state(), want[k], f"replay {k}")
        sv.close()
    finally:
        if graph:
            lib.graph_destroy(graph)
        lib.stream_destroy(st)
    for t in (captured, other_table, walls):
        t.close()


# ---- 6. wall exchange ---------------------------------------------------------------------------------------------------------
def exchange_case(lib, shape):
    """(R, C, interior walls): 16 x 16 -- the rectangle, NO_FLUX sides and a FIXED ceiling; 48 x 1040 -- the 68-node body"""
    if shape == "16x16":
        return 16, 16, rectangle(lib, 16, 16, *BODY["16x16"])
    walls = body_table(lib, 48, 1040, (FIXED, 0.6))
    assert walls.count() == 68
    return 48, 1040, walls


@FLUIDS
@pytest.mark.parametrize("shape", ["16x16", "48x1040"])
def test_the_wall_exchange_is_the_definition_bit_for_bit(lib, oracle, shape, buoyant):
    """reference order, bounce-back rows with a FIXED row_lo, after 1, 2 and 5 steps: wall_exchange_m of a KBC context and
    lbm_ade_wallx_rows_m + lbm_ade_wallx_fold on its lattices against ade_exchange_reference on the yardstick's
    post-collision lattices -- values and row table, whole and with a region and a row range"""
    R, C, walls = exchange_case(lib, shape)
    nodes = walls.nodes()
    by = yo.buoyancy() if buoyant else None
    sbc, fixed = ade.build_sbc({"row_lo": 7e-4}, R, C)
    f0, g0 = start_state(oracle, R, C, buoyant)
    region = (2, R - 3, 5, 28)
    rows = (3, R - 1)
    sv = solver(lib, R, C, REF, ROWS_BB, sbc, by, walls)
    sv.set_state(f0, g0)
    with pytest.raises(pylbm.LbmError, match=r"-> -3: lbm_ade_solver_wall_exchange_m: the state is pre-collision"):
        sv.wall_exchange_m()
    done = 0
    for n in (1, 2, 5):
        sv.step(n - done)
        done = n
        st, want_table = yo.exchange_loop(oracle, f0, g0, n, ROWS_BB, fixed, nodes, by)
        got, got_table = sv.wall_exchange_m(table=True)
        assert_np_bits(got_table, want_table, f"{shape} row table after {n} steps")
        assert_np_bits(got, xref.fold_table(want_table), f"{shape} values after {n} steps")
        state = sv.get_state()
        assert bits_equal(state["f"], st["f"]) and bits_equal(state["g"], st["g"]), "the yardstick's stream"
        assert got[pylbm.WALLX_NODES] == len(nodes) and abs(got[pylbm.WALLX_SCALAR]) > 0.0 and abs(got[pylbm.WALLX_FORCE_C]) > 0.0
        _, want_part = yo.exchange_loop(oracle, f0, g0, n, ROWS_BB, fixed, nodes, by, region)
        part, part_table = sv.wall_exchange_m(region=region, row_begin=rows[0], row_end=rows[1], table=True)
        assert_np_bits(part_table[:, rows[0]:rows[1]], want_part[:, rows[0]:rows[1]], "a region and a row range: row table")
        assert_np_bits(part, xref.fold_table(want_part, *rows), "a region and a row range: values")
        assert 0 < part[pylbm.WALLX_NODES] < len(nodes)
        f_cur, g_cur, _, _, geom = sv.lattices()
        raw, raw_table = raw_exchange_m(lib, geom, ROWS_BB, params(REF), f_cur, g_cur, walls, sbc=sbc, by=by)
        assert_np_bits(raw_table, want_table, "raw row table")
        assert_np_bits(raw, got, "raw values")
    sv.close()
    walls.close()


def test_the_wall_exchange_in_the_default_form(lib, oracle):
    """100 steps, default form against the reference order: 1e-10 of the largest magnitude among the values"""
    R, C, walls = exchange_case(lib, "16x16")
    f0, g0 = start_state(oracle, R, C, False)
    sbc = pylbm.AdeScalarBC(row_lo=7e-4)
    out = {}
    for form in (REF, DEFAULT):
        sv = solver(lib, R, C, form, ROWS_BB, sbc, None, walls)
        sv.set_state(f0, g0)
        sv.step(100)
        out[form] = sv.wall_exchange_m()
        sv.close()
    assert np.all(np.isfinite(out[REF])) and np.all(np.isfinite(out[DEFAULT]))
    scale = np.max(np.abs(out[REF][:pylbm.WALLX_NODES]))
    err = np.max(np.abs(out[DEFAULT] - out[REF])) / scale
    print("default form vs reference order, KBC wall exchange after 100 steps:", err, out[REF].tolist())
    assert err <= 1e-10
    assert out[DEFAULT][pylbm.WALLX_NODES] == out[REF][pylbm.WALLX_NODES] == walls.count()
    walls.close()


@FLUIDS
def test_the_open_table_plays_no_part_in_the_exchange(lib, oracle, buoyant):
    """the channel set on the context as well: wall_exchange_m is lbm_ade_wallx_rows_m on the context's lattices, which
    takes no open table"""
    R, C = 24, 32
    by = yo.buoyancy() if buoyant else None
    f0, g0 = start_state(oracle, R, C, buoyant)
    walls = rectangle(lib, R, C, -7, 10, 16)
    channel = aou.channel(R, C, U_IN, yo.CONC_W, 6).table(lib)
    sv = solver(lib, R, C, DEFAULT, BOTTOM, None, by, walls, channel)
    sv.set_state(f0, g0)
    for n in (1, 3):
        sv.step(n)
        got, got_table = sv.wall_exchange_m(table=True)
        f_cur, g_cur, _, _, geom = sv.lattices()
        want, want_table = raw_exchange_m(lib, geom, BOTTOM, params(DEFAULT), f_cur, g_cur, walls, by=by)
        assert np.all(np.isfinite(want_table)) and want[pylbm.WALLX_NODES] == walls.count()
        assert_np_bits(got_table, want_table, "row table")
        assert_np_bits(got, want, "values")
    sv.close()
    channel.close()
    walls.close()


# ---- 7. wall exchange over slabs ---------------------------------------------------------------------------------------------
@FLUIDS
def test_slabs_fill_one_global_table_to_the_bits_of_one_block(lib, oracle, buoyant):
    """an emulated chain of 16 + 20 + 12 rows x 64 with the 68-node body across both seams (KBC part steps:
    lbm_ade_stream_collide_part_m passive, lbm_ade_slab_stream_collide_mb buoyant): per slab lbm_ade_wallx_rows_m with the
    slab's view into ONE global row table, folded -- the bits of wall_exchange_m of one block after 1, 2 and 20 steps"""
    heights, C = (16, 20, 12), 64
    Rg = sum(heights)
    gg, prm, by = ade.geom(Rg, C, 0), params(REF), (yo.buoyancy() if buoyant else None)
    f0, g0 = start_state(oracle, Rg, C, buoyant)
    walls = body_table(lib, Rg, C, (FIXED, 0.6))
    assert walls.count() == 68
    pre, post = [ade.to_lattice(f0, gg), ade.to_lattice(g0, gg)], [ade.alloc(gg), ade.alloc(gg)]
    ade_calls.collide(lib, "_mb", gg, GBC, prm, post, pre, buoy=by)
    torch.cuda.synchronize()
    assert_finite(post, gg, "post-collision state")

    def advance(s, dst, src, e):
        if buoyant:
            mb.both_parts(lib, s["g"], s["bc"], prm, dst, src, e, buoy=by, iwalls=s["view"])
        else:
            ade_calls.both_parts(lib, "_m", s["g"], s["bc"], prm, dst, src, e, iwalls=s["view"])

    ch = Chain(lib, gg, post, heights, False, GBC, advance,
               per_slab=lambda k, r0, r1, bc: dict(view=walls.slab(r0, r1 - r0).finalize()))
    assert sum(1 for s in ch.slabs if s["view"].count() > 0) == 3  # the body crosses both seams
    sv = solver(lib, Rg, C, REF, GBC, None, by, walls)
    sv.set_state(f0, g0)
    sv.step(1)
    done = 0
    for n in (1, 2, 20):
        for _ in range(n - done):
            ch.step(4)
        sv.step(n - done)
        done = n
        tab = torch.zeros(NQ * Rg, dtype=torch.float64, device=dev())
        ade.bits(tab).fill_(SENTINEL)
        for s in ch.slabs:
            f_cur, g_cur = s["lat"][ch.cur]
            wallx_rows_m(lib, tab, Rg, s["r0"], s["g"], s["bc"], prm, f_cur, g_cur, s["view"], by=by)
        out = torch.zeros(NQ, dtype=torch.float64, device=dev())
        lib.ade_wallx_fold(_ptr(out), _ptr(tab), Rg, 0, Rg, None)
        torch.cuda.synchronize()
        want, want_table = sv.wall_exchange_m(table=True)
        assert np.all(np.isfinite(want_table)) and want[pylbm.WALLX_NODES] == 68 and abs(want[pylbm.WALLX_SCALAR]) > 0.0
        assert_np_bits(tab.cpu().numpy().reshape(NQ, Rg), want_table, f"the global table after {n} steps")
        assert_np_bits(out.cpu().numpy(), want, f"the fold after {n} steps")
    sv.close()
    ch.close()
    walls.close()


# ---- 8. the existing refusals stand beside the new calls ---------------------------------------------------------------------
def test_set_open_and_wall_exchange_keep_refusing_a_kbc_context(lib, oracle):
    R, C = 16, 16
    f0, g0 = start_state(oracle, R, C, False)
    channel = aou.channel(R, C, U_IN, yo.CONC_W, 8).table(lib)
    walls = rectangle(lib, R, C, *BODY["16x16"])
    sv = solver(lib, R, C, DEFAULT, BOTTOM, walls=walls)
    sv.set_state(f0, g0)

    def refused():
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_set_open: open boundaries .* KBC fluid"):
            sv.set_open(channel)
        with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_wall_exchange: the wall exchange .* KBC fluid"):
            sv.wall_exchange()

    refused()
    sv.set_open_m(channel)
    refused()
    sv.step(3)
    refused()
    assert sv.launches() == 2 + 4 * 2  # the accepted calls alone: collide-only + carry, then interior, edge, open, walls
    x = sv.wall_exchange_m()
    assert x[pylbm.WALLX_NODES] == walls.count()
    with pytest.raises(pylbm.LbmError, match=r"-> -1: lbm_ade_solver_set_open_m: the state is post-collision"):
        sv.set_open_m(aou.channel(R, C, 0.05, 5e-4, 3).table(lib))
    sv.step(2)
    assert sv.launches() == 2 + 4 * 4
    sv.close()
    channel.close()
    walls.close()


def test_carry_row_range_and_overlap_refusals_under_the_new_names(lib, oracle):
    """what lbm_ade_collide_o / lbm_ade_stream_collide_o refuse of a table WITH nodes (a finalized one needs a device), under
    the new names with a KBC fluid and under the siblings' with model = BGK; the fluid's own check still comes first"""
    R, C = 12, 16
    g = ade.geom(R, C, 0)
    f0, g0 = start_state(oracle, R, C, False)
    src, dst = (ade.to_lattice(f0, g), ade.to_lattice(g0, g)), (ade.poisoned(g), ade.poisoned(g))
    table = aou.channel(R, C, U_IN, yo.CONC_W, 4).table(lib)
    a, b = carry_buffer(table), carry_buffer(table)
    for model, step, coll in (("kbc", "ade_open_stream_collide_m", "ade_open_collide_m"),
                              ("bgk", "ade_stream_collide_o", "ade_collide_o")):
        prm = params(REF, model)

        def refused(call, name, msg):
            with pytest.raises(pylbm.LbmError, match=msg) as e:
                call()
            assert f"-> -1: lbm_{name}:" in str(e.value), str(e.value)

        refused(lambda: open_step_m(lib, g, BOTTOM, prm, dst, src, table, None, b), step, "NULL carry with a table of 75 nodes")
        refused(lambda: open_step_m(lib, g, BOTTOM, prm, dst, src, table, a, None), step, "NULL carry")
        refused(lambda: open_step_m(lib, g, BOTTOM, prm, dst, src, table, a, a), step, "carry_in and carry_out alias")
        refused(lambda: open_collide_m(lib, g, BOTTOM, prm, dst, src, table, None), coll, "NULL carry")
        refused(lambda: open_step_m(lib, g, BOTTOM, prm, dst, src, table, a, b, rows=(0, R - 1)), step,
                r"row range \[0, 11\): the whole block \[0, 12\) only")
        refused(lambda: open_step_m(lib, ade.geom(R, C + 2, 0), BOTTOM, prm, dst, src, table, a, b), step,
                "the table is for a 12 x 16 lattice, the call for 12 x 18")
        walls = pylbm.AdeInteriorWalls(lib, R, C).add(5, C - 1, 1, 0, 2, COL_NEG, 0).finalize()
        refused(lambda: open_step_m(lib, g, BOTTOM, prm, dst, src, table, a, b, walls=walls), step,
                r"node \(5, 15\) carries an open-boundary rule and is in the interior-wall table")
        walls.close()
        walls = pylbm.AdeInteriorWalls(lib, R, C).add(1, 5, 0, 1, 1, ROW_NEG, 0).finalize()
        refused(lambda: open_step_m(lib, g, BOTTOM, prm, dst, src, table, a, b, walls=walls), step,
                r"node \(1, 5\) is in the interior-wall table and its g slot \d is redirected")
        walls.close()
        walls = pylbm.AdeInteriorWalls(lib, R, C).add(-1, 5, 0, 1, 1, 0, mask(4, 8), FIXED, 0.0).finalize()
        open_step_m(lib, g, BOTTOM, prm, dst, src, table, a, b, walls=walls)  # the foot on the bottom wall is allowed ...
        refused(lambda: open_step_m(lib, g, pylbm.Bc(), prm, dst, src, table, a, b, walls=walls), step,  # ... while it is a wall
                r"node \(11, 5\) is in the interior-wall table and its g slot 3 is redirected")
        torch.cuda.synchronize()
        walls.close()
    bad = params(REF)
    bad[0].kbc.s2 = 2.5  # two faults: the fluid's own check comes before the carry's
    with pytest.raises(pylbm.LbmError, match=r"lbm_ade_open_stream_collide_m: KBC fluid: s2=2.5 outside \(0, 2\]"):
        open_step_m(lib, g, BOTTOM, bad, dst, src, table, a, a)
    table.close()


# ---- 9. the driver ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fluid", ["kbc", "bgk"])
def test_sedimentation_channel_equals_pylbm(lib, tmp_path, fluid):
    """24 x 32, 40 steps replayed from a graph, with the rectangle and --exchange 1: the dumps and the six values (%.17g) are
    pylbm.AdeSolver's on the driver's own initial state, bit for bit"""
    R, C, steps, om, om_g, wr, wc, u_in = 24, 32, 40, 1.2, 1.6, 2e-3, 3e-3, 0.03
    r_top, c1, c2 = -7, 10, 16
    pre = tmp_path / "sed"
    r = run_driver("sedimentation_channel", R, C, steps, om, om_g, wr, wc, "--fluid", fluid, "--s2", S2, "--u-in", u_in,
                   "--conc-w", 1e-3, "--conc-rows", 12, "--rectangle", f"{r_top},{c1},{c2},1e-3", "--exchange", 1, "--dump", pre,
                   timeout=300)
    first = dict(kv.split("=", 1) for kv in r.stdout.splitlines()[0].split())
    assert first["steps"] == str(steps) and first["nonfinite"] == "0" and first["fluid"] == fluid
    assert int(first["launches"]) == 2 + 4 * (steps - 1)  # collide-only + carry; interior, edge, open pass, interior walls
    walls = rectangle(lib, R, C, r_top, c1, c2, (FIXED, 1e-3), (FIXED, 1e-3))
    channel = pylbm.AdeOpenBoundary(lib, R, C).channel(u_in, 1e-3, 12).finalize()
    assert int(first["open_nodes"]) == channel.count() and int(first["wall_nodes"]) == walls.count()
    prm = pylbm.KbcParams(S2) if fluid == "kbc" else pylbm.BgkParams(om, 0)
    sv = pylbm.AdeSolver(lib, R, C, prm, pylbm.AdeParams(om_g, (wr, wc)), bc=BOTTOM, walls=walls)
    sv.set_open_m(channel)
    f0, g0 = [np.fromfile(f"{pre}-{k}.f64").reshape(R, C, 9) for k in ("f0", "g0")]
    sv.set_state(f0, g0)
    sv.step(steps)
    want, x = sv.get_state(), sv.wall_exchange_m()
    sv.close()
    assert yo.finite(want)
    shapes = dict(f=(R, C, 9), g=(R, C, 9), rho=(R, C), u=(R, C, 2), C=(R, C))
    got = {k: np.fromfile(f"{pre}-{k}.f64").reshape(shp) for k, shp in shapes.items()}
    ade.assert_state_bits(got, want, f"driver --fluid {fluid} vs pylbm")
    out = key_values(r)
    values = [float(out[k]) for k in ("force_r", "force_c", "mass", "uptake", "uptake_fixed", "wall_nodes")]
    assert_np_bits(np.array(values), x, "the driver's exchange values")
    assert values[5] == walls.count() and values[3] != 0.0
    channel.close()
    walls.close()
