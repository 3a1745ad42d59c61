"""GPU suite, interior walls of the fluid + scalar solver (lbm_ade_iwalls: lbm_ade_stream_collide_w,
lbm_ade_solver_set_walls; pylbm.AdeInteriorWalls; passive_scalar_box --rectangle).

The yardstick of the bitwise tests is `driver_loop` below, `oracle_loop` of tests/ade_util.py with a body: the reference's
sediment loop composed from the oracle's solver:: primitives (tests/test_gpu_ade.py), with the index assignments of test/rectangle_sedimentation_test.cpp in the
driver's order -- the fluid's walls (:179-182), the rectangle on f (:184-196), calc_rho / calc_u (:198-200), the scalar's
fixed-concentration edges (:203-218), the rectangle on g (:220-232: `-g_coll` where it absorbs), the bottom wall on g
last (:233-236) -- and, for a buoyant step, the node-local buoyant collision.  The loop never
calls the library under test.  Bitwise means equal bit patterns."""
import ctypes as ct

import numpy as np
import pytest
from conftest import relerr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
import ade_calls  # noqa: E402
import ade_util as ade  # noqa: E402
from ade_util import SENTINEL, Body  # noqa: E402
from gpu_util import bits_equal, dev  # noqa: E402
from proc_util import key_values, run_driver  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
BB, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_PERIODIC
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_POS, ROW_NEG, COL_POS, COL_NEG = (pylbm.ADE_FACE_ROW_POS, pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_POS,
                                      pylbm.ADE_FACE_COL_NEG)
W = (3e-3, 3e-3)
OMEGA, OMEGA_G = 1.2, 1.7
BETA, C_REF = (2e-3, -1.5e-3), 0.4


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def rectangle_body(R, r_top, c1, c2, g_mode=FIXED, conc=0.0):
    """:186-196 and :222-232 verbatim: f's side walls are Slice(R23 + 1, -1), g's first wall Slice(R23 + 1, None)"""
    top = r_top + R
    f_side, g_first = slice(top + 1, R - 1), slice(top + 1, R)
    f_seg = [((f_side, c1), COL_NEG), ((top, slice(c1, c2 + 1)), ROW_NEG), ((f_side, c2), COL_POS)]
    g_seg = [((g_first, c1), COL_NEG), ((top, slice(c1, c2 + 1)), ROW_NEG), ((f_side, c2), COL_POS)]
    return Body(f_seg, g_seg, g_mode, conc)


def rectangle_table(lib, R, C, r_top, c1, c2, g_mode=FIXED, conc=0.0):
    """the same rectangle as three walls of the table (four add calls: g's foot on the bottom row names slots 4 and 8
    only -- the driver's bottom wall, applied last, owns slot 7 there)"""
    t = pylbm.AdeInteriorWalls(lib, R, C)
    n_side = (R - 1) - (r_top + R + 1)
    t.add(r_top + 1, c1, 1, 0, n_side, COL_NEG, COL_NEG, g_mode, conc)
    t.add(-1, c1, 1, 0, 1, 0, COL_NEG & ~(1 << 6), g_mode, conc)
    t.add(r_top, c1, 0, 1, c2 - c1 + 1, ROW_NEG, ROW_NEG, g_mode, conc)
    t.add(r_top + 1, c2, 1, 0, n_side, COL_POS, COL_POS, g_mode, conc)
    return t.finalize()


def driver_loop(orc, f, g, n, bc, fixed, body, w=W, by=None):
    return ade.oracle_loop(orc, f, g, OMEGA, OMEGA_G, w, n, bc, fixed, body, by)


def solver(lib, R, C, form=REF, bc=None, sbc=None, by=None, table=None, stream=None, w=W):
    return pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(OMEGA, 0, form=form), pylbm.AdeParams(OMEGA_G, w, form=form), bc=bc,
                           stream=stream, scalar_bc=sbc, buoyancy=by, walls=table)


def run(lib, f0, g0, steps, **kw):
    sv = solver(lib, f0.shape[0], f0.shape[1], **kw)
    sv.set_state(f0, g0)
    sv.step(steps)
    out, launches = sv.get_state(), sv.launches()
    sv.close()
    return out, launches


RECT = (24, 32, -7, 10, 16)
ROWS_BB = pylbm.Bc(row_lo=BB, row_hi=BB)


# ---- 1. the reference loop, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("buoyancy", [None, ade.REFERENCE, ade.GUO], ids=["passive", "buoyant_reference", "buoyant_guo"])
@pytest.mark.parametrize("fixed_row_lo", [False, True], ids=["no_flux_rows", "fixed_row_lo"])
@pytest.mark.parametrize("rule", [(FIXED, 0.0), (FIXED, 1e-3), (NO_FLUX, 0.0)], ids=["absorbing", "fixed_1e-3", "no_flux"])
def test_the_rectangle_is_the_drivers_loop_bit_for_bit(lib, oracle, rule, fixed_row_lo, buoyancy):
    R, C, r_top, c1, c2 = RECT
    by = ade.buoyancy(BETA, C_REF, buoyancy) if buoyancy else None
    sbc, fixed = ade.build_sbc({"row_lo": 7e-4}, R, C) if fixed_row_lo else (None, {})
    f0, g0 = ade.buoyant_initial_state(oracle, R, C, seed=9) if by else ade.initial_state(oracle, R, C, seed=9)
    table = rectangle_table(lib, R, C, r_top, c1, c2, *rule)
    body = rectangle_body(R, r_top, c1, c2, *rule)
    sv = solver(lib, R, C, REF, ROWS_BB, sbc, by, table)
    sv.set_state(f0, g0)
    done, want = 0, dict(f=f0, g=g0)
    for n in (1, 2, 5):
        sv.step(n - done)
        want = driver_loop(oracle, want["f"], want["g"], n - done, ROWS_BB, fixed, body, by=by)
        done = n
        ade.assert_state_bits(sv.get_state(), want, f"rectangle {rule} after {n} iterations")
    assert sv.launches() == 1 + 4 * 3  # collide-only, then interior + edge pass + wall pass
    sv.close()
    # the body is felt: without it the loop holds other bits
    plain = driver_loop(oracle, f0, g0, 5, ROWS_BB, fixed, Body([], []), by=by)
    assert not bits_equal(plain["f"], want["f"]) and not bits_equal(plain["g"], want["g"])
    table.close()


@pytest.mark.parametrize("form_of_context", [REF, pylbm.FORM_DEFAULT])
def test_one_node_and_a_wall_row_through_columns_0_and_C_minus_1_of_a_periodic_box(lib, oracle, form_of_context):
    """30 x 42, fully periodic: a table of ONE node, then a full-width wall row (its end nodes gather across the
    periodic seam) with a FIXED scalar and one more node beside it; reference order bitwise (a buoyant step runs the
    reference order whatever the form of the context)"""
    R, C = 30, 42
    by = ade.buoyancy(BETA, C_REF, ade.REFERENCE) if form_of_context != REF else None
    f0, g0 = ade.buoyant_initial_state(oracle, R, C, seed=2) if by else ade.initial_state(oracle, R, C, seed=2)
    one = pylbm.AdeInteriorWalls(lib, R, C).add(5, 7, 0, 1, 1, ROW_POS, ROW_POS).finalize()
    assert one.count() == 1
    row = pylbm.AdeInteriorWalls(lib, R, C).add(12, 0, 0, 1, C, ROW_NEG, ROW_NEG, FIXED, 2e-3)
    row.add(20, -1, 0, -1, 1, COL_NEG, 0).finalize()
    bodies = {one: Body([((5, 7), ROW_POS)], [((5, 7), ROW_POS)], NO_FLUX),
              row: Body([((12, slice(None)), ROW_NEG), ((20, C - 1), COL_NEG)], [((12, slice(None)), ROW_NEG)], FIXED, 2e-3)}
    for table, body in bodies.items():
        got, launches = run(lib, f0, g0, 7, form=form_of_context, by=by, table=table)
        want = driver_loop(oracle, f0, g0, 7, pylbm.Bc(), {}, body, by=by)
        ade.assert_state_bits(got, want, f"{table.count()} nodes")
        assert launches == 1 + 6 * 2
        table.close()


# ---- 2. interior walls on the rim are the domain's walls ----------------------------------------------------------------
def rim_table(lib, R, C, axis, g_mode, conc):
    t = pylbm.AdeInteriorWalls(lib, R, C)
    if axis == "rows":
        t.add(0, 0, 0, 1, C, ROW_POS, ROW_POS, g_mode, conc)
        t.add(-1, 0, 0, 1, C, ROW_NEG, ROW_NEG, g_mode, conc)
    else:
        t.add(0, 0, 1, 0, R, COL_POS, COL_POS, g_mode, conc)
        t.add(0, -1, 1, 0, R, COL_NEG, COL_NEG, g_mode, conc)
    return t.finalize()


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
@pytest.mark.parametrize("case", ["no_flux", "fixed", "buoyant_fixed"])
@pytest.mark.parametrize("R,C,axis", [(24, 32, "rows"), (30, 42, "rows"), (8, 260, "rows"), (30, 42, "cols"), (260, 8, "cols")])
def test_interior_walls_on_the_rim_are_the_domains_walls(lib, oracle, R, C, axis, case, form):
    """a fully periodic box with the facing walls along its two rim rows (columns) == the solver with BOUNCE_BACK rows
    (columns) and the matching lbm_ade_scalar_bc, bit for bit after 20 steps, in both forms; 8 x 260 / 260 x 8: 520 table
    nodes, three workgroups of the pass"""
    conc = 1.5e-3
    by = ade.buoyancy(BETA, C_REF, ade.GUO) if case == "buoyant_fixed" else None
    f0, g0 = ade.buoyant_initial_state(oracle, R, C, seed=R) if by else ade.initial_state(oracle, R, C, seed=R)
    lo, hi = ("row_lo", "row_hi") if axis == "rows" else ("col_lo", "col_hi")
    bc = pylbm.Bc(**{lo: BB, hi: BB})
    sbc = pylbm.AdeScalarBC(**{lo: conc, hi: conc}) if case != "no_flux" else None
    table = rim_table(lib, R, C, axis, NO_FLUX if case == "no_flux" else FIXED, conc)
    assert table.count() == 2 * (C if axis == "rows" else R)
    want, base = run(lib, f0, g0, 20, form=form, bc=bc, sbc=sbc, by=by)
    got, launches = run(lib, f0, g0, 20, form=form, by=by, table=table)
    ade.assert_state_bits(got, want, f"{R}x{C} {axis} {case}")
    assert launches == base == 1 + 19 * 2  # the wall pass where the other solver has its edge pass
    periodic, _ = run(lib, f0, g0, 20, form=form, by=by)
    assert not bits_equal(periodic["g"], got["g"])
    table.close()


# ---- 3. a sealed wall seals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_a_sealed_wall_seals(lib, oracle, form):
    """rows BOUNCE_BACK, fluid at rest, w = 0, a full-width pair (row k ROW_NEG, row k + 1 ROW_POS, NO_FLUX); the scalar
    starts above the pair only: after 200 steps C below it is exactly 0.0 at every node -- and is not without the table.
    The mass above is conserved to rounding; its bound, fixed before measuring: 200 steps x about 20 roundings per
    population and step x 2^-53 = 4.4e-13 if every rounding erred the same way, so 1e-12 relative"""
    R, C, k = 24, 32, 11
    u = np.zeros((R, C, 2))
    f0 = oracle.equilibrium(u, np.ones((R, C)))
    conc = np.zeros((R, C))
    conc[:k + 1] = 1e-3 * (1.0 + 0.5 * np.cos(2 * np.pi * np.arange(C) / C))[None, :]
    g0 = oracle.equilibrium(u, conc)
    table = pylbm.AdeInteriorWalls(lib, R, C).add(k, 0, 0, 1, C, ROW_NEG, ROW_NEG).add(k + 1, 0, 0, 1, C, ROW_POS, ROW_POS)
    table.finalize()
    sealed, _ = run(lib, f0, g0, 200, form=form, bc=ROWS_BB, table=table, w=(0.0, 0.0))
    open_, _ = run(lib, f0, g0, 200, form=form, bc=ROWS_BB, w=(0.0, 0.0))
    assert np.all(sealed["C"][k + 1:] == 0.0) and np.all(sealed["g"][k + 1:] == 0.0)
    assert np.all(sealed["C"][:k + 1] > 0.0)
    assert np.all(open_["C"][k + 1:k + 4] > 0.0)
    # what was above the pair stays there: the scalar mass is conserved to rounding
    assert abs(sealed["C"].sum() - conc.sum()) <= 1e-12 * conc.sum()
    table.close()


# ---- 4. NULL or empty table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_null_and_empty_tables_are_todays_solver(lib, oracle, form):
    R, C = 24, 32
    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=pylbm.EDGE_SPECULAR)
    sbc = pylbm.AdeScalarBC(row_lo=1e-3, col_hi=0.0)
    f0, g0 = ade.initial_state(oracle, R, C, seed=4)
    empty = pylbm.AdeInteriorWalls(lib, R, C).finalize()
    box = pylbm.AdeInteriorWalls(lib, R, C).add_box(8, 12, 10, 20, FIXED, 0.0).finalize()
    plain, base = run(lib, f0, g0, 21, form=form, bc=bc, sbc=sbc)
    assert base == 1 + 20 * 2
    got, launches = run(lib, f0, g0, 21, form=form, bc=bc, sbc=sbc, table=empty)
    ade.assert_state_bits(got, plain, "empty table")
    assert launches == base
    sv = solver(lib, R, C, form, bc, sbc, table=box)
    sv.set_walls(None)  # NULL clears
    sv.set_state(f0, g0)
    sv.step(21)
    ade.assert_state_bits(sv.get_state(), plain, "cleared table")
    assert sv.launches() == base
    sv.set_walls(box)   # from the next stream on
    sv.step(4)
    assert sv.launches() == base + 4 * 3
    assert not bits_equal(sv.get_state()["g"], plain["g"])
    sv.close()
    got, launches = run(lib, f0, g0, 21, form=form, bc=bc, sbc=sbc, table=box)
    assert launches == base + 20  # one more launch per streamed step
    assert not bits_equal(got["f"], plain["f"]) and not bits_equal(got["g"], plain["g"])
    # the raw entry point with NULL and with the empty table is lbm_ade_stream_collide_b
    g = ade.geom(R, C, 0, C + 6)
    prm = ade.params(form)
    src = (ade.random_lattice(g, 1), ade.random_lattice(g, 2))
    outs = []
    for t in ("b", None, empty):
        if t == "b":
            outs.append(ade_calls.full_step(lib, "_b", g, bc, prm, *src, sbc=sbc))
        else:
            outs.append(ade_calls.full_step(lib, "_w", g, bc, prm, *src, sbc=sbc, iwalls=t))
        torch.cuda.synchronize()
    for k in range(2):
        ade.assert_bits(outs[1][k], outs[0][k], f"NULL table, lattice {k}")
        ade.assert_bits(outs[2][k], outs[0][k], f"empty table, lattice {k}")
    empty.close()
    box.close()


# ---- 5. write set -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
@pytest.mark.parametrize("lo,hi", [(3, 7), (0, 8), (0, 2), (2, 3), (6, 8), (5, 6)],
                         ids=["rows_3_7", "whole_block", "before_the_table", "table_row_2", "after_the_table", "table_row_5"])
def test_the_walled_step_writes_exactly_the_rows_of_its_range(lib, form, lo, hi):
    """8 x 260 at a padded row pitch, two full-width wall rows (520 nodes, rows 2 and 5: an index range of the table
    crosses a 256-lane workgroup): lbm_ade_stream_collide_w on rows [lo, hi) -- the table's nodes of those rows taken from
    its row index -- writes those rows only, the table's rows outside keep the pattern, never the padding, and what it
    writes is what the call on [0, R) writes there; the moment outputs likewise.  A range without a table row writes
    lbm_ade_stream_collide_b's bits: nothing of the table is applied"""
    R, C = 8, 260
    g = ade.geom(R, C, 0, C + 12)
    bc = pylbm.Bc(col_lo=BB, col_hi=BB)
    sbc = pylbm.AdeScalarBC(col_lo=5e-4)
    prm = ade.params(form)
    table = pylbm.AdeInteriorWalls(lib, R, C).add(2, 0, 0, 1, C, ROW_NEG, ROW_NEG, FIXED, 1e-3)
    table.add(5, 0, 0, 1, C, ROW_POS, ROW_POS, FIXED, 1e-3).finalize()
    assert table.count() == 520
    src = (ade.random_lattice(g, 5), ade.random_lattice(g, 6))

    def call(a, b):
        out = [ade.alloc(g), ade.alloc(g)] + [torch.zeros(n * R * C, dtype=torch.float64, device=dev()) for n in (1, 2, 1)]
        for t in out:
            ade.bits(t).fill_(SENTINEL)
        torch.cuda.synchronize()
        ade_calls.step_into(lib, "_w", g, bc, prm, out[:2], src, (a, b), sbc=sbc, iwalls=table, moments=out[2:])
        torch.cuda.synchronize()
        return out

    full, part = call(0, R), call(lo, hi)
    expect = torch.zeros(9 * g.plane_stride, dtype=torch.bool, device=dev())
    ade.owned(expect, g)[:, lo:hi] = True
    for k in range(2):
        changed = ade.bits(part[k]) != SENTINEL
        assert torch.nonzero(changed != expect).numel() == 0, f"lattice {k}: the write set is not rows [{lo}, {hi})"
        assert torch.nonzero(expect & (ade.bits(part[k]) != ade.bits(full[k]))).numel() == 0, f"lattice {k}: other bits"
        everything = torch.zeros_like(expect)
        ade.owned(everything, g)[:] = True
        assert torch.nonzero((ade.bits(full[k]) != SENTINEL) != everything).numel() == 0, f"lattice {k}: padding written"
    for k, comps in ((2, 1), (3, 2), (4, 1)):
        m, mf = ade.bits(part[k]).view(comps, R, C), ade.bits(full[k]).view(comps, R, C)
        assert bool((m[:, lo:hi] == mf[:, lo:hi]).all()) and bool((mf != SENTINEL).all())
        assert bool((m[:, :lo] == SENTINEL).all()) and bool((m[:, hi:] == SENTINEL).all())
    # the wall rows are the table's, not the plain step's
    plain = ade_calls.full_step(lib, "_b", g, bc, prm, *src, sbc=sbc)
    torch.cuda.synchronize()
    for k in range(2):
        differs = (ade.bits(ade.owned(full[k], g)) != ade.bits(ade.owned(plain[k], g))).any(dim=0).any(dim=1)
        assert differs.tolist() == [r in (2, 5) for r in range(R)], (k, differs.tolist())
        if not any(lo <= r < hi for r in (2, 5)):
            same = ade.bits(ade.owned(part[k], g))[:, lo:hi] == ade.bits(ade.owned(plain[k], g))[:, lo:hi]
            assert bool(same.all()), f"lattice {k}: rows [{lo}, {hi}) are not the plain step's"
    table.close()


# ---- 6. reassociated form -----------------------------------------------------------------------------------------------
def test_reassociated_form_agrees_with_the_reference_order_on_the_rectangle(lib, oracle):
    """the project's bound and step count (tests/test_gpu_ade_scalar_bc.py,
    test_reassociated_form_agrees_with_the_reference_order): 500 iterations, 1e-10 relative to each field's largest
    magnitude"""
    R, C, r_top, c1, c2 = RECT
    f0, g0 = ade.initial_state(oracle, R, C, seed=11)
    sbc = pylbm.AdeScalarBC(row_lo=7e-4)
    table = rectangle_table(lib, R, C, r_top, c1, c2, FIXED, 1e-3)
    out = {form: run(lib, f0, g0, 500, form=form, bc=ROWS_BB, sbc=sbc, table=table)[0] for form in (REF, FAST)}
    errs = {k: relerr(out[FAST][k], out[REF][k]) for k in ("f", "g", "rho", "u", "C")}
    print("reassociated vs reference order, rectangle, after 500 steps:", errs)
    assert max(errs.values()) <= 1e-10, errs
    assert not bits_equal(out[FAST]["g"], out[REF]["g"])
    table.close()


# ---- 7. capture ---------------------------------------------------------------------------------------------------------
def test_a_captured_graph_with_a_table_replays_the_eager_run(lib, oracle):
    R, C, r_top, c1, c2 = RECT
    f0, g0 = ade.initial_state(oracle, R, C, seed=17)
    table = rectangle_table(lib, R, C, r_top, c1, c2)
    want1, _ = run(lib, f0, g0, 11, form=pylbm.FORM_DEFAULT, bc=ROWS_BB, table=table)
    want2, _ = run(lib, f0, g0, 21, form=pylbm.FORM_DEFAULT, bc=ROWS_BB, table=table)
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        sv = solver(lib, R, C, pylbm.FORM_DEFAULT, ROWS_BB, table=table, stream=st.value)
        sv.set_state(f0, g0)
        sv.step(1)
        sv.sync()
        lib.graph_begin_capture(st)
        sv.step(10)
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


# ---- 8. the driver ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conc", [None, 1e-3], ids=["absorbing", "held_at_1e-3"])
def test_passive_scalar_box_driver_with_the_rectangle_equals_pylbm(lib, tmp_path, conc):
    R, C, r_top, c1, c2 = RECT
    steps, om, om_g, wr, wc = 40, 1.1, 1.6, 2e-3, 3e-3
    pre = tmp_path / "psb"
    rect = f"{r_top},{c1},{c2}" + (f",{conc}" if conc is not None else "")
    r = run_driver("passive_scalar_box", R, C, steps, om, om_g, wr, wc, "--dump", pre, "--walls", 2, "--rectangle", rect,
                   timeout=300)

    def load(k, shape):
        return np.fromfile(f"{pre}-{k}.f64").reshape(shape)

    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=BB)
    table = rectangle_table(lib, R, C, r_top, c1, c2, FIXED, conc or 0.0)
    sv = pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(om, 0), pylbm.AdeParams(om_g, (wr, wc)), bc=bc, walls=table)
    sv.set_state(load("f0", (R, C, 9)), load("g0", (R, C, 9)))
    sv.step(steps)
    got = sv.get_state()
    sv.close()
    want = dict(f=load("f", (R, C, 9)), g=load("g", (R, C, 9)), rho=load("rho", (R, C)), u=load("u", (R, C, 2)),
                C=load("C", (R, C)))
    ade.assert_state_bits(got, want, "driver vs pylbm")
    out = key_values(r)
    assert int(out["launches"]) == 1 + (steps - 1) * 3
    assert float(out["mass_C"]) != float(out["mass_C0"])  # the body exchanges scalar with the box
    table.close()
