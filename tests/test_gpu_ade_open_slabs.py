"""GPU suite, open boundaries of the fluid + scalar step over row slabs and the ring: lbm_ade_open_slab (the slab view of an
open table), lbm_ade_stream_collide_part_o (k_ade_open_ranges behind each part's dispatch), lbm_ring_ade_collide_o,
lbm_ring_ade_step_o and slab_ring_ade --channel.

The yardstick is one block in the SAME form: lbm_ade_collide_o / lbm_ade_stream_collide_o on the global lattice with the
global table (pinned to the oracle in tests/test_gpu_ade_open.py).  Every comparison is of bit patterns, so there are no
tolerances.  Each test asserts that every band it exercises holds a listed node (bands_hold_nodes): an inlet or outlet
column puts one into every row.  The chain of slabs, the carry helpers and the write-set check of a part are
tests/ade_slab_util.py's; every raw call goes through tests/ade_calls.py."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
from ade_open_util import build_open  # noqa: E402
import ade_calls  # noqa: E402
from ade_slab_util import (Chain, OneSlabRing, assert_part_write_sets, bands_hold_nodes, carry_like, first_index,  # noqa: E402
                           global_state, slab_bc)
from ade_util import (GUO, REFERENCE, SENTINEL, W, alloc, assert_bits, bits, buoyancy, cut_slab, geom, moment_fields,  # noqa: E402
                      owned, params, poisoned, random_lattice)
from gpu_util import dev  # noqa: E402
from proc_util import last_json, run_driver, run_ranks  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FORMS = pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
BB, SP, HALO, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO, pylbm.EDGE_PERIODIC
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
O_BB, O_SROW, O_SCOL, O_ABB, O_ABBX = (pylbm.ADE_OPEN_BOUNCE_BACK, pylbm.ADE_OPEN_SPECULAR_ROW, pylbm.ADE_OPEN_SPECULAR_COL,
                                       pylbm.ADE_OPEN_ABB, pylbm.ADE_OPEN_ABB_EXTRAPOLATED)
ALL = 0xFF
RG, CG = 48, 64
VIEWS = ((0, 24), (24, 48), (12, 36))
WALLS = pylbm.Bc(row_lo=BB, row_hi=BB)  # the chain's global edges: wall rows at both ends, periodic columns
LBM_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


# ---- tables and calls ----------------------------------------------------------------------------------------------------
def columns(lib, R, C, copies=False):
    """inlet ABB + FIXED scalar on column 0, extrapolated outlet on column C-1, all rows; copies: the outlet's zero-gradient
    copy as well"""
    t = pylbm.AdeOpenBoundary(lib, R, C)
    t.add_f(0, 0, 1, 0, R, ALL, O_ABB, (2e-3, 0.03))
    t.add_f(0, C - 1, 1, 0, R, ALL, O_ABBX, (1.5, -0.5), (0, -1))
    t.add_g(0, 0, 1, 0, R, ALL, FIXED, 1e-3)
    if copies:
        t.add_g_copy(0, C - 1, 1, 0, R, (0, -1))
    return t


def seam_copies(lib, R, C):
    """columns + copies that read one row across the seams of VIEWS: downwards (row <- row - 1) at rows 12 and 24,
    upwards (row <- row + 1) at rows 23 and 35, on columns of their own"""
    t = columns(lib, R, C)
    for r in (12, 24):
        t.add_g_copy(r, 5, 0, 1, 20, (-1, 0))
    for r in (23, 35):
        t.add_g_copy(r, 30, 0, 1, 20, (1, 0))
    return t


def specular(lib, R, C):
    t = pylbm.AdeOpenBoundary(lib, R, C)
    t.add_f(0, 0, 0, 1, C, 0x91, O_SROW).add_f(R - 1, 0, 0, 1, C, 0x64, O_SROW)
    return t.add_f(0, 0, 1, 0, R, 0x32, O_SCOL)


def channel(lib, R, C):
    return build_open(lib, "channel", R, C)


def rectangle(lib, R, C, r_top, c1, c2):
    """the driver's rectangle standing on the bottom wall, absorbing (tests/test_gpu_ade_open.py rectangle_table)"""
    neg, pos, rneg = pylbm.ADE_FACE_COL_NEG, pylbm.ADE_FACE_COL_POS, pylbm.ADE_FACE_ROW_NEG
    t = pylbm.AdeInteriorWalls(lib, R, C)
    n_side = (R - 1) - (r_top + 1)
    t.add(r_top + 1, c1, 1, 0, n_side, neg, neg, FIXED, -0.0)
    t.add(r_top + 1, c2, 1, 0, n_side, pos, pos, FIXED, -0.0)
    t.add(R - 1, c1, 1, 0, 1, 0, neg & ~(1 << 6), FIXED, -0.0)  # g's foot: the allowed overlap with the open table
    t.add(r_top, c1, 0, 1, c2 - c1 + 1, rneg, rneg, FIXED, -0.0)
    return t


def block_o(lib, g, bc, prm, src, table, cin, **kw):
    """the yardstick: lbm_ade_stream_collide_o on one block -> (fn, gn, carry_out)"""
    cout = carry_like(table)
    fn, gn = ade_calls.full_step(lib, "_o", g, bc, prm, *src, open=table, carry_in=cin, carry_out=cout, **kw)
    return fn, gn, cout


def part_o(lib, g, bc, prm, dst, src, which, E, view, cin, cout, **kw):
    ade_calls.part(lib, "_o", g, bc, prm, dst, src, which, E, view=view, carry_in=cin, carry_out=cout, **kw)


# ---- 1. FRAME + INNER with a view == the one-block step on the global lattice --------------------------------------------
CASES = {
    "channel": dict(table=channel),
    "inlet_outlet": dict(table=columns),
    "copy_across_the_seams": dict(table=seam_copies),
    "specular_rows_and_column": dict(table=specular),
    "fixed_domain_row": dict(table=lambda lib, R, C: columns(lib, R, C, copies=True), sbc=True),
    "buoyant_reference": dict(table=channel, by=REFERENCE),
    "buoyant_guo": dict(table=channel, by=GUO),
    "rectangle": dict(table=channel, walls=True),
}


@FORMS
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("C,pitch", [(CG, 0), (1040, 1056)], ids=["48x64", "48x1040_padded"])
def test_frame_plus_inner_with_a_view_is_the_one_block_step(lib, form, case, C, pitch):
    spec = CASES[case]
    prm = params(form)
    by = buoyancy((2e-2, -1e-2), 1.0, spec["by"]) if "by" in spec else None  # random_lattice: C ~ 1.0 .. 1.05
    gsbc = pylbm.AdeScalarBC(row_lo=1.02) if spec.get("sbc") else None
    gg = geom(RG, C, 0, pitch)
    src = (random_lattice(gg, 21 + C), random_lattice(gg, 22 + C))
    table = spec["table"](lib, RG, C)
    twin = spec["table"](lib, RG, C)  # never finalized
    table.finalize()
    walls = rectangle(lib, RG, C, 30, C // 2 - 3, C // 2 + 3).finalize() if spec.get("walls") else None
    cin = carry_like(table, seed=5)
    mw = moment_fields(gg)
    want = block_o(lib, gg, WALLS, prm, src, table, cin, sbc=gsbc, buoy=by, iwalls=walls, moments=mw)
    plain = block_o(lib, gg, WALLS, prm, src, None, None, sbc=gsbc, buoy=by, iwalls=walls)
    assert not torch.equal(bits(want[0]), bits(plain[0])) or not torch.equal(bits(want[1]), bits(plain[1]))  # the table is felt
    for r0, r1 in VIEWS:
        R = r1 - r0
        view, other = table.slab(r0, R), twin.slab(r0, R)
        assert view.count() > 0 and view.nodes() == other.nodes()  # a finalized parent gives the unfinalized one's view
        other.close()
        view.finalize()
        i0 = first_index(table, r0)
        wview = walls.slab(r0, R).finalize() if walls is not None else None
        if case == "rectangle" and r0 > 0:
            assert wview.count() > 0
        bc = slab_bc(WALLS, r0, r1, RG)
        sbc = gsbc if r0 == 0 else None  # a FIXED row acts where the slab keeps that edge
        slab = [cut_slab(s, gg, r0, r1, pitch) for s in src]
        sg = slab[0][0]
        vin = cin[2 * i0:2 * (i0 + view.count())].clone()
        for E in (1, 3, 8):
            assert bands_hold_nodes(view, E)
            dst, cout, mp = (alloc(sg), alloc(sg)), carry_like(view), moment_fields(sg)
            for which in (FRAME, INNER):
                part_o(lib, sg, bc, prm, dst, (slab[0][1], slab[1][1]), which, E, view, vin, cout, sbc=sbc, buoy=by, iwalls=wview,
                       moments=mp)
            torch.cuda.synchronize()
            what = f"{case} C={C} slab [{r0}, {r1}) E={E}"
            for k in range(2):
                assert_bits(owned(dst[k], sg), owned(want[k], gg)[:, r0:r1], f"{what} lattice {k}")
            assert_bits(cout, want[2][2 * i0:2 * (i0 + view.count())], f"{what} carry")
            assert_bits(mp[0].view(R, C), mw[0].view(RG, C)[r0:r1], f"{what} rho")
            assert_bits(mp[1].view(2, R, C), mw[1].view(2, RG, C)[:, r0:r1], f"{what} u")
            assert_bits(mp[2].view(R, C), mw[2].view(RG, C)[r0:r1], f"{what} C")
        view.close()
        if wview is not None:
            wview.close()
    for t in (twin, table, walls):
        if t is not None:
            t.close()


# ---- emulated chains and rings in one process ----------------------------------------------------------------------------
def one_block(lib, gg, pre, gbc, prm, steps, table, walls=None, by=None):
    """lbm_ade_collide_o + steps x lbm_ade_stream_collide_o on the global lattice: the post-collision state and its carry,
    and the (lattices, carry) after each number of steps in `steps`"""
    post, c0 = [alloc(gg), alloc(gg)], carry_like(table)
    ade_calls.collide(lib, "_o", gg, gbc, prm, post, pre, buoy=by, open=table, carry_out=c0)
    cur, carry, out = post, c0, {}
    for k in range(1, max(steps) + 1):
        fn, gn, carry = block_o(lib, gg, gbc, prm, cur, table, carry, buoy=by, iwalls=walls)
        cur = [fn, gn]
        if k in steps:
            out[k] = (cur, carry)
    torch.cuda.synchronize()
    return post, c0, out


def chain(lib, gg, post, carry0, heights, closed, gbc, prm, table, walls=None, by=None):
    """ade_slab_util.Chain through lbm_ade_stream_collide_part_o, every slab with its views and its two carries (the part
    of carry0 of its nodes, and a poisoned one).  The carry never travels."""
    def per_slab(k, a, b, bc):
        view, i0 = table.slab(a, b - a).finalize(), first_index(table, a)
        return dict(view=view, walls=walls.slab(a, b - a).finalize() if walls is not None else None,
                    carry=[carry0[2 * i0:2 * (i0 + view.count())].clone(), carry_like(view)])

    def advance(s, dst, src, e):
        for which in (FRAME, INNER):
            part_o(lib, s["g"], s["bc"], prm, dst, src, which, e, s["view"], s["carry"][s["cur"]], s["carry"][s["cur"] ^ 1],
                   buoy=by, iwalls=s["walls"])

    return Chain(lib, gg, post, heights, closed, gbc, advance, per_slab=per_slab)


def chain_carry(ch):
    return torch.cat([s["carry"][ch.cur] for s in ch.slabs])


def check_chain(ch, gg, want, what):
    torch.cuda.synchronize()
    (lat, carry) = want
    for j in range(2):
        assert_bits(ch.gather(j), owned(lat[j], gg), f"{what} lattice {j}")
    assert_bits(chain_carry(ch), carry, f"{what} carry")


CHAINS = {
    "channel_chain": dict(table=channel, closed=False),
    "channel_rectangle_chain": dict(table=channel, closed=False, walls=True),
    "columns_ring": dict(table=lambda lib, R, C: columns(lib, R, C, copies=True), closed=True),
}


@FORMS
@pytest.mark.parametrize("case", list(CHAINS))
@pytest.mark.parametrize("heights", [(24, 24), (16, 20, 12)])
def test_emulated_chains_and_rings_equal_one_block_after_1_2_and_20_steps(lib, oracle, form, case, heights):
    """on the closed ring (a periodic box) both columns also cross the wrap-around seam; the rectangle (rows 14 .. 47)
    crosses every seam of both splits"""
    spec = CHAINS[case]
    prm, gbc = params(form), (pylbm.Bc.periodic() if spec["closed"] else WALLS)
    E = 4
    gg, pre = global_state(oracle, RG, CG)
    table = spec["table"](lib, RG, CG).finalize()
    walls = rectangle(lib, RG, CG, 14, 28, 36).finalize() if spec.get("walls") else None
    post, c0, want = one_block(lib, gg, pre, gbc, prm, (1, 2, 20), table, walls)
    _, _, plain = one_block(lib, gg, pre, gbc, prm, (20,), None, walls)
    assert not torch.equal(bits(want[20][0][0]), bits(plain[20][0][0]))
    ch = chain(lib, gg, post, c0, heights, spec["closed"], gbc, prm, table, walls)
    assert all(bands_hold_nodes(s["view"], min(E, (s["g"].R - 1) // 2)) for s in ch.slabs)
    if walls is not None:
        assert all(s["walls"].count() > 0 for s in ch.slabs[1:])
    for k in range(1, 21):
        ch.step(E)
        if k in want:
            check_chain(ch, gg, want[k], f"{case} {heights} after {k} steps")
    ch.close()
    for t in (table, walls):
        if t is not None:
            t.close()


# ---- 2. the smallest shapes ----------------------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("shape", ["12x8_chain_of_four", "6x4_ring_of_two"])
def test_the_smallest_shapes(lib, oracle, form, shape):
    """12 x 8 in four slabs of 3 rows (E = 1: FRAME is rows 0 and 2, INNER row 1); 6 x 4 in two slabs of 3 rows on a closed
    ring, whose wrap-around seam both column segments cross"""
    if shape == "12x8_chain_of_four":
        Rg, C, heights, closed, gbc, make = 12, 8, (3, 3, 3, 3), False, WALLS, channel
    else:
        Rg, C, heights, closed, gbc, make = 6, 4, (3, 3), True, pylbm.Bc.periodic(), lambda lib, R, C: columns(lib, R, C, copies=True)
    prm = params(form)
    gg, pre = global_state(oracle, Rg, C, seed=4)
    table = make(lib, Rg, C).finalize()
    post, c0, want = one_block(lib, gg, pre, gbc, prm, (1, 2, 7), table)
    ch = chain(lib, gg, post, c0, heights, closed, gbc, prm, table)
    assert all(bands_hold_nodes(s["view"], 1) for s in ch.slabs)
    for k in range(1, 8):
        ch.step(1)
        if k in want:
            check_chain(ch, gg, want[k], f"{shape} after {k} steps")
    ch.close()
    table.close()


# ---- 3. NULL and empty view == _part_w, and the launches -----------------------------------------------------------------
@FORMS
def test_null_and_empty_views_are_part_w_and_a_view_costs_one_launch_a_part(lib, form):
    R, C, E = 24, CG, 3
    prm = params(form)
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO, col_lo=BB, col_hi=SP)
    sbc, by = pylbm.AdeScalarBC(row_lo=1.02, col_hi=0.0), buoyancy((2e-2, -1e-2), 1.0, GUO)
    g = geom(R, C, 1, C + 6)
    src = (random_lattice(g, 1), random_lattice(g, 2))
    empty = pylbm.AdeOpenBoundary(lib, 48, C).finalize().slab(0, R).finalize()
    none_here = pylbm.AdeOpenBoundary(lib, 48, C).add_f(40, 3, 0, 1, 5, ALL, O_BB).slab(0, R).finalize()  # no node in its rows
    real = columns(lib, 48, C).slab(0, R).finalize()
    assert empty.count() == none_here.count() == 0 and bands_hold_nodes(real, E)
    count = lib.raw.lbm_ade_part_launches
    for drive in (None, by):
        outs, launches = [], []
        for t in ("w", None, empty, none_here, real):
            dst = (poisoned(g), poisoned(g))
            cout = carry_like(real)
            before = count()
            for which in (FRAME, INNER):
                if t == "w":
                    ade_calls.part(lib, "_w", g, bc, prm, dst, src, which, E, sbc=sbc, buoy=drive)
                elif t is real:
                    part_o(lib, g, bc, prm, dst, src, which, E, t, carry_like(real, 3), cout, sbc=sbc, buoy=drive)
                else:
                    part_o(lib, g, bc, prm, dst, src, which, E, t, None, None, sbc=sbc, buoy=drive)  # no carry needed
            torch.cuda.synchronize()
            outs.append(dst)
            launches.append(count() - before)
        for i, what in ((1, "NULL"), (2, "empty"), (3, "view without a node")):
            for k in range(2):
                assert_bits(outs[i][k], outs[0][k], f"{what} view, lattice {k}")  # the whole allocation, padding included
        assert launches == [2, 2, 2, 2, 4], launches  # one dispatch per part; with listed nodes in both parts one pass each
        assert not torch.equal(bits(outs[4][0]), bits(outs[0][0]))
    for t in (empty, none_here, real):
        t.close()


# ---- 4. write sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,E", [(24, 64, 1), (24, 64, 8), (33, 96, 5)])
def test_each_part_alone_writes_its_rows_nodes_and_their_carry(lib, R, C, E):
    """NaN-poisoned targets, ghost rows and padding included: a part (its dispatch and its open pass) changes exactly its
    rows of both lattices and the carry entries of its rows' nodes, each to the value FRAME + INNER together give"""
    prm = params(FAST)
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO)
    g = geom(R, C, 1, C + 10)
    view = channel(lib, 2 * R, C).slab(0, R).finalize()
    assert bands_hold_nodes(view, E)
    src = (random_lattice(g, R), random_lattice(g, C))
    cin = carry_like(view, seed=1)
    want, wcarry, plain = [alloc(g), alloc(g)], carry_like(view), [alloc(g), alloc(g)]
    for which in (FRAME, INNER):
        part_o(lib, g, bc, prm, want, src, which, E, view, cin, wcarry)
        ade_calls.part(lib, "_w", g, bc, prm, plain, src, which, E)
    torch.cuda.synchronize()
    assert not (bits(wcarry) == SENTINEL).any()
    assert not torch.equal(bits(want[1]), bits(plain[1]))
    node_rows = torch.tensor([n["r"] for n in view.nodes()], device=dev()).repeat_interleave(2)
    couts = {}

    def launch(dst, which):
        couts[which] = carry_like(view)
        part_o(lib, g, bc, prm, dst, src, which, E, view, cin, couts[which])

    def carry_of_the_part(which, rows, what):
        cout, mine = couts[which], torch.isin(node_rows, torch.tensor(rows, device=dev()))
        assert torch.equal(bits(cout) != SENTINEL, mine), f"{what}: carry entries written outside its rows' nodes, or missed"
        assert torch.equal(bits(cout)[mine], bits(wcarry)[mine]), f"{what}: carry differs from the full call"

    assert_part_write_sets(launch, g, want, E, f"R={R} C={C} E={E}", also=carry_of_the_part)
    view.close()


# ---- 5. refusals at call time --------------------------------------------------------------------------------------------
def test_refusals_at_call_time_name_what_is_wrong(lib):
    R, C, E = 24, CG, 3
    prm, g = params(FAST), geom(24, CG, 1)
    src, dst = (random_lattice(g, 1), random_lattice(g, 2)), (alloc(g), alloc(g))
    name = "lbm_ade_stream_collide_part_o"

    def refused(view, bc, msg, cin="in", cout="out", walls=None):
        a = carry_like(view, 1) if cin == "in" else cin
        b = carry_like(view) if cout == "out" else (a if cout == "alias" else cout)
        rc = ade_calls.call_rc(lib, name, dst=dst, src=src, g=g, bc=bc, prm=prm, iwalls=walls, view=view, carry_in=a, carry_out=b,
                               part=FRAME, edge_rows=E)
        err = lib.raw.lbm_last_error_string().decode()
        assert rc == LBM_ERR_INVALID and err.startswith(name + ":") and msg in err, (rc, err)

    halo = pylbm.Bc(row_lo=HALO, row_hi=HALO)
    far = pylbm.AdeOpenBoundary(lib, RG, C).add_g_copy(24, 5, 0, 1, 10, (-2, 0)).slab(24, R).finalize()
    refused(far, halo, "node (0, 4), g slot 4: its source lies more than one row outside the slab's rows (unreachable)")
    near = pylbm.AdeOpenBoundary(lib, RG, C).add_g_copy(24, 5, 0, 1, 10, (-1, 0)).slab(24, R).finalize()
    refused(near, pylbm.Bc(row_lo=BB, row_hi=HALO), "node (0, 4), g slot 4: its source (-1, 5) lies in the ghost row of row_lo, "
            "whose edge mode is BOUNCE_BACK")
    part_o(lib, g, halo, prm, dst, src, FRAME, E, near, carry_like(near, 1), carry_like(near))  # HALO there: accepted
    # a redirected slot that the wall gather replaces is accepted at a wall, refused at a seam
    last = channel(lib, RG, C).slab(24, R).finalize()
    part_o(lib, g, pylbm.Bc(row_lo=HALO, row_hi=BB), prm, dst, src, FRAME, E, last, carry_like(last, 1), carry_like(last))
    refused(last, halo, "node (23, 0), g slot 3: its source lies more than one row outside")
    cols = columns(lib, RG, C).slab(24, R).finalize()
    refused(cols, halo, "NULL carry with a table of 72 nodes", cin=None)
    refused(cols, halo, "NULL carry with a table of 72 nodes", cout=None)
    refused(cols, halo, "carry_in and carry_out alias", cout="alias")
    ruled = pylbm.AdeInteriorWalls(lib, R, C).add(5, 0, 0, 1, 3, 0x0F, 0x0F).finalize()  # (5, 0) carries the inlet's rule
    refused(cols, halo, "node (5, 0) carries an open-boundary rule and is in the interior-wall table as well", walls=ruled)
    torch.cuda.synchronize()
    for t in (far, near, last, cols, ruled):
        t.close()


# ---- 7. real rank processes (tests/ade_ring_rank.py, entry "open") -------------------------------------------------------
@pytest.mark.parametrize("closed,kind", [(True, "columns"), (False, "channel")], ids=["closed_ring_columns", "walled_chain_channel"])
def test_ring_of_two_rank_processes_equals_one_block(lib, oracle, tmp_path, closed, kind):
    """lbm_ring_ade_collide_o + lbm_ring_ade_step_o, an open node on every seam row: the open pass of the FRAME rows runs
    before the pack -- enqueued behind it, the neighbour would receive an open node's un-fixed populations and its rows
    beside the seam would differ from one block"""
    n, R, C, steps, E, form = 2, 24, CG, 11, 4, FAST
    prm, gbc = params(form), (pylbm.Bc.periodic() if closed else WALLS)
    gg, pre = global_state(oracle, R * n, C, seed=2)
    table = build_open(lib, kind, R * n, C).finalize()
    counts = []
    for k in range(n):
        view = table.slab(k * R, R)
        assert bands_hold_nodes(view, E) and {0, R - 1} <= {nd["r"] for nd in view.nodes()}
        counts.append(view.count())
        view.close()
    _, _, want = one_block(lib, gg, pre, gbc, prm, (steps,), table)
    _, _, plain = one_block(lib, gg, pre, gbc, prm, (steps,), None)
    (wlat, wcarry), (plat, _) = want[steps], plain[steps]
    assert not torch.equal(bits(wlat[1]), bits(plat[1]))
    cfg = dict(R=R, C=C, steps=[steps], edge_rows=E, closed=int(closed), form=form, bc=bytes(gbc).hex(), w=list(W),
               entry="open", table=kind)
    outs = run_ranks(lib, tmp_path, "ade_ring_rank.py", n, cfg,
                     dict(f0=owned(pre[0], gg).cpu().numpy(), g0=owned(pre[1], gg).cpu().numpy()), timeout=240)
    for j, key in enumerate(("f", "g")):
        got = np.concatenate([o[f"{key}_{steps}"] for o in outs], axis=1)
        ref = owned(wlat[j], gg).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"{n} ranks closed={closed}: {key} differs"
    carry = np.concatenate([o["carry"] for o in outs])
    assert np.array_equal(carry.view(np.uint64), wcarry.cpu().numpy().view(np.uint64)), "carry differs"
    assert [int(o["nodes"]) for o in outs] == counts
    table.close()


# ---- 8. a chain of one slab in this process ------------------------------------------------------------------------------
@FORMS
def test_the_ring_entry_points_on_a_chain_of_one_slab_are_the_one_block(lib, oracle, form):
    """a ring of one rank, not closed: its rows keep their walls, nothing travels, both parts and both open passes run on
    the caller's stream; lbm_ring_ade_collide_o (k_ade_open_prime on the slab) + 5 x lbm_ring_ade_step_o with the whole-box
    view == lbm_ade_collide_o + 5 x lbm_ade_stream_collide_o"""
    R, C, E, steps = 34, 64, 2, 5
    prm = params(form)
    by = pylbm.AdeBuoyancy((2e-2, -1e-2), 1e-3, 0.5, (3.0, 9.0))
    gg, pre = global_state(oracle, R, C, seed=6)
    table = channel(lib, R, C).finalize()
    view = table.slab(0, R).finalize()
    assert view.count() == table.count() and bands_hold_nodes(view, E)
    post, c0, want = one_block(lib, gg, pre, WALLS, prm, (steps,), table, by=by)
    cut = [cut_slab(t, gg, 0, R, 0) for t in pre]  # ghost rows poisoned: beyond a wall nothing may read them
    sg = cut[0][0]
    lat = [[alloc(sg), alloc(sg)], [alloc(sg), alloc(sg)]]
    carry = [carry_like(view), carry_like(view)]
    with OneSlabRing(lib, sg) as ring:
        ade_calls.call(lib, "lbm_ring_ade_collide_o", rg=ring, dst=lat[0], src=(cut[0][1], cut[1][1]), bc=WALLS, prm=prm, buoy=by,
                       view=view, carry_out=carry[0])
        torch.cuda.synchronize()
        for j in range(2):
            assert_bits(owned(lat[0][j], sg), owned(post[j], gg), f"collide-only lattice {j}")
        assert_bits(carry[0], c0, "primed carry")
        for k in range(steps):
            a, b = k & 1, (k & 1) ^ 1
            ade_calls.call(lib, "lbm_ring_ade_step_o", rg=ring, dst=lat[b], src=lat[a], bc=WALLS, prm=prm, buoy=by, view=view,
                           carry_in=carry[a], carry_out=carry[b], edge_rows=E)
        torch.cuda.synchronize()
    (wlat, wcarry) = want[steps]
    for j in range(2):
        assert_bits(owned(lat[steps & 1][j], sg), owned(wlat[j], gg), f"lattice {j}")
    assert_bits(carry[steps & 1], wcarry, "carry")
    view.close()
    table.close()


# ---- 9. the tie to the reference's channel -------------------------------------------------------------------------------
def test_the_chain_channel_is_the_single_block_channel_but_for_the_lids_own_scalar(lib, oracle):
    """non-buoyant, 48 x 64, 40 steps.  The single-block channel under row_lo = PERIODIC is the configuration pinned to the
    oracle's sedimentation loop; a chain cannot wrap (nothing wraps where there are ghost rows), so its lid row is a
    BOUNCE_BACK row.  Every f population and the carry agree bit for bit, and so does g everywhere except row 0: the lid's
    own g takes the wall gather instead of the pull from the bottom row, and nothing reads it -- all nine readers of row 0
    are redirected to row 1 by the lid's copy.  Row 0 of g does differ: the test shows what it claims."""
    steps, heights = 40, (24, 24)
    prm = params(REF)
    gg, pre = global_state(oracle, RG, CG, seed=9)
    table = channel(lib, RG, CG).finalize()
    _, _, single = one_block(lib, gg, pre, pylbm.Bc(row_lo=PER, row_hi=BB), prm, (steps,), table)
    post, c0, _ = one_block(lib, gg, pre, WALLS, prm, (1,), table)
    ch = chain(lib, gg, post, c0, heights, False, WALLS, prm, table)
    for _ in range(steps):
        ch.step(4)
    torch.cuda.synchronize()
    (wlat, wcarry) = single[steps]
    assert_bits(ch.gather(0), owned(wlat[0], gg), "f")
    assert_bits(chain_carry(ch), wcarry, "carry")
    got, ref = ch.gather(1), owned(wlat[1], gg)
    assert_bits(got[:, 1:], ref[:, 1:], "g below the lid")
    assert not torch.equal(bits(got[:, 0]), bits(ref[:, 0]))
    ch.close()
    table.close()


# ---- 10. graph capture ---------------------------------------------------------------------------------------------------
def test_a_captured_graph_of_an_even_number_of_part_steps_replays_the_eager_run(lib, oracle):
    """FRAME + INNER with a view on ONE stream: the row-index lookup allocates nothing and synchronises nothing"""
    R, C, E = 24, CG, 3
    prm, bc = params(FAST), pylbm.Bc(row_lo=BB, row_hi=BB)
    gg, pre = global_state(oracle, R, C, seed=10)
    table = channel(lib, R, C).finalize()
    view = table.slab(0, R).finalize()
    post, c0, want = one_block(lib, gg, pre, bc, prm, (10, 20), table)
    cut = [cut_slab(t, gg, 0, R, 0) for t in post]
    sg = cut[0][0]
    lat = [[cut[0][1], cut[1][1]], [alloc(sg), alloc(sg)]]
    carry = [c0.clone(), carry_like(view)]
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        torch.cuda.synchronize()
        lib.graph_begin_capture(st)
        for k in range(10):  # even: lattices and carries are back where the capture found them
            a, b = k & 1, (k & 1) ^ 1
            for which in (FRAME, INNER):
                part_o(lib, sg, bc, prm, lat[b], lat[a], which, E, view, carry[a], carry[b], s=st.value)
        lib.graph_end_capture(st, ct.byref(graph))
        for n in (10, 20):
            lib.graph_launch(graph, 1, st)
            lib.stream_sync(st)
            (wlat, wcarry) = want[n]
            for j in range(2):
                assert_bits(owned(lat[0][j], sg), owned(wlat[j], gg), f"replay to step {n}, lattice {j}")
            assert_bits(carry[0], wcarry, f"replay to step {n}, carry")
    finally:
        if graph:
            lib.graph_destroy(graph)
        lib.stream_destroy(st)
    view.close()
    table.close()


# ---- 11. the driver ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["--buoyancy", "2e-2,-1e-2,5e-4"]], ids=["passive", "buoyant"])
def test_slab_ring_ade_driver_emulated_chain_of_three_with_the_channel_and_the_rectangle(extra):
    line = last_json(run_driver("slab_ring_ade", "--emulate", 3, "--rows", 16, "--cols", 64, "--walls", 1, "--channel", 1,
                                "--rectangle", 1, "--check", 1, *extra, timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["slabs"] == 3
    per_slab = line["open_nodes_per_slab"]
    assert len(per_slab) == 3 and sum(per_slab) == line["open_nodes"] and all(n > 0 for n in per_slab)
    assert line["interior_wall_nodes"] > 0
