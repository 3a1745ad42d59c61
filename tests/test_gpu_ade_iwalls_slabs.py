"""GPU suite, interior walls of the fluid + scalar step over row slabs and the ring: lbm_ade_iwalls_slab (the slab view of a
table), lbm_ade_stream_collide_part_w (k_ade_iwalls_ranges behind each part's dispatch), lbm_ring_ade_step_w and
slab_ring_ade --rectangle.

The yardstick is one block in the SAME form: lbm_ade_stream_collide_w on the global lattice with the global table (pinned
to the reference's loop bit for bit in tests/test_gpu_ade_iwalls.py).  Every comparison is bitwise, so there are no
tolerances -- except the scalar mass of the sealed seam, whose bound is that of test_a_sealed_wall_seals.

The body, on a global 48 x 64 lattice: a column wall at column 20 through ALL rows (COL_NEG for f and g) and row walls at
rows 5 and 29, columns 20..30 (ROW_NEG): 68 nodes, 34 in each of the views [0, 24), [24, 48), [12, 36).  The column wall
puts a node on the first and last row of every slab and into every FRAME and INNER band for any E; each test asserts that
each band it exercises holds a table node (bands_hold_nodes), so that none passes by testing nothing.  The body, the chain of
slabs and the write-set check of a part are tests/ade_slab_util.py's; every raw call goes through tests/ade_calls.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
import ade_calls  # noqa: E402
from ade_slab_util import (Chain, OneSlabRing, assert_part_write_sets, bands_hold_nodes, body_segments, body_table,  # noqa: E402
                           global_state, slab_bc)
from ade_util import (GBC, GUO, W, alloc, assert_bits, bits, buoyancy, cut_slab, geom, moment_fields, owned, params,  # noqa: E402
                      poisoned, random_lattice, to_lattice)
from gpu_util import dev  # noqa: E402
from proc_util import last_json, run_driver, run_ranks  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
BB, SP, HALO, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO, pylbm.EDGE_PERIODIC
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_POS, ROW_NEG, COL_NEG = pylbm.ADE_FACE_ROW_POS, pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_NEG
RG, CG = 48, 64


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


# the yardstick is lbm_ade_stream_collide_w on one block; the calls under test are lbm_ade_stream_collide_part_w's
def chain(lib, gg, post, heights, closed, gbc, prm, table):
    """ade_slab_util.Chain through lbm_ade_stream_collide_part_w, every slab with its view of the global table"""
    return Chain(lib, gg, post, heights, closed, gbc,
                 lambda s, dst, src, e: ade_calls.both_parts(lib, "_w", s["g"], s["bc"], prm, dst, src, e, iwalls=s["view"]),
                 per_slab=lambda k, a, b, bc: dict(view=table.slab(a, b - a).finalize() if table is not None else None))


# ---- 1. FRAME + INNER with a view == the one-block step on the global lattice --------------------------------------------
CASES = {"no_flux": ((NO_FLUX, 0.0), False), "absorbing": ((FIXED, 0.0), False), "fixed_row_lo_buoyant": ((FIXED, 1e-3), True)}


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("C,pitch", [(CG, 0), (1040, 1056)], ids=["48x64", "48x1040_padded"])
def test_frame_plus_inner_with_a_view_is_the_one_block_step(lib, form, case, C, pitch):
    rule, driven = CASES[case]
    prm = params(form)
    by = buoyancy((2e-2, -1e-2), 1.0, GUO) if driven else None      # random_lattice: C ~ 1.0 .. 1.05
    gsbc = pylbm.AdeScalarBC(row_lo=1.02) if driven else None        # a FIXED domain edge beside the table's FIXED slots
    gg = geom(RG, C, 0, pitch)
    src = (random_lattice(gg, 11 + C), random_lattice(gg, 12 + C))
    table = body_table(lib, RG, C, rule)
    assert table.count() == 68
    twin = body_table(lib, RG, C, rule, finalize=False)
    want = ade_calls.full_step(lib, "_w", gg, GBC, prm, *src, sbc=gsbc, buoy=by, iwalls=table)
    plain = ade_calls.full_step(lib, "_w", gg, GBC, prm, *src, sbc=gsbc, buoy=by)
    assert not torch.equal(bits(want[1]), bits(plain[1]))  # the body is felt
    for r0, r1 in ((0, 24), (24, 48), (12, 36)):
        view = table.slab(r0, r1 - r0)
        other = twin.slab(r0, r1 - r0)
        assert view.count() == 34 and view.nodes() == other.nodes()  # a finalized parent gives the unfinalized one's view
        other.close()
        view.finalize()
        bc = slab_bc(GBC, r0, r1, RG)
        sbc = gsbc if (driven and r0 == 0) else None  # a FIXED row acts where the slab keeps that edge
        slab = [cut_slab(s, gg, r0, r1, pitch) for s in src]
        sg = slab[0][0]
        for E in (1, 3, 8):
            assert bands_hold_nodes(view, E)
            dst = (alloc(sg), alloc(sg))
            ade_calls.both_parts(lib, "_w", sg, bc, prm, dst, (slab[0][1], slab[1][1]), E, sbc=sbc, buoy=by, iwalls=view)
            torch.cuda.synchronize()
            for k in range(2):
                assert_bits(owned(dst[k], sg), owned(want[k], gg)[:, r0:r1], f"{case} C={C} slab [{r0}, {r1}) E={E} lattice {k}")
        view.close()
    twin.close()
    table.close()


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_the_moment_outputs_of_wall_nodes_are_the_one_block_steps(lib, form):
    """ghost 0, periodic rows (what both entry points accept): rho, u, C of FRAME + INNER == lbm_ade_stream_collide_w's"""
    R, C, E = 24, CG, 3
    g, prm, bc = geom(R, C, 0), params(form), pylbm.Bc(col_lo=BB, col_hi=SP)
    table = body_table(lib, R, C, (FIXED, 1e-3))
    assert bands_hold_nodes(table, E)
    src = (random_lattice(g, 3), random_lattice(g, 4))

    mw, mp, mplain = moment_fields(g), moment_fields(g), moment_fields(g)
    want = ade_calls.full_step(lib, "_w", g, bc, prm, *src, iwalls=table, moments=mw)
    ade_calls.full_step(lib, "_w", g, bc, prm, *src, moments=mplain)
    dst = (alloc(g), alloc(g))
    ade_calls.both_parts(lib, "_w", g, bc, prm, dst, src, E, iwalls=table, moments=mp)
    torch.cuda.synchronize()
    for k in range(2):
        assert_bits(owned(dst[k], g), owned(want[k], g), f"lattice {k}")
    for k, name in enumerate(("rho", "u", "C")):
        assert_bits(mp[k], mw[k], name)
    assert not torch.equal(bits(mw[2]), bits(mplain[2]))  # the wall nodes' C is the table's, not the plain step's
    table.close()


# ---- 2. NULL and empty table == _part_b ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_null_and_empty_tables_are_part_b(lib, form):
    R, C, E = 24, CG, 3
    prm = params(form)
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO, col_lo=BB, col_hi=SP)
    sbc, by = pylbm.AdeScalarBC(row_lo=1.02, col_hi=0.0), buoyancy((2e-2, -1e-2), 1.0, GUO)
    g = geom(R, C, 1, C + 6)
    src = (random_lattice(g, 1), random_lattice(g, 2))
    empty = pylbm.AdeInteriorWalls(lib, R, C).finalize()
    view = pylbm.AdeInteriorWalls(lib, 48, C).add(40, 3, 0, 1, 5, ROW_NEG, ROW_NEG).slab(0, R).finalize()  # no node in its rows
    assert view.count() == 0
    for drive in (None, by):
        outs = []
        for t in ("b", None, empty, view):
            dst = (poisoned(g), poisoned(g))
            if t == "b":
                ade_calls.both_parts(lib, "_b", g, bc, prm, dst, src, E, sbc=sbc, buoy=drive)
            else:
                ade_calls.both_parts(lib, "_w", g, bc, prm, dst, src, E, sbc=sbc, buoy=drive, iwalls=t)
            torch.cuda.synchronize()
            outs.append(dst)
        for i, what in ((1, "NULL"), (2, "empty"), (3, "empty view")):
            for k in range(2):
                assert_bits(outs[i][k], outs[0][k], f"{what} table, lattice {k}")  # the whole allocation, padding included
    empty.close()
    view.close()


# ---- 3. write sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,E", [(24, 64, 1), (24, 64, 8), (33, 96, 5)])
@pytest.mark.parametrize("walls", [0, 1])
def test_each_part_alone_with_the_table_writes_exactly_its_rows(lib, R, C, E, walls):
    """NaN-poisoned destinations, ghost rows and row / plane padding included: each part (its dispatch and its wall pass)
    changes exactly its rows -- so FRAME leaves INNER's wall nodes unwritten and the reverse -- and every written double is
    the one of FRAME + INNER together; the wall nodes' are the table's, not the plain step's"""
    prm = params(FAST)
    bc = pylbm.Bc(row_lo=BB if walls else HALO, row_hi=HALO, col_lo=BB if walls else PER, col_hi=SP if walls else PER)
    g = geom(R, C, 1, C + 10)
    table = body_table(lib, R, C, (FIXED, 1e-3))  # built for the slab, not viewed
    assert bands_hold_nodes(table, E)
    src = (random_lattice(g, R), random_lattice(g, C))
    want, plain = [alloc(g), alloc(g)], [alloc(g), alloc(g)]
    for which in (FRAME, INNER):
        ade_calls.part(lib, "_w", g, bc, prm, want, src, which, E, iwalls=table)
        ade_calls.part(lib, "_b", g, bc, prm, plain, src, which, E)
    torch.cuda.synchronize()
    wall_rows = sorted({n["r"] for n in table.nodes()})
    for k in range(2):
        differs = (bits(owned(want[k], g)) != bits(owned(plain[k], g))).any(dim=0).any(dim=1)
        assert differs.tolist() == [r in wall_rows for r in range(R)], (k, differs.tolist())
    assert_part_write_sets(lambda dst, which: ade_calls.part(lib, "_w", g, bc, prm, dst, src, which, E, iwalls=table), g, want, E,
                           f"R={R} C={C} E={E} walls={walls}")
    table.close()


# ---- 4. chains and rings of slabs in one process -------------------------------------------------------------------------
def one_block(lib, gg, pre, gbc, prm, steps, table):
    """lbm_ade_collide + `steps` x lbm_ade_stream_collide_w on the global lattice: (post-collision state, after steps)"""
    post = [alloc(gg), alloc(gg)]
    ade_calls.collide(lib, "", gg, gbc, prm, post, pre)
    cur = [t.clone() for t in post]
    for _ in range(steps):
        cur = list(ade_calls.full_step(lib, "_w", gg, gbc, prm, *cur, iwalls=table))
    torch.cuda.synchronize()
    return post, cur


@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
@pytest.mark.parametrize("heights", [(24, 24), (16, 20, 12)])
def test_emulated_chain_with_the_body_equals_one_block(lib, oracle, form, closed, heights):
    """20 steps; on the closed ring (a periodic box) the column wall also crosses the wrap-around seam"""
    prm, gbc = params(form), (pylbm.Bc.periodic() if closed else GBC)
    E, steps = 4, 20
    gg, pre = global_state(oracle, RG, CG)
    table = body_table(lib, RG, CG, (FIXED, 1e-3))
    post, want = one_block(lib, gg, pre, gbc, prm, steps, table)
    _, plain = one_block(lib, gg, pre, gbc, prm, steps, None)
    assert not torch.equal(bits(want[0]), bits(plain[0])) and not torch.equal(bits(want[1]), bits(plain[1]))
    ch = chain(lib, gg, post, heights, closed, gbc, prm, table)
    assert all(bands_hold_nodes(s["view"], min(E, (s["g"].R - 1) // 2)) for s in ch.slabs)
    for _ in range(steps):
        ch.step(E)
    torch.cuda.synchronize()
    for j in range(2):
        assert_bits(ch.gather(j), owned(want[j], gg), f"{len(heights)} slabs {heights} closed={closed} lattice {j}")
    ch.close()
    table.close()


# ---- 5. real rank processes (tests/ade_ring_rank.py, entry "walls") ------------------------------------------------------
@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
def test_ring_of_rank_processes_with_the_body_equals_one_block(lib, oracle, tmp_path, closed):
    """two ranks, lbm_ring_ade_step_w: the wall pass of the FRAME rows runs before the pack -- enqueued behind it, the
    neighbour would receive a wall node's un-fixed populations and its rows beside the seam would differ from one block"""
    n, R, C, steps, E, form = 2, 24, CG, 11, 4, FAST
    rule = (FIXED, 1e-3)
    prm, gbc = params(form), (pylbm.Bc.periodic() if closed else GBC)
    gg, pre = global_state(oracle, R * n, C, seed=2)
    table = body_table(lib, R * n, C, rule)
    for k in range(n):
        view = table.slab(k * R, R)
        assert bands_hold_nodes(view, E)
        view.close()
    _, want = one_block(lib, gg, pre, gbc, prm, steps, table)
    _, plain = one_block(lib, gg, pre, gbc, prm, steps, None)
    assert not torch.equal(bits(want[1]), bits(plain[1]))
    cfg = dict(R=R, C=C, steps=[steps], edge_rows=E, closed=int(closed), form=form, bc=bytes(gbc).hex(), w=list(W),
               entry="walls", segments=body_segments(R * n), g_mode=rule[0], conc=rule[1])
    outs = run_ranks(lib, tmp_path, "ade_ring_rank.py", n, cfg,
                     dict(f0=owned(pre[0], gg).cpu().numpy(), g0=owned(pre[1], gg).cpu().numpy()), timeout=240)
    for j, key in enumerate(("f", "g")):
        got = np.concatenate([o[f"{key}_{steps}"] for o in outs], axis=1)
        ref = owned(want[j], gg).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"{n} ranks closed={closed}: {key} differs"
    assert [int(o["nodes"]) for o in outs] == [34, 34]
    table.close()


# ---- 6. a chain of one slab in this process ------------------------------------------------------------------------------
def test_ring_step_w_on_a_chain_of_one_slab_is_the_one_block_step(lib):
    """a ring of one rank, not closed: its rows keep their walls, nothing travels, both parts and both wall passes run on
    the caller's stream.  lbm_ring_ade_step_w with the body, a FIXED row, a FIXED profile column and buoyancy ==
    lbm_ade_stream_collide_w on the same block after 3 steps, bit for bit"""
    R, C, E, steps = 34, 64, 2, 3
    prm = params(FAST)
    by = pylbm.AdeBuoyancy((2e-2, -1e-2), 1.0, 0.5, (3.0, 9.0))  # random_lattice: C ~ 1.0 .. 1.05
    prof = torch.from_numpy(np.linspace(0.9, 1.1, R)).to(dev())
    sbc = pylbm.AdeScalarBC(row_lo=1.02, col_lo=(0.0, prof), col_hi=0.0)
    table = body_table(lib, R, C, (FIXED, 1.01))
    assert bands_hold_nodes(table, E)
    gg = geom(R, C, 0)
    want = [random_lattice(gg, 1), random_lattice(gg, 2)]
    plain = want
    cut = [cut_slab(t, gg, 0, R, 0) for t in want]  # ghost rows poisoned: beyond a wall nothing may read them
    sg = cut[0][0]
    lat = [[cut[0][1], cut[1][1]], [alloc(sg), alloc(sg)]]
    for _ in range(steps):
        want = ade_calls.full_step(lib, "_w", gg, GBC, prm, *want, sbc=sbc, buoy=by, iwalls=table)
        plain = ade_calls.full_step(lib, "_w", gg, GBC, prm, *plain, sbc=sbc, buoy=by)
    with OneSlabRing(lib, sg) as ring:
        for k in range(steps):
            ade_calls.call(lib, "lbm_ring_ade_step_w", rg=ring, dst=lat[(k & 1) ^ 1], src=lat[k & 1], bc=GBC, prm=prm, sbc=sbc,
                           buoy=by, iwalls=table, edge_rows=E)
        torch.cuda.synchronize()
    for j in range(2):
        assert_bits(owned(lat[steps & 1][j], sg), owned(want[j], gg), f"lattice {j}")
        assert not torch.equal(bits(owned(want[j], gg)), bits(owned(plain[j], gg)))
    table.close()


# ---- 7. a sealed wall on a seam ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
def test_a_sealed_wall_on_a_seam_seals(lib, oracle, form):
    """rows BOUNCE_BACK, fluid at rest, w = 0, two slabs of 12 rows; a full-width pair on the seam -- ROW_NEG on the last
    row of slab 0, ROW_POS on the first row of slab 1, NO_FLUX; the scalar starts above the pair only: after 200 steps C
    and g in slab 1 are exactly 0.0 at every node -- and are not without the table.  The mass above is conserved to
    rounding; the bound is test_a_sealed_wall_seals's, fixed before measuring: 200 steps x about 20 roundings per
    population and step x 2^-53 = 4.4e-13 if every rounding erred the same way, so 1e-12 relative"""
    heights, C, k, steps = (12, 12), 32, 11, 200
    Rg = sum(heights)
    prm, gbc = params(form, w=(0.0, 0.0)), pylbm.Bc(row_lo=BB, row_hi=BB)
    u = np.zeros((Rg, C, 2))
    conc = np.zeros((Rg, C))
    conc[:k + 1] = 1e-3 * (1.0 + 0.5 * np.cos(2 * np.pi * np.arange(C) / C))[None, :]
    gg = geom(Rg, C, 0)
    pre = [to_lattice(a, gg) for a in (oracle.equilibrium(u, np.ones((Rg, C))), oracle.equilibrium(u, conc))]
    post, _ = one_block(lib, gg, pre, gbc, prm, 0, None)
    table = pylbm.AdeInteriorWalls(lib, Rg, C).add(k, 0, 0, 1, C, ROW_NEG, ROW_NEG).add(k + 1, 0, 0, 1, C, ROW_POS, ROW_POS)
    table.finalize()
    out = {}
    for name, t in (("sealed", table), ("open", None)):
        ch = chain(lib, gg, post, heights, False, gbc, prm, t)
        if t is not None:  # E = 2: the pair lies in the FRAME bands of both slabs
            assert [s["view"].count() for s in ch.slabs] == [C, C]
            assert {n["r"] for n in ch.slabs[0]["view"].nodes()} == {11} and {n["r"] for n in ch.slabs[1]["view"].nodes()} == {0}
        for _ in range(steps):
            ch.step(2)
        torch.cuda.synchronize()
        out[name] = ch.gather(1).cpu().numpy()  # [9, Rg, C]
        ch.close()
    sealed_C, open_C = out["sealed"].sum(axis=0), out["open"].sum(axis=0)
    assert np.all(out["sealed"][:, k + 1:] == 0.0) and np.all(sealed_C[k + 1:] == 0.0)
    assert np.all(sealed_C[:k + 1] > 0.0)
    assert np.all(open_C[k + 1:k + 4] > 0.0)
    assert abs(sealed_C.sum() - conc.sum()) <= 1e-12 * conc.sum()
    table.close()


# ---- 8. the driver -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fast", "ref"])
def test_slab_ring_ade_driver_emulated_chain_of_four_with_the_rectangle(form):
    line = last_json(run_driver("slab_ring_ade", "--emulate", 4, "--rows", 48, "--cols", 200, "--steps", 9, "--warmup", 2,
                                "--edge-rows", 8, "--walls", 1, "--rectangle", 1, "--form", form, "--check", 1, timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["slabs"] == 4
    assert line["interior_wall_nodes"] > 0
    per_slab = line["interior_wall_nodes_per_slab"]
    assert len(per_slab) == 4 and sum(per_slab) == line["interior_wall_nodes"]
    assert sum(1 for n in per_slab if n > 0) >= 2 and per_slab[2] > 0 and per_slab[3] > 0  # the body crosses the seam 2 | 3


def test_slab_ring_ade_driver_self_ring_with_the_rectangle(tmp_path):
    """one forked rank with walls: a chain of one slab through lbm_ring_ade_step_w == one block bit for bit"""
    line = last_json(run_driver("slab_ring_ade", "--spawn", 1, "--rows", 96, "--cols", 256, "--steps", 5, "--warmup", 1,
                                "--edge-rows", 16, "--walls", 1, "--rectangle", 1, "--check", 1, "--id-file", tmp_path / "id",
                                timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["n_gpus"] == 1 and line["interior_wall_nodes"] > 0


def test_slab_ring_ade_driver_refuses_the_rectangle_without_walls():
    r = run_driver("slab_ring_ade", "--emulate", 2, "--rows", 48, "--cols", 64, "--rectangle", 1, timeout=60, check=False)
    assert r.returncode != 0
    assert "--rectangle 1 needs --walls 1" in r.stderr
