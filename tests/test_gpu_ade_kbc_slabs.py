"""GPU suite, the fluid + scalar step with a KBC fluid over row slabs and the ring: lbm_ade_stream_collide_part_m (the part
kernel of ade_kbc.hpp, k_ade_kbc_stream_collide_part, + the interior-wall pass of the part's rows), lbm_ring_ade_collide_m,
lbm_ring_ade_step_m and slab_ring_ade --fluid kbc (its --check reports the non-finite values of its one block, asserted 0).

The yardstick is one block in the SAME form: lbm_ade_collide_m / lbm_ade_stream_collide_m on the global lattice (pinned to
the CPU composition of the oracle's kbc::collide bit for bit in tests/test_gpu_ade_kbc.py), computed once per case, left
unchanged and asserted finite wherever it is used -- equal NaNs must not pass.  One chain is also tied to
ade_kbc_util.oracle_loop, which never calls the library.  Every comparison is on bit patterns, in both forms, so there
are no tolerances.  Start states: ade_util.initial_state (off equilibrium: KBC's gamma is 0/0 on a lattice at equilibrium)
with ade_kbc_util.S2.  The body, the chain of slabs and the write-set check of a part are tests/ade_slab_util.py's; every raw
call goes through tests/ade_calls.py, the rank processes run tests/ade_ring_rank.py with entry "model"."""
import ctypes as ct
import functools
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ade_calls  # noqa: E402
import ade_kbc_util as kbc  # noqa: E402
import pylbm  # noqa: E402
from ade_slab_util import (Chain, OneSlabRing, assert_finite, assert_part_write_sets, bands_hold_nodes, body_segments,  # noqa: E402
                           body_table, slab_bc)
from ade_util import (GBC, SENTINEL, W, alloc, assert_bits, bits, cut_slab, geom, initial_state, moment_fields, owned,  # noqa: E402
                      poisoned, to_lattice)
from ade_util import params as bgk_params  # noqa: E402
from gpu_util import dev  # noqa: E402
from proc_util import ipc_env, last_json, run_driver, run_ranks  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FORMS = pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
BB, SP, HALO, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO, pylbm.EDGE_PERIODIC
FIXED = pylbm.ADE_SCALAR_FIXED
ROW_NEG, COL_NEG = pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_NEG
S2, OMEGA_G = kbc.S2, kbc.OMEGA_G
RG = 48
RULE = (FIXED, 1e-3)  # of the body's g slots


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(autouse=True)
def _default_knobs_afterwards(lib):
    yield
    lib.reset_tuning()


# ---- the calls under test and the one block ------------------------------------------------------------------------------
def chain(lib, gg, post, heights, closed, gbc, prm):
    return Chain(lib, gg, post, heights, closed, gbc,
                 lambda s, dst, src, e: ade_calls.both_parts(lib, "_m", s["g"], s["bc"], prm, dst, src, e))


@functools.lru_cache(maxsize=None)
def _start(R, C, seed):
    from pyoracle import Oracle
    f, g = initial_state(Oracle(), R, C, seed=seed)
    f.setflags(write=False)
    g.setflags(write=False)
    return f, g


def post_collision(lib, gg, gbc, prm, seed=None):
    """(pre, post): ade_util.initial_state on the lattice of gg and its post-collision pair, lbm_ade_collide_m"""
    f, g = _start(gg.R, gg.C, gg.R * gg.C if seed is None else seed)
    pre = [to_lattice(f, gg), to_lattice(g, gg)]
    post = [alloc(gg), alloc(gg)]
    ade_calls.collide(lib, "_m", gg, gbc, prm, post, pre)
    torch.cuda.synchronize()
    assert_finite(post, gg, "post-collision state")
    return pre, post


# ---- 1. FRAME + INNER == lbm_ade_stream_collide_m on one block (ghost = 0) ---------------------------------------------------
SHAPES = {"3x2": (3, 2, 0, (1,)), "6x8": (6, 8, 0, (1, 2)), "48x64": (48, 64, 0, (1, 3, 8)), "48x1040_padded": (48, 1040, 1056, (8,))}
EDGES = {"periodic": pylbm.Bc(), "box": GBC}


@FORMS
@pytest.mark.parametrize("edges", list(EDGES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frame_plus_inner_is_the_one_block_step(lib, form, edges, shape):
    """with and without moments; rho, u and conc are equal too"""
    R, C, pitch, Es = SHAPES[shape]
    g, bc, prm = geom(R, C, 0, pitch), EDGES[edges], kbc.params(form)
    _, src = post_collision(lib, g, bc, prm)
    mw = moment_fields(g)
    want = ade_calls.full_step(lib, "_m", g, bc, prm, *src, moments=mw)
    torch.cuda.synchronize()
    assert_finite(want, g, shape)
    assert all(bool(torch.isfinite(t).all()) for t in mw)
    for E in Es:
        for with_moments in (True, False):
            dst, mp = (alloc(g), alloc(g)), (moment_fields(g) if with_moments else None)
            ade_calls.both_parts(lib, "_m", g, bc, prm, dst, src, E, moments=mp)
            torch.cuda.synchronize()
            for k in range(2):
                assert_bits(owned(dst[k], g), owned(want[k], g), f"{shape} {edges} E={E} moments={with_moments} lattice {k}")
            if with_moments:
                for k, name in enumerate(("rho", "u", "C")):
                    assert_bits(mp[k], mw[k], f"{shape} {edges} E={E} {name}")


# ---- 2. each part alone writes exactly its rows ----------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("walls", [0, 1])
@pytest.mark.parametrize("R,C,pitch,E", [(48, 1040, 1056, 8), (6, 8, 18, 1)], ids=["48x1040_padded", "6x8"])
def test_each_part_alone_writes_exactly_its_rows(lib, form, walls, R, C, pitch, E):
    """NaN-poisoned targets on a ghost-1 slab cut from a global lattice of R + 2 rows: ghost rows, row-pitch padding and
    plane padding stay untouched, and every written double is the one FRAME + INNER write together"""
    prm = kbc.params(form)
    bc = pylbm.Bc(row_lo=HALO, row_hi=HALO, col_lo=BB if walls else PER, col_hi=SP if walls else PER)
    gg = geom(R + 2, C, 0)
    _, post = post_collision(lib, gg, pylbm.Bc(col_lo=bc.col_lo, col_hi=bc.col_hi), prm)
    cut = [cut_slab(p, gg, 1, R + 1, pitch) for p in post]
    g, src = cut[0][0], (cut[0][1], cut[1][1])
    want = (alloc(g), alloc(g))
    ade_calls.both_parts(lib, "_m", g, bc, prm, want, src, E)
    torch.cuda.synchronize()
    assert_finite(want, g, "FRAME + INNER")
    assert_part_write_sets(lambda dst, which: ade_calls.part(lib, "_m", g, bc, prm, dst, src, which, E), g, want, E,
                           f"{R}x{C} E={E} walls={walls}")


# ---- 3. slabs cut from a global 48 x C lattice -----------------------------------------------------------------------------
def fixed_edges(r0, r1, prof):
    """the scalar's FIXED edges of the slab of global rows [r0, r1): row 0 constant where the slab keeps it, column 0 the
    profile's slice, column C - 1 absorbing"""
    kw = dict(col_lo=(0.0, prof[r0:r1]), col_hi=0.0)
    if r0 == 0:
        kw["row_lo"] = 7e-4
    return pylbm.AdeScalarBC(**kw)


@FORMS
@pytest.mark.parametrize("case", ["box", "fixed", "body"])
@pytest.mark.parametrize("C,pitch", [(64, 0), (1040, 1056)], ids=["48x64", "48x1040_padded"])
def test_slabs_cut_from_the_global_lattice_give_the_one_blocks_rows(lib, form, case, C, pitch):
    """views [0, 24), [24, 48), [12, 36) with ghost = 1 and HALO seams, ghost rows from the global post-collision lattices"""
    prm = kbc.params(form)
    gg = geom(RG, C, 0, pitch)
    _, src = post_collision(lib, gg, GBC, prm)
    prof = torch.from_numpy(np.linspace(1.5e-3, 3e-4, RG)).to(dev())
    gsbc = fixed_edges(0, RG, prof) if case == "fixed" else None
    table = body_table(lib, RG, C, RULE) if case == "body" else None
    want = ade_calls.full_step(lib, "_m", gg, GBC, prm, *src, sbc=gsbc, iwalls=table)
    plain = ade_calls.full_step(lib, "_m", gg, GBC, prm, *src)
    torch.cuda.synchronize()
    assert_finite(want, gg, case)
    if case != "box":
        assert not torch.equal(bits(want[1]), bits(plain[1]))  # the walls of the case are felt
    for r0, r1 in ((0, 24), (24, 48), (12, 36)):
        view = table.slab(r0, r1 - r0).finalize() if table is not None else None
        sbc = fixed_edges(r0, r1, prof) if case == "fixed" else None
        bc = slab_bc(GBC, r0, r1, RG)
        cut = [cut_slab(s, gg, r0, r1, pitch) for s in src]
        sg = cut[0][0]
        for E in (1, 3, 8):
            assert view is None or bands_hold_nodes(view, E)
            dst = (alloc(sg), alloc(sg))
            ade_calls.both_parts(lib, "_m", sg, bc, prm, dst, (cut[0][1], cut[1][1]), E, sbc=sbc, iwalls=view)
            torch.cuda.synchronize()
            for k in range(2):
                assert_bits(owned(dst[k], sg), owned(want[k], gg)[:, r0:r1], f"{case} C={C} slab [{r0}, {r1}) E={E} lattice {k}")
        if view is not None:
            view.close()
    if table is not None:
        table.close()


# ---- 4. emulated chains and closed rings -----------------------------------------------------------------------------------
@FORMS
@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
@pytest.mark.parametrize("heights,C", [((24, 24), 64), ((16, 20, 12), 64), ((3, 3, 3, 3), 8)], ids=["2x24x64", "16_20_12x64", "4x3x8"])
def test_emulated_chain_equals_one_block(lib, form, closed, heights, C):
    """after 1, 2 and 20 steps"""
    prm, gbc = kbc.params(form), (pylbm.Bc.periodic() if closed else GBC)
    gg = geom(sum(heights), C, 0)
    _, post = post_collision(lib, gg, gbc, prm)
    ch = chain(lib, gg, post, heights, closed, gbc, prm)
    want, done = [t.clone() for t in post], 0
    for n in (1, 2, 20):
        for _ in range(n - done):
            want = list(ade_calls.full_step(lib, "_m", gg, gbc, prm, *want))
            ch.step(4)
        done = n
        torch.cuda.synchronize()
        assert_finite(want, gg, f"{n} steps")
        for j in range(2):
            assert_bits(ch.gather(j), owned(want[j], gg), f"slabs {heights} closed={closed} after {n} steps, lattice {j}")


@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
def test_emulated_chain_in_the_reference_order_equals_the_oracle_loop(lib, oracle, closed):
    """2 slabs of 24 x 64 after 2 steps against a yardstick that never calls the library: the pre-collision state through
    ade_kbc_util.oracle_loop on the CPU (2 iterations, each a collision and a stream), then collided once more for the
    post-collision pair the lattices hold"""
    heights, C, steps = (24, 24), 64, 2
    prm, gbc = kbc.params(REF), (pylbm.Bc.periodic() if closed else GBC)
    gg = geom(sum(heights), C, 0)
    _, post = post_collision(lib, gg, gbc, prm)
    f0, g0 = _start(gg.R, C, gg.R * C)
    st = kbc.oracle_loop(oracle, f0.copy(), g0.copy(), S2, OMEGA_G, W, steps, gbc)
    assert kbc.finite(st)
    c = kbc.collide(oracle, st["f"], st["g"], S2, OMEGA_G, W)
    assert np.all(np.isfinite(c["fc"])) and np.all(np.isfinite(c["gc"]))
    ch = chain(lib, gg, post, heights, closed, gbc, prm)
    for _ in range(steps):
        ch.step(4)
    torch.cuda.synchronize()
    for j, key in enumerate(("fc", "gc")):
        want = torch.from_numpy(np.ascontiguousarray(c[key].transpose(2, 0, 1))).to(dev())
        assert_bits(ch.gather(j), want, f"closed={closed} lattice {j} against the oracle loop")


# ---- 5. rank processes (tests/ade_ring_rank.py, entry "model") -------------------------------------------------------------
def one_block_after(lib, gg, gbc, prm, post, counts, table=None):
    """{n: the lattices after n steps of lbm_ade_stream_collide_m from the post-collision pair}"""
    out, cur, done = {}, [t.clone() for t in post], 0
    for n in counts:
        for _ in range(n - done):
            cur = list(ade_calls.full_step(lib, "_m", gg, gbc, prm, *cur, iwalls=table))
        done = n
        torch.cuda.synchronize()
        assert_finite(cur, gg, f"one block after {n} steps")
        out[n] = cur
    return out


@FORMS
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
def test_ring_of_rank_processes_equals_one_block(lib, tmp_path, form, n, closed):
    """n ranks sharing this GPU on the peer-mapped transport through lbm_ring_ade_collide_m / lbm_ring_ade_step_m, with a
    wall node on every seam row: the wall pass of the FRAME rows runs before the pack -- behind it, the neighbour would
    receive a wall node's un-fixed populations.  Equal to one block after 1 and 20 steps"""
    R, C, E, counts = 24, 64, 4, (1, 20)
    rule = (FIXED, 1e-3)
    prm, gbc = kbc.params(form), (pylbm.Bc.periodic() if closed else GBC)
    gg = geom(R * n, C, 0)
    pre, post = post_collision(lib, gg, gbc, prm)
    table = body_table(lib, R * n, C, rule)
    rows = {nd["r"] for nd in table.nodes()}
    assert all(k * R in rows and k * R + R - 1 in rows for k in range(n))  # a wall node on every seam row
    want = one_block_after(lib, gg, gbc, prm, post, counts, table)
    plain = one_block_after(lib, gg, gbc, prm, post, counts)
    assert not torch.equal(bits(want[20][1]), bits(plain[20][1]))
    cfg = dict(R=R, C=C, steps=list(counts), edge_rows=E, closed=int(closed), form=form, bc=bytes(gbc).hex(), w=list(W), s2=S2,
               omega_g=OMEGA_G, entry="model", segments=body_segments(R * n), g_mode=rule[0], conc=rule[1])
    outs = run_ranks(lib, tmp_path, "ade_ring_rank.py", n, cfg,
                     dict(f0=owned(pre[0], gg).cpu().numpy(), g0=owned(pre[1], gg).cpu().numpy()), timeout=240)
    for steps in counts:
        for j, key in enumerate(("f", "g")):
            got = np.concatenate([o[f"{key}_{steps}"] for o in outs], axis=1)
            ref = owned(want[steps][j], gg).cpu().numpy()
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"{n} ranks closed={closed} after {steps}: {key} differs"
    assert sum(int(o["nodes"]) for o in outs) == table.count() and all(int(o["nodes"]) > 0 for o in outs)
    table.close()


def test_ring_entry_points_refuse_a_ring_without_one_ghost_row(lib, tmp_path):
    """ghost = 2 on the ring: both `_m` ring entries refuse it on the host with the existing message"""
    cfg = dict(case="refusals", entry="model", R=32, C=64, s2=S2, omega_g=OMEGA_G, form=FAST, w=list(W))
    outs = run_ranks(lib, tmp_path, "ade_ring_rank.py", 1, cfg, {}, timeout=240)
    msgs = json.loads(str(outs[0]["msgs"]))
    assert len(msgs) == 2
    for name, m in zip(("lbm_ring_ade_collide_m", "lbm_ring_ade_step_m"), msgs):
        assert f"{name}: ghost=2: the fluid + scalar step over slabs exchanges one ghost row per side" in m, m


@FORMS
def test_ring_step_m_on_a_chain_of_one_slab_is_the_one_block_step(lib, form):
    """with the body, a FIXED row, a FIXED profile column and an absorbing column, after 3 steps"""
    R, C, E, steps = 34, 64, 2, 3
    prm = kbc.params(form)
    prof = torch.from_numpy(np.linspace(1.5e-3, 3e-4, R)).to(dev())
    sbc = pylbm.AdeScalarBC(row_lo=7e-4, col_lo=(0.0, prof), col_hi=0.0)
    table = body_table(lib, R, C, RULE)
    assert bands_hold_nodes(table, E)
    gg = geom(R, C, 0)
    _, want = post_collision(lib, gg, GBC, prm)
    plain = want
    cut = [cut_slab(t, gg, 0, R, 0) for t in want]  # ghost rows poisoned: beyond a wall nothing may read them
    sg = cut[0][0]
    lat = [[cut[0][1], cut[1][1]], [alloc(sg), alloc(sg)]]
    for _ in range(steps):
        want = ade_calls.full_step(lib, "_m", gg, GBC, prm, *want, sbc=sbc, iwalls=table)
        plain = ade_calls.full_step(lib, "_m", gg, GBC, prm, *plain)
    torch.cuda.synchronize()
    assert_finite(want, gg, "one block")
    with OneSlabRing(lib, sg) as ring:
        for k in range(steps):
            src, dst = lat[k & 1], lat[(k & 1) ^ 1]
            ade_calls.call(lib, "lbm_ring_ade_step_m", rg=ring, dst=dst, src=src, bc=GBC, prm=prm, sbc=sbc, iwalls=table, edge_rows=E)
        torch.cuda.synchronize()
    for j in range(2):
        assert_bits(owned(lat[steps & 1][j], sg), owned(want[j], gg), f"lattice {j}")
        assert not torch.equal(bits(owned(want[j], gg)), bits(owned(plain[j], gg)))
    table.close()


# ---- 6. LBM_MODEL_BGK through the `_m` calls --------------------------------------------------------------------------------
@FORMS
def test_model_bgk_through_the_m_calls_is_part_w_and_step_w(lib, form):
    """the bits of the whole allocation and the lbm_ade_part_launches count of lbm_ade_stream_collide_part_w /
    lbm_ring_ade_step_w"""
    R, C, E = 24, 64, 3
    bprm = bgk_params(form)
    mprm = (pylbm.AdeFluid(bprm[0]), bprm[1])
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO, col_lo=BB, col_hi=SP)
    sbc = pylbm.AdeScalarBC(row_lo=7e-4, col_hi=0.0)
    gg = geom(R + 1, C, 0)
    _, post = post_collision(lib, gg, pylbm.Bc(row_lo=BB, col_lo=BB, col_hi=SP), kbc.params(form))
    cut = [cut_slab(p, gg, 0, R, C + 6) for p in post]
    g, src = cut[0][0], (cut[0][1], cut[1][1])
    table = body_table(lib, R, C, RULE)
    count = lib.raw.lbm_ade_part_launches
    outs, launches = [], []
    for which_call in ("w", "m"):
        dst = (poisoned(g), poisoned(g))
        before = count()
        for which in (FRAME, INNER):
            if which_call == "w":
                ade_calls.part(lib, "_w", g, bc, bprm, dst, src, which, E, sbc=sbc, iwalls=table)
            else:
                ade_calls.part(lib, "_m", g, bc, mprm, dst, src, which, E, sbc=sbc, iwalls=table)
        torch.cuda.synchronize()
        outs.append(dst)
        launches.append(count() - before)
    assert launches == [4, 4], launches
    for k in range(2):
        assert bool(torch.isfinite(owned(outs[0][k], g)).all())
        assert_bits(outs[1][k], outs[0][k], f"part_m with a BGK fluid, lattice {k}")
    # the ring's step on a chain of one slab
    gbc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=SP)
    gg = geom(R, C, 0)
    _, post = post_collision(lib, gg, gbc, kbc.params(form))
    cut = [cut_slab(p, gg, 0, R, 0) for p in post]
    sg, src = cut[0][0], (cut[0][1], cut[1][1])
    outs, launches = [], []
    with OneSlabRing(lib, sg) as ring:
        for which_call in ("w", "m"):
            dst = (poisoned(sg), poisoned(sg))
            before = count()
            ade_calls.call(lib, "lbm_ring_ade_step_" + which_call, rg=ring, dst=dst, src=src, bc=gbc,
                           prm=bprm if which_call == "w" else mprm, sbc=sbc, iwalls=table, edge_rows=E)
            torch.cuda.synchronize()
            outs.append(dst)
            launches.append(count() - before)
    assert launches == [4, 4], launches
    for k in range(2):
        assert bool(torch.isfinite(owned(outs[0][k], sg)).all())
        assert_bits(outs[1][k], outs[0][k], f"ring_ade_step_m with a BGK fluid, lattice {k}")
    table.close()


# ---- 7. launch counts with KBC ---------------------------------------------------------------------------------------------
@FORMS
def test_a_part_is_one_launch_and_two_where_its_rows_hold_wall_nodes(lib, form):
    """never three: there is no edge pass, with wall edges and FIXED scalar edges too; a NULL or empty table adds none"""
    R, C, E = 24, 64, 3
    prm = kbc.params(form)
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO, col_lo=BB, col_hi=SP)
    sbc = pylbm.AdeScalarBC(row_lo=7e-4, col_hi=0.0)
    gg = geom(R + 1, C, 0)
    _, post = post_collision(lib, gg, pylbm.Bc(row_lo=BB, col_lo=BB, col_hi=SP), prm)
    cut = [cut_slab(p, gg, 0, R, 0) for p in post]
    g, src = cut[0][0], (cut[0][1], cut[1][1])
    empty = pylbm.AdeInteriorWalls(lib, R, C).finalize()
    none_here = pylbm.AdeInteriorWalls(lib, 48, C).add(40, 3, 0, 1, 5, ROW_NEG, ROW_NEG).slab(0, R).finalize()
    inner_only = pylbm.AdeInteriorWalls(lib, R, C).add(10, 20, 0, 1, 11, ROW_NEG, ROW_NEG).finalize()
    everywhere = body_table(lib, R, C, RULE)
    assert empty.count() == none_here.count() == 0 and bands_hold_nodes(everywhere, E)
    count = lib.raw.lbm_ade_part_launches
    got, outs = {}, {}
    for name, t in (("null", None), ("empty", empty), ("none_here", none_here), ("inner_only", inner_only), ("everywhere", everywhere)):
        dst = (poisoned(g), poisoned(g))
        per_part = []
        for which in (FRAME, INNER):
            before = count()
            ade_calls.part(lib, "_m", g, bc, prm, dst, src, which, E, sbc=sbc, iwalls=t)
            per_part.append(count() - before)
        torch.cuda.synchronize()
        got[name], outs[name] = per_part, dst
    assert got == dict(null=[1, 1], empty=[1, 1], none_here=[1, 1], inner_only=[1, 2], everywhere=[2, 2]), got
    for k in range(2):
        assert bool(torch.isfinite(owned(outs["null"][k], g)).all())
        for name in ("empty", "none_here"):
            assert_bits(outs[name][k], outs["null"][k], f"{name} table, lattice {k}")  # the whole allocation
        assert not torch.equal(bits(outs["everywhere"][k]), bits(outs["null"][k]))
    for t in (empty, none_here, inner_only, everywhere):
        t.close()


# ---- 8. graph capture ------------------------------------------------------------------------------------------------------
@FORMS
def test_a_captured_graph_of_frame_then_inner_replays_to_the_same_bits(lib, form):
    """both parts and both wall passes captured on ONE stream: the call allocates nothing and synchronises nothing"""
    R, C, E = 24, 64, 3
    prm = kbc.params(form)
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO, col_lo=BB, col_hi=SP)
    sbc = pylbm.AdeScalarBC(row_lo=7e-4, col_hi=0.0)
    gg = geom(R + 1, C, 0)
    _, post = post_collision(lib, gg, pylbm.Bc(row_lo=BB, col_lo=BB, col_hi=SP), prm)
    cut = [cut_slab(p, gg, 0, R, C + 6) for p in post]
    g, src = cut[0][0], (cut[0][1], cut[1][1])
    table = body_table(lib, R, C, RULE)
    want, dst = (poisoned(g), poisoned(g)), (poisoned(g), poisoned(g))
    ade_calls.both_parts(lib, "_m", g, bc, prm, want, src, E, sbc=sbc, iwalls=table)
    torch.cuda.synchronize()
    assert_finite(want, g, "the eager run")
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        lib.graph_begin_capture(st)
        ade_calls.both_parts(lib, "_m", g, bc, prm, dst, src, E, sbc=sbc, iwalls=table, s=st.value)
        lib.graph_end_capture(st, ct.byref(graph))
        for replay in range(2):
            for d in dst:
                bits(d).fill_(SENTINEL)
            torch.cuda.synchronize()
            lib.graph_launch(graph, 1, st)
            lib.stream_sync(st)
            for k in range(2):
                assert_bits(dst[k], want[k], f"replay {replay}, lattice {k}")  # the whole allocation: the same write set
    finally:
        if graph:
            lib.graph_destroy(graph)
        lib.stream_destroy(st)
    table.close()


# ---- 9. the driver ---------------------------------------------------------------------------------------------------------
DRIVER = ("--rows", 12, "--cols", 64, "--steps", 9, "--warmup", 2, "--fluid", "kbc", "--s2", 1.9, "--check", 1)


def assert_checked(line):
    """--check compares bit patterns, and equal NaNs are equal bits: the one block must be finite as well"""
    assert line["one_block_nonfinite"] == 0, line
    assert line["check"] == "bitwise equal to one block", line


@pytest.mark.parametrize("form", ["ref", "fast"])
@pytest.mark.parametrize("flags", [("--walls", 0), ("--walls", 1), ("--walls", 1, "--scalar-fixed", 1), ("--walls", 1, "--rectangle", 1)],
                         ids=["ring", "walls", "scalar_fixed", "rectangle"])
def test_slab_ring_ade_driver_emulated_chain_of_four_with_a_kbc_fluid(flags, form):
    line = last_json(run_driver("slab_ring_ade", "--emulate", 4, *DRIVER, *flags, "--form", form, timeout=120))
    assert_checked(line)
    assert line["slabs"] == 4 and line["message_rows_per_side"] == 6
    assert line["fluid"] == "kbc" and line["s2"] == 1.9 and line["form"] == form
    if "--rectangle" in flags:
        assert sum(1 for k in line["interior_wall_nodes_per_slab"] if k > 0) >= 2  # the body crosses a seam


def test_slab_ring_ade_driver_default_fluid_is_bgk():
    line = last_json(run_driver("slab_ring_ade", "--emulate", 2, "--rows", 12, "--cols", 64, "--steps", 3, "--warmup", 1,
                                "--omega", 1.3, "--check", 1, timeout=120))
    assert_checked(line)
    assert line["fluid"] == "bgk" and line["s2"] == 1.3


@pytest.mark.parametrize("walls", [0, 1])
def test_slab_ring_ade_driver_two_ranks_on_one_gpu_with_a_kbc_fluid(tmp_path, walls):
    """two forked rank processes sharing this GPU over the peer-mapped transport (lbm_ring_ade_collide_m /
    lbm_ring_ade_step_m): a closed ring, or a chain whose ends carry the walls"""
    line = last_json(run_driver("slab_ring_ade", "--spawn", 2, "--one-gpu", 1, "--transport", "ipc", *DRIVER, "--walls", walls,
                                "--id-file", tmp_path / "id", timeout=240, env=ipc_env()))
    assert_checked(line)
    assert line["n_gpus"] == 2 and line["fluid"] == "kbc"


@pytest.mark.parametrize("flags,word", [(("--buoyancy", "1e-3,0,0"), "--buoyancy"), (("--walls", 1, "--channel", 1), "--channel 1"),
                                        (("--walls", 1, "--rectangle", 1, "--exchange", 1), "--exchange 1")],
                         ids=["buoyancy", "channel", "exchange"])
def test_slab_ring_ade_driver_refuses_what_a_kbc_fluid_cannot_do(flags, word):
    r = run_driver("slab_ring_ade", "--emulate", 2, "--rows", 12, "--cols", 64, "--fluid", "kbc", *flags, timeout=60, check=False)
    assert r.returncode != 0
    assert f"{word} is not supported with --fluid kbc" in r.stderr, r.stderr
