"""GPU suite, the forced KBC collision (buoyancy) of the fluid + scalar step over row slabs and the ring:
lbm_ade_slab_stream_collide_mb (the buoyant part kernel of ade_kbc.hpp, k_ade_kbc_stream_collide_part_buoyant, + the
interior-wall pass of the part's rows), lbm_ring_ade_slab_collide_mb, lbm_ring_ade_slab_step_mb and the driver
slab_ring_benard.

The yardstick is one block: lbm_ade_collide_mb / lbm_ade_stream_collide_mb on the global lattice (pinned to the CPU
composition of the oracle's kbc::collide bit for bit in tests/test_gpu_ade_kbc_buoyancy.py), computed once per case, left
unchanged and asserted finite wherever it is used -- equal NaNs must not pass.  One chain is also tied to
ade_kbc_buoyancy_util.oracle_loop, which never calls the library.  Every comparison of lattices and moments is on bit
patterns, so there are no tolerances but the conservation test's.  s2 = 1.9, beta = (1.2e-2, -8e-3), u_shift = 1,
w = (3e-3, -2e-3); start states: ade_util.buoyant_initial_state.  The chain of slabs, the body and the write-set check of a
part are tests/ade_slab_util.py's; the three new entries are called through tests/ade_kbc_buoyancy_slab_calls.py, every other
raw call through tests/ade_calls.py; the rank processes run tests/ade_kbc_buoyancy_ring_rank.py."""
import ctypes as ct
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ade_calls  # noqa: E402
import ade_kbc_buoyancy_slab_calls as mb  # noqa: E402
import ade_kbc_buoyancy_util as yb  # noqa: E402
import ade_kbc_util as kbc  # noqa: E402
import pylbm  # noqa: E402
from ade_slab_util import (Chain, OneSlabRing, assert_finite, assert_part_write_sets, bands_hold_nodes, body_segments,  # noqa: E402
                           body_table, slab_bc)
from ade_util import (GBC, SENTINEL, alloc, assert_bits, bits, buoyant_initial_state, cut_slab, geom, moment_fields, owned,  # noqa: E402
                      poisoned, to_lattice)
from ade_util import params as bgk_params  # noqa: E402
from gpu_util import dev  # noqa: E402
from proc_util import ipc_env, last_json, run_driver, run_ranks  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FORMS = pytest.mark.parametrize("form", [REF, FAST], ids=["reference_order", "reassociated"])
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
BB, SP, HALO, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO, pylbm.EDGE_PERIODIC
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ROW_NEG = pylbm.ADE_FACE_ROW_NEG
S2, OMEGA_G, W = 1.9, kbc.OMEGA_G, (3e-3, -2e-3)
BETA, C_REF = (1.2e-2, -8e-3), 0.4
BY = pylbm.AdeBuoyancy(BETA, C_REF)  # u_shift = 1
ZERO = pylbm.AdeBuoyancy((0.0, 0.0), C_REF)


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(autouse=True)
def _default_knobs_afterwards(lib):
    yield
    lib.reset_tuning()


def params(form=REF):
    return kbc.params(form, s2=S2, w=W)


# ---- the one block ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _start(R, C, seed):
    from pyoracle import Oracle
    f, g = buoyant_initial_state(Oracle(), R, C, seed=seed, w=W)
    f.setflags(write=False)
    g.setflags(write=False)
    return f, g


def post_collision(lib, gg, gbc, prm, seed=None, buoy=BY):
    """(pre, post): ade_util.buoyant_initial_state on the lattice of gg and its post-collision pair, lbm_ade_collide_mb"""
    f, g = _start(gg.R, gg.C, gg.R * gg.C if seed is None else seed)
    pre = [to_lattice(f, gg), to_lattice(g, gg)]
    post = [alloc(gg), alloc(gg)]
    ade_calls.collide(lib, "_mb", gg, gbc, prm, post, pre, buoy=buoy)
    torch.cuda.synchronize()
    assert_finite(post, gg, "post-collision state")
    return pre, post


def one_block(lib, gg, gbc, prm, src, **kw):
    """lbm_ade_stream_collide_mb on every row -> (fn, gn), with BY unless the caller names another descriptor"""
    kw.setdefault("buoy", BY)
    return ade_calls.full_step(lib, "_mb", gg, gbc, prm, *src, **kw)


def profile(n, lo=1.5, hi=0.3):
    return torch.from_numpy(np.linspace(lo, hi, n)).to(dev())


def assert_moments(got, want, g, what, rows=None):
    """rho, the shifted u, C: dense fields of g.R rows against rows `rows` of the one block's"""
    for k, (name, planes) in enumerate((("rho", 1), ("u", 2), ("C", 1))):
        a = got[k].view(planes, g.R, g.C)
        b = want[k].view(planes, -1, g.C)
        b = b[:, rows[0]:rows[1]] if rows is not None else b
        assert bool(torch.isfinite(b).all()), f"{what}: the one block's {name} is not finite"
        assert_bits(a, b, f"{what} {name}")


# ---- 1. FRAME + INNER == lbm_ade_stream_collide_mb on one block ------------------------------------------------------------
GHOST0 = {"3x2": (3, 2, 0, (1,)), "16x16": (16, 16, 0, (1, 3, 7)), "3x1040": (3, 1040, 1056, (1,)), "48x1040": (48, 1040, 1056, (1, 8))}
EDGES = ["periodic", "box", "box_fixed"]


def box_fixed(R, C):
    """every wall edge of GBC FIXED, constants and profiles mixed"""
    return pylbm.AdeScalarBC(row_lo=0.7, row_hi=(0.0, profile(C, 0.2, 1.2)), col_lo=(0.0, profile(R)), col_hi=0.0)


@pytest.mark.parametrize("edges", EDGES)
@pytest.mark.parametrize("shape", list(GHOST0))
def test_frame_plus_inner_is_the_one_block_step_without_ghost_rows(lib, shape, edges):
    """ghost = 0 with PERIODIC rows and with BOUNCE_BACK rows, wall columns (bounce-back and specular), every edge of the
    scalar FIXED (constants and profiles); f, g and rho, the shifted u, C; with and without moments.  3 x 2: every row is an
    edge row"""
    R, C, pitch, Es = GHOST0[shape]
    g, prm = geom(R, C, 0, pitch), params()
    bc = pylbm.Bc() if edges == "periodic" else GBC
    sbc = box_fixed(R, C) if edges == "box_fixed" else None
    _, src = post_collision(lib, g, bc, prm)
    mw = moment_fields(g)
    want = one_block(lib, g, bc, prm, src, sbc=sbc, moments=mw)
    passive = ade_calls.full_step(lib, "_m", g, bc, prm, *src, sbc=sbc)
    torch.cuda.synchronize()
    assert_finite(want, g, shape)
    assert not torch.equal(bits(owned(want[0], g)), bits(owned(passive[0], g)))  # the scalar does push on the fluid
    for E in Es:
        for with_moments in (True, False):
            dst, mp = (alloc(g), alloc(g)), (moment_fields(g) if with_moments else None)
            mb.both_parts(lib, g, bc, prm, dst, src, E, sbc=sbc, buoy=BY, moments=mp)
            torch.cuda.synchronize()
            for k in range(2):
                assert_bits(owned(dst[k], g), owned(want[k], g), f"{shape} {edges} E={E} moments={with_moments} lattice {k}")
            if with_moments:
                assert_moments(mp, mw, g, f"{shape} {edges} E={E}")


HALOS = {"4x2": (4, 2, 0, (1,)), "16x16": (16, 16, 22, (1, 4)), "48x1040": (48, 1040, 1056, (1, 8))}


@pytest.mark.parametrize("walls", [0, 1, 2], ids=["periodic_columns", "wall_columns", "fixed_columns"])
@pytest.mark.parametrize("shape", list(HALOS))
def test_frame_plus_inner_is_the_one_blocks_rows_with_halo_rows(lib, shape, walls):
    """ghost = 1 with HALO rows: a slab of R rows cut from the middle of a global lattice of R + 2 rows, ghost rows from the
    global post-collision lattices; wall columns, the scalar FIXED on them (a profile's slice and a constant)"""
    R, C, pitch, Es = HALOS[shape]
    prm = params()
    gbc = pylbm.Bc(col_lo=BB if walls else PER, col_hi=SP if walls else PER)
    gg = geom(R + 2, C, 0)
    _, post = post_collision(lib, gg, gbc, prm)
    prof = profile(R + 2)
    gsbc = pylbm.AdeScalarBC(col_lo=(0.0, prof), col_hi=0.0) if walls == 2 else None
    sbc = pylbm.AdeScalarBC(col_lo=(0.0, prof[1:R + 1]), col_hi=0.0) if walls == 2 else None
    mw = moment_fields(gg)
    want = one_block(lib, gg, gbc, prm, post, sbc=gsbc, moments=mw)
    torch.cuda.synchronize()
    assert_finite(want, gg, shape)
    cut = [cut_slab(p, gg, 1, R + 1, pitch) for p in post]
    g, src = cut[0][0], (cut[0][1], cut[1][1])
    bc = pylbm.Bc(row_lo=HALO, row_hi=HALO, col_lo=gbc.col_lo, col_hi=gbc.col_hi)
    for E in Es:
        dst, mp = (alloc(g), alloc(g)), moment_fields(g)
        mb.both_parts(lib, g, bc, prm, dst, src, E, sbc=sbc, buoy=BY, moments=mp)
        torch.cuda.synchronize()
        for k in range(2):
            assert_bits(owned(dst[k], g), owned(want[k], gg)[:, 1:R + 1], f"{shape} walls={walls} E={E} lattice {k}")
        assert_moments(mp, mw, g, f"{shape} walls={walls} E={E}", rows=(1, R + 1))


@pytest.mark.parametrize("nt", [0, 1, 2, 3])
@pytest.mark.parametrize("grid_cap", [0, 7])
def test_every_launch_variant(lib, nt, grid_cap):
    """ "nt" x "grid_cap" on 48 x 1040 (three tiles per row, the last partial; a capped grid strides over 192 items) with
    walls all round, FIXED edges and moments"""
    R, C, pitch, E = 48, 1040, 1056, 5
    g, prm = geom(R, C, 0, pitch), params()
    sbc = box_fixed(R, C)
    _, src = post_collision(lib, g, GBC, prm)
    mw = moment_fields(g)
    want = one_block(lib, g, GBC, prm, src, sbc=sbc, moments=mw)  # default knobs
    torch.cuda.synchronize()
    assert_finite(want, g, "one block")
    lib.set_tuning(b"nt", nt)
    lib.set_tuning(b"grid_cap", grid_cap)
    dst, mp = (alloc(g), alloc(g)), moment_fields(g)
    mb.both_parts(lib, g, GBC, prm, dst, src, E, sbc=sbc, buoy=BY, moments=mp)
    torch.cuda.synchronize()
    for k in range(2):
        assert_bits(owned(dst[k], g), owned(want[k], g), f"nt={nt} grid_cap={grid_cap} lattice {k}")
    assert_moments(mp, mw, g, f"nt={nt} grid_cap={grid_cap}")


# ---- 2. each part alone writes exactly its rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("walls", [0, 1])
@pytest.mark.parametrize("R,C,pitch,E", [(48, 1040, 1056, 8), (6, 8, 18, 1)], ids=["48x1040_padded", "6x8"])
def test_each_part_alone_writes_exactly_its_rows(lib, walls, R, C, pitch, E):
    """NaN-poisoned targets on a ghost-1 slab cut from a global lattice of R + 2 rows: FRAME writes the edge bands only, INNER
    the rest; ghost rows, row-pitch padding and plane padding stay untouched, and every written double is the one FRAME +
    INNER write together"""
    prm = params()
    bc = pylbm.Bc(row_lo=HALO, row_hi=HALO, col_lo=BB if walls else PER, col_hi=SP if walls else PER)
    gg = geom(R + 2, C, 0)
    _, post = post_collision(lib, gg, pylbm.Bc(col_lo=bc.col_lo, col_hi=bc.col_hi), prm)
    cut = [cut_slab(p, gg, 1, R + 1, pitch) for p in post]
    g, src = cut[0][0], (cut[0][1], cut[1][1])
    want = (alloc(g), alloc(g))
    mb.both_parts(lib, g, bc, prm, want, src, E, buoy=BY)
    torch.cuda.synchronize()
    assert_finite(want, g, "FRAME + INNER")
    assert_part_write_sets(lambda dst, which: mb.part(lib, g, bc, prm, dst, src, which, E, buoy=BY), g, want, E,
                           f"{R}x{C} E={E} walls={walls}")


# ---- 3. emulated chains and closed rings -----------------------------------------------------------------------------------
def end_edges(r0, r1, Rg, prof):
    """the scalar's FIXED edges of the slab of global rows [r0, r1): the row edges where the slab keeps them (the chain's
    ends), column 0 the profile's slice, column C - 1 absorbing"""
    kw = dict(col_lo=(0.0, prof[r0:r1]), col_hi=0.0)
    if r0 == 0:
        kw["row_lo"] = 0.7
    if r1 == Rg:
        kw["row_hi"] = 0.1
    return pylbm.AdeScalarBC(**kw)


def chain(lib, gg, post, heights, closed, gbc, prm, per_slab=None, buoy=BY, moments=False):
    def advance(s, dst, src, e):
        if moments:
            s["moments"] = moment_fields(s["g"])
        mb.both_parts(lib, s["g"], s["bc"], prm, dst, src, e, sbc=s.get("sbc"), buoy=buoy, iwalls=s.get("view"),
                      moments=s.get("moments"))
    return Chain(lib, gg, post, heights, closed, gbc, advance, per_slab=per_slab)


CHAINS = {"closed_ring": ((3, 5, 4), 16, True), "box": ((3, 5, 4), 16, False), "fixed_ends": ((3, 5, 4), 16, False),
          "body_no_flux": ((16, 20, 12), 64, False), "body_fixed": ((16, 20, 12), 64, False), "one_slab": ((12,), 16, False)}


@pytest.mark.parametrize("case", list(CHAINS))
def test_emulated_chain_equals_one_block(lib, case):
    """slabs of uneven heights cut from a global lattice, after 1, 2 and 20 steps: a closed ring; a chain whose ends carry
    the box's walls; FIXED row edges at the chain's ends (and FIXED columns); the 68-node body across both seams with
    NO_FLUX and with FIXED slots; a chain of one slab"""
    heights, C, closed = CHAINS[case]
    prm, gbc = params(), (pylbm.Bc.periodic() if closed else GBC)
    Rg = sum(heights)
    gg = geom(Rg, C, 0)
    _, post = post_collision(lib, gg, gbc, prm)
    prof = profile(Rg)
    gsbc = end_edges(0, Rg, Rg, prof) if case == "fixed_ends" else None
    table = body_table(lib, Rg, C, (FIXED, 0.6) if case == "body_fixed" else (NO_FLUX, 0.0)) if case.startswith("body") else None
    if table is not None:
        assert table.count() == 68

    def per_slab(k, r0, r1, bc):
        d = {}
        if gsbc is not None:
            d["sbc"] = end_edges(r0, r1, Rg, prof)
        if table is not None:
            d["view"] = table.slab(r0, r1 - r0).finalize()
        return d

    ch = chain(lib, gg, post, heights, closed, gbc, prm, per_slab)
    if table is not None:
        assert sum(1 for s in ch.slabs if s["view"].count() > 0) == 3  # the body crosses both seams
    want, plain, done = [t.clone() for t in post], [t.clone() for t in post], 0
    for n in (1, 2, 20):
        for _ in range(n - done):
            want = list(one_block(lib, gg, gbc, prm, want, sbc=gsbc, iwalls=table))
            plain = list(one_block(lib, gg, gbc, prm, plain))
            ch.step(4)
        done = n
        torch.cuda.synchronize()
        assert_finite(want, gg, f"{n} steps")
        for j in range(2):
            assert_bits(ch.gather(j), owned(want[j], gg), f"{case}: slabs {heights} after {n} steps, lattice {j}")
    if gsbc is not None or table is not None:
        assert not torch.equal(bits(want[1]), bits(plain[1]))  # the walls of the case are felt
    ch.close()
    if table is not None:
        table.close()


@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
def test_emulated_chain_equals_the_oracle_loop(lib, oracle, closed):
    """3 + 5 + 4 rows x 16 after 2 steps against a yardstick that never calls the library: the pre-collision state through
    ade_kbc_buoyancy_util.oracle_loop on the CPU (2 iterations, each a forced collision and a stream), then collided once more
    for the post-collision pair the lattices hold"""
    heights, C, steps = (3, 5, 4), 16, 2
    prm, gbc = params(), (pylbm.Bc.periodic() if closed else GBC)
    gg = geom(sum(heights), C, 0)
    _, post = post_collision(lib, gg, gbc, prm)
    f0, g0 = _start(gg.R, C, gg.R * C)
    st = yb.oracle_loop(oracle, f0.copy(), g0.copy(), S2, OMEGA_G, W, steps, BY, gbc)
    assert yb.finite(st)
    c = yb.collide(oracle, st["f"], st["g"], S2, OMEGA_G, W, BY)
    assert np.all(np.isfinite(c["fc"])) and np.all(np.isfinite(c["gc"]))
    ch = chain(lib, gg, post, heights, closed, gbc, prm)
    for _ in range(steps):
        ch.step(4)
    torch.cuda.synchronize()
    for j, key in enumerate(("fc", "gc")):
        want = torch.from_numpy(np.ascontiguousarray(c[key].transpose(2, 0, 1))).to(dev())
        assert_bits(ch.gather(j), want, f"closed={closed} lattice {j} against the oracle loop")


# ---- 4. beta = (0, 0), a NULL descriptor and the form ----------------------------------------------------------------------
def slab_case(lib, prm, R=24, C=64, pitch=0, buoy=BY):
    """a ghost-1 slab with a wall row, a seam, wall columns, a FIXED row and column, and the body's table"""
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO, col_lo=BB, col_hi=SP)
    sbc = pylbm.AdeScalarBC(row_lo=0.7, col_hi=0.0)
    gg = geom(R + 1, C, 0)
    _, post = post_collision(lib, gg, pylbm.Bc(row_lo=BB, col_lo=BB, col_hi=SP), prm, buoy=buoy)
    cut = [cut_slab(p, gg, 0, R, pitch) for p in post]
    return cut[0][0], (cut[0][1], cut[1][1]), bc, sbc


@FORMS
def test_zero_beta_and_null_are_the_passive_part_m(lib, form):
    """the bits of the whole allocation and the lbm_ade_part_launches count of lbm_ade_stream_collide_part_m, in both forms"""
    R, C, E = 24, 64, 3
    prm = params(form)
    g, src, bc, sbc = slab_case(lib, prm, R, C, C + 6, buoy=None)
    table = body_table(lib, R, C, (FIXED, 0.6))
    count = lib.raw.lbm_ade_part_launches
    outs, launches = {}, {}
    for name, buoy in (("part_m", None), ("null", None), ("zero", ZERO)):
        dst = (poisoned(g), poisoned(g))
        before = count()
        if name == "part_m":
            ade_calls.both_parts(lib, "_m", g, bc, prm, dst, src, E, sbc=sbc, iwalls=table)
        else:
            mb.both_parts(lib, g, bc, prm, dst, src, E, sbc=sbc, buoy=buoy, iwalls=table)
        torch.cuda.synchronize()
        outs[name], launches[name] = dst, count() - before
    assert launches == dict(part_m=4, null=4, zero=4), launches
    for k in range(2):
        assert bool(torch.isfinite(owned(outs["part_m"][k], g)).all())
        for name in ("null", "zero"):
            assert_bits(outs[name][k], outs["part_m"][k], f"{name} descriptor, lattice {k}")


def test_a_buoyant_part_runs_the_reference_order_whatever_the_form(lib):
    R, C, E = 24, 64, 3
    g, src, bc, sbc = slab_case(lib, params(REF), R, C)
    outs = []
    for form in (REF, FAST, pylbm.FORM_DEFAULT):
        dst = (poisoned(g), poisoned(g))
        mb.both_parts(lib, g, bc, params(form), dst, src, E, sbc=sbc, buoy=BY)
        torch.cuda.synchronize()
        outs.append(dst)
    passive = (poisoned(g), poisoned(g))
    mb.both_parts(lib, g, bc, params(REF), passive, src, E, sbc=sbc, buoy=ZERO)
    torch.cuda.synchronize()
    for k in range(2):
        assert bool(torch.isfinite(owned(outs[0][k], g)).all())
        assert_bits(outs[1][k], outs[0][k], f"reassociated against reference order, lattice {k}")
        assert_bits(outs[2][k], outs[0][k], f"default form against reference order, lattice {k}")
    assert not torch.equal(bits(outs[0][0]), bits(passive[0]))


# ---- 5. LBM_MODEL_BGK through the new entries ------------------------------------------------------------------------------
@FORMS
def test_model_bgk_through_the_new_entries_is_part_w_and_step_w(lib, form):
    """the bits of the whole allocation and the launch count of lbm_ade_stream_collide_part_w / lbm_ring_ade_step_w with the
    same descriptor"""
    R, C, E = 24, 64, 3
    bprm = bgk_params(form, w=W)
    mprm = (pylbm.AdeFluid(bprm[0]), bprm[1])
    by = pylbm.AdeBuoyancy(BETA, C_REF, 0.5, (3.0, 9.0))
    g, src, bc, sbc = slab_case(lib, params(REF), R, C, C + 6)
    table = body_table(lib, R, C, (FIXED, 0.6))
    count = lib.raw.lbm_ade_part_launches
    outs, launches = [], []
    for which_call in ("w", "mb"):
        dst = (poisoned(g), poisoned(g))
        before = count()
        if which_call == "w":
            ade_calls.both_parts(lib, "_w", g, bc, bprm, dst, src, E, sbc=sbc, buoy=by, iwalls=table)
        else:
            mb.both_parts(lib, g, bc, mprm, dst, src, E, sbc=sbc, buoy=by, iwalls=table)
        torch.cuda.synchronize()
        outs.append(dst)
        launches.append(count() - before)
    assert launches == [4, 4], launches
    passive = (poisoned(g), poisoned(g))
    ade_calls.both_parts(lib, "_w", g, bc, bprm, passive, src, E, sbc=sbc, iwalls=table)
    torch.cuda.synchronize()
    for k in range(2):
        assert bool(torch.isfinite(owned(outs[0][k], g)).all())
        assert_bits(outs[1][k], outs[0][k], f"slab_stream_collide_mb with a BGK fluid, lattice {k}")
    assert not torch.equal(bits(outs[0][0]), bits(passive[0]))  # the descriptor arrives
    # the ring's step on a chain of one slab
    gbc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=SP)
    gg = geom(R, C, 0)
    _, post = post_collision(lib, gg, gbc, params(REF))
    cut = [cut_slab(p, gg, 0, R, 0) for p in post]
    sg, src = cut[0][0], (cut[0][1], cut[1][1])
    outs, launches = [], []
    with OneSlabRing(lib, sg) as ring:
        for which_call in ("w", "mb"):
            dst = (poisoned(sg), poisoned(sg))
            before = count()
            if which_call == "w":
                ade_calls.call(lib, "lbm_ring_ade_step_w", rg=ring, dst=dst, src=src, bc=gbc, prm=bprm, sbc=sbc, buoy=by,
                               iwalls=table, edge_rows=E)
            else:
                mb.call(lib, mb.RING_STEP, rg=ring, dst=dst, src=src, bc=gbc, prm=mprm, sbc=sbc, buoy=by, iwalls=table, edge_rows=E)
            torch.cuda.synchronize()
            outs.append(dst)
            launches.append(count() - before)
    assert launches == [4, 4], launches
    for k in range(2):
        assert bool(torch.isfinite(owned(outs[0][k], sg)).all())
        assert_bits(outs[1][k], outs[0][k], f"ring_ade_slab_step_mb with a BGK fluid, lattice {k}")
    table.close()


def test_ring_entries_on_a_chain_of_one_slab_are_the_one_block(lib):
    """lbm_ring_ade_slab_collide_mb, then 3 x lbm_ring_ade_slab_step_mb with the body, a FIXED row, a FIXED profile column
    and an absorbing column: nothing travels, both parts run on `main`"""
    R, C, E, steps = 34, 64, 2, 3
    prm = params()
    sbc = pylbm.AdeScalarBC(row_lo=0.7, col_lo=(0.0, profile(R)), col_hi=0.0)
    table = body_table(lib, R, C, (FIXED, 0.6))
    assert bands_hold_nodes(table, E)
    gg = geom(R, C, 0)
    pre, want = post_collision(lib, gg, GBC, prm)
    cut = [cut_slab(t, gg, 0, R, 0) for t in pre]  # ghost rows poisoned: beyond a wall nothing may read them
    sg = cut[0][0]
    lat = [[alloc(sg), alloc(sg)], [alloc(sg), alloc(sg)]]
    for _ in range(steps):
        want = one_block(lib, gg, GBC, prm, want, sbc=sbc, iwalls=table)
    torch.cuda.synchronize()
    assert_finite(want, gg, "one block")
    with OneSlabRing(lib, sg) as ring:
        mb.call(lib, mb.RING_COLLIDE, rg=ring, dst=lat[0], src=(cut[0][1], cut[1][1]), bc=GBC, prm=prm, sbc=sbc, buoy=BY)
        for k in range(steps):
            src, dst = lat[k & 1], lat[(k & 1) ^ 1]
            mb.call(lib, mb.RING_STEP, rg=ring, dst=dst, src=src, bc=GBC, prm=prm, sbc=sbc, buoy=BY, iwalls=table, edge_rows=E)
        torch.cuda.synchronize()
    for j in range(2):
        assert_bits(owned(lat[steps & 1][j], sg), owned(want[j], gg), f"lattice {j}")
    table.close()


# ---- 6. launch counts and graph capture ------------------------------------------------------------------------------------
def test_a_part_is_one_launch_and_two_where_its_rows_hold_wall_nodes(lib):
    """never three: there is no edge pass, with wall edges and FIXED scalar edges too; a NULL or empty table adds none"""
    R, C, E = 24, 64, 3
    prm = params()
    g, src, bc, sbc = slab_case(lib, prm, R, C)
    empty = pylbm.AdeInteriorWalls(lib, R, C).finalize()
    none_here = pylbm.AdeInteriorWalls(lib, 48, C).add(40, 3, 0, 1, 5, ROW_NEG, ROW_NEG).slab(0, R).finalize()
    inner_only = pylbm.AdeInteriorWalls(lib, R, C).add(10, 20, 0, 1, 11, ROW_NEG, ROW_NEG).finalize()
    everywhere = body_table(lib, R, C, (FIXED, 0.6))
    assert empty.count() == none_here.count() == 0 and bands_hold_nodes(everywhere, E)
    count = lib.raw.lbm_ade_part_launches
    got, outs = {}, {}
    for name, t in (("null", None), ("empty", empty), ("none_here", none_here), ("inner_only", inner_only), ("everywhere", everywhere)):
        dst = (poisoned(g), poisoned(g))
        per_part = []
        for which in (FRAME, INNER):
            before = count()
            mb.part(lib, g, bc, prm, dst, src, which, E, sbc=sbc, buoy=BY, iwalls=t)
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


def test_a_captured_graph_replays_to_the_same_bits_and_keeps_its_descriptor(lib):
    """both parts and both wall passes captured on ONE stream: the call allocates nothing and synchronises nothing; the
    descriptor is changed after the capture, and the replays still give the bits of the captured one"""
    R, C, E = 24, 64, 3
    prm = params()
    g, src, bc, sbc = slab_case(lib, prm, R, C, C + 6)
    table = body_table(lib, R, C, (FIXED, 0.6))
    want, other, dst = (poisoned(g), poisoned(g)), (poisoned(g), poisoned(g)), (poisoned(g), poisoned(g))
    by = pylbm.AdeBuoyancy(BETA, C_REF)
    mb.both_parts(lib, g, bc, prm, want, src, E, sbc=sbc, buoy=by, iwalls=table)
    mb.both_parts(lib, g, bc, prm, other, src, E, sbc=sbc, buoy=pylbm.AdeBuoyancy((-3e-2, 2e-2), 0.1), iwalls=table)
    torch.cuda.synchronize()
    assert_finite(want, g, "the eager run")
    assert not torch.equal(bits(want[0]), bits(other[0]))
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        lib.graph_begin_capture(st)
        mb.both_parts(lib, g, bc, prm, dst, src, E, sbc=sbc, buoy=by, iwalls=table, s=st.value)
        lib.graph_end_capture(st, ct.byref(graph))
        by.beta_r, by.beta_c, by.c_ref = -3e-2, 2e-2, 0.1  # the caller's descriptor changes: the graph holds a copy
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


# ---- 7. rank processes (tests/ade_kbc_buoyancy_ring_rank.py) ---------------------------------------------------------------
def one_block_after(lib, gg, gbc, prm, post, counts, table=None):
    """{n: the lattices after n steps of lbm_ade_stream_collide_mb from the post-collision pair}"""
    out, cur, done = {}, [t.clone() for t in post], 0
    for n in counts:
        for _ in range(n - done):
            cur = list(one_block(lib, gg, gbc, prm, cur, iwalls=table))
        done = n
        torch.cuda.synchronize()
        assert_finite(cur, gg, f"one block after {n} steps")
        out[n] = cur
    return out


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("closed", [True, False], ids=["closed_ring", "walled_chain"])
def test_ring_of_rank_processes_equals_one_block(lib, tmp_path, n, closed):
    """n ranks sharing this GPU on the peer-mapped transport through lbm_ring_ade_slab_collide_mb / lbm_ring_ade_slab_step_mb,
    with a wall node on every seam row: the wall pass of the FRAME rows runs before the pack.  Equal to one block after 1, 2
    and 9 steps"""
    R, C, E, counts = 12, 32, 2, (1, 2, 9)
    rule = (FIXED, 0.6)
    prm, gbc = params(), (pylbm.Bc.periodic() if closed else GBC)
    gg = geom(R * n, C, 0)
    pre, post = post_collision(lib, gg, gbc, prm)
    table = body_table(lib, R * n, C, rule)
    rows = {nd["r"] for nd in table.nodes()}
    assert all(k * R in rows and k * R + R - 1 in rows for k in range(n))  # a wall node on every seam row
    want = one_block_after(lib, gg, gbc, prm, post, counts, table)
    plain = one_block_after(lib, gg, gbc, prm, post, counts)
    assert not torch.equal(bits(want[9][1]), bits(plain[9][1]))
    cfg = dict(R=R, C=C, steps=list(counts), edge_rows=E, closed=int(closed), form=REF, bc=bytes(gbc).hex(), w=list(W), s2=S2,
               omega_g=OMEGA_G, buoy=[BY.beta_r, BY.beta_c, BY.c_ref, BY.u_shift], segments=body_segments(R * n), g_mode=rule[0],
               conc=rule[1])
    outs = run_ranks(lib, tmp_path, "ade_kbc_buoyancy_ring_rank.py", n, cfg,
                     dict(f0=owned(pre[0], gg).cpu().numpy(), g0=owned(pre[1], gg).cpu().numpy()), timeout=240)
    for steps in counts:
        for j, key in enumerate(("f", "g")):
            got = np.concatenate([o[f"{key}_{steps}"] for o in outs], axis=1)
            ref = owned(want[steps][j], gg).cpu().numpy()
            assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"{n} ranks closed={closed} after {steps}: {key} differs"
    assert sum(int(o["nodes"]) for o in outs) == table.count() and all(int(o["nodes"]) > 0 for o in outs)
    table.close()


# ---- 8. conservation over a chain ------------------------------------------------------------------------------------------
def slab_diag(lib, ch, gg, prm, E):
    """the diagnostics of the streamed state the chain's lattices lead to, slab by slab: one passive reference-order part step
    per slab into scratch lattices for its moments (rho, the UNSHIFTED u = calc_u(f, rho), C -- what lbm_ade_solver_diag
    forms), lbm_diag_rows into the slab's rows of ONE global table, lbm_diag_fold over all of them"""
    NQ = pylbm.DIAG_NQ
    table = torch.zeros(NQ * gg.R, dtype=torch.float64, device=dev())
    for s in ch.slabs:
        g = s["g"]
        m, scratch = moment_fields(g), (alloc(g), alloc(g))
        ade_calls.both_parts(lib, "_m", g, s["bc"], prm, scratch, s["lat"][ch.cur], min(E, (g.R - 1) // 2), moments=m)
        lib.diag_rows(pylbm._ptr(table), gg.R, s["r0"], pylbm._ptr(m[0]), pylbm._ptr(m[1]), pylbm._ptr(m[2]), None, g.R, g.C, 0, g.R, None)
    out = torch.zeros(NQ, dtype=torch.float64, device=dev())
    lib.diag_fold(pylbm._ptr(out), pylbm._ptr(table), gg.R, 0, gg.R, None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_mass_and_momentum_over_a_chain_of_three_slabs(lib):
    """a closed ring of 3 + 5 + 4 rows x 16, 20 iterations (the collide-only one, then 19 steps): the per-slab lbm_diag_rows
    folds are bitwise lbm_ade_solver_diag of the one-block context after the same iterations; the mass is unchanged (to
    1e-13, the one-block test's bound) and the momentum grows by the sum over the iterations of sum rho u_shift F, rho and C
    those the slabs' own moment outputs report.  The bound on the momentum is the one-block test's
    (tests/test_gpu_ade_kbc_buoyancy.py: 1e-12 relative over 50 steps) scaled by the steps: 4e-13.  Measured on an MI355X:
    4.4e-16 and 2.2e-16 (two ulps and one of the sums -13.54 and 9.03), the mass 191.83338451894647 before and after"""
    heights, C, E, iterations = (3, 5, 4), 16, 4, 20
    prm, gbc = params(), pylbm.Bc.periodic()
    Rg = sum(heights)
    gg = geom(Rg, C, 0)
    f0, g0 = _start(Rg, C, Rg * C)
    sv = pylbm.AdeSolver(lib, Rg, C, pylbm.KbcParams(S2, REF), pylbm.AdeParams(OMEGA_G, W, form=REF), bc=gbc, buoyancy=BY)
    try:
        sv.set_state(f0, g0)
        first = sv.diag()
        sv.step(iterations)
        last = sv.diag()
    finally:
        sv.close()
    assert first[pylbm.DIAG_NONFINITE] == 0.0 and last[pylbm.DIAG_NONFINITE] == 0.0
    assert np.all(np.isfinite(first)) and np.all(np.isfinite(last))
    pre = [to_lattice(f0, gg), to_lattice(g0, gg)]
    post, m0 = [alloc(gg), alloc(gg)], moment_fields(gg)
    ade_calls.collide(lib, "_mb", gg, gbc, prm, post, pre, buoy=BY, moments=m0)
    torch.cuda.synchronize()
    assert_finite(post, gg, "post-collision state")
    added = np.zeros(2)

    def add(rho, conc):
        rho, conc = rho.cpu().numpy(), conc.cpu().numpy()
        added[:] += [float(np.sum(rho * (BY.u_shift * (beta * (conc - C_REF))))) for beta in BETA]

    add(m0[0], m0[2])
    ch = chain(lib, gg, post, heights, True, gbc, prm, moments=True)
    for _ in range(iterations - 1):
        ch.step(E)
        torch.cuda.synchronize()
        for s in ch.slabs:
            add(s["moments"][0], s["moments"][2])
    got = slab_diag(lib, ch, gg, prm, E)
    assert np.array_equal(got.view(np.uint64), np.asarray(last).view(np.uint64)), (got, last)
    SUM_RHO, SUM_MR, SUM_MC = pylbm.DIAG_SUM_RHO, pylbm.DIAG_SUM_MR, pylbm.DIAG_SUM_MC
    grown = np.array([got[SUM_MR] - first[SUM_MR], got[SUM_MC] - first[SUM_MC]])
    print(f"momentum grown by {grown!r}, sum of rho u_shift F {added!r}, relative {np.abs(grown / added - 1)!r}; "
          f"mass {first[SUM_RHO]!r} -> {got[SUM_RHO]!r}")
    assert np.all(np.abs(grown - added) <= 1e-12 * iterations / 50 * np.abs(added)), (grown, added)
    assert abs(got[SUM_RHO] - first[SUM_RHO]) <= 1e-13 * first[SUM_RHO]


# ---- 9. the driver ---------------------------------------------------------------------------------------------------------
def benard_flags(fluid):
    return ("--fluid", fluid, "--s2" if fluid == "kbc" else "--omega", 1.9 if fluid == "kbc" else 1.4, "--omega-g", 1.3, "--ra", 5000.0)


def assert_checked(line):
    """--check compares bit patterns, and equal NaNs are equal bits: the one block must be finite as well"""
    assert line["one_block_nonfinite"] == 0, line
    assert line["check"] == "bitwise equal to one block", line
    assert line["nonfinite"] == 0, line


def rayleigh_benard(fluid, rows, cols, iterations):
    """the JSON line of drivers/rayleigh_benard (lbm_ade_solver on one block) for the same box and iterations"""
    return last_json(run_driver("rayleigh_benard", *benard_flags(fluid), "--rows", rows, "--cols", cols, "--steps", iterations, timeout=120))


@pytest.mark.parametrize("fluid", ["kbc", "bgk"])
def test_slab_ring_benard_emulated_chain_of_four(fluid):
    """4 slabs of 6 x 64: --check against one block, and nusselt and max_u -- from lbm_diag_rows per slab, folded -- equal to
    those rayleigh_benard prints for the 24 x 64 box after the same iterations, digit for digit (the JSON numbers are
    written with 17 significant digits: equal numbers are equal doubles)"""
    line = last_json(run_driver("slab_ring_benard", "--emulate", 4, "--rows", 6, "--cols", 64, "--steps", 9, "--warmup", 2, "--check", 1,
                                *benard_flags(fluid), timeout=120))
    assert_checked(line)
    assert line["slabs"] == 4 and line["global_rows"] == 24 and line["iterations"] == 12 and line["fluid"] == fluid
    one = rayleigh_benard(fluid, 24, 64, line["iterations"])
    assert one["nonfinite"] == 0 and one["beta"] == line["beta"] and (one["u_shift"], one["guo"]) == (line["u_shift"], line["guo"])
    print(f"{fluid}: nusselt {line['nusselt']!r} / {one['nusselt']!r}, max_u {line['max_u']!r} / {one['max_u']!r}")
    assert line["nusselt"] == one["nusselt"], (line["nusselt"], one["nusselt"])
    assert line["max_u"] == one["max_u"] and one["max_u"] > 0.0, (line["max_u"], one["max_u"])


@pytest.mark.parametrize("fluid", ["kbc", "bgk"])
def test_slab_ring_benard_two_ranks_on_one_gpu(tmp_path, fluid):
    """two forked rank processes sharing this GPU over the peer-mapped transport (lbm_ring_ade_slab_collide_mb /
    lbm_ring_ade_slab_step_mb): a chain whose end slabs carry the plates; the row tables gathered and folded on the host"""
    line = last_json(run_driver("slab_ring_benard", "--spawn", 2, "--one-gpu", 1, "--transport", "ipc", "--rows", 6, "--cols", 64,
                                "--steps", 9, "--warmup", 2, "--check", 1, *benard_flags(fluid), "--id-file", tmp_path / "id",
                                timeout=240, env=ipc_env()))
    assert_checked(line)
    assert line["n_gpus"] == 2 and line["fluid"] == fluid and line["global_rows"] == 12
    one = rayleigh_benard(fluid, 12, 64, line["iterations"])
    assert line["nusselt"] == one["nusselt"] and line["max_u"] == one["max_u"], (line, one)
