"""GPU suite, the fluid + scalar step over row slabs: lbm_ade_stream_collide_part (FRAME / INNER, one dispatch each,
wall fix-ups inline), lbm_ring_ade_collide / lbm_ring_ade_step / lbm_ring_exchange_pair and the slab_ring_ade driver.

The yardstick is one block: lbm_ade_stream_collide on the global lattice (pinned to the reference loop bit for bit in
tests/test_gpu_ade.py).  Post-collision f and g are compared BITWISE on every owned node:
  * FRAME + INNER == the full step, on single blocks and on ghost-1 slabs cut from the global lattice;
  * each part alone writes exactly its rows, nothing of the ghost rows or the padding (NaN-poisoned destinations);
  * chains / rings of 2..4 slabs, the one-row halos of both lattices moved by ade_slab_util.Chain, == one block;
  * real rank processes over the peer-mapped transport (tests/ade_ring_rank.py) == one block;
  * the driver's own --check; and the scalar's mass and transport across the seams.
The chain of slabs, the edges of a slab and the write-set check of a part are tests/ade_slab_util.py's; every raw call goes
through tests/ade_calls.py with the suffix-less entries."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
import ade_calls  # noqa: E402
from ade_slab_util import Chain, OneSlabRing, assert_part_write_sets, global_state, slab_bc  # noqa: E402
from ade_util import GBC, W, alloc, assert_bits, cut_slab, geom, owned, params, random_lattice  # noqa: E402
from gpu_util import dev  # noqa: E402
from proc_util import last_json, run_driver, run_ranks  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
BB, SP, HALO, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO, pylbm.EDGE_PERIODIC


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


def wall_bc(walls):
    return pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=SP) if walls else pylbm.Bc.periodic()


def pitch_of(C):
    return C + 16 if C >= 1024 else 0  # 1040 columns: a padded row pitch


# every call of this suite goes through the suffix-less entry points
def chain(lib, gg, post, heights, closed, gbc, prm):
    return Chain(lib, gg, post, heights, closed, gbc,
                 lambda s, dst, src, e: ade_calls.both_parts(lib, "", s["g"], s["bc"], prm, dst, src, e))


# ---- 1. FRAME + INNER == the full step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST])
@pytest.mark.parametrize("walls", [0, 1])
def test_frame_plus_inner_is_the_full_step_on_one_block(lib, form, walls):
    prm, bc = params(form), wall_bc(walls)
    for R in (64, 130, 257):
        for C in (96, 200, 1040):
            g = geom(R, C, 0, pitch_of(C))
            src = (random_lattice(g, R + C), random_lattice(g, R * C))
            want = ade_calls.full_step(lib, "", g, bc, prm, *src)
            for E in (1, 3, 16, 40):
                if 2 * E >= R:
                    continue
                dst = (alloc(g), alloc(g))
                ade_calls.part(lib, "", g, bc, prm, dst, src, FRAME, E)
                ade_calls.part(lib, "", g, bc, prm, dst, src, INNER, E)
                torch.cuda.synchronize()
                for k in range(2):
                    assert_bits(owned(dst[k], g), owned(want[k], g), f"R={R} C={C} E={E} walls={walls} lattice {k}")


@pytest.mark.parametrize("form", [REF, FAST])
@pytest.mark.parametrize("walls", [0, 1])
def test_frame_plus_inner_on_slabs_cut_from_the_global_lattice(lib, form, walls):
    """ghost-1 slabs (HALO on one or both sides, the global walls on a chain end) == the global step on their rows"""
    prm, gbc = params(form), wall_bc(walls)
    for R in (64, 130, 257):
        for C in (96, 200, 1040):
            gg = geom(R, C, 0, pitch_of(C))
            src = (random_lattice(gg, R + 7 * C), random_lattice(gg, 3 * R + C))
            want = ade_calls.full_step(lib, "", gg, gbc, prm, *src)
            h = R // 2
            for r0, r1 in ((0, h), (h, R), (R // 4, R // 4 + h)):
                bc = slab_bc(gbc, r0, r1, R, not walls)
                slab = [cut_slab(s, gg, r0, r1, pitch_of(C), not walls) for s in src]
                sg = slab[0][0]
                for E in (1, 3, 16, 40):
                    if 2 * E >= sg.R:
                        continue
                    dst = (alloc(sg), alloc(sg))
                    ade_calls.part(lib, "", sg, bc, prm, dst, (slab[0][1], slab[1][1]), FRAME, E)
                    ade_calls.part(lib, "", sg, bc, prm, dst, (slab[0][1], slab[1][1]), INNER, E)
                    torch.cuda.synchronize()
                    for k in range(2):
                        assert_bits(owned(dst[k], sg), owned(want[k], gg)[:, r0:r1],
                                    f"R={R} C={C} slab [{r0}, {r1}) E={E} walls={walls} lattice {k}")


# ---- 2. write sets -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,E", [(64, 96, 1), (64, 96, 16), (130, 200, 3), (130, 1040, 40), (50, 200, 16),
                                   (57, 96, 28), (131, 200, 64), (33, 96, 5)])
@pytest.mark.parametrize("walls", [0, 1])
def test_each_part_alone_writes_exactly_its_rows(lib, R, C, E, walls):
    """NaN-poisoned destinations, ghost rows and row / plane padding included: the changed doubles of both lattices in
    all 9 planes are exactly the part's rows, each bit-equal to the full-range call"""
    assert 2 * E < R
    prm = params(FAST)
    # a chain-end slab with walls (bounce-back row 0, wall columns) or a middle slab (HALO both sides)
    bc = pylbm.Bc(row_lo=BB if walls else HALO, row_hi=HALO, col_lo=BB if walls else PER, col_hi=SP if walls else PER)
    g = geom(R, C, 1, pitch_of(C))
    src = (random_lattice(g, R), random_lattice(g, C))
    want = [alloc(g), alloc(g)]
    ade_calls.part(lib, "", g, bc, prm, want, src, FRAME, E)
    ade_calls.part(lib, "", g, bc, prm, want, src, INNER, E)
    assert_part_write_sets(lambda dst, which: ade_calls.part(lib, "", g, bc, prm, dst, src, which, E), g, want, E,
                           f"R={R} C={C} E={E} walls={walls}")


# ---- 3. chains and rings of slabs in one process -------------------------------------------------------------------------
def one_block(lib, gg, pre, gbc, prm, steps):
    """lbm_ade_collide + `steps` x lbm_ade_stream_collide on the global lattice: (post-collision state, after steps)"""
    post = [alloc(gg), alloc(gg)]
    ade_calls.collide(lib, "", gg, gbc, prm, post, pre)
    cur = [t.clone() for t in post]
    for _ in range(steps):
        cur = list(ade_calls.full_step(lib, "", gg, gbc, prm, *cur))
    torch.cuda.synchronize()
    return post, cur


@pytest.mark.parametrize("form", [REF, FAST])
@pytest.mark.parametrize("closed", [True, False])
@pytest.mark.parametrize("heights,C", [((64, 64), 96), ((48, 48, 48), 200), ((40, 40, 40, 40), 96), ((50, 130), 200),
                                       ((130, 50, 130), 200)])
def test_emulated_chain_equals_one_block(lib, oracle, form, closed, heights, C):
    prm, gbc = params(form), (pylbm.Bc.periodic() if closed else wall_bc(True))
    Rg, steps = sum(heights), 53
    gg, pre = global_state(oracle, Rg, C)
    post, want = one_block(lib, gg, pre, gbc, prm, steps)
    ch = chain(lib, gg, post, heights, closed, gbc, prm)
    for _ in range(steps):
        ch.step(16)
    torch.cuda.synchronize()
    for j in range(2):
        assert_bits(ch.gather(j), owned(want[j], gg), f"{len(heights)} slabs {heights} closed={closed} lattice {j}")


# ---- 4. real rank processes (tests/ade_ring_rank.py, entry "plain") ------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("closed", [True, False])
def test_ring_of_rank_processes_equals_one_block(lib, oracle, tmp_path, n, closed):
    R, C, steps, form = 48, 200, 31, FAST
    prm, gbc = params(form), (pylbm.Bc.periodic() if closed else wall_bc(True))
    gg, pre = global_state(oracle, R * n, C, seed=n)
    _, want = one_block(lib, gg, pre, gbc, prm, steps)
    cfg = dict(R=R, C=C, steps=[steps], edge_rows=16, closed=int(closed), form=form, bc=bytes(gbc).hex(), w=list(W),
               entry="plain")
    outs = run_ranks(lib, tmp_path, "ade_ring_rank.py", n, cfg,
                     dict(f0=owned(pre[0], gg).cpu().numpy(), g0=owned(pre[1], gg).cpu().numpy()), timeout=240)
    for j, key in enumerate(("f", "g")):
        got = np.concatenate([o[f"{key}_{steps}"] for o in outs], axis=1)
        ref = owned(want[j], gg).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), f"{n} ranks closed={closed}: {key} differs"
    # refresh after a restore (lbm_ring_exchange_pair) is checked by the ranks themselves: ghost rows == neighbours' rows
    assert all(bool(o["pair_ok"]) for o in outs)


def test_ring_entry_points_refuse_a_ring_without_one_ghost_row(lib, tmp_path):
    """ghost != 1 on the ring: every ring entry point of the pair refuses it on the host (one rank, its own process)"""
    cfg = dict(case="refusals", entry="plain", R=32, C=64)
    outs = run_ranks(lib, tmp_path, "ade_ring_rank.py", 1, cfg, {}, timeout=240)
    msgs = json.loads(str(outs[0]["msgs"]))
    assert len(msgs) == 3
    for m in msgs:
        assert "ghost=2" in m, m


def test_ring_step_with_walls_fixed_edges_and_buoyancy_is_the_one_block_step(lib):
    """a ring of one rank in this process, not closed -- a chain of one slab: its rows keep their walls, nothing travels.
    lbm_ring_ade_step_b with a FIXED row, a FIXED profile column and buoyancy (FRAME and INNER launched from one resolved
    call) == lbm_ade_stream_collide_b on the same block after 3 steps, bit for bit"""
    R, C, E, steps = 34, 64, 2, 3
    prm = params(FAST)
    by = pylbm.AdeBuoyancy((2e-2, -1e-2), 1.0, 0.5, (3.0, 9.0))  # random_lattice: C ~ 1.0 .. 1.05
    prof = torch.from_numpy(np.linspace(0.9, 1.1, R)).to(dev())
    sbc = pylbm.AdeScalarBC(row_lo=1.02, col_lo=(0.0, prof), col_hi=0.0)
    gg = geom(R, C, 0)
    want = [random_lattice(gg, 1), random_lattice(gg, 2)]
    cut = [cut_slab(t, gg, 0, R, 0) for t in want]  # ghost rows poisoned: beyond a wall nothing may read them
    sg = cut[0][0]
    lat = [[cut[0][1], cut[1][1]], [alloc(sg), alloc(sg)]]
    for _ in range(steps):
        want = ade_calls.full_step(lib, "_b", gg, GBC, prm, *want, sbc=sbc, buoy=by)
    with OneSlabRing(lib, sg) as ring:
        for k in range(steps):
            ade_calls.call(lib, "lbm_ring_ade_step_b", rg=ring, dst=lat[(k & 1) ^ 1], src=lat[k & 1], bc=GBC, prm=prm, sbc=sbc,
                           buoy=by, edge_rows=E)
        torch.cuda.synchronize()
    for j in range(2):
        assert_bits(owned(lat[steps & 1][j], sg), owned(want[j], gg), f"lattice {j}")


# ---- 5. the driver -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walls", [0, 1])
@pytest.mark.parametrize("form", ["fast", "ref"])
def test_slab_ring_ade_driver_emulated_chain_of_four(walls, form):
    line = last_json(run_driver("slab_ring_ade", "--emulate", 4, "--rows", 48, "--cols", 200, "--steps", 9, "--warmup", 2,
                                "--edge-rows", 8, "--walls", walls, "--form", form, "--check", 1, timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["slabs"] == 4 and line["message_rows_per_side"] == 6
    assert line["slowest_slab_ms_per_step"] > 0 and line["one_block_slab_sized_ms_per_step"] > 0


@pytest.mark.parametrize("walls", [0, 1])
def test_slab_ring_ade_driver_self_ring(tmp_path, walls):
    """one forked rank: closed, its neighbours are itself (every step exchanges through the ring); with walls a chain
    of one slab (nothing travels) -- both == one block bit for bit"""
    line = last_json(run_driver("slab_ring_ade", "--spawn", 1, "--rows", 96, "--cols", 256, "--steps", 5, "--warmup", 1,
                                "--edge-rows", 16, "--walls", walls, "--check", 1, "--id-file", tmp_path / "id", timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["n_gpus"] == 1


# ---- 6. physics across the seams -----------------------------------------------------------------------------------------
def test_scalar_mass_and_transport_across_the_seams_of_a_walled_chain(lib, oracle):
    """walls all round, w across the seams (+r), the scalar on the first slab only: sum C stays to 1e-12 relative over
    500 steps, and C rises from exactly 0 beyond the seam"""
    heights, C = (40, 40, 40), 64
    w = (0.05, 0.0)
    prm, gbc = params(FAST, w=w), wall_bc(True)
    gg, pre = global_state(oracle, sum(heights), C, seed=5, w=w, conc_rows=(4, 36))
    assert float(owned(pre[1], gg)[:, 40:].abs().sum()) == 0.0
    post, _ = one_block(lib, gg, pre, gbc, prm, 0)
    ch = chain(lib, gg, post, heights, False, gbc, prm)
    m0 = float(ch.gather(1).sum())
    for _ in range(500):
        ch.step(8)
    torch.cuda.synchronize()
    conc = ch.gather(1).sum(dim=0)
    m1 = float(conc.sum())
    assert abs(m1 - m0) <= 1e-12 * abs(m0), (m0, m1)
    beyond = float(conc[40:80].sum())
    assert beyond > 1e-3 * m0, f"no scalar crossed the seam: {beyond} of {m0}"
