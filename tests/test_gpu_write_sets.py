"""Write sets of the partial launches the slab steps are built from (lbm_ring_bgk_step, lbm_ring_kbc_step,
lbm_ring_cg_step: edge rows on the ring's stream, pack and exchange behind them, the interior on the caller's stream
beside them).  That schedule is only correct if every launch writes EXACTLY the nodes its contract names: fewer, and
the exchange packs stale rows; more, and two streams race on the same rows.  A test that runs all the parts and
compares the union with one full call cannot see either, so each launch here runs ALONE on a destination poisoned with
a NaN of a distinctive payload -- every plane, the ghost rows, the row-pitch padding and the plane padding included --
and the test asserts

  * the nodes whose bits changed are exactly the expected set, in all 9 planes (both colours for the two-phase step);
  * every written node is bit-equal to the same node of one full-range call (pinned to the oracle elsewhere).

A failure names the first wrong (colour, plane, row, column) and whether it was missed or over-written."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
from gpu_util import dev  # noqa: E402
from pylbm import _ptr  # noqa: E402
from test_cg_plan import DEFAULT_KNOBS, plans as cg_plans  # noqa: E402

SENTINEL = 0x7FF8DEADBEEF5A5A       # a quiet NaN no kernel computes: "never written"
PLANE_PAD = 40                      # doubles of padding behind every plane (even: keeps 16-byte alignment)
W9 = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1
    yield lib
    lib.reset_tuning()


# ---- the helper --------------------------------------------------------------------------------------------------------
def geom(R, C, ghost, pitch=0):
    P = pitch or C
    return pylbm.Geom(R, C, ghost, (R + 2 * ghost) * P + PLANE_PAD, pitch)


def alloc(g):
    return torch.empty(9 * g.plane_stride, dtype=torch.float64, device=dev())


def source(g, seed, scale=None):
    """a finite lattice in geometry g: every double of the allocation (ghost rows and padding too) near w_q"""
    rng = np.random.default_rng(seed)
    w = W9 if scale is None else scale
    a = np.repeat(w, g.plane_stride).reshape(9, g.plane_stride) * (1.0 + 0.05 * rng.random((9, g.plane_stride)))
    return torch.from_numpy(a.reshape(-1)).to(dev())


def owned(t, g):
    """[9, R, C] view of the owned nodes of a flat lattice"""
    P = g.row_pitch or g.C
    return t.view(9, g.plane_stride)[:, :(g.R + 2 * g.ghost) * P].view(9, g.R + 2 * g.ghost, P)[:, g.ghost:g.ghost + g.R, :g.C]


def rows_mask(g, *ranges):
    m = torch.zeros((g.R, g.C), dtype=torch.bool, device=dev())
    for r0, r1 in ranges:
        m[r0:r1] = True
    return m


def locate(i, g):
    """flat index of one colour's allocation -> (plane, row in owned numbering, column, what lies there)"""
    P = g.row_pitch or g.C
    q, off = divmod(int(i), g.plane_stride)
    if off >= (g.R + 2 * g.ghost) * P:
        return q, None, off - (g.R + 2 * g.ghost) * P, "plane padding"
    r, c = divmod(off, P)
    r -= g.ghost
    where = "row padding" if c >= g.C else ("ghost row" if r < 0 or r >= g.R else "node")
    return q, r, c, where


def run_poisoned(launch, dsts):
    for d in dsts:
        d.view(torch.int64).fill_(SENTINEL)
    torch.cuda.synchronize()
    launch()
    torch.cuda.synchronize()


def write_set(launch, dsts, g, expected, refs, what):
    """poison `dsts`, run `launch()` (one launch of the API under test), and return the list of what is wrong:
    the changed bits must cover exactly `expected` ([R, C] bool, owned nodes) in all 9 planes of every lattice of
    `dsts`, nothing of the ghost rows / padding, and every written node must equal the same node of `refs`"""
    run_poisoned(launch, dsts)
    errs = []
    for k, (d, ref) in enumerate(zip(dsts, refs)):
        want = torch.zeros(9 * g.plane_stride, dtype=torch.bool, device=dev())
        owned(want, g)[:] = expected
        changed = d.view(torch.int64) != SENTINEL
        bad = torch.nonzero(changed != want)
        if bad.numel():
            i = int(bad[0, 0])
            q, r, c, where = locate(i, g)
            P = g.row_pitch or g.C
            rows = sorted(set(((bad[:, 0] % g.plane_stride) // P - g.ghost).tolist()))
            errs.append(f"{what}: lattice {k}: {int(bad.shape[0])} doubles wrong; first: plane {q}, row {r}, column {c} ({where}) "
                        f"{'MISSED' if bool(want[i]) else 'OVER-WRITTEN'}; rows with wrong doubles: {rows[:24]}{' ...' if len(rows) > 24 else ''}")
            continue
        diff = torch.nonzero(want & (d.view(torch.int64) != ref.view(torch.int64)))
        if diff.numel():
            i = int(diff[0, 0])
            q, r, c, _ = locate(i, g)
            errs.append(f"{what}: lattice {k}: {int(diff.shape[0])} written doubles differ from the full-range call; first: "
                        f"plane {q}, row {r}, column {c}: {float(d[i])!r} != {float(ref[i])!r}")
    return errs


def full_call(launch_into, g, n=1):
    """the reference: the same API on the whole row range into fresh lattices (owned nodes must be finite)"""
    refs = [alloc(g) for _ in range(n)]
    for t in refs:
        t.zero_()
    launch_into(refs)
    torch.cuda.synchronize()
    for t in refs:
        assert bool(torch.isfinite(owned(t, g)).all()), "the full-range call itself produced non-finite values"
    return refs


def report(errs):
    assert not errs, f"{len(errs)} launch(es) with a wrong write set:\n" + "\n".join(errs[:40])


# ---- two-phase step: FRAME and INNER each alone --------------------------------------------------------------------------
def cg_setup(lib, g, halo):
    bc = pylbm.Bc()
    lib.raw.lbm_cg_default_bc(ct.byref(bc))
    if halo:
        bc.row_lo = bc.row_hi = pylbm.EDGE_HALO
    pg = pylbm.cg_params()
    # two colours of the shipped Rayleigh-Taylor densities (3 : 1), so the interface terms see varying fields
    src = [source(g, 1, 3.0 * W9), source(g, 2, W9)]
    return bc, pg, src


CG_SHAPES = [(R, C) for C in (61, 64) for R in (128, 129, 130, 146)] + [(R, 1040) for R in (128, 129, 130, 144, 146, 2050)]


@pytest.mark.parametrize("layout", ["halo3", "walls0"])
@pytest.mark.parametrize("R,C", CG_SHAPES)
def test_cg_step_parts_write_exactly_their_nodes(lib, R, C, layout):
    """lbm_cg_step_fused_part, FRAME alone and INNER alone (edge_rows 3, 16, 40): FRAME writes every node of rows
    [0, edge) and [R - edge, R) and of the wall / copy columns, INNER one rectangle of whole 16 x 32 tiles inside rows
    [edge, R - edge) (on 1040 columns a non-empty one, through the 16 x 64 big tiles), the two are disjoint and cover
    [0, R) x [0, C), neither touches a ghost row or the padding.  Slab layout: 3 ghost rows, HALO row edges; single block:
    no ghost rows, the driver's walls.  Heights with 0 < R % 16 < edge are where the frame once lost rows to INNER."""
    _cg_parts(lib, R, C, layout, 0)


def test_cg_step_parts_write_exactly_their_nodes_row_padded(lib):
    """the same on a row-padded slab (row_pitch = C + 64): the padding columns stay poisoned"""
    _cg_parts(lib, 130, 1040, "halo3", 1104)


def _cg_parts(lib, R, C, layout, pitch):
    halo = layout == "halo3"
    g = geom(R, C, 3 if halo else 0, pitch)
    bc, pg, src = cg_setup(lib, g, halo)

    def fused(d):
        lib.cg_step_fused(_ptr(d[0]), _ptr(d[1]), _ptr(src[0]), _ptr(src[1]), ct.byref(g), ct.byref(bc), ct.byref(pg), 0, R,
                          None, None, None, None, None, None)

    refs = full_call(fused, g, 2)
    dst = [alloc(g), alloc(g)]
    full = rows_mask(g, (0, R))
    errs = []
    edges = [e for e in (3, 16, 40) if 2 * e <= R]
    # the rectangle the host-only planner (drivers/cg_plan_dump) names for the same case, the knobs at their defaults
    planned = cg_plans([(R, C, g.ghost, halo, halo, 0, R, pylbm.CG_PART_INNER, e) + DEFAULT_KNOBS for e in edges])
    for edge, plan in zip(edges, planned):

        def part(p):
            lib.cg_step_fused_part(_ptr(dst[0]), _ptr(dst[1]), _ptr(src[0]), _ptr(src[1]), ct.byref(g), ct.byref(bc), ct.byref(pg),
                                   p, edge, None, None, None, None, None, None)

        # INNER first: the nodes it writes (plane 0 of the red lattice) are the rectangle the FRAME must leave out
        run_poisoned(lambda: part(pylbm.CG_PART_INNER), dst)
        inner = owned(dst[0], g).view(torch.int64)[0] != SENTINEL
        rows = torch.nonzero(inner.any(dim=1)).flatten().tolist()
        cols = torch.nonzero(inner.any(dim=0)).flatten().tolist()
        what = f"R={R} C={C} {layout}{' pitch=%d' % pitch if pitch else ''} edge_rows={edge}"
        if rows:
            r0, r1, c0, c1 = rows[0], rows[-1] + 1, cols[0], cols[-1] + 1
            rect = torch.zeros_like(full)
            rect[r0:r1, c0:c1] = True
            wall = 0 if halo else 3      # the tile kernel's ring rows stay off the wall rows
            allowed = rows_mask(g, (max(edge, wall), R - max(edge, wall)))
            if not (bool((rect == inner).all()) and r0 % 16 == 0 and r1 % 16 == 0 and c0 % 32 == 0 and c1 % 32 == 0
                    and r0 >= max(edge, wall) and r1 <= R - max(edge, wall) and c0 >= 2 and c1 <= C - 2):
                errs.append(f"{what}: INNER wrote {'a rectangle' if bool((rect == inner).all()) else 'a non-rectangle'} "
                            f"rows [{r0}, {r1}) x columns [{c0}, {c1}), not whole tiles inside rows [{edge}, {R - edge}) and away from the walls")
                # INNER is checked against what it may write, the FRAME against all the rest: the edge rows INNER took
                # from it show up as MISSED below
                inner = inner & allowed
            want = (16 * plan["ir0"], 16 * plan["ir1"], 32 * plan["ic0"], 32 * plan["ic1"])
            if not plan["split"] or (r0, r1, c0, c1) != want:
                errs.append(f"{what}: INNER wrote rows [{r0}, {r1}) x columns [{c0}, {c1}), cg_plan_dump plans "
                            f"{'rows [%d, %d) x columns [%d, %d)' % want if plan['split'] else 'no inner rectangle'}")
        if C == 1040:
            if not rows:
                errs.append(f"{what}: INNER wrote nothing where the lattice holds an inner rectangle")
            elif lib.raw.lbm_cg_last_inner_form() != 102:
                errs.append(f"{what}: INNER ran inner form {lib.raw.lbm_cg_last_inner_form()}, not the 16 x 64 big tiles (102)")
        # the exact check of INNER's own nodes (values against the one-call step; nothing outside the rectangle)
        errs += write_set(lambda: part(pylbm.CG_PART_INNER), dst, g, inner, refs, f"{what} INNER")
        # FRAME: exactly the complement -- hence every node of the edge rows and of the wall / copy columns
        errs += write_set(lambda: part(pylbm.CG_PART_FRAME), dst, g, full & ~inner, refs, f"{what} FRAME")
    report(errs)


# ---- row-range kernels, each on [r0, r1) alone: the expected set is exactly [r0, r1) x [0, C) ------------------------------
def ranges_for(R, G, window):
    """heights 1, 2, 3, 15, 17 at non-zero offsets, a height that ends mid-chunk (window kernels run with 8-row chunks),
    and the exact triples of the ring steps: (0, E), (R - E, R), (E, R - E) for E in {G, 16, 40}"""
    out = [(5, 6), (7, 9), (1, 4), (20, 35), (R - 20, R - 3)]
    if window:
        out.append((11, 32))
    for E in sorted({max(G, 1), 16, 40}):
        if 2 * E < R:
            out += [(0, E), (R - E, R), (E, R - E)]
    return out


def bc_for(layout):
    if layout == "halo":
        return pylbm.Bc(pylbm.EDGE_HALO, pylbm.EDGE_HALO)
    if layout == "walls":   # bounce-back rows and columns: the single-step path adds its edge pass, the window its fix-ups
        return pylbm.Bc(pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_BOUNCE_BACK)
    return pylbm.Bc.periodic()


def _row_ranges(g, call, ranges, what):
    """call(dst, r0, r1): one launch of the kernel under test on [r0, r1)"""
    src = source(g, 7)
    refs = full_call(lambda d: call(d[0], src, 0, g.R), g)
    dst = [alloc(g)]
    errs = []
    for r0, r1 in ranges:
        errs += write_set(lambda: call(dst[0], src, r0, r1), dst, g, rows_mask(g, (r0, r1)), refs, f"{what} rows [{r0}, {r1})")
    report(errs)


R_RANGE = 96


@pytest.mark.parametrize("model", ["bgk", "kbc"])
@pytest.mark.parametrize("C,ghost,layout", [(61, 0, "periodic"), (100, 0, "periodic"), (100, 1, "halo"), (128, 3, "halo"),
                                            (100, 0, "walls"), (61, 0, "walls")])
def test_single_step_row_ranges(lib, model, C, ghost, layout):
    """lbm_bgk_stream_collide / lbm_kbc_stream_collide (61 columns: the generic kernel; even widths: the fast kernel,
    plus the edge pass on walls)"""
    g, bc = geom(R_RANGE, C, ghost), bc_for(layout)
    if model == "bgk":
        prm = pylbm.BgkParams(1.2)
        fn = lib.bgk_stream_collide
    else:
        prm = pylbm.KbcParams(1.3)
        fn = lib.kbc_stream_collide
    _row_ranges(g, lambda d, s, r0, r1: fn(_ptr(d), _ptr(s), ct.byref(g), ct.byref(bc), ct.byref(prm), r0, r1, None, None, None),
                ranges_for(R_RANGE, ghost, False), f"{model} C={C} ghost={ghost} {layout}")


@pytest.mark.parametrize("ghost", [0, 2])
def test_bgk_x2_row_ranges(lib, ghost):
    """lbm_bgk_stream_collide_x2 (C % 64 == 0, ghost 0 or 2; 8-row tiles, so 15, 17 and 21 rows end mid-tile)"""
    g, bc, prm = geom(R_RANGE, 128, ghost), bc_for("halo" if ghost else "periodic"), pylbm.BgkParams(1.2)
    _row_ranges(g, lambda d, s, r0, r1: lib.bgk_stream_collide_x2(_ptr(d), _ptr(s), ct.byref(g), ct.byref(bc), ct.byref(prm),
                                                                       r0, r1, None),
                ranges_for(R_RANGE, ghost, True), f"bgk x2 ghost={ghost}")


WINDOW = [(d, 0, "periodic") for d in (2, 3, 4, 5, 6)] + [(d, d, "halo") for d in (2, 3, 4, 5, 6)] + [(d, 0, "walls") for d in (2, 3, 5)]


@pytest.mark.parametrize("depth,ghost,layout", WINDOW)
@pytest.mark.parametrize("chunk", [0, 8])
def test_bgk_xn_row_ranges(lib, depth, ghost, layout, chunk):
    """lbm_bgk_stream_collide_xn, 2..6 steps per launch (walls: up to 5); chunk 8: the window walks 8-row chunks, so most
    ranges end mid-chunk"""
    g, bc, prm = geom(R_RANGE, 100, ghost), bc_for(layout), pylbm.BgkParams(1.2)
    lib.set_tuning(b"sw_rows", chunk or -1)
    try:
        _row_ranges(g, lambda d, s, r0, r1: lib.bgk_stream_collide_xn(_ptr(d), _ptr(s), ct.byref(g), ct.byref(bc), ct.byref(prm),
                                                                           depth, r0, r1, None),
                    ranges_for(R_RANGE, ghost, True), f"bgk xn depth={depth} ghost={ghost} {layout} chunk={chunk}")
    finally:
        lib.set_tuning(b"sw_rows", -1)


@pytest.mark.parametrize("depth,ghost,layout", [(2, 2, "halo"), (4, 4, "halo"), (6, 6, "halo"), (5, 0, "periodic"), (3, 0, "walls")])
def test_bgk_xn2_both_ranges_in_one_launch(lib, depth, ghost, layout):
    """lbm_bgk_stream_collide_xn2: [r0, r1) and [b2, b2 + r1 - r0) in one launch -- the two edge ranges of a slab (walls: two
    launches behind the same call) -- and nothing between them"""
    g, bc, prm = geom(R_RANGE, 100, ghost), bc_for(layout), pylbm.BgkParams(1.2)
    src = source(g, 7)
    refs = full_call(lambda d: lib.bgk_stream_collide_xn(_ptr(d[0]), _ptr(src), ct.byref(g), ct.byref(bc), ct.byref(prm), depth, 0, g.R,
                                                         None), g)
    dst = [alloc(g)]
    pairs = [(0, E, R_RANGE - E) for E in sorted({max(ghost, 1), 16, 40})] + [(3, 20, 50), (5, 6, 90), (2, 19, 19), (10, 27, 79)]
    errs = []
    for r0, r1, b2 in pairs:
        errs += write_set(lambda: lib.bgk_stream_collide_xn2(_ptr(dst[0]), _ptr(src), ct.byref(g), ct.byref(bc), ct.byref(prm), depth,
                                                             r0, r1, b2, None),
                          dst, g, rows_mask(g, (r0, r1), (b2, b2 + r1 - r0)), refs,
                          f"bgk xn2 depth={depth} ghost={ghost} {layout} rows [{r0}, {r1}) + [{b2}, {b2 + r1 - r0})")
    report(errs)


@pytest.mark.parametrize("depth,ghost,layout", [(2, 0, "periodic"), (3, 3, "halo"), (4, 4, "halo"), (4, 0, "periodic"), (2, 0, "walls"),
                                                (3, 0, "walls")])
@pytest.mark.parametrize("chunk", [0, 8])
def test_kbc_xn_row_ranges(lib, depth, ghost, layout, chunk):
    """lbm_kbc_stream_collide_xn, 2..4 steps per launch with the reassociated collision (walls: single block, up to 3)"""
    g, bc, prm = geom(R_RANGE, 100, ghost), bc_for(layout), pylbm.KbcParams(1.3, pylbm.FORM_REASSOCIATED)
    lib.set_tuning(b"sw_rows", chunk or -1)
    try:
        _row_ranges(g, lambda d, s, r0, r1: lib.kbc_stream_collide_xn(_ptr(d), _ptr(s), ct.byref(g), ct.byref(bc), ct.byref(prm),
                                                                           depth, r0, r1, None),
                    ranges_for(R_RANGE, ghost, True), f"kbc xn depth={depth} ghost={ghost} {layout} chunk={chunk}")
    finally:
        lib.set_tuning(b"sw_rows", -1)


@pytest.mark.parametrize("kernel", ["two_pass", "fused"])
@pytest.mark.parametrize("C,layout", [(100, "halo3"), (61, "walls0"), (1040, "halo3")])
def test_cg_row_ranges(lib, kernel, C, layout):
    """lbm_cg_stream_collide (pass B of the reference-order step, fields from pass A on the same source) and
    lbm_cg_step_fused on a row range: both colours, exactly [r0, r1) x [0, C)"""
    halo = layout == "halo3"
    R = R_RANGE
    g = geom(R, C, 3 if halo else 0)
    bc, pg, src = cg_setup(lib, g, halo)
    fr = R + 4 if halo else R            # the macroscopic fields of a slab carry 2 ghost rows
    rho_r, rho_b = [torch.empty((fr, C), dtype=torch.float64, device=dev()) for _ in range(2)]
    u = torch.empty((2, fr, C), dtype=torch.float64, device=dev())
    lib.cg_stream_moments(_ptr(rho_r), _ptr(rho_b), _ptr(u), _ptr(src[0]), _ptr(src[1]), ct.byref(g), ct.byref(bc), ct.byref(pg), None)

    def call(d, r0, r1):
        if kernel == "fused":
            lib.cg_step_fused(_ptr(d[0]), _ptr(d[1]), _ptr(src[0]), _ptr(src[1]), ct.byref(g), ct.byref(bc), ct.byref(pg), r0, r1,
                              None, None, None, None, None, None)
        else:
            lib.cg_stream_collide(_ptr(d[0]), _ptr(d[1]), _ptr(src[0]), _ptr(src[1]), _ptr(rho_r), _ptr(rho_b), _ptr(u), ct.byref(g),
                                  ct.byref(bc), ct.byref(pg), r0, r1, None, None, None)

    refs = full_call(lambda d: call(d, 0, R), g, 2)
    dst = [alloc(g), alloc(g)]
    errs = []
    for r0, r1 in ranges_for(R, 3, False):
        errs += write_set(lambda: call(dst, r0, r1), dst, g, rows_mask(g, (r0, r1)), refs, f"cg {kernel} C={C} {layout} rows [{r0}, {r1})")
    report(errs)
