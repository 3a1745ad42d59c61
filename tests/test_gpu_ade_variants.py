"""GPU suite, the fluid + scalar step where the other suites do not go: every launch variant and the smallest shapes.

The step's launches read two process-wide knobs, `nt` (bit 0: non-temporal loads, bit 1: non-temporal stores; default 3)
and `grid_cap` (0: one workgroup per item; n > 0: at most n workgroups, each striding over the items).  The other
suites of the step run with the defaults only, so three quarters of the instantiations of k_ade_stream_collide /
k_ade_stream_collide_part and the second iteration of their grid-stride loops were never executed.  Here:
  A. the one-block step (lbm_ade_stream_collide_b) on 6 x 1030 -- three 512-column tiles per row, three live lanes in the
     last -- under nt in {0, 1, 2, 3} x grid_cap in {0, 1, 7}: bitwise the yardstick in the reference order, bitwise the
     default launch in the reassociated form;
  B. the part launches (lbm_ade_stream_collide_part_b / _part_w, FRAME + INNER) under the same twelve combinations, on one
     block and on ghost-1 slabs: bitwise the full step, and the write set of each part;
  C. lattices of 1 x 2 to 3 x 6 nodes, and 5 x 514 / 4 x 1026 (a last tile of one live lane, which is also the wall
     lane), through pylbm.AdeSolver against the yardstick;
  D. the smallest slab the part entry accepts, R = 3 with one edge row.
The yardstick is `oracle_loop` of tests/ade_util.py: numpy over the oracle's primitives, never the library under test.
The caps 1 and 7 are coprime to the tile count 3, so one workgroup's stride walks across rows, and in a FRAME launch
across the jump from the first edge band to the second."""
import numpy as np
import pytest
from conftest import relerr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
from ade_calls import full_step, part, step_into  # noqa: E402
from ade_slab_util import slab_bc  # noqa: E402
from ade_util import (GBC, GUO, W, alloc, assert_bits, assert_state_bits, assert_write_set, bits, build_sbc,  # noqa: E402
                      buoyancy, buoyant_initial_state, collide, cut_slab, from_lattice, geom, initial_state, moment_fields,
                      oracle_loop, owned, params, poisoned, random_lattice, to_lattice)
from gpu_util import bits_equal, dev  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
FORMS = {"reference_order": REF, "reassociated": FAST}
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
BB, SP, HALO = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO
FIXED = pylbm.ADE_SCALAR_FIXED
ROW_NEG, COL_NEG = pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_COL_NEG
OMEGA, OMEGA_G = 1.2, 1.7                      # the rates of ade_util.params
WB, BETA, C_REF = (3e-3, -2e-3), (2e-3, -1.5e-3), 0.4  # the buoyant cases of the yardstick (C in [0, 1])
R0, C0 = 6, 1030                               # A and B: 3 tiles per row, the last with 3 live lanes
COMBOS = [(nt, cap) for nt in (0, 1, 2, 3) for cap in (0, 1, 7)]
TOL = 1e-10  # reassociated form against the reference order: test_reassociated_form_agrees_with_the_reference_order's


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


@pytest.fixture(autouse=True)
def _default_knobs_afterwards(lib):
    yield
    lib.reset_tuning()


def knobs(lib, nt, cap):
    lib.set_tuning(b"nt", nt)
    lib.set_tuning(b"grid_cap", cap)


def default_knobs(lib):
    knobs(lib, -1, -1)  # unset: nt = 3, no cap


def assert_moments(got, want, what):
    for k, name in enumerate(("rho", "u", "C")):
        assert_bits(got[k], want[k], f"{what}: {name}")


# ---- A. every variant of the one-block step ------------------------------------------------------------------------------
def run_steps(lib, g, bc, prm, src, steps, sbc, by, with_moments):
    """`steps` ping-pong steps of lbm_ade_stream_collide_b: (the last pair of lattices, the moments of the last step)"""
    cur, m = src, (moment_fields(g) if with_moments else None)
    for _ in range(steps):
        cur = full_step(lib, "_b", g, bc, prm, *cur, sbc=sbc, buoy=by, moments=m)
    torch.cuda.synchronize()
    return cur, m


def assert_same_run(got, want, what):
    """the whole allocations (the padding stays the zeros of alloc) and, where written, the three moment fields"""
    for k, name in enumerate("fg"):
        assert_bits(got[0][k], want[0][k], f"{what}: {name}")
    if got[1] is not None:
        assert_moments(got[1], want[1], what)


@pytest.mark.parametrize("descriptor", ["none", "fixed_rows", "buoyant"])
@pytest.mark.parametrize("edges", ["periodic", "box"])
def test_every_variant_of_the_one_block_step(lib, oracle, edges, descriptor):
    """three raw steps from the yardstick's own post-collision state, with the moment outputs and with them NULL.
    Reference order: f, g, rho, u, C of every (nt, grid_cap) == the yardstick, bit for bit.  Reassociated: every
    combination == the default launch of that form bit for bit (the same arithmetic, other memory instructions and another
    schedule), and the default launch agrees with the yardstick to 1e-10 of each field's largest magnitude (a buoyant step
    runs the reference order whatever the form: bit for bit).  Then one step over rows [0, R) as the calls [0, 2) and
    [2, R) under grid_cap = 7 == the default launch.  FIXED rows on a periodic box do not exist: the host refuses them.
    Measured on MI355X, reassociated default launch against the yardstick after the 3 steps, the largest of the cases:
    f 1.3e-15, g 1.6e-15, rho 8.8e-16, u 9.9e-15, C 6.4e-16."""
    R, C, steps = R0, C0, 3
    g, bc = geom(R, C, 0), (GBC if edges == "box" else pylbm.Bc())
    by = buoyancy(BETA, C_REF, GUO) if descriptor == "buoyant" else None
    w = WB if by else W
    f0, g0 = buoyant_initial_state(oracle, R, C, 3, w) if by else initial_state(oracle, R, C, 3, w)
    sbc, fixed = (build_sbc({"row_lo": 7e-4, "row_hi": ("profile", np.linspace(2e-4, 1.2e-3, C))}, R, C)
                  if descriptor == "fixed_rows" else (None, {}))
    p0 = collide(oracle, f0, g0, OMEGA, OMEGA_G, w, by)
    src = to_lattice(p0["fc"], g), to_lattice(p0["gc"], g)
    if fixed and edges == "periodic":
        for form in FORMS.values():
            with pytest.raises(pylbm.LbmError, match="FIXED on a PERIODIC"):
                full_step(lib, "_b", g, bc, params(form, w=w), *src, sbc=sbc)
        return
    st = oracle_loop(oracle, f0, g0, OMEGA, OMEGA_G, w, steps, bc, fixed, by=by)
    yard = collide(oracle, st["f"], st["g"], OMEGA, OMEGA_G, w, by)
    yard_dev = ((to_lattice(yard["fc"], g), to_lattice(yard["gc"], g)),
                [torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dev())
                 for a in (yard["rho"], yard["u"].transpose(2, 0, 1), yard["C"])])
    for fname, form in FORMS.items():
        prm = params(form, w=w)
        default_knobs(lib)
        base = run_steps(lib, g, bc, prm, src, steps, sbc, by, True)
        if form == REF or by:
            assert_same_run(base, yard_dev, f"{fname} default launch against the yardstick")
        else:
            got = dict(f=from_lattice(base[0][0], g), g=from_lattice(base[0][1], g), rho=base[1][0].cpu().numpy(),
                       u=base[1][1].cpu().numpy(), C=base[1][2].cpu().numpy())
            want = dict(f=yard["fc"], g=yard["gc"], rho=yard["rho"].reshape(-1), u=yard["u"].transpose(2, 0, 1).reshape(-1),
                        C=yard["C"].reshape(-1))
            errs = {k: relerr(got[k], want[k]) for k in got}
            print(f"A {edges} {descriptor}: reassociated default launch vs the yardstick after {steps} steps:", errs)
            assert max(errs.values()) <= TOL, errs
            assert not bits_equal(got["g"], want["g"])  # the two forms are different code
        for with_moments in (True, False):
            for nt, cap in COMBOS:
                knobs(lib, nt, cap)
                got = run_steps(lib, g, bc, prm, src, steps, sbc, by, with_moments)
                assert_same_run(got, base, f"{fname} nt={nt} grid_cap={cap} moments={with_moments}")
        # one step over two row ranges, strided
        default_knobs(lib)
        first = run_steps(lib, g, bc, prm, src, 1, sbc, by, True)
        for nt in (0, 1, 2, 3):
            knobs(lib, nt, 7)
            dst, m = (alloc(g), alloc(g)), moment_fields(g)
            for rows in ((0, 2), (2, R)):
                step_into(lib, "_b", g, bc, prm, dst, src, rows, sbc=sbc, buoy=by, moments=m)
            torch.cuda.synchronize()
            assert_same_run((dst, m), first, f"{fname} rows [0, 2) + [2, {R}) nt={nt} grid_cap=7")


# ---- B. every variant of the part launches -------------------------------------------------------------------------------
LAYOUTS = {"one_block": (R0, 0, R0), "slab_halo_halo": (14, 4, 10), "slab_halo_wall": (14, 8, 14)}  # global rows, [r0, r1)
BY_B = ((2e-2, -1e-2), 1.0)  # random_lattice: C ~ 1.0 .. 1.05


def global_lattice(Rg, C, block_R):
    """the global box: the one block itself (dense), or the lattice the slabs are cut from (padded rows)"""
    return geom(Rg, C, 0, 0 if Rg == block_R else C + 10)


def cut(gg, gbc, src, r0, r1):
    """geometry, edges and source lattices of the launch on global rows [r0, r1): the block itself, or a ghost-1 slab
    with HALO where it is cut and the global wall where it ends"""
    if (r0, r1) == (0, gg.R):
        return gg, gbc, src
    slab = [cut_slab(s, gg, r0, r1, gg.row_pitch) for s in src]
    return slab[0][0], slab_bc(gbc, r0, r1, gg.R), (slab[0][1], slab[1][1])


def scalar_walls(prof, r0, r1, Rg):
    """FIXED edges of rows [r0, r1) of the global box: a device profile along col_lo, absorbing col_hi, and the constant
    rows the launch keeps"""
    kw = dict(col_lo=(0.0, prof[r0:r1]), col_hi=0.0)
    if r0 == 0:
        kw["row_lo"] = 0.98
    if r1 == Rg:
        kw["row_hi"] = 1.02
    return pylbm.AdeScalarBC(**kw)


def descriptors_b(descriptor, Rg, r0, r1):
    """(global scalar walls, the launch's, buoyancy)"""
    by = buoyancy(*BY_B, GUO) if "buoyant" in descriptor else None
    if "fixed" not in descriptor:
        return None, None, by
    prof = torch.from_numpy(np.linspace(0.9, 1.1, Rg)).to(dev())
    return scalar_walls(prof, 0, Rg, Rg), scalar_walls(prof, r0, r1, Rg), by


def check_parts(lib, launch, g, E, gg, want, want_m, r0, r1, what):
    """FRAME then INNER into SENTINEL lattices under every (nt, grid_cap), with and without moments: after FRAME exactly
    the edge rows are written, after INNER exactly the owned nodes, each double the full step's"""
    Rg = gg.R
    frame = list(range(E)) + list(range(g.R - E, g.R))
    for with_moments in (False, True):
        for nt, cap in COMBOS:
            knobs(lib, nt, cap)
            tag = f"{what} E={E} nt={nt} grid_cap={cap} moments={with_moments}"
            dst, m = (poisoned(g), poisoned(g)), (moment_fields(g) if with_moments else None)
            launch(dst, FRAME, E, m)
            torch.cuda.synchronize()
            for k, name in enumerate("fg"):
                assert_write_set(dst[k], g, frame, f"{tag}: FRAME, {name}")
            launch(dst, INNER, E, m)
            torch.cuda.synchronize()
            for k, name in enumerate("fg"):
                assert_write_set(dst[k], g, list(range(g.R)), f"{tag}: FRAME + INNER, {name}")
                assert_bits(owned(dst[k], g), owned(want[k], gg)[:, r0:r1], f"{tag}: {name}")
            if m is not None:
                assert_moments([m[0].view(g.R, g.C), m[1].view(2, g.R, g.C), m[2].view(g.R, g.C)],
                               [want_m[0].view(Rg, g.C)[r0:r1], want_m[1].view(2, Rg, g.C)[:, r0:r1],
                                want_m[2].view(Rg, g.C)[r0:r1]], tag)


@pytest.mark.parametrize("descriptor", ["none", "fixed", "buoyant", "buoyant_fixed"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_variant_of_the_part_launches(lib, layout, form, descriptor):
    """6 rows x 1030 columns with 1 and 2 edge rows, as one block (the box) and as ghost-1 slabs of a 14-row box (HALO on
    both sides; HALO above and the bounce-back wall below): FRAME + INNER of lbm_ade_stream_collide_part_b == the
    default launch of the full step on the global box, bit for bit, lattices and moments"""
    Rg, r0, r1 = LAYOUTS[layout]
    gg, prm = global_lattice(Rg, C0, R0), params(FORMS[form])
    gsbc, sbc, by = descriptors_b(descriptor, Rg, r0, r1)
    src_g = random_lattice(gg, 1), random_lattice(gg, 2)
    default_knobs(lib)
    want_m = moment_fields(gg)
    want = full_step(lib, "_b", gg, GBC, prm, *src_g, sbc=gsbc, buoy=by, moments=want_m)
    g, bc, src = cut(gg, GBC, src_g, r0, r1)
    assert g.R == R0

    def launch(dst, which, E, m):
        part(lib, "_b", g, bc, prm, dst, src, which, E, sbc=sbc, buoy=by, moments=m)

    for E in (1, 2):
        check_parts(lib, launch, g, E, gg, want, want_m, r0, r1, f"{layout} {form} {descriptor}")


def body(lib, Rg, C):
    """interior walls of the global box: a column wall through EVERY row on the last lane pair of tile 0 (so every FRAME
    and INNER band of every layout holds a node and the body crosses their boundaries), and row walls across the seam
    between tile 0 and tile 1 on every fourth row; FIXED at 1.01"""
    t = pylbm.AdeInteriorWalls(lib, Rg, C)
    t.add(0, 511, 1, 0, Rg, COL_NEG, COL_NEG, FIXED, 1.01)
    for r in range(2, Rg, 4):
        t.add(r, 500, 0, 1, 24, ROW_NEG, ROW_NEG, FIXED, 1.01)
    return t.finalize()


@pytest.mark.parametrize("descriptor", ["none", "buoyant_fixed"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_every_variant_of_the_part_launches_with_interior_walls(lib, layout, form, descriptor):
    """the same launches through lbm_ade_stream_collide_part_w with a table whose body crosses the FRAME / INNER
    boundary: k_ade_iwalls_ranges behind a capped, strided dispatch == lbm_ade_stream_collide_w on the global box"""
    Rg, r0, r1 = LAYOUTS[layout]
    gg, prm = global_lattice(Rg, C0, R0), params(FORMS[form])
    gsbc, sbc, by = descriptors_b(descriptor, Rg, r0, r1)
    src_g = random_lattice(gg, 3), random_lattice(gg, 4)
    table = body(lib, Rg, C0)
    view = table if (r0, r1) == (0, Rg) else table.slab(r0, r1 - r0).finalize()
    rows = {n["r"] for n in view.nodes()}
    assert rows == set(range(R0))  # every band of E = 1 and E = 2 holds a node
    default_knobs(lib)
    want_m = moment_fields(gg)
    want = full_step(lib, "_w", gg, GBC, prm, *src_g, sbc=gsbc, buoy=by, iwalls=table, moments=want_m)
    plain = full_step(lib, "_b", gg, GBC, prm, *src_g, sbc=gsbc, buoy=by)
    assert not torch.equal(bits(want[1]), bits(plain[1]))  # the body is felt
    g, bc, src = cut(gg, GBC, src_g, r0, r1)

    def launch(dst, which, E, m):
        part(lib, "_w", g, bc, prm, dst, src, which, E, sbc=sbc, buoy=by, iwalls=view, moments=m)

    for E in (1, 2):
        check_parts(lib, launch, g, E, gg, want, want_m, r0, r1, f"{layout} {form} {descriptor} with the body")
    if view is not table:
        view.close()
    table.close()


# ---- C. the smallest shapes against the yardstick ------------------------------------------------------------------------
SHAPES = [(1, 2), (1, 4), (2, 2), (2, 4), (3, 2), (3, 6), (5, 514), (4, 1026)]
EDGES_C = {"periodic": pylbm.Bc(), "bounce_back_rows": pylbm.Bc(row_lo=BB, row_hi=BB),
           "specular_col_lo_bounce_back_col_hi": pylbm.Bc(col_lo=SP, col_hi=BB), "box": GBC}
MEASURED = {}  # field -> the largest reassociated-form error of the cases run


def fixed_on_every_wall(bc, R, C):
    """FIXED on every wall edge of bc, constants and profiles mixed (no wall: the all-NO_FLUX descriptor)"""
    spec, rows = {}, bc.row_lo == BB
    if rows:
        spec["row_lo"] = 7e-4
        spec["row_hi"] = ("profile", np.linspace(2e-4, 1.2e-3, C))
    if bc.col_lo in (BB, SP):
        spec["col_lo"] = ("profile", np.linspace(1.5e-3, 3e-4, R)) if rows else 2e-3
        spec["col_hi"] = 0.0 if rows else ("profile", np.linspace(1e-4, 9e-4, R))
    return spec


@pytest.mark.parametrize("descriptor", ["none", "fixed", "buoyant"])
@pytest.mark.parametrize("edges", list(EDGES_C))
@pytest.mark.parametrize("R,C", SHAPES)
def test_the_smallest_shapes_are_the_reference_loop(lib, oracle, R, C, edges, descriptor):
    """9 driver iterations through pylbm.AdeSolver (set_state, the collide-only first iteration, 8 fused steps and the
    lazily streamed level of get_state) at the shapes where a row's only pair is its first and its last, a row is its own
    neighbour (R = 1: one node is row_lo and row_hi at once) or two rows are each other's in both directions, and where
    the last 512-column tile holds one live lane.  Reference order, and a buoyant step in either form: f, g, rho, u, C ==
    the yardstick bit for bit.  Reassociated form: each field within 1e-10 of the yardstick, relative to the field's
    largest magnitude (conftest.relerr) -- the bound test_reassociated_form_agrees_with_the_reference_order states for 500
    steps, fixed before measuring.  Measured on MI355X, the largest over all cases: f 2.1e-15,
    g 1.6e-15, rho 1.8e-15, u 7.2e-14, C 1.8e-15."""
    bc = EDGES_C[edges]
    by = buoyancy(BETA, C_REF, GUO) if descriptor == "buoyant" else None
    w = WB if by else W
    f0, g0 = buoyant_initial_state(oracle, R, C, R * C, w) if by else initial_state(oracle, R, C, R * C, w)
    sbc, fixed = build_sbc(fixed_on_every_wall(bc, R, C), R, C) if descriptor == "fixed" else (None, {})
    want = oracle_loop(oracle, f0, g0, OMEGA, OMEGA_G, w, 9, bc, fixed, by=by)
    assert all(np.all(np.isfinite(v)) for v in want.values())
    for fname, form in FORMS.items():
        sv = pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(OMEGA, 0, form=form), pylbm.AdeParams(OMEGA_G, w, form=form), bc=bc,
                             scalar_bc=sbc, buoyancy=by)
        sv.set_state(f0, g0)
        sv.step(9)
        got = sv.get_state()
        sv.close()
        what = f"{R}x{C} {edges} {descriptor} {fname}"
        if form == REF or by:
            assert_state_bits(got, want, what)
            continue
        errs = {k: relerr(got[k], want[k]) for k in ("f", "g", "rho", "u", "C")}
        print(f"C {what} vs the yardstick after 9 steps:", errs)
        for k, e in errs.items():
            MEASURED[k] = max(MEASURED.get(k, 0.0), e)
        print("C largest so far:", MEASURED)
        assert max(errs.values()) <= TOL, (what, errs)


# ---- D. the smallest slab ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descriptor", ["fixed", "buoyant_fixed"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("layout", ["one_block", "slab_halo_halo"])
@pytest.mark.parametrize("C", [2, 514])
def test_the_smallest_slab(lib, C, layout, form, descriptor):
    """R = 3 with one edge row -- the smallest the part entry accepts (2 x edge_rows < R): FRAME is rows 0 and 2, INNER
    the middle row.  As one block (the box) and as a ghost-1 slab with HALO rows cut from a 7-row box, FIXED edges,
    without and with a one-node table of interior walls on the middle row (at C = 2 the node is also the col_lo wall node,
    at C = 514 the one live lane of the last tile): FRAME + INNER == the full step bit for bit, and the write sets"""
    R, E = 3, 1
    Rg, r0, r1 = (R, 0, R) if layout == "one_block" else (7, 2, 5)
    gg, prm = global_lattice(Rg, C, R), params(FORMS[form])
    gsbc, sbc, by = descriptors_b(descriptor, Rg, r0, r1)
    src_g = random_lattice(gg, 5), random_lattice(gg, 6)
    g, bc, src = cut(gg, GBC, src_g, r0, r1)
    assert g.R == R
    table = pylbm.AdeInteriorWalls(lib, Rg, C).add(r0 + 1, C - 2, 0, 1, 1, ROW_NEG, ROW_NEG, FIXED, 1.01).finalize()
    view = table if (r0, r1) == (0, Rg) else table.slab(r0, R).finalize()
    assert [(n["r"], n["c"]) for n in view.nodes()] == [(1, C - 2)]
    wants = []
    for t, v in ((None, None), (table, view)):
        what = f"R=3 C={C} {layout} {form} {descriptor} table={t is not None}"
        want = full_step(lib, "_w", gg, GBC, prm, *src_g, sbc=gsbc, buoy=by, iwalls=t)
        wants.append(want)
        dst = poisoned(g), poisoned(g)
        for which, rows in ((FRAME, [0, 2]), (INNER, [0, 1, 2])):
            if t is None:
                part(lib, "_b", g, bc, prm, dst, src, which, E, sbc=sbc, buoy=by)
            else:
                part(lib, "_w", g, bc, prm, dst, src, which, E, sbc=sbc, buoy=by, iwalls=v)
            torch.cuda.synchronize()
            for k, name in enumerate("fg"):
                assert_write_set(dst[k], g, rows, f"{what}: after part {which}, {name}")
        for k, name in enumerate("fg"):
            assert_bits(owned(dst[k], g), owned(want[k], gg)[:, r0:r1], f"{what}: {name}")
    assert not torch.equal(bits(wants[0][1]), bits(wants[1][1]))  # the node is felt
    if view is not table:
        view.close()
    table.close()
