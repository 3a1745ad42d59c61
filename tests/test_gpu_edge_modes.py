"""Every edge mode of lbm_bc against a reference that shares no code with the kernels (tests/edge_reference.py: numpy
np.roll + whole-edge slice assignments + the oracle's collision operators; pinned on the CPU by test_edge_reference.py).

What is compared, with which bar:
  lbm_stream                      all 3^2 x 4^2 = 144 edge sets                  bitwise (data movement; the velocity-row term too)
  single steps                    the same 144, BGK and KBC                      reference order bitwise, reassociated relerr < 1e-12
  moments, row ranges             the same 144                                   the same
  multi-step windows              the 24 unmixed wall sets, every split / chunk  BGK reference order bitwise; reassociated and KBC
                                                                                 relerr < 1e-12 AND bitwise equal to single steps
  lbm_solver_step, mixed axes     wall on one side, PERIODIC on the other        the same bars over 7 iterations
  mass in sealed boxes            pylbm.Solver, default launches, 200 steps      8 x the reference's own drift, floor 64 eps

1e-12 is the tolerance test_gpu_bgk.py / test_gpu_kbc.py state for the reassociated forms over <= 20 steps.  Horizons stay
<= 12 iterations: the noisy state's KBC populations go negative soon after, velocity rows on small noisy boxes blow up
within a few hundred."""
import ctypes as ct

import numpy as np
import pytest
from conftest import relerr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import edge_reference as er  # noqa: E402
import pylbm  # noqa: E402
from gpu_util import bits_equal, dev, download_aos, upload_soa  # noqa: E402
from pylbm import _ptr  # noqa: E402

S2 = 1.0 / (0.5 + 3.0 * 1.70766666e-4)  # the shear driver's, ulbm_double_shear_flow.cpp:75-76
OMEGA = 1.3
UW = (0.04, 0.01)                       # both wall-velocity components live
REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
SENTINEL = 0x7FF8DEADBEEF5A5A           # a quiet NaN no kernel computes: "never written"
EPS = float(np.finfo(np.float64).eps)

# name -> (model number, library parameters, the reference's model, bitwise?)
FORMS = {
    "bgk_ref": (pylbm.MODEL_BGK, pylbm.BgkParams(OMEGA, 0, 0, form=REF), er.Bgk(OMEGA, 0, 0), True),
    "bgk_ref_delta": (pylbm.MODEL_BGK, pylbm.BgkParams(OMEGA, 0, 1, form=REF), er.Bgk(OMEGA, 0, 1), True),
    "bgk_ref_incomp": (pylbm.MODEL_BGK, pylbm.BgkParams(OMEGA, 1, 0, form=REF), er.Bgk(OMEGA, 1, 0), True),
    "bgk_ref_incomp_delta": (pylbm.MODEL_BGK, pylbm.BgkParams(OMEGA, 1, 1, form=REF), er.Bgk(OMEGA, 1, 1), True),
    "bgk_fast": (pylbm.MODEL_BGK, pylbm.BgkParams(OMEGA, 0, 0, form=FAST), er.Bgk(OMEGA, 0, 0), False),
    "kbc_ref": (pylbm.MODEL_KBC, pylbm.KbcParams(S2, form=REF), er.Kbc(S2), True),
    "kbc_fast": (pylbm.MODEL_KBC, pylbm.KbcParams(S2, form=FAST), er.Kbc(S2), False),
}


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


_STATES = {}


def state(oracle, R, C):
    """the noisy pre-collision lattice of a shape, computed once and never written"""
    if (R, C) not in _STATES:
        f = er.noisy_state(oracle, R, C, seed=1000 * R + C)
        f.setflags(write=False)
        _STATES[(R, C)] = f
    return _STATES[(R, C)]


def to_bc(e):
    return pylbm.Bc(row_lo=e.row_lo, row_hi=e.row_hi, col_lo=e.col_lo, col_hi=e.col_hi, uw_r=e.uw[0], uw_c=e.uw[1])


def mode_id(prefix):
    return lambda m: prefix + er.MODE_NAME[m]


def pair_id(prefix):
    return lambda p: prefix + er.MODE_NAME[p[0]] + "_" + er.MODE_NAME[p[1]]


def where(got, want):
    """the first differing (row, column, slot ...) entries with both values, for a failure message"""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64))
    return f"{bad.shape[0]} differ, first {[(tuple(b.tolist()), float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:4]]}"


def check(got, want, bitwise, what):
    if bitwise:
        assert bits_equal(got, want), f"{what}: {where(got, want)}"
    else:
        assert np.isfinite(got).all(), f"{what}: not finite"
        assert relerr(got, want) < 1e-12, f"{what}: relerr {relerr(got, want):.3e}"


class Stepper:
    """the raw entry points of one model / form on one geometry"""

    def __init__(self, lib, form, R, C):
        self.lib, self.g, self.R, self.C = lib, pylbm.Geom(R, C, 0), R, C
        self.model, self.prm, self.ref_model, self.bitwise = FORMS[form]
        self.kbc = self.model == pylbm.MODEL_KBC

    def collide(self, dst, src, bc):
        fn = self.lib.kbc_collide if self.kbc else self.lib.bgk_collide
        fn(_ptr(dst), _ptr(src), ct.byref(self.g), ct.byref(bc), ct.byref(self.prm), None, None, None)

    def step(self, dst, src, bc, rows=None, rho=None, u=None):
        r0, r1 = rows if rows is not None else (0, self.R)
        fn = self.lib.kbc_stream_collide if self.kbc else self.lib.bgk_stream_collide
        fn(_ptr(dst), _ptr(src), ct.byref(self.g), ct.byref(bc), ct.byref(self.prm), r0, r1, _ptr(rho), _ptr(u), None)

    def window(self, dst, src, bc, D):
        fn = self.lib.kbc_stream_collide_xn if self.kbc else self.lib.bgk_stream_collide_xn
        fn(_ptr(dst), _ptr(src), ct.byref(self.g), ct.byref(bc), ct.byref(self.prm), D, 0, self.R, None)

    def stream(self, dst, src, bc):
        self.lib.stream(_ptr(dst), _ptr(src), ct.byref(self.g), ct.byref(bc), None)


def sentinel_like(t):
    out = torch.empty_like(t)
    out.view(torch.int64).fill_(SENTINEL)
    return out


# ---- a. lbm_stream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C", [(7, 6), (16, 64)])
def test_stream_moves_every_population_of_every_edge_set(lib, oracle, R, C):
    """lbm_stream on a post-collision-like lattice, all 144 edge sets: bitwise, the anti-bounce-back term included (same
    operation order: (2 + 9 (c.u_w)^2 - 3 u_w.u_w) w_q, then -f + that)"""
    fc = state(oracle, R, C)
    g = pylbm.Geom(R, C, 0)
    p = upload_soa(lib, fc)
    out = torch.empty_like(p)
    for e in er.all_edges(uw=UW):
        bc = to_bc(e)
        out.zero_()
        lib.stream(_ptr(out), _ptr(p), ct.byref(g), ct.byref(bc), None)
        got = download_aos(lib, out)
        want = er.stream(fc, e)
        assert bits_equal(got, want), f"lbm_stream {R}x{C} {er.edges_name(e)}: {where(got, want)}"


# ---- b. single steps -------------------------------------------------------------------------------------------------------------
# 7x6: the generic kernel, every node through the gather; 16x64, 24x66: the fast kernel + the edge pass; 9x65: the generic
# kernel on a wide lattice (odd C)
@pytest.mark.parametrize("row_lo", er.ROW_MODES, ids=mode_id("row_lo_"))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("R,C", [(7, 6), (16, 64), (24, 66), (9, 65)])
def test_single_steps_of_every_edge_set(lib, oracle, R, C, form, row_lo):
    """collide, two fused stream + collide launches, stream: three driver iterations.  The resident post-collision lattice
    and the streamed state against the reference, 48 edge sets per case (mixed axes included)."""
    n = 3
    f0 = state(oracle, R, C)
    st = Stepper(lib, form, R, C)
    p0 = upload_soa(lib, f0)
    a, b, out = torch.empty_like(p0), torch.empty_like(p0), torch.empty_like(p0)
    for e in er.all_edges(uw=UW):
        if e.row_lo != row_lo:
            continue
        bc = to_bc(e)
        st.collide(a, p0, bc)
        for _ in range(n - 1):
            st.step(b, a, bc)
            a, b = b, a
        st.stream(out, a, bc)
        want = er.run(oracle, f0, n, e, st.ref_model)
        what = f"{form} {R}x{C} {er.edges_name(e)}"
        check(download_aos(lib, a), want["coll"], st.bitwise, what + " post-collision")
        check(download_aos(lib, out), want["f"], st.bitwise, what + " streamed")


@pytest.mark.parametrize("row_lo", er.ROW_MODES, ids=mode_id("row_lo_"))
@pytest.mark.parametrize("form", ["bgk_ref", "bgk_fast", "kbc_ref", "kbc_fast"])
@pytest.mark.parametrize("R,C", [(7, 6), (24, 66)])
def test_moments_and_row_ranges_of_every_edge_set(lib, oracle, R, C, form, row_lo):
    """One fused launch with the rho / u outputs: they are the moments of the STREAMED state at every node, wall and corner
    nodes included.  Then partial launches into lattices nobody wrote: a range that starts and ends on non-edge rows,
    row 0 alone, row R-1 alone (the edge pass gives the corners to its row lists) -- the rows of the range equal the whole
    launch, every other double stays untouched."""
    f0 = state(oracle, R, C)
    st = Stepper(lib, form, R, C)
    p0 = upload_soa(lib, f0)
    p1 = torch.empty_like(p0)
    st.collide(p1, p0, pylbm.Bc.periodic())   # node-local: the same for every edge set
    c1 = er.collide(oracle, f0, st.ref_model)
    check(download_aos(lib, p1), c1, st.bitwise, f"{form} {R}x{C} collide")
    rho = torch.empty((R, C), dtype=torch.float64, device=dev())
    u = torch.empty((2, R, C), dtype=torch.float64, device=dev())
    for e in er.all_edges(uw=UW):
        if e.row_lo != row_lo:
            continue
        bc = to_bc(e)
        what = f"{form} {R}x{C} {er.edges_name(e)}"
        f1 = er.stream(c1, e)
        want_rho, want_u = er.moments(oracle, f1, st.ref_model)
        want = er.collide(oracle, f1, st.ref_model)
        whole = sentinel_like(p0)
        rho.view(torch.int64).fill_(SENTINEL)
        u.view(torch.int64).fill_(SENTINEL)
        st.step(whole, p1, bc, rho=rho, u=u)
        got = download_aos(lib, whole)
        check(got, want, st.bitwise, what + " post-collision")
        check(rho.cpu().numpy(), want_rho, st.bitwise, what + " rho")
        check(u.cpu().numpy().transpose(1, 2, 0), want_u, st.bitwise, what + " u")
        for r0, r1 in ((2, R - 2), (0, 1), (R - 1, R)):
            part = sentinel_like(p0)
            rho.view(torch.int64).fill_(SENTINEL)
            u.view(torch.int64).fill_(SENTINEL)
            st.step(part, p1, bc, rows=(r0, r1), rho=rho, u=u)
            expect = sentinel_like(p0)
            expect[:, r0:r1] = whole[:, r0:r1]
            assert torch.equal(part.view(torch.int64), expect.view(torch.int64)), \
                f"{what} rows [{r0}, {r1}): {where(download_aos(lib, part), download_aos(lib, expect))}"
            inside = np.zeros((R, C), dtype=bool)
            inside[r0:r1] = True
            got_rho, got_u = rho.cpu().numpy(), u.cpu().numpy().transpose(1, 2, 0)
            check(got_rho[inside], want_rho[inside], st.bitwise, what + f" rho of rows [{r0}, {r1})")
            check(got_u[inside], want_u[inside], st.bitwise, what + f" u of rows [{r0}, {r1})")
            assert (got_rho[~inside].view(np.uint64) == SENTINEL).all() and (got_u[~inside].view(np.uint64) == SENTINEL).all(), \
                f"{what} rows [{r0}, {r1}): moments written outside the range"


# ---- c. windows ---------------------------------------------------------------------------------------------------------------
ROW_PAIRS = [(er.PERIODIC, er.PERIODIC)] + [(a, b) for a in (er.BOUNCE_BACK, er.ABB_VELOCITY) for b in (er.BOUNCE_BACK, er.ABB_VELOCITY)]
STRIP = 56   # output columns per wave of the 2..5-step windows


def window_shape(kind, D):
    """min: the smallest lattice the launcher accepts, all of it frame; split: one interior strip and R - 32 interior rows, so
    the frame / interior split is live; thin: an odd row count and a one-column last strip (C = 2 x 56 + 1; the launcher
    refuses C < 64, so 56 + 1 does not exist)"""
    return {"min": (4 * D + 8, 64), "split": (40, 150), "thin": (4 * D + 9, 2 * STRIP + 1)}[kind]


def run_windows(lib, oracle, form, D, kind, rows):
    R, C = window_shape(kind, D)
    f0 = state(oracle, R, C)
    st = Stepper(lib, form, R, C)
    p0 = upload_soa(lib, f0)
    p1, a, b, x, y = (torch.empty_like(p0) for _ in range(5))
    launches = 2
    try:
        for e in er.unmixed_wall_edges(uw=UW):
            if (e.row_lo, e.row_hi) != rows:
                continue
            bc = to_bc(e)
            what = f"{form} D={D} {R}x{C} {er.edges_name(e)}"
            st.collide(p1, p0, bc)
            want = er.run(oracle, f0, 1 + launches * D, e, st.ref_model)["coll"]
            want_dev = upload_soa(lib, want)
            singles = None
            if not st.bitwise:   # the same property as before: D steps in one launch == D single-step launches, bit for bit
                a.copy_(p1)
                for _ in range(launches * D):
                    st.step(b, a, bc)
                    a, b = b, a
                singles = a
                check(download_aos(lib, singles), want, False, what + " single steps")
            for split in (0, 1, 2):
                for sw_rows in (8, -1):
                    lib.set_tuning(b"sw_split", split)
                    lib.set_tuning(b"sw_rows", sw_rows)
                    x.copy_(p1)
                    y.zero_()
                    for _ in range(launches):
                        st.window(y, x, bc, D)
                        x, y = y, x
                    torch.cuda.synchronize()
                    tag = f"{what} sw_split={split} sw_rows={sw_rows}"
                    if st.bitwise:
                        assert torch.equal(x.view(torch.int64), want_dev.view(torch.int64)), f"{tag}: {where(download_aos(lib, x), want)}"
                    else:
                        assert torch.equal(x.view(torch.int64), singles.view(torch.int64)), \
                            f"{tag} against single steps: {where(download_aos(lib, x), download_aos(lib, singles))}"
                        check(download_aos(lib, x), want, False, tag)
    finally:
        lib.set_tuning(b"sw_split", -1)
        lib.set_tuning(b"sw_rows", -1)


@pytest.mark.parametrize("rows", ROW_PAIRS, ids=pair_id("rows_"))
@pytest.mark.parametrize("form", ["bgk_ref", "bgk_ref_incomp_delta", "bgk_fast"])
@pytest.mark.parametrize("kind", ["min", "split", "thin"])
@pytest.mark.parametrize("D", [2, 3, 4, 5])
def test_bgk_windows_against_the_reference(lib, oracle, D, kind, form, rows):
    """lbm_bgk_stream_collide_xn, two launches of D steps on the 24 unmixed wall sets, every frame / interior split and both
    chunk heights, against the REFERENCE after 1 + 2 D iterations (not against single steps, which read the same fix-ups)."""
    run_windows(lib, oracle, form, D, kind, rows)


@pytest.mark.parametrize("rows", ROW_PAIRS, ids=pair_id("rows_"))
@pytest.mark.parametrize("kind", ["min", "split", "thin"])
@pytest.mark.parametrize("D", [2, 3])
def test_kbc_windows_against_the_reference(lib, oracle, D, kind, rows):
    """lbm_kbc_stream_collide_xn (reassociated collision) the same way: bounce-back, specular and velocity edges"""
    run_windows(lib, oracle, "kbc_fast", D, kind, rows)


@pytest.mark.parametrize("R,C", [(24, 64), (40, 2 * STRIP + 1)])
def test_periodic_kbc_window_ring_in_registers_and_in_lds(lib, oracle, R, C):
    """the periodic KBC window keeps its ring in wave-private LDS (sw_ldsring = 1, the default) or in registers (0): both
    instantiations, D = 2, 3, 4, two launches -- equal to each other and to single steps bit for bit, and to the reference"""
    f0 = state(oracle, R, C)
    st = Stepper(lib, "kbc_fast", R, C)
    bc = pylbm.Bc.periodic()
    p0 = upload_soa(lib, f0)
    p1, a, b, x, y = (torch.empty_like(p0) for _ in range(5))
    st.collide(p1, p0, bc)
    try:
        for D in (2, 3, 4):
            a.copy_(p1)
            for _ in range(2 * D):
                st.step(b, a, bc)
                a, b = b, a
            want = er.run(oracle, f0, 1 + 2 * D, er.Edges(), st.ref_model)["coll"]
            check(download_aos(lib, a), want, False, f"kbc {R}x{C} {2 * D} single steps")
            for ring in (0, 1):
                lib.set_tuning(b"sw_ldsring", ring)
                x.copy_(p1)
                y.zero_()
                for _ in range(2):
                    st.window(y, x, bc, D)
                    x, y = y, x
                torch.cuda.synchronize()
                assert torch.equal(x.view(torch.int64), a.view(torch.int64)), \
                    f"kbc {R}x{C} D={D} sw_ldsring={ring}: {where(download_aos(lib, x), download_aos(lib, a))}"
    finally:
        lib.set_tuning(b"sw_ldsring", -1)


MIXED = [er.Edges(er.BOUNCE_BACK, er.PERIODIC, er.PERIODIC, er.PERIODIC, UW),
         er.Edges(er.PERIODIC, er.ABB_VELOCITY, er.PERIODIC, er.PERIODIC, UW),
         er.Edges(er.PERIODIC, er.PERIODIC, er.BOUNCE_BACK, er.PERIODIC, UW),
         er.Edges(er.PERIODIC, er.PERIODIC, er.PERIODIC, er.SPECULAR, UW),
         er.Edges(er.ABB_VELOCITY, er.PERIODIC, er.SPECULAR, er.SPECULAR, UW),
         er.Edges(er.PERIODIC, er.BOUNCE_BACK, er.SPECULAR, er.PERIODIC, UW)]


@pytest.mark.parametrize("form", ["bgk_ref", "bgk_fast", "kbc_ref", "kbc_fast"])
def test_solver_with_a_mixed_axis_against_the_reference(lib, oracle, form):
    """lbm_solver_step with a wall on one side of an axis and PERIODIC on the other (the windows refuse it, the context falls
    back to single steps): 7 driver iterations and the recorded moments against the reference"""
    R, C, n = 40, 150, 7
    f0 = state(oracle, R, C)
    model, prm, ref_model, bitwise = FORMS[form]
    for e in MIXED:
        sv = pylbm.Solver(lib, model, R, C, prm, bc=to_bc(e))
        try:
            sv.set_f(f0)
            sv.step(n, record_moments=True)
            got = sv.get_f()
            rho, u = sv.moments()
        finally:
            sv.close()
        what = f"{form} {er.edges_name(e)}"
        check(got, er.run(oracle, f0, n, e, ref_model)["f"], bitwise, what + " f")
        before = er.run(oracle, f0, n - 1, e, ref_model)   # the drivers' tensors: the moments at the top of iteration n
        check(rho, before["rho"], bitwise, what + " rho")
        check(u, before["u"], bitwise, what + " u")


# ---- d. mass in sealed boxes -------------------------------------------------------------------------------------------------
SEALED = {
    "closed_box": er.Edges(er.BOUNCE_BACK, er.BOUNCE_BACK, er.BOUNCE_BACK, er.BOUNCE_BACK),
    "bb_rows_specular_cols": er.Edges(er.BOUNCE_BACK, er.BOUNCE_BACK, er.SPECULAR, er.SPECULAR),
    "bb_rows_periodic_cols": er.Edges(er.BOUNCE_BACK, er.BOUNCE_BACK, er.PERIODIC, er.PERIODIC),
    "periodic_rows_bb_specular_cols": er.Edges(er.PERIODIC, er.PERIODIC, er.BOUNCE_BACK, er.SPECULAR),
}
MASS_CASES = [(24, 64, k) for k in SEALED] + [(96, 150, "closed_box")]


@pytest.mark.parametrize("R,C,edges", MASS_CASES, ids=[f"{r}x{c}_{k}" for r, c, k in MASS_CASES])
@pytest.mark.parametrize("model", ["bgk", "kbc"])
def test_sealed_boxes_keep_their_mass(lib, oracle, model, R, C, edges):
    """Bounce-back and specular edges move populations and create none, so the sum of all populations of a sealed box only
    drifts by rounding.  pylbm.Solver with its default launches (fused windows) and the default (reassociated) form, 200
    steps; BGK omega = 1.3 from the noisy state, KBC from the smooth shear layer.  The bar is not a number chosen here:
    8 x the relative drift of the numpy reference on the same case and steps (the factor covers the different rounding of
    the reassociated forms), with a floor of 64 eps = 1.4e-14; the sums are taken on the host in extended precision.  A
    single mis-routed population at one corner node leaks >= 1e-6 of the mass per step.

    Measured on an MI355X, relative drift after 200 steps (the numpy reference's in brackets):
      BGK  24x64 closed box 3.31e-14 (1.55e-14), bounce-back rows + specular columns 3.31e-14 (1.55e-14), bounce-back rows +
           periodic columns 3.33e-14 (1.54e-14), periodic rows + bounce-back / specular columns 3.31e-14 (1.55e-14);
           96x150 closed box 3.32e-14 (1.54e-14) -- bar 1.2e-13;
      KBC  the same five cases 9.8e-17 (3.0e-18), 2.4e-17 (8.5e-18), 5.7e-17 (2.2e-18), 4.4e-17 (6.8e-18), 1.4e-17 (7.8e-18)
           -- bar 64 eps = 1.4e-14."""
    steps = 200
    e = SEALED[edges]
    if model == "bgk":
        f0 = state(oracle, R, C)
        lib_model, prm, ref_model = pylbm.MODEL_BGK, pylbm.BgkParams(OMEGA, 0), er.Bgk(OMEGA)
    else:
        f0 = oracle.kbc_equilibrium(*oracle.kbc_shear_init(R, C))
        lib_model, prm, ref_model = pylbm.MODEL_KBC, pylbm.KbcParams(S2), er.Kbc(S2)
    sv = pylbm.Solver(lib, lib_model, R, C, prm, bc=to_bc(e))
    try:
        sv.set_f(f0)
        sv.step(steps)
        got = sv.get_f()
    finally:
        sv.close()
    assert np.isfinite(got).all()
    ref_drift = er.relative_mass_drift(er.run(oracle, f0, steps, e, ref_model)["f"], f0)
    drift = er.relative_mass_drift(got, f0)
    limit = max(8.0 * ref_drift, 64.0 * EPS)
    print(f"mass drift {model} {R}x{C} {edges}: gpu {drift:.3e}, reference {ref_drift:.3e}, limit {limit:.3e}")
    assert drift <= limit, f"{model} {R}x{C} {edges}: relative mass drift {drift:.3e} after {steps} steps, reference {ref_drift:.3e}, limit {limit:.3e}"
