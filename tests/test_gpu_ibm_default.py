"""GPU tests of the immersed boundary in the DEFAULT form (the reassociated collision: what the benchmark runs), tied
bitwise link by link -- the forcing has no forms, only the collision differs:

1. the solver's single steps (ibm_depth = 1: forcing on the side stream, the gate, the split source) equal a plain loop of
   the operators on one stream: lbm_bgk_collide, then lbm_bgk_stream_collide over all rows + lbm_ibm_step;
2. in that loop the forcing equals the oracle's on the very moments the default-form collision wrote, and the lattice
   after the source term is the lattice before plus the numpy source term (tests/test_gpu_collision_accuracy.py bounds
   the collision itself, the delta form and the streamed call included);
3. every launch variant -- bands, boxes and their switches, slab layouts and slab block forms, the ring wrappers --
   equals those single steps, with the block counts of the reference order;
4. the qualification bounds of solver_ibm_block, each met exactly and missed by one, in both forms;
5. a solver whose boundary is replaced by a larger and then a smaller one.
The reference-order arms are compared with the oracle, the default-form arms with their own single steps."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ibm_util as iu  # noqa: E402
import pylbm  # noqa: E402
import test_gpu_ibm as base  # noqa: E402
from gpu_util import bits_equal, dev, download_aos, ulp_diff, upload_soa  # noqa: E402
from pylbm import _ptr  # noqa: E402

OMEGA, U_IN, GUO_A, GUO_B = 1.0 / 0.55, 0.05, 1.0 / 3.0, 1.0 / 9.0
DEFAULT, REFERENCE = pylbm.FORM_DEFAULT, pylbm.FORM_REFERENCE_ORDER
FORM_IDS = {DEFAULT: "default", REFERENCE: "reference_order"}


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1
    return lib


def start_state(oracle, X, Y):
    """a pre-collision state that is no fixed point of anything: the equilibrium of a wavy flow"""
    rr, cc = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    u0 = np.stack([U_IN + 0.01 * np.sin(rr / 5.0 + cc / 7.0), 0.008 * np.cos(rr / 6.0 - cc / 4.0)], axis=-1)
    rho0 = 1 + 0.02 * np.sin((rr + 2 * cc) / 9.0)
    return oracle.incomp_equilibrium(u0, rho0)


def single_steps(lib, x, y, f0, form, checkpoints, record_moments=False):
    """the solver under ibm_depth = 1, stepped from checkpoint to checkpoint: {n: (f, rho, u, surface force)}"""
    X, Y = f0.shape[:2]
    out, done = {}, 0
    try:
        lib.set_tuning(b"ibm_depth", 1)
        sv, ib = iu.cylinder_solver(lib, X, Y, OMEGA, U_IN, x, y, form=form)
        sv.set_f(f0)
        for n in checkpoints:
            sv.step(n - done, record_moments=record_moments)
            done = n
            rho, u = sv.moments() if record_moments else (None, None)
            out[n] = (sv.get_f(), rho, u, ib.surface_force())
        assert int(lib.raw.lbm_solver_block_launches(sv.h)) == 0
        sv.close(); ib.close()
    finally:
        lib.set_tuning(b"ibm_depth", -1)
    return out


def operator_steps(lib, oracle, x, y, f0, checkpoints, probes=()):
    """The plain loop on one stream, form = REASSOCIATED and delta_form = 1: lbm_bgk_collide first, then
    lbm_bgk_stream_collide over all rows with moments, each followed by lbm_ibm_step.  At the steps in `probes` the forcing
    is pinned on the moments the collision wrote: lbm_ibm_force's F against oracle.ibm_force, the lattice after the source
    against the lattice before plus the numpy source term.  {n: (f, rho, u, surface force)}"""
    X, Y = f0.shape[:2]
    prm = pylbm.BgkParams(OMEGA, 0, 1, form=pylbm.FORM_REASSOCIATED)
    bc, flat = iu.cylinder_bc(U_IN), pylbm.Geom(X, Y, 0)
    ib = pylbm.Ibm(lib, x, y, X, Y)
    roi = ib.roi()
    lat = [upload_soa(lib, f0), torch.empty((9, X, Y), dtype=torch.float64, device=dev())]
    rho = torch.empty((X, Y), dtype=torch.float64, device=dev())
    u = torch.empty((2, X, Y), dtype=torch.float64, device=dev())
    F = torch.empty((2, roi[1] - roi[0], roi[3] - roi[2]), dtype=torch.float64, device=dev())
    streamed = torch.empty_like(lat[0])
    out, cur = {}, 0
    for n in range(1, max(checkpoints) + 1):
        if n == 1:
            lib.bgk_collide(_ptr(lat[1]), _ptr(lat[0]), ct.byref(flat), ct.byref(bc), ct.byref(prm), _ptr(rho), _ptr(u), None)
        else:
            lib.bgk_stream_collide(_ptr(lat[cur ^ 1]), _ptr(lat[cur]), ct.byref(flat), ct.byref(bc), ct.byref(prm), 0, X,
                                   _ptr(rho), _ptr(u), None)
        cur ^= 1
        if n in probes:
            u_h, rho_h, before = download_aos(lib, u), download_aos(lib, rho), download_aos(lib, lat[cur])
            lib.ibm_force(ib.h, _ptr(u), _ptr(rho), _ptr(F), None)
            got_F, want_F = download_aos(lib, F), oracle.ibm_force(x, y, u_h, rho_h)
            assert np.abs(want_F).max() > 1e-4
            assert bits_equal(got_F, want_F), (n, ulp_diff(got_F, want_F))
        lib.ibm_step(ib.h, _ptr(lat[cur]), ct.byref(flat), _ptr(u), _ptr(rho), ct.c_double(OMEGA), ct.c_double(GUO_A),
                     ct.c_double(GUO_B), None)
        if n in probes:
            after, want = download_aos(lib, lat[cur]), iu.add_source(before, roi, u_h, want_F, OMEGA, GUO_A, GUO_B)
            assert not bits_equal(after, before)
            assert bits_equal(after, want), (n, ulp_diff(after, want))
        if n in checkpoints:
            lib.stream(_ptr(streamed), _ptr(lat[cur]), ct.byref(flat), ct.byref(bc), None)
            out[n] = (download_aos(lib, streamed), download_aos(lib, rho), download_aos(lib, u), ib.surface_force())
    ib.close()
    return out


# ---- 1., 2. single steps against the operators; the forcing on default-form moments -----------------------------------------
@pytest.mark.parametrize("X,Y", [(88, 80), (72, 51)])     # the fast kernel + edge pass, and the generic kernel
def test_default_form_single_steps_equal_the_operators(lib, oracle, X, Y):
    steps = (1, 2, 5, 13)
    x, y = iu.circle(X * 0.4 + 0.3, Y / 2.0 - 0.4, 6.0)
    f0 = start_state(oracle, X, Y)
    ops = operator_steps(lib, oracle, x, y, f0, steps, probes=(1, 5))
    overlap = single_steps(lib, x, y, f0, DEFAULT, steps)                        # the side stream, the gate, the split source
    recorded = single_steps(lib, x, y, f0, DEFAULT, steps, record_moments=True)  # each call's last step on one stream
    named = single_steps(lib, x, y, f0, pylbm.FORM_REASSOCIATED, steps)
    in_order = single_steps(lib, x, y, f0, REFERENCE, (13,))
    assert not bits_equal(in_order[13][0], ops[13][0])                          # (it really is the other operation order)
    for n in steps:
        f, rho, u, Fs = ops[n]
        assert bits_equal(overlap[n][0], f), (n, ulp_diff(overlap[n][0], f))
        assert np.array_equal(overlap[n][3], Fs), n
        assert bits_equal(recorded[n][0], f), (n, ulp_diff(recorded[n][0], f))
        assert bits_equal(recorded[n][1], rho) and bits_equal(recorded[n][2], u), n
        assert np.array_equal(recorded[n][3], Fs), n
        assert bits_equal(named[n][0], f) and np.array_equal(named[n][3], Fs), n


# ---- 3. every launch variant equals the default-form single steps -------------------------------------------------------------
@pytest.mark.parametrize("cx_frac", [0.5, 0.12])
def test_forced_band_blocks_equal_single_steps_in_the_default_form(lib, oracle, cx_frac):
    """test_forced_band_blocks_equal_single_steps with the reassociated collision: depths 5 and 3 (and the fallback next to the
    inlet) against depth 1, bit for bit, the surface force included; the same blocks as in the reference order"""
    res, (x, y, f0, omega, u_in) = base._band_runs(lib, oracle, cx_frac, DEFAULT)
    f1, Fs1, blocks1 = res[1]
    assert blocks1 == 0
    for depth in (5, 3):
        f, Fs, blocks = res[depth]
        assert blocks == iu.expected_blocks(160, 128, iu.roi_of(x, y), 13, max_depth=depth) > 0, (depth, blocks)
        assert bits_equal(f, f1), (depth, ulp_diff(f, f1))
        assert np.array_equal(Fs, Fs1), depth


_box_single_steps = {}


@pytest.mark.parametrize("tune,cy_frac", base.BOX_VARIANTS)
def test_forced_box_variants_equal_single_steps_in_the_default_form(lib, oracle, tune, cy_frac):
    """the ten tunings of test_forced_box_variants_equal_the_oracle with the reassociated collision, against ibm_depth = 1"""
    (f, Fs, blocks), (x, y, f0, omega, u_in) = base._box_variant_run(lib, oracle, tune, cy_frac, DEFAULT)
    if cy_frac not in _box_single_steps:
        _box_single_steps[cy_frac] = single_steps(lib, x, y, f0, DEFAULT, (16,))[16]
    f1, _, _, Fs1 = _box_single_steps[cy_frac]
    assert blocks == 3, blocks
    assert bits_equal(f, f1), ulp_diff(f, f1)
    assert np.array_equal(Fs, Fs1)


@pytest.mark.parametrize("case", base.SLAB_LAYOUTS)
def test_cylinder_blocks_over_slabs_equal_single_steps_in_the_default_form(lib, oracle, case):
    """the six slab layouts with the reassociated collision; the one-block yardstick runs single steps (ibm_depth = 1)"""
    base._slab_layout_check(lib, oracle, case, DEFAULT, yardstick_depth=1)


@pytest.mark.parametrize("case,tunes", base.SLAB_FORMS, ids=base.SLAB_FORM_IDS)
def test_cylinder_slab_block_forms_equal_single_steps_in_the_default_form(lib, oracle, case, tunes):
    base._slab_form_check(lib, oracle, case, tunes, DEFAULT, yardstick_depth=1)


def test_ring_ibm_block_wrappers_on_a_self_ring_in_the_default_form(lib, oracle):
    base._self_ring_run(lib, oracle, DEFAULT)


# ---- 4. the qualification bounds of solver_ibm_block --------------------------------------------------------------------------
# One marker (a 5 x 5 ROI: rows [fx - 2, fx + 3), columns [fy - 2, fy + 3)) on the smallest lattices that take a depth-5
# block, 16 steps in one call = 1 + 15.  D = 5 needs q0 - 10 >= 2 and q1 + 10 <= R - 2, hence R >= 29 with 5 ROI rows: on
# 29 rows both row bounds are met exactly at once, on 30 rows one at a time.  Missing a bound by one leaves the 15 steps to
# single steps -- except that the LAST four then fit a depth-4 block (q0 - 8 >= 2), so the count on that side is 1, not 0;
# only a width below 64 refuses every depth.  "R >= 4 D + 8" can never decide: the two row bounds already need R >= 4 D + 9
# (on 28 rows no depth-5 block fits, and on 27 lbm_solver_step itself steps down to depth 4).
# (name, R, C, fx, fy, blocks, takes the box at depth 5)
BOUNDS = [
    ("rows_both_exact",      29, 64, 14, 30, 3, True),    # q0 - 2D = 2 and q1 + 2D = R - 2
    ("q0_exact",             30, 64, 14, 30, 3, True),    # q0 - 2D = 2
    ("q0_one_short",         30, 64, 13, 30, 1, None),    # q0 - 2D = 1
    ("q1_exact",             30, 64, 15, 30, 3, True),    # q1 + 2D = R - 2
    ("q1_one_over",          30, 64, 16, 30, 1, None),    # q1 + 2D = R - 1
    ("rows_4D_plus_8",       28, 64, 13, 30, 1, None),    # R = 4D + 8: no place for a depth-5 block
    ("rows_4D_plus_7",       27, 64, 13, 30, 4, None),    # one less: depth 4 from the start (4 + 4 + 4 + 3)
    ("cols_63",              29, 63, 14, 30, 0, None),    # C = 63 (C = 64: rows_both_exact)
    ("box_c0_exact",         29, 64, 14, 20, 3, True),    # c0 - 2D = 8: the box
    ("band_c0_one_short",    29, 64, 14, 19, 3, False),   # c0 - 2D = 7: the band
    ("box_bc1_exact",        29, 65, 14, 47, 3, True),    # bc1 = 64 = C - 1: the box
    ("band_bc1_one_over",    29, 64, 14, 47, 3, False),   # bc1 = 64 = C: the band
]


@pytest.mark.parametrize("form", [REFERENCE, DEFAULT], ids=FORM_IDS.get)
@pytest.mark.parametrize("name,R,C,fx,fy,want_blocks,box", BOUNDS, ids=[b[0] for b in BOUNDS])
def test_block_qualification_bounds(lib, oracle, name, R, C, fx, fy, want_blocks, box, form):
    x, y = np.array([fx + 0.3]), np.array([fy + 0.6])
    roi = iu.roi_of(x, y)
    assert roi == (fx - 2, fx + 3, fy - 2, fy + 3)
    assert iu.expected_blocks(R, C, roi, 16) == want_blocks                 # the table above is the rule's
    if box is not None:
        assert iu.block_qualifies(R, C, roi, 5) and iu.takes_the_box(C, roi, 5) == box
    else:
        assert not iu.block_qualifies(R, C, roi, 5)
    f0 = start_state(oracle, R, C)
    sv, ib = iu.cylinder_solver(lib, R, C, OMEGA, U_IN, x, y, form=form)
    sv.set_f(f0)
    sv.step(16)
    f, Fs, blocks = sv.get_f(), ib.surface_force(), int(lib.raw.lbm_solver_block_launches(sv.h))
    sv.close(); ib.close()
    assert blocks == want_blocks, blocks
    if form == REFERENCE:
        fo, uo, rhoo, Fso = oracle.cylinder_steps(x, y, f0, OMEGA, U_IN, 16)
        assert bits_equal(f, fo), ulp_diff(f, fo)
        assert np.allclose(Fs, Fso, rtol=1e-11, atol=1e-16)
    else:
        f1, _, _, Fs1 = single_steps(lib, x, y, f0, DEFAULT, (16,))[16]
        assert bits_equal(f, f1), ulp_diff(f, f1)
        assert np.array_equal(Fs, Fs1)


# ---- 5. re-attaching ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REFERENCE, DEFAULT], ids=FORM_IDS.get)
def test_reattached_boundaries(lib, oracle, form):
    """One solver: a small boundary for 6 steps, a larger one (the forced box is reallocated), the small one again (the box
    is now larger than needed and keeps the larger plane stride), 6 steps each, one depth-5 block per call."""
    X, Y = 88, 88
    small, large = iu.circle(44.3, 43.6, 4.0), iu.circle(43.7, 44.2, 9.0)
    f0 = start_state(oracle, X, Y)

    def run(depth):
        try:
            if depth is not None:
                lib.set_tuning(b"ibm_depth", depth)
            prm = pylbm.BgkParams(OMEGA, 0, 1, form=form)
            sv = pylbm.Solver(lib, pylbm.MODEL_BGK, X, Y, prm, bc=iu.cylinder_bc(U_IN))
            sv.set_f(f0)
            fs, Fss, ibs = [], [], []
            for x, y in (small, large, small):
                ibs.append(pylbm.Ibm(lib, x, y, X, Y))
                sv.attach_ibm(ibs[-1])
                sv.step(6)
                fs.append(sv.get_f()); Fss.append(ibs[-1].surface_force())
            blocks = int(lib.raw.lbm_solver_block_launches(sv.h))
            sv.close()
            for ib in ibs:
                ib.close()
        finally:
            lib.set_tuning(b"ibm_depth", -1)
        return fs, Fss, blocks

    for x, y in (small, large):
        assert iu.block_qualifies(X, Y, iu.roi_of(x, y), 5) and iu.takes_the_box(Y, iu.roi_of(x, y), 5)
    fs, Fss, blocks = run(None)
    assert blocks == 3, blocks
    if form == REFERENCE:
        f = f0
        for k, (x, y) in enumerate((small, large, small)):
            f, uo, rhoo, Fso = oracle.cylinder_steps(x, y, f, OMEGA, U_IN, 6)
            assert bits_equal(fs[k], f), (k, ulp_diff(fs[k], f))
            assert np.allclose(Fss[k], Fso, rtol=1e-11, atol=1e-16), k
    else:
        f1, Fs1, blocks1 = run(1)
        assert blocks1 == 0
        for k in range(3):
            assert bits_equal(fs[k], f1[k]), (k, ulp_diff(fs[k], f1[k]))
            assert np.array_equal(Fss[k], Fs1[k]), k
