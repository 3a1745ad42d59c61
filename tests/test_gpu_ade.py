"""GPU suite, fluid + transported scalar (lbm_ade_*, capi_ade.hip): the sediment loop of
test/rectangle_sedimentation_test.cpp:88-247 without its driver-specific edges -- a compressible BGK fluid f and a
second D2Q9 distribution g with equilibrium(g_equi, u + w, C), its own BGK rate, streamed like f.

The yardstick is the reference's loop composed from the oracle's solver:: primitives (pinned to the unmodified
reference by tests/golden/solver_units.npz, tests/test_oracle_golden.py):
    rho = calc_rho(f); u = calc_u(f, rho); C = calc_rho(g)
    f_equi = equilibrium(u, rho); g_equi = equilibrium(u + w, C)
    f_coll = collision(f, f_equi, omega); g_coll = collision(g, g_equi, omega_g)
    f = advect(f_coll); g = advect(g_coll)          (+ the halfway wall fix-ups on both, see _walls)
In the reference operation order the fused step is compared BITWISE with it."""
import ctypes as ct

import numpy as np
import pytest
from conftest import relerr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
from ade_calls import collide, step_into  # noqa: E402
from ade_util import W, assert_state_bits, initial_state  # noqa: E402
from gpu_util import bits_equal, dev, download_aos, upload_soa  # noqa: E402
from proc_util import key_values, run_driver  # noqa: E402
from pylbm import _ptr  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


def _walls(bc):
    """numpy restatement of the halfway wall fix-ups (d2q9.hpp gather_bc): rows first, columns win at the corners;
    applied to BOTH distributions, each from its own post-collision populations"""
    def fix(a, coll):
        if bc.row_lo == pylbm.EDGE_BOUNCE_BACK:
            a[0, :, 1], a[0, :, 5], a[0, :, 8] = coll[0, :, 3], coll[0, :, 7], coll[0, :, 6]
        if bc.row_hi == pylbm.EDGE_BOUNCE_BACK:
            a[-1, :, 3], a[-1, :, 7], a[-1, :, 6] = coll[-1, :, 1], coll[-1, :, 5], coll[-1, :, 8]
        if bc.col_hi == pylbm.EDGE_BOUNCE_BACK:
            a[:, -1, 4], a[:, -1, 7], a[:, -1, 8] = coll[:, -1, 2], coll[:, -1, 5], coll[:, -1, 6]
        elif bc.col_hi == pylbm.EDGE_SPECULAR:
            a[:, -1, 4], a[:, -1, 7], a[:, -1, 8] = coll[:, -1, 2], coll[:, -1, 6], coll[:, -1, 5]
        if bc.col_lo == pylbm.EDGE_BOUNCE_BACK:
            a[:, 0, 2], a[:, 0, 5], a[:, 0, 6] = coll[:, 0, 4], coll[:, 0, 7], coll[:, 0, 8]
        elif bc.col_lo == pylbm.EDGE_SPECULAR:
            a[:, 0, 2], a[:, 0, 5], a[:, 0, 6] = coll[:, 0, 4], coll[:, 0, 8], coll[:, 0, 7]
    return fix


def oracle_loop(orc, f, g, omega, omega_g, w, n, bc=None):
    fix = _walls(bc) if bc is not None else None
    for _ in range(n):
        rho = orc.calc_rho(f)
        u = orc.calc_u(f, rho)
        conc = orc.calc_rho(g)
        fe = orc.equilibrium(u, rho)
        ge = orc.equilibrium(u + np.asarray(w), conc)
        fc = orc.collision(f, fe, omega)
        gc = orc.collision(g, ge, omega_g)
        f, g = orc.advect(fc), orc.advect(gc)
        if fix:
            fix(f, fc)
            fix(g, gc)
    rho = orc.calc_rho(f)
    return dict(f=f, g=g, rho=rho, u=orc.calc_u(f, rho), C=orc.calc_rho(g))


def ade(lib, R, C, omega, omega_g, w, form, bc=None, stream=None):
    return pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(omega, 0, form=form), pylbm.AdeParams(omega_g, w, form=form),
                           bc=bc, stream=stream)


@pytest.mark.parametrize("R,C", [(96, 70), (1024, 1024)])
def test_reference_order_periodic_is_the_reference_loop_bit_for_bit(lib, oracle, R, C):
    """1, 2 and 37 driver iterations on a periodic box (1024 x 1024: padded rows and planes) == the oracle loop"""
    f0, g0 = initial_state(oracle, R, C)
    sv = ade(lib, R, C, 1.2, 1.7, W, REF)
    if C == 1024:
        assert sv.lattices()[4].row_pitch > C  # the padded layout is what is exercised
    sv.set_state(f0, g0)
    done, want = 0, dict(f=f0, g=g0)
    for n in (1, 2, 37):
        sv.step(n - done)
        want = oracle_loop(oracle, want["f"], want["g"], 1.2, 1.7, W, n - done)
        done = n
        assert_state_bits(sv.get_state(), want, f"{R}x{C} after {n} steps")
    sv.close()


@pytest.mark.parametrize("walls", ["bb_cols", "bb_rows_specular_cols"])
def test_walls_are_the_reference_fixups_on_both_distributions(lib, oracle, walls):
    """halfway bounce-back / specular walls: g takes the fix-up f takes (a no-flux wall), bit for bit"""
    R, C = 80, 102
    if walls == "bb_cols":
        bc = pylbm.Bc(col_lo=pylbm.EDGE_BOUNCE_BACK, col_hi=pylbm.EDGE_BOUNCE_BACK)
    else:
        bc = pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK, col_lo=pylbm.EDGE_SPECULAR,
                      col_hi=pylbm.EDGE_SPECULAR)
    f0, g0 = initial_state(oracle, R, C, seed=3)
    sv = ade(lib, R, C, 1.2, 1.7, W, REF, bc=bc)
    sv.set_state(f0, g0)
    sv.step(23)
    assert_state_bits(sv.get_state(), oracle_loop(oracle, f0, g0, 1.2, 1.7, W, 23, bc=bc), walls)
    sv.close()


def test_raw_entry_points_with_moments(lib, oracle):
    """lbm_ade_collide + lbm_ade_stream_collide on dense lattices: the moments they write are the reference's
    rho, u, C of the streamed state (the next iteration's calc_rho / calc_u / calc_rho(g))"""
    R, C = 64, 130
    bc = pylbm.Bc(col_lo=pylbm.EDGE_BOUNCE_BACK, col_hi=pylbm.EDGE_SPECULAR)
    f0, g0 = initial_state(oracle, R, C, seed=5)
    geo = pylbm.Geom(R, C, 0)
    fl, sc = pylbm.BgkParams(1.3, 0, form=REF), pylbm.AdeParams(0.9, (2e-3, -1e-3), form=REF)
    fa, ga = upload_soa(lib, f0), upload_soa(lib, g0)
    fb, gb = torch.empty_like(fa), torch.empty_like(ga)
    rho = torch.empty((R, C), dtype=torch.float64, device=dev())
    u = torch.empty((2, R, C), dtype=torch.float64, device=dev())
    conc = torch.empty((R, C), dtype=torch.float64, device=dev())
    collide(lib, "", geo, bc, (fl, sc), (fb, gb), (fa, ga), moments=(rho, u, conc))
    torch.cuda.synchronize()
    want0 = oracle_loop(oracle, f0, g0, 1.3, 0.9, (2e-3, -1e-3), 0)
    assert bits_equal(rho.cpu().numpy(), want0["rho"]) and bits_equal(conc.cpu().numpy(), want0["C"])
    for _ in range(6):
        step_into(lib, "", geo, bc, (fl, sc), (fa, ga), (fb, gb), moments=(rho, u, conc))
        fa, fb, ga, gb = fb, fa, gb, ga
    torch.cuda.synchronize()
    want = oracle_loop(oracle, f0, g0, 1.3, 0.9, (2e-3, -1e-3), 6, bc=bc)
    assert bits_equal(rho.cpu().numpy(), want["rho"])
    assert bits_equal(np.moveaxis(u.cpu().numpy(), 0, -1), want["u"])
    assert bits_equal(conc.cpu().numpy(), want["C"])


@pytest.mark.parametrize("form", [REF, FAST])
@pytest.mark.parametrize("walls", [False, True])
def test_the_fluid_is_the_existing_bgk_fluid(lib, oracle, form, walls):
    """200 iterations: f of the ADE context == lbm_solver BGK with the same bc and parameters, bit for bit, in both
    forms; rho, u == the BGK solver's recorded moments of the same f_adve (reference order) / calc_rho, calc_u of its f
    (reassociated: the BGK solver records the reassociated moments, the ADE context returns the reference's calc_rho /
    calc_u).  The BGK solver records the moments its loop computes at the TOP of an iteration (the Poiseuille drivers'
    order), the sediment loop at the END (:199-200, :237): one more recorded iteration lines them up."""
    R, C = 96, 160
    bc = pylbm.Bc(col_lo=pylbm.EDGE_BOUNCE_BACK, col_hi=pylbm.EDGE_BOUNCE_BACK) if walls else pylbm.Bc.periodic()
    f0, g0 = initial_state(oracle, R, C, seed=7)
    sv = ade(lib, R, C, 1.2, 1.7, W, form, bc=bc)
    sv.set_state(f0, g0)
    sv.step(200)
    got = sv.get_state()
    sv.close()
    bgk = pylbm.Solver(lib, pylbm.MODEL_BGK, R, C, pylbm.BgkParams(1.2, 0, form=form), bc=bc)
    bgk.set_f(f0)
    bgk.step(200)
    f_bgk = bgk.get_f()
    bgk.step(1, record_moments=True)   # records the moments at the top of its iteration 201: those of f_adve(200)
    rho_b, u_b = bgk.moments()
    bgk.close()
    assert bits_equal(got["f"], f_bgk)
    if form == REF:
        assert bits_equal(got["rho"], rho_b) and bits_equal(got["u"], u_b)
    else:
        rho_o = oracle.calc_rho(f_bgk)
        assert bits_equal(got["rho"], rho_o) and bits_equal(got["u"], oracle.calc_u(f_bgk, rho_o))


def test_reassociated_form_agrees_with_the_reference_order(lib, oracle):
    """500 iterations, stated tolerance 1e-10 relative (to the field's largest magnitude), fixed before measuring.
    Measured on MI355X: f 6.1e-14, g 1.3e-13, rho 6.0e-14, u 7.3e-13, C 1.3e-13.  This guards the trajectory; the accuracy
    of one collision of either half is bounded per population in units in the last place by
    tests/test_gpu_collision_accuracy.py."""
    R, C = 128, 192
    bc = pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK)
    f0, g0 = initial_state(oracle, R, C, seed=11)
    out = {}
    for form in (REF, FAST):
        sv = ade(lib, R, C, 1.2, 1.7, W, form, bc=bc)
        sv.set_state(f0, g0)
        sv.step(500)
        out[form] = sv.get_state()
        sv.close()
    errs = {k: relerr(out[FAST][k], out[REF][k]) for k in ("f", "g", "rho", "u", "C")}
    print("reassociated vs reference order after 500 steps:", errs)
    assert max(errs.values()) <= 1e-10, errs
    assert not bits_equal(out[FAST]["g"], out[REF]["g"])  # the two forms are really different code


def test_full_size_equals_the_unfused_operators_composed_on_the_gpu(lib, oracle):
    """4096 x 4096, 20 iterations: the reference-order context == the loop composed from the existing unfused ABI
    operators (lbm_calc_rho, lbm_calc_u, lbm_axpb for u + w, lbm_equilibrium, lbm_collision, lbm_advect)"""
    R = C = 4096
    n = R * C
    rng = np.random.default_rng(1)
    f0, g0 = initial_state(oracle, 256, 256, seed=2)
    f0 = np.tile(f0, (16, 16, 1)) * (1 + 1e-4 * rng.standard_normal((R, C, 1)))
    g0 = np.tile(g0, (16, 16, 1))
    sv = ade(lib, R, C, 1.2, 1.7, W, REF)
    sv.set_state(f0, g0)
    sv.step(20)
    got = sv.get_state()
    sv.close()
    f, g = upload_soa(lib, f0), upload_soa(lib, g0)
    del f0, g0
    fe, ge, fc, gc = (torch.empty_like(f) for _ in range(4))
    rho = torch.empty((R, C), dtype=torch.float64, device=dev())
    conc = torch.empty_like(rho)
    u = torch.empty((2, R, C), dtype=torch.float64, device=dev())
    uw = torch.empty_like(u)
    for _ in range(20):
        lib.calc_rho(_ptr(rho), _ptr(f), R, C, None)
        lib.calc_u(_ptr(u), _ptr(f), _ptr(rho), R, C, None)
        lib.calc_rho(_ptr(conc), _ptr(g), R, C, None)
        lib.equilibrium(_ptr(fe), _ptr(u), _ptr(rho), R, C, None)
        lib.axpb(_ptr(uw[0]), _ptr(u[0]), ct.c_double(1.0), ct.c_double(W[0]), ct.c_longlong(n), None)
        lib.axpb(_ptr(uw[1]), _ptr(u[1]), ct.c_double(1.0), ct.c_double(W[1]), ct.c_longlong(n), None)
        lib.equilibrium(_ptr(ge), _ptr(uw), _ptr(conc), R, C, None)
        lib.collision(_ptr(fc), _ptr(f), _ptr(fe), ct.c_double(1.2), R, C, None)
        lib.collision(_ptr(gc), _ptr(g), _ptr(ge), ct.c_double(1.7), R, C, None)
        lib.advect(_ptr(f), _ptr(fc), R, C, None)
        lib.advect(_ptr(g), _ptr(gc), R, C, None)
    lib.calc_rho(_ptr(rho), _ptr(f), R, C, None)
    lib.calc_u(_ptr(u), _ptr(f), _ptr(rho), R, C, None)
    lib.calc_rho(_ptr(conc), _ptr(g), R, C, None)
    torch.cuda.synchronize()
    assert bits_equal(got["rho"], rho.cpu().numpy())
    assert bits_equal(got["C"], conc.cpu().numpy())
    assert bits_equal(got["u"], np.moveaxis(u.cpu().numpy(), 0, -1))
    del fe, ge, fc, gc
    assert bits_equal(got["f"], download_aos(lib, f))
    assert bits_equal(got["g"], download_aos(lib, g))


@pytest.mark.parametrize("walls", [False, True])
def test_scalar_mass_is_conserved(lib, oracle, walls):
    """sum C over 2000 iterations: constant to 1e-12 relative, periodic and inside bounce-back walls"""
    R, C = 128, 128
    bc = (pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK, col_lo=pylbm.EDGE_BOUNCE_BACK,
                   col_hi=pylbm.EDGE_BOUNCE_BACK) if walls else pylbm.Bc.periodic())
    f0, g0 = initial_state(oracle, R, C, seed=13)
    sv = ade(lib, R, C, 1.2, 1.7, W, pylbm.FORM_DEFAULT, bc=bc)
    sv.set_state(f0, g0)
    m0 = oracle.calc_rho(g0).sum()
    for _ in range(4):
        sv.step(500)
        m = sv.get_state()["C"].sum()
        assert abs(m - m0) <= 1e-12 * m0, (m, m0)
    sv.close()


def test_gaussian_advects_with_u_plus_w_and_spreads_with_the_lattice_diffusivity(lib, oracle):
    """A Gaussian (sigma0 = 8) in uniform flow u0 = (0.02, 0.01), periodic 256^2, 1000 iterations, omega_g = 1:
    centroid moves by (u0 + w) t within 0.05 lattice units, variance grows by 2 D t within 1 % per axis,
    D = (1/omega_g - 1/2) / 3"""
    R = C = 256
    T, om_g = 1000, 1.0
    u0, w = np.array([0.02, 0.01]), np.array(W)
    r, c = np.meshgrid(np.arange(R, dtype=float), np.arange(C, dtype=float), indexing="ij")
    conc = 1e-3 * np.exp(-((r - 128) ** 2 + (c - 128) ** 2) / (2 * 8.0 ** 2))
    u = np.broadcast_to(u0, (R, C, 2)).copy()
    f0 = oracle.equilibrium(u, np.ones((R, C)))
    g0 = oracle.equilibrium(u + w, conc)

    def moments(x):
        m = x.sum()
        xr, xc = (x * r).sum() / m, (x * c).sum() / m
        return np.array([xr, xc]), np.array([(x * (r - xr) ** 2).sum() / m, (x * (c - xc) ** 2).sum() / m])

    sv = ade(lib, R, C, 1.0, om_g, tuple(w), pylbm.FORM_DEFAULT)
    sv.set_state(f0, g0)
    sv.step(T)
    st = sv.get_state()
    sv.close()
    x0, v0 = moments(oracle.calc_rho(g0))
    x1, v1 = moments(st["C"])
    D = (1.0 / om_g - 0.5) / 3.0
    assert np.all(np.abs((x1 - x0) - (u0 + w) * T) <= 0.05), (x1 - x0, (u0 + w) * T)
    assert np.all(np.abs((v1 - v0) / (2 * D * T) - 1) <= 0.01), (v1 - v0, 2 * D * T)


def test_launches_per_step_and_graph_replay(lib, oracle):
    """at most 2 launches per fused step (+1 for the collide-only first one); ten steps captured on one created
    stream (no parallel branches) and replayed == ten direct steps, bit for bit"""
    R, C = 96, 128
    bc = pylbm.Bc(col_lo=pylbm.EDGE_BOUNCE_BACK, col_hi=pylbm.EDGE_BOUNCE_BACK)
    f0, g0 = initial_state(oracle, R, C, seed=17)
    for b, per_step in ((pylbm.Bc.periodic(), 1), (bc, 2)):
        sv = ade(lib, R, C, 1.2, 1.7, W, pylbm.FORM_DEFAULT, bc=b)
        sv.set_state(f0, g0)
        sv.step(11)
        assert sv.launches() == 1 + 10 * per_step <= 2 * 11 + 1
        sv.close()
    direct = ade(lib, R, C, 1.2, 1.7, W, pylbm.FORM_DEFAULT, bc=bc)
    direct.set_state(f0, g0)
    direct.step(11)
    want = direct.get_state()
    direct.close()
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        sv = ade(lib, R, C, 1.2, 1.7, W, pylbm.FORM_DEFAULT, bc=bc, stream=st.value)
        sv.set_state(f0, g0)
        sv.step(1)                       # the collide-only first iteration, direct
        sv.sync()
        lib.graph_begin_capture(st)
        sv.step(10)
        lib.graph_end_capture(st, ct.byref(graph))
        lib.graph_launch(graph, 1, st)
        lib.stream_sync(st)
        assert_state_bits(sv.get_state(), want, "graph replay")
        sv.close()
    finally:
        if graph:
            lib.graph_destroy(graph)
        lib.stream_destroy(st)


@pytest.mark.parametrize("walls", ["0", "1"])
def test_passive_scalar_box_driver_equals_pylbm(lib, tmp_path, walls):
    """the C++ facade (lbm::AdeSolver) in drivers/passive_scalar_box: its dumps == pylbm.AdeSolver on the driver's
    own initial state, bit for bit"""
    R, C, steps, om, om_g, wr, wc = 72, 90, 40, 1.1, 1.6, 2e-3, 3e-3
    pre = tmp_path / "psb"
    out = key_values(run_driver("passive_scalar_box", R, C, steps, om, om_g, wr, wc, "--dump", pre, "--walls", walls, timeout=300))
    assert int(out["steps"]) == steps
    assert abs(float(out["mass_C"]) - float(out["mass_C0"])) <= 1e-12 * float(out["mass_C0"])

    def load(k, shape):
        return np.fromfile(f"{pre}-{k}.f64").reshape(shape)

    bc = pylbm.Bc(col_lo=pylbm.EDGE_BOUNCE_BACK, col_hi=pylbm.EDGE_BOUNCE_BACK) if walls == "1" else None
    sv = pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(om, 0), pylbm.AdeParams(om_g, (wr, wc)), bc=bc)
    sv.set_state(load("f0", (R, C, 9)), load("g0", (R, C, 9)))
    sv.step(steps)
    got = sv.get_state()
    sv.close()
    want = dict(f=load("f", (R, C, 9)), g=load("g", (R, C, 9)), rho=load("rho", (R, C)), u=load("u", (R, C, 2)),
                C=load("C", (R, C)))
    assert_state_bits(got, want, "driver vs pylbm")
