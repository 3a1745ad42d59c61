"""GPU suite, buoyancy of the fluid + scalar solver (lbm_ade_buoyancy: lbm_ade_collide_b, lbm_ade_stream_collide_b /
_part_b, lbm_ade_solver_set_buoyancy, lbm_ring_ade_*_b through the slab_ring_ade driver; pylbm.AdeBuoyancy; the drivers'
--buoyancy).

The yardstick of every bitwise test is `oracle_loop` of tests/ade_util.py with a buoyancy: the reference's sediment loop
composed from the oracle's solver:: primitives (calc_rho, calc_u, equilibrium, advect, collision for the scalar), with the
force, the velocity shift and the fluid's forced collision (items 4-6 of the step in include/lbm_hip.h) written in numpy
in exactly that order -- numpy's element-wise f64 operations do not fuse -- and the wall rules, which take
u = calc_u(f_adve), the UNSHIFTED velocity.  The loop never calls the library under test.  The slab tests run the chain of
tests/ade_slab_util.py through the _b entries (tests/ade_calls.py)."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
import ade_calls  # noqa: E402
import ade_util as ade  # noqa: E402
from ade_slab_util import Chain  # noqa: E402
from ade_util import GUO, REFERENCE, buoyancy, buoyant_collide, from_lattice, stream, to_lattice  # noqa: E402
from gpu_util import bits_equal, dev  # noqa: E402
from proc_util import last_json, run_driver  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
BB, SP, HALO, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO, pylbm.EDGE_PERIODIC
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER
W = (3e-3, -2e-3)
OMEGA, OMEGA_G = 1.2, 1.7


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


def initial_state(orc, R, C, seed):
    return ade.buoyant_initial_state(orc, R, C, seed, W)


def solver(lib, R, C, by, bc=None, sbc=None, form=REF, stream_=None, w=W, omega=OMEGA, omega_g=OMEGA_G):
    return pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(omega, 0, form=form), pylbm.AdeParams(omega_g, w, form=form), bc=bc,
                           stream=stream_, scalar_bc=sbc, buoyancy=by)


BETA, C_REF = (2e-3, -1.5e-3), 0.4


# ---- 1. periodic box ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [REFERENCE, GUO], ids=["reference", "guo"])
def test_periodic_box_is_the_loop_bit_for_bit(lib, oracle, variant):
    """96 x 70 after 1, 2 and 37 steps, both components of beta and of w non-zero; a buoyant step runs the reference order
    whatever the form says, so a context of the default form is held to the same bits"""
    R, C = 96, 70
    by = buoyancy(BETA, C_REF, variant)
    f0, g0 = initial_state(oracle, R, C, seed=3)
    svs = [solver(lib, R, C, by, form=form) for form in (REF, pylbm.FORM_DEFAULT)]
    for sv in svs:
        sv.set_state(f0, g0)
    done, want = 0, dict(f=f0, g=g0)
    for n in (1, 2, 37):
        want = ade.oracle_loop(oracle, want["f"], want["g"], OMEGA, OMEGA_G, W, n - done, by=by)
        for sv in svs:
            sv.step(n - done)
            ade.assert_state_bits(sv.get_state(), want, f"periodic {variant} after {n} steps")
        done = n
    for sv in svs:
        assert sv.launches() == 37  # one launch per step, as the passive periodic step
        sv.close()
    passive = ade.oracle_loop(oracle, f0, g0, OMEGA, OMEGA_G, W, 37, pylbm.Bc(), {})
    assert not bits_equal(passive["f"], want["f"])  # the scalar does push on the fluid


# ---- 2. walls with FIXED edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [REFERENCE, GUO], ids=["reference", "guo"])
def test_walls_with_fixed_edges_are_the_loop_bit_for_bit(lib, oracle, variant):
    """80 x 102, 23 steps, bounce-back rows and specular columns, row_lo FIXED at a constant and col_hi at a device profile:
    the wall rule sees u0 (the loop's fix_up takes calc_u of the streamed f), the collisions the shifted u"""
    R, C = 80, 102
    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=SP, col_hi=SP)
    prof = np.linspace(0.1, 0.9, R) ** 2
    sbc, fixed = ade.build_sbc({"row_lo": 0.7, "col_hi": ("profile", prof)}, R, C)
    by = buoyancy(BETA, C_REF, variant)
    f0, g0 = initial_state(oracle, R, C, seed=5)
    sv = solver(lib, R, C, by, bc=bc, sbc=sbc)
    sv.set_state(f0, g0)
    sv.step(23)
    want = ade.oracle_loop(oracle, f0, g0, OMEGA, OMEGA_G, W, 23, bc, fixed, by=by)
    ade.assert_state_bits(sv.get_state(), want, f"walls + FIXED {variant}")
    assert sv.launches() == 1 + 22 * 2  # interior + edge pass, as the passive step with walls
    sv.close()


# ---- 3. the fluid half is the forced BGK of lbm_solver ------------------------------------------------------------------
def test_fluid_half_is_the_existing_forced_bgk(lib, oracle):
    """g = 0, c_ref = -1, beta = (Fr, Fc), u_shift = 1, guo = (1/3, 1/9): F = (0 - -1) beta = (Fr, Fc) exactly and g stays
    0, so f after 20 steps is the f of an lbm_solver BGK context with force_mode = 1 -- the kernel the oracle's gravity_run
    pins -- bit for bit"""
    R, C, Fr, Fc = 64, 96, -3e-4, 1.1e-4
    f0, _ = initial_state(oracle, R, C, seed=9)
    g0 = np.zeros((R, C, 9))
    sv = solver(lib, R, C, pylbm.AdeBuoyancy((Fr, Fc), -1.0), w=(0.0, 0.0))
    sv.set_state(f0, g0)
    sv.step(20)
    got = sv.get_state()
    sv.close()
    bgk = pylbm.Solver(lib, pylbm.MODEL_BGK, R, C, pylbm.BgkParams(OMEGA, 0, force=(Fr, Fc)))
    bgk.set_f(f0)
    bgk.step(20)
    want = bgk.get_f()
    bgk.close()
    assert not got["g"].any() and not got["C"].any()
    assert bits_equal(got["f"], want), np.max(np.abs(got["f"] - want))
    plain = pylbm.Solver(lib, pylbm.MODEL_BGK, R, C, pylbm.BgkParams(OMEGA, 0, form=REF))
    plain.set_f(f0)
    plain.step(20)
    assert not bits_equal(plain.get_f(), want)  # the force is felt
    plain.close()


# ---- 4. the raw entry points and their moments --------------------------------------------------------------------------
@pytest.mark.parametrize("with_walls", [False, True], ids=["periodic", "walls_fixed"])
def test_raw_entry_points_write_the_shifted_velocity(lib, oracle, with_walls):
    R, C = 48, 66
    g = ade.geom(R, C, 0)
    by = buoyancy(BETA, C_REF, GUO)
    prm = pylbm.BgkParams(OMEGA, 0, form=FAST), pylbm.AdeParams(OMEGA_G, W, form=FAST)  # the form is overruled
    if with_walls:
        bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=SP, col_hi=BB)
        sbc, fixed = ade.build_sbc({"row_lo": 0.7, "col_hi": ("profile", np.linspace(0.0, 1.0, R))}, R, C)
    else:
        bc, sbc, fixed = pylbm.Bc(), None, {}
    f0, g0 = initial_state(oracle, R, C, seed=21)
    c0 = buoyant_collide(oracle, f0, g0, OMEGA, OMEGA_G, W, by)
    f1, g1 = stream(oracle, bc, fixed, c0["fc"], c0["gc"], W)
    c1 = buoyant_collide(oracle, f1, g1, OMEGA, OMEGA_G, W, by)

    def moments():
        return [torch.full((n, R, C), np.nan, dtype=torch.float64, device=dev()) for n in (1, 2, 1)]

    def check(what, lat, mom, want):
        torch.cuda.synchronize()
        assert bits_equal(from_lattice(lat[0], g), want["fc"]), what + ": f"
        assert bits_equal(from_lattice(lat[1], g), want["gc"]), what + ": g"
        assert bits_equal(mom[0][0].cpu().numpy(), want["rho"]), what + ": rho"
        assert bits_equal(mom[1].cpu().numpy().transpose(1, 2, 0), want["u"]), what + ": u is not the shifted velocity"
        assert bits_equal(mom[2][0].cpu().numpy(), want["C"]), what + ": conc"

    pre = to_lattice(f0, g), to_lattice(g0, g)
    post = ade.alloc(g), ade.alloc(g)
    m = moments()
    ade_calls.collide(lib, "_b", g, bc, prm, post, pre, sbc=sbc, buoy=by, moments=m)
    check("lbm_ade_collide_b", post, m, c0)
    nxt = ade.alloc(g), ade.alloc(g)
    m = moments()
    ade_calls.step_into(lib, "_b", g, bc, prm, nxt, post, sbc=sbc, buoy=by, moments=m)
    check("lbm_ade_stream_collide_b", nxt, m, c1)
    for which in (FRAME, INNER):  # the part launch writes the same moments at its nodes
        part, m = (ade.alloc(g), ade.alloc(g)), moments()
        ade_calls.part(lib, "_b", g, bc, prm, part, post, which, 5, sbc=sbc, buoy=by, moments=m)
        torch.cuda.synchronize()
        rows = np.r_[0:5, R - 5:R] if which == FRAME else np.r_[5:R - 5]
        assert bits_equal(m[1].cpu().numpy().transpose(1, 2, 0)[rows], c1["u"][rows]), f"part {which}: u"
        assert bits_equal(m[0][0].cpu().numpy()[rows], c1["rho"][rows]) and bits_equal(m[2][0].cpu().numpy()[rows], c1["C"][rows])
        assert bits_equal(from_lattice(part[0], g)[rows], c1["fc"][rows]) and bits_equal(from_lattice(part[1], g)[rows], c1["gc"][rows])


# ---- 5. beta = (0, 0) and NULL ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST], ids=["ref", "fast"])
@pytest.mark.parametrize("with_walls", [False, True], ids=["periodic", "walls_fixed"])
def test_zero_beta_and_null_are_the_passive_solver(lib, oracle, form, with_walls):
    R, C = 72, 96
    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=SP) if with_walls else None
    sbc = pylbm.AdeScalarBC(row_lo=0.6, col_hi=0.0) if with_walls else None
    f0, g0 = initial_state(oracle, R, C, seed=4)
    runs = {}
    for key, by in (("plain", "unset"), ("null", None), ("zero", pylbm.AdeBuoyancy((0.0, 0.0), 0.3, 0.5, (3.0, 9.0))),
                    ("buoyant", buoyancy(BETA, C_REF, GUO))):
        sv = solver(lib, R, C, None, bc=bc, sbc=sbc, form=form)
        if by != "unset":
            sv.set_buoyancy(by)
        sv.set_state(f0, g0)
        sv.step(11)
        runs[key] = (sv.get_state(), sv.launches())
        sv.close()
    for key in ("null", "zero"):
        ade.assert_state_bits(runs[key][0], runs["plain"][0], key)
        assert runs[key][1] == runs["plain"][1]
    assert runs["buoyant"][1] == runs["plain"][1] == 1 + 10 * (2 if with_walls else 1)  # buoyancy adds no launch
    assert not bits_equal(runs["buoyant"][0]["f"], runs["plain"][0]["f"])


# ---- 6. graphs ----------------------------------------------------------------------------------------------------------
def test_graph_replay_keeps_the_buoyancy_of_its_capture(lib, oracle):
    """10 steps captured and replayed 3 times == 30 plain steps; set_buoyancy between the replays changes nothing the graph
    does (the descriptor travels by value in the kernel arguments)"""
    R, C = 96, 128
    bc = pylbm.Bc(row_lo=BB, col_lo=BB, col_hi=SP)
    sbc = pylbm.AdeScalarBC(row_lo=0.5, col_hi=0.0)
    by = buoyancy(BETA, C_REF, GUO)
    f0, g0 = initial_state(oracle, R, C, seed=17)
    eager = solver(lib, R, C, by, bc=bc, sbc=sbc)
    eager.set_state(f0, g0)
    eager.step(31)
    want = eager.get_state()
    assert eager.launches() == 1 + 30 * 2
    eager.close()
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        sv = solver(lib, R, C, by, bc=bc, sbc=sbc, stream_=st.value)
        sv.set_state(f0, g0)
        sv.step(1)
        sv.sync()
        lib.graph_begin_capture(st)
        sv.step(10)
        lib.graph_end_capture(st, ct.byref(graph))
        lib.graph_launch(graph, 1, st)
        lib.stream_sync(st)
        sv.set_buoyancy(pylbm.AdeBuoyancy((0.5, 0.5), 0.0))  # not what the graph holds
        lib.graph_launch(graph, 1, st)
        sv.set_buoyancy(None)
        lib.graph_launch(graph, 1, st)
        lib.stream_sync(st)
        ade.assert_state_bits(sv.get_state(), want, "three replays of ten steps")  # get_state does not read the buoyancy
        sv.close()
    finally:
        if graph:
            lib.graph_destroy(graph)
        lib.stream_destroy(st)


# ---- 7. parts and slabs -------------------------------------------------------------------------------------------------
SLAB_BY = pylbm.AdeBuoyancy((2e-2, -1e-2), 1.0, 0.5, (3.0, 9.0))  # random_lattice: C ~ 1.0 .. 1.05


@pytest.mark.parametrize("with_walls", [False, True], ids=["periodic", "walls_fixed"])
@pytest.mark.parametrize("R,C,E", [(64, 96, 1), (130, 200, 3)])
def test_frame_plus_inner_is_the_full_buoyant_step(lib, R, C, E, with_walls):
    prm = ade.params(FAST, W, OMEGA, OMEGA_G)
    gg = ade.geom(R, C, 0)
    prof = torch.from_numpy(np.linspace(0.9, 1.1, R)).to(dev())
    bc = ade.GBC if with_walls else pylbm.Bc()
    sbc = pylbm.AdeScalarBC(row_lo=1.02, col_lo=(0.0, prof), col_hi=0.0) if with_walls else None
    src = (ade.random_lattice(gg, R + C), ade.random_lattice(gg, R * C))
    want = ade_calls.full_step(lib, "_b", gg, bc, prm, *src, sbc=sbc, buoy=SLAB_BY)
    passive = ade_calls.full_step(lib, "_b", gg, bc, prm, *src, sbc=sbc, buoy=pylbm.AdeBuoyancy())
    dst = (ade.alloc(gg), ade.alloc(gg))
    for d in dst:
        ade.bits(d).fill_(ade.SENTINEL)
    ade_calls.both_parts(lib, "_b", gg, bc, prm, dst, src, E, sbc=sbc, buoy=SLAB_BY)
    torch.cuda.synchronize()
    for k in range(2):
        ade.assert_bits(ade.owned(dst[k], gg), ade.owned(want[k], gg), f"R={R} C={C} E={E} lattice {k}")
        # nothing outside the owned nodes was written
        mask = torch.zeros(9 * gg.plane_stride, dtype=torch.bool, device=dev())
        ade.owned(mask, gg)[:] = True
        assert bool(((ade.bits(dst[k]) != ade.SENTINEL) == mask).all())
    assert bool((ade.bits(want[0]) != ade.bits(passive[0])).any())


@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
@pytest.mark.parametrize("heights", [(48, 48, 48), (50, 130)])
def test_emulated_chain_equals_one_block(lib, oracle, heights, closed):
    """slabs with one ghost row stepped by lbm_ade_stream_collide_part_b (ade_slab_util.Chain, which moves the halos of both
    lattices); open: a chain with walls on its ends and FIXED edges, closed: a periodic ring with wall columns; 9 steps"""
    C, steps = 200, 9
    prm = ade.params(FAST, W, OMEGA, OMEGA_G)
    Rg = sum(heights)
    gg = ade.geom(Rg, C, 0)
    by = buoyancy(BETA, C_REF, GUO)
    f0, g0 = initial_state(oracle, Rg, C, seed=Rg)
    pre = [to_lattice(a, gg) for a in (f0, g0)]
    prof = torch.from_numpy(np.linspace(0.0, 1.0, Rg)).to(dev())
    gbc = pylbm.Bc(col_lo=BB, col_hi=SP) if closed else ade.GBC

    def descriptor(r0, bc):
        kw = dict(col_lo=(0.0, prof.data_ptr() + 8 * r0), col_hi=0.0)
        if bc.row_lo == BB:
            kw["row_lo"] = 0.8
        return pylbm.AdeScalarBC(**kw)

    gsbc = descriptor(0, gbc)
    post = [ade.alloc(gg), ade.alloc(gg)]
    ade_calls.collide(lib, "_b", gg, gbc, prm, post, pre, buoy=by)
    cur = [t.clone() for t in post]
    for _ in range(steps):
        cur = list(ade_calls.full_step(lib, "_b", gg, gbc, prm, *cur, sbc=gsbc, buoy=by))
    ch = Chain(lib, gg, post, heights, closed, gbc,
               lambda s, dst, src, e: ade_calls.both_parts(lib, "_b", s["g"], s["bc"], prm, dst, src, e, sbc=s["sbc"], buoy=by),
               per_slab=lambda k, a, b, bc: dict(sbc=descriptor(a, bc)))
    for _ in range(steps):
        ch.step(16)
    torch.cuda.synchronize()
    for j in range(2):
        ade.assert_bits(ch.gather(j), ade.owned(cur[j], gg), f"chain {heights} closed={closed} lattice {j}")


DRIVER_BUOYANCY = "0.8,-0.5,0.0004,0.5,3,9"  # the drivers' scalars are ~1e-3


def test_slab_ring_ade_driver_emulated_chain_with_buoyancy():
    line = last_json(run_driver("slab_ring_ade", "--emulate", 4, "--rows", 48, "--cols", 200, "--steps", 9, "--edge-rows", 8,
                                "--walls", 1, "--buoyancy", DRIVER_BUOYANCY, "--check", 1, timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["slabs"] == 4
    assert line["buoyancy"] == [0.8, -0.5, 0.0004, 0.5, 3.0, 9.0]


def test_passive_scalar_box_driver_with_buoyancy_equals_pylbm(lib, tmp_path):
    R, C, steps, om, om_g, wr, wc = 72, 90, 40, 1.1, 1.6, 2e-3, 3e-3
    pre = tmp_path / "psb"
    run_driver("passive_scalar_box", R, C, steps, om, om_g, wr, wc, "--dump", pre, "--walls", 2,
               "--fixed", "row_lo=0.001,col_hi=0", "--buoyancy", DRIVER_BUOYANCY, timeout=300)

    def load(k, shape):
        return np.fromfile(f"{pre}-{k}.f64").reshape(shape)

    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=BB)
    out = []
    for by in (pylbm.AdeBuoyancy((0.8, -0.5), 0.0004, 0.5, (3.0, 9.0)), None):
        sv = pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(om, 0), pylbm.AdeParams(om_g, (wr, wc)), bc=bc,
                             scalar_bc=pylbm.AdeScalarBC(row_lo=1e-3, col_hi=0.0), buoyancy=by)
        sv.set_state(load("f0", (R, C, 9)), load("g0", (R, C, 9)))
        sv.step(steps)
        out.append(sv.get_state())
        sv.close()
    want = dict(f=load("f", (R, C, 9)), g=load("g", (R, C, 9)), rho=load("rho", (R, C)), u=load("u", (R, C, 2)),
                C=load("C", (R, C)))
    ade.assert_state_bits(out[0], want, "driver vs pylbm")
    assert not bits_equal(out[1]["f"], want["f"])


# ---- 8. vertical slot, conduction regime --------------------------------------------------------------------------------
def slot_run(step_fn, orc, R, C):
    """fluid at rest, uniform C = c_ref; returns the state after n = 6 C^2 / nu steps"""
    u = np.zeros((R, C, 2))
    f0 = orc.equilibrium(u, np.ones((R, C)))
    g0 = orc.equilibrium(u, np.full((R, C), 0.5))
    nu = (1.0 / 1.0 - 0.5) / 3.0
    return step_fn(f0, g0, int(round(6 * C * C / nu)))


def slot_errors(st, C, beta=1e-4):
    """(relative L2 error of the shifted u_r against the cubic profile, max deviation of C from the linear profile)"""
    nu, L, K = (1.0 / 1.0 - 0.5) / 3.0, float(C), 1.0
    x = np.arange(C) + 0.5
    exact = -(K * beta * 1.0 / nu) * (x ** 3 / (6 * L) - x ** 2 / 4 + x * L / 12)
    u_r = st["u"][..., 0] + 0.5 * (beta * (st["C"] - 0.5))  # the velocity that enters the equilibria
    assert np.array_equal(u_r, np.repeat(u_r[:1], u_r.shape[0], axis=0)), "u differs across the rows"
    assert np.array_equal(st["C"], np.repeat(st["C"][:1], st["C"].shape[0], axis=0))
    return (float(np.linalg.norm(u_r[0] - exact) / np.linalg.norm(exact)), float(np.max(np.abs(st["C"][0] - x / L))))


SLOT_BC = dict(col_lo=BB, col_hi=BB)
SLOT_BY = dict(beta=(1e-4, 0.0), c_ref=0.5, u_shift=0.5, guo=(3.0, 9.0))


def test_vertical_slot_conduction_regime_converges_to_the_cubic_profile(lib, oracle):
    """periodic rows, bounce-back columns with the scalar FIXED at 0 / 1, c_ref = 0.5, beta = (1e-4, 0), w = 0, omega = 1,
    omega_g = 1.2, Guo's coefficients, R = 8: linear C, u_r(x) = -(K beta dC / nu)(x^3 / 6L - x^2 / 4 + x L / 12).  A numpy
    model of exactly this scheme gives relative L2 errors 8.15e-3 at C = 16 and 2.04e-3 at C = 32 (C linear to 4e-14);
    asserted: the error at 32 <= 2.5e-3, the observed order >= 1.9, C linear to 1e-12, u identical across the rows"""
    errs = {}
    for C in (16, 32):
        def run(f0, g0, n):
            sv = solver(lib, 8, C, pylbm.AdeBuoyancy(**SLOT_BY), bc=pylbm.Bc(**SLOT_BC),
                        sbc=pylbm.AdeScalarBC(col_lo=0.0, col_hi=1.0), w=(0.0, 0.0), omega=1.0, omega_g=1.2)
            sv.set_state(f0, g0)
            sv.step(n)
            st = sv.get_state()
            sv.close()
            return st

        errs[C] = slot_errors(slot_run(run, oracle, 8, C), C)
    order = float(np.log2(errs[16][0] / errs[32][0]))
    print(f"vertical slot: rel L2 error {errs[16][0]:.3e} at C=16, {errs[32][0]:.3e} at C=32, order {order:.3f}; "
          f"C off linear by {errs[16][1]:.1e}, {errs[32][1]:.1e}")
    assert errs[32][0] <= 2.5e-3, errs
    assert order >= 1.9, (errs, order)
    assert max(errs[16][1], errs[32][1]) <= 1e-12, errs


# ---- 9. Rayleigh-Benard onset -------------------------------------------------------------------------------------------
RB_R, RB_C, RB_OMEGA = 24, 48, 1.4
RB_NU = (1.0 / RB_OMEGA - 0.5) / 3.0
RA_THEORY = 1707.76  # rigid-rigid, critical wavenumber ~ pi / R: the box holds one wavelength 2 R


def rb_initial(orc):
    r, c = np.meshgrid(np.arange(RB_R, dtype=float), np.arange(RB_C, dtype=float), indexing="ij")
    conc = 1.0 - (r + 0.5) / RB_R + 1e-3 * np.sin(np.pi * (r + 0.5) / RB_R) * np.cos(2 * np.pi * c / RB_C)
    u = np.zeros((RB_R, RB_C, 2))
    return orc.equilibrium(u, np.ones((RB_R, RB_C))), orc.equilibrium(u, conc)


def rb_growth(step_fn, orc, Ra):
    """sigma T = 1/2 ln(E(2T) / E(T)), E = sum u_c^2, T = int(R^2 / nu)"""
    T = int(RB_R ** 2 / RB_NU)
    f0, g0 = rb_initial(orc)
    e1, e2 = step_fn(f0, g0, Ra * RB_NU ** 2 / RB_R ** 3, T)
    return 0.5 * float(np.log(e2 / e1))


def test_rayleigh_benard_onset(lib, oracle):
    """R = 24, C = 48, bounce-back rows, periodic columns, the scalar FIXED at 1 below and 0 above, c_ref = 0.5,
    beta = (Ra nu^2 / R^3, 0), omega = omega_g = 1.4, Guo's coefficients; conduction profile plus 1e-3 sin cos.  The numpy
    model gives sigma T = -1.731 at Ra = 1500 and +1.698 at 1950, zero crossing at Ra_c = 1727 (+1.1 % off 1707.76);
    asserted: decay at 1500, growth at 1950, the interpolated Ra_c within 3 % of 1707.76"""
    assert int(RB_R ** 2 / RB_NU) == 8063

    def run(f0, g0, beta, T):
        sv = solver(lib, RB_R, RB_C, pylbm.AdeBuoyancy((beta, 0.0), 0.5, 0.5, (3.0, 9.0)), bc=pylbm.Bc(row_lo=BB, row_hi=BB),
                    sbc=pylbm.AdeScalarBC(row_lo=1.0, row_hi=0.0), w=(0.0, 0.0), omega=RB_OMEGA, omega_g=RB_OMEGA)
        sv.set_state(f0, g0)
        out = []
        for _ in range(2):
            sv.step(T)
            out.append(float(np.sum(sv.get_state()["u"][..., 1] ** 2)))
        sv.close()
        return out

    s_lo, s_hi = rb_growth(run, oracle, 1500.0), rb_growth(run, oracle, 1950.0)
    ra_c = 1500.0 + 450.0 * (0.0 - s_lo) / (s_hi - s_lo)
    print(f"Rayleigh-Benard: sigma T = {s_lo:.3f} at Ra = 1500, {s_hi:.3f} at Ra = 1950, Ra_c = {ra_c:.1f}")
    assert s_lo < 0.0, s_lo
    assert s_hi > 0.0, s_hi
    assert abs(ra_c - RA_THEORY) <= 0.03 * RA_THEORY, ra_c
