"""GPU suite, the scalar's fixed-concentration walls (lbm_ade_scalar_bc: lbm_ade_stream_collide_ex / _part_ex,
lbm_ring_ade_step_ex, lbm_ade_solver_set_scalar_bc; pylbm.AdeScalarBC; the drivers' flags).

The yardstick is the loop of tests/test_gpu_ade.py -- the reference's sediment loop composed from the oracle's solver::
primitives -- restated in tests/ade_util.py with the anti-bounce-back of test/rectangle_sedimentation_test.cpp:203-232 in numpy, in the
driver's expression order:
    g_adve[qbar] = -g_coll[q] + 2.0 * ((((1.0 + 3.0 cv) + 4.5 cv^2) - 1.5 vv) * E_q * C_w),  v = u + w,
    u = calc_u(f_adve) after the fluid's wall fix-ups, cv = c_q.v, vv = v.v
at every population a FIXED edge wins (rows first, columns win at the corners).  In the reference operation order the
step is compared BITWISE with it.  The slab tests run the chain and the write-set check of tests/ade_slab_util.py through the
_ex entries (tests/ade_calls.py)."""
import ctypes as ct

import numpy as np
import pytest
from conftest import relerr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pylbm  # noqa: E402
import ade_calls  # noqa: E402
from ade_slab_util import Chain, assert_part_write_sets, global_state  # noqa: E402
from ade_util import (GBC, W, alloc, assert_bits, assert_state_bits, build_sbc, cut_slab, geom, initial_state,  # noqa: E402
                      oracle_loop, owned, params, random_lattice)
from gpu_util import bits_equal, dev  # noqa: E402
from proc_util import ipc_env, key_values, last_json, run_driver  # noqa: E402

REF, FAST = pylbm.FORM_REFERENCE_ORDER, pylbm.FORM_REASSOCIATED
BB, SP, HALO, PER = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR, pylbm.EDGE_HALO, pylbm.EDGE_PERIODIC
FRAME, INNER = pylbm.ADE_PART_FRAME, pylbm.ADE_PART_INNER


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1, "no HIP device visible"
    return lib


def ade(lib, R, C, omega, omega_g, w, form, bc, scalar_bc=None, stream=None):
    return pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(omega, 0, form=form), pylbm.AdeParams(omega_g, w, form=form),
                           bc=bc, stream=stream, scalar_bc=scalar_bc)


def reference_profile(n, tail=None, value=1e-3):
    """the sedimentation driver's inlet shape (:90-93): value on the last `tail` nodes of the edge, 0 elsewhere"""
    p = np.zeros(n)
    p[-(tail or max(1, n // 4)):] = value
    return p


def _cases(R, C):
    """name -> (bc, {edge: C_w spec}); spec: a float, or ('profile', host array)"""
    prof = reference_profile(R)
    return {
        "cols_const_and_absorbing": (pylbm.Bc(col_lo=BB, col_hi=BB), {"col_lo": 1e-3, "col_hi": 0.0}),
        "bb_rows_specular_cols_mixed_corners": (pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=SP, col_hi=SP),
                                                {"row_lo": 7e-4, "col_lo": 2e-3}),
        "reference_profile": (pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=BB), {"col_lo": ("profile", prof), "col_hi": 0.0}),
        "all_four_fixed": (pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=SP),
                           {"row_lo": 1e-3, "row_hi": 2e-4, "col_lo": ("profile", reference_profile(R, R // 3, 5e-4)),
                            "col_hi": 0.0}),
    }


# ---- 1. reference order, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,R,C", [("cols_const_and_absorbing", 80, 102), ("bb_rows_specular_cols_mixed_corners", 80, 102),
                                      ("reference_profile", 96, 70), ("all_four_fixed", 64, 130),
                                      ("reference_profile", 1024, 1024)])
def test_reference_order_is_the_reference_loop_with_the_rule_bit_for_bit(lib, oracle, case, R, C):
    bc, spec = _cases(R, C)[case]
    sbc, fixed = build_sbc(spec, R, C)
    f0, g0 = initial_state(oracle, R, C, seed=R + C)
    sv = ade(lib, R, C, 1.2, 1.7, W, REF, bc, scalar_bc=sbc)
    if C == 1024:
        assert sv.lattices()[4].row_pitch > C  # the padded layout
    sv.set_state(f0, g0)
    done, want = 0, dict(f=f0, g=g0)
    for n in (1, 2, 37):
        sv.step(n - done)
        want = oracle_loop(oracle, want["f"], want["g"], 1.2, 1.7, W, n - done, bc, fixed)
        done = n
        assert_state_bits(sv.get_state(), want, f"{case} {R}x{C} after {n} steps")
    sv.close()


def test_the_rule_changes_the_state(lib, oracle):
    """the FIXED walls are not the no-flux walls: the scalar mass is no longer constant and g differs"""
    R, C = 64, 96
    bc = pylbm.Bc(col_lo=BB, col_hi=BB)
    f0, g0 = initial_state(oracle, R, C, seed=1)
    out = []
    for sbc in (None, pylbm.AdeScalarBC(col_lo=2e-3)):
        sv = ade(lib, R, C, 1.2, 1.7, W, REF, bc, scalar_bc=sbc)
        sv.set_state(f0, g0)
        sv.step(50)
        out.append(sv.get_state())
        sv.close()
    assert bits_equal(out[0]["f"], out[1]["f"])  # the fluid does not see the scalar
    assert out[1]["C"].sum() > out[0]["C"].sum() * (1 + 1e-6)  # the wall feeds the scalar in


# ---- 2. the no-op descriptor, launches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST])
def test_no_flux_descriptor_and_null_are_todays_solver(lib, oracle, form):
    R, C = 72, 96
    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=SP)
    f0, g0 = initial_state(oracle, R, C, seed=4)
    runs = {}
    for key, sbc in (("plain", "unset"), ("null", None), ("no_flux", pylbm.AdeScalarBC()),
                     ("fixed", pylbm.AdeScalarBC(row_lo=1e-3, row_hi=0.0, col_lo=5e-4, col_hi=0.0))):
        sv = ade(lib, R, C, 1.2, 1.7, W, form, bc)
        if sbc != "unset":
            sv.set_scalar_bc(sbc)
        sv.set_state(f0, g0)
        sv.step(21)
        runs[key] = (sv.get_state(), sv.launches())
        sv.close()
    for key in ("null", "no_flux"):
        assert_state_bits(runs[key][0], runs["plain"][0], key)
        assert runs[key][1] == runs["plain"][1]
    assert runs["fixed"][1] == runs["plain"][1] == 1 + 20 * 2  # FIXED edges add no launch
    assert not bits_equal(runs["fixed"][0]["g"], runs["plain"][0]["g"])


# ---- 3. reassociated form -----------------------------------------------------------------------------------------------
def test_reassociated_form_agrees_with_the_reference_order(lib, oracle):
    """500 iterations, all four edges FIXED (a profile on one): stated bound 1e-10 relative to each field's largest
    magnitude, fixed before measuring"""
    R, C = 128, 192
    bc, spec = _cases(R, C)["all_four_fixed"]
    sbc, _ = build_sbc(spec, R, C)
    f0, g0 = initial_state(oracle, R, C, seed=11)
    out = {}
    for form in (REF, FAST):
        sv = ade(lib, R, C, 1.2, 1.7, W, form, bc, scalar_bc=sbc)
        sv.set_state(f0, g0)
        sv.step(500)
        out[form] = sv.get_state()
        sv.close()
    errs = {k: relerr(out[FAST][k], out[REF][k]) for k in ("f", "g", "rho", "u", "C")}
    print("reassociated vs reference order, FIXED walls, after 500 steps:", errs)
    assert max(errs.values()) <= 1e-10, errs
    assert not bits_equal(out[FAST]["g"], out[REF]["g"])


# ---- 4. fixed point -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [REF, FAST])
def test_uniform_state_at_the_wall_concentration_stays_put(lib, oracle, form):
    """u = 0, w = 0, C = C_w on every FIXED edge (all four, specular column included): the state stays to rounding"""
    R, C, cw = 48, 64, 3e-3
    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=SP, col_hi=BB)
    u = np.zeros((R, C, 2))
    f0 = oracle.equilibrium(u, np.ones((R, C)))
    g0 = oracle.equilibrium(u, np.full((R, C), cw))
    sv = ade(lib, R, C, 1.3, 0.8, (0.0, 0.0), form, bc,
             scalar_bc=pylbm.AdeScalarBC(row_lo=cw, row_hi=cw, col_lo=cw, col_hi=(0.0, torch.full((R,), cw,
                                                                                                   dtype=torch.float64,
                                                                                                   device=dev()))))
    sv.set_state(f0, g0)
    sv.step(300)
    st = sv.get_state()
    sv.close()
    assert relerr(st["g"], g0) <= 1e-14 and relerr(st["C"], np.full((R, C), cw)) <= 1e-14, (relerr(st["g"], g0),)
    assert relerr(st["f"], f0) <= 1e-14 and np.max(np.abs(st["u"])) <= 1e-16


# ---- 5. physics ---------------------------------------------------------------------------------------------------------
def _steady_rows(lib, oracle, R, omega_g, w_r, c_lo, c_hi, steps, start):
    """fluid at rest, rows FIXED at c_lo / c_hi, columns periodic (8 wide), w = (w_r, 0): C along r after `steps`"""
    C = 8
    bc = pylbm.Bc(row_lo=BB, row_hi=BB)
    u = np.zeros((R, C, 2))
    f0 = oracle.equilibrium(u, np.ones((R, C)))
    g0 = oracle.equilibrium(u + np.array([w_r, 0.0]), np.repeat(start[:, None], C, axis=1))
    sv = ade(lib, R, C, 1.0, omega_g, (w_r, 0.0), REF, bc, scalar_bc=pylbm.AdeScalarBC(row_lo=c_lo, row_hi=c_hi))
    sv.set_state(f0, g0)
    sv.step(steps)
    a = sv.get_state()["C"]
    sv.step(steps // 10)
    b = sv.get_state()["C"]
    sv.close()
    assert np.max(np.abs(a - b)) <= 1e-15, "not yet steady"
    assert np.max(np.abs(b - b[:, :1])) <= 1e-17  # uniform along the rows
    return b[:, 0]


def test_pure_diffusion_between_fixed_rows_is_the_linear_profile(lib, oracle):
    """w = 0: the steady state is linear with the walls halfway, C(r) = C_lo + dC (r + 1/2) / R -- to rounding"""
    R, omega_g, c_lo, c_hi = 16, 1.2, 1e-3, 4e-3
    x = np.arange(R) + 0.5
    exact = c_lo + (c_hi - c_lo) * x / R
    got = _steady_rows(lib, oracle, R, omega_g, 0.0, c_lo, c_hi, 20000, np.full(R, c_lo))
    err = np.max(np.abs(got - exact)) / (c_hi - c_lo)
    print(f"linear profile, R={R}: max |C - exact| / dC = {err:.3e}")
    assert err <= 1e-12, err


def test_advection_diffusion_between_fixed_rows_converges_to_the_exponential_profile(lib, oracle):
    """w_r != 0 normal to the walls: C = C_lo + dC (e^{w x/D} - 1) / (e^{w L/D} - 1), x from the halfway wall,
    D = (1/omega_g - 1/2)/3, at Peclet w L / D = 2 on L = 16, 32, 64: the error falls at least at first order at each
    refinement and the two measured orders agree within 0.5 (no hand-picked error tolerance)"""
    omega_g, pe, c_lo, c_hi = 1.2, 2.0, 1e-3, 2e-3
    D = (1.0 / omega_g - 0.5) / 3.0
    errs = []
    for L in (16, 32, 64):
        w = pe * D / L
        x = np.arange(L) + 0.5
        exact = c_lo + (c_hi - c_lo) * np.expm1(w * x / D) / np.expm1(w * L / D)
        steps = int(40 * L * L / (np.pi ** 2 * D)) + 1000
        got = _steady_rows(lib, oracle, L, omega_g, w, c_lo, c_hi, steps, exact)
        errs.append(np.max(np.abs(got - exact)) / (c_hi - c_lo))
    orders = [float(np.log2(errs[0] / errs[1])), float(np.log2(errs[1] / errs[2]))]
    print(f"exponential profile, Pe={pe}: errors {errs}, orders {orders}")
    assert min(orders) >= 0.9, (errs, orders)
    assert abs(orders[0] - orders[1]) <= 0.5, (errs, orders)


# ---- 6. capture ---------------------------------------------------------------------------------------------------------
def test_graph_replay_reads_the_profile_array_at_every_replay(lib, oracle):
    """ten steps captured with a profile on col_lo; replay, rewrite the profile on the device, replay again == the same
    sequence run eagerly (the descriptor is the capture's, the array is read by every step)"""
    R, C = 96, 128
    bc = pylbm.Bc(row_lo=BB, col_lo=BB, col_hi=SP)
    f0, g0 = initial_state(oracle, R, C, seed=17)
    p1 = torch.from_numpy(reference_profile(R)).to(dev())
    p2 = torch.from_numpy(reference_profile(R, R // 2, 3e-3)).to(dev())

    def sbc(p):
        return pylbm.AdeScalarBC(row_lo=5e-4, col_lo=(0.0, p), col_hi=0.0)

    eager = ade(lib, R, C, 1.2, 1.7, W, pylbm.FORM_DEFAULT, bc, scalar_bc=sbc(p1))
    eager.set_state(f0, g0)
    eager.step(11)
    want1 = eager.get_state()
    eager.set_scalar_bc(sbc(p2))
    eager.step(10)
    want2 = eager.get_state()
    eager.close()
    prof = p1.clone()
    st, graph = ct.c_void_p(), ct.c_void_p()
    lib.stream_create(ct.byref(st))
    try:
        sv = ade(lib, R, C, 1.2, 1.7, W, pylbm.FORM_DEFAULT, bc, scalar_bc=sbc(prof), stream=st.value)
        sv.set_state(f0, g0)
        sv.step(1)
        sv.sync()
        lib.graph_begin_capture(st)
        sv.step(10)
        lib.graph_end_capture(st, ct.byref(graph))
        lib.graph_launch(graph, 1, st)
        lib.stream_sync(st)
        assert_state_bits(sv.get_state(), want1, "first replay")
        prof.copy_(p2)
        torch.cuda.synchronize()
        lib.graph_launch(graph, 1, st)
        lib.stream_sync(st)
        sv.set_scalar_bc(sbc(prof))  # the lazy stream of get_state reads the context's descriptor
        assert_state_bits(sv.get_state(), want2, "replay after the profile was rewritten")
        sv.close()
    finally:
        if graph:
            lib.graph_destroy(graph)
        lib.stream_destroy(st)


# ---- 7. slabs -----------------------------------------------------------------------------------------------------------
# every slab call of this suite goes through the entry points it is about (the _ex ones)
def slab_descriptor(prof, r0, bc):
    """FIXED row 0 (a chain end only), row R-1 NO_FLUX, column 0 a profile slice, column C-1 absorbing"""
    kw = dict(col_lo=(0.0, prof.data_ptr() + 8 * r0), col_hi=0.0)
    if bc.row_lo == BB:
        kw["row_lo"] = 1e-3
    return pylbm.AdeScalarBC(**kw)


@pytest.mark.parametrize("form", [REF, FAST])
def test_frame_plus_inner_is_the_one_block_step_with_fixed_walls(lib, form):
    """single blocks and ghost-1 slabs cut from the global lattice (chain ends keep the FIXED row, seams are HALO and
    NO_FLUX, column profiles sliced): FRAME + INNER == the global lbm_ade_stream_collide_ex on their rows"""
    prm = params(form)
    for R, C in ((64, 96), (130, 200), (257, 1040)):
        pitch = C + 16 if C >= 1024 else 0
        gg = geom(R, C, 0, pitch)
        prof = torch.from_numpy(reference_profile(R)).to(dev())
        gsbc = slab_descriptor(prof, 0, GBC)
        src = (random_lattice(gg, R + C), random_lattice(gg, R * C))
        want = ade_calls.full_step(lib, "_ex", gg, GBC, prm, *src, sbc=gsbc)
        for E in (1, 3, 16, 40):
            if 2 * E >= R:
                continue
            dst = (alloc(gg), alloc(gg))
            ade_calls.part(lib, "_ex", gg, GBC, prm, dst, src, FRAME, E, sbc=gsbc)
            ade_calls.part(lib, "_ex", gg, GBC, prm, dst, src, INNER, E, sbc=gsbc)
            torch.cuda.synchronize()
            for k in range(2):
                assert_bits(owned(dst[k], gg), owned(want[k], gg), f"one block R={R} C={C} E={E} lattice {k}")
        h = R // 2
        for r0, r1 in ((0, h), (h, R), (R // 4, R // 4 + h)):
            bc = pylbm.Bc(row_lo=BB if r0 == 0 else HALO, row_hi=BB if r1 == R else HALO, col_lo=BB, col_hi=SP)
            sbc = slab_descriptor(prof, r0, bc)
            slab = [cut_slab(s, gg, r0, r1, pitch) for s in src]
            sg = slab[0][0]
            for E in (1, 3, 16):
                if 2 * E >= sg.R:
                    continue
                dst = (alloc(sg), alloc(sg))
                ade_calls.part(lib, "_ex", sg, bc, prm, dst, (slab[0][1], slab[1][1]), FRAME, E, sbc=sbc)
                ade_calls.part(lib, "_ex", sg, bc, prm, dst, (slab[0][1], slab[1][1]), INNER, E, sbc=sbc)
                torch.cuda.synchronize()
                for k in range(2):
                    assert_bits(owned(dst[k], sg), owned(want[k], gg)[:, r0:r1],
                                f"R={R} C={C} slab [{r0}, {r1}) E={E} lattice {k}")


@pytest.mark.parametrize("R,C,E", [(64, 96, 1), (130, 200, 3), (50, 200, 16), (131, 1040, 40)])
def test_each_fixed_part_alone_writes_exactly_its_rows(lib, R, C, E):
    prm = params(FAST)
    bc = pylbm.Bc(row_lo=BB, row_hi=HALO, col_lo=BB, col_hi=SP)
    g = geom(R, C, 1, C + 16 if C >= 1024 else 0)
    prof = torch.from_numpy(reference_profile(R)).to(dev())
    sbc = slab_descriptor(prof, 0, bc)
    src = (random_lattice(g, R), random_lattice(g, C))
    want = [alloc(g), alloc(g)]
    ade_calls.part(lib, "_ex", g, bc, prm, want, src, FRAME, E, sbc=sbc)
    ade_calls.part(lib, "_ex", g, bc, prm, want, src, INNER, E, sbc=sbc)
    assert_part_write_sets(lambda dst, which: ade_calls.part(lib, "_ex", g, bc, prm, dst, src, which, E, sbc=sbc), g, want, E,
                           f"R={R} C={C} E={E}")


@pytest.mark.parametrize("form", [REF, FAST])
@pytest.mark.parametrize("heights,C", [((50, 130), 200), ((40, 40, 40, 40), 96)])
def test_emulated_chain_with_fixed_walls_equals_one_block(lib, oracle, form, heights, C):
    """a chain (walls on its ends) stepped slab by slab (ade_slab_util.Chain, which moves the halos of both lattices), FIXED row
    0 on the first slab only, column profile sliced per slab: == one block, 41 steps"""
    prm = params(form)
    Rg, steps = sum(heights), 41
    gg, pre = global_state(oracle, Rg, C, seed=Rg)
    prof = torch.from_numpy(reference_profile(Rg)).to(dev())
    gsbc = slab_descriptor(prof, 0, GBC)
    post = [alloc(gg), alloc(gg)]
    ade_calls.collide(lib, "", gg, GBC, prm, post, pre)
    cur = [t.clone() for t in post]
    for _ in range(steps):
        cur = list(ade_calls.full_step(lib, "_ex", gg, GBC, prm, *cur, sbc=gsbc))
    ch = Chain(lib, gg, post, heights, False, GBC,
               lambda s, dst, src, e: ade_calls.both_parts(lib, "_ex", s["g"], s["bc"], prm, dst, src, e, sbc=s["sbc"]),
               per_slab=lambda k, a, b, bc: dict(sbc=slab_descriptor(prof, a, bc)))
    for _ in range(steps):
        ch.step(16)
    torch.cuda.synchronize()
    for j in range(2):
        assert_bits(ch.gather(j), owned(cur[j], gg), f"chain {heights} lattice {j}")


# ---- 8. drivers and real rank processes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["fast", "ref"])
def test_slab_ring_ade_driver_emulated_chain_with_fixed_walls(form):
    line = last_json(run_driver("slab_ring_ade", "--emulate", 4, "--rows", 50, "--cols", 200, "--steps", 9, "--warmup", 2,
                                "--edge-rows", 8, "--walls", 1, "--scalar-fixed", 1, "--form", form, "--check", 1, timeout=300))
    assert line["check"] == "bitwise equal to one block" and line["slabs"] == 4 and line["scalar_fixed"] == 1


def test_slab_ring_ade_driver_rank_processes_with_fixed_walls(tmp_path):
    """two forked rank processes sharing this GPU over the peer-mapped transport (lbm_ring_ade_step_ex): a chain whose
    ends carry the FIXED row / NO_FLUX row, == one block bit for bit"""
    line = last_json(run_driver("slab_ring_ade", "--spawn", 2, "--one-gpu", 1, "--transport", "ipc", "--rows", 50, "--cols", 200,
                                "--steps", 7, "--warmup", 1, "--edge-rows", 8, "--walls", 1, "--scalar-fixed", 1,
                                "--check", 1, "--id-file", tmp_path / "id", timeout=300, env=ipc_env()))
    assert line["check"] == "bitwise equal to one block" and line["n_gpus"] == 2 and line["scalar_fixed"] == 1


def test_passive_scalar_box_driver_with_fixed_edges_equals_pylbm(lib, tmp_path):
    R, C, steps, om, om_g, wr, wc = 72, 90, 40, 1.1, 1.6, 2e-3, 3e-3
    pre = tmp_path / "psb"
    r = run_driver("passive_scalar_box", R, C, steps, om, om_g, wr, wc, "--dump", pre, "--walls", 2,
                   "--fixed", "row_lo=0.001,col_hi=0", timeout=300)

    def load(k, shape):
        return np.fromfile(f"{pre}-{k}.f64").reshape(shape)

    bc = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=BB)
    sv = pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(om, 0), pylbm.AdeParams(om_g, (wr, wc)), bc=bc,
                         scalar_bc=pylbm.AdeScalarBC(row_lo=1e-3, col_hi=0.0))
    sv.set_state(load("f0", (R, C, 9)), load("g0", (R, C, 9)))
    sv.step(steps)
    got = sv.get_state()
    sv.close()
    want = dict(f=load("f", (R, C, 9)), g=load("g", (R, C, 9)), rho=load("rho", (R, C)), u=load("u", (R, C, 2)),
                C=load("C", (R, C)))
    assert_state_bits(got, want, "driver vs pylbm")
    out = key_values(r)
    assert float(out["mass_C"]) != float(out["mass_C0"])  # the FIXED walls exchange scalar with the box
