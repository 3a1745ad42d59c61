"""CPU suite of the two-phase step's 80-bit yardstick (tests/exact_cg.py): the oracle's rotated entry
(orc_cg_step_from_post) against the driver-order loop bit for bit, the yardstick's own sanity (conservation in long
double, exact zeros, agreement with oracle/torch_restatement.py), the edge-state lattices (what they hold, the tile plan
they exercise, the cap on ill-conditioned nodes) and the reference order measured against the yardstick.

The bounds on the reference order -- per class the power of two at or above four times the maximum measured over every
case and lattice (profiles/cg_accuracy.txt) -- only guard against a slip in the yardstick or the generator, which shows at
>= 1e6 units:
    class   measured maximum   bound
    pop     1730.33            8192     (density ratio 100: alpha_r = 0.991 leaves f_q = 0.0018 rho beside f_0 = 0.991 rho,
                                         and the MRT sums cancel at the size of f_0; every other point: <= 46.87)
    mom     3.22               16
    psi     2.76               16
    s_nu    107.11             512      (the blend's slope, up to 2 (s_1 - omega_b) / delta = 30, times the error of psi)
The bar on the GPU forms is the reference order's own error on the same nodes: tests/test_gpu_cg_accuracy.py."""
import os

import numpy as np
import pytest
from conftest import ROOT, relerr

import exact_cg as xg
import pyoracle
from gpu_util import bits_equal, ulp_diff
from test_cg_plan import plans

REPORT = os.path.join(ROOT, "profiles", "cg_accuracy.txt")
CASES = xg.cases()
ALL = [(c, lat) for lat in xg.LATTICES for c in CASES]
IDS = [f"{c.name}-{lat}" for c, lat in ALL]
BOUND = {"pop": 8192, "mom": 16, "psi": 16, "s_nu": 512}
_rows = {}
LDBL = xg.LD


def oracle_params(case, lattice):
    R, C = xg.LATTICES[lattice]
    return pyoracle.cg_params(R, C, red=tuple(case.red), blue=tuple(case.blue), sigma=case.sigma, gravity=case.g_r,
                              delta=case.delta, gravity_c=case.g_c, add_source=case.add_source)


def as_classes(s, pop=("col_r", "col_b")):
    """a state dict in the reference's shapes -> the arrays xg.measure takes"""
    return dict(pop=np.concatenate([s[pop[0]], s[pop[1]]], axis=-1),
                mom=np.concatenate([s["rho_r"][..., None], s["rho_b"][..., None], s["u"]], axis=-1), psi=s["psi"], s_nu=s["s_nu"])


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if len(_rows) == len(ALL):   # a full run only
        lines = ["%-20s %-7s %s" % (c.name, lat, xg.fmt_row(_rows[(c.name, lat)])) for c, lat in ALL]
        worst = {cls: max(m[cls][2] for m in _rows.values()) for cls in xg.CLASSES}
        lines.append("maximum over every case: " + "   ".join("%s %.2f (bound %d)" % (cls, worst[cls], BOUND[cls]) for cls in xg.CLASSES))
        try:
            xg.write_report(REPORT, "CPU, reference order", lines)
        except OSError:
            pass                 # a read-only tree: the assertions are the test


@pytest.mark.parametrize("droplet", [False, True], ids=["rayleigh-taylor", "static-droplet"])
def test_rotated_entry_is_the_loop_body_bit_for_bit(oracle, droplet):
    """orc_cg_step_from_post on the col of step 1 = the col, psi and s_nu of step 2; its streamed populations and
    moments = the state after step 1"""
    R, C = 48, 37
    if droplet:
        p = pyoracle.cg_params(R, C, gravity=0.0, gravity_c=-6.25e-6, add_source=0)
        s0 = oracle.cg_init_droplet(p)
    else:
        p = pyoracle.cg_params(R, C)
        s0 = oracle.cg_init(p)
    one, two = oracle.cg_steps(p, s0, 1, want_col=True), oracle.cg_steps(p, s0, 2, want_col=True)
    assert not bits_equal(one["col_r"], two["col_r"])
    got = oracle.cg_step_from_post(p, one["col_r"], one["col_b"])
    for k in ("col_r", "col_b", "psi", "s_nu"):
        assert bits_equal(got[k], two[k]), (k, ulp_diff(got[k], two[k]))
    for k in ("f_r", "f_b", "rho_r", "rho_b", "u"):
        assert bits_equal(got[k], one[k]), (k, ulp_diff(got[k], one[k]))


@pytest.mark.parametrize("lattice", list(xg.LATTICES))
def test_lattices_hold_every_edge_state(lattice):
    """what the generator promises, on the composition and on the populations of every parameter point"""
    R, C = xg.LATTICES[lattice]
    x = xg.composition(lattice)
    assert x.shape == (R, C) and np.all((0 <= x) & (x <= 1))
    third = C // 3
    bands = (x[:, :third], x[:, third:2 * third], x[:, 2 * third:])
    assert np.all((bands[0] == 0) | (bands[0] == 1))                          # the exact step
    for band in bands:                                                         # bulk of either pure colour in every band
        assert np.mean(band == 1) > 0.02 and np.mean(band == 0) > 0.02
    for band in bands[1:]:                                                     # tanh profiles: mixed nodes
        assert np.mean((band > 0) & (band < 1)) > 0.05
    mixed = (x > 0) & (x < 1)
    flips = lambda v: int(np.sum(np.abs(np.diff(v)) > 0))
    assert flips(x[0]) >= 2                                                    # an interface meets wall row 0
    assert flips(x[:, 0]) >= 1 and (flips(x[:, C - 1]) >= 1 or mixed[:, C - 1].any())   # ... and both copy columns
    r0, c0 = xg.DROPLET[lattice]
    assert x[r0, c0] in (0, 1) and abs(x[r0, c0] - x[r0, c0 + 14]) > 0.3       # the droplet exchanges the colours
    for case in CASES:
        (p_r, p_b), exact = xg.case_data(case, lattice)
        assert np.all(np.isfinite(p_r)) and np.all(np.isfinite(p_b))
        assert np.all(np.sum(p_r + p_b, axis=-1) >= 0.2)
        assert np.all(p_r >= 0) and np.all(p_b >= 0)                           # ... so the streamed density cannot cancel
        assert np.all(exact.parts["rho"] >= 0.2)
        assert np.all(p_r[x == 0] == 0) and np.all(p_b[x == 1] == 0)           # an absent colour: nine exact zeros
        assert np.all(np.any(p_r[x > 0] != 0, axis=-1))
        # the noise by quadrant, relative to the equilibrium, and mirrored: one factor per pair of opposite directions
        feq_r, feq_b, level = xg.equilibrium(case, lattice)
        tot = feq_r + feq_b                                                    # the equilibrium's velocity: shear up to Mach 0.1
        j = np.stack([tot @ np.array(xg.CX, dtype=float), tot @ np.array(xg.CY, dtype=float)], axis=-1)
        mach = np.hypot(j[..., 0], j[..., 1]) / np.sum(tot, axis=-1) * np.sqrt(3.0)
        assert 0.09 < np.max(mach) < 0.105
        with np.errstate(invalid="ignore", divide="ignore"):
            dev = np.where(feq_r != 0, p_r / feq_r - 1.0, 0.0)
        quadrants = (np.s_[:R // 2, :C // 2], np.s_[:R // 2, C // 2:], np.s_[R // 2:, :C // 2], np.s_[R // 2:, C // 2:])
        for sl, lv in zip(quadrants, xg.NOISE):
            assert np.all(level[sl] == lv)
            worst = np.max(np.abs(dev[sl]))
            assert worst == 0 if lv == 0 else 1.5 * lv < worst < 3.01 * lv, (lv, worst)
        for a, b in ((1, 3), (2, 4), (5, 7), (6, 8)):
            assert np.max(np.abs(dev[..., a] - dev[..., b])) < 1e-14


def test_tile_plan_of_the_lattices():
    """80 x 200: a 3 x 2 rectangle of 16 x 64 tiles on rows 16 .. 63 and columns 32 .. 159, the tile column 160 .. 191 and
    the partial one beyond it in the frame; 37 x 45: no inner rectangle; FRAME + INNER with edge_rows = 3 the same
    rectangle"""
    knobs = (1, 2, 402)
    big, small, inner, plain = plans([(80, 200, 0, 0, 0, 0, 80, 0, 0) + knobs, (37, 45, 0, 0, 0, 0, 37, 0, 0) + knobs,
                                      (80, 200, 0, 0, 0, 0, 80, 2, 3) + knobs, (80, 200, 0, 0, 0, 0, 80, 0, 0, 1, 0, 402)])
    assert big["split"] and big["shape"] == 2 and (big["n_btr"], big["n_btc"]) == (3, 2)
    assert (16 * big["ir0"], 16 * big["ir1"], 32 * big["ic0"], 32 * big["ic1"]) == (16, 64, 32, 160)
    assert (big["tiles_r"], big["tiles_c"]) == (5, 7) and big["frame"] == 35 - 12
    assert not small["split"] and small["inner"] == 0
    assert inner == big
    assert plain["split"] and plain["shape"] == 0 and (32 * plain["ic0"], 32 * plain["ic1"]) == (32, 192)


@pytest.mark.parametrize("case,lattice", ALL, ids=IDS)
def test_yardstick_conserves_and_keeps_the_cap(case, lattice):
    """in long double, per node: mass is conserved (the source's nine terms sum to zero), momentum changes by the force
    input 2 (1 - s_nu / 2) Fg -- the source is added to both colours -- or by nothing without the source (beta_r = -beta_b
    in every case: the recolouring's momentum cancels between the colours); the carve-out stays within its cap"""
    _, exact = xg.case_data(case, lattice)
    assert case.red.beta == -case.blue.beta
    assert np.mean(exact.ill) <= xg.CAP, f"{np.sum(exact.ill)} ill-conditioned nodes"
    tot_in, tot_out = exact.f[..., :9] + exact.f[..., 9:], exact.pop[..., :9] + exact.pop[..., 9:]
    scale = np.sum(np.abs(exact.f), axis=-1) + sum(np.sum(np.abs(exact.parts[k]), axis=-1) for k in ("om1_r", "om1_b"))
    tol = scale * LDBL(2) ** -52    # ~400 operations of 2^-64 on terms of this size
    assert np.all(np.abs(np.sum(tot_out, axis=-1) - np.sum(tot_in, axis=-1)) <= tol)
    push = 2 * (1 - exact.s_nu[..., 0] / 2) if case.add_source else 0 * exact.s_nu[..., 0]
    for comp, cq, g in ((0, xg.CX, case.g_r), (1, xg.CY, case.g_c)):
        dj = sum((tot_out[..., q] - tot_in[..., q]) * cq[q] for q in range(9))
        assert np.all(np.abs(dj - push * LDBL(g)) <= tol), comp
    total = np.sum(tot_out) - np.sum(tot_in)
    assert abs(total) <= np.sum(tol)
    if case.add_source:
        assert np.any(np.abs(exact.parts["src"]) > 0)
    else:   # a pure-colour bulk node: nine exact zeros for the absent colour
        for k, sl in ((0, slice(0, 9)), (1, slice(9, 18))):
            absent = np.asarray(exact.mom[..., k] == 0)
            assert np.mean(absent) > 0.05 and np.all(exact.pop[..., sl][absent] == 0)


def test_yardstick_agrees_with_the_torch_restatement():
    import torch_restatement as tr
    case, lattice = CASES[0], "37x45"
    (p_r, p_b), exact = xg.case_data(case, lattice)
    want = as_classes(tr.cg_step_from_post(p_r, p_b, tuple(case.red), tuple(case.blue), case.sigma, (case.g_r, case.g_c),
                                           case.delta, bool(case.add_source)))
    for cls in xg.CLASSES:
        have = np.asarray(getattr(exact, cls), dtype=np.float64).reshape(np.shape(want[cls]))
        assert relerr(have, want[cls]) < 1e-12, (cls, relerr(have, want[cls]))


@pytest.mark.parametrize("case,lattice", ALL, ids=IDS)
def test_reference_order_against_80_bit(oracle, case, lattice):
    (p_r, p_b), exact = xg.case_data(case, lattice)
    got = as_classes(oracle.cg_step_from_post(oracle_params(case, lattice), p_r, p_b))
    assert all(np.all(np.isfinite(v)) for v in got.values())
    m = xg.measure(got, exact)
    _rows[(case.name, lattice)] = m
    print("%-20s %-7s %s" % (case.name, lattice, xg.fmt_row(m)))
    for cls in xg.CLASSES:
        assert np.all(np.isfinite(m[cls])) and max(m[cls]) <= BOUND[cls], (cls, m[cls], BOUND[cls])
