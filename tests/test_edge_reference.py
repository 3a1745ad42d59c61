"""The edge-mode yardstick (tests/edge_reference.py) pinned on the CPU, before a GPU is involved:

  * bitwise equal to the oracle's own driver loops wherever the oracle has one -- periodic BGK, the free-stream channel
    (anti-bounce-back velocity rows, specular columns), periodic KBC, and the two pressure-row drivers (bounce-back
    columns: horizontal_poiseuille_test.cpp; specular columns: specular_boundary_test.cpp);
  * a hand-written table on a 3 x 3 lattice in which every population carries its own mark: for every mode on every edge,
    where each population must arrive -- all 144 edge sets, the four corners spelled out for the sets whose row and column
    rules disagree there.

The tables below are copied by hand from the driver lines include/lbm_hip.h cites for each mode; edge_reference.py derives
the same pairs from the velocity set, so a slip in either shows here."""
import numpy as np
import pytest

import edge_reference as er
from edge_reference import ABB_VELOCITY as ABB, BOUNCE_BACK as BB, PERIODIC as PER, SPECULAR as SP, WRAP_NOSHIFT as WRAP
from pyoracle import hpt_params

S2 = 1.0 / (0.5 + 3.0 * 1.70766666e-4)  # ulbm_double_shear_flow.cpp:75-76


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_mode_numbers_are_the_header_s():
    import pylbm
    assert (PER, BB, SP, ABB, WRAP) == (pylbm.EDGE_PERIODIC, pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR,
                                        pylbm.EDGE_ABB_VELOCITY, pylbm.EDGE_WRAP_NOSHIFT)
    assert len(er.all_edges()) == 144 and len(set(er.all_edges())) == 144
    assert len(er.unmixed_wall_edges()) == 24 and set(er.unmixed_wall_edges()) <= set(er.all_edges())


# ---- against the oracle's driver loops: bitwise ---------------------------------------------------------------------------
@pytest.mark.parametrize("inc", [0, 1])
def test_periodic_bgk_is_the_oracle_loop(oracle, inc):
    f0 = er.noisy_state(oracle, 13, 11, seed=1)
    want_f, want_rho, want_u = oracle.bgk_periodic_steps(f0, 1.3, 7, incompressible=bool(inc))
    got = er.run(oracle, f0, 7, er.Edges(), er.Bgk(1.3, inc))
    assert bits_equal(got["f"], want_f)
    # the oracle's tensors hold the moments of the state BEFORE its last iteration
    before = er.run(oracle, f0, 6, er.Edges(), er.Bgk(1.3, inc))
    assert bits_equal(before["rho"], want_rho) and bits_equal(before["u"], want_u)


def test_velocity_rows_and_specular_columns_are_the_free_stream_loop(oracle):
    f0 = er.noisy_state(oracle, 13, 11, seed=2)
    want_f, _, _ = oracle.free_stream_steps(f0, 1.3, 0.04, 9)
    e = er.Edges(ABB, ABB, SP, SP, (0.04, 0.0))
    assert bits_equal(er.run(oracle, f0, 9, e, er.Bgk(1.3, 1))["f"], want_f)


def test_periodic_kbc_is_the_oracle_loop(oracle):
    f0 = er.noisy_state(oracle, 13, 11, seed=3)
    m0 = oracle.calc_rho(f0)
    want_f, want_m0, want_m1 = oracle.kbc_steps(f0, m0, oracle.calc_u(f0, m0), S2, 6)
    got = er.run(oracle, f0, 6, er.Edges(), er.Kbc(S2))
    assert bits_equal(got["f"], want_f) and bits_equal(got["rho"], want_m0) and bits_equal(got["u"], want_m1)


def test_pressure_rows_compose_the_same_way(oracle):
    """both pressure-row drivers: the virtual rows are two more slice assignments on the post-collision lattice"""
    H, W, T = 9, 8, 25
    start = oracle.incomp_equilibrium(np.zeros((H, W, 2)), np.ones((H, W)))
    p = hpt_params(H, W, T, check_convergence=0)
    want = oracle.hpt_run(p)
    assert want["steps"] == T
    got = er.run(oracle, start, T, er.Edges(col_lo=BB, col_hi=BB), er.Bgk(p.omega, 1), pressure=(p.rho_inlet, p.rho_outlet))
    assert bits_equal(got["f"], want["f"])
    want = oracle.sbt_run(H, W, T, 1.1, 1.002, 1.0)
    got = er.run(oracle, start, T, er.Edges(col_lo=SP, col_hi=SP), er.Bgk(1.1, 0), pressure=(1.002, 1.0))
    assert bits_equal(got["f"], want["f"])


# ---- the hand-written table ---------------------------------------------------------------------------------------------------
# population q of a node moves to the node (r + DR[q], c + DC[q])
DR = {0: 0, 1: 1, 2: 0, 3: -1, 4: 0, 5: 1, 6: -1, 7: -1, 8: 1}
DC = {0: 0, 1: 0, 2: 1, 3: 0, 4: -1, 5: 1, 6: 1, 7: -1, 8: -1}
WEIGHT = {0: 4 / 9, 1: 1 / 9, 2: 1 / 9, 3: 1 / 9, 4: 1 / 9, 5: 1 / 36, 6: 1 / 36, 7: 1 / 36, 8: 1 / 36}
# (destination slot, source slot of the SAME node), as the drivers write them
BB_ROW_LO = [(1, 3), (5, 7), (8, 6)]      # mrtcg_rayleigh_taylor.cpp:529-531
BB_ROW_HI = [(3, 1), (7, 5), (6, 8)]      # :525-527
BB_COL_HI = [(4, 2), (7, 5), (8, 6)]      # horizontal_poiseuille_test.cpp:146-148
BB_COL_LO = [(2, 4), (5, 7), (6, 8)]      # :150-152
SP_COL_HI = [(4, 2), (7, 6), (8, 5)]      # cylinder_test.cpp:157-159
SP_COL_LO = [(2, 4), (5, 8), (6, 7)]      # :161-163
ABB_ROW = [(3, 1), (4, 2), (1, 3), (2, 4), (7, 5), (8, 6), (5, 7), (6, 8)]   # cylinder_test.cpp:136-143 = :147-154
# slots copied from the opposite column of the same row, rows 1..R-2
WRAP_COL_LO = [2, 5, 6]                   # mrtcg_rayleigh_taylor.cpp:517-519
WRAP_COL_HI = [4, 8, 7]                   # :521-523
UW = (0.04, 0.01)
R3 = C3 = 3


def mark(r, c, q):
    return 1000.0 + 100 * r + 10 * c + q


def marked_lattice():
    fc = np.empty((R3, C3, 9))
    for r in range(R3):
        for c in range(C3):
            for q in range(9):
                fc[r, c, q] = mark(r, c, q)
    return fc


def abb_value(q):
    cu = UW[0] * DR[q] + UW[1] * DC[q]
    return (2.0 + 9.0 * (cu * cu) - 3.0 * (UW[0] * UW[0] + UW[1] * UW[1])) * WEIGHT[q]


def table(e):
    """node by node: what every slot of the streamed 3 x 3 lattice must hold"""
    want = np.full((R3, C3, 9), np.nan)
    for r in range(R3):
        for c in range(C3):
            for q in range(9):   # periodic arrival
                want[(r + DR[q]) % R3, (c + DC[q]) % C3, q] = mark(r, c, q)
    for r in range(R3):
        for c in range(C3):
            for row, mode, pairs in ((0, e.row_lo, BB_ROW_LO), (R3 - 1, e.row_hi, BB_ROW_HI)):   # rows first
                if r == row and mode == BB:
                    for dst, src in pairs:
                        want[r, c, dst] = mark(r, c, src)
                if r == row and mode == ABB:
                    for dst, src in ABB_ROW:
                        want[r, c, dst] = -mark(r, c, src) + abb_value(src)
            for col, other, mode, bb, sp, wrap in ((C3 - 1, 0, e.col_hi, BB_COL_HI, SP_COL_HI, WRAP_COL_HI),
                                                   (0, C3 - 1, e.col_lo, BB_COL_LO, SP_COL_LO, WRAP_COL_LO)):   # columns win
                if c != col:
                    continue
                if mode in (BB, SP):
                    for dst, src in (bb if mode == BB else sp):
                        want[r, c, dst] = mark(r, c, src)
                if mode == WRAP and r == 1:
                    for q in wrap:
                        want[r, c, q] = mark(r, other, q)
    return want


@pytest.mark.parametrize("row_lo", er.ROW_MODES, ids=lambda m: "row_lo_" + er.MODE_NAME[m])
def test_every_population_arrives_where_the_drivers_put_it(row_lo):
    fc = marked_lattice()
    for e in er.all_edges(uw=UW):
        if e.row_lo != row_lo:
            continue
        got = er.stream(fc, e)
        want = table(e)
        assert not np.isnan(want).any()
        bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        assert bad.size == 0, f"{er.edges_name(e)}: (node r, c, slot) {bad[:8].tolist()} hold {[got[tuple(b)] for b in bad[:8]]}, " \
                              f"want {[want[tuple(b)] for b in bad[:8]]}"


def test_corners_spelled_out():
    """the four corners of two edge sets, every slot by hand.  Closed bounce-back box: the row and the column rule agree on
    the diagonal both claim.  Velocity rows with specular columns: they disagree, and the column wins slots 4, 7, 8 at
    column C-1 and 2, 5, 6 at column 0; the row keeps the other moving slots; slot 0 stays."""
    fc = marked_lattice()
    m = mark
    box = er.stream(fc, er.Edges(BB, BB, BB, BB, UW))
    assert box[0, 0].tolist() == [m(0, 0, 0), m(0, 0, 3), m(0, 0, 4), m(1, 0, 3), m(0, 1, 4), m(0, 0, 7), m(0, 0, 8), m(1, 1, 7), m(0, 0, 6)]
    assert box[0, 2].tolist() == [m(0, 2, 0), m(0, 2, 3), m(0, 1, 2), m(1, 2, 3), m(0, 2, 2), m(0, 2, 7), m(1, 1, 6), m(0, 2, 5), m(0, 2, 6)]
    assert box[2, 0].tolist() == [m(2, 0, 0), m(1, 0, 1), m(2, 0, 4), m(2, 0, 1), m(2, 1, 4), m(2, 0, 7), m(2, 0, 8), m(2, 0, 5), m(1, 1, 8)]
    assert box[2, 2].tolist() == [m(2, 2, 0), m(1, 2, 1), m(2, 1, 2), m(2, 2, 1), m(2, 2, 2), m(1, 1, 5), m(2, 2, 8), m(2, 2, 5), m(2, 2, 6)]

    def a(r, c, q):   # the anti-bounce-back value written to slot opposite of q
        return -m(r, c, q) + abb_value(q)

    ch = er.stream(fc, er.Edges(ABB, ABB, SP, SP, UW))
    for r in (0, 2):
        assert ch[r, 0].tolist() == [m(r, 0, 0), a(r, 0, 3), m(r, 0, 4), a(r, 0, 1), a(r, 0, 2), m(r, 0, 8), m(r, 0, 7), a(r, 0, 5), a(r, 0, 6)]
        assert ch[r, 2].tolist() == [m(r, 2, 0), a(r, 2, 3), a(r, 2, 4), a(r, 2, 1), m(r, 2, 2), a(r, 2, 7), a(r, 2, 8), m(r, 2, 6), m(r, 2, 5)]
        # a mid-row node of a velocity row: all eight moving populations replaced
        assert ch[r, 1].tolist() == [m(r, 1, 0), a(r, 1, 3), a(r, 1, 4), a(r, 1, 1), a(r, 1, 2), a(r, 1, 7), a(r, 1, 8), a(r, 1, 5), a(r, 1, 6)]
    # the same-row column copy leaves rows 0 and R-1 to the periodic wrap
    wr = er.stream(fc, er.Edges(PER, PER, WRAP, WRAP, UW))
    assert wr[1, 0].tolist() == [m(1, 0, 0), m(0, 0, 1), m(1, 2, 2), m(2, 0, 3), m(1, 1, 4), m(1, 2, 5), m(1, 2, 6), m(2, 1, 7), m(0, 1, 8)]
    assert wr[1, 2].tolist() == [m(1, 2, 0), m(0, 2, 1), m(1, 1, 2), m(2, 2, 3), m(1, 0, 4), m(0, 1, 5), m(2, 1, 6), m(1, 0, 7), m(1, 0, 8)]
    assert bits_equal(wr[0], er.advect(fc)[0]) and bits_equal(wr[2], er.advect(fc)[2])


def test_sealed_edges_conserve_the_marks():
    """bounce-back and specular edges move populations and create none: the streamed lattice is a permutation"""
    fc = marked_lattice()
    for e in er.all_edges(row_modes=(PER, BB), col_modes=(PER, BB, SP)):
        if (e.row_lo == PER) != (e.row_hi == PER) or (e.col_lo == PER) != (e.col_hi == PER):
            continue   # a wall facing a periodic edge is open: what leaves through the wrap is overwritten at the wall
        got = er.stream(fc, e)
        assert sorted(got.ravel().tolist()) == sorted(fc.ravel().tolist()), er.edges_name(e)
