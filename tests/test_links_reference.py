"""The yardstick of the link / wall-term / force-row tests (tests/links_reference.py) against what is already pinned:
apply_slices glues a periodic box cut into four unequal blocks back together so that it equals oracle.advect (pinned by the
golden vectors) of the whole box bit for bit, and wall_terms / force_rows give their hand-computed known answers."""
import numpy as np
import pytest

import links_reference as lr

ROWS, COLS = (5, 3), (6, 4)


def box(R, C, seed=0):
    """[9, R, C] with every element distinct"""
    rng = np.random.default_rng(seed)
    return (rng.permutation(9 * R * C).astype(np.float64) + 1.0).reshape(9, R, C) / 64.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle_advect(oracle, a):
    return np.ascontiguousarray(oracle.advect(np.ascontiguousarray(a.transpose(1, 2, 0))).transpose(2, 0, 1))


def glued(a, rows, cols, corners=True):
    src = lr.split(a, rows, cols)
    dst = [lr.advect_alone(b) for b in src]
    lr.apply_slices(lr.split_slices(rows, cols, corners), dst, src)
    return lr.join(dst, rows, cols)


def test_split_box_glued_by_slices_equals_oracle_advect(oracle):
    a = box(sum(ROWS), sum(COLS))
    want = oracle_advect(oracle, a)
    assert np.array_equal(bits(lr.join(lr.split(a, ROWS, COLS), ROWS, COLS)), bits(a))
    assert not np.array_equal(bits(lr.join([lr.advect_alone(b) for b in lr.split(a, ROWS, COLS)], ROWS, COLS)), bits(want))
    assert np.array_equal(bits(glued(a, ROWS, COLS)), bits(want))


def test_without_the_corner_slices_the_result_differs(oracle):
    """the order and "the later slice wins" matter on this input: the row and column slices both leave the corner element of
    every diagonal population wrong"""
    a = box(sum(ROWS), sum(COLS))
    want = oracle_advect(oracle, a)
    got = glued(a, ROWS, COLS, corners=False)
    wrong = np.argwhere(bits(got) != bits(want))
    assert len(wrong) == 16                      # 4 blocks x 4 diagonal populations, one corner element each
    assert {int(q) for q, _, _ in wrong} == {5, 6, 7, 8}
    n = len(lr.split_slices(ROWS, COLS))
    assert n - len(lr.split_slices(ROWS, COLS, corners=False)) == 16


def test_later_slice_wins_whole_and_in_place_reads_the_old_values():
    a = box(4, 5, 1)
    add = np.array([0.5, 0.25])
    d = [np.zeros((9, 4, 5))]
    lr.apply_slices([(0, 1, 0, 0, 0, 1, 0, 3, 1, 0, 0, 1, 5, -1.0, 0, 0), (0, 1, 0, 2, 0, 1, 0, 4, 2, 2, 0, 1, 2)], d, [a], add)
    want = -1.0 * a[3, 1] + 0.5
    want[2:4] = a[4, 2, 2:4]                     # the plain slice took scale and addend with it
    assert np.array_equal(bits(d[0][1, 0]), bits(want))
    assert lr.link_map([(0, 1, 0, 0, 0, 1, 0, 3, 1, 0, 0, 1, 5, -1.0, 0, 0), (0, 1, 0, 2, 0, 1, 0, 4, 2, 2, 0, 1, 2)])[(0, 1, 0, 2)] \
        == (0, (4, 2, 2), 1.0, -1)
    b = a.copy()                                 # in place: row 0 from row 1, both sides the same array
    lr.apply_slices([(0, q, 0, 0, 0, 1, 0, q, 1, 0, 0, 1, 5) for q in range(9)], [b], [b])
    assert np.array_equal(bits(b[:, 0]), bits(a[:, 1])) and np.array_equal(bits(b[:, 1:]), bits(a[:, 1:]))
    with pytest.raises(ValueError, match="chain"):  # row 0 from row 1 and row 1 from row 2 in one list
        lr.apply_slices([(0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 5), (0, 0, 1, 0, 0, 1, 0, 0, 2, 0, 0, 1, 5)], [b], [b])
    lr.apply_slices([(0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 5), (0, 0, 1, 0, 0, 1, 0, 0, 2, 0, 0, 1, 5)], [b], [b.copy()])
    with pytest.raises(IndexError):
        lr.apply_slices([(0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 6)], [np.zeros((9, 4, 5))], [a])


def test_wall_terms_at_rest():
    """u = 0: mode 0 gives factor * 2 w_q, mode 1 factor * w_q * field[r]"""
    X, Y = 7, 3
    u = np.zeros((2, X, Y))
    field = np.arange(1, X + 1) / 8.0
    for factor in (1.0, 2.0, -0.5):
        t0 = lr.wall_terms(u, Y - 1, 1.5, Y - 2, -0.5, 0.0, 0, None, factor)
        assert np.array_equal(bits(t0), bits(np.tile(factor * (2.0 * lr.W9), (X, 1))))
        t1 = lr.wall_terms(u, 0, 1.0, 0, 0.0, 0.0, 1, field, factor)
        assert np.array_equal(bits(t1), bits(factor * (lr.W9[None, :] * field[:, None])))


def test_wall_terms_known_answer():
    """one node, uw = (1/4, 1/8), every product exact in binary: (2 + 9 (uw.c)^2 - 3 uw.uw) w_q by hand"""
    u = np.array([0.5, 0.25]).reshape(2, 1, 1)
    got = lr.wall_terms(u, 0, 0.5, 0, 0.0, 0.0, 0, None, 1.0)[0]
    uc = np.array([0, 1 / 4, 1 / 8, -1 / 4, -1 / 8, 3 / 8, -1 / 8, -3 / 8, 1 / 8])
    assert np.array_equal(bits(got), bits((2.0 + 9.0 * uc ** 2 - 3.0 * (5 / 64)) * lr.W9))
    u2 = np.array([0.5, 0.25, 4.0, -8.0]).reshape(2, 1, 2)      # 1.5 u[-1] - 0.5 u[-2] + shift, columns (a, b) = (1, 0)
    w = lr.wall_terms(u2, 1, 1.5, 0, -0.5, 0.125, 1, np.array([2.0]), 1.0)[0]
    w0, w1 = 1.5 * 0.25 - 0.5 * 0.5 + 0.125, 1.5 * -8.0 - 0.5 * 4.0 + 0.125
    want = ((((1.0 + 3.0 * w0) + 4.5 * (w0 * w0)) - 1.5 * (w0 * w0 + w1 * w1)) * (1 / 9)) * 2.0   # q = 1: uw.c = w0
    assert np.array_equal(bits(w[1]), bits(want))


def test_force_rows_known_answers():
    rng = np.random.default_rng(3)
    p = lr.W9[:, None, None] * (1 + 0.05 * rng.random((9, 6, 5)))
    u = 0.05 * rng.standard_normal((2, 6, 5))
    assert np.array_equal(bits(lr.force_rows(p, u, 1.2, 0.0, 0.0, 3.0, 9.0, 0, 6)), bits(p))       # F = 0: p unchanged
    got = lr.force_rows(p, u, 1.2, 3e-3, -1e-3, 3.0, 9.0, 2, 4)
    assert np.array_equal(bits(got[:, :2]), bits(p[:, :2])) and np.array_equal(bits(got[:, 4:]), bits(p[:, 4:]))
    assert (bits(got[1:, 2:4]) != bits(p[1:, 2:4])).all()
    assert np.array_equal(bits(lr.force_rows(p, u, 1.2, 3e-3, -1e-3, 3.0, 9.0, 3, 3)), bits(p))   # the empty range
    # u = 0, omega = 1, F = (1/4, 0), (a, b) = (3, 9): S_q = 0.5 * 3 * c_qx / 4 * w_q
    z = np.zeros((9, 1, 1))
    s = lr.force_rows(z, np.zeros((2, 1, 1)), 1.0, 0.25, 0.0, 3.0, 9.0, 0, 1)[:, 0, 0]
    assert np.array_equal(bits(s + 0.0), bits(0.375 * lr.CX * lr.W9 + 0.0))
