"""CPU suite: the refusals of lbm_ibm_create / lbm_ibm_create_slab.  Every check of lbm_ibm_create_slab comes before
its first allocation, and the library loads where no device is visible (as in tests/test_abi.py), so these calls are
made here, without a GPU: each must return a non-zero code and a message that names the function.  (The refusals of
lbm_solver_attach_ibm need a solver, which needs a device: tests/test_gpu_ibm_markers.py.)  Also the host arithmetic
behind lbm_ibm_step's choice of kernel."""
import ctypes as ct

import numpy as np
import pytest

import ibm_util as iu
import pylbm
from pylbm import _hptr


@pytest.fixture(scope="module")
def lib():
    return pylbm.Lib()


def _create(lib, x, y, n, m_max, X, Y, row_offset=None, out=True):
    """the raw call: (code, message, handle value); row_offset None: lbm_ibm_create"""
    h = ct.c_void_p()
    xp = _hptr(np.ascontiguousarray(x, dtype=np.float64)) if x is not None else None
    yp = _hptr(np.ascontiguousarray(y, dtype=np.float64)) if y is not None else None
    outp = ct.byref(h) if out else None
    if row_offset is None:
        rc = lib.raw.lbm_ibm_create(outp, xp, yp, int(n), int(m_max), int(X), int(Y))
    else:
        rc = lib.raw.lbm_ibm_create_slab(outp, xp, yp, int(n), int(m_max), int(X), int(Y), int(row_offset))
    return rc, lib.raw.lbm_last_error_string().decode(), h.value


def _refused(res, what):
    rc, msg, h = res
    assert rc != 0 and "lbm_ibm_create" in msg and what in msg, (rc, msg)
    assert h is None          # nothing was handed out


@pytest.mark.parametrize("row_offset", [None, 0, 37])
def test_create_refuses_bad_arguments(lib, row_offset):
    x, y, X, Y = iu.tight_fit()
    x = x + (row_offset or 0)
    _refused(_create(lib, x, y, 0, 5, X, Y, row_offset), "bad argument")
    _refused(_create(lib, x, y, -3, 5, X, Y, row_offset), "bad argument")
    _refused(_create(lib, None, y, len(x), 5, X, Y, row_offset), "bad argument")
    _refused(_create(lib, x, None, len(x), 5, X, Y, row_offset), "bad argument")
    _refused(_create(lib, x, y, len(x), 5, X, Y, row_offset, out=False), "bad argument")
    _refused(_create(lib, x, y, len(x), 1, X, Y, row_offset), "m_max=1")
    _refused(_create(lib, x, y, len(x), 0, X, Y, row_offset), "m_max=0")


@pytest.mark.parametrize("row_offset", [None, 0, 37, 4080])
@pytest.mark.parametrize("side,dx,dy", [("first row", -1, 0), ("last row", 1, 0), ("first column", 0, -1), ("last column", 0, 1)])
def test_create_refuses_an_roi_one_node_too_far(lib, row_offset, side, dx, dy):
    """the tightest fit (one node left on each of the four sides) shifted by one node towards each side in turn, on a
    block and on a slab whose first row is the global row row_offset"""
    x, y, X, Y = iu.tight_fit()
    off = row_offset or 0
    r0, r1, c0, c1 = iu.roi_of(x + off, y)
    assert (r0 - off, r1 - off, c0, c1) == (1, X - 1, 1, Y - 1)      # the unshifted set is the tight fit
    _refused(_create(lib, x + off + dx, y + dy, len(x), 5, X, Y, row_offset), "strictly inside")
    # a lattice one row / column larger on that side would take it: the refusal is about the bound, not the set
    if dx > 0 or dy > 0:
        r0, r1, c0, c1 = iu.roi_of(x + off + dx, y + dy)
        assert (r0 - off, r1 - off, c0, c1) == (1 + dx, X - 1 + dx, 1 + dy, Y - 1 + dy)


def test_a_row_offset_moves_the_bound_with_it(lib):
    """global coordinates that fit a block do not fit a slab that starts elsewhere, and the other way round"""
    x, y, X, Y = iu.tight_fit()
    _refused(_create(lib, x, y, len(x), 5, X, Y, 1), "strictly inside")          # the slab starts one row later
    _refused(_create(lib, x + 37, y, len(x), 5, X, Y, None), "strictly inside")  # slab coordinates on a block
    _refused(_create(lib, x + 37, y, len(x), 5, X, Y, 36), "strictly inside")
    _refused(_create(lib, x + 37, y, len(x), 5, X, Y, 38), "strictly inside")


def test_the_eight_nodes_per_thread_kernels_cannot_be_reached():
    """lbm_ibm_step takes k_ibm_step<., 8> above 6144 touched nodes, and the launch chain above 150 KB of dynamic LDS,
    (3 n_touched + 2 n_markers) doubles.  A marker touches at most 16 nodes, so n_touched > 6144 needs n_markers >= 385,
    and the smallest such boundary already asks for 153 640 bytes: every boundary that would select 8 nodes per thread
    runs the launch chain instead (so does every one above 8192 touched nodes: that test never decides).  Exhaustive
    over the marker counts that matter, and confirmed on the sets of tests/test_gpu_ibm_markers.py."""
    for n_markers in range(1, 9601):                       # beyond 9600 markers the marker term alone exceeds the limit
        nt_min = 6145                                      # the fewest touched nodes that select 8 per thread
        if nt_min > 16 * n_markers:
            continue                                       # not enough markers to touch that many nodes
        assert (3 * nt_min + 2 * n_markers) * 8 > iu.LDS_LIMIT, n_markers
    assert 2 * 9601 * 8 > iu.LDS_LIMIT
    # the largest boundary that still takes one workgroup, and the first that does not
    x, y = iu.disjoint_grid(384)
    assert iu.n_touched(x, y) == 6144 and iu.lds_bytes(x, y) == iu.LDS_LIMIT and iu.own_of(x, y) == 6 and iu.takes_one_workgroup(x, y)
    x, y = iu.disjoint_grid(385)
    assert iu.own_of(x, y) == 8 and not iu.takes_one_workgroup(x, y)


def test_block_schedule_restatement():
    """ibm_util.expected_blocks, which the qualification tests of tests/test_gpu_ibm_default.py assert against: the
    known schedules of the existing tests (16 steps = 1 + three blocks of 5; 13 steps = 1 + 5 + 5 + 2)"""
    roi = (60, 90, 80, 110)
    assert iu.expected_blocks(176, 200, roi, 16) == 3 and iu.expected_blocks(176, 200, roi, 13) == 3
    assert iu.expected_blocks(176, 63, roi, 16) == 0
    assert iu.expected_blocks(176, 200, (11, 40, 80, 110), 16) == 1     # too close to the inlet for depth 5, not for 4
