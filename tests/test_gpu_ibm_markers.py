"""GPU tests of the forcing kernels against the oracle at the edges of the marker geometry: the tables that
lbm_ibm_create_slab builds on the host (Peskin weights, box0, the CSR in marker order, the touched list, the lane-major
ELL copies) and the rule by which lbm_ibm_step picks its kernel (4 / 6 touched nodes per thread, the launch chain above
150 KB of LDS).  Everything is compared BITWISE, in the reference order; the fields are random (|u| <= 0.25, rho 0.2 .. 5),
the lattice is the ROI plus a margin of three nodes unless the set says otherwise.  Every set is the smallest that reaches
its edge, and the test asserts that it does (touched nodes and pairs per node from the floor-based 4 x 4 boxes).
The refusals of lbm_solver_attach_ibm are here too: a solver needs a device (lbm_ibm_create's are in tests/test_ibm_abi.py)."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ibm_util as iu  # noqa: E402
import pylbm  # noqa: E402
from gpu_util import bits_equal, dev, download_aos, ulp_diff, upload_soa  # noqa: E402
from pylbm import _ptr  # noqa: E402

OMEGA, GUO_A, GUO_B = 1.0 / 0.55, 1.0 / 3.0, 1.0 / 9.0
# lbm_ibm_step under no tuning at all, under each form of the one-workgroup kernel, and as the launch chain
CONFIGS = [{}] + [{"ibm_step_opt": o, "ibm_step_split": s} for o in (0, 1) for s in (0, 1)] + [{"ibm_step_chain": 1}]


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1
    return lib


# ---- the sets: name -> (x, y, m_max, (X, Y) or None, property check) --------------------------------------------------
def _one():
    x, y = iu.one_marker()
    assert len(x) == 1 and iu.n_touched(x, y) == 16
    return x, y, 5, None


def _branch():
    x, y = iu.branch_points()
    frac = np.concatenate([x - np.floor(x), y - np.floor(y)])
    assert (frac == 0).any() and (frac == 0.5).any() and (frac == 1 - 2.0 ** -40).any()
    w = iu.tap_weights(x, y)
    assert (w == 0).any() and (w > 0).any() and (w >= 0).all()      # taps of weight exactly 0 where the branches meet
    on_grid = (x == np.floor(x)) | (y == np.floor(y))
    assert ((w == 0).sum(axis=1)[on_grid] >= 4).all()               # r = 2 exactly: a whole line of the box
    return x, y, 5, None


def _crowded(k):
    def make():
        x, y = iu.crowded(k)
        assert len(x) == k and (np.floor(x) == 7).all() and (np.floor(y) == 6).all()
        cnt = iu.pairs_per_node(x, y)
        assert iu.n_touched(x, y) == 16 and set(cnt[cnt > 0]) == {k}    # ell_deg = k, every node's count = k
        if k >= 2:
            assert x[1] == x[0] and y[1] == y[0]
        if k == 67:
            cx, cy = iu.circle(13.3, 13.6, 8.0)
            assert k > 4 * iu.pairs_per_node(cx, cy).max()              # far beyond what a circle gives
        return x, y, 5, None
    return make


def _shuffled():
    x, y, perm = iu.shuffled_circle()
    assert (np.abs(np.diff(perm)) > 1).sum() > len(x) // 2      # neighbours in index are not neighbours in space
    return x, y, 5, None


def _counted(n):
    def make():
        x, y = iu.counted_circle(n)
        assert len(x) == n and iu.takes_one_workgroup(x, y)
        return x, y, 5, None
    return make


def _disjoint(n):
    def make():
        x, y = iu.disjoint_grid(n)
        cnt = iu.pairs_per_node(x, y)
        assert cnt.max() == 1 and iu.n_touched(x, y) == 16 * n
        if n == 256:
            assert iu.n_touched(x, y) == 4096 and iu.own_of(x, y) == 4 and iu.takes_one_workgroup(x, y)
        elif n == 257:
            assert iu.own_of(x, y) == 6 and iu.takes_one_workgroup(x, y)
        elif n == 384:   # the largest one-workgroup launch the library will make: exactly the 150 KB limit
            assert iu.n_touched(x, y) == 6144 and iu.own_of(x, y) == 6
            assert iu.lds_bytes(x, y) == 153600 == iu.LDS_LIMIT and iu.takes_one_workgroup(x, y)
        else:            # the automatic launch chain
            assert iu.lds_bytes(x, y) > iu.LDS_LIMIT and not iu.takes_one_workgroup(x, y)
        return x, y, 5, None
    return make


def _m_max(m):
    def make():
        x, y = iu.circle(9.3, 9.6, 6.0)
        return x, y, m, None
    return make


def _tight():
    x, y, X, Y = iu.tight_fit()
    r0, r1, c0, c1 = iu.roi_of(x, y)
    assert (r0, r1, c0, c1) == (1, X - 1, 1, Y - 1)
    return x, y, 5, (X, Y)


SETS = {"one_marker": _one, "branch_points": _branch, "shuffled_circle": _shuffled, "tight_fit": _tight}
SETS.update({f"crowded_{k}": _crowded(k) for k in (1, 2, 3, 4, 5, 67)})
SETS.update({f"circle_of_{n}": _counted(n) for n in (63, 64, 65, 1025)})
SETS.update({f"disjoint_{n}": _disjoint(n) for n in (256, 257, 384, 385, 400)})
SETS.update({f"m_max_{m}": _m_max(m) for m in (2, 3, 5, 8)})


def test_the_crowded_sets_reach_every_remainder_of_the_pair_fetch():
    assert {k % 4 for k in (1, 2, 3, 4, 5, 67)} == {0, 1, 2, 3} and 1025 > 1024


def _check_forcing(lib, oracle, x, y, m_max, X, Y, u, rho, p, want_F, roi_want, row_offset=0, seed_tag=""):
    """the three checks on one boundary object of an X x Y block / slab whose first row is the global row row_offset;
    u, rho, p: the block's own rows; want_F: the oracle's F on the ROI; roi_want: the ROI in the block's rows"""
    ib = pylbm.Ibm(lib, x, y, X, Y, m_max=m_max, row_offset=row_offset)
    assert ib.roi() == roi_want
    r0, r1, c0, c1 = roi_want
    ud, rd = upload_soa(lib, u), upload_soa(lib, rho)
    geom = pylbm.Geom(X, Y, 0)
    # 1. the launch chain's F
    F = torch.empty((2, r1 - r0, c1 - c0), dtype=torch.float64, device=dev())
    lib.ibm_force(ib.h, _ptr(ud), _ptr(rd), _ptr(F), None)
    got_F = download_aos(lib, F)
    assert bits_equal(got_F, want_F), ulp_diff(got_F, want_F)
    Fs_want = want_F.reshape(-1, 2).sum(0)
    assert np.allclose(ib.surface_force(), Fs_want, rtol=1e-12, atol=1e-15)
    # 2. the lattice after the source term: numpy on the oracle's F, the two separate calls, lbm_ibm_step in every form
    want_p = iu.add_source(p, roi_want, u, want_F, OMEGA, GUO_A, GUO_B)
    assert not bits_equal(want_p, p)
    outside_roi = np.ones((X, Y), dtype=bool)
    outside_roi[r0:r1, c0:c1] = False
    untouched = np.ones((X, Y), dtype=bool)
    untouched[r0:r1, c0:c1] = iu.pairs_per_node(x, y) == 0
    pd = upload_soa(lib, p)
    lib.ibm_add_source(ib.h, _ptr(pd), ct.byref(geom), _ptr(ud), ct.c_double(OMEGA), ct.c_double(GUO_A), ct.c_double(GUO_B), None)
    got = download_aos(lib, pd)
    assert bits_equal(got, want_p), ("force + add_source", ulp_diff(got, want_p))
    for tune in CONFIGS:
        try:
            for k, v in tune.items():
                lib.set_tuning(k.encode(), v)
            pd = upload_soa(lib, p)
            lib.ibm_step(ib.h, _ptr(pd), ct.byref(geom), _ptr(ud), _ptr(rd), ct.c_double(OMEGA), ct.c_double(GUO_A),
                         ct.c_double(GUO_B), None)
            torch.cuda.synchronize()
            got, Fs = download_aos(lib, pd), ib.surface_force()
        finally:
            for k in iu.IBM_STEP_KEYS:
                lib.set_tuning(k.encode(), -1)
        assert bits_equal(got, want_p), (seed_tag, tune, ulp_diff(got, want_p))
        assert bits_equal(got[outside_roi], p[outside_roi]), tune          # not one bit outside the ROI
        if tune.get("ibm_step_split", 1) and not tune.get("ibm_step_chain"):
            assert bits_equal(got[untouched], p[untouched]), tune          # nor outside the touched nodes
        # 3. the surface force of this very launch
        assert np.allclose(Fs, Fs_want, rtol=1e-12, atol=1e-15), (tune, Fs, Fs_want)
    ib.close()


@pytest.mark.parametrize("name", sorted(SETS))
def test_marker_set_vs_oracle(lib, oracle, name):
    x, y, m_max, lattice = SETS[name]()
    X, Y = lattice or iu.lattice_around(x, y)
    assert X <= 88 and Y <= 88
    u, rho, p = iu.random_fields(X, Y, seed=len(name) + len(x))
    want_F = oracle.ibm_force(x, y, u, rho, m_max=m_max)
    assert np.abs(want_F).max() > 1e-3
    assert oracle.ibm_roi(x, y) == iu.roi_of(x, y)
    if name == "shuffled_circle":   # the spread follows marker index: the sorted circle gives other bits
        xs, ys = iu.circle(13.3, 13.6, 8.0)
        sorted_F = oracle.ibm_force(xs, ys, u, rho)
        assert sorted_F.shape == want_F.shape and not bits_equal(sorted_F, want_F)
        assert np.allclose(sorted_F, want_F, rtol=1e-9, atol=1e-12)        # (the same boundary all the same)
    _check_forcing(lib, oracle, x, y, m_max, X, Y, u, rho, p, want_F, oracle.ibm_roi(x, y), seed_tag=name)


def test_m_max_changes_the_result(oracle):
    """(the four m_max sets are four different answers)"""
    x, y = iu.circle(9.3, 9.6, 6.0)
    X, Y = iu.lattice_around(x, y)
    u, rho, _ = iu.random_fields(X, Y, seed=3)
    F = [oracle.ibm_force(x, y, u, rho, m_max=m) for m in (2, 3, 5, 8)]
    assert all(not bits_equal(F[i], F[i + 1]) for i in range(3))


def test_large_coordinates_and_a_slab_offset(lib, oracle):
    """A radius-6 circle centred near row 4100.37 of a 4120 x 40 lattice, as one block and as the boundary of a 40-row
    slab that starts at row 4080: the weights come from the global coordinates minus the ROI origin, only the stored
    origin is slab-local.  Both equal the oracle on the big lattice."""
    X, Y, off, R = 4120, 40, 4080, 40
    x, y = iu.circle(4100.37, 20.21, 6.0)
    u, rho, p = iu.random_fields(X, Y, seed=17)
    want_F = oracle.ibm_force(x, y, u, rho)
    r0, r1, c0, c1 = oracle.ibm_roi(x, y)
    assert off < r0 and r1 < off + R and r0 > 4000
    _check_forcing(lib, oracle, x, y, 5, X, Y, u, rho, p, want_F, (r0, r1, c0, c1))
    _check_forcing(lib, oracle, x, y, 5, R, Y, u[off:], rho[off:], p[off:], want_F, (r0 - off, r1 - off, c0, c1), row_offset=off)


def test_tight_fit_with_a_row_offset(lib, oracle):
    """the tightest fit inside a slab that starts at global row 37"""
    x, y, X, Y = iu.tight_fit()
    off = 37
    u, rho, p = iu.random_fields(off + X, Y, seed=23)
    want_F = oracle.ibm_force(x + off, y, u, rho)
    _check_forcing(lib, oracle, x + off, y, 5, X, Y, u[off:], rho[off:], p[off:], want_F, (1, X - 1, 1, Y - 1), row_offset=off)


# ---- refusals that need a solver, hence a device ------------------------------------------------------------------------
def _refused(lib, rc, name):
    msg = lib.raw.lbm_last_error_string().decode()
    assert rc != 0 and name in msg, (rc, msg)
    return msg


def test_attach_refuses_a_kbc_solver_and_an_roi_on_the_edge(lib):
    x, y, X, Y = iu.tight_fit()
    ib = pylbm.Ibm(lib, x, y, X, Y)
    kbc = pylbm.Solver(lib, pylbm.MODEL_KBC, X, Y, pylbm.KbcParams(1.9))
    rc = lib.raw.lbm_solver_attach_ibm(kbc.h, ib.h, ct.c_double(GUO_A), ct.c_double(GUO_B))
    assert "BGK solvers only" in _refused(lib, rc, "lbm_solver_attach_ibm")
    kbc.close()
    # the boundary of an X x Y lattice on solvers one row / one column smaller: the ROI touches their last row / column
    for R, C in ((X - 1, Y), (X, Y - 1)):
        sv = pylbm.Solver(lib, pylbm.MODEL_BGK, R, C, pylbm.BgkParams(1.2, 0, 1))
        rc = lib.raw.lbm_solver_attach_ibm(sv.h, ib.h, ct.c_double(GUO_A), ct.c_double(GUO_B))
        assert "strictly inside" in _refused(lib, rc, "lbm_solver_attach_ibm")
        sv.close()
    sv = pylbm.Solver(lib, pylbm.MODEL_BGK, X, Y, pylbm.BgkParams(1.2, 0, 1))
    sv.attach_ibm(ib)          # the tight fit itself is accepted
    sv.close(); ib.close()
