"""Part 8 of the C ABI (csrc/capi_links.hip) kernel by kernel: the link gather and its affine form, lbm_wall_terms,
lbm_pressure_row, lbm_bgk_add_force_rows and lbm_axpb against tests/links_reference.py (plain numpy, pinned on the CPU by
tests/test_links_reference.py) and the oracle's advect / equilibrium -- bit for bit, the file is built with
-ffp-contract=off and numpy does not fuse.  Every destination is an allocation poisoned with a NaN no kernel computes, ghost
rows and padding included, and every test asserts two things: the doubles that changed are EXACTLY the ones the call names,
and each of them has the reference's bits."""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import links_reference as lr  # noqa: E402
import pylbm  # noqa: E402
from gpu_util import dev  # noqa: E402
from pylbm import _ptr  # noqa: E402

SENTINEL = 0x7FF8DEADBEEF5A5A       # a quiet NaN no kernel computes: "never written" (tests/test_gpu_write_sets.py)
_dp = ct.POINTER(ct.c_double)


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1
    yield lib
    lib.reset_tuning()


# ---- lattices --------------------------------------------------------------------------------------------------------------
class Lat:
    """a lattice geometry and where its doubles lie: plane q at q * plane, owned row r at row r + ghost, row pitch P"""

    def __init__(self, R, C, ghost=0, pad=0, pitch=0):
        self.R, self.C, self.ghost, self.P = R, C, ghost, pitch or C
        self.plane = (R + 2 * ghost) * self.P + pad
        self.n = 9 * self.plane
        # plane_stride 0 = "dense" where that is what the lattice is: the library's default path
        self.g = pylbm.Geom(R, C, ghost, self.plane if (pad or pitch) else 0, pitch)
        q, r, c = np.meshgrid(np.arange(9), np.arange(R), np.arange(C), indexing="ij")
        self.off = q * self.plane + (r + ghost) * self.P + c          # [9, R, C] -> index into the flat allocation

    def distinct(self, k):
        """a flat allocation in which every double -- ghost rows and padding too -- is distinct, also from lattice k' != k"""
        return (1.0 + 100000.0 * k + np.arange(self.n)) / 8.0

    def near_w(self, seed):
        rng = np.random.default_rng(seed)
        return (np.repeat(lr.W9, self.plane) * (1.0 + 0.05 * rng.random(self.n)))

    def mask(self, elements):
        m = np.zeros(self.n, dtype=bool)
        for e in elements:
            m[self.off[e]] = True
        return m


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev())


def poisoned(n):
    t = torch.empty(n, dtype=torch.float64, device=dev())
    t.view(torch.int64).fill_(SENTINEL)
    return t


def down_bits(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def nan_like(shape):
    return np.full(shape, SENTINEL, dtype=np.uint64).view(np.float64)


def assert_same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{what}: {len(bad)} doubles differ; first at {tuple(bad[0])}: "
                           f"{int(got[tuple(bad[0])]):#018x} != {int(want[tuple(bad[0])]):#018x}")


def assert_write_set(flat_bits, want_mask, what):
    """of an allocation that was SENTINEL everywhere: exactly the doubles of want_mask changed"""
    bad = np.flatnonzero((flat_bits != np.uint64(SENTINEL)) != want_mask)
    assert len(bad) == 0, (f"{what}: {len(bad)} doubles wrong; first flat index {bad[0]} "
                           f"({'MISSED' if want_mask[bad[0]] else 'OVER-WRITTEN'})")


# ---- link tables -----------------------------------------------------------------------------------------------------------
def make_table(lib, lats, slices):
    t = ct.c_void_p()
    geoms = (pylbm.Geom * len(lats))(*[la.g for la in lats])
    lib.links_create(ct.byref(t), len(lats), geoms)
    for s in slices:
        if len(s) == 13:
            lib.links_add(t, *[int(x) for x in s])
        else:
            lib.links_add_affine(t, *[int(x) for x in s[:13]], ct.c_double(s[13]), ct.c_longlong(s[14]), ct.c_longlong(s[15]))
    return t


def ptrs(tensors):
    return (_dp * len(tensors))(*[_ptr(t) for t in tensors])


def apply_table(lib, t, dst, src, addends=None, affine_call=False):
    if addends is not None or affine_call:
        lib.links_apply_affine(t, ptrs(dst), ptrs(src), _ptr(addends), None)
    else:
        lib.links_apply(t, ptrs(dst), ptrs(src), None)
    torch.cuda.synchronize()


def run_links(lib, lats, slices, addends=None, affine_call=False, plant=()):
    """the table of `slices` over `lats`, applied once from distinct sources into poisoned destinations: lbm_links_count, the
    write set of every lattice (whole allocation) and the bits of every owned element against apply_slices;
    plant: ((lattice, (q, r, c), value), ...) put into the sources first"""
    links = lr.link_map(slices)
    src_flat = [la.distinct(k) for k, la in enumerate(lats)]
    for k, e, v in plant:
        src_flat[k][lats[k].off[e]] = v
    t = make_table(lib, lats, slices)
    try:
        assert lib.raw.lbm_links_count(t) == len(links)
        lib.links_finalize(t)
        assert lib.raw.lbm_links_count(t) == len(links)
        src = [up(a) for a in src_flat]
        dst = [poisoned(la.n) for la in lats]
        apply_table(lib, t, dst, src, up(addends) if addends is not None else None, affine_call)
    finally:
        lib.links_destroy(t)
    want = [nan_like((9, la.R, la.C)) for la in lats]
    lr.apply_slices(slices, want, [a[la.off] for a, la in zip(src_flat, lats)], addends)
    for k, la in enumerate(lats):
        got = down_bits(dst[k])
        assert_write_set(got, la.mask([d[1:] for d in links if d[0] == k]), f"lattice {k}")
        assert_same_bits(got[la.off], bits(want[k]), f"lattice {k}")


def eight_lattices():
    """the four shapes twice: dense, ghost rows with a padded plane, more than one wave per row, an odd width"""
    four = [dict(R=7, C=6), dict(R=5, C=6, ghost=2, pad=40), dict(R=16, C=64), dict(R=9, C=65, ghost=1, pad=24)]
    lats = [Lat(**kw) for kw in four + four]
    assert lats[1].plane == (5 + 4) * 6 + 40
    return lats


GATHER = [
    (0, 1, 0, 0, 0, 1, 1, 3, 4, 0, 0, 1, 6),          # a row of the dense lattice from the last owned row of a ghost-row one
    (1, 2, 0, 5, 1, 0, 0, 4, 1, 0, 1, 0, 5),          # a column, every owned row of the ghost-row lattice
    (1, 7, 4, 0, 0, 1, 2, 6, 9, 7, 0, 1, 6),          # its last owned row (the ghost rows behind it stay poisoned)
    (2, 5, 0, 0, 1, 1, 3, 7, 0, 10, 1, 1, 9),         # a diagonal, dr = dc = 1 on both sides
    (3, 6, 8, 64, 0, -1, 2, 8, 15, 0, 0, 1, 64),      # destination reversed, source forward
    (6, 2, 3, 0, 0, 1, 7, 2, 8, 64, 0, -1, 64),       # source reversed, destination forward; lattice 7 as a source
    (7, 4, 8, 3, -1, 0, 3, 4, 8, 64, -1, 0, 9),       # both reversed; lattice 7 as a destination
    (7, 2, 0, 0, 0, 1, 7, 5, 4, 1, 0, 1, 64),         # lattice 7 to lattice 7
    (4, 0, 6, 5, 5, 5, 5, 0, 4, 5, 3, 3, 0),          # count 0: nothing, whatever the strides
    (4, 0, 6, 5, 0, 0, 5, 8, 4, 5, 0, 0, 1),          # count 1: the last element of the lattice
    (5, 3, 2, 0, 0, 1, 4, 3, 6, 0, 0, 1, 6),
    (5, 3, 2, 2, 0, 1, 0, 1, 3, 1, 0, 1, 3),          # overrides three elements of the slice before from another lattice
]


def test_gather_over_eight_lattices(lib):
    run_links(lib, eight_lattices(), GATHER)


def test_gather_without_the_override_differs():
    """the input makes "the later slice wins" visible: the yardstick itself gives other values without the last slice"""
    lats = eight_lattices()
    src = [la.distinct(k)[la.off] for k, la in enumerate(lats)]
    a = lr.apply_slices(GATHER, [np.zeros((9, la.R, la.C)) for la in lats], src)
    b = lr.apply_slices(GATHER[:-1], [np.zeros((9, la.R, la.C)) for la in lats], src)
    assert int((bits(a[5]) != bits(b[5])).sum()) == 3


def counted_slices(n):
    """n distinct destination elements in lattice 2 (16 x 64) from lattice 6 reversed, the first of them written twice"""
    s = [(2, 1, i, 0, 0, 1, 6, 2, 15 - i, 63, 0, -1, 64) for i in range(n // 64)]
    if n % 64:
        s.append((2, 1, n // 64, 0, 0, 1, 6, 2, 15 - n // 64, 63, 0, -1, n % 64))
    s.append((2, 1, 0, 0, 0, 1, 3, 8, 8, 64, 0, -1, min(n, 10)))
    return s


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_link_count_against_the_block(lib, n):
    slices = counted_slices(n)
    assert len(lr.link_map(slices)) == n
    run_links(lib, eight_lattices(), slices)


@pytest.mark.parametrize("affine_call", [False, True])
def test_empty_table_is_a_no_op(lib, affine_call):
    run_links(lib, eight_lattices(), [(4, 0, 6, 5, 5, 5, 5, 0, 4, 5, 3, 3, 0)], affine_call=affine_call)
    run_links(lib, eight_lattices(), [], affine_call=affine_call)


AFFINE = [
    (0, 1, 0, 0, 0, 1, 1, 3, 4, 0, 0, 1, 6, -1.0, 0, 1),             # anti-bounce-back: -src + addends[k]
    (0, 2, 6, 0, 0, 1, 4, 2, 0, 0, 0, 1, 6, -1.0, 5, -1),            # a negative stride that stays at >= 0
    (1, 2, 0, 5, 1, 0, 0, 4, 1, 0, 1, 0, 5, 0.5, 7, 0),              # stride 0: one addend for the slice
    (3, 6, 8, 64, 0, -1, 2, 8, 15, 0, 0, 1, 64, -0.25, 3, 9),        # stride 9: the driver's per-row layout
    (2, 5, 0, 0, 1, 1, 3, 7, 0, 10, 1, 1, 9, 1.0, 20, 1),            # scale 1 with an addend
    (6, 2, 3, 0, 0, 1, 7, 2, 8, 64, 0, -1, 64, -1.0, -1, 0),         # scale -1 without one (the zeros are planted here)
    (7, 4, 8, 3, -1, 0, 3, 4, 8, 64, -1, 0, 9),                      # a plain link in an affine table
    (5, 3, 2, 0, 0, 1, 4, 3, 6, 0, 0, 1, 6, -1.0, 40, 1),
    (5, 3, 2, 2, 0, 1, 0, 1, 3, 1, 0, 1, 3),                         # plain over affine: scale and addend are gone
    (4, 0, 0, 0, 0, 1, 5, 8, 4, 0, 0, 1, 6),
    (4, 0, 0, 1, 0, 1, 1, 2, 0, 1, 0, 1, 4, 0.5, 50, 1),             # affine over plain
    (1, 7, 4, 0, 0, 1, 2, 6, 9, 7, 0, 1, 6, 0.5, -1, 0),
    (1, 7, 4, 3, 0, 1, 6, 1, 2, 2, 0, 1, 2, -0.25, 60, 0),           # affine over affine: source, scale and addend together
]
ZEROS = ((7, (2, 8, 10), 0.0), (7, (2, 8, 11), -0.0))


def addend_array():
    n = 3 + 63 * 9 + 1                                                 # the largest index any slice above reaches, + 1
    assert n == 1 + max(ai for _, _, _, ai in lr.link_map(AFFINE).values())
    return 0.001 * (1.0 + np.random.default_rng(5).random(n))


def test_affine_over_eight_lattices(lib):
    run_links(lib, eight_lattices(), AFFINE, addends=addend_array(), plant=ZEROS)


def test_affine_input_shows_signed_zeros_and_overrides():
    """what the affine case relies on, on the yardstick alone: -1 * (+0.0) and -1 * (-0.0) differ in bits, and each override
    changes the result of its element"""
    lats = eight_lattices()
    src = [la.distinct(k)[la.off] for k, la in enumerate(lats)]
    for k, e, v in ZEROS:
        src[k][e] = v
    add = addend_array()

    def run(slices):
        return lr.apply_slices(slices, [np.zeros((9, la.R, la.C)) for la in lats], src, add)

    full = run(AFFINE)
    z = bits(full[6][2, 3])                                            # destination column k <- source column 64 - k
    assert z[54] == bits(np.float64(-0.0)) and z[53] == bits(np.float64(0.0))
    for drop, lat in ((8, 5), (10, 4), (12, 1)):
        other = run(AFFINE[:drop] + AFFINE[drop + 1:])
        assert (bits(other[lat]) != bits(full[lat])).any()


def test_plain_table_through_the_affine_entry_point(lib):
    run_links(lib, eight_lattices(), GATHER, affine_call=True)


# ---- composition: four blocks of a periodic box, each streamed alone, glued by one gather ------------------------------------
@pytest.mark.parametrize("rows, cols", [((5, 3), (6, 4)), ((33, 31), (70, 58))])
def test_split_box_glued_by_one_gather_equals_oracle_advect(lib, oracle, rows, cols):
    R, C = sum(rows), sum(cols)
    a = (np.random.default_rng(2).permutation(9 * R * C).astype(np.float64) + 1.0).reshape(9, R, C) / 64.0
    want = np.ascontiguousarray(oracle.advect(np.ascontiguousarray(a.transpose(1, 2, 0))).transpose(2, 0, 1))
    blocks = lr.split(a, rows, cols)
    lats = [Lat(b.shape[1], b.shape[2]) for b in blocks]
    slices = lr.split_slices(rows, cols)
    coll = [up(b.reshape(-1)) for b in blocks]
    adve = [poisoned(la.n) for la in lats]
    t = make_table(lib, lats, slices)
    try:
        lib.links_finalize(t)
        n = lib.raw.lbm_links_count(t)
        assert n == len(lr.link_map(slices))
        assert n > 256 or R < 64
        for la, d, s in zip(lats, adve, coll):
            lib.advect(_ptr(d), _ptr(s), la.R, la.C, None)
        apply_table(lib, t, adve, coll)
    finally:
        lib.links_destroy(t)
    got = lr.join([down_bits(d).reshape(9, la.R, la.C) for d, la in zip(adve, lats)], rows, cols)
    assert_same_bits(got, bits(want), "joined blocks")


# ---- in place: the zero-gradient pair of the sedimentation driver -------------------------------------------------------------
def in_place_tables(lib, la):
    R, C = la.R, la.C
    z1 = make_table(lib, [la], [(0, q, 0, 0, 0, 1, 0, q, 1, 0, 0, 1, C) for q in range(9)])
    z2 = make_table(lib, [la], [(0, q, 1, C - 1, 1, 0, 0, q, 1, C - 2, 1, 0, R - 2) for q in range(9)])
    return z1, z2


@pytest.mark.parametrize("R, C", [(5, 4), (9, 70)])
def test_in_place_tables_one_after_the_other(lib, R, C):
    la = Lat(R, C)
    a = la.distinct(0)
    t = up(a)
    z1, z2 = in_place_tables(lib, la)
    try:
        for z in (z1, z2):
            lib.links_finalize(z)
            apply_table(lib, z, [t], [t])
    finally:
        lib.links_destroy(z1)
        lib.links_destroy(z2)
    want = a.reshape(9, R, C).copy()
    want[:, 0] = want[:, 1]
    want[:, 1:R - 1, C - 1] = want[:, 1:R - 1, C - 2]
    assert_same_bits(down_bits(t).reshape(9, R, C), bits(want), "g_coll")


def test_in_place_chain_is_refused(lib):
    """one table in which a link reads what another writes, applied with dst == src, would depend on the order of the
    threads: refused on the host, naming the two lattices, with the buffer untouched; on separate buffers the same table is
    fine, and so is the in-place use that aliases a lattice no link writes"""
    la = Lat(5, 4)
    chain = [(0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 4), (0, 0, 1, 0, 0, 1, 0, 0, 2, 0, 0, 1, 4)]
    a = la.distinct(0)
    t = make_table(lib, [la], chain)
    try:
        lib.links_finalize(t)
        buf = up(a)
        for affine_call in (False, True):
            with pytest.raises(pylbm.LbmError, match=r"in-place chain: dst\[0\] and src\[0\]"):
                apply_table(lib, t, [buf], [buf], affine_call=affine_call)
        assert_same_bits(down_bits(buf), bits(a), "the buffer after the refusal")
        dst = poisoned(la.n)
        apply_table(lib, t, [dst], [buf])
        want = lr.apply_slices(chain, [nan_like((9, 5, 4))], [a.reshape(9, 5, 4)])
        assert_same_bits(down_bits(dst).reshape(9, 5, 4), bits(want[0]), "separate buffers")
    finally:
        lib.links_destroy(t)
    # two lattices: lattice 0 is written at rows 0 and 1, lattice 1 read at rows 1 and 0
    cross = [(0, 0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1, 4), (0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 4)]
    t = make_table(lib, [la, la], cross)
    try:
        lib.links_finalize(t)
        x, y = up(a), up(la.distinct(1))
        with pytest.raises(pylbm.LbmError, match=r"in-place chain: dst\[0\] and src\[1\]"):
            apply_table(lib, t, [x, y], [y, x])
        assert_same_bits(down_bits(x), bits(a), "x after the refusal")
        assert_same_bits(down_bits(y), bits(la.distinct(1)), "y after the refusal")
        apply_table(lib, t, [x, y], [y, y])       # dst[1] == src[1]: no link writes lattice 1
        y_np = la.distinct(1).reshape(9, 5, 4)
        want = lr.apply_slices(cross, [a.reshape(9, 5, 4).copy(), y_np.copy()], [np.zeros((9, 5, 4)), y_np])
        assert_same_bits(down_bits(x).reshape(9, 5, 4), bits(want[0]), "lattice 0")
    finally:
        lib.links_destroy(t)


# ---- wall terms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y", [2, 3, 70])
@pytest.mark.parametrize("X", [1, 255, 256, 257])
def test_wall_terms(lib, X, Y):
    rng = np.random.default_rng(100 * X + Y)
    u = 0.05 * rng.standard_normal((2, X, Y))
    field = 1e-3 * (1.0 + rng.random(X))
    u_nan = u.copy()
    u_nan[:, :, Y - 1] = np.nan                  # column col_b of the wb == 0 cases: never to be read
    w_s = 3e-3
    cases = [  # (u, col_a, wa, col_b, wb, shift, mode, field?, factor)
        (u, Y - 1, 1.5, Y - 2, -0.5, 0.0, 0, False, 1.0),            # the driver's outlet term
        (u, 0, 1.0, 0, 0.0, w_s, 1, True, 2.0),                      # the driver's inlet term
        (u, Y - 1, 0.75, Y - 1, 0.25, -2e-3, 0, False, -1.5),        # col_a == col_b with wb != 0; negative shift and factor
        (u, 0, 1.5, Y - 1, -0.5, -1e-3, 1, True, -2.0),              # mode 1 through the wb != 0 branch
        (u_nan, 0, 1.0, Y - 1, 0.0, w_s, 0, False, 1.0),             # wb == 0: u[:, :, col_b] is NaN
        (u_nan, 0, 0.5, Y - 1, 0.0, -w_s, 1, True, 2.0),
    ]
    d_field = up(field)
    tail = 37
    for i, (uu, ca, wa, cb, wb, shift, mode, with_field, factor) in enumerate(cases):
        out, d_uu = poisoned(9 * X + tail), up(uu.reshape(-1))
        lib.wall_terms(_ptr(out), _ptr(d_uu), X, Y, ca, ct.c_double(wa), cb, ct.c_double(wb), ct.c_double(shift),
                       mode, _ptr(d_field) if with_field else None, ct.c_double(factor), None)
        got = down_bits(out)
        want = lr.wall_terms(uu, ca, wa, cb, wb, shift, mode, field if with_field else None, factor)
        assert np.isfinite(want).all()
        assert_write_set(got, np.arange(9 * X + tail) < 9 * X, f"case {i}")
        assert_same_bits(got[:9 * X].reshape(X, 9), bits(want), f"case {i}")


# ---- pressure row ------------------------------------------------------------------------------------------------------------
def pressure_lat(R, C, kind):
    return Lat(R, C, pad=40) if kind == "pad" else Lat(R, C, pitch=C + 8)


def pressure_reference(oracle, la, coll, equi, u, src_row, rho_bc, incompressible):
    """[9, C]: (feq(rho_bc, u[src_row]) + coll[src_row]) - equi[src_row]"""
    ur = np.ascontiguousarray(u[:, src_row].T)[None]                  # [1, C, 2]
    feq = (oracle.incomp_equilibrium if incompressible else oracle.equilibrium)(ur, np.full((1, la.C), rho_bc))[0].T
    return (feq + coll[la.off][:, src_row]) - equi[la.off][:, src_row]


@pytest.mark.parametrize("C", [1, 255, 256, 257])
def test_pressure_row_between_blocks(lib, oracle, C):
    Rs, Rd, rho_bc = 3, 5, 1.013
    rng = np.random.default_rng(C)
    u = 0.05 * rng.standard_normal((2, Rs, C))
    d_u = up(u.reshape(-1))
    for dst_kind, src_kind in (("pad", "pitch"), ("pitch", "pad")):
        ld, ls = pressure_lat(Rd, C, dst_kind), pressure_lat(Rs, C, src_kind)
        coll, equi = ls.near_w(1), ls.near_w(2)
        d_coll, d_equi = up(coll), up(equi)
        for incompressible in (0, 1):
            for dst_row, src_row in ((0, Rs - 2), (Rd - 1, 1), (Rd - 1, 0), (0, Rs - 1)):
                what = f"dst {dst_kind} row {dst_row}, src {src_kind} row {src_row}, incompressible {incompressible}"
                dst = poisoned(ld.n)
                lib.pressure_row(_ptr(dst), ct.byref(ld.g), dst_row, _ptr(d_coll), _ptr(d_equi), _ptr(d_u), ct.byref(ls.g),
                                 src_row, ct.c_double(rho_bc), incompressible, None)
                got = down_bits(dst)
                assert_write_set(got, ld.mask([(slice(None), dst_row, slice(None))]), what)
                want = pressure_reference(oracle, ls, coll, equi, u, src_row, rho_bc, incompressible)
                assert_same_bits(got[ld.off][:, dst_row], bits(want), what)


@pytest.mark.parametrize("C", [1, 257])
@pytest.mark.parametrize("kind", ["pad", "pitch"])
def test_pressure_row_on_one_lattice(lib, oracle, C, kind):
    """dst == src with different rows (the single-block Poiseuille use): everything but row dst_row keeps its bits"""
    R, rho_bc = 5, 0.9875
    la = pressure_lat(R, C, kind)
    rng = np.random.default_rng(7 + C)
    u = 0.05 * rng.standard_normal((2, R, C))
    coll, equi = la.near_w(3), la.near_w(4)
    d_equi, d_u = up(equi), up(u.reshape(-1))
    for incompressible in (0, 1):
        for dst_row, src_row in ((0, R - 2), (R - 1, 1)):
            t = up(coll)
            lib.pressure_row(_ptr(t), ct.byref(la.g), dst_row, _ptr(t), _ptr(d_equi), _ptr(d_u), ct.byref(la.g),
                             src_row, ct.c_double(rho_bc), incompressible, None)
            got = down_bits(t)
            row = la.mask([(slice(None), dst_row, slice(None))])
            assert_same_bits(got[~row], bits(coll)[~row], "outside the row")
            want = pressure_reference(oracle, la, coll, equi, u, src_row, rho_bc, incompressible)
            assert_same_bits(got[la.off][:, dst_row], bits(want), f"row {dst_row} from {src_row}")


# ---- momentum source on a row window ------------------------------------------------------------------------------------------
def force_case(lib, la, ranges, ab, seed):
    rng = np.random.default_rng(seed)
    u = 0.05 * rng.standard_normal((2, la.R, la.C))
    p = la.near_w(seed + 1)
    d_u, omega, Fr, Fc = up(u.reshape(-1)), 1.2, 3e-3, -1e-3
    for r0, r1 in ranges:
        t = up(p)
        lib.bgk_add_force_rows(_ptr(t), ct.byref(la.g), _ptr(d_u), ct.c_double(omega), ct.c_double(Fr), ct.c_double(Fc),
                               ct.c_double(ab[0]), ct.c_double(ab[1]), r0, r1, None)
        got = down_bits(t)
        inside = la.mask([(slice(None), slice(r0, r1), slice(None))])
        assert_same_bits(got[~inside], bits(p)[~inside], f"rows [{r0}, {r1}): outside the range")
        want = lr.force_rows(p[la.off], u, omega, Fr, Fc, ab[0], ab[1], r0, r1)
        assert_same_bits(got[la.off], bits(want), f"rows [{r0}, {r1})")
        if r1 > r0:
            assert (got[la.off][:, r0:r1] != bits(p[la.off][:, r0:r1])).any()


@pytest.mark.parametrize("ab", [(3.0, 9.0), (1.0 / 3.0, 1.0 / 9.0)])
@pytest.mark.parametrize("C", [1, 64, 257])
@pytest.mark.parametrize("layout", [dict(), dict(ghost=2, pad=40)])
def test_force_rows(lib, layout, C, ab):
    R = 6
    force_case(lib, Lat(R, C, **layout), [(0, R), (R - 1, R), (2, 4), (3, 3)], ab, seed=C)


def test_force_rows_second_trip_of_the_grid_stride_loop(lib):
    R, C = 8197, 64
    assert R * C > 2048 * 256                    # more nodes than the capped grid has threads
    force_case(lib, Lat(R, C), [(0, R)], (3.0, 9.0), seed=11)


# ---- axpb ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2048 * 256 + 1])
def test_axpb(lib, n):
    x = 0.05 * np.random.default_rng(n).standard_normal(max(n, 1))
    d_x, tail = up(x), 19
    for a, b in ((1.0, 3e-3), (-0.5, 0.0), (0.0, 3.0)):
        out = poisoned(n + tail)
        lib.axpb(_ptr(out), _ptr(d_x), ct.c_double(a), ct.c_double(b), ct.c_longlong(n), None)
        got = down_bits(out)
        assert_write_set(got, np.arange(n + tail) < n, f"a {a}, b {b}")
        assert_same_bits(got[:n], bits(a * x[:n] + b), f"a {a}, b {b}")
