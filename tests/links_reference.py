"""The yardstick of tests/test_gpu_links.py: part 8 of the C ABI (csrc/capi_links.hip) restated in plain numpy -- the slice
assignments a link table stands for, the wall terms and the momentum source on a row window, each in the expression order
of the comments in include/lbm_hip.h (numpy's element-wise f64 operations do not fuse, the library is built with
-ffp-contract=off, so the comparison is bitwise).  It never imports the library under test or the oracle.

A slice is a tuple with the fields of lbm_links_add_affine,

    (dst_lat, q_dst, r0, c0, dr, dc, src_lat, q_src, sr0, sc0, sdr, sdc, count[, scale, add0, add_stride])

-- the 13-field form is lbm_links_add: scale 1, no addend (add0 < 0).  Lattices are numpy arrays [9, R, C] of the owned rows,
CX along rows."""
import numpy as np

W9 = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])   # tests/ade_util.py
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])


def full(s):
    """a slice in the 16-field form"""
    s = tuple(s)
    assert len(s) in (13, 16), s
    return s + (1.0, -1, 0) if len(s) == 13 else s


def elements(s):
    """(k, destination (q, r, c), source (q, r, c), addend index or -1) of every link of a slice"""
    dl, qd, r0, c0, dr, dc, sl, qs, sr0, sc0, sdr, sdc, count, scale, add0, stride = full(s)
    for k in range(count):
        yield k, (qd, r0 + k * dr, c0 + k * dc), (qs, sr0 + k * sdr, sc0 + k * sdc), (add0 + k * stride if add0 >= 0 else -1)


def link_map(slices):
    """what the table holds after the slices: {(dst_lat, q, r, c): (src_lat, (q, r, c), scale, addend index)} -- the later
    slice wins an element whole"""
    m = {}
    for s in slices:
        s = full(s)
        for _, d, e, ai in elements(s):
            m[(s[0],) + d] = (s[6], e, s[13], ai)
    return m


def _inside(a, e):
    return all(0 <= i < n for i, n in zip(e, a.shape))


def apply_slices(slices, dst, src, addends=None):
    """the slice assignments, one after the other in list order, as the reference drivers execute them:

        dst[dl][qd, r0 + k dr, c0 + k dc] = scale * src[sl][qs, sr0 + k sdr, sc0 + k sdc] (+ addends[add0 + k add_stride])

    Where dst[i] is src[j] (in place) every read sees the value from before the call -- the one-launch gather.  A list in
    which one slice reads an element of such a shared array that a slice writes is order-dependent on a device and not
    modelled here: ValueError."""
    slices = [full(s) for s in slices]
    for i, d in enumerate(dst):
        for j, s in enumerate(src):
            if d is not s:
                continue
            written = {e for sl in slices if sl[0] == i for _, e, _, _ in elements(sl)}
            read = {e for sl in slices if sl[6] == j for _, _, e, _ in elements(sl)}
            if written & read:
                raise ValueError(f"in-place chain: dst[{i}] is src[{j}] and element {sorted(written & read)[0]} is both written and read")
    before = [s.copy() if any(s is d for d in dst) else s for s in src]
    for s in slices:
        scale = s[13]
        for _, d, e, ai in elements(s):
            if not (_inside(dst[s[0]], d) and _inside(before[s[6]], e)):
                raise IndexError(f"slice {s} leaves the lattice at {d} <- {e}")
            v = before[s[6]][e]
            if scale != 1.0 or ai >= 0:
                v = np.float64(scale) * v
            if ai >= 0:
                v = v + addends[ai]
            dst[s[0]][d] = v
    return dst


def wall_terms(u, col_a, wa, col_b, wb, shift, mode, field, factor):
    """out [X, 9] from the moment field u [2, X, Y]: uw = wa u[:, :, col_a] + wb u[:, :, col_b] + shift (the second term
    is not formed, u[:, :, col_b] not read, when wb == 0);
    mode 0: factor ((2 + 9 (uw.c_q)^2) - 3 uw.uw) w_q;  mode 1: factor ((((1 + 3 uw.c_q) + 4.5 (uw.c_q)^2) - 1.5 uw.uw) w_q) field[r]
    (the library writes wa ua - (-wb) ub: in IEEE arithmetic the same bits as wa ua + wb ub)"""
    u = np.asarray(u, dtype=np.float64)
    if wb != 0.0:
        w0 = wa * u[0, :, col_a] + wb * u[0, :, col_b]
        w1 = wa * u[1, :, col_a] + wb * u[1, :, col_b]
    else:
        w0 = wa * u[0, :, col_a]
        w1 = wa * u[1, :, col_a]
    w0 = w0 + shift
    w1 = w1 + shift
    uu = w0 * w0 + w1 * w1
    out = np.empty((u.shape[1], 9))
    for q in range(9):
        uc = w0 * float(CX[q]) + w1 * float(CY[q])
        if mode == 0:
            t = ((2.0 + 9.0 * (uc * uc)) - 3.0 * uu) * W9[q]
        else:
            t = ((((1.0 + 3.0 * uc) + 4.5 * (uc * uc)) - 1.5 * uu) * W9[q]) * field
        out[:, q] = factor * t
    return out


def force_rows(p, u, omega, Fr, Fc, a, b, r0, r1):
    """a copy of p [9, R, C] with p_q + (((1 - 0.5 omega) * ((a + b cu) cF - a uF)) * w_q) on rows [r0, r1); u [2, R, C]"""
    p = np.array(p, dtype=np.float64)
    ux, uy = u[0, r0:r1], u[1, r0:r1]
    uF = ux * Fr + uy * Fc
    for q in range(9):
        cu = ux * float(CX[q]) + uy * float(CY[q])
        cF = Fr * float(CX[q]) + Fc * float(CY[q])
        p[q, r0:r1] = p[q, r0:r1] + (((1 - 0.5 * omega) * ((a + b * cu) * cF - a * uF)) * W9[q])
    return p


# ---- a periodic box cut into blocks: the slice list that glues them after each block streamed alone ----------------------
def split(a, row_sizes, col_sizes):
    """[9, R, C] -> blocks [9, Rb, Cb] (copies), block (bi, bj) at index bi * len(col_sizes) + bj"""
    r = np.concatenate(([0], np.cumsum(row_sizes)))
    c = np.concatenate(([0], np.cumsum(col_sizes)))
    return [a[:, r[i]:r[i + 1], c[j]:c[j + 1]].copy() for i in range(len(row_sizes)) for j in range(len(col_sizes))]


def join(blocks, row_sizes, col_sizes):
    n = len(col_sizes)
    return np.concatenate([np.concatenate(blocks[i * n:(i + 1) * n], axis=2) for i in range(len(row_sizes))], axis=1)


def advect_alone(a):
    """periodic streaming of one lattice [9, R, C] onto itself: new[q][r][c] = old[q][r - cx][c - cy]"""
    return np.stack([np.roll(a[q], (CX[q], CY[q]), axis=(0, 1)) for q in range(9)])


def _rolled(dl, q, sl, r, sr, n, shift, along_row):
    """the full edge line of n elements, destination index i <- source index (i - shift) mod n, as linear slices (the
    wrapped element is a slice of its own); along_row: the line is row r (source row sr), else column r (source column sr)"""
    def one(i0, s0, count):
        if along_row:
            return (dl, q, r, i0, 0, 1, sl, q, sr, s0, 0, 1, count)
        return (dl, q, i0, r, 1, 0, sl, q, s0, sr, 1, 0, count)
    if shift == 0:
        return [one(0, 0, n)]
    if shift > 0:
        return [one(1, 0, n - 1), one(0, n - 1, 1)]
    return [one(0, 1, n - 1), one(n - 1, 0, 1)]


def split_slices(row_sizes, col_sizes, corners=True):
    """the repair of the edge populations of every block of a periodic box after each block streamed alone (wrapping onto
    itself): destination = the streamed lattices, source = the lattices before streaming, lattice index as in split().
    In the order a driver would write them -- full-length row slices from the row neighbour (wrong in one corner element
    for the diagonal populations), then full-length column slices from the column neighbour (wrong in that element too),
    then the single corner elements from the diagonal neighbour: only the last write of a corner is right."""
    nr, nc = len(row_sizes), len(col_sizes)
    rows, cols, corner = [], [], []
    for bi in range(nr):
        for bj in range(nc):
            me, R, C = bi * nc + bj, row_sizes[bi], col_sizes[bj]
            for q in range(1, 9):
                cx, cy = int(CX[q]), int(CY[q])
                ni, nj = (bi - cx) % nr, (bj - cy) % nc
                r_e, sr = (0, row_sizes[ni] - 1) if cx > 0 else (R - 1, 0)
                c_e, sc = (0, col_sizes[nj] - 1) if cy > 0 else (C - 1, 0)
                if cx:
                    rows += _rolled(me, q, ni * nc + bj, r_e, sr, C, cy, True)
                if cy:
                    cols += _rolled(me, q, bi * nc + nj, c_e, sc, R, cx, False)
                if cx and cy and corners:
                    corner.append((me, q, r_e, c_e, 0, 0, ni * nc + nj, q, sr, sc, 0, 0, 1))
    return rows + cols + corner
