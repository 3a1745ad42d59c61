"""Shared by the immersed-boundary tests: the cylinder preset, the marker sets of tests/test_gpu_ibm_markers.py, the
host-side picture of the tables lbm_ibm_create_slab builds (floor-based 4 x 4 boxes, touched nodes, pairs per node,
Peskin tap weights) and a numpy restatement of the driver's source term.  numpy and pylbm only: importable without
a device."""
import numpy as np

import pylbm

# D2Q9 in the library's order (d2q9.hpp)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1], dtype=np.float64)
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1], dtype=np.float64)
WQ = np.array([4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4)

IBM_STEP_KEYS = ("ibm_step_opt", "ibm_step_split", "ibm_step_chain")
LDS_LIMIT = 150 * 1024     # lbm_ibm_step: dynamic LDS of the one-workgroup kernel, (3 n_touched + 2 n_markers) doubles


def circle(cx, cy, radius, spacing=1.0, n=None):
    """n markers evenly spaced on a circle, sorted by angle (n: round(circumference / spacing) unless given)"""
    if n is None:
        n = int(round(2 * np.pi * radius / spacing))
    t = 2 * np.pi * np.arange(n) / n
    return cx + radius * np.cos(t), cy + radius * np.sin(t)


def cylinder_bc(u_in):
    bc = pylbm.Bc.periodic()
    bc.row_lo = bc.row_hi = pylbm.EDGE_ABB_VELOCITY      # cylinder_test.cpp:135-154
    bc.col_lo = bc.col_hi = pylbm.EDGE_SPECULAR          # :157-163
    bc.uw_r, bc.uw_c = u_in, 0.0
    return bc


def cylinder_solver(lib, X, Y, omega, u_in, x, y, form=pylbm.FORM_REFERENCE_ORDER, m_max=5):
    """the cylinder preset; the parity tests hold it to the oracle BITWISE, i.e. in the reference's operation order
    (the library's default is the reassociated collision: test_cylinder_with_the_default_collision and
    tests/test_gpu_ibm_default.py)"""
    sv = pylbm.Solver(lib, pylbm.MODEL_BGK, X, Y, pylbm.BgkParams(omega, 0, 1, form=form), bc=cylinder_bc(u_in))
    ib = pylbm.Ibm(lib, x, y, X, Y, m_max=m_max)
    sv.attach_ibm(ib)
    return sv, ib


def source_term(u, F, omega, a, b):
    """cylinder_test.cpp:116-127 as k_ibm_add_source writes it, left to right:
    S_q = ((1 - 0.5 omega) ((a + b c_q.u)(c_q.F) - a (u.F))) w_q;  u, F: [..., 2] -> [..., 9]"""
    ux, uy, Fx, Fy = u[..., 0, None], u[..., 1, None], F[..., 0, None], F[..., 1, None]
    uF = ux * Fx + uy * Fy
    cu = ux * CX + uy * CY
    cF = Fx * CX + Fy * CY
    return ((1 - 0.5 * omega) * ((a + b * cu) * cF - a * uF) * WQ)


def add_source(p, roi, u, F, omega, a, b):
    """p [X, Y, 9] + S(u, F) on the ROI only (u: the full field [X, Y, 2], F: [RR, RC, 2])"""
    r0, r1, c0, c1 = roi
    out = p.copy()
    out[r0:r1, c0:c1] += source_term(u[r0:r1, c0:c1], F, omega, a, b)
    return out


# ---- the host-side picture of the boundary's tables ---------------------------------------------------------------------
def roi_of(x, y):
    """ibm.cpp:124-153: rows [r0, r1) x columns [c0, c1)"""
    fx, fy = np.floor(x).astype(int), np.floor(y).astype(int)
    return int(fx.min()) - 2, int(fx.max()) + 3, int(fy.min()) - 2, int(fy.max()) + 3


def pairs_per_node(x, y):
    """[RR, RC] number of (marker, tap) pairs of every ROI node: marker j touches rows floor(x_j) - 1 .. + 2 and
    columns floor(y_j) - 1 .. + 2"""
    r0, r1, c0, c1 = roi_of(x, y)
    cnt = np.zeros((r1 - r0, c1 - c0), dtype=int)
    for fx, fy in zip(np.floor(x).astype(int), np.floor(y).astype(int)):
        cnt[fx - 1 - r0:fx + 3 - r0, fy - 1 - c0:fy + 3 - c0] += 1
    return cnt


def n_touched(x, y):
    return int((pairs_per_node(x, y) > 0).sum())


def lds_bytes(x, y):
    return (3 * n_touched(x, y) + 2 * len(x)) * 8


def takes_one_workgroup(x, y):
    """lbm_ibm_step's rule: the one-workgroup kernel unless the boundary is too large for it"""
    return n_touched(x, y) <= 8 * 1024 and lds_bytes(x, y) <= LDS_LIMIT


def own_of(x, y):
    """touched nodes per thread of the k_ibm_step instantiation lbm_ibm_step picks"""
    nt = n_touched(x, y)
    return 4 if nt <= 4096 else (6 if nt <= 6144 else 8)


def peskin4(r):
    r = np.abs(np.asarray(r, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        inner = 0.125 * (3.0 - 2.0 * r + np.sqrt(1.0 + 4.0 * r - 4.0 * r * r))
        outer = 0.125 * (5.0 - 2.0 * r - np.sqrt(-7.0 + 12.0 * r - 4.0 * r * r))
    return np.where(r <= 1, inner, np.where(r <= 2, outer, 0.0))


def tap_weights(x, y):
    """[n, 16] the 16 tap weights of every marker (k = 4 i + j; the kernel of x runs along j: SURVEY Q9)"""
    r0, _, c0, _ = roi_of(x, y)
    xr, yr = np.asarray(x, dtype=np.float64) - float(r0), np.asarray(y, dtype=np.float64) - float(c0)
    k = np.arange(16)
    sx = xr[:, None] - ((k % 4).astype(np.float64) + np.floor(xr)[:, None] - 1.0)
    sy = yr[:, None] - ((k // 4).astype(np.float64) + np.floor(yr)[:, None] - 1.0)
    return peskin4(sx) * peskin4(sy)


# ---- the marker sets: each the smallest that reaches its edge (asserted in test_gpu_ibm_markers.py) ------------------
def one_marker():
    return np.array([7.3]), np.array([6.8])


def branch_points():
    """markers on integer and half-integer coordinates and one ulp-scale step below an integer: the branches of the
    Peskin kernel meet at r = 0, 1, 2"""
    e = 2.0 ** -40
    x = np.array([6.0, 9.0, 7.5, 10.5, 8.0 - e, 11.0, 12.0 - e, 8.0])
    y = np.array([7.0, 6.5, 9.5, 6.0, 8.0, 9.0 - e, 12.0 - e, 10.0])
    return x, y


def crowded(k, seed=11):
    """k markers inside the cell [7, 8) x [6, 7); from k = 2 on the second equals the first, and with k = 67 every
    tenth repeats its predecessor"""
    rng = np.random.default_rng(seed + k)
    x, y = 7.0 + rng.random(k), 6.0 + rng.random(k)
    if k >= 2:
        x[1], y[1] = x[0], y[0]
    for j in range(10, k, 10):
        x[j], y[j] = x[j - 1], y[j - 1]
    return x, y


def shuffled_circle(seed=5):
    x, y = circle(13.3, 13.6, 8.0)
    perm = np.random.default_rng(seed).permutation(len(x))
    return x[perm], y[perm], perm


def counted_circle(n):
    return circle(15.3, 15.6, 10.0, n=n)


def disjoint_grid(n, per_row=20):
    """n markers on a grid 4 apart, row-major: the 4 x 4 boxes do not overlap, every marker touches 16 nodes of its own"""
    j = np.arange(n)
    return 4.0 * (j // per_row) + 5.3, 4.0 * (j % per_row) + 5.6


def tight_fit():
    """(x, y, X, Y): the ROI leaves exactly one node on each of the four sides of an X x Y lattice"""
    x, y = np.array([3.2, 8.9, 5.5]), np.array([3.7, 9.4, 6.1])
    return x, y, 12, 13


def lattice_around(x, y, margin=3):
    """the ROI plus a margin of a few nodes"""
    r0, r1, c0, c1 = roi_of(x, y)
    assert r0 >= 1 and c0 >= 1
    return r1 + margin, c1 + margin


def random_fields(X, Y, seed):
    """u [X, Y, 2] with |u| <= 0.25 in a random direction, rho [X, Y] in 0.2 .. 5, p [X, Y, 9] ordinary numbers"""
    rng = np.random.default_rng(seed)
    mag, ang = 0.25 * rng.random((X, Y)), 2 * np.pi * rng.random((X, Y))
    u = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=-1)
    rho = 0.2 + 4.8 * rng.random((X, Y))
    p = rng.standard_normal((X, Y, 9))
    return u, rho, p


# ---- the block schedule of lbm_solver_step with an immersed boundary --------------------------------------------------
def block_qualifies(R, C, roi, D):
    """solver_ibm_block's bounds (the forced band; the box inside it changes no count)"""
    q0, q1, _, _ = roi
    return D >= 2 and q0 - 2 * D >= 2 and q1 + 2 * D <= R - 2 and R >= 4 * D + 8 and C >= 64


def takes_the_box(C, roi, D):
    """the forced box of a qualifying block, else the full-width band"""
    _, _, c0, c1 = roi
    bc1 = (c1 + 2 * D + 7) // 8 * 8
    return c0 - 2 * D >= 8 and bc1 <= C - 1


def expected_blocks(R, C, roi, n, max_depth=5):
    """blocks lbm_solver_step launches in ONE call of n steps from a pre-collision state, no moments recorded: the first
    step runs singly, then the deepest block that fits the steps left, the lattice and the bounds, else a single step"""
    blocks, i = 0, 1
    while i < n:
        depth = min(n - i, max_depth)
        while depth >= 2 and R < 4 * depth + 8:
            depth -= 1
        if depth >= 2 and block_qualifies(R, C, roi, depth):
            blocks, i = blocks + 1, i + depth
        else:
            i += 1
    return blocks
