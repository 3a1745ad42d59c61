"""The yardstick of the edge-mode tests (tests/test_edge_reference.py, tests/test_gpu_edge_modes.py): one driver iteration
of the reference -- collide, solver::advect, the driver's post-advect boundary assignments -- restated in numpy on the
reference layout f[R, C, 9], for ANY supported mode on each of the four edges.

It shares nothing with the library under test: no table, no index helper, no gather.  The data movement is written the
way the reference drivers write it -- a periodic advect of the whole lattice (np.roll per population), then whole-edge
slice assignments that read the post-collision populations -- and every rule is the sentence of include/lbm_hip.h
(`enum lbm_edge_mode`, `struct lbm_bc`) it restates, with the driver lines that sentence cites:

  PERIODIC       nothing: the advect's own wrap                                        (solver.cpp:84-128)
  BOUNCE_BACK    halfway bounce-back: a population that cannot arrive from inside the domain is the node's own
                 post-collision population of the opposite direction
                 (columns: horizontal_poiseuille_test.cpp:146-152, rows: mrtcg_rayleigh_taylor.cpp:525-531)
  SPECULAR       columns: ... is the node's own post-collision population mirrored at the wall (c_y -> -c_y)
                                                                                        (cylinder_test.cpp:157-163)
  ABB_VELOCITY   rows: ALL EIGHT moving populations of the row are replaced,
                 f[opp(q)] = -f_coll[q] + (2 + 9 (c_q.u_w)^2 - 3 u_w.u_w) w_q          (cylinder_test.cpp:135-154)
  WRAP_NOSHIFT   columns, rows 1..R-2 only: ... is the post-collision population of the same direction in the
                 OPPOSITE column of the SAME row                                        (mrtcg_rayleigh_taylor.cpp:517-523)

Rows are applied first, then columns, so a column wins the populations both claim at a corner (cylinder_test.cpp applies
its inlet / outlet rows before its side walls).  "Cannot arrive from inside" is geometry, not a table: population q moves
by (c_x[q], c_y[q]) in (row, column), so row 0 cannot receive c_x = +1, row R-1 c_x = -1, column 0 c_y = +1 and column
C-1 c_y = -1.

The collision is composed from the oracle's operators (oracle/pyoracle.py), which evaluate the reference's expressions in
the reference's order; element-wise numpy f64 operations do not fuse, so the forms written out here keep their order too.
The module imports neither torch nor the library."""
from collections import namedtuple

import numpy as np

# enum lbm_edge_mode (include/lbm_hip.h); HALO (1) belongs to slabs and is not an edge of a single block
PERIODIC, BOUNCE_BACK, SPECULAR, ABB_VELOCITY, WRAP_NOSHIFT = 0, 2, 3, 4, 5
ROW_MODES = (PERIODIC, BOUNCE_BACK, ABB_VELOCITY)
COL_MODES = (PERIODIC, BOUNCE_BACK, SPECULAR, WRAP_NOSHIFT)
MODE_NAME = {PERIODIC: "per", BOUNCE_BACK: "bb", SPECULAR: "spec", ABB_VELOCITY: "abb", WRAP_NOSHIFT: "wrap"}

# the velocity set and the weights: solver::c rows 0 / 1 and solver::E (src/solver.cpp:12-21); c_x pairs with the row index
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
E = np.array([4.0 / 9.0] + [1.0 / 9.0] * 4 + [1.0 / 36.0] * 4)


def _direction(cx, cy):
    return int(np.flatnonzero((CX == cx) & (CY == cy))[0])


OPP = [_direction(-CX[q], -CY[q]) for q in range(9)]       # the opposite direction
MIRROR_COL = [_direction(CX[q], -CY[q]) for q in range(9)]  # mirrored at a wall that runs along a column

Edges = namedtuple("Edges", "row_lo row_hi col_lo col_hi uw")
Edges.__new__.__defaults__ = (PERIODIC, PERIODIC, PERIODIC, PERIODIC, (0.0, 0.0))
Edges.__doc__ = "struct lbm_bc without the pressure rows: the mode of each edge and the wall velocity (uw_r, uw_c)"


def edges_name(e):
    return "rows %s/%s cols %s/%s" % tuple(MODE_NAME[m] for m in e[:4])


def all_edges(row_modes=ROW_MODES, col_modes=COL_MODES, uw=(0.04, 0.01)):
    """every (row_lo, row_hi) x (col_lo, col_hi) of the given modes: 3^2 x 4^2 = 144 by default"""
    return [Edges(a, b, c, d, uw) for a in row_modes for b in row_modes for c in col_modes for d in col_modes]


def unmixed_wall_edges(uw=(0.04, 0.01)):
    """what the multi-step windows carry: per axis PERIODIC / PERIODIC or a wall on both edges; all-periodic left out (24)"""
    rows = [(PERIODIC, PERIODIC)] + [(a, b) for a in (BOUNCE_BACK, ABB_VELOCITY) for b in (BOUNCE_BACK, ABB_VELOCITY)]
    cols = [(PERIODIC, PERIODIC)] + [(a, b) for a in (BOUNCE_BACK, SPECULAR) for b in (BOUNCE_BACK, SPECULAR)]
    return [Edges(r[0], r[1], c[0], c[1], uw) for r in rows for c in cols if r[0] != PERIODIC or c[0] != PERIODIC]


# ---- data movement ----------------------------------------------------------------------------------------------------------
def advect(fc):
    """solver::advect: g[r, c, q] = f[r - c_x[q], c - c_y[q], q], periodic in both directions"""
    f = np.empty_like(fc)
    for q in range(9):
        f[..., q] = np.roll(fc[..., q], (CX[q], CY[q]), axis=(0, 1))
    return f


def abb_term(uw):
    """(2 + 9 (c_q.u_w)^2 - 3 u_w.u_w) w_q per direction, in the order cylinder_test.cpp:135 evaluates it"""
    uw_r, uw_c = float(uw[0]), float(uw[1])
    uu = uw_r * uw_r + uw_c * uw_c
    cu = uw_r * CX.astype(np.float64) + uw_c * CY.astype(np.float64)
    return ((2.0 + 9.0 * (cu * cu)) - 3.0 * uu) * E


def apply_edges(f, fc, e):
    """the post-advect assignments of one iteration, in place on the advected f; fc: the post-collision lattice"""
    R, C = f.shape[:2]
    abb = abb_term(e.uw)
    # rows first
    for row, mode, arriving_cx in ((0, e.row_lo, 1), (R - 1, e.row_hi, -1)):
        if mode == BOUNCE_BACK:
            for q in np.flatnonzero(CX == arriving_cx):
                f[row, :, q] = fc[row, :, OPP[q]]
        elif mode == ABB_VELOCITY:
            for q in range(1, 9):
                f[row, :, OPP[q]] = -fc[row, :, q] + abb[q]
        else:
            assert mode == PERIODIC, f"row mode {mode}"
    # then columns: they win at the corners
    for col, other, mode, arriving_cy in ((C - 1, 0, e.col_hi, -1), (0, C - 1, e.col_lo, 1)):
        missing = np.flatnonzero(CY == arriving_cy)
        if mode == BOUNCE_BACK:
            for q in missing:
                f[:, col, q] = fc[:, col, OPP[q]]
        elif mode == SPECULAR:
            for q in missing:
                f[:, col, q] = fc[:, col, MIRROR_COL[q]]
        elif mode == WRAP_NOSHIFT:
            for q in missing:
                f[1:R - 1, col, q] = fc[1:R - 1, other, q]
        else:
            assert mode == PERIODIC, f"column mode {mode}"
    return f


def stream(fc, e):
    """f_adve of the reference: advect + the driver's boundary assignments"""
    return apply_edges(advect(fc), fc, e)


# ---- collision ----------------------------------------------------------------------------------------------------------------
Bgk = namedtuple("Bgk", "omega incompressible delta_form")
Bgk.__new__.__defaults__ = (0, 0)
Kbc = namedtuple("Kbc", "s2")


def moments(orc, f, model):
    """what the driver's calc_rho / calc_u (calc_incomp_u) hold for the lattice f"""
    rho = orc.calc_rho(f)
    if isinstance(model, Bgk) and model.incompressible:
        return rho, orc.calc_incomp_u(f)
    return rho, orc.calc_u(f, rho)


def collide(orc, f, model, pressure=None):
    """the node-local half of one driver iteration: the post-collision lattice of the pre-collision f.  pressure =
    (rho_inlet, rho_outlet): the pressure-periodic virtual rows of horizontal_poiseuille_test.cpp:25-45 on top (BGK)"""
    rho, u = moments(orc, f, model)
    if isinstance(model, Kbc):   # ulbm_double_shear_flow.cpp:141-143: the moments recomputed from the populations, kbc::collide
        assert pressure is None
        return orc.kbc_collide(f, rho, u, model.s2)[0]
    equilibrium = orc.incomp_equilibrium if model.incompressible else orc.equilibrium
    feq = equilibrium(u, rho)
    if model.delta_form:         # cylinder_test.cpp:108, :123-125
        fc = f + (-model.omega * (f - feq))
    else:
        fc = orc.collision(f, feq, model.omega)   # solver.cpp:73
    if pressure is not None:     # virtual inlet row 0 from the outlet row R-2, virtual outlet row R-1 from the inlet row 1
        R, C = rho.shape
        rows = {}
        for dst, src, rho_bc in ((0, R - 2, pressure[0]), (R - 1, 1, pressure[1])):
            te = equilibrium(u[src:src + 1], rho_bc * np.ones((1, C)))
            rows[dst] = (te[0] + fc[src]) - feq[src]
        for dst, row in rows.items():
            fc[dst] = row
    return fc


def run(orc, f, n, e, model, pressure=None):
    """n >= 1 driver iterations from the pre-collision lattice f.  Returns
      coll   the post-collision lattice of iteration n (what the engine keeps resident),
      f      the streamed state after iteration n (f_adve),
      rho, u the moments of that streamed state (what the drivers' tensors hold at the top of iteration n + 1)."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    assert n >= 1
    for _ in range(n):
        fc = collide(orc, f, model, pressure)
        f = stream(fc, e)
    rho, u = moments(orc, f, model)
    return dict(coll=fc, f=f, rho=rho, u=u)


def mass(f):
    """sum of every population of the lattice, accumulated in extended precision on the host"""
    return np.sum(np.asarray(f, dtype=np.longdouble))


def relative_mass_drift(f_end, f_start):
    m0 = mass(f_start)
    return float(abs(mass(f_end) - m0) / m0)


# ---- the state recipe of the GPU suites -------------------------------------------------------------------------------------
def noisy_state(orc, R, C, seed):
    """equilibrium of rho = 1 + 0.01 N, u = 0.03 N, times (1 + 0.01 N)"""
    rng = np.random.default_rng(seed)
    rho = 1 + 0.01 * rng.standard_normal((R, C))
    u = 0.03 * rng.standard_normal((R, C, 2))
    return orc.equilibrium(u, rho) * (1 + 0.01 * rng.standard_normal((R, C, 9)))
