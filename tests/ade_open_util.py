"""Yardstick of the open boundaries of the fluid + scalar step (lbm_ade_open; tests/test_gpu_ade_open.py): the driver's
iteration with its open edges as SEQUENTIAL INDEX ASSIGNMENTS in numpy, on the oracle's solver:: primitives -- the
zero-gradient copies written into g_coll before advect (test/rectangle_sedimentation_test.cpp:138-141), advect, the domain's
walls, the f assignments in the order given (:150-182) with the outlet's u_w from the u at the start of the iteration (:163),
calc_rho / calc_u, the domain's FIXED rows, the g assignments in the order given (:203-218), an optional body
(tests/ade_util.py).  There is no source map and no per-slot table here: later assignments simply overwrite earlier ones,
as in the driver.  One list of segments (`Segments`) feeds both this loop and the pylbm.AdeOpenBoundary under test.  The
loop never calls the library under test."""
import numpy as np

import ade_util as ade
import pylbm

BB_RULE, SPEC_ROW, SPEC_COL, ABB, ABB_X = (pylbm.ADE_OPEN_BOUNCE_BACK, pylbm.ADE_OPEN_SPECULAR_ROW,
                                           pylbm.ADE_OPEN_SPECULAR_COL, pylbm.ADE_OPEN_ABB, pylbm.ADE_OPEN_ABB_EXTRAPOLATED)
NO_FLUX, FIXED = pylbm.ADE_SCALAR_NO_FLUX, pylbm.ADE_SCALAR_FIXED
ALL = 0xFF
FLIP_ROW = [0, 3, 2, 1, 4, 6, 5, 8, 7]  # slot with c_x (rows) negated
FLIP_COL = [0, 1, 4, 3, 2, 8, 7, 6, 5]  # slot with c_y negated


def mask(*slots):
    return sum(1 << (s - 1) for s in slots)


class Segments:
    """the segments of an open table in the order added; each (kind, r0, c0, dr, dc, n, ...) with r0, c0 >= 0"""

    def __init__(self, R, C):
        self.R, self.C, self.items = R, C, []

    def f(self, r0, c0, dr, dc, n, slots, rule, p=(0.0, 0.0), neighbour=(0, 0)):
        self.items.append(("f", r0 % self.R, c0 % self.C, dr, dc, n, slots, rule, p, neighbour))
        return self

    def g(self, r0, c0, dr, dc, n, slots, mode=NO_FLUX, conc=0.0):
        self.items.append(("g", r0 % self.R, c0 % self.C, dr, dc, n, slots, mode, conc))
        return self

    def copy(self, r0, c0, dr, dc, n, source):
        self.items.append(("copy", r0 % self.R, c0 % self.C, dr, dc, n, source))
        return self

    def reversed_rules(self):
        """the same segments with the f rules among themselves and the g rules among themselves in the opposite order"""
        out = Segments(self.R, self.C)
        rules = [it for it in self.items if it[0] != "copy"]
        out.items = [it for it in self.items if it[0] == "copy"] + rules[::-1]
        return out

    def table(self, lib):
        t = pylbm.AdeOpenBoundary(lib, self.R, self.C)
        for it in self.items:
            if it[0] == "f":
                t.add_f(*it[1:8], it[8], it[9])
            elif it[0] == "g":
                t.add_g(*it[1:9])
            else:
                t.add_g_copy(*it[1:7])
        return t.finalize()


def channel(R, C, u_in, conc_w=1e-3, conc_rows=50):
    """the sedimentation driver's open edges, assignment by assignment (:138-141, :150-182, :203-218); the bottom row's
    own assignments (:180-182, :234-236) are the domain's BOUNCE_BACK row_hi, but for the corner the outlet takes first"""
    s = Segments(R, C)
    s.copy(0, 0, 0, 1, C, (1, 0))
    s.copy(1, C - 1, 1, 0, R - 2, (0, -1))
    s.f(1, 0, 1, 0, R - 2, ALL, ABB, (0.0, u_in))
    s.f(0, C - 1, 1, 0, R, ALL, ABB_X, (1.5, -0.5), (0, -1))
    s.f(0, 0, 0, 1, C, mask(8, 1, 5), SPEC_ROW)
    s.f(R - 1, C - 1, 0, 1, 1, mask(7, 3, 6), BB_RULE)
    s.g(1, 0, 1, 0, R - 2, ALL, FIXED, 0.0)
    first = max(R - conc_rows, 1)
    if first <= R - 2:
        s.g(first, 0, 1, 0, R - 1 - first, ALL, FIXED, conc_w)
    return s


def build_open(lib, kind, R, C):
    """the global open tables of the slab suite by name (tests/test_gpu_ade_open_slabs.py and, from cfg["table"], its rank
    processes tests/ade_ring_rank.py): 'channel' -- lbm_ade_open_add_channel; 'columns' -- an ABB inlet with a FIXED scalar
    on column 0 and an extrapolated outlet with its zero-gradient copy on column C-1, ALL rows: an open node on the first
    and last row of every slab, whatever the seams"""
    t = pylbm.AdeOpenBoundary(lib, R, C)
    if kind == "channel":
        return t.channel(0.03, 1e-3, max(2, R // 4))
    assert kind == "columns", kind
    t.add_f(0, 0, 1, 0, R, ALL, ABB, (2e-3, 0.03))
    t.add_f(0, C - 1, 1, 0, R, ALL, ABB_X, (1.5, -0.5), (0, -1))
    t.add_g(0, 0, 1, 0, R, ALL, FIXED, 1e-3)
    t.add_g_copy(0, C - 1, 1, 0, R, (0, -1))
    return t


def _idx(it):
    k = np.arange(it[5])
    return it[1] + k * it[3], it[2] + k * it[4]


def calc_u(orc, f):
    return orc.calc_u(f, orc.calc_rho(f))


def stream(orc, segs, bc, fixed, fc, gc, u_prev, w, body=None):
    """one iteration after the collisions: (f_adve, g_adve) from the post-collision pair and the u at its start.  fixed:
    {row edge: C_w array} of the domain's FIXED rows (columns are not restated here)"""
    assert all(k in ("row_lo", "row_hi") for k in fixed)
    R, C = fc.shape[:2]
    gc = gc.copy()
    for it in segs.items:                                                # the copies, into g_coll (:138-141)
        if it[0] == "copy":
            rr, cc = _idx(it)
            gc[rr, cc] = gc[rr + it[6][0], cc + it[6][1]]                # (fancy indexing reads before it writes)
    f, g = orc.advect(fc), orc.advect(gc)
    ade.fix_up(orc, bc, {}, f, fc, g, gc, w)                             # the domain's walls, g no-flux
    for it in segs.items:                                                # the f assignments (:150-182)
        if it[0] != "f":
            continue
        rr, cc = _idx(it)
        rule, p, nb = it[7], it[8], it[9]
        for s in ade.slots_of(it[6]):
            q = ade.OPP[s]
            if rule == BB_RULE:
                f[rr, cc, s] = fc[rr, cc, q]
            elif rule == SPEC_ROW:
                f[rr, cc, s] = fc[rr, cc, FLIP_ROW[s]]
            elif rule == SPEC_COL:
                f[rr, cc, s] = fc[rr, cc, FLIP_COL[s]]
            else:
                if rule == ABB:
                    uw0, uw1 = np.float64(p[0]), np.float64(p[1])
                else:
                    uw = p[0] * u_prev[rr, cc] + p[1] * u_prev[rr + nb[0], cc + nb[1]]
                    uw0, uw1 = uw[:, 0], uw[:, 1]
                uu = uw0 * uw0 + uw1 * uw1
                uc = uw0 * float(ade.CX[q]) + uw1 * float(ade.CY[q])
                f[rr, cc, s] = -fc[rr, cc, q] + ((2.0 + 9.0 * (uc * uc)) - 3.0 * uu) * ade.E9[q]
    if body is not None:
        for idx, m in body.f_segments:
            for s in ade.slots_of(m):
                f[idx + (s,)] = fc[idx + (ade.OPP[s],)]
    v = calc_u(orc, f) + np.asarray(w)                                   # :198-200

    def abb(rr, cc, s, cw):
        q = ade.OPP[s]
        vr, vc = v[rr, cc, 0], v[rr, cc, 1]
        cv = vr * float(ade.CX[q]) + vc * float(ade.CY[q])
        vv = vr * vr + vc * vc
        return -gc[rr, cc, q] + 2.0 * ((((1.0 + 3.0 * cv) + 4.5 * (cv * cv)) - 1.5 * vv) * ade.E9[q] * cw)

    for name, r in (("row_lo", 0), ("row_hi", R - 1)):                   # the domain's FIXED rows
        if name in fixed:
            cc = np.arange(C)
            for s in ade.ROW_SLOTS[name]:
                g[r, cc, s] = abb(np.full(C, r), cc, s, fixed[name])
    for it in segs.items:                                                # the g assignments (:203-218)
        if it[0] != "g":
            continue
        rr, cc = _idx(it)
        for s in ade.slots_of(it[6]):
            g[rr, cc, s] = abb(rr, cc, s, it[8]) if it[7] == FIXED else gc[rr, cc, ade.OPP[s]]
    if body is not None:                                                 # the rectangle on g (:220-232)
        for idx, m in body.g_segments:
            for s in ade.slots_of(m):
                assert body.g_mode == FIXED and body.conc == 0.0
                g[idx + (s,)] = -gc[idx + (ade.OPP[s],)]
        if bc.row_hi == ade.BB and "row_hi" not in fixed:                # the bottom wall on g, last (:233-236)
            for s in ade.ROW_SLOTS["row_hi"]:
                g[R - 1, :, s] = gc[R - 1, :, ade.OPP[s]]
    return f, g


def loop(orc, segs, f, g, omega, omega_g, w, n, bc=None, fixed=None, body=None, by=None):
    """n iterations from the pre-collision (f, g): dict f, g, rho, u, C as ade_util.oracle_loop returns it"""
    bc = bc if bc is not None else pylbm.Bc()
    for _ in range(n):
        u_prev = calc_u(orc, f)
        c = ade.collide(orc, f, g, omega, omega_g, w, by)
        f, g = stream(orc, segs, bc, fixed or {}, c["fc"], c["gc"], u_prev, w, body)
    rho = orc.calc_rho(f)
    return dict(f=f, g=g, rho=rho, u=orc.calc_u(f, rho), C=orc.calc_rho(g))


def carry_of(table, u):
    """the carry of a table for the u [R, C, 2] of a state: two doubles per listed node, in the table's order"""
    return np.array([u[n["r"], n["c"]] for n in table.nodes()]).reshape(-1)
