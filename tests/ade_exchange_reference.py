"""Independent numpy restatement of the wall exchange (include/lbm_hip.h "wall exchange"), shared by
test_ade_wall_exchange_abi.py and test_gpu_ade_wall_exchange.py.  Nothing here calls the library.

One stream of the driver loop from the post-collision pair (fc, gc), as the index assignments of ade_util.driver_fix_up
with the TABLE as the body -- `nodes`: the merged table as a list of dicts r, c, f_slots, g_slots, g_fixed_slots, conc
(what pylbm.AdeInteriorWalls.nodes() lists on the host) -- noting every table-named slot immediately before the body's
assignment to that distribution (x_in) and after it (x_out).  d = x_in - x_out is what the wall takes; the per-node
terms accumulate from +0.0 over s = 1..8 ascending, named slots only; rows fold with fold64 over the row's nodes in
column order (a node outside the region is an element that adds nothing), ranges with fold64 over the row values."""
import numpy as np

import ade_util as ade
from ade_util import CX, CY, E9, OPP, ROW_SLOTS, slots_of
from diag_reference import fold64

NQ = 6
FORCE_R, FORCE_C, MASS, SCALAR, SCALAR_FIXED, NODES = range(NQ)


def streamed_in_out(orc, bc, fixed, fc, gc, w, nodes):
    """(f_in, f_out, g_in, g_out): the streamed lattices before and after the table's rule for each distribution"""
    f, g = orc.advect(fc), orc.advect(gc)
    ade.fix_up(orc, bc, {}, f, fc, g, gc, w)                           # the domain's walls, g no-flux
    f_in = f.copy()
    for nd in nodes:                                                   # the table on f
        for s in slots_of(nd["f_slots"]):
            f[nd["r"], nd["c"], s] = fc[nd["r"], nd["c"], OPP[s]]
    rho = orc.calc_rho(f)
    v = orc.calc_u(f, rho) + np.asarray(w)                             # the unshifted u of the fixed-up f

    def abb(idx, s, cw):
        q = OPP[s]
        vr, vc = v[idx + (0,)], v[idx + (1,)]
        cv = vr * CX[q] + vc * CY[q]
        vv = vr * vr + vc * vc
        return -gc[idx + (q,)] + 2.0 * ((((1.0 + 3.0 * cv) + 4.5 * (cv * cv)) - 1.5 * vv) * E9[q] * cw)

    R = f.shape[0]
    for name in ("row_lo", "row_hi"):                                  # the scalar's FIXED edges
        if name in fixed:
            idx = (0 if name == "row_lo" else R - 1, slice(None))
            for s in ROW_SLOTS[name]:
                g[idx + (s,)] = abb(idx, s, fixed[name])
    g_in = g.copy()
    for nd in nodes:                                                   # the table on g: it wins every slot it names
        idx = (nd["r"], nd["c"])
        for s in slots_of(nd["g_slots"]):
            if (nd["g_fixed_slots"] >> (s - 1)) & 1:
                g[idx + (s,)] = abb(idx, s, nd["conc"])
            else:
                g[idx + (s,)] = gc[idx + (OPP[s],)]
    return f_in, f, g_in, g


def node_terms(nd, f_in, f_out, g_in, g_out):
    """the NQ terms of one table node"""
    r, c = nd["r"], nd["c"]
    t = [0.0] * NQ
    for s in slots_of(nd["f_slots"]):
        d = f_in[r, c, s] - f_out[r, c, s]
        if CX[s] == 1:
            t[FORCE_R] = t[FORCE_R] + d
        if CX[s] == -1:
            t[FORCE_R] = t[FORCE_R] - d
        if CY[s] == 1:
            t[FORCE_C] = t[FORCE_C] + d
        if CY[s] == -1:
            t[FORCE_C] = t[FORCE_C] - d
        t[MASS] = t[MASS] + d
    for s in slots_of(nd["g_slots"]):
        d = g_in[r, c, s] - g_out[r, c, s]
        t[SCALAR] = t[SCALAR] + d
        if (nd["g_fixed_slots"] >> (s - 1)) & 1:
            t[SCALAR_FIXED] = t[SCALAR_FIXED] + d
    t[NODES] = 1.0
    return t


def row_table(R, C, nodes, f_in, f_out, g_in, g_out, region=None):
    """the row values [NQ, R]; region = (r0, r1, c0, c1), clipped to the lattice, None: every node"""
    r0, r1, c0, c1 = (0, R, 0, C) if region is None else region
    table = np.zeros((NQ, R))
    for r in range(R):
        row = sorted((nd for nd in nodes if nd["r"] == r), key=lambda nd: nd["c"])
        if not row:
            continue
        x = np.zeros((NQ, len(row)))
        for k, nd in enumerate(row):
            if r0 <= r < r1 and c0 <= nd["c"] < c1:
                x[:, k] = node_terms(nd, f_in, f_out, g_in, g_out)
        table[:, r] = fold64(x)
    return table


def fold_table(table, row_begin=0, row_end=None):
    """rows [row_begin, row_end) of a row table [NQ, rows] -> the NQ values"""
    table = np.asarray(table)
    row_end = table.shape[1] if row_end is None else row_end
    return np.array([fold64(table[q, row_begin:row_end]) for q in range(NQ)])


def exchange(orc, bc, fixed, fc, gc, w, nodes, region=None):
    """(values [NQ], row table [NQ, R]) of the stream from (fc, gc)"""
    R, C = fc.shape[:2]
    table = row_table(R, C, nodes, *streamed_in_out(orc, bc, fixed or {}, fc, gc, w, nodes), region)
    return fold_table(table), table
