"""Yardstick of the open boundaries and the wall exchange of the fluid + scalar step with a KBC fluid
(tests/test_gpu_ade_kbc_open.py): the driver's iteration composed on the CPU from parts the other suites already hold --
the collision of tests/ade_kbc_util.py (kbc::collide on the populations' own moments) or, with a buoyancy, of
tests/ade_kbc_buoyancy_util.py (on the held moments rho, u0 + u_shift F), the stream of tests/ade_open_util.py (the open
edges as sequential index assignments, the carry as the u at the start of the iteration) and, for the exchange, the
definition of tests/ade_exchange_reference.py.  Everything is imported, nothing is restated, and nothing here calls the
library under test (a table's node list is read from the host object the test built).

Interior walls enter the open stream as FURTHER ASSIGNMENTS of the same list: a wall node's f slots are bounce-back
assignments, its g slots NO_FLUX or FIXED assignments with the node's C_w, one node each, after the open table's own
-- which is what the step computes, since the two tables share no node that carries an open rule (the host checks) and the
interior-wall pass runs last and wins every slot it names."""
import numpy as np

import ade_exchange_reference as xref
import ade_kbc_buoyancy_util as kbc_buoyant
import ade_kbc_util as kbc
import ade_open_util as aou
import pylbm
from ade_open_util import BB_RULE, FIXED, NO_FLUX, Segments

S2, OMEGA_G, W = 1.9, kbc.OMEGA_G, (3e-3, -2e-3)
U_IN, CONC_W = 0.03, 1e-3
BETA, C_REF = (1.2e-2, -8e-3), 0.4  # both components, u_shift = 1 (pylbm.AdeBuoyancy's default)


def buoyancy():
    return pylbm.AdeBuoyancy(BETA, C_REF)


def collide(orc, f, g, by=None, s2=S2, omega_g=OMEGA_G, w=W):
    """the collision half of one iteration: fc, gc and the moments a raw call writes (u: the shifted one with `by`)"""
    if by is None:
        return kbc.collide(orc, f, g, s2, omega_g, w)
    c = kbc_buoyant.collide(orc, f, g, s2, omega_g, w, by)
    c.pop("gamma")
    return c


def with_walls(segs, wall_nodes):
    """the open table's segments followed by the interior-wall table (pylbm.AdeInteriorWalls.nodes()) as assignments"""
    out = Segments(segs.R, segs.C)
    out.items = list(segs.items)
    for nd in wall_nodes or ():
        r, c, fixed = nd["r"], nd["c"], nd["g_fixed_slots"]
        if nd["f_slots"]:
            out.f(r, c, 0, 1, 1, nd["f_slots"], BB_RULE)
        if nd["g_slots"] & ~fixed:
            out.g(r, c, 0, 1, 1, nd["g_slots"] & ~fixed, NO_FLUX)
        if fixed:
            out.g(r, c, 0, 1, 1, fixed, FIXED, nd["conc"])
    return out


def finite(state):
    return all(np.all(np.isfinite(v)) for v in state.values())


def loop(orc, segs, f, g, n, bc, fixed=None, wall_nodes=None, by=None, w=W):
    """n iterations from the pre-collision (f, g) -> dict f, g, rho, u, C (u = calc_u(f, rho), unshifted: what get_state
    returns, and the carry of the next step); asserted finite, since equal NaNs are equal bits"""
    segs = with_walls(segs, wall_nodes)
    for _ in range(n):
        u_prev = aou.calc_u(orc, f)
        c = collide(orc, f, g, by, w=w)
        f, g = aou.stream(orc, segs, bc, fixed or {}, c["fc"], c["gc"], u_prev, w)
    rho = orc.calc_rho(f)
    out = dict(f=f, g=g, rho=rho, u=orc.calc_u(f, rho), C=orc.calc_rho(g))
    assert finite(out), f"the yardstick is not finite after {n} iterations"
    return out


def exchange_loop(orc, f, g, n, bc, fixed, wall_nodes, by=None, region=None, w=W):
    """n iterations of a box with interior walls and no open table, the stream being the exchange definition's own
    (ade_exchange_reference.streamed_in_out): (state, values [NQ], row table [NQ, R]) of the LAST stream"""
    R, C = f.shape[:2]
    for _ in range(n):
        c = collide(orc, f, g, by, w=w)
        f_in, f, g_in, g = xref.streamed_in_out(orc, bc, fixed or {}, c["fc"], c["gc"], w, wall_nodes)
    table = xref.row_table(R, C, wall_nodes, f_in, f, g_in, g, region)
    state = dict(f=f, g=g)
    assert finite(state) and np.all(np.isfinite(table)), f"the yardstick is not finite after {n} iterations"
    return state, table
