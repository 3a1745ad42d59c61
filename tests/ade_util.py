"""Helpers shared by the GPU suites of the fluid + scalar solver (tests/test_gpu_ade_*.py): flat lattices with ghost rows
and padding, the write set of a launch into SENTINEL lattices, the start states, and the yardstick of the bitwise tests --
the reference's sediment loop composed from the oracle's solver:: primitives, with the wall rules, the interior walls and
the buoyant collision restated in numpy in the driver's expression order.  The yardstick never calls the library under
test.  The raw calls of the entry points are in tests/ade_calls.py, the chain of slabs in tests/ade_slab_util.py."""
import numpy as np
import torch

import pylbm
from gpu_util import bits_equal, dev

BB, SP = pylbm.EDGE_BOUNCE_BACK, pylbm.EDGE_SPECULAR
NO_FLUX = pylbm.ADE_SCALAR_NO_FLUX
SENTINEL = 0x7FF8DEADBEEF5A5A  # a quiet NaN no kernel computes: "never written"
PLANE_PAD = 40                 # doubles behind every plane (even: 16-byte alignment kept)
W = (3e-3, 3e-3)
E9 = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
OPP = [0, 3, 4, 1, 2, 7, 8, 5, 6]
GBC = pylbm.Bc(row_lo=BB, row_hi=BB, col_lo=BB, col_hi=SP)
REFERENCE = (1.0, (1.0 / 3.0, 1.0 / 9.0))  # buoyancy (u_shift, guo): test/gravity_test.cpp
GUO = (0.5, (3.0, 9.0))


# ---- lattices -----------------------------------------------------------------------------------------------------------
def geom(R, C, ghost, pitch=0):
    P = pitch or C
    return pylbm.Geom(R, C, ghost, (R + 2 * ghost) * P + PLANE_PAD, pitch)


def alloc(g):
    return torch.zeros(9 * g.plane_stride, dtype=torch.float64, device=dev())


def rows_view(t, g):
    """[9, R + 2 ghost, C] view: every stored row (ghost rows included) of a flat lattice"""
    P = g.row_pitch or g.C
    return t.view(9, g.plane_stride)[:, :(g.R + 2 * g.ghost) * P].view(9, g.R + 2 * g.ghost, P)[:, :, :g.C]


def owned(t, g):
    return rows_view(t, g)[:, g.ghost:g.ghost + g.R]


def random_lattice(g, seed):
    """a finite post-collision-like lattice: every double of the allocation near w_q"""
    rng = np.random.default_rng(seed)
    a = np.repeat(E9, g.plane_stride).reshape(9, g.plane_stride) * (1.0 + 0.05 * rng.random((9, g.plane_stride)))
    return torch.from_numpy(a.reshape(-1)).to(dev())


def to_lattice(a, g):
    """numpy AoS [R, C, 9] -> the owned rows of a fresh flat lattice"""
    t = alloc(g)
    owned(t, g)[:] = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(dev())
    return t


def from_lattice(t, g):
    return np.ascontiguousarray(owned(t, g).cpu().numpy().transpose(1, 2, 0))


def bits(t):
    return t.view(torch.int64)


def assert_bits(got, want, what):
    bad = torch.nonzero(bits(got) != bits(want))
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} doubles differ; first at {tuple(bad[0].tolist())}"


def assert_state_bits(got, want, what):
    for k in ("f", "g", "rho", "u", "C"):
        assert bits_equal(got[k], want[k]), f"{what}: {k} differs, max |d| = {np.max(np.abs(got[k] - want[k]))}"


def cut_slab(glob, gg, r0, r1, pitch, closed=False):
    """ghost-1 slab of global rows [r0, r1): owned rows and the ghost rows beside them (wrapped on a closed domain;
    left poisoned beyond a wall end -- nothing may read them)"""
    sg = geom(r1 - r0, gg.C, 1, pitch)
    t = alloc(sg)
    bits(t).fill_(SENTINEL)
    rv, src = rows_view(t, sg), owned(glob, gg)
    rv[:, 1:1 + sg.R] = src[:, r0:r1]
    for slab_row, grow in ((0, r0 - 1), (sg.R + 1, r1)):
        if 0 <= grow < gg.R or closed:
            rv[:, slab_row] = src[:, grow % gg.R]
    return sg, t


# ---- parameters, poisoned targets and the write set ---------------------------------------------------------------------
def params(form, w=W, omega=1.2, omega_g=1.7):
    return pylbm.BgkParams(omega, 0, form=form), pylbm.AdeParams(omega_g, w, form=form)


def poisoned(g):
    """a flat lattice with every double of the allocation -- ghost rows and padding included -- set to SENTINEL"""
    t = alloc(g)
    bits(t).fill_(SENTINEL)
    return t


def moment_fields(g):
    """dense rho [R C], u [2 R C], conc [R C] for the raw entry points, every double SENTINEL"""
    m = [torch.zeros(n * g.R * g.C, dtype=torch.float64, device=dev()) for n in (1, 2, 1)]
    for t in m:
        bits(t).fill_(SENTINEL)
    return m


def assert_write_set(t, g, rows, what):
    """of a lattice that was SENTINEL everywhere: exactly the owned nodes of `rows` are written, in all 9 planes -- no
    ghost row, no row padding, no plane padding"""
    expect = torch.zeros(9 * g.plane_stride, dtype=torch.bool, device=dev())
    owned(expect, g)[:, rows] = True
    wrong = torch.nonzero((bits(t) != SENTINEL) != expect)
    assert wrong.numel() == 0, f"{what}: {wrong.shape[0]} doubles wrong, first flat index {int(wrong[0, 0])} " \
                               f"({'missed' if bool(expect[int(wrong[0, 0])]) else 'over-written'})"


# ---- the yardstick ------------------------------------------------------------------------------------------------------
def initial_state(orc, R, C, seed=0, w=W, conc_rows=None, scale=1.0):
    """f: shear wave plus noise; g: equilibrium(u + w, C) of a Gaussian, C in [0, scale * 1e-3] -- or, with conc_rows = (a, b),
    of a blob confined to rows [a, b): exactly zero elsewhere"""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(R, dtype=float), np.arange(C, dtype=float), indexing="ij")
    u = np.zeros((R, C, 2))
    u[..., 1] = 0.03 * np.sin(2 * np.pi * r / R)
    u += 0.005 * rng.standard_normal((R, C, 2))
    rho = 1 + 0.01 * rng.standard_normal((R, C))
    f = orc.equilibrium(u, rho) * (1 + 0.005 * rng.standard_normal((R, C, 9)))
    s = 0.15 * min(R, C)
    if conc_rows is None:
        conc = scale * 1e-3 * np.exp(-((r - 0.4 * R) ** 2 + (c - 0.55 * C) ** 2) / (2 * s * s))
    else:
        a, b = conc_rows
        conc = np.where((r >= a) & (r < b), scale * 1e-3 * np.exp(-((r - (a + b) / 2) ** 2 + (c - C / 2) ** 2) / (2 * s * s)), 0.0)
    return f, orc.equilibrium(u + np.asarray(w), conc)


def buoyant_initial_state(orc, R, C, seed, w=(3e-3, -2e-3)):
    """that state with the scalar scaled to C in [0, 1]: forces of ~1e-3 with beta ~ 1e-3"""
    f, g = initial_state(orc, R, C, seed=seed, w=w)
    return f, g * 1e3


def buoyancy(beta, c_ref, variant):
    return pylbm.AdeBuoyancy(beta, c_ref, variant[0], variant[1])


def build_sbc(spec, R, C):
    """(pylbm.AdeScalarBC, numpy C_w per edge for the yardstick, device profiles kept alive); spec: edge -> a float, or
    ('profile', host array)"""
    kw, fixed = {}, {}
    for name, v in spec.items():
        n = C if name.startswith("row") else R
        if isinstance(v, tuple):
            t = torch.from_numpy(np.ascontiguousarray(v[1])).to(dev())
            kw[name] = (0.0, t)
            fixed[name] = v[1].copy()
        else:
            kw[name] = v
            fixed[name] = np.full(n, float(v))
    return pylbm.AdeScalarBC(**kw), fixed


ROW_SLOTS = {"row_lo": (1, 5, 8), "row_hi": (3, 7, 6)}
COL_SLOTS = {"col_lo": (2, 5, 6), "col_hi": (4, 7, 8)}


def _edge_index(name, R, C):
    return {"row_lo": (0, slice(None)), "row_hi": (R - 1, slice(None)), "col_lo": (slice(None), 0),
            "col_hi": (slice(None), C - 1)}[name]


def fix_up(orc, bc, fixed, f, fc, g, gc, w):
    """the wall fix-ups of one iteration: f as d2q9.hpp gather_bc (rows first, columns win); g the same where its edge
    is NO_FLUX, anti-bounce-back where fixed[edge] = C_w array along the edge (length C or R)"""
    R, C = f.shape[:2]
    for name in ("row_lo", "row_hi"):
        if getattr(bc, name) == BB:
            idx = _edge_index(name, R, C)
            for s in ROW_SLOTS[name]:
                f[idx + (s,)] = fc[idx + (OPP[s],)]
                g[idx + (s,)] = gc[idx + (OPP[s],)]
    for name in ("col_hi", "col_lo"):
        mode = getattr(bc, name)
        if mode not in (BB, SP):
            continue
        idx = _edge_index(name, R, C)
        a, b, d = COL_SLOTS[name]  # a: straight; b, d: the diagonals (swapped by specular)
        src = {a: OPP[a], b: OPP[b], d: OPP[d]}
        if mode == SP:
            src = {a: OPP[a], b: OPP[d], d: OPP[b]}
        for s, q in src.items():
            f[idx + (s,)] = fc[idx + (q,)]
            if name not in fixed:
                g[idx + (s,)] = gc[idx + (q,)]
    if not fixed:
        return
    rho = orc.calc_rho(f)
    u = orc.calc_u(f, rho)
    v = u + np.asarray(w)
    for name in ("row_lo", "row_hi", "col_lo", "col_hi"):  # rows first: the columns overwrite the corners
        if name not in fixed:
            continue
        idx = _edge_index(name, R, C)
        slots = ROW_SLOTS.get(name) or COL_SLOTS[name]
        vr, vc = v[idx + (0,)], v[idx + (1,)]
        vv = vr * vr + vc * vc
        cw = fixed[name]
        for s in slots:
            q = OPP[s]
            cv = vr * CX[q] + vc * CY[q]
            g[idx + (s,)] = -gc[idx + (q,)] + 2.0 * ((((1.0 + 3.0 * cv) + 4.5 * (cv * cv)) - 1.5 * vv) * E9[q] * cw)
    # a NO_FLUX column wins its corner slots back from a FIXED row
    for name in ("col_hi", "col_lo"):
        mode = getattr(bc, name)
        if name in fixed or mode not in (BB, SP):
            continue
        idx = _edge_index(name, R, C)
        a, b, d = COL_SLOTS[name]
        src = {a: OPP[a], b: OPP[b], d: OPP[d]} if mode == BB else {a: OPP[a], b: OPP[d], d: OPP[b]}
        for s, q in src.items():
            g[idx + (s,)] = gc[idx + (q,)]


def slots_of(mask):
    return [s for s in range(1, 9) if (mask >> (s - 1)) & 1]


class Body:
    """interior walls as index assignments in the order the sedimentation driver makes them: f segments and g segments,
    each (rows, cols, slot mask) with numpy indices; the g segments share one rule (absorbing = FIXED at 0, FIXED at conc,
    or NO_FLUX)"""

    def __init__(self, f_segments, g_segments, g_mode=pylbm.ADE_SCALAR_FIXED, conc=0.0):
        self.f_segments, self.g_segments, self.g_mode, self.conc = f_segments, g_segments, g_mode, conc


def driver_fix_up(orc, bc, fixed, body, f, fc, g, gc, w):
    """one iteration's index assignments after advect with a body, in the driver's order (columns periodic)"""
    fix_up(orc, bc, {}, f, fc, g, gc, w)                              # the domain's walls, g no-flux (:179-182)
    for idx, mask in body.f_segments:                                  # the rectangle on f (:184-196)
        for s in slots_of(mask):
            f[idx + (s,)] = fc[idx + (OPP[s],)]
    rho = orc.calc_rho(f)                                              # :198-200
    v = orc.calc_u(f, rho) + np.asarray(w)

    def abb(idx, s, cw):
        q = OPP[s]
        vr, vc = v[idx + (0,)], v[idx + (1,)]
        cv = vr * CX[q] + vc * CY[q]
        vv = vr * vr + vc * vc
        return -gc[idx + (q,)] + 2.0 * ((((1.0 + 3.0 * cv) + 4.5 * (cv * cv)) - 1.5 * vv) * E9[q] * cw)

    R, C = f.shape[:2]
    for name in ("row_lo", "row_hi"):                                  # the scalar's FIXED edges (:203-218)
        if name in fixed:
            idx = _edge_index(name, R, C)
            for s in ROW_SLOTS[name]:
                g[idx + (s,)] = abb(idx, s, fixed[name])
    for idx, mask in body.g_segments:                                  # the rectangle on g (:220-232)
        for s in slots_of(mask):
            if body.g_mode == NO_FLUX:
                g[idx + (s,)] = gc[idx + (OPP[s],)]
            elif body.conc == 0.0:
                g[idx + (s,)] = -gc[idx + (OPP[s],)]                   # the driver's own expression
            else:
                g[idx + (s,)] = abb(idx, s, body.conc)
    if bc.row_hi == BB and "row_hi" not in fixed:                      # the bottom wall on g, last (:233-236)
        for s in ROW_SLOTS["row_hi"]:
            g[R - 1, :, s] = gc[R - 1, :, OPP[s]]


def buoyant_collide(orc, f, g, omega, omega_g, w, by):
    """one node-local half iteration on the pre-collision (f, g): items 1 and 3-7 of the step in include/lbm_hip.h, in
    numpy in exactly that order (element-wise f64 operations do not fuse); returns the post-collision pair and the moments
    the raw entry points write (u: the shifted one)"""
    rho = orc.calc_rho(f)                                               # 1
    u0 = orc.calc_u(f, rho)
    conc = orc.calc_rho(g)                                              # 3
    dc = conc - by.c_ref                                                # 4
    Fr, Fc = dc * by.beta_r, dc * by.beta_c
    u = np.empty_like(u0)                                               # 5
    u[..., 0] = u0[..., 0] + by.u_shift * Fr
    u[..., 1] = u0[..., 1] + by.u_shift * Fc
    fe = orc.equilibrium(u, rho)                                        # 6
    uF = u[..., 0] * Fr + u[..., 1] * Fc
    fc = np.empty_like(f)
    for q in range(9):
        cu = u[..., 0] * float(CX[q]) + u[..., 1] * float(CY[q])
        cF = Fr * float(CX[q]) + Fc * float(CY[q])
        S = ((1 - 0.5 * omega) * ((by.guo_a + by.guo_b * cu) * cF - by.guo_a * uF) * E9[q])
        fc[..., q] = f[..., q] + (-omega * (f[..., q] - fe[..., q])) + S
    ge = orc.equilibrium(u + np.asarray(w), conc)                       # 7
    gc = orc.collision(g, ge, omega_g)
    return dict(fc=fc, gc=gc, rho=rho, u=u, C=conc)


def collide(orc, f, g, omega, omega_g, w, by=None):
    """the collision half of one driver iteration on the pre-collision (f, g): what the raw entry points store -- the
    post-collision pair fc, gc -- and the moments they write (u: the shifted one where there is a buoyancy)"""
    if by is not None:
        return buoyant_collide(orc, f, g, omega, omega_g, w, by)
    rho = orc.calc_rho(f)
    u = orc.calc_u(f, rho)
    conc = orc.calc_rho(g)
    fc = orc.collision(f, orc.equilibrium(u, rho), omega)
    gc = orc.collision(g, orc.equilibrium(u + np.asarray(w), conc), omega_g)
    return dict(fc=fc, gc=gc, rho=rho, u=u, C=conc)


def stream(orc, bc, fixed, fc, gc, w, body=None):
    """advect both and apply the wall rules (the scalar's rule sees calc_u of the streamed f, the UNSHIFTED velocity)"""
    f, g = orc.advect(fc), orc.advect(gc)
    if body is None:
        fix_up(orc, bc, fixed, f, fc, g, gc, w)
    else:
        driver_fix_up(orc, bc, fixed, body, f, fc, g, gc, w)
    return f, g


def oracle_loop(orc, f, g, omega, omega_g, w, n, bc=None, fixed=None, body=None, by=None):
    """n iterations of the driver loop from the pre-collision (f, g); fixed: {edge: C_w array} of the scalar's FIXED
    edges, body: interior walls (Body), by: pylbm.AdeBuoyancy -- each None: not there"""
    bc = bc if bc is not None else pylbm.Bc()
    fixed = fixed or {}
    for _ in range(n):
        if by is None:
            rho = orc.calc_rho(f)
            u = orc.calc_u(f, rho)
            conc = orc.calc_rho(g)
            fe = orc.equilibrium(u, rho)
            ge = orc.equilibrium(u + np.asarray(w), conc)
            fc = orc.collision(f, fe, omega)
            gc = orc.collision(g, ge, omega_g)
        else:
            c = buoyant_collide(orc, f, g, omega, omega_g, w, by)
            fc, gc = c["fc"], c["gc"]
        f, g = stream(orc, bc, fixed, fc, gc, w, body)
    rho = orc.calc_rho(f)
    return dict(f=f, g=g, rho=rho, u=orc.calc_u(f, rho), C=orc.calc_rho(g))
