"""The yardstick of tests/test_gpu_ade_kbc_buoyancy.py: the driver loop of the fluid + scalar step with a KBC fluid and
buoyancy, composed on the CPU.  It is tests/ade_kbc_util.collide with m1 replaced by u0 + u_shift F -- the oracle's
kbc::collide (Oracle.kbc_collide) on the moments the driver holds, F from calc_rho(g), the scalar half on the same shifted
u -- and tests/ade_util.stream for walls, FIXED edges and the body (they see calc_u of the streamed f: the unshifted u0).
The force and the shift are numpy expressions in the order of include/lbm_hip.h (element-wise f64 operations do not fuse).
Nothing here calls the library under test."""
import numpy as np

import pylbm
from ade_util import stream


def collide(orc, f, g, s2, omega_g, w, by):
    """the collision half of one iteration on the pre-collision (f, g): the post-collision pair and the moments the raw
    entry points write (u: the shifted one); gamma: kbc::collide's second result, for the stability report"""
    rho = orc.calc_rho(f)                                               # 1
    u0 = orc.calc_u(f, rho)
    conc = orc.calc_rho(g)                                              # 3
    dc = conc - by.c_ref                                                # 4
    Fr, Fc = dc * by.beta_r, dc * by.beta_c
    u = np.empty_like(u0)                                               # 5
    u[..., 0] = u0[..., 0] + by.u_shift * Fr
    u[..., 1] = u0[..., 1] + by.u_shift * Fc
    out = orc.kbc_collide(f, rho, u, s2)                                # 6: the held moments m0 = rho, m1 = u
    gc = orc.collision(g, orc.equilibrium(u + np.asarray(w), conc), omega_g)  # 7
    return dict(fc=out[0], gc=gc, rho=rho, u=u, C=conc, gamma=out[1])


def oracle_loop(orc, f, g, s2, omega_g, w, n, by, bc=None, fixed=None, body=None):
    """n iterations from the pre-collision (f, g); fixed, body as ade_util.oracle_loop.  The state get_state returns:
    u = calc_u(f, rho), unshifted"""
    bc = bc if bc is not None else pylbm.Bc()
    for _ in range(n):
        c = collide(orc, f, g, s2, omega_g, w, by)
        f, g = stream(orc, bc, fixed or {}, c["fc"], c["gc"], w, body)
    rho = orc.calc_rho(f)
    return dict(f=f, g=g, rho=rho, u=orc.calc_u(f, rho), C=orc.calc_rho(g))


def finite(state):
    return all(np.all(np.isfinite(v)) for v in state.values())


# ---- the vertical slot and the Rayleigh-Benard box of tests/test_gpu_ade_buoyancy.py, with a KBC fluid -------------------
SLOT_S2, SLOT_OMEGA_G, SLOT_BETA = 1.0, 1.2, 1e-4


def slot_initial(orc, R, C):
    """fluid at rest, uniform C = c_ref = 0.5; (f0, g0, n = 6 C^2 / nu steps)"""
    u = np.zeros((R, C, 2))
    nu = (1.0 / SLOT_S2 - 0.5) / 3.0
    return orc.equilibrium(u, np.ones((R, C))), orc.equilibrium(u, np.full((R, C), 0.5)), int(round(6 * C * C / nu))


def slot_errors(st, C):
    """(relative L2 error of the physical u_r = u0 + F / 2 against the cubic profile, max deviation of C from the linear
    profile, rows identical); u_shift = 1"""
    nu, L = (1.0 / SLOT_S2 - 0.5) / 3.0, float(C)
    x = np.arange(C) + 0.5
    exact = -(SLOT_BETA * 1.0 / nu) * (x ** 3 / (6 * L) - x ** 2 / 4 + x * L / 12)
    u_r = st["u"][..., 0] + 0.5 * (SLOT_BETA * (st["C"] - 0.5))
    same = bool(np.array_equal(u_r, np.repeat(u_r[:1], u_r.shape[0], axis=0)) and
                np.array_equal(st["C"], np.repeat(st["C"][:1], st["C"].shape[0], axis=0)))
    return (float(np.linalg.norm(u_r[0] - exact) / np.linalg.norm(exact)), float(np.max(np.abs(st["C"][0] - x / L))), same)


RB_R, RB_C, RB_S2 = 24, 48, 1.4
RB_NU = (1.0 / RB_S2 - 0.5) / 3.0
RB_T = int(RB_R ** 2 / RB_NU)
RA_THEORY = 1707.76  # rigid-rigid, critical wavenumber ~ pi / R: the box holds one wavelength 2 R


def rb_initial(orc):
    r, c = np.meshgrid(np.arange(RB_R, dtype=float), np.arange(RB_C, dtype=float), indexing="ij")
    conc = 1.0 - (r + 0.5) / RB_R + 1e-3 * np.sin(np.pi * (r + 0.5) / RB_R) * np.cos(2 * np.pi * c / RB_C)
    u = np.zeros((RB_R, RB_C, 2))
    return orc.equilibrium(u, np.ones((RB_R, RB_C))), orc.equilibrium(u, conc)


def rb_beta(Ra):
    return Ra * RB_NU ** 2 / RB_R ** 3


def rb_sigma(e1, e2):
    """sigma T = 1/2 ln(E(2T) / E(T)), E = sum u_c^2"""
    return 0.5 * float(np.log(e2 / e1))


def rb_ra_c(s_lo, s_hi):
    return 1500.0 + 450.0 * (0.0 - s_lo) / (s_hi - s_lo)
