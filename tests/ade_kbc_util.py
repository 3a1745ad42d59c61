"""Helpers of the suites of the fluid + scalar step with a KBC fluid (tests/test_ade_kbc_abi.py, tests/test_gpu_ade_kbc.py):
the parameters of the `_m` calls (made through tests/ade_calls.py) and the yardstick -- one driver iteration composed on
the CPU from the oracle's kbc::collide (Oracle.kbc_collide on the populations' own moments, as
ulbm_double_shear_flow.cpp:141-142 forms them) and the scalar half and wall rules of tests/ade_util.py.  The yardstick
never calls the library under test."""
import numpy as np

import pylbm
from ade_util import W, stream

S2 = 1.0 / (0.5 + 3 * 0.02)  # nu = 0.02: gamma far from its limits on the random states of ade_util.initial_state
OMEGA_G = 1.7


def params(form, s2=S2, w=W, omega_g=OMEGA_G):
    """(lbm_ade_fluid with a KBC fluid, lbm_ade_params), both halves in `form`"""
    return pylbm.AdeFluid(pylbm.KbcParams(s2, form)), pylbm.AdeParams(omega_g, w, form=form)


def collide(orc, f, g, s2, omega_g, w):
    """the collision half of one driver iteration on the pre-collision (f, g): the post-collision pair and the moments the
    raw entry points write"""
    m0 = orc.calc_rho(f)
    m1 = orc.calc_u(f, m0)
    fc = orc.kbc_collide(f, m0, m1, s2)[0]
    conc = orc.calc_rho(g)
    gc = orc.collision(g, orc.equilibrium(m1 + np.asarray(w), conc), omega_g)
    return dict(fc=fc, gc=gc, rho=m0, u=m1, C=conc)


def oracle_loop(orc, f, g, s2, omega_g, w, n, bc=None, fixed=None, body=None):
    """n iterations of the driver loop with a KBC fluid from the pre-collision (f, g); fixed, body as ade_util.oracle_loop"""
    bc = bc if bc is not None else pylbm.Bc()
    for _ in range(n):
        c = collide(orc, f, g, s2, omega_g, w)
        f, g = stream(orc, bc, fixed or {}, c["fc"], c["gc"], w, body)
    rho = orc.calc_rho(f)
    return dict(f=f, g=g, rho=rho, u=orc.calc_u(f, rho), C=orc.calc_rho(g))


def finite(state):
    return all(np.all(np.isfinite(v)) for v in state.values())
