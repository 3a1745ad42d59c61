"""The 80-bit yardstick of the collisions: the mathematics of every node-local collision evaluated in vectorised
np.longdouble (x87 extended precision, 64-bit significand), the unit in which a double result is judged against it, and
the states on which tests/test_exact_collide.py (CPU oracle) and tests/test_gpu_collision_accuracy.py (HIP kernels, both
forms) measure.

Nothing here calls the library under test or the oracle: every value comes from numpy.  Constants are built in long
double (LD(1) / 3, never 1.0 / 3.0); inputs are doubles and convert exactly; outputs are long double.

The yardstick's own error: the longest chain (KBC) is about 200 long-double operations per output, none of them a
cancellation the double forms do not share, so its result is within about 200 x 2^-64 ~ 1e-17 relative of the exact
value -- below 0.1 unit (a unit is >= 2^-53 relative to the largest term of the update).  It resolves single units.

The unit of an output is the spacing of doubles at a magnitude the update's own terms set, so that a cancelling update
(omega > 1: keep = 1 - omega < 0) is not judged against a tiny result:
  population q   np.spacing(max(|f_q|, |feq_q|, |f*_q|)) of the 80-bit values;
  rho, C         the spacing at sum_q |f_q| (sum_q |g_q|);
  u              the spacing at (sum_q |c_q f_q|) / |rho|, the sum taken per component (six populations each) and the
                 larger of the two used for both components.
"""
import collections
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, \
    f"np.longdouble has a {np.finfo(LD).nmant}-bit significand here: the 80-bit yardstick needs x87 extended precision"

CX = (0, 1, 0, -1, 0, 1, -1, -1, 1)   # row component of c_q (the reference calls the rows x)
CY = (0, 0, 1, 0, -1, 1, 1, -1, -1)
_ONE = LD(1)
_W = [LD(4) / 9] + [_ONE / 9] * 4 + [_ONE / 36] * 4
_CS2, _CS4 = _ONE / 3, _ONE / 9
_HALF, _QUARTER, _EIGHTH = _ONE / 2, _ONE / 4, _ONE / 8

# pop [n, 9 or 18]: f* (then g*); mom [n, 3 or 4]: rho, u_r, u_c (then C); the units alike; u [n, 2]: the 80-bit velocity
Exact = collections.namedtuple("Exact", "pop pop_unit mom mom_unit u")


def _ld(a):
    a = np.asarray(a)
    assert a.dtype == np.float64, a.dtype
    return a.astype(LD)


def _spacing(mag):
    """spacing of doubles at the magnitudes mag (long double), as long double"""
    return np.spacing(np.abs(mag).astype(np.float64)).astype(LD)


def _pop_unit(f, feq, fstar):
    return _spacing(np.maximum(np.maximum(np.abs(f), np.abs(feq)), np.abs(fstar)))


def _moments(f):
    rho = sum(f[:, q] for q in range(9))
    jx = sum(f[:, q] * CX[q] for q in range(1, 9))
    jy = sum(f[:, q] * CY[q] for q in range(1, 9))
    u = np.stack([jx / rho, jy / rho], axis=1)
    unit_rho = _spacing(np.sum(np.abs(f), axis=1))
    ax = sum(np.abs(f[:, q]) for q in range(9) if CX[q])
    ay = sum(np.abs(f[:, q]) for q in range(9) if CY[q])
    unit_u = _spacing(np.maximum(ax, ay) / np.abs(rho))
    return rho, u, np.stack([unit_rho, unit_u, unit_u], axis=1)


def _feq(rho, ux, uy):
    """solver::equilibrium: w_q rho (1 + 3 c.u + 4.5 (c.u)^2 - 1.5 u.u)"""
    uu = ux * ux + uy * uy
    cols = []
    for q in range(9):
        cu = ux * CX[q] + uy * CY[q]
        cols.append(_W[q] * rho * (1 + 3 * cu + LD(9) / 2 * cu * cu - LD(3) / 2 * uu))
    return np.stack(cols, axis=1)


def bgk(f, omega):
    """BGK: rho, u = j / rho, f* = f + omega (feq - f) -- both ways the drivers write the relaxation are this"""
    f = _ld(f)
    rho, u, mom_unit = _moments(f)
    feq = _feq(rho, u[:, 0], u[:, 1])
    fstar = f + LD(omega) * (feq - f)
    return Exact(fstar, _pop_unit(f, feq, fstar), np.concatenate([rho[:, None], u], axis=1), mom_unit, u)


def _kbc_feq_poly(ux, uy, ux2, uy2):
    """eval_equilibrium / eval_iequilibrium, to be scaled by m0"""
    c2, c4 = _CS2, _CS4
    return [
        2 * c2 * (_HALF * ux2 + _HALF * uy2 - 1) + c4 + ux2 * uy2 - ux2 - uy2 + 1,
        _HALF * (-c2 * (ux2 + uy2 + ux - 1) - c4 - ux2 * uy2 + ux2 - uy2 * ux + ux),
        _HALF * (-c2 * (ux2 + uy2 + uy - 1) - c4 - ux2 * uy2 - ux2 * uy + uy2 + uy),
        _HALF * (-c2 * (ux2 + uy2 - ux - 1) - c4 - ux2 * uy2 + ux2 + uy2 * ux - ux),
        _HALF * (-c2 * (ux2 + uy2 - uy - 1) - c4 - ux2 * uy2 + ux2 * uy + uy2 - uy),
        _QUARTER * (c2 * (ux2 + uy2 + ux + uy) + c4 + ux2 * uy2 + ux2 * uy + uy2 * ux + ux * uy),
        _QUARTER * (c2 * (ux2 + uy2 - ux + uy) + c4 + ux2 * uy2 + ux2 * uy - uy2 * ux - ux * uy),
        _QUARTER * (c2 * (ux2 + uy2 - ux - uy) + c4 + ux2 * uy2 - ux2 * uy - uy2 * ux + ux * uy),
        _QUARTER * (c2 * (ux2 + uy2 + ux - uy) + c4 + ux2 * uy2 - ux2 * uy + uy2 * ux - ux * uy),
    ]


def kbc(f, s2):
    """kbc::collide (the reference's src/ulbm.cpp:91-320, the lines the oracle and kbc.hpp KbcModel cite) on the
    populations' own moments m0 = rho, m1 = j / rho.  The "ux2 + uy" terms of eval_delta_h rows 5-8 are kept as the
    reference writes them: both GPU forms reproduce them on purpose."""
    f = _ld(f)
    m0, u, mom_unit = _moments(f)
    ux, uy = u[:, 0], u[:, 1]
    s2 = LD(s2)
    is2 = 1 / s2
    c2, c4, H, Q4, E8 = _CS2, _CS4, _HALF, _QUARTER, _EIGHTH
    ux2, uy2 = ux * ux, uy * uy
    # eval_central_momenta
    T = [0] * 9
    for q in range(9):
        cmx, cmy = CX[q] - ux, CY[q] - uy
        cmx2, cmy2 = cmx * cmx, cmy * cmy
        fq = f[:, q]
        T[0] = T[0] + fq
        T[1] = T[1] + fq * cmx
        T[2] = T[2] + fq * cmy
        T[3] = T[3] + fq * (cmx2 + cmy2)
        T[4] = T[4] + fq * (cmx2 - cmy2)
        T[5] = T[5] + fq * cmx * cmy
        T[6] = T[6] + fq * cmx2 * cmy
        T[7] = T[7] + fq * cmx * cmy2
        T[8] = T[8] + fq * cmx2 * cmy2
    C4, C5, C6, C7, C8 = T[4], T[5], T[6], T[7], T[8]
    D3 = T[3] - 2 * c2 * m0
    x2y2 = ux2 * uy2
    # eval_delta_s
    ds = [
        -H * C4 * (ux2 - uy2) + 4 * C5 * ux * uy - c4 * m0 - m0 * (x2y2 - ux2 - uy2 + 1) + D3 * (H * ux2 + H * uy2 - 1),
        Q4 * C4 * (ux2 - uy2 + ux + 1) - C5 * uy * (2 * ux + 1) + H * c4 * m0 + H * m0 * (x2y2 - ux2 + uy2 * ux - ux) - Q4 * D3 * (ux2 + uy2 + ux - 1),
        -Q4 * C4 * (-ux2 + uy2 + uy + 1) - C5 * ux * (2 * uy + 1) + H * c4 * m0 + H * m0 * (x2y2 - uy2 + ux2 * uy - uy) - Q4 * D3 * (ux2 + uy2 + uy - 1),
        Q4 * C4 * (ux2 - uy2 - ux + 1) - C5 * uy * (2 * ux - 1) + H * c4 * m0 + H * m0 * (x2y2 - ux2 - uy2 * ux + ux) - Q4 * D3 * (ux2 + uy2 - ux - 1),
        Q4 * C4 * (ux2 - uy2 + uy - 1) - C5 * ux * (2 * uy - 1) + H * c4 * m0 + H * m0 * (x2y2 - uy2 - ux2 * uy + uy) - Q4 * D3 * (ux2 + uy2 - uy - 1),
        -E8 * C4 * (ux2 - uy2 + ux - uy) + C5 * (ux * uy + H * ux + H * uy + Q4) - Q4 * c4 * m0 - Q4 * m0 * (x2y2 + ux2 * uy + uy2 * ux + ux * uy) + E8 * D3 * (ux2 + uy2 + ux + uy),
        E8 * C4 * (-ux2 + uy2 + ux + uy) + C5 * (ux * uy + H * ux - H * uy - Q4) - Q4 * c4 * m0 - Q4 * m0 * (x2y2 + ux2 * uy - uy2 * ux - ux * uy) + E8 * D3 * (ux2 + uy2 - ux + uy),
        -E8 * C4 * (ux2 - uy2 - ux + uy) + C5 * (ux * uy - H * ux - H * uy + Q4) - Q4 * c4 * m0 - Q4 * m0 * (x2y2 - ux2 * uy - uy2 * ux + ux * uy) + E8 * D3 * (ux2 + uy2 - ux - uy),
        -E8 * C4 * (ux2 - uy2 + ux + uy) + C5 * (ux * uy - H * ux + H * uy - Q4) - Q4 * c4 * m0 - Q4 * m0 * (x2y2 - ux2 * uy + uy2 * ux - ux * uy) + E8 * D3 * (ux2 + uy2 + ux - uy),
    ]
    # eval_delta_h; rows 5-8: "ux2 + uy" where the algebra has ux2 * uy, as the reference writes it
    dh = [
        2 * C6 * uy + 2 * C7 * ux + C8 - 2 * c2 * m0 * (H * ux2 + H * uy2 - 1) - c4 * m0 - m0 * (x2y2 - ux2 - uy2 + 1),
        -C6 * uy - C7 * (ux + H) - H * C8 + H * c2 * m0 * (ux2 + uy2 + ux - 1) + H * c4 * m0 + H * m0 * (x2y2 - ux2 + uy2 * ux - ux),
        -C6 * (uy + H) - C7 * ux - H * C8 + H * c2 * m0 * (ux2 + uy2 + uy - 1) + H * c4 * m0 + H * m0 * (x2y2 + ux2 * uy - uy2 - uy),
        -C6 * uy - C7 * (ux - H) - H * C8 + H * c2 * m0 * (ux2 + uy2 - ux - 1) + H * c4 * m0 + H * m0 * (x2y2 - ux2 - uy2 * ux + ux),
        -C6 * (uy - H) - C7 * ux - H * C8 + H * c2 * m0 * (ux2 + uy2 - uy - 1) + H * c4 * m0 + H * m0 * (x2y2 - ux2 * uy - uy2 + uy),
        C6 * (H * uy + Q4) + C7 * (H * ux + Q4) + Q4 * C8 - Q4 * c2 * m0 * (ux2 + uy2 + ux + uy) - Q4 * c4 * m0 - Q4 * m0 * (x2y2 + ux2 + uy + uy2 * ux + ux * uy),
        C6 * (H * uy + Q4) + C7 * (H * ux - Q4) + Q4 * C8 - Q4 * c2 * m0 * (ux2 + uy2 - ux + uy) - Q4 * c4 * m0 - Q4 * m0 * (x2y2 + ux2 + uy - uy2 * ux - ux * uy),
        C6 * (H * uy - Q4) + C7 * (H * ux - Q4) + Q4 * C8 - Q4 * c2 * m0 * (ux2 + uy2 - ux - uy) - Q4 * c4 * m0 - Q4 * m0 * (x2y2 - ux2 + uy - uy2 * ux + ux * uy),
        C6 * (H * uy - Q4) + C7 * (H * ux + Q4) + Q4 * C8 - Q4 * c2 * m0 * (ux2 + uy2 + ux - uy) - Q4 * c4 * m0 - Q4 * m0 * (x2y2 - ux2 + uy + uy2 * ux - ux * uy),
    ]
    poly = _kbc_feq_poly(ux, uy, ux2, uy2)
    # eval_gamma
    num = sum(ds[q] * dh[q] / (poly[q] * m0) for q in range(9))
    den = sum(dh[q] * dh[q] / (poly[q] * m0) for q in range(9))
    gamma = is2 - (1 - is2) * num / den
    # collide: the deviations from the equilibrium's central moments, relaxed, back to populations
    T[0] = T[0] - m0
    T[3] = T[3] - 2 * c2 * m0
    T[8] = T[8] - c4 * m0
    gs = gamma * s2
    T0, T1, T2, T3, T4, T5, T6, T7, T8 = T[0], T[1], T[2], T[3] * s2, T[4] * s2, T[5] * s2, T[6] * gs, T[7] * gs, T[8] * gs
    i0 = T0
    i1 = T0 * ux + T1
    i2 = T0 * uy + T2
    i3 = T0 * (ux2 + uy2) + 2 * T1 * ux + 2 * T2 * uy + T3
    i4 = T0 * (ux2 - uy2) + 2 * T1 * ux - 2 * T2 * uy + T4
    i5 = T0 * ux * uy + T1 * uy + T2 * ux + T5
    i6 = T0 * ux2 * uy + 2 * T1 * ux * uy + T2 * ux2 + H * T3 * uy + H * T4 * uy + 2 * T5 * ux + T6
    i7 = T0 * ux * uy2 + T1 * uy2 + 2 * T2 * ux * uy + H * T3 * ux - H * T4 * ux + 2 * T5 * uy + T7
    i8 = T0 * x2y2 + 2 * T1 * ux * uy2 + 2 * T2 * ux2 * uy + H * T3 * (ux2 + uy2) - H * T4 * (ux2 - uy2) + 4 * T5 * ux * uy + 2 * T6 * uy + 2 * T7 * ux + T8
    o = [
        i0 - i3 + i8,
        H * i1 + Q4 * i3 + Q4 * i4 - H * i7 - H * i8,
        H * i2 + Q4 * i3 - Q4 * i4 - H * i6 - H * i8,
        -H * i1 + Q4 * i3 + Q4 * i4 + H * i7 - H * i8,
        -H * i2 + Q4 * i3 - Q4 * i4 + H * i6 - H * i8,
        Q4 * (i5 + i6 + i7 + i8),
        Q4 * (-i5 + i6 - i7 + i8),
        Q4 * (i5 - i6 - i7 + i8),
        Q4 * (-i5 - i6 + i7 + i8),
    ]
    fstar = f - np.stack(o, axis=1)
    feq = np.stack(poly, axis=1) * m0[:, None]
    return Exact(fstar, _pop_unit(f, feq, fstar), np.concatenate([m0[:, None], u], axis=1), mom_unit, u)


def with_scalar(fluid, g, omega_g, w):
    """the scalar half behind a fluid's Exact: C = sum g, geq = feq(C, u + w) with the fluid's 80-bit u, g* = g +
    omega_g (geq - g); pop becomes f* then g*, mom rho, u, C"""
    g = _ld(g)
    conc = sum(g[:, q] for q in range(9))
    geq = _feq(conc, fluid.u[:, 0] + LD(w[0]), fluid.u[:, 1] + LD(w[1]))
    gstar = g + LD(omega_g) * (geq - g)
    unit_c = _spacing(np.sum(np.abs(g), axis=1))
    return Exact(np.concatenate([fluid.pop, gstar], axis=1), np.concatenate([fluid.pop_unit, _pop_unit(g, geq, gstar)], axis=1),
                 np.concatenate([fluid.mom, conc[:, None]], axis=1), np.concatenate([fluid.mom_unit, unit_c[:, None]], axis=1),
                 fluid.u)


def errors(got, exact, unit):
    """per node, the largest |got - exact| / unit over that node's outputs (got: doubles [n, k])"""
    return np.max(np.abs(_ld(np.ascontiguousarray(got, dtype=np.float64)) - exact) / unit, axis=1).astype(np.float64)


def stats(err):
    """(median, 99th percentile, maximum) over nodes"""
    err = np.asarray(err, dtype=np.float64)
    return float(np.median(err)), float(np.percentile(err, 99)), float(np.max(err))


# ---- the states ---------------------------------------------------------------------------------------------------------
# The edges where kernels go wrong, not the workload: rho far from 1, Mach 0.25, populations at, next to and far from
# equilibrium, and the exact corner cases below, each on 2 % of the nodes, laid out by node index.
E9 = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
NOISE = (0.0, 1e-9, 1e-2, 0.3)
CONC = (1e-12, 1e-3, 1.0, 50.0)   # and C = 0 exactly on every node with index % ZERO_C_EVERY == ZERO_C_AT: 4 %
ZERO_C_EVERY, ZERO_C_AT = 25, 7
CORNER_EVERY = 50                 # index % 50 == 0: rest; 1: u on an axis; 2: ux = +-uy; 3: f_1 = f_3 and f_2 = f_4


def _feq_bgk(rho, u):
    uu = u[:, 0] ** 2 + u[:, 1] ** 2
    cu = u[:, :1] * np.array(CX, dtype=float) + u[:, 1:] * np.array(CY, dtype=float)
    return E9 * rho[:, None] * (1 + 3 * cu + 4.5 * cu * cu - 1.5 * uu[:, None])


def _feq_product(rho, u):
    """KbcModel::feq_poly in its product form: rho psi_cx(u_r) psi_cy(u_c), psi_0 = 2/3 - u^2, psi_+- = (u^2 + 1/3 +- u) / 2"""
    def psi(v):
        return {0: 2 / 3 - v * v, 1: 0.5 * (v * v + 1 / 3 + v), -1: 0.5 * (v * v + 1 / 3 - v)}
    px, py = psi(u[:, 0]), psi(u[:, 1])
    return np.stack([rho * px[CX[q]] * py[CY[q]] for q in range(9)], axis=1)


def states(cls, n, seed, w=(0.0, 0.0)):
    """n pre-collision nodes of class cls ("bgk", "kbc": f; "ade_bgk", "ade_kbc": f and g with the scalar's drift w):
    f = feq_model(rho, u) (1 + noise N(0, 1)) rounded to double, rho uniform in [0.2, 5], |u| <= 0.25 in any direction,
    noise drawn per node from NOISE; g = geq(C, u + w) (1 + noise N), C drawn from CONC or exactly 0.  Returns a dict:
    f [n, 9], and for the ade classes g [n, 9] and zero_c [n] (True where all nine g_q are 0)."""
    assert cls in ("bgk", "kbc", "ade_bgk", "ade_kbc"), cls
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    kind = i % CORNER_EVERY
    rho = rng.uniform(0.2, 5.0, n)
    mag, ang = 0.25 * rng.random(n), 2 * np.pi * rng.random(n)
    u = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    flip = (i // CORNER_EVERY) % 2 == 0
    axis = kind == 1
    u[axis & flip] = np.stack([sign * mag, 0 * mag], axis=1)[axis & flip]       # on the row axis
    u[axis & ~flip] = np.stack([0 * mag, sign * mag], axis=1)[axis & ~flip]     # on the column axis
    diag = kind == 2
    u[diag, 0] = (sign * mag / np.sqrt(2.0))[diag]                              # |u| = mag <= 0.25 on the diagonal too
    u[diag, 1] = np.where(flip, u[:, 0], -u[:, 0])[diag]                        # us or ud exactly 0
    u[kind == 0] = 0.0
    noise = np.asarray(NOISE)[rng.integers(0, len(NOISE), n)]
    noise[kind == 0] = 0.0
    feq = _feq_product if cls.endswith("kbc") else _feq_bgk
    f = feq(rho, u) * (1 + noise[:, None] * rng.standard_normal((n, 9)))
    f[kind == 0] = (E9 * rho[:, None])[kind == 0]                               # u = 0 with f = w_q rho exactly
    # the noisy populations of an axis or diagonal node are mirrored, so that the node's own momentum -- not only the u
    # it was drawn from -- has j_c = 0, j_r = 0 or j_r = +-j_c exactly (the product-form feq is not bitwise symmetric)
    for mask, swaps in ((axis & flip, ((4, 2), (8, 5), (7, 6))),                # c_c -> -c_c: j_c = 0
                        (axis & ~flip, ((3, 1), (6, 5), (7, 8))),               # c_r -> -c_r: j_r = 0
                        (diag & flip, ((2, 1), (4, 3), (8, 6))),                # (r, c) -> (c, r): j_r = j_c, ud = 0
                        (diag & ~flip, ((4, 1), (3, 2), (7, 5)))):              # (r, c) -> (-c, -r): j_r = -j_c, us = 0
        for dst, src in swaps:
            f[mask, dst] = f[mask, src]
    pair = kind == 3
    f[pair, 3], f[pair, 4] = f[pair, 1], f[pair, 2]                             # jx, jy contain exact zeros
    out = dict(f=np.ascontiguousarray(f))
    if cls.startswith("ade"):
        conc = np.asarray(CONC)[rng.integers(0, len(CONC), n)]
        zero_c = i % ZERO_C_EVERY == ZERO_C_AT
        g = _feq_bgk(conc, u + np.asarray(w)) * (1 + noise[:, None] * rng.standard_normal((n, 9)))
        g[zero_c] = 0.0
        out.update(g=np.ascontiguousarray(g), zero_c=zero_c)
    return out


# ---- the classes: one parameter point of a call each ----------------------------------------------------------------------
S2_SHEAR = 1.0 / (0.5 + 3.0 * 1.70766666e-4)   # the shear layer's s2
OMEGA = (0.6, 1.0, 1.2, 1.999)                 # 1.0: keep = 0
S2 = (0.6, 1.6, S2_SHEAR, 2.0)
OMEGA_G = (0.6, 1.0, 1.7, 1.999)
DRIFT = ((0.0, 0.0), (3e-3, 3e-3))
N_NODES = 48 * 430                             # >= 20 000 and no multiple of 256

Case = collections.namedtuple("Case", "name cls fluid delta_form omega_g w seed")


def cases():
    """Every parameter value of every model at least once.  BGK: omega x delta_form; KBC: s2; fluid + scalar: per
    fluid and drift the four fluid parameters, each with one omega_g -- the pairing shifted by one between the two
    drifts, so that every omega_g meets two fluid parameters and both drifts (the halves are coupled through u alone,
    which does not depend on either rate)."""
    out, seed = [], 100
    for delta in (0, 1):
        for om in OMEGA:
            out.append(Case(f"bgk-omega{om}-delta{delta}", "bgk", om, delta, None, None, seed))
            seed += 1
    for s2 in S2:
        out.append(Case(f"kbc-s2_{s2:.6g}", "kbc", s2, 0, None, None, seed))
        seed += 1
    for cls, params in (("ade_bgk", OMEGA), ("ade_kbc", S2)):
        for k, w in enumerate(DRIFT):
            for j, p in enumerate(params):
                og = OMEGA_G[(j + k) % 4]
                out.append(Case(f"{cls}-{p:.6g}-omega_g{og}-w{w[0]:g}", cls, p, 0, og, w, seed))
                seed += 1
    return out


@functools.lru_cache(maxsize=None)
def case_data(case, n=N_NODES):
    """(states, Exact) of a case, computed once per process and shared; treat both as read-only"""
    st = states(case.cls, n, case.seed, case.w or (0.0, 0.0))
    fluid = kbc(st["f"], case.fluid) if case.cls.endswith("kbc") else bgk(st["f"], case.fluid)
    exact = with_scalar(fluid, st["g"], case.omega_g, case.w) if case.cls.startswith("ade") else fluid
    for a in list(st.values()) + list(exact):
        a.setflags(write=False)
    return st, exact


def measure(pop, mom, exact, keep=None):
    """(stats of the populations, stats of the moments) of double results pop [n, 9 or 18], mom [n, 3 or 4] over the
    nodes keep (a mask; None: all of them)"""
    ep, em = errors(pop, exact.pop, exact.pop_unit), errors(mom, exact.mom, exact.mom_unit)
    if keep is not None:
        ep, em = ep[keep], em[keep]
    return stats(ep), stats(em)


def fmt(st):
    return "%7.2f / %7.2f / %7.2f" % st


def write_section(path, heading, lines):
    """replace (or add) the section `heading` of the report at path; sections start with '## '"""
    try:
        with open(path) as fh:
            text = fh.read()
    except OSError:
        text = ("Rounding error of the collisions against 80-bit arithmetic (tests/exact_collide.py), per node the worst\n"
                "output, in units (the spacing of doubles at the update's largest term): median / 99 % / maximum over nodes.\n"
                "pop: f* (and g*); mom: rho, u (and C).\n")
    parts = text.split("\n## ")
    body = "\n".join(lines) + "\n"
    for k in range(1, len(parts)):
        if parts[k].split("\n", 1)[0].strip() == heading:
            parts[k] = heading + "\n" + body
            break
    else:
        parts.append(heading + "\n" + body)
    parts[0] = parts[0].rstrip("\n") + "\n"
    with open(path, "w") as fh:
        fh.write("\n## ".join(p.rstrip("\n") + "\n" for p in parts))
