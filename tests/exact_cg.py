"""The 80-bit yardstick of the colour-gradient two-phase step: one unit of work of the GPU step -- stream + boundaries,
moments, phase field, stencils, MRT, perturbation, recolouring, source (test/mrtcg_rayleigh_taylor.cpp:431-477 rotated
to start at the post-collision populations) -- on a whole lattice in vectorised np.longdouble, the units in which a double
result is judged against it, and the edge-state lattices on which tests/test_exact_cg.py (CPU oracle) and
tests/test_gpu_cg_accuracy.py (both GPU forms) measure.  The companion of tests/exact_collide.py, whose helpers it uses.

Nothing here calls the library under test, the oracle or oracle/torch_restatement.py: every value comes from numpy and
the formulas.  Every constant of the model (weights, M, 36 M^-1, B_q, xi / 5040, 1.25, 1.14, 1.6, 1.8, 0.8, 1e-20 ...) is
formed in long double from integers; the parameters of a case (rho_0, alpha, nu, beta, sigma, Fg, delta) are doubles and
convert exactly, as the populations do.

The yardstick's own error: about 400 long-double operations reach a population, none of them a cancellation the double
forms do not share, so it is within ~400 x 2^-64 ~ 2e-17 relative of the exact value: below 0.1 unit.

Units (the spacing of doubles at the largest term of the output's own update):
  pn_{k,q}   the largest of the streamed f_{k,q}, the colour's MRT term, the perturbation term, tot_q, rho_k tot_q / rho,
             beta_k kappa_q and F_q;
  rho_k      sum_q |f_{k,q}|;
  u          (sum_q |c_q (f_r + f_b)_q|) / |rho| per component, the larger used for both (exact_collide._moments);
  psi        max(rho_r / rho_0r, rho_b / rho_0b) / (rho_r / rho_0r + rho_b / rho_0b);
  s_nu       the largest term of the branch's polynomial (the rate itself on the two constant branches).

Ill-conditioned nodes.  n = grad psi / (1e-20 + |grad psi|) is noise in every form where the stencil sum cancels.  A node
is marked where both hold: rho_r rho_b != 0, and |grad psi| < 2^-30 sum_ij |xi_ij psi_ij| (xi = the 5 x 5 weights / 5040
over the node's replicate-padded window).  Marked nodes are left out of the population statistics only; at most CAP of a
lattice's nodes may be marked (asserted on every case by tests/test_exact_cg.py)."""
import collections
import functools

import numpy as np

from exact_collide import CX, CY, LD, _ld, _spacing, errors, fmt, stats, write_section  # noqa: F401  (re-exported)

_ONE = LD(1)
_W = [LD(4) / 9] + [_ONE / 9] * 4 + [_ONE / 36] * 4
_B = [-LD(4) / 27] + [LD(2) / 27] * 4 + [LD(5) / 108] * 4
_M = ((1, 1, 1, 1, 1, 1, 1, 1, 1), (-4, -1, -1, -1, -1, 2, 2, 2, 2), (4, -2, -2, -2, -2, 1, 1, 1, 1),
      (0, 1, 0, -1, 0, 1, -1, -1, 1), (0, -2, 0, 2, 0, 1, -1, -1, 1), (0, 0, 1, 0, -1, 1, 1, -1, -1),
      (0, 0, -2, 0, 2, 1, 1, -1, -1), (0, 1, -1, 1, -1, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1, -1, 1, -1))
_MI36 = ((4, -4, 4, 0, 0, 0, 0, 0, 0), (4, -1, -2, 6, -6, 0, 0, 9, 0), (4, -1, -2, 0, 0, 6, -6, -9, 0),
         (4, -1, -2, -6, 6, 0, 0, 9, 0), (4, -1, -2, 0, 0, -6, 6, -9, 0), (4, 2, 1, 6, 3, 6, 3, 0, 9),
         (4, 2, 1, -6, -3, 6, 3, 0, -9), (4, 2, 1, -6, -3, -6, -3, 0, 9), (4, 2, 1, 6, 3, -6, -3, 0, -9))
_XI = ((1, 32, 84, 32, 1), (32, 448, 960, 448, 32), (84, 960, 0, 960, 84), (32, 448, 960, 448, 32), (1, 32, 84, 32, 1))
_EPS = _ONE / LD(10) ** 20
_SQRT2 = np.sqrt(LD(2))
_S_FIXED = (LD(0), LD(5) / 4, LD(114) / 100, LD(0), LD(8) / 5, LD(0), LD(8) / 5)   # S_0 .. S_6; S_7 = S_8 = s_nu
assert np.all(np.array(_M, dtype=np.int64) @ np.array(_MI36, dtype=np.int64) == 36 * np.eye(9, dtype=np.int64))
ILL_SHIFT = 30
CAP = 0.01

Colour = collections.namedtuple("Colour", "rho_0 alpha nu beta")
Params = collections.namedtuple("Params", "name red blue sigma g_r g_c add_source delta")
# pop [R, C, 18]: pn_r then pn_b; mom [R, C, 4]: rho_r, rho_b, u_r, u_c; psi, s_nu [R, C, 1]; the units alike;
# f [R, C, 18] the streamed populations; ill [R, C] the mask of ill-conditioned nodes; parts: named intermediate terms
Exact = collections.namedtuple("Exact", "pop pop_unit mom mom_unit psi psi_unit s_nu s_nu_unit f ill parts")
CLASSES = ("pop", "mom", "psi", "s_nu")


# ---- the step ------------------------------------------------------------------------------------------------------------
def _colour_consts(k):
    alpha = LD(k.alpha)
    cs2 = 3 * (1 - alpha) / 5
    phi = [alpha] + [(1 - alpha) / 5] * 4 + [(1 - alpha) / 20] * 4
    eta = [1 + (3 * cs2 - 1) * (3 * (CX[q] * CX[q] + CY[q] * CY[q]) - 4) / 2 for q in range(9)]
    omega = 1 / (_ONE / 2 + LD(k.nu) / cs2)
    return alpha, phi, eta, omega


def _feq(rho_k, phi, eta, ux, uy):
    uu = ux * ux + uy * uy
    out = []
    for q in range(9):
        cu = ux * CX[q] + uy * CY[q]
        out.append(rho_k * (phi[q] + _W[q] * (3 * cu * eta[q] + 9 * cu * cu - 3 * uu)))
    return out


def stream(p):
    """advect (periodic pull) then the driver's boundary set: same-row column copies on rows 1 .. R - 2, then halfway
    bounce-back on rows 0 and R - 1 (the rows win the corners); p [R, C, 9] of any dtype"""
    f = np.stack([np.roll(p[..., q], (CX[q], CY[q]), axis=(0, 1)) for q in range(9)], axis=-1)
    for q in (2, 5, 6):
        f[1:-1, 0, q] = p[1:-1, -1, q]
    for q in (4, 8, 7):
        f[1:-1, -1, q] = p[1:-1, 0, q]
    for dst, src in ((3, 1), (7, 5), (6, 8)):
        f[-1, :, dst] = p[-1, :, src]
    for dst, src in ((1, 3), (5, 7), (8, 6)):
        f[0, :, dst] = p[0, :, src]
    return f


def _windows(a):
    """a [R, C] -> the 25 shifted copies of its replicate-padded 5 x 5 windows, [i][j] = a(r + i - 2, c + j - 2)"""
    R, C = a.shape
    pad = np.pad(a, 2, mode="edge")
    return [[pad[i:i + R, j:j + C] for j in range(5)] for i in range(5)]


def _diff(win, direction):
    return sum(win[i][j] * (LD(_XI[i][j]) / 5040 * ((i - 2) if direction == 0 else (j - 2)))
               for i in range(5) for j in range(5) if _XI[i][j] and ((i - 2) if direction == 0 else (j - 2)))


def relaxation(psi, om_r, om_b, delta):
    """the s_nu blend (:34-101) and the largest term of the branch taken"""
    s1 = 2 * om_r * om_b / (om_r + om_b)
    s2 = 2 * (om_r - s1) / delta
    s3 = -s2 / (2 * delta)
    t2 = 2 * (s1 - om_b) / delta
    t3 = t2 / (2 * delta)
    zero = psi * 0
    pos = s1 + s2 * psi + s3 * psi * psi
    neg = s1 + t2 * psi + t3 * psi * psi
    big_pos = np.maximum(np.maximum(abs(s1) + zero, np.abs(s2 * psi)), np.abs(s3 * psi * psi))
    big_neg = np.maximum(np.maximum(abs(s1) + zero, np.abs(t2 * psi)), np.abs(t3 * psi * psi))
    s_nu = np.where(psi > delta, om_r + zero, np.where(psi > 0, pos, np.where(psi >= -delta, neg, om_b + zero)))
    big = np.where(psi > delta, om_r + zero, np.where(psi > 0, big_pos, np.where(psi >= -delta, big_neg, om_b + zero)))
    return s_nu, big


def step(p_r, p_b, prm):
    """one step from the post-collision populations p_r, p_b [R, C, 9] (doubles) with the parameters prm; an Exact"""
    p = [_ld(p_r), _ld(p_b)]
    R, C = p[0].shape[:2]
    col = (prm.red, prm.blue)
    alpha, phi, eta, omega = zip(*[_colour_consts(k) for k in col])
    rho_0 = [LD(k.rho_0) for k in col]
    beta = [LD(k.beta) for k in col]
    sigma, g_r, g_c, delta = LD(prm.sigma), LD(prm.g_r), LD(prm.g_c), LD(prm.delta)
    f = [stream(a) for a in p]
    # moments, with the Fg / (2 rho) shift
    rk = [sum(a[..., q] for q in range(9)) for a in f]
    rho = rk[0] + rk[1]
    ft = f[0] + f[1]
    j_r = sum(ft[..., q] * CX[q] for q in range(1, 9))
    j_c = sum(ft[..., q] * CY[q] for q in range(1, 9))
    ux, uy = j_r / rho + g_r / 2 / rho, j_c / rho + g_c / 2 / rho
    a_r = sum(np.abs(f[0][..., q]) + np.abs(f[1][..., q]) for q in range(9) if CX[q])
    a_c = sum(np.abs(f[0][..., q]) + np.abs(f[1][..., q]) for q in range(9) if CY[q])
    unit_u = _spacing(np.maximum(a_r, a_c) / np.abs(rho))
    mom = np.stack([rk[0], rk[1], ux, uy], axis=-1)
    mom_unit = np.stack([_spacing(np.sum(np.abs(f[0]), axis=-1)), _spacing(np.sum(np.abs(f[1]), axis=-1)), unit_u, unit_u],
                        axis=-1)
    # phase field and relaxation blend
    na, nb = rk[0] / rho_0[0], rk[1] / rho_0[1]
    psi = (na - nb) / (na + nb)
    psi_unit = _spacing(np.maximum(np.abs(na), np.abs(nb)) / np.abs(na + nb))
    s_nu, s_big = relaxation(psi, omega[0], omega[1], delta)
    # stencils
    wpsi = _windows(psi)
    gx, gy = _diff(wpsi, 0), _diff(wpsi, 1)
    gnorm = np.sqrt(gx * gx + gy * gy)
    spread = sum(np.abs(wpsi[i][j]) * (LD(_XI[i][j]) / 5040) for i in range(5) for j in range(5))
    ill = ((rk[0] * rk[1]) != 0) & (gnorm < spread / LD(2) ** ILL_SHIFT)
    om1 = []
    for k in range(2):
        qf = LD(9) / 5 * alpha[k] - LD(4) / 5
        dxq = _diff(_windows(qf * rk[k] * ux), 0)
        dyq = _diff(_windows(qf * rk[k] * uy), 1)
        ck = {1: 3 * (1 - _S_FIXED[1] / 2) * (dxq + dyq), 7: (1 - s_nu / 2) * (dxq - dyq)}
        feq = _feq(rk[k], phi[k], eta[k], ux, uy)
        neq = [feq[q] - f[k][..., q] for q in range(9)]
        m = []
        for a in range(9):
            s_a = _S_FIXED[a] if a < 7 else s_nu
            m.append(s_a * sum(neq[q] * _M[a][q] for q in range(9) if _M[a][q]) + ck.get(a, 0))
        om1.append([sum(m[a] * (LD(_MI36[q][a]) / 36) for a in range(9) if _MI36[q][a]) for q in range(9)])
    # perturbation, recolouring, source
    amp = LD(9) / 2 * sigma * s_nu
    inv = 1 / (_EPS + gnorm)
    pop, unit, parts = [[], []], [[], []], collections.defaultdict(list)
    for q in range(9):
        g_e = gx * CX[q] + gy * CY[q]
        t1 = g_e * inv
        om2 = amp * (gnorm / 2 * (_W[q] * t1 * t1 - _B[q]))
        d = _ONE if q < 5 else _SQRT2
        g_u = gx * (CX[q] / d) + gy * (CY[q] / d)
        kappa = rk[0] * rk[1] * g_u * (rk[0] * phi[0][q] + rk[1] * phi[1][q]) / (rho * rho) * inv
        tot = f[0][..., q] + om1[0][q] + om2 + f[1][..., q] + om1[1][q] + om2
        cu = ux * CX[q] + uy * CY[q]
        fg_e = g_r * CX[q] + g_c * CY[q]
        src = (1 - s_nu / 2) * ((3 + 9 * cu) * fg_e - 3 * (ux * g_r + uy * g_c)) * _W[q]
        if not prm.add_source:
            src = src * 0
        for k in range(2):
            share = rk[k] * tot / rho
            out = share + beta[k] * kappa + src
            big = np.abs(f[k][..., q])
            for term in (om1[k][q], om2, tot, share, beta[k] * kappa, src):
                big = np.maximum(big, np.abs(term))
            pop[k].append(out)
            unit[k].append(_spacing(big))
        for name, v in (("om2", om2), ("kappa", kappa), ("tot", tot), ("src", src), ("om1_r", om1[0][q]), ("om1_b", om1[1][q])):
            parts[name].append(v)
    parts = {k: np.stack(v, axis=-1) for k, v in parts.items()}
    parts.update(gx=gx, gy=gy, rho=rho)
    return Exact(np.stack(pop[0] + pop[1], axis=-1), np.stack(unit[0] + unit[1], axis=-1), mom, mom_unit,
                 psi[..., None], psi_unit[..., None], s_nu[..., None], _spacing(s_big)[..., None],
                 np.concatenate(f, axis=-1), ill, parts)


# ---- the edge-state lattices -----------------------------------------------------------------------------------------------
LATTICES = {"37x45": (37, 45), "80x200": (80, 200)}
DROPLET = {"37x45": (18, 22), "80x200": (32, 96)}   # the lattice centre; the corner of four 16 x 64 tiles
RADIUS = 10.0
NOISE = (0.0, 1e-9, 1e-2, 0.1)                      # per quadrant: (top, left), (top, right), (bottom, left), (bottom, right)
MACH = 0.1
_RED, _BLUE = Colour(3.0, 0.7, 0.04, 0.7), Colour(1.0, 0.1, 0.04, -0.7)   # mrtcg-rayleigh-taylor-gamma3.toml


def cases():
    """the parameter points, each a Params"""
    return [
        Params("shipped-toml", _RED, _BLUE, 0.1, 6.25e-6, 0.0, 1, 0.1),
        Params("static-droplet", _RED, _BLUE, 0.1, 0.0, -6.25e-6, 0, 0.1),
        Params("equal-densities", Colour(1.0, 0.2, 0.04, 0.7), Colour(1.0, 0.2, 0.04, -0.7), 0.1, 6.25e-6, 0.0, 1, 0.1),
        Params("density-ratio-100", Colour(100.0, 0.991, 0.04, 0.7), _BLUE, 0.1, 6.25e-6, 0.0, 1, 0.1),
        Params("viscosity-ratio-10", Colour(3.0, 0.7, 0.05, 0.7), Colour(1.0, 0.1, 0.005, -0.7), 0.1, 6.25e-6, 0.0, 1, 0.1),
        Params("sigma0-delta0.02", _RED, _BLUE, 0.0, 6.25e-6, 0.0, 1, 0.02),
    ]


def _profile(d, width):
    """the fraction inside an interface at signed distance d (negative: inside): an exact step where width = 0, else
    (1 - tanh(d / width)) / 2, exactly 0 or 1 beyond four widths -- the bulk is exactly pure"""
    w = np.where(width > 0, width, 1.0)
    smooth = 0.5 * (1.0 - np.tanh(d / w))
    smooth = np.where(d > 4 * w, 0.0, np.where(d < -4 * w, 1.0, smooth))
    return np.where(width > 0, smooth, np.where(d < 0, 1.0, 0.0))


def composition(lattice):
    """the red fraction X [R, C] in [0, 1]: red above the driver's cosine interface (which meets both copy columns), the
    colours exchanged inside a droplet of radius 10 and inside a half disc of radius 7 on wall row 0; interface width by
    column band: exact step, tanh of width 1, tanh of width 3"""
    R, C = LATTICES[lattice]
    r, c = np.meshgrid(np.arange(R, dtype=float), np.arange(C, dtype=float), indexing="ij")
    width = np.where(c < C // 3, 0.0, np.where(c < 2 * (C // 3), 1.0, 3.0))
    x = _profile(r - (R / 2.0 - 0.1 * C * np.cos(2.0 * np.pi * c / C)), width)
    r0, c0 = DROPLET[lattice]
    for centre, radius in (((r0, c0), RADIUS), ((0, C // 4), 7.0)):
        inside = _profile(np.hypot(r - centre[0], c - centre[1]) - radius, width)
        x = x * (1.0 - inside) + (1.0 - x) * inside
    return x


def _feq_double(rho_k, k, u):
    cs2 = 3.0 * (1.0 - k.alpha) / 5.0
    phi = np.array([k.alpha] + [0.2 * (1.0 - k.alpha)] * 4 + [0.05 * (1.0 - k.alpha)] * 4)
    e2 = np.array([cx * cx + cy * cy for cx, cy in zip(CX, CY)], dtype=float)
    eta = 1.0 + 0.5 * (3.0 * cs2 - 1.0) * (3.0 * e2 - 4.0)
    w = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
    cu = u[..., :1] * np.array(CX, dtype=float) + u[..., 1:] * np.array(CY, dtype=float)
    uu = np.sum(u * u, axis=-1, keepdims=True)
    return rho_k[..., None] * (phi + w * (3.0 * cu * eta + 9.0 * cu * cu - 3.0 * uu))


def equilibrium(prm, lattice):
    """(feq_r, feq_b [R, C, 9], noise level [R, C]): cg_feq of rho_k = rho_0k x fraction x a density wave in [0.4, 1.6]
    and of a shear velocity up to Mach 0.1 -- the populations before the noise -- and the node's noise level.
    Every population is >= 0: where the shear would take a population of a colour that is present below a quarter of its
    value at rest (alpha_r = 0.991 leaves 0.0018 rho beside 0.5 u rho) the node's velocity is halved until it does not.
    The streamed densities are then sums of non-negative numbers and rho = rho_r + rho_b cannot cancel: where it does
    (a negative density, which no run reaches) u = j / rho is noise in every form, the reference order included."""
    R, C = LATTICES[lattice]
    r, c = np.meshgrid(np.arange(R, dtype=float), np.arange(C, dtype=float), indexing="ij")
    x = composition(lattice)
    wave = 1.0 + 0.6 * np.sin(2.0 * np.pi * (r / R + 2.0 * c / C))
    cs = 1.0 / np.sqrt(3.0)
    u = np.stack([0.3 * MACH * cs * np.cos(2.0 * np.pi * c / C), MACH * cs * np.sin(2.0 * np.pi * r / R)], axis=-1)
    level = np.asarray(NOISE)[2 * (r >= R // 2).astype(int) + (c >= C // 2).astype(int)]
    rho = (prm.red.rho_0 * x * wave, prm.blue.rho_0 * (1.0 - x) * wave)
    for _ in range(12):   # halve u where a colour that is present would get a negative population (see state)
        feq = [_feq_double(rho[k], col, u) for k, col in enumerate((prm.red, prm.blue))]
        low = np.zeros((R, C), dtype=bool)
        for k, col in enumerate((prm.red, prm.blue)):
            rest = _feq_double(rho[k], col, 0.0 * u)
            low |= np.any(feq[k] < 0.25 * rest, axis=-1)
        if not low.any():
            break
        u = np.where(low[..., None], 0.5 * u, u)
    assert not low.any()
    return feq[0], feq[1], level


def state(prm, lattice):
    """post-collision populations p_r, p_b [R, C, 9]: equilibrium() times (1 + level N) with the level of the node's
    quadrant and N mirrored (the same factor for c_q and -c_q, exact_collide.states), so that the noise adds no
    momentum of its own.  A colour that is absent has nine exact zeros."""
    R, C = LATTICES[lattice]
    seed = 7000 + 100 * [p.name for p in cases()].index(prm.name) + list(LATTICES).index(lattice)
    rng = np.random.default_rng(seed)
    x = composition(lattice)
    feq_r, feq_b, level = equilibrium(prm, lattice)
    out = []
    for feq, frac in ((feq_r, x), (feq_b, 1.0 - x)):
        half = np.clip(rng.standard_normal((R, C, 5)), -3.0, 3.0)           # rest, then one factor per pair of opposites
        n = half[..., [0, 1, 2, 1, 2, 3, 4, 3, 4]]
        p = feq * (1.0 + level[..., None] * n)
        p[frac == 0.0] = 0.0                                                # (rho_k (...) may be -0.0)
        out.append(np.ascontiguousarray(p))
    assert np.all(np.sum(out[0] + out[1], axis=-1) >= 0.2)
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def case_data(case, lattice):
    """((p_r, p_b), Exact) of a parameter point on a lattice, computed once per process and shared; read-only"""
    p_r, p_b = state(case, lattice)
    exact = step(p_r, p_b, case)
    for a in (p_r, p_b) + tuple(v for v in exact[:-1]) + tuple(exact.parts.values()):
        a.setflags(write=False)
    return (p_r, p_b), exact


def measure(got, exact):
    """got: dict of double results pop [R, C, 18], mom [R, C, 4], psi, s_nu [R, C]; per class (median, 99 %, maximum) of
    the per-node worst error in units -- the populations over the well-conditioned nodes only"""
    R, C = exact.ill.shape
    out = {}
    for cls in CLASSES:
        k = getattr(exact, cls).shape[-1]
        err = errors(np.asarray(got[cls]).reshape(R * C, k), getattr(exact, cls).reshape(R * C, k),
                     getattr(exact, cls + "_unit").reshape(R * C, k))
        out[cls] = stats(err[~exact.ill.reshape(-1)] if cls == "pop" else err)
    return out


def fmt_row(m):
    return "   ".join("%s %s" % (cls, fmt(m[cls])) for cls in CLASSES)


HEADER = ("Rounding error of the two-phase (colour-gradient) step against 80-bit arithmetic (tests/exact_cg.py), per node the\n"
          "worst output of its class, in units (the spacing of doubles at the update's largest term): median / 99 % / maximum\n"
          "over nodes.  pop: pn_r, pn_b (ill-conditioned nodes left out); mom: rho_r, rho_b, u; psi; s_nu.\n")


def write_report(path, heading, lines):
    try:
        open(path).close()
    except OSError:
        with open(path, "w") as fh:
            fh.write(HEADER)
    write_section(path, heading, lines)
