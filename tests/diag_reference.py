"""Independent numpy restatement of the diagnostics' summation order (DESIGN.md "Diagnostics"), shared by
test_diag_abi.py and test_gpu_diag.py.  Nothing here calls the library.

fold64(x[0..n)): 64 accumulators p[j] = +0.0, p[j] += x[j + 64 k] for k ascending (missing elements add nothing), then
p[j] += p[j + s] (j < s) for s = 32 .. 1; the value is p[0].  Here: K = ceil(n / 64) slices of a padded copy, then six
halvings.  An accumulator that starts at +0.0 never becomes -0.0, so zero padding is exact."""
import numpy as np

NQ = 17
(SUM_RHO, SUM_UR, SUM_UC, SUM_MR, SUM_MC, SUM_KE, MAX_U2, MIN_RHO, MAX_RHO, NONFINITE,
 SUM_C, SUM_CUR, SUM_CUC, MIN_C, MAX_C, SUM_C2, SUM_DEV2) = range(NQ)
OPS = {q: "add" for q in range(NQ)}
OPS.update({MAX_U2: "max", MIN_RHO: "min", MAX_RHO: "max", MIN_C: "min", MAX_C: "max"})
_FN = {"add": np.add, "min": np.fmin, "max": np.fmax}          # fmin / fmax skip NaN operands
_IDENT = {"add": 0.0, "min": np.inf, "max": -np.inf}


def fold64(x, op="add"):
    """fold64 along the last axis of x ([n] -> scalar, [N, n] -> [N])"""
    x = np.asarray(x, dtype=np.float64)
    f, ident = _FN[op], _IDENT[op]
    n = x.shape[-1]
    K = -(-n // 64)
    pad = np.full(x.shape[:-1] + (64 * K,), ident)
    pad[..., :n] = x
    p = np.full(x.shape[:-1] + (64,), ident)
    for k in range(K):
        p = f(p, pad[..., 64 * k:64 * k + 64])
    for s in (32, 16, 8, 4, 2, 1):
        p = f(p[..., :s], p[..., s:2 * s])
    return p[..., 0]


def row_table(rho, ur, uc, conc=None, profile=None):
    """the row values [NQ, R] of dense fields [R, C]: the per-node terms exactly as the quantity table writes them"""
    R = rho.shape[0]
    t = np.zeros((NQ, R))
    with np.errstate(all="ignore"):
        u2 = ur * ur + uc * uc
        t[SUM_RHO] = fold64(rho)
        t[SUM_UR] = fold64(ur)
        t[SUM_UC] = fold64(uc)
        t[SUM_MR] = fold64(rho * ur)
        t[SUM_MC] = fold64(rho * uc)
        t[SUM_KE] = fold64(0.5 * (rho * u2))
        t[MAX_U2] = fold64(u2, "max")
        t[MIN_RHO] = fold64(rho, "min")
        t[MAX_RHO] = fold64(rho, "max")
        bad = ~np.isfinite(rho) | ~np.isfinite(ur) | ~np.isfinite(uc)
        if conc is not None:
            bad |= ~np.isfinite(conc)
            t[SUM_C] = fold64(conc)
            t[SUM_CUR] = fold64(conc * ur)
            t[SUM_CUC] = fold64(conc * uc)
            t[MIN_C] = fold64(conc, "min")
            t[MAX_C] = fold64(conc, "max")
            t[SUM_C2] = fold64(conc * conc)
        t[NONFINITE] = fold64(bad.astype(np.float64))
        if profile is not None:
            d = ur - profile[None, :]
            t[SUM_DEV2] = fold64(d * d)
    return t


def fold_table(table, row_begin=0, row_end=None):
    """rows [row_begin, row_end) of a row table [NQ, rows] -> the NQ values"""
    table = np.asarray(table)
    row_end = table.shape[1] if row_end is None else row_end
    with np.errstate(all="ignore"):
        return np.array([fold64(table[q, row_begin:row_end], OPS[q]) for q in range(NQ)])


def bits_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
