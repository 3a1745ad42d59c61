"""GPU suite: the device-side diagnostics (DESIGN.md "Diagnostics") -- lbm_diag_rows / lbm_diag_fold, the two
solver contexts' diag and run_until, and the Poiseuille driver's --device-check path -- pinned BITWISE to the
independent numpy restatement of the summation order in tests/diag_reference.py (nothing there calls the library)."""
import functools

import numpy as np
import pytest
import torch

import ade_util as ade
import diag_reference as ref
import pylbm
from gpu_util import dev
from proc_util import key_values, run_driver
from pylbm import _ptr

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF8DEADBEEF5A5A  # a quiet NaN no kernel computes: "never written"
ROWS = (1, 2, 63, 65, 200)      # fewer rows than a workgroup takes, one short of / one past the accumulator count, many
COLS = (1, 2, 63, 64, 65, 130)  # straddle the lane count, ragged last slice, more than one slice


@pytest.fixture(scope="module")
def lib():
    lib = pylbm.Lib()
    assert lib.device_count() >= 1
    lib.reset_tuning()
    return lib


# ---- fields and their reference (computed once per shape, never modified) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def fields(R, C):
    """rho, ur, uc, conc [R, C] and profile [C]: mixed signs, magnitudes over three decades (the order of the additions
    visibly matters), no exact zeros"""
    rng = np.random.default_rng(1000 * R + C)
    mag = lambda: 10.0 ** rng.uniform(-3.0, 0.0, (R, C))
    rho = 1.0 + 0.3 * rng.standard_normal((R, C)) * mag()
    ur, uc = (0.1 * rng.standard_normal((R, C)) * mag() for _ in range(2))
    conc = rng.standard_normal((R, C)) * mag()
    profile = 0.05 * rng.standard_normal(C)
    for a in (rho, ur, uc, conc, profile):
        a.setflags(write=False)
    return rho, ur, uc, conc, profile


@functools.lru_cache(maxsize=None)
def reference(R, C, with_conc, with_profile):
    rho, ur, uc, conc, profile = fields(R, C)
    t = ref.row_table(rho, ur, uc, conc if with_conc else None, profile if with_profile else None)
    t.setflags(write=False)
    return t


def up(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, device=dev())   # (a copy: the cached fields are read-only)


def poisoned_table(rows):
    t = torch.zeros((ref.NQ, rows), dtype=torch.float64, device=dev())
    t.view(torch.int64).fill_(SENTINEL)
    return t


def device_rows(lib, table, row0, rho, ur, uc, conc, profile, row_begin, row_end):
    """one lbm_diag_rows call on host fields [R, C] into the device table given"""
    R, C = rho.shape
    d = [up(rho), up(np.stack([ur, uc])), up(conc) if conc is not None else None, up(profile) if profile is not None else None]
    lib.diag_rows(_ptr(table), table.shape[1], row0, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), R, C, row_begin, row_end, None)
    torch.cuda.synchronize()


def device_fold(lib, table, row_begin, row_end):
    out = poisoned_table(1).reshape(-1)
    lib.diag_fold(_ptr(out), _ptr(table), table.shape[1], row_begin, row_end, None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def written(table):
    """mask [NQ, rows] of the doubles that are no longer the sentinel"""
    return (table.view(torch.int64) != SENTINEL).cpu().numpy()


def slot_names(got, want):
    g, w = (np.ascontiguousarray(x).view(np.uint64) for x in (got, want))
    return [pylbm.DIAG_NAMES[q] for q in range(ref.NQ) if not np.array_equal(g[q], w[q])]


def check_rows_and_fold(lib, R, C, with_conc, with_profile, row_begin, row_end, what):
    rho, ur, uc, conc, profile = fields(R, C)
    want = reference(R, C, with_conc, with_profile)
    table = poisoned_table(R)
    device_rows(lib, table, 0, rho, ur, uc, conc if with_conc else None, profile if with_profile else None, row_begin, row_end)
    mask = written(table)
    assert mask[:, row_begin:row_end].all() and mask.sum() == ref.NQ * (row_end - row_begin), f"{what}: write set"
    got = table.cpu().numpy()[:, row_begin:row_end]
    assert ref.bits_equal(got, want[:, row_begin:row_end]), f"{what}: rows differ in {slot_names(got, want[:, row_begin:row_end])}"
    folded = device_fold(lib, table, row_begin, row_end)
    want_f = ref.fold_table(want, row_begin, row_end)
    assert ref.bits_equal(folded, want_f), f"{what}: fold differs in {slot_names(folded[:, None], want_f[:, None])}"
    if not with_conc:
        assert not got[ref.SUM_C:ref.SUM_C2 + 1].any()
    if not with_profile:
        assert not got[ref.SUM_DEV2].any()
    return got, folded


def sub_ranges(R):
    return sorted({(0, R), (R // 3, R - R // 4), (R - 1, R), (min(1, R - 1), R)} - {(0, 0)})


@pytest.mark.parametrize("C", COLS)
@pytest.mark.parametrize("R", ROWS)
def test_rows_and_fold_equal_the_numpy_restatement_bitwise(lib, R, C):
    for with_conc in (False, True):
        for with_profile in (False, True):
            for a, b in sub_ranges(R):
                if a < b:
                    check_rows_and_fold(lib, R, C, with_conc, with_profile, a, b,
                                        f"{R}x{C} conc={with_conc} profile={with_profile} rows [{a}, {b})")


def test_the_order_of_the_additions_matters_on_these_fields():
    """otherwise the bitwise comparisons of this file would pass for any summation order"""
    rho, ur, uc, conc, _ = fields(200, 130)
    t = reference(200, 130, True, False)
    assert np.sum(rho * ur) != ref.fold_table(t)[ref.SUM_MR] or np.sum(conc) != ref.fold_table(t)[ref.SUM_C]
    assert any(np.sum(ur[r]) != t[ref.SUM_UR, r] for r in range(200))


@pytest.mark.parametrize("R,C", [(200, 130), (65, 64), (2, 1)])
def test_grid_cap_does_not_enter_the_value(lib, R, C):
    try:
        out = []
        for cap in (1, 7, -1):
            lib.set_tuning(b"grid_cap", cap)
            out.append(check_rows_and_fold(lib, R, C, True, True, 0, R, f"{R}x{C} grid_cap={cap}"))
        for rows, folded in out[1:]:
            assert ref.bits_equal(rows, out[0][0]) and ref.bits_equal(folded, out[0][1])
    finally:
        lib.set_tuning(b"grid_cap", -1)


@pytest.mark.parametrize("R,C,row0,rows,rb,re", [(65, 130, 7, 80, 3, 64), (2, 63, 0, 2, 1, 2), (63, 65, 137, 200, 0, 63)])
def test_write_set_is_the_row_range_of_the_17_planes(lib, R, C, row0, rows, rb, re):
    rho, ur, uc, conc, profile = fields(R, C)
    table = poisoned_table(rows)
    device_rows(lib, table, row0, rho, ur, uc, conc, profile, rb, re)
    expect = np.zeros((ref.NQ, rows), dtype=bool)
    expect[:, row0 + rb:row0 + re] = True
    assert np.array_equal(written(table), expect)
    assert ref.bits_equal(table.cpu().numpy()[:, row0 + rb:row0 + re], reference(R, C, True, True)[:, rb:re])


@pytest.mark.parametrize("heights", [(200,), (100, 100), (1, 64, 135), (37, 63, 100)])
def test_slabs_fill_one_table_and_fold_to_the_bits_of_one_block(lib, heights):
    R, C = 200, 130
    rho, ur, uc, conc, profile = fields(R, C)
    want = reference(R, C, True, True)
    table = poisoned_table(R)
    r0 = 0
    for h in heights:   # each slab: its own dense fields, its own call, its rows of the global table
        s = slice(r0, r0 + h)
        device_rows(lib, table, r0, rho[s], ur[s], uc[s], conc[s], profile, 0, h)
        r0 += h
    assert r0 == R and written(table).all()
    assert ref.bits_equal(table.cpu().numpy(), want)
    assert ref.bits_equal(device_fold(lib, table, 0, R), ref.fold_table(want))
    # the host fold of the gathered table: what a ring host computes
    assert ref.bits_equal(lib.diag_fold_host(table.cpu().numpy()), ref.fold_table(want))


@pytest.mark.parametrize("with_conc", [False, True])
def test_planted_non_finite_values_are_counted_and_stay_in_their_rows(lib, with_conc):
    R, C = 200, 130
    rho, ur, uc, conc, profile = (a.copy() for a in fields(R, C))
    nan, inf = float("nan"), float("inf")
    # planted from the host; (20, 7) carries two bad fields and counts once
    rho[3, 5], ur[10, 64], uc[10, 70], rho[199, 129], ur[20, 7], uc[20, 7] = nan, inf, -inf, inf, nan, -inf
    nodes = {(3, 5), (10, 64), (10, 70), (199, 129), (20, 7)}
    conc[150, 0], conc[150, 129], conc[63, 63], conc[20, 7] = nan, -inf, inf, inf
    if with_conc:
        nodes |= {(150, 0), (150, 129), (63, 63)}
    table = poisoned_table(R)
    device_rows(lib, table, 0, rho, ur, uc, conc if with_conc else None, profile, 0, R)
    got = table.cpu().numpy()
    per_row = np.zeros(R)
    for r, _ in nodes:
        per_row[r] += 1.0
    assert np.array_equal(got[ref.NONFINITE], per_row)
    assert device_fold(lib, table, 0, R)[ref.NONFINITE] == len(nodes)
    assert device_fold(lib, table, 11, 150)[ref.NONFINITE] == sum(11 <= r < 150 for r, _ in nodes)
    clean = np.array([r not in {n[0] for n in nodes} for r in range(R)])
    assert ref.bits_equal(got[:, clean], reference(R, C, with_conc, True)[:, clean])


# ---- the solver contexts --------------------------------------------------------------------------------------------
def moments_table(rho, u, conc=None, profile=None):
    return ref.row_table(rho, np.ascontiguousarray(u[..., 0]), np.ascontiguousarray(u[..., 1]), conc, profile)


def check_solver_diag(sv, want, profile_dev, what):
    R = want.shape[1]
    for a, b in ((0, R), (R // 3, R - R // 4)):
        got, table = sv.diag(profile=profile_dev, row_begin=a, row_end=b, table=True)
        want_f = ref.fold_table(want, a, b)
        assert ref.bits_equal(got, want_f), f"{what} rows [{a}, {b}): {slot_names(got[:, None], want_f[:, None])}"
        assert ref.bits_equal(table[:, a:b], want[:, a:b]), f"{what} rows [{a}, {b}): table"
        assert not table[:, :a].any() and not table[:, b:].any()
        assert ref.bits_equal(sv.diag(profile=profile_dev, row_begin=a, row_end=b), want_f)


@pytest.mark.parametrize("model", ["bgk", "kbc"])
def test_solver_diag_equals_the_fold_of_moments(lib, oracle, model):
    R, C = 37, 70
    rng = np.random.default_rng(5)
    f0 = oracle.equilibrium(0.05 * rng.standard_normal((R, C, 2)), 1 + 0.01 * rng.standard_normal((R, C)))
    if model == "bgk":
        sv = pylbm.Solver(lib, pylbm.MODEL_BGK, R, C, pylbm.BgkParams(1.2, 0))
    else:
        sv = pylbm.Solver(lib, pylbm.MODEL_KBC, R, C, pylbm.KbcParams(1.0 / (0.5 + 3.0 * 1.70766666e-4)))
    try:
        sv.set_f(f0)
        with pytest.raises(pylbm.LbmError, match=r"lbm_solver_diag: no step\(.., record_moments=1\) since the last set_f"):
            sv.diag()
        profile = 0.05 * rng.standard_normal(C)
        pd = up(profile)
        for n in (1, 7):
            sv.step(n, record_moments=True)
            rho, u = sv.moments()
            check_solver_diag(sv, moments_table(rho, u, None, profile), pd, f"{model} after {n} more steps")
        rho, u = sv.moments()
        got = sv.diag()
        assert not got[ref.SUM_C:].any()      # no conc, no profile
        assert got[ref.NONFINITE] == 0.0 and got[ref.SUM_RHO] == ref.fold_table(moments_table(rho, u))[ref.SUM_RHO]
    finally:
        sv.close()


ADE_CASES = {
    "periodic": dict(bc=None, sbc=None, by=None),
    "walled_fixed": dict(bc=pylbm.Bc(row_lo=ade.BB, row_hi=ade.BB, col_lo=ade.BB, col_hi=ade.BB), sbc=dict(row_lo=1e-3, col_hi=0.0), by=None),
    "buoyant": dict(bc=pylbm.Bc(row_lo=ade.BB, row_hi=ade.BB), sbc=None, by=((2e-3, -1.5e-3), 0.4)),
}


@pytest.mark.parametrize("case", sorted(ADE_CASES))
def test_ade_solver_diag_equals_the_fold_of_get_state(lib, oracle, case):
    R, C = 40, 70
    k = ADE_CASES[case]
    buoyant = k["by"] is not None
    f0, g0 = (ade.buoyant_initial_state if buoyant else ade.initial_state)(oracle, R, C, 3)
    fluid, scalar = ade.params(pylbm.FORM_DEFAULT)
    sv = pylbm.AdeSolver(lib, R, C, fluid, scalar, bc=k["bc"], scalar_bc=pylbm.AdeScalarBC(**k["sbc"]) if k["sbc"] else None,
                         buoyancy=ade.buoyancy(*k["by"], ade.REFERENCE) if buoyant else None)
    try:
        sv.set_state(f0, g0)
        profile = 0.01 * np.random.default_rng(9).standard_normal(C)
        pd = up(profile)
        for n in (0, 1, 12):      # the state as given, after the collide-only iteration, after fused steps
            sv.step(n)
            s = sv.get_state()
            check_solver_diag(sv, moments_table(s["rho"], s["u"], s["C"], profile), pd, f"{case} after {n} more steps")
            again = sv.get_state()  # the reduction left the state alone
            assert all(ref.bits_equal(s[key], again[key]) for key in s)
    finally:
        sv.close()


def test_periodic_passive_scalar_keeps_its_mean_to_rounding(lib, oracle):
    """SUM_C / (R C) after 50 steps against its initial value, to 1e-13 relative: mass conservation of a periodic BGK
    scalar up to rounding.  A step rounds each population a handful of times at relative 2^-53 = 1.1e-16; were all of
    them aligned over 50 steps the mean would move by 50 * O(10) * 1.1e-16 = 5e-14, and over 4096 nodes they are not
    aligned.  The achieved figure is printed."""
    R = C = 64
    f0, g0 = ade.initial_state(oracle, R, C, 1)
    fluid, scalar = ade.params(pylbm.FORM_DEFAULT)
    sv = pylbm.AdeSolver(lib, R, C, fluid, scalar)
    try:
        sv.set_state(f0, g0)
        before = sv.diag()[ref.SUM_C] / (R * C)
        sv.step(50)
        after = sv.diag()[ref.SUM_C] / (R * C)
    finally:
        sv.close()
    rel = abs(after / before - 1.0)
    print(f"periodic passive scalar, {R}x{C}, 50 steps: mean C {before:.17g} -> {after:.17g}, relative change {rel:.3e}")
    assert before > 0 and rel <= 1e-13


# ---- run_until: the 21 x 21 Poiseuille case of the reference driver -----------------------------------------------------
H = W = 21
T_DRIVER = 8301            # the driver's default T (horizontal_poiseuille_test.cpp)
RULE = dict(quantity=pylbm.DIAG_SUM_UR, interval=100, offset=1, tolerance=1e-12, old_value=1.0)
WEIGHTS = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)


def poiseuille_solver(lib):
    tau = np.sqrt(3.0 / 16.0) + 0.5
    u_max = 1.030985714E-1
    nu = (2.0 * tau - 1.0) / 6.0
    p_grad = 8.0 * nu * u_max / (W * W)
    bc = pylbm.Bc(col_lo=pylbm.EDGE_BOUNCE_BACK, col_hi=pylbm.EDGE_BOUNCE_BACK, pressure_rows=1,
                  rho_inlet=3.0 * (H - 1) * p_grad + 1.0, rho_outlet=1.0)
    sv = pylbm.Solver(lib, pylbm.MODEL_BGK, H, W, pylbm.BgkParams(1.0 / tau, 1), bc=bc)
    sv.set_f(np.broadcast_to(WEIGHTS, (H, W, 9)))   # incomp_equilibrium(u = 0, rho = 1)
    return sv


def host_loop(sv, max_steps):
    """the rule applied in Python to the numpy fold of moments() from 100-step calls: the driver's loop (:66-79) with the
    sum in the diagnostics' order"""
    t, old, last, converged = 0, RULE["old_value"], RULE["old_value"], False
    while t < max_steps:
        if t % RULE["interval"] == RULE["offset"]:
            rho, u = sv.moments()
            last = ref.fold_table(moments_table(rho, u))[ref.SUM_UR] / (float(H) * W)
            with np.errstate(divide="ignore", invalid="ignore"):   # old = 0.0 after the first check: inf, as in the C loop
                if abs(last / old - 1.0) < RULE["tolerance"]:
                    converged = True
                    break
            old = last
        nxt = 1 if t == 0 else t + RULE["interval"]
        n = min(nxt, max_steps) - t
        sv.step(n, record_moments=True)
        t += n
    return t, converged, last


def driver(*args):
    """the key=value lines of horizontal_poiseuille_test; it ran to exit 0"""
    return key_values(run_driver("horizontal_poiseuille_test", *args, timeout=300))


@pytest.fixture(scope="module")
def poiseuille_runs(lib):
    """run once, shared: run_until and the Python loop on fresh solvers, generous max_steps"""
    max_steps = 40000
    sv = poiseuille_solver(lib)
    try:
        device = sv.run_until(pylbm.Converge(**RULE), max_steps)
        device_state = sv.moments()
    finally:
        sv.close()
    sv = poiseuille_solver(lib)
    try:
        host = host_loop(sv, max_steps)
        host_state = sv.moments()
    finally:
        sv.close()
    return device, host, device_state, host_state


def test_run_until_equals_the_python_loop_bitwise(poiseuille_runs):
    device, host, device_state, host_state = poiseuille_runs
    print(f"run_until: steps_done={device[0]} converged={device[1]} last_value={device[2]!r}; python loop: {host}")
    assert device[0] == host[0] and device[1] == host[1]
    assert np.float64(device[2]).view(np.uint64) == np.float64(host[2]).view(np.uint64)
    assert device[1] is True                       # converged == 1
    assert device[0] % 100 == 1 and device[0] < 40000
    assert all(ref.bits_equal(a, b) for a, b in zip(device_state, host_state))


def test_run_until_stops_where_the_existing_driver_stops(poiseuille_runs):
    """the driver's own loop sums row-major on the host; run_until sums in the diagnostics' order.  Both numbers are
    printed; they must agree -- with the driver's default T as with a T beyond the stopping step."""
    device = poiseuille_runs[0]
    out = driver("--T", 40000)
    print(f"driver --T 40000: steps={out['steps']}; run_until(max_steps=40000): steps_done={device[0]}")
    assert int(out["steps"]) == device[0]
    out = driver()
    assert int(out["steps"]) == min(T_DRIVER, device[0])


def test_run_until_ends_at_max_steps_below_the_stopping_step(lib, poiseuille_runs):
    stop = poiseuille_runs[0][0]
    for max_steps in (250, 301, 1):
        assert max_steps < stop
        sv = poiseuille_solver(lib)
        try:
            got = sv.run_until(pylbm.Converge(**RULE), max_steps)
        finally:
            sv.close()
        sv = poiseuille_solver(lib)
        try:
            want = host_loop(sv, max_steps)
        finally:
            sv.close()
        assert got[0] == max_steps == want[0] and got[1] is False and want[1] is False
        assert np.float64(got[2]).view(np.uint64) == np.float64(want[2]).view(np.uint64)


def test_ade_run_until_applies_the_same_rule(lib, oracle):
    """the fluid + scalar context: the watched value is the mean of C over a row range of the streamed state"""
    R, C = 24, 70
    f0, g0 = ade.initial_state(oracle, R, C, 2)
    fluid, scalar = ade.params(pylbm.FORM_DEFAULT)
    rule = dict(quantity=pylbm.DIAG_SUM_C, interval=10, offset=3, tolerance=1e-9, old_value=1.0, row_begin=2, row_end=20)

    def make():
        sv = pylbm.AdeSolver(lib, R, C, fluid, scalar, bc=pylbm.Bc(row_lo=ade.BB, row_hi=ade.BB))
        sv.set_state(f0, g0)
        return sv

    sv = make()
    try:
        got = sv.run_until(pylbm.Converge(**rule), 47)
    finally:
        sv.close()
    sv = make()
    try:
        t, old, last, conv = 0, 1.0, 1.0, False
        while t < 47:
            if t > 0 and t % 10 == 3:
                s = sv.get_state()
                last = ref.fold_table(moments_table(s["rho"], s["u"], s["C"]), 2, 20)[ref.SUM_C] / (18.0 * C)
                if abs(last / old - 1.0) < 1e-9:
                    conv = True
                    break
                old = last
            n = min(t - t % 10 + 3 + (10 if t % 10 >= 3 else 0), 47) - t
            sv.step(n)
            t += n
    finally:
        sv.close()
    assert got[0] == t and got[1] == conv and np.float64(got[2]).view(np.uint64) == np.float64(last).view(np.uint64)


def test_driver_with_device_check_prints_the_reference_assertion():
    out = driver("--device-check", 1)                                  # exit 0: the driver's own L2 <= 1e-11 check passed
    out0 = driver()
    print(f"--device-check 1: steps={out['steps']} L2={out['L2']}; default: steps={out0['steps']} L2={out0['L2']}")
    assert float(out["L2"]) <= 1e-11                                   # horizontal_poiseuille_test.cpp:172
    assert out["steps"] == out0["steps"]
