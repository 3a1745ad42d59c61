"""The oracle's reference-order collisions against the 80-bit yardstick (tests/exact_collide.py) on the edge states
of every class.  The bound here -- 256 units -- only guards against a transcription slip in the yardstick (a slip shows
at >= 1e6 units; rounding measures up to 55 units, profiles/collision_accuracy.txt); the bar of the reassociated GPU forms is the reference order's own error on the same nodes, tests/test_gpu_collision_accuracy.py.  The measured table goes to
profiles/collision_accuracy.txt."""
import os
from fractions import Fraction

import numpy as np
import pytest
from conftest import ROOT

import exact_collide as xc
from collide_reference import reference_order

REPORT = os.path.join(ROOT, "profiles", "collision_accuracy.txt")
CASES = xc.cases()
_rows = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if len(_rows) == len(CASES):   # a full run only
        lines = ["%-44s pop %s   mom %s" % (c.name, xc.fmt(_rows[c.name][0]), xc.fmt(_rows[c.name][1])) for c in CASES]
        try:
            xc.write_section(REPORT, "CPU, reference order", [f"{xc.N_NODES} nodes per class"] + lines)
        except OSError:
            pass                   # a read-only tree: the assertions above are the test


def test_yardstick_needs_extended_precision():
    assert np.finfo(xc.LD).nmant >= 63


def exact_momentum(f):
    """(j_r, j_c) of the nodes f [n, 9] in exact rational arithmetic"""
    out = []
    for node in f:
        q = [Fraction(float(v)) for v in node]
        out.append((sum(q[k] * xc.CX[k] for k in range(9)), sum(q[k] * xc.CY[k] for k in range(9))))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_states_hold_every_corner_case(case):
    """each exact corner case on 2 % of the nodes of every class, by node index, and in the first 42 nodes (the 7 x 6
    lattice); exact means exact in the node's own populations: the momentum in rational arithmetic"""
    st, _ = xc.case_data(case)
    f = st["f"]
    n = len(f)
    assert n >= 20000 and all(np.all(np.isfinite(a)) for a in st.values())
    kind, flip = np.arange(n) % xc.CORNER_EVERY, (np.arange(n) // xc.CORNER_EVERY) % 2 == 0
    for k in range(4):
        assert 0.019 * n <= np.sum(kind == k) <= 0.021 * n and np.any(kind[:42] == k)
    rest = f[kind == 0]                               # u = 0 with f = w_q rho exactly
    assert np.all(rest[:, 1:5] == rest[:, 1:2]) and np.all(rest[:, 5:] == rest[:, 5:6])
    assert np.all(rest[:, 0] == 4 * rest[:, 1]) and all(j == (0, 0) for j in exact_momentum(rest))
    on_rows, on_cols = exact_momentum(f[(kind == 1) & flip]), exact_momentum(f[(kind == 1) & ~flip])   # u on an axis
    assert all(jc == 0 for _, jc in on_rows) and all(jr == 0 for jr, _ in on_cols)
    assert any(jr != 0 for jr, _ in on_rows) and any(jc != 0 for _, jc in on_cols)
    same, opposite = exact_momentum(f[(kind == 2) & flip]), exact_momentum(f[(kind == 2) & ~flip])    # ux = +-uy
    assert all(jr == jc for jr, jc in same) and all(jr == -jc for jr, jc in opposite)
    assert any(jr != 0 for jr, _ in same) and any(jr != 0 for jr, _ in opposite)
    pair = f[kind == 3]                               # exact zeros inside jx and jy
    assert np.all(pair[:, 1] == pair[:, 3]) and np.all(pair[:, 2] == pair[:, 4])
    if "g" in st:                                     # C = 0 exactly: the one carve-out of the unit statistics
        g, zero_c = st["g"], st["zero_c"]
        assert 0.015 * n <= np.sum(zero_c) <= 0.05 * n and np.any(zero_c[:42])
        assert np.all(g[zero_c] == 0) and np.all(np.any(g[~zero_c] != 0, axis=1))


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reference_order_against_80_bit(oracle, case):
    st, exact = xc.case_data(case)
    pop, mom = reference_order(oracle, case, st)
    assert np.all(np.isfinite(pop)) and np.all(np.isfinite(mom))
    keep = None
    if case.cls.startswith("ade"):
        zero = st["zero_c"]
        assert np.sum(zero) <= 0.05 * len(zero)
        assert np.all(pop[zero, 9:] == 0) and np.all(mom[zero, 3] == 0)   # nine zeros and conc = 0
        keep = ~zero
    sp, sm = xc.measure(pop, mom, exact, keep)
    _rows[case.name] = (sp, sm)
    print("%-44s pop %s   mom %s" % (case.name, xc.fmt(sp), xc.fmt(sm)))
    assert np.all(np.isfinite(sp + sm)), (sp, sm)
    assert max(sp) <= 256 and max(sm) <= 256, (sp, sm)
