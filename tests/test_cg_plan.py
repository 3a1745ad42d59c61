"""CPU suite: the tile plan of the fused two-phase step (csrc/cg_plan.hpp: inner rectangle, frame, big tiles, patch order)
through drivers/cg_plan_dump -- one batch of cases in one subprocess -- against the invariants the launches rely on,
stated here in rows and columns and checked in Python, and against a Python statement of the same arithmetic.

`python tests/test_cg_plan.py` prints the sweep, one case per line, for a cg_plan_dump built with sanitizers (make san)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "lattice-boltzmann-method_amd", "drivers")
FIELDS = "R C ghost lo_halo hi_halo row_begin row_end part edge_rows cg_split cg_big cg_big_xcd".split()
FRAME, INNER = 1, 2
DEFAULT_KNOBS = (1, 2, 402)
# no ghost rows with walls; 3 ghost rows with HALO on both row edges / the low edge only / the high edge only
LAYOUTS = [(0, 0, 0), (3, 1, 1), (3, 1, 0), (3, 0, 1)]
HEIGHTS = list(range(7, 200)) + [2048, 2050, 2063]
WIDTHS = (2, 3, 34, 35, 61, 64, 66, 67, 96, 99, 100, 131, 200, 1040)
EDGES = (0, 3, 16, 40)
N_CASES, N_SPLIT = 87808, 38542   # of the sweep below, counted once with the arithmetic of the commit that introduced the planner


def sweep():
    """part 0 on the whole block, FRAME and INNER with every edge_rows the API admits (2 * edge_rows <= R)"""
    out = []
    for R in HEIGHTS:
        for C in WIDTHS:
            for ghost, lo, hi in LAYOUTS:
                out.append((R, C, ghost, lo, hi, 0, R, 0, 0) + DEFAULT_KNOBS)
                out += [(R, C, ghost, lo, hi, 0, R, part, e) + DEFAULT_KNOBS
                        for part in (FRAME, INNER) for e in EDGES if 2 * e <= R]
    return out


def row_range_cases():
    out = []
    for R in (64, 130, 200):
        for r0, r1 in ((0, R), (5, R), (16, R - 7), (3, 40), (R - 40, R)):
            out += [(R, C, ghost, lo, hi, r0, r1, 0, 0) + DEFAULT_KNOBS for C in WIDTHS for ghost, lo, hi in LAYOUTS]
    return out


def plans(cases):
    """the plans cg_plan_dump gives for `cases` (tuples in the order of FIELDS, optionally + experiments), as dicts"""
    subprocess.check_call(["make", "-s", "-C", DRIVERS, "bin/cg_plan_dump"])
    text = "".join(" ".join(str(int(v)) for v in c) + "\n" for c in cases)
    r = subprocess.run([os.path.join(DRIVERS, "bin", "cg_plan_dump")], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-300:] + r.stderr[-300:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def expected(case, experiments=False):
    """the same arithmetic in Python, 16 x 32 tiles"""
    R, C, ghost, lo, hi, rb0, re, part, edge, cg_split, cg_big, cg_big_xcd = case
    TR, TC = 16, 32
    tiles_r, tiles_c = -(-(re - rb0) // TR), -(-C // TC)
    lo_row = -2 if ghost and lo else 1
    hi_row = R + 1 if ghost and hi else R - 2
    ok = [i for i in range(tiles_r)
          if rb0 + i * TR - 2 >= lo_row and rb0 + i * TR + TR + 1 <= hi_row and rb0 + i * TR + TR <= re]
    ir0, ir1 = (ok[0], ok[-1] + 1) if ok else (tiles_r, 0)
    ic0, ic1 = 1, min(int((C - 3) / TC), tiles_c)   # (C = 2: the quotient rounds towards zero)
    if part and edge > 0:
        ir0, ir1 = max(ir0, -(-edge // TR)), min(ir1, (re - rb0 - edge) // TR)
    split = bool(part or cg_split) and ir1 - ir0 >= 1 and ic1 - ic0 >= 1
    shapes = [(32, 32), (16, 64), (16, 128), (32, 64), (32, 64), (8, 64), (16, 64), (16, 128), (16, 32)]
    shape = (cg_big if 1 <= cg_big <= 10 else 0) if experiments else (2 if cg_big > 0 else 0)
    n_btr = n_btc = 0
    if split and shape:
        br, bc = shapes[1 if shape == 10 else shape - 1]
        rows16 = ((ir1 - ir0) * 16 // br) * br // 16 * 16
        n_btr, n_btc = rows16 // br, (ic1 - ic0) * 32 // bc
        if n_btr >= 1 and n_btc >= 1 and n_btr * br == rows16 and (n_btc * bc) % 32 == 0:
            ir1, ic1 = ir0 + rows16 // 16, ic0 + n_btc * bc // 32
        else:
            n_btr = n_btc = 0
    inner = (ir1 - ir0) * (ic1 - ic0) if split else 0
    zero_side = cg_big_xcd >= 100 and (cg_big_xcd // 100 == 0 or cg_big_xcd % 100 == 0)
    return dict(tiles_r=tiles_r, tiles_c=tiles_c, ir0=ir0, ir1=ir1, ic0=ic0, ic1=ic1, split=int(split),
                frame=tiles_r * tiles_c - inner, inner=inner, n_btr=n_btr, n_btc=n_btc, shape=shape,
                big_xcd=402 if zero_side else cg_big_xcd)


def violations(case, p):
    """what a SPLIT plan must hold, in rows and columns of the block"""
    R, C, ghost, lo, hi, rb0, re, part, edge = case[:9]
    lo_row = -2 if ghost and lo else 1
    hi_row = R + 1 if ghost and hi else R - 2
    r0, r1, c0, c1 = rb0 + 16 * p["ir0"], rb0 + 16 * p["ir1"], 32 * p["ic0"], 32 * p["ic1"]
    bad = []
    if not (0 <= p["ir0"] < p["ir1"] <= p["tiles_r"] and 1 <= p["ic0"] < p["ic1"] <= p["tiles_c"]):
        bad.append("tile rectangle outside the tiles")
    if not (r0 - 2 >= lo_row and r1 + 1 <= hi_row and r1 <= re):
        bad.append(f"ring rows of [{r0}, {r1}) leave the plain rows [{lo_row}, {hi_row}] or the row range")
    if not (c0 - 2 >= 1 and c1 + 1 <= C - 2):
        bad.append(f"ring columns of [{c0}, {c1}) leave [1, {C - 2}]")
    if part and not (r0 >= edge and r1 <= R - edge):
        bad.append(f"rows [{r0}, {r1}) reach into the {edge} edge rows")
    if p["n_btr"] and not (p["ir1"] - p["ir0"] == p["n_btr"] and (p["ic1"] - p["ic0"]) * 32 == p["n_btc"] * 64):
        bad.append("the rectangle is not n_btr x n_btc tiles of 16 x 64")
    if p["frame"] + p["inner"] != p["tiles_r"] * p["tiles_c"] or p["inner"] != (p["ir1"] - p["ir0"]) * (p["ic1"] - p["ic0"]):
        bad.append("frame + inner is not every tile")
    return bad


def check(cases):
    got = plans(cases)
    bad = [f"{dict(zip(FIELDS, c))}: {v}; plan {p}" for c, p in zip(cases, got) if p["split"] for v in violations(c, p)]
    assert not bad, f"{len(bad)} violations, first:\n" + "\n".join(bad[:10])
    diff = [f"{dict(zip(FIELDS, c))}: {p} != {expected(c)}" for c, p in zip(cases, got) if p != expected(c)]
    assert not diff, f"{len(diff)} plans differ from the Python statement, first:\n" + "\n".join(diff[:5])
    return got


def test_sweep_of_whole_blocks_and_parts():
    cases = sweep()
    assert len(cases) == N_CASES
    got = check(cases)
    assert sum(p["split"] for p in got) == N_SPLIT
    # an unsplit plan is one launch of every tile
    assert all(p["inner"] == 0 and p["frame"] == p["tiles_r"] * p["tiles_c"] and p["n_btr"] == 0 for p in got if not p["split"])
    # FRAME and INNER of one case are the two halves of the same plan
    by_case = {c: p for c, p in zip(cases, got)}
    for c, p in by_case.items():
        if c[7] == FRAME:
            assert p == by_case[c[:7] + (INNER,) + c[8:]]


def test_row_ranges():
    cases = row_range_cases()
    got = check(cases)
    assert sum(p["split"] for p in got) == sum(expected(c)["split"] for c in cases) > 200


def test_heights_that_once_lost_edge_rows_to_inner():
    """0 < R % 16 < edge_rows: the last edge rows lie in the partial tile row AND the one above"""
    cases = [(R, 1040, 3, 1, 1, 0, R, INNER, e) + DEFAULT_KNOBS for R in (130, 2050) for e in (3, 16, 40)]
    got = check(cases)
    assert [(16 * p["ir0"], 16 * p["ir1"]) for p in got] == [(16, 112), (16, 112), (48, 80), (16, 2032), (16, 2032), (48, 2000)]


def test_split_and_big_knobs():
    base = (200, 1040, 0, 0, 0, 0, 200)
    off, small, dflt, big7 = plans([base + (0, 0, 0, 2, 402), base + (0, 0, 1, 0, 402), base + (0, 0, 1, 2, 402), base + (0, 0, 1, 7, 402)])
    assert not off["split"] and off["frame"] == 13 * 33
    assert small["split"] and small["shape"] == 0 and small["n_btr"] == 0
    assert (small["ir0"], small["ir1"], small["ic0"], small["ic1"]) == (1, 12, 1, 32)    # ... and an odd number of tile columns
    assert dflt["shape"] == 2 and (dflt["n_btr"], dflt["n_btc"]) == (11, 15) and dflt["ic1"] == 31
    assert big7 == dflt                                                                  # the default build ships shape 2 only
    inner_off = plans([base + (INNER, 16, 0, 2, 402)])[0]
    assert inner_off["split"], "a part launch splits whatever \"cg_split\" says"
    # the experiments build: every shape of the sweep, the walking tile on the tiles of shape 2, nothing beyond
    cases = [base + (0, 0, 1, big, 402) for big in range(0, 13)]
    got = plans([c + (1,) for c in cases])
    assert [p["shape"] for p in got] == [0] + list(range(1, 11)) + [0, 0]
    assert got == [expected(c, True) for c in cases]
    assert {k: got[10][k] for k in ("ir1", "ic1", "n_btr", "n_btc")} == {k: got[2][k] for k in ("ir1", "ic1", "n_btr", "n_btc")}
    assert (got[1]["n_btr"], got[1]["n_btc"]) == (5, 31) and (got[3]["n_btr"], got[3]["n_btc"]) == (11, 7)


def test_patch_order_code():
    """the code k_cg_tile_mn gets: as given, except that a patch code (>= 100 = 100 PR + PC) with a zero side is 4 x 2"""
    codes = (402, 202, 801, 2, 100, 200, 400, 7, 99)
    got = plans([(130, 1040, 3, 1, 1, 0, 130, 0, 0, 1, 2, x) for x in codes])
    assert [p["big_xcd"] for p in got] == [402, 202, 801, 2, 402, 402, 402, 7, 99]


if __name__ == "__main__":
    sys.stdout.write("".join(" ".join(map(str, c)) + "\n" for c in sweep() + row_range_cases()))
