#!/usr/bin/env python3
"""Fluid + transported scalar (lbm_ade_*): the fused step against the same step composed from the unfused operators
and against the single-step BGK launch, on one periodic box, in one process, alternated.  Prints one JSON line.

  fused      lbm_ade_solver_step: one launch per step on a periodic box (ade.hpp k_ade_stream_collide)
  composed   calc_rho, calc_u, calc_rho(g), equilibrium x2, axpb x2 (u + w), collision x2, advect x2 per step (11 launches)
  bgk        lbm_bgk_stream_collide on two padded lattices (the single-step BGK launch, f only)
  --fixed-walls adds two walled boxes (bounce-back rows and columns, two launches per step): walls_no_flux, the scalar's
  no-flux walls, and walls_fixed, all four edges FIXED (lbm_ade_scalar_bc; C_w = 1e-3 on row 0, a device profile on
  column 0, 0 on the others)
  --buoyancy adds a second periodic box whose scalar pushes on the fluid (lbm_ade_buoyancy, beta = (0.5, -0.3),
  c_ref = 5e-4, Guo's coefficients): buoyant, the same one launch and 288 B per node update in the reference order
  whatever --form says, beside the passive step of the same run
  --interior-walls adds two boxes with bounce-back rows: iwalls_plain, and iwalls_rectangle with the sedimentation
  driver's rectangle (rectangle_sedimentation_test.cpp:73-75 scaled to the box: ceiling R/3 above the last row, columns
  2C/8 .. 5C/16; absorbing) as interior walls (lbm_ade_iwalls): one more launch per step, one lane per table node
  --open adds two boxes with a bounce-back bottom row: open_plain, and open_channel with the sedimentation channel's open
  boundaries (lbm_ade_open_add_channel: inlet, extrapolated outlet, specular lid, zero-gradient copies, concentration
  inlet): one more launch per step, one lane per listed node (3 R + 3 C - 9 of them)
  --wall-exchange is a mode of its own (nothing else is measured): on the iwalls_rectangle box after `warmup` steps, one
  AdeSolver.wall_exchange call (row kernel + fold + 48-byte copy + synchronise; 20 calls per repeat) alternated with the
  only other route to the same figures, both lattices of lbm_ade_solver_get_state copied into preallocated, touched host
  arrays (the host arithmetic on top is not counted); host clock around each call, after one forced call of either
  route, medians
  --kbc is a mode of its own (nothing else is measured): the pair step with a KBC fluid (lbm_ade_solver_create_m,
  ade_kbc.hpp) in both forms against what a user could assemble without it -- (a) the BGK pair step plus (c) one single-step lbm_kbc_stream_collide launch of
  the form, 432 B per node where the fused step moves 288 B.  All start from the reference KBC driver's state
  (lbm_kbc_equilibrium without the u^2 terms) on a drifting shear wave: a lattice exactly at equilibrium makes KBC's
  gamma 0/0.  ms per step of every repeat, the condition (b) < (a) + (c) per repeat, (b) / (a), the algorithmic TB/s of (b)
  --kbc --buoyancy adds to that mode, in the same process and alternated with the rest: kbc_pair_buoyant, the pair step with
  the forced KBC collision (lbm_ade_solver_set_buoyancy_m, beta = (0.5, -0.3), c_ref = 5e-4, u_shift = 1; the reference order),
  and bgk_pair_buoyant, the BGK buoyant pair step (Guo's coefficients); under "buoyant": the condition kbc_pair_buoyant < bgk_pair + kbc_single_ref
  per repeat, and kbc_pair_buoyant over the passive reference-order kbc_pair_ref and over bgk_pair_buoyant
  --kbc --open is a mode of its own: the sedimentation channel with a KBC fluid (lbm_ade_solver_set_open_m, the open pass of
  capi_ade_kbc_open.hip) -- a bounce-back bottom row, the channel's open table (lbm_ade_open_add_channel, u_in = 0.02, s2 = 1.6) and the
  scaled rectangle as interior walls -- in one process, alternated: kbc_channel (default form: interior, edge pass, open
  pass, interior-wall pass), kbc_plain (the same box without tables: interior + edge pass), bgk_channel (the BGK fluid with
  the same tables, the lbm_ade_stream_collide_o path) and, with --buoyancy, kbc_channel_buoyant (the forced collision).  ms
  per step of every repeat, kbc_channel over kbc_plain and over bgk_channel per repeat, the table sizes, the launches per
  step, and the host time of one wall_exchange_m call on the KBC channel (20 calls, median)
MLUPS count node updates (of the pair for fused / composed).  Algorithmic bytes of the fused step: 288 B per node update
(18 loads + 18 stores of 8 bytes), of the BGK step 144 B.  Time: device events around `steps` steps after `warmup`.
usage: ade_bench.py [--size 8192] [--steps 50] [--warmup 5] [--repeats 3] [--form default|ref|fast] [--fixed-walls] [--buoyancy]
       [--interior-walls] [--open] [--wall-exchange] [--kbc] [--kbc --open [--buoyancy]]"""
import argparse
import ctypes as ct
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lattice-boltzmann-method_amd"))

import torch  # noqa: E402

import pylbm  # noqa: E402
from pylbm import _ptr  # noqa: E402

HBM_TBS = 8.0
W = (3e-3, 3e-3)


def rectangle_table(lib, R, C):
    """the sedimentation driver's rectangle (rectangle_sedimentation_test.cpp:73-75) scaled to the box, absorbing"""
    r_top, c1, c2 = -(R // 3), C * 2 // 8, C * 5 // 16
    n_side = R // 3 - 2  # rows r_top + 1 .. R - 2
    fx, neg, pos = pylbm.ADE_SCALAR_FIXED, pylbm.ADE_FACE_COL_NEG, pylbm.ADE_FACE_COL_POS
    table = pylbm.AdeInteriorWalls(lib, R, C)
    table.add(r_top + 1, c1, 1, 0, n_side, neg, neg, fx, 0.0)          # first wall; g runs through the last row,
    table.add(-1, c1, 1, 0, 1, 0, neg & ~0x40, fx, 0.0)                # slot 7 of its foot left to the bottom wall
    table.add(r_top, c1, 0, 1, c2 - c1 + 1, pylbm.ADE_FACE_ROW_NEG, pylbm.ADE_FACE_ROW_NEG, fx, 0.0)  # ceiling
    table.add(r_top + 1, c2, 1, 0, n_side, pos, pos, fx, 0.0)          # second wall
    return table.finalize()


def wall_exchange_bench(lib, a, fluid, scalar, f, g, st):
    """--wall-exchange: the JSON fields of that mode; f, g: the dense pre-collision state on the device"""
    import numpy as np
    R = C = a.size
    rbc = pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK)
    table = rectangle_table(lib, R, C)
    w = pylbm.AdeSolver(lib, R, C, fluid, scalar, bc=rbc, stream=st.value, walls=table)
    wf, wg, _, _, wgeo = w.lattices()
    dg = pylbm.Geom(R, C, 0)
    lib.lattice_copy_rows(_ptr(wf), ct.byref(wgeo), 0, _ptr(f), ct.byref(dg), 0, R, st)
    lib.lattice_copy_rows(_ptr(wg), ct.byref(wgeo), 0, _ptr(g), ct.byref(dg), 0, R, st)
    w.step(max(a.warmup, 2))
    w.sync()
    hf, hg = np.zeros((R, C, 9)), np.zeros((R, C, 9))  # preallocated and touched

    def state():
        lib.ade_solver_get_state(w.h, pylbm._hptr(hf), pylbm._hptr(hg), None, None, None)

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    values = w.wall_exchange()  # the forced warm-up of either route: first-use allocations
    state()
    t_x, t_s = [], []
    for _ in range(a.repeats):
        t_x += [clock(w.wall_exchange) for _ in range(20)]
        t_s.append(clock(state))

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "calls": len(v)}

    out = {"metric": "wall exchange of the iwalls_rectangle box against get_state of both lattices to the host",
           "size": [R, C], "form": a.form, "steps_before": max(a.warmup, 2), "iwalls_table_nodes": table.count(),
           "wall_exchange": summary(t_x), "get_state_f_g": summary(t_s),
           "get_state_over_wall_exchange": round(statistics.median(t_s) / statistics.median(t_x), 1),
           "values": dict(zip(pylbm.WALLX_NAMES, values.tolist()))}
    w.close()
    table.close()
    return out


def kbc_bench(lib, a, rho, conc, u, st, timed):
    """--kbc: the JSON fields of that mode; rho, conc, u: the dense initial moments on the device (u overwritten)"""
    R = C = a.size
    n = R * C
    dev = rho.device
    s2 = 1.0 / (0.5 + 3.0 * 1.7e-4)
    u[0] = 0.01  # no node at rest
    f, g = (torch.empty((9, R, C), dtype=torch.float64, device=dev) for _ in range(2))
    lib.kbc_equilibrium(_ptr(f), _ptr(rho), _ptr(u), R, C, 1, None)
    lib.equilibrium(_ptr(g), _ptr(u), _ptr(conc), R, C, None)
    torch.cuda.synchronize()
    dg = pylbm.Geom(R, C, 0)
    forms = {"fast": pylbm.FORM_REASSOCIATED, "ref": pylbm.FORM_REFERENCE_ORDER}
    solvers = {"bgk_pair": pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(1.2, 0), pylbm.AdeParams(1.7, W), stream=st.value)}
    for name, form in forms.items():
        solvers["kbc_pair_" + name] = pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(s2, form), pylbm.AdeParams(1.7, W, form=form),
                                                      stream=st.value)
    if a.buoyancy:
        ref = forms["ref"]
        solvers["kbc_pair_buoyant"] = pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(s2, ref), pylbm.AdeParams(1.7, W, form=ref),
                                                      stream=st.value, buoyancy=pylbm.AdeBuoyancy((0.5, -0.3), 5e-4, 1.0))
        solvers["bgk_pair_buoyant"] = pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(1.2, 0), pylbm.AdeParams(1.7, W), stream=st.value,
                                                      buoyancy=pylbm.AdeBuoyancy((0.5, -0.3), 5e-4, 0.5, (3.0, 9.0)))
    for sv in solvers.values():
        fc, gc, _, _, sg = sv.lattices()
        lib.lattice_copy_rows(_ptr(fc), ct.byref(sg), 0, _ptr(f), ct.byref(dg), 0, R, st)
        lib.lattice_copy_rows(_ptr(gc), ct.byref(sg), 0, _ptr(g), ct.byref(dg), 0, R, st)
    # (c): the single-step KBC launch on two padded lattices, per form
    plane = n + lib.default_plane_pad(R, C)
    lat = [torch.empty(9 * plane, dtype=torch.float64, device=dev) for _ in range(2)]
    pg, pbc = pylbm.Geom(R, C, 0, plane, 0), pylbm.Bc.periodic()
    lib.lattice_copy_rows(_ptr(lat[0]), ct.byref(pg), 0, _ptr(f), ct.byref(dg), 0, R, st)
    lib.kbc_collide(_ptr(lat[1]), _ptr(lat[0]), ct.byref(pg), ct.byref(pbc), ct.byref(pylbm.KbcParams(s2, forms["fast"])), None, None, st)
    lib.stream_sync(st)
    del f, g
    cur = [1]

    def single(form):
        prm = pylbm.KbcParams(s2, form)

        def run(k):
            for _ in range(k):
                lib.kbc_stream_collide(_ptr(lat[cur[0] ^ 1]), _ptr(lat[cur[0]]), ct.byref(pg), ct.byref(pbc), ct.byref(prm), 0, R,
                                       None, None, st)
                cur[0] ^= 1
        return run

    runs = {k: sv.step for k, sv in solvers.items()}
    for name, form in forms.items():
        runs["kbc_single_" + name] = single(form)
    for fn in runs.values():
        timed(fn, a.warmup)
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            times[k].append(timed(fn, a.steps))
    ms = {k: [round(t / a.steps * 1e3, 4) for t in v] for k, v in times.items()}
    nonfinite = {k: float(sv.diag()[pylbm.DIAG_NONFINITE]) for k, sv in solvers.items()}
    out = {"metric": "fluid + scalar pair step with a KBC fluid, D2Q9 f64, periodic box", "size": [R, C], "steps": a.steps,
           "repeats": a.repeats, "s2": s2, "ms_per_step": ms, "nonfinite_after": nonfinite}
    for name in forms:
        b, c = ms["kbc_pair_" + name], ms["kbc_single_" + name]
        out[name] = {"b_lt_a_plus_c_per_repeat": [x < y + z for x, y, z in zip(b, ms["bgk_pair"], c)],
                     "a_plus_c_ms": [round(y + z, 4) for y, z in zip(ms["bgk_pair"], c)],
                     "b_over_a": [round(x / y, 3) for x, y in zip(b, ms["bgk_pair"])],
                     "b_algorithmic_tbs": round(288.0 * n / (statistics.median(b) * 1e-3) / 1e12, 3)}
    if a.buoyancy:
        x, p, bb, sgl = ms["kbc_pair_buoyant"], ms["kbc_pair_ref"], ms["bgk_pair_buoyant"], ms["kbc_single_ref"]
        out["buoyant"] = {"a_lt_bgk_pair_plus_kbc_single_ref_per_repeat": [v < y + z for v, y, z in zip(x, ms["bgk_pair"], sgl)],
                          "bgk_pair_plus_kbc_single_ref_ms": [round(y + z, 4) for y, z in zip(ms["bgk_pair"], sgl)],
                          "a_over_passive_ref": [round(v / y, 3) for v, y in zip(x, p)],
                          "a_over_bgk_buoyant": [round(v / y, 3) for v, y in zip(x, bb)],
                          "a_algorithmic_tbs": round(288.0 * n / (statistics.median(x) * 1e-3) / 1e12, 3)}
    for sv in solvers.values():
        sv.close()
    return out


def kbc_open_bench(lib, a, rho, conc, u, st, timed):
    """--kbc --open: the JSON fields of that mode; rho, conc, u: the dense initial moments on the device (u overwritten)"""
    R = C = a.size
    dev = rho.device
    # s2 = 1.6: next to 2 the channel does not stay finite with this collision (nor does the CPU yardstick's: DESIGN.md
    # section 11); the time of a step does not depend on the rate
    s2 = 1.6
    u[0] = 0.01   # no node at rest: the reference KBC driver's state on a shear wave ...
    u[1] += 0.02  # ... drifting towards the outlet with the inlet's velocity
    f, g = (torch.empty((9, R, C), dtype=torch.float64, device=dev) for _ in range(2))
    lib.kbc_equilibrium(_ptr(f), _ptr(rho), _ptr(u), R, C, 1, None)
    lib.equilibrium(_ptr(g), _ptr(u), _ptr(conc), R, C, None)
    torch.cuda.synchronize()
    dg = pylbm.Geom(R, C, 0)
    obc = pylbm.Bc(row_hi=pylbm.EDGE_BOUNCE_BACK)
    channel = pylbm.AdeOpenBoundary(lib, R, C).channel(0.02, 1e-3, R // 4).finalize()
    body = rectangle_table(lib, R, C)
    scalar = pylbm.AdeParams(1.7, W)
    kw = dict(bc=obc, stream=st.value)
    solvers = {"kbc_channel": pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(s2), scalar, walls=body, open=channel, **kw),
               "kbc_plain": pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(s2), scalar, **kw),
               "bgk_channel": pylbm.AdeSolver(lib, R, C, pylbm.BgkParams(1.2, 0), scalar, walls=body, open=channel, **kw)}
    if a.buoyancy:
        solvers["kbc_channel_buoyant"] = pylbm.AdeSolver(lib, R, C, pylbm.KbcParams(s2), scalar, walls=body, open=channel,
                                                         buoyancy=pylbm.AdeBuoyancy((0.5, -0.3), 5e-4, 1.0), **kw)
    for sv in solvers.values():  # the state through the context, which primes the carry of its table
        fc, gc, _, _, sg = sv.lattices()
        lib.lattice_copy_rows(_ptr(fc), ct.byref(sg), 0, _ptr(f), ct.byref(dg), 0, R, st)
        lib.lattice_copy_rows(_ptr(gc), ct.byref(sg), 0, _ptr(g), ct.byref(dg), 0, R, st)
        lib.stream_sync(st)
        if sv.open is not None:  # the carry of the state just copied in: the table again, on the pre-collision state
            sv.set_open_m(None)
            sv.set_open_m(channel)
    del f, g
    runs = {k: sv.step for k, sv in solvers.items()}
    for fn in runs.values():
        timed(fn, a.warmup)
    before = {k: sv.launches() for k, sv in solvers.items()}
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            times[k].append(timed(fn, a.steps))
    ms = {k: [round(t / a.steps * 1e3, 4) for t in v] for k, v in times.items()}
    per_step = {k: (sv.launches() - before[k]) / (a.steps * a.repeats) for k, sv in solvers.items()}
    nonfinite = {k: float(sv.diag()[pylbm.DIAG_NONFINITE]) for k, sv in solvers.items()}
    x = solvers["kbc_channel"]
    values = x.wall_exchange_m()  # the forced first call: its allocations
    calls = []
    for _ in range(20):
        t0 = time.perf_counter()
        x.wall_exchange_m()
        calls.append((time.perf_counter() - t0) * 1e3)
    out = {"metric": "sedimentation channel (open table + rectangle) with a KBC fluid, D2Q9 f64", "size": [R, C], "steps": a.steps,
           "repeats": a.repeats, "s2": s2, "open_table_nodes": channel.count(), "iwalls_table_nodes": body.count(),
           "ms_per_step": ms, "launches_per_step": per_step, "nonfinite_after": nonfinite,
           "kbc_channel_over_kbc_plain": [round(p / q, 4) for p, q in zip(ms["kbc_channel"], ms["kbc_plain"])],
           "kbc_channel_over_bgk_channel": [round(p / q, 4) for p, q in zip(ms["kbc_channel"], ms["bgk_channel"])],
           "wall_exchange_m_ms": {"median": round(statistics.median(calls), 4), "min": round(min(calls), 4), "calls": len(calls)},
           "wall_exchange_values": dict(zip(pylbm.WALLX_NAMES, values.tolist()))}
    for sv in solvers.values():
        sv.close()
    channel.close()
    body.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--form", choices=["default", "ref", "fast"], default="default")
    ap.add_argument("--skip-composed", action="store_true")
    ap.add_argument("--fixed-walls", action="store_true")
    ap.add_argument("--buoyancy", action="store_true")
    ap.add_argument("--interior-walls", action="store_true")
    ap.add_argument("--open", action="store_true")
    ap.add_argument("--wall-exchange", action="store_true")
    ap.add_argument("--kbc", action="store_true")
    a = ap.parse_args()
    form = {"default": pylbm.FORM_DEFAULT, "ref": pylbm.FORM_REFERENCE_ORDER, "fast": pylbm.FORM_REASSOCIATED}[a.form]
    lib = pylbm.Lib()
    if lib.device_count() < 1:
        raise SystemExit("ade_bench.py: no HIP device visible")
    R = C = a.size
    n = R * C
    dev = torch.device("cuda:0")
    st = ct.c_void_p()
    lib.stream_create(ct.byref(st))
    e0, e1 = ct.c_void_p(), ct.c_void_p()
    lib.event_create(ct.byref(e0))
    lib.event_create(ct.byref(e1))

    def timed(fn, steps):
        lib.event_record(e0, st)
        fn(steps)
        lib.event_record(e1, st)
        ms = ct.c_float()
        lib.event_elapsed_ms(ct.byref(ms), e0, e1)
        return ms.value / 1e3

    # initial state built on the device: a shear wave and a scalar band, equilibrium populations (dense SoA)
    r = torch.arange(R, dtype=torch.float64, device=dev).view(R, 1).expand(R, C)
    c = torch.arange(C, dtype=torch.float64, device=dev).view(1, C).expand(R, C)
    rho = torch.ones((R, C), dtype=torch.float64, device=dev)
    conc = 1e-3 * torch.exp(-((c - C / 2) / (C / 8)) ** 2)
    u = torch.zeros((2, R, C), dtype=torch.float64, device=dev)
    u[1] = 0.02 * torch.sin(2 * math.pi * r / R)
    del r, c
    if a.kbc:
        out = (kbc_open_bench if a.open else kbc_bench)(lib, a, rho, conc, u, st, timed)
        lib.event_destroy(e0)
        lib.event_destroy(e1)
        lib.stream_destroy(st)
        print(json.dumps(out))
        return
    f = torch.empty((9, R, C), dtype=torch.float64, device=dev)
    g = torch.empty_like(f)
    lib.equilibrium(_ptr(f), _ptr(u), _ptr(rho), R, C, None)
    lib.equilibrium(_ptr(g), _ptr(u), _ptr(conc), R, C, None)
    torch.cuda.synchronize()

    fluid, scalar = pylbm.BgkParams(1.2, 0, form=form), pylbm.AdeParams(1.7, W, form=form)
    if a.wall_exchange:
        out = wall_exchange_bench(lib, a, fluid, scalar, f, g, st)
        lib.event_destroy(e0)
        lib.event_destroy(e1)
        lib.stream_destroy(st)
        print(json.dumps(out))
        return

    # fused: the solver context; its lattices are filled from the dense arrays (pre-collision state)
    sv = pylbm.AdeSolver(lib, R, C, fluid, scalar, stream=st.value)
    f_cur, g_cur, _, _, sg = sv.lattices()   # device addresses as Python ints: through _ptr, never bare (a bare int is a C int)
    dg = pylbm.Geom(R, C, 0)
    lib.lattice_copy_rows(_ptr(f_cur), ct.byref(sg), 0, _ptr(f), ct.byref(dg), 0, R, st)
    lib.lattice_copy_rows(_ptr(g_cur), ct.byref(sg), 0, _ptr(g), ct.byref(dg), 0, R, st)
    lib.stream_sync(st)

    # single-step BGK on two padded lattices (as bench.py's box)
    plane = n + lib.default_plane_pad(R, C)
    bgk = [torch.empty(9 * plane, dtype=torch.float64, device=dev) for _ in range(2)]
    bg = pylbm.Geom(R, C, 0, plane, 0)
    lib.lattice_copy_rows(_ptr(bgk[0]), ct.byref(bg), 0, _ptr(f), ct.byref(dg), 0, R, st)
    bprm, bbc = pylbm.BgkParams(1.2, 0, form=form), pylbm.Bc.periodic()
    lib.bgk_collide(_ptr(bgk[1]), _ptr(bgk[0]), ct.byref(bg), ct.byref(bbc), ct.byref(bprm), None, None, st)
    cur = [1]

    def run_bgk(k):
        for _ in range(k):
            s, d = bgk[cur[0]], bgk[cur[0] ^ 1]
            lib.bgk_stream_collide(_ptr(d), _ptr(s), ct.byref(bg), ct.byref(bbc), ct.byref(bprm), 0, R, None, None, st)
            cur[0] ^= 1

    def run_fused(k):
        sv.step(k)

    walled = {}
    if a.fixed_walls:
        wbc = pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK, col_lo=pylbm.EDGE_BOUNCE_BACK,
                       col_hi=pylbm.EDGE_BOUNCE_BACK)
        prof = torch.zeros(R, dtype=torch.float64, device=dev)
        prof[R - R // 4:] = 1e-3
        for key, sbc in (("walls_no_flux", None),
                         ("walls_fixed", pylbm.AdeScalarBC(row_lo=1e-3, row_hi=0.0, col_lo=(0.0, prof), col_hi=0.0))):
            w = pylbm.AdeSolver(lib, R, C, fluid, scalar, bc=wbc, stream=st.value, scalar_bc=sbc)
            wf, wg, _, _, wgeo = w.lattices()
            lib.lattice_copy_rows(_ptr(wf), ct.byref(wgeo), 0, _ptr(f), ct.byref(dg), 0, R, st)
            lib.lattice_copy_rows(_ptr(wg), ct.byref(wgeo), 0, _ptr(g), ct.byref(dg), 0, R, st)
            walled[key] = w
        lib.stream_sync(st)

    buoyant = None
    if a.buoyancy:
        buoyant = pylbm.AdeSolver(lib, R, C, fluid, scalar, stream=st.value,
                                  buoyancy=pylbm.AdeBuoyancy((0.5, -0.3), 5e-4, 0.5, (3.0, 9.0)))
        bf, bgl, _, _, bgeo = buoyant.lattices()
        lib.lattice_copy_rows(_ptr(bf), ct.byref(bgeo), 0, _ptr(f), ct.byref(dg), 0, R, st)
        lib.lattice_copy_rows(_ptr(bgl), ct.byref(bgeo), 0, _ptr(g), ct.byref(dg), 0, R, st)
        lib.stream_sync(st)

    bodies, table = {}, None
    if a.interior_walls:
        rbc = pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK)
        table = rectangle_table(lib, R, C)
        for key, t in (("iwalls_plain", None), ("iwalls_rectangle", table)):
            w = pylbm.AdeSolver(lib, R, C, fluid, scalar, bc=rbc, stream=st.value, walls=t)
            wf, wg, _, _, wgeo = w.lattices()
            lib.lattice_copy_rows(_ptr(wf), ct.byref(wgeo), 0, _ptr(f), ct.byref(dg), 0, R, st)
            lib.lattice_copy_rows(_ptr(wg), ct.byref(wgeo), 0, _ptr(g), ct.byref(dg), 0, R, st)
            bodies[key] = w
        lib.stream_sync(st)

    channels, open_table = {}, None
    if a.open:
        obc = pylbm.Bc(row_hi=pylbm.EDGE_BOUNCE_BACK)
        open_table = pylbm.AdeOpenBoundary(lib, R, C).channel(0.02, 1e-3, R // 4).finalize()
        for key, t in (("open_plain", None), ("open_channel", open_table)):
            w = pylbm.AdeSolver(lib, R, C, fluid, scalar, bc=obc, stream=st.value, open=t)
            wf, wg, _, _, wgeo = w.lattices()
            lib.lattice_copy_rows(_ptr(wf), ct.byref(wgeo), 0, _ptr(f), ct.byref(dg), 0, R, st)
            lib.lattice_copy_rows(_ptr(wg), ct.byref(wgeo), 0, _ptr(g), ct.byref(dg), 0, R, st)
            channels[key] = w
        lib.stream_sync(st)

    # composed: the reference loop from the unfused operators (dense lattices f, g advance in place of the loop)
    if not a.skip_composed:
        fe, ge, fc, gc = (torch.empty_like(f) for _ in range(4))
        uw = torch.empty_like(u)

    def run_composed(k):
        for _ in range(k):
            lib.calc_rho(_ptr(rho), _ptr(f), R, C, st)
            lib.calc_u(_ptr(u), _ptr(f), _ptr(rho), R, C, st)
            lib.calc_rho(_ptr(conc), _ptr(g), R, C, st)
            lib.equilibrium(_ptr(fe), _ptr(u), _ptr(rho), R, C, st)
            lib.axpb(_ptr(uw[0]), _ptr(u[0]), ct.c_double(1.0), ct.c_double(W[0]), ct.c_longlong(n), st)
            lib.axpb(_ptr(uw[1]), _ptr(u[1]), ct.c_double(1.0), ct.c_double(W[1]), ct.c_longlong(n), st)
            lib.equilibrium(_ptr(ge), _ptr(uw), _ptr(conc), R, C, st)
            lib.collision(_ptr(fc), _ptr(f), _ptr(fe), ct.c_double(1.2), R, C, st)
            lib.collision(_ptr(gc), _ptr(g), _ptr(ge), ct.c_double(1.7), R, C, st)
            lib.advect(_ptr(f), _ptr(fc), R, C, st)
            lib.advect(_ptr(g), _ptr(gc), R, C, st)

    runs = {"fused": run_fused, "bgk": run_bgk}
    for key, w in walled.items():
        runs[key] = w.step
    if buoyant is not None:
        runs["buoyant"] = buoyant.step
    for key, w in bodies.items():
        runs[key] = w.step
    for key, w in channels.items():
        runs[key] = w.step
    if not a.skip_composed:
        runs["composed"] = run_composed
    for fn in runs.values():
        timed(fn, a.warmup)
    launches0 = sv.launches()
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            times[k].append(timed(fn, a.steps))
    launches = sv.launches() - launches0
    mlups = {k: n * a.steps / statistics.median(v) / 1e6 for k, v in times.items()}
    fused_tbs = 288.0 * n * a.steps / statistics.median(times["fused"]) / 1e12
    bgk_tbs = 144.0 * n * a.steps / statistics.median(times["bgk"]) / 1e12
    out = {"metric": "fused fluid + scalar step, D2Q9 f64, periodic box", "size": [R, C], "steps": a.steps,
           "repeats": a.repeats, "form": a.form,
           "fused_mlups": round(mlups["fused"], 1),
           "composed_mlups": round(mlups["composed"], 1) if "composed" in mlups else None,
           "bgk_single_step_mlups": round(mlups["bgk"], 1),
           "fused_over_composed": round(mlups["fused"] / mlups["composed"], 3) if "composed" in mlups else None,
           "fused_over_bgk": round(mlups["fused"] / mlups["bgk"], 3),
           "fused_algorithmic_tbs": round(fused_tbs, 3), "fused_fraction_of_8tbs": round(fused_tbs / HBM_TBS, 3),
           "bgk_algorithmic_tbs": round(bgk_tbs, 3),
           "fused_launches_per_step": launches / (a.steps * a.repeats),
           "times_s": {k: [round(t, 5) for t in v] for k, v in times.items()}}
    if walled:
        out["walls_no_flux_mlups"] = round(mlups["walls_no_flux"], 1)
        out["walls_fixed_mlups"] = round(mlups["walls_fixed"], 1)
        out["walls_fixed_over_no_flux"] = round(mlups["walls_fixed"] / mlups["walls_no_flux"], 4)
        out["walls_fixed_over_no_flux_per_repeat"] = [round(b / a, 4) for a, b in zip(times["walls_fixed"], times["walls_no_flux"])]
        out["walls_launches_total"] = {k: w.launches() for k, w in walled.items()}
        for w in walled.values():
            w.close()
    if buoyant is not None:
        out["buoyant_mlups"] = round(mlups["buoyant"], 1)
        out["buoyant_over_fused"] = round(mlups["buoyant"] / mlups["fused"], 4)
        out["buoyant_over_fused_per_repeat"] = [round(p / b, 4) for p, b in zip(times["fused"], times["buoyant"])]
        out["buoyant_launches_total"] = buoyant.launches()
        buoyant.close()
    if bodies:
        out["iwalls_plain_mlups"] = round(mlups["iwalls_plain"], 1)
        out["iwalls_rectangle_mlups"] = round(mlups["iwalls_rectangle"], 1)
        out["iwalls_rectangle_over_plain"] = round(mlups["iwalls_rectangle"] / mlups["iwalls_plain"], 4)
        out["iwalls_rectangle_over_plain_per_repeat"] = [round(p / b, 4) for p, b in
                                                         zip(times["iwalls_plain"], times["iwalls_rectangle"])]
        out["iwalls_table_nodes"] = table.count()
        out["iwalls_launches_total"] = {k: w.launches() for k, w in bodies.items()}
        for w in bodies.values():
            w.close()
        table.close()
    if channels:
        out["open_plain_mlups"] = round(mlups["open_plain"], 1)
        out["open_channel_mlups"] = round(mlups["open_channel"], 1)
        out["open_channel_over_plain"] = round(mlups["open_channel"] / mlups["open_plain"], 4)
        out["open_channel_over_plain_per_repeat"] = [round(p / b, 4) for p, b in zip(times["open_plain"], times["open_channel"])]
        out["open_table_nodes"] = open_table.count()
        out["open_launches_total"] = {k: w.launches() for k, w in channels.items()}
        for w in channels.values():
            w.close()
        open_table.close()
    sv.close()
    lib.event_destroy(e0)
    lib.event_destroy(e1)
    lib.stream_destroy(st)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
