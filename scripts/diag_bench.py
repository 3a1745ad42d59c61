#!/usr/bin/env python3
"""The measurements of profiles/diag.txt (DESIGN.md "Diagnostics"): N x N with N = DIAG_N (default 8192), one process per
mode, one "RESULT {json}" line each.
usage: diag_bench.py MODE
  kern_rows | kern_rows_conc | kern_fold | kern_bgk1 | kern_calc_rho   25 launches of one kernel, to run under
                         `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/diag_bench.py MODE`
                         (each in a run of its own; drop the first 5 dispatches, take the median of the trace)
  wall_new               wall time of one lbm_solver_diag call (median of 20 after 3)
  wall_parent            the same information through lbm_solver_get_moments_aos + a host sum (median of 5 after 2)
  run_new                1000 steps of the Poiseuille-type channel through run_until, after a forced 201-step warm-up
  run_parent             the same through the drivers' loop: 100-step calls, moments to the host, host mean
The *_parent modes use only entry points the parent commit has: run them with LBM_HIP_LIB pointing at a build of the parent
(scripts/r04_ab_setup.sh builds one) and the others with this tree's library, alternating."""
import ctypes as ct
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lattice-boltzmann-method_amd"))
import numpy as np
import torch

import pylbm
from pylbm import _hptr, _ptr

N = int(os.environ.get("DIAG_N", "8192"))
mode = sys.argv[1]
lib = pylbm.Lib()
dev = torch.device("cuda:0")
out = dict(mode=mode, N=N, lib=os.environ.get("LBM_HIP_LIB", "tree"))


def sync():
    torch.cuda.synchronize()


def rand(*shape):
    return torch.rand(shape, dtype=torch.float64, device=dev) + 0.5


def poiseuille(n):
    tau = np.sqrt(3.0 / 16.0) + 0.5
    u_max = 1.030985714E-1
    nu = (2.0 * tau - 1.0) / 6.0
    p_grad = 8.0 * nu * u_max / (n * n)
    bc = pylbm.Bc(col_lo=pylbm.EDGE_BOUNCE_BACK, col_hi=pylbm.EDGE_BOUNCE_BACK, pressure_rows=1,
                  rho_inlet=3.0 * (n - 1) * p_grad + 1.0, rho_outlet=1.0)
    sv = pylbm.Solver(lib, pylbm.MODEL_BGK, n, n, pylbm.BgkParams(1.0 / tau, 1), bc=bc)
    w = torch.tensor([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4, dtype=torch.float64, device=dev)
    f = w[:, None, None].expand(9, n, n).contiguous()
    lib.solver_set_f_soa_dev(sv.h, _ptr(f))
    sync()
    del f
    return sv


if mode in ("kern_rows", "kern_rows_conc", "kern_fold"):
    rho, u, conc = rand(N, N), rand(2, N, N) - 1.0, rand(N, N)
    table = torch.zeros((17, N), dtype=torch.float64, device=dev)
    res = torch.zeros(17, dtype=torch.float64, device=dev)
    c = _ptr(conc) if mode == "kern_rows_conc" else None
    for i in range(25):   # 5 warm-up + 20
        if mode == "kern_fold":
            if i == 0:
                lib.diag_rows(_ptr(table), N, 0, _ptr(rho), _ptr(u), c, None, N, N, 0, N, None)
            lib.diag_fold(_ptr(res), _ptr(table), N, 0, N, None)
        else:
            lib.diag_rows(_ptr(table), N, 0, _ptr(rho), _ptr(u), c, None, N, N, 0, N, None)
        sync()
elif mode == "kern_calc_rho":
    f, rho = rand(9, N, N), rand(N, N)
    for i in range(25):
        lib.calc_rho(_ptr(rho), _ptr(f), N, N, None)
        sync()
elif mode == "kern_bgk1":
    sv = pylbm.Solver(lib, pylbm.MODEL_BGK, N, N, pylbm.BgkParams(1.2, 0))
    f = rand(9, N, N) / 9.0
    lib.solver_set_f_soa_dev(sv.h, _ptr(f))
    sv.step(1)
    sv.sync()
    for i in range(25):
        sv.step(1)                        # one launch, no moments: 144 B per node
        sv.sync()
    for i in range(25):
        sv.step(1, record_moments=True)   # one launch with moments: 168 B per node
        sv.sync()
    sv.close()
elif mode in ("wall_new", "wall_parent"):
    sv = pylbm.Solver(lib, pylbm.MODEL_BGK, N, N, pylbm.BgkParams(1.2, 0))
    f = rand(9, N, N) / 9.0
    lib.solver_set_f_soa_dev(sv.h, _ptr(f))
    del f
    sv.step(2, record_moments=True)
    sv.sync()
    times = []
    if mode == "wall_new":
        val = np.empty(17)
        for i in range(23):   # 3 warm-up + 20
            t0 = time.perf_counter()
            lib.solver_diag(sv.h, None, 0, N, _hptr(val), None)
            times.append(time.perf_counter() - t0)
        times = times[3:]
        out["mean_ur"] = val[1] / (float(N) * N)
    else:
        rho_h, u_h = np.empty((N, N)), np.empty((N, N, 2))   # allocated and touched once, outside the timed calls
        rho_h.fill(0.0)
        u_h.fill(0.0)
        for i in range(7):    # 2 warm-up + 5
            t0 = time.perf_counter()
            lib.solver_get_moments_aos(sv.h, _hptr(rho_h), _hptr(u_h))
            t1 = time.perf_counter()
            mean = float(np.sum(u_h[:, :, 0])) / (float(N) * N)
            times.append((time.perf_counter() - t0, t1 - t0))
        out["copy_s_median"] = statistics.median(t[1] for t in times[2:])
        times = [t[0] for t in times[2:]]
        out["mean_ur"] = mean
    out["wall_s_median"] = statistics.median(times)
    out["wall_s_min"], out["wall_s_max"], out["n"] = min(times), max(times), len(times)
    sv.close()
elif mode in ("run_new", "run_parent"):
    sv = poiseuille(N)
    STEPS = 1000

    def run_new(steps):
        return sv.run_until(pylbm.Converge(), steps)

    rho_h, u_h = np.zeros((N, N)), np.zeros((N, N, 2))

    def run_parent(steps):   # the driver's loop (horizontal_poiseuille_test.cpp:66-79) on preallocated host arrays
        t, old, mean = 0, 1.0, 1.0
        while t < steps:
            if t % 100 == 1:
                mean = float(np.sum(u_h[:, :, 0])) / (float(N) * N)
                if old != 0.0 and abs(mean / old - 1.0) < 1e-12:
                    break
                old = mean
            n = min(1 if t == 0 else t + 100, steps) - t
            sv.step(n, record_moments=True)
            lib.solver_get_moments_aos(sv.h, _hptr(rho_h), _hptr(u_h))
            t += n
        return t, False, mean

    run = run_new if mode == "run_new" else run_parent
    run(201)          # forced warm-up: every launch shape and both check paths
    sv.sync()
    times = []
    for rep in range(3):
        t0 = time.perf_counter()
        r = run(STEPS)
        sv.sync()
        times.append(time.perf_counter() - t0)
    out["steps"], out["last_value"] = r[0], r[2]
    out["wall_s_median"], out["wall_s_all"] = statistics.median(times), times
    out["mlups_median"] = N * N * STEPS / statistics.median(times) / 1e6
    sv.close()
else:
    raise SystemExit(f"unknown mode {mode}")
print("RESULT " + json.dumps(out), flush=True)
