"""One RANK of a fluid + scalar slab ring with a KBC fluid, run as a process of its own (tests/proc_util.py run_ranks) by
tests/test_gpu_ade_kbc_slabs.py:

    python tests/ade_kbc_ring_rank.py <rank> <nranks> <workdir>

<workdir> holds cfg.json, id.bin (the 128 bytes of lbm_ring_unique_id_ex, peer-mapped transport) and the global
pre-collision lattices f0.npy, g0.npy (dense SoA [9][R x nranks][C]).  The rank takes its rows, builds the GLOBAL
interior-wall table from cfg["segments"] (r0, c0, dr, dc, n, slots -- f and g alike, rule cfg["g_mode"], cfg["conc"];
none: no table) and takes its view (lbm_ade_iwalls_slab), runs lbm_ring_ade_collide_m and max(cfg["steps"]) x
lbm_ring_ade_step_m with the lbm_ade_fluid of cfg (s2, form), and writes out_<rank>.npz: the owned rows of f and g,
post-collision, SoA, after each step count of cfg["steps"] (f_<n>, g_<n>), and the node count of the view.
Case "refusals": one rank without neighbours on a ghost-2 slab; the messages of the two ring entry points.
Every compute call goes through the C ABI."""
import ctypes as ct
import json
import os
import sys

import numpy as np

from proc_util import rank_prologue


def refusals(lib, ident, R, C, fluid, sc):
    import torch
    import pylbm
    from pylbm import _ptr
    geom = pylbm.Geom(R, C, 2)
    ring = ct.c_void_p()
    lib.ring_create_ex(ct.byref(ring), ident, 0, 1, ct.byref(geom), 0, pylbm.RING_IPC)
    lat = [torch.zeros(9 * (R + 4) * C, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    bc = pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK)
    msgs = []
    for call in (lambda: lib.ring_ade_collide_m(ring, *[_ptr(t) for t in lat], ct.byref(bc), ct.byref(fluid), ct.byref(sc), None, None),
                 lambda: lib.ring_ade_step_m(ring, *[_ptr(t) for t in lat], ct.byref(bc), ct.byref(fluid), ct.byref(sc), None, None,
                                             8, None)):
        try:
            call()
            msgs.append("accepted")
        except pylbm.LbmError as e:
            msgs.append(str(e))
    lib.ring_destroy(ring)
    return dict(msgs=json.dumps(msgs))


def main():
    rank, n, work, cfg, ident = rank_prologue(sys.argv)
    import torch
    import pylbm
    from pylbm import _ptr

    lib = pylbm.Lib()
    d = torch.device("cuda:0")
    R, C, G = cfg["R"], cfg["C"], 1
    fluid = pylbm.AdeFluid(pylbm.KbcParams(cfg["s2"], cfg["form"]))
    sc = pylbm.AdeParams(cfg["omega_g"], tuple(cfg["w"]), form=cfg["form"])
    if cfg.get("case") == "refusals":
        np.savez(os.path.join(work, f"out_{rank}.npz"), **refusals(lib, ident, R, C, fluid, sc))
        return 0

    geom = pylbm.Geom(R, C, G)
    bc = pylbm.Bc.from_buffer_copy(bytes.fromhex(cfg["bc"]))
    table = view = None  # one global table per process, never finalized: only its view is used
    if cfg.get("segments"):
        table = pylbm.AdeInteriorWalls(lib, R * n, C)
        for r0, c0, dr, dc, cnt, slots in cfg["segments"]:
            table.add(r0, c0, dr, dc, cnt, slots, slots, cfg["g_mode"], cfg["conc"])
        view = table.slab(rank * R, R).finalize()

    def zeros():
        return torch.zeros((9, R + 2 * G, C), dtype=torch.float64, device=d)

    pre = [zeros(), zeros()]
    for k, name in enumerate(("f0", "g0")):
        pre[k][:, G:G + R] = torch.from_numpy(np.load(os.path.join(work, name + ".npy"))[:, rank * R:(rank + 1) * R]).to(d)
    lat = [[zeros(), zeros()], [zeros(), zeros()]]  # [time level][f, g]
    ring = ct.c_void_p()
    lib.ring_create_ex(ct.byref(ring), ident, rank, n, ct.byref(geom), int(cfg["closed"]), pylbm.RING_IPC)
    prm = (ct.byref(bc), ct.byref(fluid), ct.byref(sc))
    lib.ring_ade_collide_m(ring, _ptr(lat[0][0]), _ptr(lat[0][1]), _ptr(pre[0]), _ptr(pre[1]), *prm, None, None)
    out, cur = {}, 0
    for t in range(1, max(cfg["steps"]) + 1):
        lib.ring_ade_step_m(ring, _ptr(lat[cur ^ 1][0]), _ptr(lat[cur ^ 1][1]), _ptr(lat[cur][0]), _ptr(lat[cur][1]), *prm, None,
                            view.h if view is not None else None, cfg["edge_rows"], None)
        cur ^= 1
        if t in cfg["steps"]:
            torch.cuda.synchronize()
            lib.ring_status(ring)
            out[f"f_{t}"] = lat[cur][0][:, G:G + R].cpu().numpy()
            out[f"g_{t}"] = lat[cur][1][:, G:G + R].cpu().numpy()
    torch.cuda.synchronize()
    lib.ring_status(ring)
    out["nodes"] = view.count() if view is not None else 0
    lib.ring_destroy(ring)
    np.savez(os.path.join(work, f"out_{rank}.npz"), **out)
    if view is not None:
        view.close()
        table.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
