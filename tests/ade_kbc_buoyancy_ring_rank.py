"""One RANK of a fluid + scalar slab ring with the fluid by model AND buoyancy, run as a process of its own
(tests/proc_util.py run_ranks) by tests/test_gpu_ade_kbc_buoyancy_slabs.py:

    python tests/ade_kbc_buoyancy_ring_rank.py <rank> <nranks> <workdir>

<workdir> holds cfg.json, id.bin (the 128 bytes of lbm_ring_unique_id_ex, peer-mapped transport) and the global
pre-collision lattices f0.npy, g0.npy (dense SoA [9][R x nranks][C]).  The rank takes its rows, runs
lbm_ring_ade_slab_collide_mb and max(cfg["steps"]) x lbm_ring_ade_slab_step_mb with a KBC fluid (cfg["s2"], cfg["form"]),
the scalar cfg["omega_g"], cfg["w"], the descriptor cfg["buoy"] = [beta_r, beta_c, c_ref, u_shift] and, where cfg has
segments, the view of the GLOBAL interior-wall table (r0, c0, dr, dc, n, slots -- f and g alike, rule cfg["g_mode"],
cfg["conc"]); it writes out_<rank>.npz: the owned rows of f and g, post-collision, SoA, after each step count of
cfg["steps"] (f_<n>, g_<n>), and the node count of its view.  Every compute call goes through the C ABI
(tests/ade_kbc_buoyancy_slab_calls.py)."""
import ctypes as ct
import os
import sys

import numpy as np

from proc_util import rank_prologue


def main():
    rank, n, work, cfg, ident = rank_prologue(sys.argv)
    import torch
    import pylbm
    from ade_kbc_buoyancy_slab_calls import RING_COLLIDE, RING_STEP, call

    lib = pylbm.Lib()
    d = torch.device("cuda:0")
    R, C, G = cfg["R"], cfg["C"], 1
    form = cfg["form"]
    prm = (pylbm.AdeFluid(pylbm.KbcParams(cfg["s2"], form)), pylbm.AdeParams(cfg["omega_g"], tuple(cfg["w"]), form=form))
    b = cfg["buoy"]
    buoy = pylbm.AdeBuoyancy((b[0], b[1]), b[2], b[3])
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
    call(lib, RING_COLLIDE, rg=ring, dst=lat[0], src=pre, bc=bc, prm=prm, buoy=buoy)
    out, cur = {}, 0
    for t in range(1, max(cfg["steps"]) + 1):
        call(lib, RING_STEP, rg=ring, dst=lat[cur ^ 1], src=lat[cur], bc=bc, prm=prm, buoy=buoy, iwalls=view,
             edge_rows=cfg["edge_rows"])
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
