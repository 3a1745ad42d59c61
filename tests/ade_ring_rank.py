"""One RANK of a fluid + scalar slab ring, run as a process of its own (tests/proc_util.py run_ranks) by
tests/test_gpu_ade_slabs.py, tests/test_gpu_ade_iwalls_slabs.py and tests/test_gpu_ade_open_slabs.py:

    python tests/ade_ring_rank.py <rank> <nranks> <workdir>

<workdir> holds cfg.json, id.bin (the 128 bytes of lbm_ring_unique_id_ex, peer-mapped transport) and the global
pre-collision lattices f0.npy, g0.npy (dense SoA [9][R x nranks][C]).  The rank takes its rows, runs the collide-only call
and cfg["steps"] x the step of cfg["entry"], and writes out_<rank>.npz (owned rows of f and g, post-collision, SoA):
  "plain"  lbm_ring_ade_collide / lbm_ring_ade_step; then checks that lbm_ring_exchange_pair refills its ghost rows with
           what the last step's exchange left there (pair_ok).  Case "refusals": one rank without neighbours on a ghost-2
           slab; the messages of the three ring entry points.
  "walls"  the GLOBAL interior-wall table from cfg["segments"] (r0, c0, dr, dc, n, slots -- f and g alike, rule
           cfg["g_mode"], cfg["conc"]), its view (lbm_ade_iwalls_slab), lbm_ring_ade_collide_b / lbm_ring_ade_step_w;
           also writes the node count of the view.
  "open"   the GLOBAL open table cfg["table"] (tests/ade_open_util.py build_open), its view (lbm_ade_open_slab),
           lbm_ring_ade_collide_o / lbm_ring_ade_step_o; also writes the view's carry and its node count.
Every compute call goes through the C ABI."""
import ctypes as ct
import json
import os
import sys

import numpy as np

from proc_util import rank_prologue


def refusals(lib, ident, R, C):
    import torch
    import pylbm
    from pylbm import _ptr
    geom = pylbm.Geom(R, C, 2)
    ring = ct.c_void_p()
    lib.ring_create_ex(ct.byref(ring), ident, 0, 1, ct.byref(geom), 0, pylbm.RING_IPC)
    lat = [torch.zeros(9 * (R + 4) * C, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    fl, sc = pylbm.BgkParams(1.2, 0), pylbm.AdeParams(1.7, (0.0, 0.0))
    bc = pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK)
    msgs = []
    for call in (lambda: lib.ring_ade_collide(ring, *[_ptr(t) for t in lat], ct.byref(bc), ct.byref(fl), ct.byref(sc), None),
                 lambda: lib.ring_ade_step(ring, *[_ptr(t) for t in lat], ct.byref(bc), ct.byref(fl), ct.byref(sc), 8, None),
                 lambda: lib.ring_exchange_pair(ring, _ptr(lat[0]), _ptr(lat[1]), None)):
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
    if cfg.get("case") == "refusals":
        np.savez(os.path.join(work, f"out_{rank}.npz"), **refusals(lib, ident, R, C))
        return 0

    entry = cfg["entry"]
    geom = pylbm.Geom(R, C, G)
    bc = pylbm.Bc.from_buffer_copy(bytes.fromhex(cfg["bc"]))
    fl = pylbm.BgkParams(1.2, 0, form=cfg["form"])
    sc = pylbm.AdeParams(1.7, tuple(cfg["w"]), form=cfg["form"])

    table = view = None  # one global table per process, never finalized: only its view is used
    if entry == "walls":
        table = pylbm.AdeInteriorWalls(lib, R * n, C)
        for r0, c0, dr, dc, cnt, slots in cfg["segments"]:
            table.add(r0, c0, dr, dc, cnt, slots, slots, cfg["g_mode"], cfg["conc"])
    elif entry == "open":
        from ade_open_util import build_open
        table = build_open(lib, cfg["table"], R * n, C)
    else:
        assert entry == "plain", entry
    if table is not None:
        view = table.slab(rank * R, R).finalize()

    def zeros():
        return torch.zeros((9, R + 2 * G, C), dtype=torch.float64, device=d)

    pre = [zeros(), zeros()]
    for k, name in enumerate(("f0", "g0")):
        pre[k][:, G:G + R] = torch.from_numpy(np.load(os.path.join(work, name + ".npy"))[:, rank * R:(rank + 1) * R]).to(d)
    lat = [[zeros(), zeros()], [zeros(), zeros()]]  # [time level][f, g]
    carry = [torch.zeros(view.carry_len(), dtype=torch.float64, device=d) for _ in range(2)] if entry == "open" else None
    ring = ct.c_void_p()
    lib.ring_create_ex(ct.byref(ring), ident, rank, n, ct.byref(geom), int(cfg["closed"]), pylbm.RING_IPC)
    prm = (ct.byref(bc), ct.byref(fl), ct.byref(sc))
    first = (ring, _ptr(lat[0][0]), _ptr(lat[0][1]), _ptr(pre[0]), _ptr(pre[1]), *prm)
    if entry == "plain":
        lib.ring_ade_collide(*first, None)
    elif entry == "walls":
        lib.ring_ade_collide_b(*first, None, None, None)
    else:
        lib.ring_ade_collide_o(*first, None, None, view.h, _ptr(carry[0]), None)
    cur = 0
    for _ in range(cfg["steps"]):
        step = (ring, _ptr(lat[cur ^ 1][0]), _ptr(lat[cur ^ 1][1]), _ptr(lat[cur][0]), _ptr(lat[cur][1]), *prm)
        if entry == "plain":
            lib.ring_ade_step(*step, cfg["edge_rows"], None)
        elif entry == "walls":
            lib.ring_ade_step_w(*step, None, None, view.h, cfg["edge_rows"], None)
        else:
            lib.ring_ade_step_o(*step, None, None, None, view.h, _ptr(carry[cur]), _ptr(carry[cur ^ 1]), cfg["edge_rows"], None)
        cur ^= 1
    torch.cuda.synchronize()
    lib.ring_status(ring)
    out = {"f": lat[cur][0][:, G:G + R].cpu().numpy(), "g": lat[cur][1][:, G:G + R].cpu().numpy()}
    if view is not None:
        out["nodes"] = view.count()
    if entry == "open":
        out["carry"] = carry[cur].cpu().numpy()
    if entry == "plain":
        out["pair_ok"] = pair_refresh_ok(lib, ring, lat[cur], R, rank, n, bool(cfg["closed"]))
    lib.ring_destroy(ring)
    np.savez(os.path.join(work, f"out_{rank}.npz"), **out)
    if view is not None:
        view.close()
        table.close()
    return 0


def pair_refresh_ok(lib, ring, lat, R, rank, n, closed):
    """a restored state: ghost rows lost, refreshed by lbm_ring_exchange_pair -- the populations that cross each seam
    (cx = +1 into the ghost row above, cx = -1 into the one below) come back as the step's exchange left them"""
    import torch
    from pylbm import _ptr
    has_prev, has_next = closed or rank > 0, closed or rank < n - 1
    planes = {0: [1, 5, 8], R + 1: [3, 6, 7]}
    rows = [r for r, ok in ((0, has_prev), (R + 1, has_next)) if ok]
    saved = [[lat[k][planes[r], r].clone() for r in rows] for k in range(2)]
    for k in range(2):
        for r in (0, R + 1):
            lat[k][:, r] = float("nan")
    lib.ring_exchange_pair(ring, _ptr(lat[0]), _ptr(lat[1]), None)
    lib.ring_join(ring, None)
    torch.cuda.synchronize()
    lib.ring_status(ring)
    return all(torch.equal(lat[k][planes[r], r].view(torch.int64), saved[k][i].view(torch.int64))
               for k in range(2) for i, r in enumerate(rows))


if __name__ == "__main__":
    sys.exit(main())
