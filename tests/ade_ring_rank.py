"""One RANK of a fluid + scalar slab ring, run as a process of its own (tests/proc_util.py run_ranks) by
tests/test_gpu_ade_slabs.py, tests/test_gpu_ade_iwalls_slabs.py, tests/test_gpu_ade_open_slabs.py and
tests/test_gpu_ade_kbc_slabs.py:

    python tests/ade_ring_rank.py <rank> <nranks> <workdir>

<workdir> holds cfg.json, id.bin (the 128 bytes of lbm_ring_unique_id_ex, peer-mapped transport) and the global
pre-collision lattices f0.npy, g0.npy (dense SoA [9][R x nranks][C]).  The rank takes its rows, runs the collide-only call
and max(cfg["steps"]) x the step of cfg["entry"], and writes out_<rank>.npz: the owned rows of f and g, post-collision,
SoA, after each step count of cfg["steps"] (f_<n>, g_<n>), and the node count of its view (0: no table):
  "plain"  lbm_ring_ade_collide / lbm_ring_ade_step; then checks that lbm_ring_exchange_pair refills its ghost rows with
           what the last step's exchange left there (pair_ok).
  "walls"  the GLOBAL interior-wall table from cfg["segments"] (r0, c0, dr, dc, n, slots -- f and g alike, rule
           cfg["g_mode"], cfg["conc"]), its view (lbm_ade_iwalls_slab), lbm_ring_ade_collide_b / lbm_ring_ade_step_w.
  "open"   the GLOBAL open table cfg["table"] (tests/ade_open_util.py build_open), its view (lbm_ade_open_slab),
           lbm_ring_ade_collide_o / lbm_ring_ade_step_o; also writes the view's carry.
  "model"  the fluid by lbm_ade_fluid (KBC with cfg["s2"]; the scalar's rate cfg["omega_g"]), the table of "walls" where
           cfg has segments, lbm_ring_ade_collide_m / lbm_ring_ade_step_m.
Case "refusals": one rank without neighbours on a ghost-2 slab; the messages of the entry's two ring calls ("plain":
and of lbm_ring_exchange_pair).  Every compute call goes through the C ABI (tests/ade_calls.py)."""
import ctypes as ct
import json
import os
import sys

import numpy as np

from proc_util import rank_prologue

CALLS = {"plain": ("lbm_ring_ade_collide", "lbm_ring_ade_step"), "walls": ("lbm_ring_ade_collide_b", "lbm_ring_ade_step_w"),
         "open": ("lbm_ring_ade_collide_o", "lbm_ring_ade_step_o"), "model": ("lbm_ring_ade_collide_m", "lbm_ring_ade_step_m")}


def refusals(lib, ident, R, C, entry, prm):
    import torch
    import pylbm
    from ade_calls import call
    from pylbm import _ptr
    geom = pylbm.Geom(R, C, 2)
    ring = ct.c_void_p()
    lib.ring_create_ex(ct.byref(ring), ident, 0, 1, ct.byref(geom), 0, pylbm.RING_IPC)
    lat = [torch.zeros(9 * (R + 4) * C, dtype=torch.float64, device="cuda:0") for _ in range(4)]
    bc = pylbm.Bc(row_lo=pylbm.EDGE_BOUNCE_BACK, row_hi=pylbm.EDGE_BOUNCE_BACK)
    collide, step = CALLS[entry]
    calls = [lambda: call(lib, collide, rg=ring, dst=lat[:2], src=lat[2:], bc=bc, prm=prm),
             lambda: call(lib, step, rg=ring, dst=lat[:2], src=lat[2:], bc=bc, prm=prm, edge_rows=8)]
    if entry == "plain":
        calls.append(lambda: lib.ring_exchange_pair(ring, _ptr(lat[0]), _ptr(lat[1]), None))
    msgs = []
    for c in calls:
        try:
            c()
            msgs.append("accepted")
        except pylbm.LbmError as e:
            msgs.append(str(e))
    lib.ring_destroy(ring)
    return dict(msgs=json.dumps(msgs))


def main():
    rank, n, work, cfg, ident = rank_prologue(sys.argv)
    import torch
    import pylbm
    from ade_calls import call

    lib = pylbm.Lib()
    d = torch.device("cuda:0")
    R, C, G = cfg["R"], cfg["C"], 1
    entry = cfg["entry"]
    collide, step = CALLS[entry]
    form, w = cfg.get("form", pylbm.FORM_DEFAULT), tuple(cfg.get("w", (0.0, 0.0)))
    fl = pylbm.AdeFluid(pylbm.KbcParams(cfg["s2"], form)) if entry == "model" else pylbm.BgkParams(1.2, 0, form=form)
    prm = (fl, pylbm.AdeParams(cfg.get("omega_g", 1.7), w, form=form))
    if cfg.get("case") == "refusals":
        np.savez(os.path.join(work, f"out_{rank}.npz"), **refusals(lib, ident, R, C, entry, prm))
        return 0

    geom = pylbm.Geom(R, C, G)
    bc = pylbm.Bc.from_buffer_copy(bytes.fromhex(cfg["bc"]))
    table = view = None  # one global table per process, never finalized: only its view is used
    if entry == "open":
        from ade_open_util import build_open
        table = build_open(lib, cfg["table"], R * n, C)
    elif cfg.get("segments"):
        assert entry in ("walls", "model"), entry
        table = pylbm.AdeInteriorWalls(lib, R * n, C)
        for r0, c0, dr, dc, cnt, slots in cfg["segments"]:
            table.add(r0, c0, dr, dc, cnt, slots, slots, cfg["g_mode"], cfg["conc"])
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
    call(lib, collide, rg=ring, dst=lat[0], src=pre, bc=bc, prm=prm, **(dict(view=view, carry_out=carry[0]) if entry == "open" else {}))
    out, cur = {}, 0
    for t in range(1, max(cfg["steps"]) + 1):
        if entry == "open":
            extra = dict(view=view, carry_in=carry[cur], carry_out=carry[cur ^ 1])
        else:
            extra = dict(iwalls=view) if entry != "plain" else {}
        call(lib, step, rg=ring, dst=lat[cur ^ 1], src=lat[cur], bc=bc, prm=prm, edge_rows=cfg["edge_rows"], **extra)
        cur ^= 1
        if t in cfg["steps"]:
            torch.cuda.synchronize()
            lib.ring_status(ring)
            out[f"f_{t}"] = lat[cur][0][:, G:G + R].cpu().numpy()
            out[f"g_{t}"] = lat[cur][1][:, G:G + R].cpu().numpy()
    torch.cuda.synchronize()
    lib.ring_status(ring)
    out["nodes"] = view.count() if view is not None else 0
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
