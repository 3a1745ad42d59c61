"""Starting processes from the suite, in one place: the driver binaries (run_driver and the two parsers of what they
print) and the rank processes of a slab ring (run_ranks; rank_prologue is their side of it).  A failing rank ends the
rest and every run has a time limit, so that nothing is left spinning on a shared GPU.  tests/test_proc_util.py holds
this logic to its word without a GPU; no import of this module brings torch or pylbm with it."""
import ctypes as ct
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "lattice-boltzmann-method_amd")
BIN = os.path.join(PKG, "drivers", "bin")


def ipc_env():
    """the environment of a process that opens peer-mapped windows"""
    return dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")


# ---- driver binaries -----------------------------------------------------------------------------------------------------
def run_driver(name, *args, timeout, env=None, cwd=None, tune=None, check=True):
    """BIN/name with the arguments as strings -> its CompletedProcess; check: exit 0 or an AssertionError with the tails
    of what it printed.  tune: LBM_TUNE, the process-wide tuning of the library, through the environment"""
    exe = os.path.join(BIN, name)
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    if tune:
        env = dict(os.environ if env is None else env, LBM_TUNE=tune)
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, cwd=cwd, timeout=timeout, env=env)
    if check:
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def last_json(r):
    """the JSON line a ring driver ends its output with"""
    return json.loads(r.stdout.strip().splitlines()[-1])


def key_values(r):
    """the key=value lines of a driver's output (a key holds no space)"""
    return dict(ln.split("=", 1) for ln in r.stdout.splitlines() if "=" in ln and " " not in ln.split("=")[0])


# ---- rank processes ------------------------------------------------------------------------------------------------------
def run_ranks(lib, tmp_path, script, n, cfg, arrays, *, args=(), timeout, what=None):
    """n processes `python tests/<script> *args <rank> <n> <workdir>` on this GPU over the peer-mapped transport ->
    their out_<rank>.npz.  A failing rank ends the rest, and the whole run has a time limit; either raises an
    AssertionError (prefixed `what`) with every rank's return code and the tail of its log"""
    import pylbm  # here, not above: a rank script reads its prologue from this module before the package is on sys.path
    work = str(tmp_path)
    json.dump(cfg, open(os.path.join(work, "cfg.json"), "w"))
    ident = (ct.c_ubyte * 128)()
    lib.ring_unique_id_ex(ident, pylbm.RING_IPC)
    open(os.path.join(work, "id.bin"), "wb").write(bytes(ident))
    for k, a in arrays.items():
        np.save(os.path.join(work, k + ".npy"), a)
    env = ipc_env()
    procs = []
    for r in range(n):
        log = open(os.path.join(work, f"rank{r}.log"), "w")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, script), *map(str, args), str(r), str(n), work],
                                       stdout=log, stderr=subprocess.STDOUT, env=env), log))
    t0, failed = time.time(), None
    while any(p.poll() is None for p, _ in procs):
        bad = [r for r, (p, _) in enumerate(procs) if p.poll() not in (None, 0)]
        if bad or time.time() - t0 > timeout:
            failed = f"rank(s) {bad} failed" if bad else f"timed out after {timeout} s"
            for p, _ in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.05)
    for p, log in procs:
        p.wait()
        log.close()
    bad = [r for r, (p, _) in enumerate(procs) if p.returncode != 0]
    if failed or bad:
        logs = "\n".join(f"--- rank {r} (rc {procs[r][0].returncode}) ---\n" + open(os.path.join(work, f"rank{r}.log")).read()[-3000:]
                         for r in range(n))
        raise AssertionError(f"{what + ': ' if what else ''}{failed or bad}\n{logs}")
    return [np.load(os.path.join(work, f"out_{r}.npz")) for r in range(n)]


def rank_prologue(argv):
    """a rank script's side of run_ranks: the package on sys.path, then (rank, n, workdir, cfg, the ring's 128-byte id)
    from the last three arguments"""
    for p in (HERE, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    rank, n, work = int(argv[-3]), int(argv[-2]), argv[-1]
    cfg = json.load(open(os.path.join(work, "cfg.json")))
    ident = (ct.c_ubyte * 128).from_buffer_copy(open(os.path.join(work, "id.bin"), "rb").read())
    return rank, n, work, cfg, ident
