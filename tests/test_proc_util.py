"""tests/proc_util.py without a GPU: run_ranks on throw-away rank scripts (standard library and numpy only) that succeed,
fail or outstay the time limit, and run_driver on a stand-in driver in a temporary BIN.  The children are plain CPU
processes that exit or sleep."""
import json
import os
import stat
import sys
import time

import numpy as np
import pytest

import proc_util

# <rank> <n> <workdir>: what every fake rank starts with -- its pid on disk before anything else
RANK_HEAD = """import os, sys, time
rank, n, work = int(sys.argv[-3]), int(sys.argv[-2]), sys.argv[-1]
open(os.path.join(work, f"pid_{rank}"), "w").write(str(os.getpid()))
import numpy as np
"""


class StubLib:
    """lbm_ring_unique_id_ex that fills nothing: no library is loaded"""

    def ring_unique_id_ex(self, ident, transport):
        self.transport = transport


@pytest.fixture
def fake_rank(tmp_path, monkeypatch):
    """write a rank script where run_ranks looks for it"""
    scripts = tmp_path / "scripts"
    scripts.mkdir()
    monkeypatch.setattr(proc_util, "HERE", str(scripts))

    def write(body):
        (scripts / "rank.py").write_text(RANK_HEAD + body)
        return "rank.py"

    return write


def workdir(tmp_path):
    work = tmp_path / "work"
    work.mkdir()
    return work


def gone(pid):
    """the process is no more (run_ranks has waited for it, so no zombie is left either)"""
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return True
    return False


def pids(work, n):
    return [int((work / f"pid_{r}").read_text()) for r in range(n)]


def wait_for_pids(body):
    """a rank that fails or is waited on: not before every rank has written its pid, so that the test can look them all up"""
    return ("while not all(os.path.exists(os.path.join(work, f'pid_{r}')) for r in range(n)):\n"
            "    time.sleep(0.01)\n") + body


def test_all_ranks_succeed(tmp_path, fake_rank):
    import pylbm
    script = fake_rank("np.savez(os.path.join(work, f'out_{rank}.npz'), rank=rank, n=n, extra=sys.argv[1:-3],\n"
                       "         legacy=os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY', 'unset'),\n"
                       "         a=np.load(os.path.join(work, 'a.npy')), cfg=open(os.path.join(work, 'cfg.json')).read())\n")
    work, lib = workdir(tmp_path), StubLib()
    arrays = dict(a=np.arange(6.0).reshape(2, 3), b=np.array([1, 2, 3]))
    outs = proc_util.run_ranks(lib, work, script, 3, dict(R=4, name="x"), arrays, args=("case", 7), timeout=30)
    assert [int(o["rank"]) for o in outs] == [0, 1, 2] and all(int(o["n"]) == 3 for o in outs)
    assert all(str(o["legacy"]) == "0" for o in outs)
    assert all(list(o["extra"]) == ["case", "7"] for o in outs)  # args stand before <rank> <n> <workdir>
    assert json.load(open(work / "cfg.json")) == dict(R=4, name="x") == json.loads(str(outs[0]["cfg"]))
    assert (work / "id.bin").stat().st_size == 128 and lib.transport == pylbm.RING_IPC
    for k, a in arrays.items():
        assert np.array_equal(np.load(work / f"{k}.npy"), a)
    assert np.array_equal(outs[2]["a"], arrays["a"])
    assert all((work / f"rank{r}.log").exists() for r in range(3))


def test_a_failing_rank_ends_the_rest(tmp_path, fake_rank):
    script = fake_rank(wait_for_pids("if rank == 1:\n"
                                     "    print('MARKER rank one gives up', flush=True)\n"
                                     "    sys.exit(3)\n"
                                     "time.sleep(60)\n"))
    work = workdir(tmp_path)
    t0 = time.time()
    with pytest.raises(AssertionError) as e:
        proc_util.run_ranks(StubLib(), work, script, 2, {}, {}, timeout=30, what="the case")
    assert time.time() - t0 < 10
    msg = str(e.value)
    assert msg.startswith("the case: rank(s) [1] failed")
    assert "--- rank 1 (rc 3) ---\nMARKER rank one gives up" in msg
    assert "--- rank 0 (rc -9) ---" in msg  # killed, and said so
    assert all(gone(p) for p in pids(work, 2))


def test_the_time_limit_holds(tmp_path, fake_rank):
    script = fake_rank("time.sleep(60)\n")
    work = workdir(tmp_path)
    t0 = time.time()
    with pytest.raises(AssertionError) as e:
        proc_util.run_ranks(StubLib(), work, script, 2, {}, {}, timeout=1)
    assert time.time() - t0 < 10
    assert str(e.value).startswith("timed out after 1 s")  # no prefix without `what`
    assert all(gone(p) for p in pids(work, 2))


def test_a_rank_that_leaves_no_output_is_an_error_of_its_own(tmp_path, fake_rank):
    """exit 0 without out_<rank>.npz: nothing to report as a failed rank, the load fails"""
    with pytest.raises(FileNotFoundError):
        proc_util.run_ranks(StubLib(), workdir(tmp_path), fake_rank(""), 1, {}, {}, timeout=30)


# ---- run_driver and the parsers ------------------------------------------------------------------------------------------
DRIVER = f"""#!{sys.executable}
import os, sys
print("argv=" + " ".join(sys.argv[1:]))
print("tune=" + os.environ.get("LBM_TUNE", "unset"))
print("cwd=" + os.getcwd())
print("not a key=ignored")
print("plain line")
code = int(sys.argv[1])
if code:
    print("the reason it failed", file=sys.stderr)
else:
    print('{{"check": "fine", "n": 3}}')
sys.exit(code)
"""


@pytest.fixture
def fake_bin(tmp_path, monkeypatch):
    exe = tmp_path / "bin" / "driver"
    exe.parent.mkdir()
    exe.write_text(DRIVER)
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setattr(proc_util, "BIN", str(exe.parent))
    return exe.parent


def test_run_driver_returns_the_process_and_the_parsers_read_it(fake_bin, tmp_path, monkeypatch):
    monkeypatch.delenv("LBM_TUNE", raising=False)
    r = proc_util.run_driver("driver", 0, "--dump", tmp_path / "x", 1.5, timeout=30)
    assert r.returncode == 0
    assert proc_util.last_json(r) == dict(check="fine", n=3)
    kv = proc_util.key_values(r)
    assert kv == dict(argv=f"0 --dump {tmp_path / 'x'} 1.5", tune="unset", cwd=os.getcwd())  # arguments as str(), no "not a key"


def test_run_driver_hands_over_tune_env_and_cwd(fake_bin, tmp_path):
    kv = proc_util.key_values(proc_util.run_driver("driver", 0, timeout=30, tune="a=1", cwd=tmp_path))
    assert kv["tune"] == "a=1" and os.path.samefile(kv["cwd"], tmp_path)
    kv = proc_util.key_values(proc_util.run_driver("driver", 0, timeout=30, env=dict(os.environ, LBM_TUNE="b=2")))
    assert kv["tune"] == "b=2"
    assert proc_util.ipc_env()["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and proc_util.ipc_env()["PATH"] == os.environ["PATH"]


def test_run_driver_checks_the_exit_code_unless_told_not_to(fake_bin):
    with pytest.raises(AssertionError, match="the reason it failed"):
        proc_util.run_driver("driver", 2, timeout=30)
    r = proc_util.run_driver("driver", 2, timeout=30, check=False)
    assert r.returncode == 2 and "the reason it failed" in r.stderr


def test_run_driver_names_a_missing_binary(fake_bin):
    with pytest.raises(AssertionError, match=r"no_such_driver missing: run __graft_entry__\.build\(\)"):
        proc_util.run_driver("no_such_driver", timeout=30)
