"""The scheduler's chunk queues and the server loop over them under AddressSanitizer +
UndefinedBehaviorSanitizer (CPU only, host code only).

tests/host/fuzz_queue.cpp is a stand-alone program: compiled here with g++
-fsanitize=address,undefined together with plan.cpp, sched.cpp, server.cpp and message.cpp (as
tests/test_host_sanitize.py builds fuzz_host.cpp) and run directly.  It drives
mh_sched_create_ex / mh_server_create_ex at random depths with random join / submit / next /
result / lose / drop sequences and checks coverage, FIFO order and the guard (see its header)."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bitcoin-miner_amd", "csrc")
SRCS = [os.path.join(CSRC, f) for f in ("plan.cpp", "sched.cpp", "server.cpp", "message.cpp")]
DRIVER = os.path.join(ROOT, "tests", "host", "fuzz_queue.cpp")


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("asan_queue") / "fuzz_queue")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out, DRIVER] + SRCS
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


@pytest.mark.parametrize("seed", [440, 1, 2])
def test_queue_fuzz_under_sanitizers(fuzz_bin, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_bin, str(seed), "60"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "failures=0" in r.stdout
    # the run was not trivial: Results completed, skipping miners rejected, deep queues formed
    m = re.search(r"results=(\d+) rejected=(\d+) deepest=(\d+)", r.stdout)
    assert m and int(m.group(1)) > 2000 and int(m.group(2)) > 20 and int(m.group(3)) >= 16, r.stdout
