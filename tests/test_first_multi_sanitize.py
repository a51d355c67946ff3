"""Host code under sanitizers (CPU only): mh_search_first_multi's coordinator -- worker threads over
a target job of the scheduler (search_first_chunks in csrc/multi.cpp) -- built with
tests/host/tsan_first_multi.cpp under ThreadSanitizer and under AddressSanitizer + UBSan, with a
stand-in search, failing workers and host threads that do not start."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bitcoin-miner_amd", "csrc")


@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_first_multi_coordinator_under_sanitizers(tmp_path, san):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "tsan_first_multi")
    extra = ["-fno-sanitize-recover=undefined"] if "undefined" in san else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-fsanitize={san}", *extra, "-Wall",
           "-o", out, os.path.join(ROOT, "tests", "host", "tsan_first_multi.cpp"), os.path.join(CSRC, "multi.cpp"),
           os.path.join(CSRC, "plan.cpp"), os.path.join(CSRC, "sched.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    for seed in (440, 7):
        p = subprocess.run([out, str(seed), "150"], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
        assert "failures=0" in p.stdout and "WARNING: ThreadSanitizer" not in p.stderr
