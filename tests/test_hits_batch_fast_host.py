"""The host side of mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST) under AddressSanitizer and
UndefinedBehaviorSanitizer (CPU, no GPU touched): tests/host/hits_batch_fast_host.cpp, a stand-alone
program with its own main, replays the pass planning (plan_hits_batch_pass_ex), the table image
hits_batch_run_pass_ex builds and the table checks (hits_batch_tables_ex_ok, csrc/plan.cpp) over the
shapes of tests/test_gpu_hits_batch_fast.py and a seeded fuzz of requests, caps and window sizes --
one writer per slot, every item's cursor and region are its request's, the regions of a window are
disjoint and inside the buffer, a request's tiles and chunks count each nonce once (at the top of
u64 as well), and tables corrupted on purpose are refused."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT, PKG


def test_tables_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "hits_batch_fast_host")
    csrc = os.path.join(PKG, "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out,
           os.path.join(ROOT, "tests", "host", "hits_batch_fast_host.cpp"), os.path.join(csrc, "plan.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out, "440", "40"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    # the run was about what it claims: passes with fast items, several windows, regions cut short,
    # fallbacks, and a drain forced by the table buffer
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.strip().splitlines()[-1])}
    assert got["passes"] >= 20 and got["fast_passes"] >= 10 and got["items"] >= 50 and got["fallbacks"] > 0
    assert got["windows"] > 5 and got["cut"] > 5 and got["table_drains"] > 0
