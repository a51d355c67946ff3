"""The host tables of mh_search_first_batch_ex(MH_BATCH_FUSE_FAST) under AddressSanitizer and
UndefinedBehaviorSanitizer (CPU, no GPU touched): tests/host/first_batch_fast_host.cpp, a
stand-alone program with its own main, replays build_first_batch_tables_ex and
first_batch_tables_ex_ok (csrc/plan.cpp) over the shapes of tests/test_gpu_first_batch_fast.py and a
seeded fuzz of request lists -- one writer per slot, every item's request owns its slots, the
scanned counts of a request's tiles and chunks sum to its size (at the top of u64 as well),
chunk_floor_host equals the chunk's smallest nonce by enumeration for the last-digit and the Early
layouts, and tables corrupted on purpose are refused."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT, PKG


def test_tables_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "first_batch_fast_host")
    csrc = os.path.join(PKG, "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out,
           os.path.join(ROOT, "tests", "host", "first_batch_fast_host.cpp"), os.path.join(csrc, "plan.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out, "440", "40"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    # the run was about what it claims: several passes, fast items, both layout families, fallbacks
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.strip().splitlines()[-1])}
    assert got["passes"] >= 10 and got["items"] >= 50 and got["fallbacks"] > 0
    assert got["early_chunks"] > 100 and got["last_digit_chunks"] > 1000
