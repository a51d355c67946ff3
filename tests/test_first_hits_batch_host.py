"""The host side of mh_search_first_hits_batch under AddressSanitizer and UndefinedBehaviorSanitizer
(CPU, no GPU touched): tests/host/first_hits_batch_host.cpp, a stand-alone program with its own main,
replays the pass planning (plan_first_hits_batch_pass), the table image first_hits_batch_run_pass
copies to the device (build_first_hits_batch_image: words, items, order tables and slices offsets),
the table and image checks, and the host's reading of a pass (read_first_hits_batch: the sort,
stored, the minimum of k and the `cursor > slots` decision) over the shapes of
tests/test_gpu_first_hits_batch.py and a seeded fuzz of requests, k values and window sizes -- one
writer per slot; every item's bound, cursor, region and slices are its request's; the slices of
different requests do not overlap; corrupted tables and images are refused."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT, PKG


def test_tables_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "first_hits_batch_host")
    csrc = os.path.join(PKG, "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out,
           os.path.join(ROOT, "tests", "host", "first_hits_batch_host.cpp"), os.path.join(csrc, "plan.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out, "440", "120"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    # the run was about what it claims: passes with fast items, several windows, regions cut short,
    # drains, fallbacks, and both outcomes of the host's reading
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.strip().splitlines()[-1])}
    assert got["passes"] >= 100 and got["fast_passes"] >= 30 and got["items"] >= 100 and got["fallbacks"] > 0
    assert got["windows"] > 10 and got["cut"] > 10 and got["drains"] > 10
    assert got["rebuilds"] > 50 and got["answered"] > 50
