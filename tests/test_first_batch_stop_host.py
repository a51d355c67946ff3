"""The `scanned` arithmetic of batch_stop<J, MODE> under AddressSanitizer and
UndefinedBehaviorSanitizer (CPU, no GPU touched): tests/host/first_batch_stop_host.cpp, a stand-alone
program with its own main, replays what the waves add at a chunk's end -- valid lanes x groups run x
10, nothing for a skipped chunk -- over the chunks and waves of pieces with a partial last chunk
(n_runs in {1, 63, 64, 65, 255, 256, 257, 2000}, n_groups in {1, 10, 100}): without a stop the sum is
the piece's nonce count and equals batch_first's up-front adds; with a hit in chunk c it stays
between the nonces of chunks 0..c and the piece's count, whatever the chunks above do."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_scanned_arithmetic_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "first_batch_stop_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out,
           os.path.join(ROOT, "tests", "host", "first_batch_stop_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", r.stdout.strip().splitlines()[-1])}
    # 8 x 3 pieces; 1 + 1 + 1 + 1 + 1 + 1 + 2 + 8 chunks per n_groups; partial and empty waves were met
    assert got["pieces"] == 24 and got["chunks"] == 3 * 16 and got["waves"] == 4 * got["chunks"]
    assert got["partial_waves"] > 0 and got["empty_waves"] > 0 and got["stops"] == 6 * got["chunks"]
