"""Over real LSP/UDP: minehip-server, two target-aware CPU miners (tests/e2e_target_miner.py) and
minehip-client with its optional fourth argument, the target, as separate processes on 127.0.0.1.
One cluster serves a client with a hit, one without a hit and a four-argument client."""
import os
import subprocess
import sys
import time

from conftest import ROOT
from test_e2e_cluster import BIN, ENV, free_udp_port

TARGET_MINER = os.path.join(ROOT, "tests", "e2e_target_miner.py")


def client(hp, *args, timeout=120):
    return subprocess.run([os.path.join(BIN, "minehip-client"), hp, *args], capture_output=True, text=True,
                          timeout=timeout, env=ENV)


def test_client_usage_with_a_target():
    r = client("127.0.0.1:1", "m", "9", "x7")
    assert r.returncode == 2 and r.stdout == "x7 is not a number.\n"
    r = client("127.0.0.1:1", "m", "9", "7", "8")
    assert r.returncode == 2 and r.stdout.startswith("Usage: ") and "<maxNonce>" in r.stdout
    r = client("127.0.0.1:1", "m")
    assert r.returncode == 2 and r.stdout.endswith("<hostport> <message> <maxNonce>")  # the usage line is unchanged


def test_target_jobs_over_lsp(tmp_path):
    port = free_udp_port()
    hp = f"127.0.0.1:{port}"
    env = dict(ENV, MINEHIP_CHUNK="100000")
    procs = []
    try:
        with open(tmp_path / "server.err", "w") as serr:
            srv = subprocess.Popen([os.path.join(BIN, "minehip-server"), str(port)], stdout=subprocess.PIPE,
                                   stderr=serr, env=env, text=True)
            procs.append(srv)
            assert srv.stdout.readline().strip() == f"Server listening on port {port}"
            for _ in range(2):
                procs.append(subprocess.Popen([sys.executable, TARGET_MINER, hp], stdout=subprocess.DEVNULL,
                                              stderr=subprocess.DEVNULL, env=env))
            time.sleep(0.5)  # let the miners join before the Requests
            err = lambda: open(tmp_path / "server.err").read()[-2000:]  # noqa: E731
            r = client(hp, "cmu440", "1999999", "18446744073709")
            assert r.stdout == "First 14415379299797 393322\n", err()
            r = client(hp, "cmu440", "1999999", "18446744073")
            assert r.stdout == "None 1228377698034 1067492\n", err()
            r = client(hp, "cmu440", "1999999")
            assert r.stdout == "Result 1228377698034 1067492\n", err()
    finally:
        for p in procs:  # exactly the processes started here, by PID
            if p.poll() is None:
                p.kill()
            p.wait()
