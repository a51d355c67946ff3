"""End to end over real LSP/UDP with a deep queue: bin/minehip-server with MINEHIP_QUEUE_DEPTH=8,
12 concurrent bin/minehip-client processes with small Requests, and three CPU miners
(tests/e2e_oracle_miner.py).  The clients connect first, so their Requests wait at the server; the
first miner to join is then handed 8 chunks at once, answers one and vanishes on its second Request
with the 7 it still holds.  Every client must print the oracle's Result: the server queues several
clients' chunks on each miner, matches the miners' Results to them in order, checks each against
the host Hash, and hands the lost miner's whole queue to the others.  That the lost miner held
several chunks -- which only a depth above 1 can produce -- shows in the server's count of requeued
chunks.  The GPU form is tests/test_gpu_queue.py."""
import os
import re
import select
import subprocess
import time

import pytest

from oracle import oracle
from test_e2e_cluster import BIN, ENV, ORACLE_MINER, PY, free_udp_port

SIZES = [1_000, 200_000, 57_123, 9_999, 10_000, 150_001, 2_560, 2_561, 99_999, 100_000, 31_337, 4_242]


def start_server(port, env, stderr, timeout=20.0):
    """minehip-server on `port`, once it has printed its listening line (within `timeout` seconds:
    a server that prints nothing fails the test instead of hanging it)."""
    srv = subprocess.Popen([os.path.join(BIN, "minehip-server"), str(port)], stdout=subprocess.PIPE, stderr=stderr,
                           env=env, text=True)
    try:
        ready, _, _ = select.select([srv.stdout], [], [], timeout)
        assert ready, "minehip-server printed nothing"
        assert srv.stdout.readline().strip() == f"Server listening on port {port}"
    except BaseException:
        srv.kill()
        srv.wait()
        raise
    return srv


def test_twelve_clients_three_miners_one_dropped(tmp_path):
    port = free_udp_port()
    hp = f"127.0.0.1:{port}"
    env = dict(ENV, MINEHIP_QUEUE_DEPTH="8")
    jobs = [(f"queue-{k:02d}", n) for k, n in enumerate(SIZES)]
    exp = {msg: oracle.search(msg, 0, n, threads=8) for msg, n in jobs}
    procs = []
    err_path = str(tmp_path / "server.err")
    try:
        with open(err_path, "w") as serr:
            procs.append(start_server(port, env, serr))
            clients = []
            for msg, n in jobs:
                c = subprocess.Popen([os.path.join(BIN, "minehip-client"), hp, msg, str(n)], stdout=subprocess.PIPE,
                                     stderr=subprocess.PIPE, env=env, text=True)
                procs.append(c)
                clients.append((msg, c))
            time.sleep(0.5)  # every Request is at the server before the first miner joins
            for drop in (2, 0, 0):  # the first to join takes 8 chunks, answers one, and is gone
                procs.append(subprocess.Popen([PY, ORACLE_MINER, hp] + ([str(drop)] if drop else []),
                                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, env=env))
                time.sleep(0.3 if drop else 0.0)
            got = {msg: c.communicate(timeout=120)[0].strip() for msg, c in clients}
        err = open(err_path).read()
        assert got == {msg: f"Result {h} {n}" for msg, (h, n) in exp.items()}, err[-2000:]
        # the dropped miner was seen through LSP, and it held several chunks when it went: with one
        # chunk per miner (depth 1, or a depth that never reached the scheduler) this count is 1
        requeued = [int(x) for x in re.findall(r"lost; chunks requeued so far (\d+)", err)]
        assert requeued and max(requeued) >= 2, err[-2000:]
    finally:
        for p in procs:  # exactly the processes started here, by PID
            if p.poll() is None:
                p.kill()
            p.wait()


@pytest.mark.parametrize("name,value", [("MINEHIP_QUEUE_DEPTH", "0"), ("MINEHIP_QUEUE_DEPTH", "65"),
                                        ("MINEHIP_QUEUE_DEPTH", "eight"), ("MINEHIP_QUEUE_DEPTH", ""),
                                        ("MINEHIP_QUEUE_NS", "-5")])
def test_server_refuses_bad_queue_settings(name, value):
    r = subprocess.run([os.path.join(BIN, "minehip-server"), str(free_udp_port())], capture_output=True, text=True,
                       timeout=30, env=dict(ENV, **{name: value}))
    assert r.returncode == 2 and r.stdout.startswith(f"bad {name}"), (r.returncode, r.stdout, r.stderr)


def test_server_accepts_the_depth_range():
    for value in ("1", "64"):
        srv = start_server(free_udp_port(), dict(ENV, MINEHIP_QUEUE_DEPTH=value, MINEHIP_QUEUE_NS="1000000"),
                           subprocess.DEVNULL)
        srv.kill()
        srv.wait()
