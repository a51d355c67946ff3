"""GPU, over real LSP/UDP: minehip-server, two minehip-miner processes and minehip-client with a
target.  One miner runs with MINEHIP_MINER_STOP_RUNNING=1 (Target chunks through the stopping
forms), the other without; the client's answer is a direct search_first's either way."""
import os
import subprocess
import time

import pytest

from test_e2e_cluster import BIN, ENV, free_udp_port

pytestmark = pytest.mark.gpu


def test_target_job_over_lsp_with_gpu_miners(gpu, tmp_path):
    hi = (1 << 32) - 1
    port = free_udp_port()
    hp = f"127.0.0.1:{port}"
    env = dict(ENV, MINEHIP_CHUNK=str(1 << 28))
    procs = []
    try:
        with open(tmp_path / "server.err", "w") as serr:
            srv = subprocess.Popen([os.path.join(BIN, "minehip-server"), str(port)], stdout=subprocess.PIPE,
                                   stderr=serr, env=env, text=True)
            procs.append(srv)
            assert srv.stdout.readline().strip() == f"Server listening on port {port}"
            for stop in ("1", "0"):
                procs.append(subprocess.Popen([os.path.join(BIN, "minehip-miner"), hp], stdout=subprocess.DEVNULL,
                                              stderr=subprocess.DEVNULL,
                                              env=dict(env, MINEHIP_MINER_STOP_RUNNING=stop)))
            time.sleep(0.5)  # let the miners join before the Requests
            err = lambda: open(tmp_path / "server.err").read()[-2000:]  # noqa: E731
            for target in ((1 << 64) // 10 ** 9, (1 << 64) // 10 ** 6, 0):
                found, h, n, _ = gpu.search_first("cmu440", 0, hi, target)
                r = subprocess.run([os.path.join(BIN, "minehip-client"), hp, "cmu440", str(hi), str(target)],
                                   capture_output=True, text=True, timeout=120, env=env)
                assert r.stdout == f"{'First' if found else 'None'} {h} {n}\n", err()
            r = subprocess.run([os.path.join(BIN, "minehip-client"), hp, "cmu440", str(hi)], capture_output=True,
                               text=True, timeout=120, env=env)
            assert r.stdout == "Result %d %d\n" % gpu.search("cmu440", 0, hi), err()
    finally:
        for p in procs:  # exactly the processes started here, by PID
            if p.poll() is None:
                p.kill()
            p.wait()
