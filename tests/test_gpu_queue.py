"""GPU: a deep per-miner queue end to end -- the server loop at depth 64 hands each GPU miner the
chunks of many small client Requests at once, the miner answers what it holds with one
mh_miner_handle_batch call (one fused pass), and every client's Result is the oracle's.  In
process first (tests/test_gpu_server.py's cluster, with miners that answer their whole queue),
then once over LSP with the real minehip-server, minehip-miner and minehip-client processes.
Bit-exact throughout."""
import json
import os
import random
import subprocess
import time

import pytest

from oracle import oracle
from test_e2e_cluster import BIN, ENV, free_udp_port
from test_e2e_queue import start_server

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
MINERS = (100, 101, 102)
# both sides of mh_search_batch's fused / fallback split, and the 2,560-nonce tile edge
SIZES = (1, 7, 10 ** 4, 2_561, 10 ** 5, 2 * 10 ** 6, 3 * 10 ** 6)


def cluster_jobs():
    """48 jobs of 48 clients: (client, msg, lo, hi), the last one at the top of the u64 range."""
    rng = random.Random(440)
    jobs = []
    for c in range(47):
        lo = rng.choice([0, 0, 0, 1, 999, 10 ** 6 - 3])
        jobs.append((c, b"cmu440-%02d" % c, lo, lo + rng.choice(SIZES) - 1))
    assert {hi - lo + 1 for _, _, lo, hi in jobs} == set(SIZES)
    jobs.append((47, b"cmu440-47", U64 - 10 ** 5 + 1, U64))
    return jobs


_expected = {}


def expected(jobs):
    """The oracle's answers, computed once for the tests of this file."""
    for c, msg, lo, hi in jobs:
        if (msg, lo, hi) not in _expected:
            _expected[(msg, lo, hi)] = oracle.search(msg, lo, hi, threads=8)
    return {c: _expected[(msg, lo, hi)] for c, msg, lo, hi in jobs}


def run_cluster(gpu, jobs, lose=None, fuse_fast=False, **opts):
    """test_gpu_server.run_cluster with miners that collect every payload pending for them and
    answer them with one miner_handle_batch call, Results in order.  `lose` = a miner that dies,
    without answering, the first time it holds several chunks.  Returns {client: (hash, nonce)},
    the server's stats, the largest batch issued and how many chunks the lost miner held."""
    v = gpu.Server(**opts)
    for m in MINERS:
        v.read(m, gpu.marshal(gpu.NewJoin()))
    for c, msg, lo, hi in jobs:
        v.read(c, gpu.marshal(gpu.NewRequest(msg, lo, hi)))
    inbox = {m: [] for m in MINERS}
    results, t, largest, lost_with = {}, 0, 0, 0

    def route():
        for conn, payload in v.writes():
            if conn in MINERS:
                inbox[conn].append(payload)       # a write to a miner that is gone cannot happen
            else:
                m = json.loads(payload)
                assert m["Type"] == 2 and conn not in results
                results[conn] = (m["Hash"], m["Nonce"])

    route()
    while any(inbox.values()):
        for m in MINERS:
            batch = inbox.get(m)
            if not batch:
                continue
            inbox[m] = []
            t += 1000
            if m == lose and not lost_with and len(batch) >= 2:
                lost_with = len(batch)
                del inbox[m]
                v.lost(m, now=t)                  # dies holding all of them
                route()
                continue
            largest = max(largest, len(batch))
            for r in gpu.miner_handle_batch(batch, fuse_fast=fuse_fast, errors="raise"):
                t += 1000
                v.read(m, r, now=t)
                route()
    return results, v.stats(), largest, lost_with


def test_cluster_depth_64_vs_oracle(gpu):
    jobs = cluster_jobs()
    res, st, largest, lost_with = run_cluster(gpu, jobs, lose=101, depth=64)
    assert res == expected(jobs)
    assert largest >= 16 and lost_with >= 2
    assert st["jobs"] == 0 and st["jobs_done"] == 48 and st["chunks_requeued"] == lost_with


def test_cluster_depth_64_fuse_fast(gpu):
    """The same run with miners that fuse fast pieces too, plus 10^7-nonce jobs (fused only with
    fuse_fast), those compared against a direct search."""
    jobs = cluster_jobs()
    big = [(200 + k, b"big-%d" % k, lo, lo + 10 ** 7 - 1) for k, lo in enumerate((0, 5, 10 ** 7, 123_456_789))]
    res, st, largest, lost_with = run_cluster(gpu, jobs + big, lose=102, fuse_fast=True, depth=64)
    exp = expected(jobs)
    exp.update({c: gpu.search(msg, lo, hi) for c, msg, lo, hi in big})
    assert res == exp
    assert largest >= 16 and lost_with >= 2 and st["jobs"] == 0 and st["jobs_done"] == 52


def test_miner_handle_batch_fuse_fast_matches_miner_handle(gpu):
    ps = [gpu.marshal(gpu.NewRequest(b"q-%d" % k, lo, hi)) for k, (lo, hi) in enumerate(
        [(0, 0), (0, 9_999), (7, 2_567), (0, 10 ** 7 - 1), (10 ** 9 - 5, 10 ** 9 + 2 * 10 ** 8),
         (U64 - 10 ** 5, U64), (0, 3 * 10 ** 6 - 1)])]
    ps.insert(2, b"not json")                                       # invalid payload
    ps.insert(4, gpu.marshal(gpu.NewRequest(b"rev", 9, 1)))         # Lower > Upper
    ps.insert(6, gpu.marshal(gpu.NewJoin()))                        # not a Request
    ps.append(gpu.marshal(gpu.NewRequest(b"fallback", 3, 15 * 10 ** 8)))   # above 10^9 nonces: never fused
    one = []
    for p in ps:
        try:
            one.append(gpu.miner_handle(p))
        except gpu.MinehipError as e:
            one.append(e.code)
    for fuse_fast in (True, False):
        got = gpu.miner_handle_batch(ps, fuse_fast=fuse_fast)
        assert [g.code if isinstance(g, gpu.MinehipError) else g for g in got] == one, fuse_fast
    assert one[2] == gpu.MH_ENOTREQ and one[4] == gpu.MH_ERANGE and one[6] == gpu.MH_ENOTREQ
    assert one[-1] == gpu.marshal(gpu.NewResult(*gpu.search(b"fallback", 3, 15 * 10 ** 8)))
    assert one[1] == gpu.marshal(gpu.NewResult(*oracle.search(b"q-1", 0, 9_999)))
    # an unknown flag bit
    import ctypes
    n = ctypes.c_size_t()
    st = ctypes.c_int()
    arr = (ctypes.c_int * 1)(0)
    reqs = (ctypes.c_char_p * 1)(ps[0])
    lens = (ctypes.c_size_t * 1)(len(ps[0]))
    buf = ctypes.create_string_buffer(256)
    assert gpu.lib.mh_miner_handle_batch_ex(arr, 1, reqs, lens, 1, 2, buf, 256, ctypes.byref(n),
                                            ctypes.byref(st)) == gpu.MH_EINVAL


@pytest.mark.parametrize("fuse_fast", [False, True])
def test_over_lsp_miner_batches_queued_requests(gpu, tmp_path, fuse_fast):
    """minehip-server at depth 64, 32 concurrent minehip-client processes of 10^5 nonces each, and
    one minehip-miner (the only process that opens the GPU), which joins once the Requests are at
    the server: every client prints the oracle's Result, and the miner's stats line shows that
    Requests reached it in batches.  Only a lower bound of 2 is asserted: batch sizes over a real
    transport depend on timing.  Every process step has its own timeout."""
    port = free_udp_port()
    hp = f"127.0.0.1:{port}"
    jobs = [(k, b"lsp-%02d" % k, 0, 10 ** 5 - 1) for k in range(32)]
    exp = expected(jobs)
    procs = []
    miner_err = tmp_path / "miner.err"
    try:
        srv = start_server(port, dict(ENV, MINEHIP_QUEUE_DEPTH="64"), open(tmp_path / "server.err", "w"))
        procs.append(srv)
        clients = []
        for c, msg, lo, hi in jobs:
            p = subprocess.Popen([os.path.join(BIN, "minehip-client"), hp, msg.decode(), str(hi)],
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, text=True)
            procs.append(p)
            clients.append((c, p))
        time.sleep(0.5)  # the Requests are at the server before the miner joins
        menv = dict(ENV, MINEHIP_MINER_STATS="1", **({"MINEHIP_MINER_FUSE_FAST": "1"} if fuse_fast else {}))
        miner = subprocess.Popen([os.path.join(BIN, "minehip-miner"), hp], stdout=subprocess.DEVNULL,
                                 stderr=open(miner_err, "w"), env=menv)
        procs.append(miner)
        got = {c: p.communicate(timeout=60)[0].strip() for c, p in clients}
        assert got == {c: f"Result {h} {n}" for c, (h, n) in exp.items()}, open(miner_err).read()[-2000:]
        srv.kill()                 # the miner sees the server go (LSP epochs) and exits with its stats line
        srv.wait(timeout=30)
        assert miner.wait(timeout=30) == 0
        err = open(miner_err).read()
        import re
        m = re.search(r"minehip-miner: requests=(\d+) batches=(\d+) largest=(\d+)", err)
        assert m, err[-2000:]
        requests, batches, largest = (int(x) for x in m.groups())
        assert requests == 32 and batches <= 31 and largest >= 2, err[-2000:]
    finally:
        for p in procs:  # exactly the processes started here, by PID
            if p.poll() is None:
                p.kill()
            p.wait()
