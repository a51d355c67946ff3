"""GPU tests of the batched search: mh_search_batch runs many small Requests as tiles of one
batch_scan launch per pass (a lane's unit of work is an aligned decade of ten nonces), folds each
request's slot segment with merge_segments, and sends the requests it does not fuse through the
single-search path.  Bit-exact: every expected value comes from the CPU oracle, and every result is
also what minehip.search gives for the same request."""
import functools
import json
import os
import random
import socket
import subprocess
import sys

import pytest

from oracle import oracle
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
TILE = 2560  # nonces of one tile: 256 lanes x 1 decade x 10


@functools.lru_cache(maxsize=None)
def expected(msg, lo, hi):
    """The oracle's answer, computed once per request of this module."""
    return oracle.search(msg, lo, hi, threads=8)


def check(gpu, reqs, got=None):
    """search_batch(reqs) against the oracle and against search() of every request."""
    if got is None:
        got = gpu.search_batch(reqs)
    assert len(got) == len(reqs)
    for r, g in zip(reqs, got):
        assert g == expected(*r), (r[0][:8], r[1], r[2], g)
        assert g == gpu.search(*r), (r[0][:8], r[1], r[2], g)
    return got


EDGES = [
    (b"cmu440", 0, 0),                                  # the u = 0 decade, one nonce
    (b"cmu440", 7, 7),                                  # a single nonce inside a decade
    (b"cmu440", 0, 9),                                  # exactly one decade
    (b"cmu440", 95, 1005),                              # ragged both ends, crosses 2 -> 3 -> 4 digits
    (b"cmu440", 9, 10),                                 # a digit boundary inside a two-nonce request
    (b"cmu440", 999990000, 1000010000),                 # crosses 9 -> 10 digits
    (b"cmu440", 10 ** 19 - 3000, 10 ** 19 + 3000),      # crosses 19 -> 20 digits
    (b"cmu440", U64 - 5000, U64),                       # the u64 overflow and the short last decade
    (b"cmu440", U64, U64),                              # a single nonce at the top
    (b"", 0, 20000),                                    # empty prefix
    (b"x" * 50, 9990, 10010),                           # t = 51: 4 digits one tail block, 5 digits two
    (b"x" * 60, 0, 99999),                              # two tail blocks throughout
    (b"x" * 64, 0, 20000),                              # host midstate
    (b"x" * 110, 0, 20000),
    (b"cmu440", 95, 1005),                              # the same request twice
    (b"cmu440", 2000, 9000),                            # two ranges of one message
    (b"tile", 0, TILE - 1),                             # exactly one tile
    (b"tile", 0, TILE),                                 # one tile + 1 nonce
    (b"tile", 5, TILE + 4),                             # one tile of nonces over two tiles of decades
]


def test_edges_in_one_call(gpu):
    plan = gpu.batch_plan(EDGES)
    assert all(it["kind"] == 0 and it["pass"] == 0 for it in plan)  # all fused, one pass
    slots = {it["req"]: it["slots"] for it in plan}
    assert (slots[16], slots[17], slots[18]) == (1, 2, 2)
    check(gpu, EDGES)


def fuzz_requests(seed=440, n=200):
    rng = random.Random(seed)
    reqs = []
    for _ in range(n):
        msg = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 131)))
        d = rng.randrange(1, 21)
        lo = rng.randrange(0 if d == 1 else 10 ** (d - 1), min(U64, 10 ** d - 1) + 1)
        reqs.append((msg, lo, min(U64, lo + rng.randrange(1, 3001) - 1)))
    return reqs


def test_fuzz_seed440_one_call(gpu):
    check(gpu, fuzz_requests())


def capacity_requests():
    return [(b"pass%d" % i, 1000 * i, 1000 * i + 29_999) for i in range(40)] + [(b"cmu440", 5, 200_004)]


@pytest.mark.parametrize("slots,passes", [(8, 0), (32, 20)])
def test_passes_and_fallback_by_capacity(gpu, slots, passes):
    """MINEHIP_BATCH_SLOTS (a child process) against the default capacity, same results.  The 40
    requests of 30,000 nonces take 12 tiles each and the one of 200,000 takes 79: with 8 slots no
    pass holds any of them (all fallbacks), with 32 they go two to a pass (20 passes) and the
    large one is a fallback."""
    reqs = capacity_requests()
    got = check(gpu, reqs)
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import json, minehip, test_gpu_batch as t\n"
            "reqs = t.capacity_requests()\n"
            "plan = minehip.batch_plan(reqs)\n"
            f"assert 1 + max(it['pass'] for it in plan) == {passes} and plan[-1]['kind'] == 1, plan[-3:]\n"
            "print(json.dumps(minehip.search_batch(reqs)))\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MINEHIP_BATCH_SLOTS=str(slots)),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert [tuple(x) for x in json.loads(r.stdout.strip().splitlines()[-1])] == got


def test_mixed_sizes_and_order(gpu):
    """[0, 3*10^6] plans a fast piece (a fallback) between small requests, [0, 2*10^6] is fused."""
    reqs = [(b"cmu440", 10, 500), (b"cmu440", 0, 3 * 10 ** 6), (b"abc", 0, 999), (b"cmu440", 0, 2 * 10 ** 6),
            (b"cmu440", 123, 456)]
    kinds = {it["req"]: it["kind"] for it in gpu.batch_plan(reqs)}
    assert kinds == {0: 0, 1: 1, 2: 0, 3: 0, 4: 0}
    check(gpu, reqs)


def test_per_request_errors(gpu):
    reqs = [(b"cmu440", 0, 999), (b"cmu440", 9, 3), (b"cmu440", 1000, 1999)]
    got = gpu.search_batch(reqs, errors="return")
    assert isinstance(got[1], gpu.MinehipError) and got[1].code == gpu.MH_ERANGE and got[1].index == 1
    check(gpu, [reqs[0], reqs[2]], [got[0], got[2]])
    with pytest.raises(gpu.MinehipError) as e:
        gpu.search_batch(reqs)
    assert e.value.code == gpu.MH_ERANGE and e.value.index == 1


def test_profile_counts_batch_in_generic_class(gpu):
    reqs = EDGES[:6]
    gpu.profile_enable(0, True)
    gpu.search_batch(reqs)
    p = gpu.profile_read(0)
    gpu.profile_enable(0, False)
    assert p["generic_nonces"] == sum(hi - lo + 1 for _, lo, hi in reqs) and p["generic_ns"] > 0
    assert p["fast_launches"] == 0


def miner_payloads(gpu, requests=22):
    """`requests` Requests, plus one message that is no Request and one with Lower > Upper."""
    ps = [gpu.marshal(gpu.NewRequest("miner%d" % i, 997 * i, 997 * i + 19_999)) for i in range(requests)]
    ps.insert(5, gpu.marshal(gpu.NewJoin()))
    ps.insert(11, gpu.marshal(gpu.NewRequest("cmu440", 9, 3)))
    return ps


def miner_expected(gpu, payloads):
    out = []
    for p in payloads:
        m = gpu.unmarshal(p)
        if m.Type == gpu.Request and m.Lower <= m.Upper:
            out.append(gpu.marshal(gpu.NewResult(*expected(m.Data, m.Lower, m.Upper))))
    return out


def test_miner_handle_batch_matches_miner_handle(gpu):
    ps = miner_payloads(gpu)
    assert len(ps) == 24
    got = gpu.miner_handle_batch(ps)
    one = []
    for p in ps:
        try:
            one.append(gpu.miner_handle(p))
        except gpu.MinehipError as e:
            one.append(e.code)
    assert [g.code if isinstance(g, gpu.MinehipError) else g for g in got] == one
    assert one[5] == gpu.MH_ENOTREQ and one[11] == gpu.MH_ERANGE
    assert [g for g in got if isinstance(g, bytes)] == miner_expected(gpu, ps)


def test_miner_process_answers_queued_requests_in_order(gpu, tmp_path):
    """minehip-miner against an LSP server that writes 24 Requests (and two messages a miner
    ignores) back to back after the Join: 24 Results come back, in order, equal to the oracle's;
    the ignored messages get no answer."""
    from minehip import lsp
    ps = miner_payloads(gpu, 24)
    want = miner_expected(gpu, ps)
    assert len(want) == 24
    s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    srv, err = lsp.NewServer(port, lsp.Params(5, 200, 32))
    assert err is None, err
    proc = subprocess.Popen([os.path.join(PKG, "bin", "minehip-miner"), f"127.0.0.1:{port}"],
                            env=dict(os.environ, LSP_EPOCH_MILLIS="200", LSP_EPOCH_LIMIT="5", LSP_WINDOW_SIZE="32"),
                            stdout=subprocess.DEVNULL, stderr=open(tmp_path / "miner.err", "w"))
    try:
        conn, payload, err = srv.Read(20_000)
        assert err is None and gpu.unmarshal(payload) == gpu.NewJoin(), (err, payload)
        for p in ps:
            assert srv.Write(conn, p) is None
        got = []
        while len(got) < len(want):
            c, payload, err = srv.Read(30_000)
            assert err is None and c == conn, (err, len(got), open(tmp_path / "miner.err").read()[-2000:])
            got.append(payload)
        assert got == want
    finally:
        srv.Close()
        if proc.poll() is None:
            proc.kill()
        proc.wait()
