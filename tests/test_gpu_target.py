"""GPU: the proof-of-work question end to end -- Target Requests through the server loop with GPU
miners (mh_miner_handle answers a chunk with its first hit), the batched miner step on mixed
payloads, and mh_search_first_multi -- against brute force on small ranges.  Bit-exact."""
import json

import pytest

from oracle import oracle
from target_cases import EXTRA, FIXTURES, FIXTURE_ANSWERS, FIXTURE_MINIMA, T3, T6, T9, U64, brute_first

pytestmark = pytest.mark.gpu

CASES = FIXTURES + EXTRA


def run_cluster(gpu, jobs, miners=(10, 11, 12), lose=None, **opts):
    """tests/test_gpu_server.py's run_cluster with Target clients: serve `jobs` [(client, msg, lo, hi,
    target or None)] with GPU miners; `lose` = a miner that dies (without answering) holding its first
    chunk.  Returns {client: (hash, nonce)}, the server's stats and its target-job stats."""
    v = gpu.Server(**opts)
    for m in miners:
        v.read(m, gpu.marshal(gpu.NewJoin()))
    for c, msg, lo, hi, t in jobs:
        v.read(c, gpu.marshal(gpu.NewRequest(msg, lo, hi) if t is None else gpu.NewTargetRequest(msg, lo, hi, t)))
    results, t, lost = {}, 0, False
    pending = v.writes()
    while pending:
        conn, payload = pending.pop(0)
        t += 1
        if conn == lose and lost:
            continue                          # written to the miner before it was lost (depth > 1)
        if conn in miners:
            if conn == lose:
                lost = True
                v.lost(conn, now=t)           # dies holding this chunk
            else:
                v.read(conn, gpu.miner_handle(payload), now=t)
        else:
            m = json.loads(payload)
            assert m["Type"] == 2 and "Target" not in m
            results[conn] = (m["Hash"], m["Nonce"])
        pending += v.writes()
    return results, v.stats(), v.first_stats()


@pytest.mark.parametrize("depth", [None, 8])
def test_target_jobs_through_the_server(gpu, depth):
    jobs = [(c + 1, *case) for c, case in enumerate(CASES)] + [(9, b"cmu440", 0, 999_999, None)]
    res, st, fs = run_cluster(gpu, jobs, lose=11, depth=depth, init_chunk=50_000, min_chunk=20_000, max_chunk=100_000)
    for c, msg, lo, hi, t in jobs:
        want = oracle.search(msg, lo, hi, threads=8) if t is None else brute_first(msg, lo, hi, t)
        assert res[c] == want, c
    assert res[1] == FIXTURE_ANSWERS[0] and res[2] == FIXTURE_ANSWERS[1] and res[3] == FIXTURE_ANSWERS[2]
    assert st["jobs_done"] == len(jobs) and st["jobs"] == 0
    assert fs["jobs_first"] == len(CASES) and fs["jobs_found"] == sum(res[c + 1][0] <= CASES[c][3] for c in range(len(CASES)))


def handle(gpu, payload, devs=(0,)):
    """miner_handle's Result payload, or the code it fails with."""
    try:
        return gpu.miner_handle(payload, devs=devs)
    except gpu.MinehipError as e:
        return e.code


def test_miner_handle_answers_a_target_chunk_with_its_first_hit(gpu):
    msg, _, _, t = FIXTURES[0]
    for lo, hi in ((300_000, 399_999), (0, 99_999), (0, 1_999_999)):  # a hit chunk, a no-hit chunk, the range
        found, h, n, _ = gpu.search_first(msg, lo, hi, t)
        assert (h, n) == brute_first(msg, lo, hi, t) and found == (h <= t)
        want = gpu.marshal(gpu.NewResult(h, n))
        assert gpu.miner_handle(gpu.marshal(gpu.NewTargetRequest(msg, lo, hi, t))) == want
        assert gpu.miner_handle(gpu.marshal(gpu.NewTargetRequest(msg, lo, hi, t)), devs=(0, 0)) == want
    # without the key: the minimum, as always
    assert gpu.miner_handle(gpu.marshal(gpu.NewRequest(msg, 300_000, 399_999))) == \
        gpu.marshal(gpu.NewResult(*oracle.search(msg, 300_000, 399_999)))


def mixed_payloads(gpu):
    R, T = gpu.NewRequest, gpu.NewTargetRequest
    msgs = [T(b"cmu440", 300_000, 399_999, T6), R(b"cmu440", 300_000, 399_999), T(b"cmu440", 0, 99_999, T6),
            T(b"cmu440", 0, 299_999, T3), gpu.NewJoin(), R(b"x" * 60, 10 ** 9 - 5_000, 10 ** 9 + 300_000),
            T(b"x" * 60, 10 ** 9 - 5_000, 10 ** 9 + 300_000, T3), T(b"a" * 100, U64 - 200_000, U64, T3),
            R(b"q", 9, 1), T(b"q", 9, 1, 5), T(b"cmu440", 0, 20_000_000, T6), R(b"", 7, 7), T(b"", 7, 7, U64)]
    return [gpu.marshal(m) for m in msgs]


@pytest.mark.parametrize("fuse_fast", [False, True])
def test_miner_handle_batch_on_mixed_payloads(gpu, fuse_fast):
    payloads = mixed_payloads(gpu)
    want = [handle(gpu, p) for p in payloads]
    assert want[4] == gpu.MH_ENOTREQ and want[8] == want[9] == gpu.MH_ERANGE
    # [300000, 399999] holds one hit, which is also its minimum; [0, 299999] has 285, and the first is not the minimum
    assert want[0] == gpu.marshal(gpu.NewResult(*FIXTURE_ANSWERS[0])) == want[1]
    assert want[3] == gpu.marshal(gpu.NewResult(*FIXTURE_ANSWERS[2])) != gpu.marshal(gpu.NewResult(*FIXTURE_MINIMA[2]))
    got = gpu.miner_handle_batch(payloads, fuse_fast=fuse_fast)
    assert [g.code if isinstance(g, gpu.MinehipError) else g for g in got] == want
    # a list with only Target payloads, and one with a single payload
    only = [p for p in payloads if b"Target" in p]
    got = gpu.miner_handle_batch(only, fuse_fast=fuse_fast)
    assert [g.code if isinstance(g, gpu.MinehipError) else g for g in got] == [handle(gpu, p) for p in only]
    assert gpu.miner_handle_batch(payloads[:1], fuse_fast=fuse_fast) == want[:1]


@pytest.mark.parametrize("fuse_fast", [False, True])
def test_miner_handle_batch_without_a_target_is_unchanged(gpu, fuse_fast):
    payloads = [p for p in mixed_payloads(gpu) if b"Target" not in p]
    got = gpu.miner_handle_batch(payloads, fuse_fast=fuse_fast)
    assert [g.code if isinstance(g, gpu.MinehipError) else g for g in got] == [handle(gpu, p) for p in payloads]
    assert got[0] == gpu.marshal(gpu.NewResult(*oracle.search(b"cmu440", 300_000, 399_999)))


@pytest.mark.parametrize("stop_running", [False, True])
@pytest.mark.parametrize("case", range(len(FIXTURES)))
def test_search_first_multi(gpu, case, stop_running):
    msg, lo, hi, t = FIXTURES[case]
    found, h, n, _ = gpu.search_first(msg, lo, hi, t)
    assert (h, n) == FIXTURE_ANSWERS[case]
    for devs in ([0], [0, 0, 0]):
        for chunk in (100_000, 0):
            f, fh, fn, scanned = gpu.search_first_multi(msg, lo, hi, t, devs=devs, chunk=chunk, stop_running=stop_running)
            assert (f, fh, fn) == (found, h, n), (devs, chunk)
            if found:
                assert n - lo + 1 <= scanned <= hi - lo + 1, (devs, chunk, scanned)
            else:
                assert scanned == hi - lo + 1, (devs, chunk, scanned)
            if case == 0 and devs == [0] and chunk == 100_000:
                # one worker takes the chunks in order and the hit is in the fourth: nothing above it runs
                assert scanned <= 400_000, scanned


def test_search_first_multi_failure_hand_back(gpu):
    """A worker whose device fails hands its chunk back and the others finish with the same answer; if
    the only worker fails, the call fails (the dev build's MINEHIP_TEST_FAIL_WORKER, in a child process)."""
    from conftest import run_dev
    msg, lo, hi, t = FIXTURES[0]
    r = run_dev(f"""
import os, minehip
os.environ["MINEHIP_TEST_FAIL_WORKER"] = "1"
print(*minehip.search_first_multi("cmu440", {lo}, {hi}, {t}, devs=[0, 0, 0], chunk=100000))
print(*minehip.search_first_multi("cmu440", {lo}, {hi}, {T9}, devs=[0, 0, 0], chunk=100000))
os.environ["MINEHIP_TEST_FAIL_WORKER"] = "0"   # the only worker fails
try:
    minehip.search_first_multi("cmu440", {lo}, {hi}, {t}, devs=[0], chunk=100000)
    raise SystemExit("search_first_multi succeeded with its only worker failing")
except minehip.MinehipError as e:
    assert e.code == minehip.MH_EHIP and "injected" in str(e), e
""")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.strip().splitlines()[-2:]]
    assert (lines[0][0], int(lines[0][1]), int(lines[0][2])) == ("True",) + FIXTURE_ANSWERS[0]
    assert (lines[1][0], int(lines[1][1]), int(lines[1][2])) == ("False",) + FIXTURE_ANSWERS[1]
    assert int(lines[1][3]) == hi - lo + 1
