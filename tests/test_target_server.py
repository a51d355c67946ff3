"""CPU: the server loop (mh_server_*) with Target and plain clients mixed, served by stub miners
written here.  A target job's chunk Requests all carry its Target and a plain job's carry none; the
clients get plain Results.  And the mixed-cluster caveat, pinned: a miner that ignores the key and
answers chunk minima (as a reference miner would) still gets the job completed, with a qualifying
nonce -- not necessarily the first."""
import json

import pytest

import minehip
from oracle import oracle
from target_cases import FIXTURES, FIXTURE_ANSWERS, T3, U64, brute_first, chunk_answer, hashes


def serve(jobs, miners=(10, 11, 12), lose=None, aware=True, **opts):
    """Serve jobs [(client, msg, lo, hi, target or None)] with stub miners; `lose` = a miner that dies
    holding its first chunk.  aware=False: the stubs ignore Target.  Returns {client: payload}, the
    chunk Requests seen [(Data, Lower, Upper, Target)], the stats and the target-job stats."""
    v = minehip.Server(**opts)
    for m in miners:
        v.read(m, minehip.marshal(minehip.NewJoin()))
    for c, msg, lo, hi, t in jobs:
        v.read(c, minehip.marshal(minehip.NewRequest(msg, lo, hi) if t is None
                                  else minehip.NewTargetRequest(msg, lo, hi, t)))
    results, chunks, t, lost = {}, [], 0, False
    pending = v.writes()
    while pending:
        conn, payload = pending.pop(0)
        t += 1
        if conn == lose and lost:
            continue                      # written to the miner before it was lost (depth > 1)
        if conn in miners:
            r = minehip.unmarshal(payload)
            assert r.Type == minehip.Request
            chunks.append((r.Data, r.Lower, r.Upper, r.Target))
            if conn == lose and not lost:
                lost = True
                v.lost(conn, now=t)
            else:
                ans = chunk_answer(r.Data, r.Lower, r.Upper, r.Target if aware else None)
                v.read(conn, minehip.marshal(minehip.NewResult(*ans)), now=t)
        else:
            assert conn not in results
            results[conn] = payload
        pending += v.writes()
    return results, chunks, v.stats(), v.first_stats()


@pytest.mark.parametrize("depth", [None, 8])
def test_target_and_plain_clients(depth):
    jobs = [(1, *FIXTURES[0]), (2, b"cmu440", 0, 1_999_999, None), (3, *FIXTURES[1]), (4, *FIXTURES[2]),
            (5, b"a" * 100, U64 - 200_000, U64, T3), (6, b"a" * 100, U64 - 200_000, U64, None), (7, b"", 7, 7, 0)]
    for msg, lo, hi in {(j[1], j[2], j[3]) for j in jobs}:
        hashes(msg, lo, hi)
    res, chunks, st, fs = serve(jobs, lose=11, depth=depth, init_chunk=50_000, min_chunk=20_000, max_chunk=100_000)
    for c, msg, lo, hi, t in jobs:
        h, n = oracle.search(msg, lo, hi, threads=4) if t is None else brute_first(msg, lo, hi, t)
        # a plain Result: the six reference keys, no Target
        assert res[c] == minehip.marshal(minehip.NewResult(h, n)), c
        assert set(json.loads(res[c])) == {"Type", "Data", "Lower", "Upper", "Hash", "Nonce"}
    assert json.loads(res[1])["Nonce"] == FIXTURE_ANSWERS[0][1] == 393_322
    # every chunk carries its job's Target, or none: the jobs are told apart by (Data, range, Target)
    want = {(j[1], j[4]) for j in jobs}
    assert {(d, t) for d, lo, hi, t in chunks} == want
    for d, lo, hi, t in chunks:
        assert any(d == j[1] and j[2] <= lo <= hi <= j[3] and t == j[4] for j in jobs)
    assert st["jobs_done"] == len(jobs) and st["jobs"] == 0 and st["idle_miners"] == 2
    assert fs["jobs_first"] == 5 and fs["jobs_found"] == 3 and fs["nonces_dropped"] > 0


def test_miners_that_ignore_target_still_complete_the_job():
    """The caveat of a mixed cluster (include/minehip_server.h): chunk minima instead of first hits.
    The job completes, and with a qualifying nonce; with one miner and fixed chunks the run is
    deterministic: chunk [300000, 399999] holds the hit 393,322, and that chunk's minimum is it or a
    smaller hash of the same chunk."""
    msg, lo, hi, t = FIXTURES[0]
    res, chunks, st, fs = serve([(1, msg, lo, hi, t)], miners=(10,), aware=False, init_chunk=100_000,
                                min_chunk=100_000, max_chunk=100_000)
    m = minehip.unmarshal(res[1])
    assert m.Type == minehip.Result and m.Hash <= t and oracle.hash_(msg, m.Nonce) == m.Hash
    assert (m.Hash, m.Nonce) == chunk_answer(msg, 300_000, 399_999)
    assert [c[1] for c in chunks] == [0, 100_000, 200_000, 300_000] and all(c[3] == t for c in chunks)
    assert st["jobs"] == 0 and fs["jobs_found"] == 1
    # with many hits per chunk the minimum of the first chunk is a hit, but not the first one
    msg, lo, hi, t = FIXTURES[2]
    res, _, _, _ = serve([(1, msg, lo, hi, t)], miners=(10,), aware=False, init_chunk=100_000, min_chunk=100_000,
                         max_chunk=100_000)
    m = minehip.unmarshal(res[1])
    assert m.Hash <= t and (m.Hash, m.Nonce) == chunk_answer(msg, 0, 99_999) != brute_first(msg, lo, hi, t)


def test_refused_target_request():
    v = minehip.Server()
    with pytest.raises(minehip.MinehipError) as e:
        v.read(1, minehip.marshal(minehip.NewTargetRequest("x", 9, 1, 5)))
    assert e.value.code == minehip.MH_EREJECTED
    with pytest.raises(minehip.MinehipError) as e:
        v.read(1, b'{"Type":1,"Data":"x","Lower":0,"Upper":9,"Target":-1}')
    assert e.value.code == minehip.MH_EINVAL
    assert v.first_stats()["jobs_first"] == 0 and v.stats()["jobs"] == 0
