"""The proof-of-work question through the scheduler: target jobs of the in-process Server, and
search_first_multi, against a direct search_first over "cmu440", [0, 2^32 - 1].

One process, every path warmed, then alternating rounds; the host clock runs around calls that end
in a synchronise.  Medians and interquartile ranges.  Targets 2^64 // 10^6 and 2^64 // 10^9, and 0,
which nothing meets (the whole range is hashed).

 (a) per target and init_chunk (2^28, and the scheduler's default, 2^30): a target job through
     minehip.Server with one GPU miner that answers every chunk Request with miner_handle -- the
     codec, the scheduler and one first-hit search per chunk -- beside the same range as a plain job
     (mh_search per chunk, the whole range always) and a direct search_first.  `chunks` is how many
     chunk Requests the job took.
 (b) per target: search_first_multi(devs=[0]) and devs=[0, 0] at the default chunk (2^30) against
     search_first, with `scanned` beside each.

Nothing is required of the numbers: the exit code is 0 once every answer matched.

    python tools/first_cluster.py [--rounds 11] [--out profiles/first_cluster.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitcoin-miner_amd")]
import minehip  # noqa: E402

MSG, LO, HI = "cmu440", 0, 2 ** 32 - 1
TARGETS = {"k6": 2 ** 64 // 10 ** 6, "k9": 2 ** 64 // 10 ** 9, "nohit": 0}
CHUNKS = {"chunk_2p28": 1 << 28, "chunk_default": None}


def quartiles(ts):
    s = sorted(ts)
    q = lambda f: s[min(len(s) - 1, int(f * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_ms": round(q(0.5) * 1e3, 4), "iqr_ms": round((q(0.75) - q(0.25)) * 1e3, 4),
            "min_ms": round(s[0] * 1e3, 4)}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def serve(target, init_chunk):
    """One job through a fresh Server and one GPU miner: ((hash, nonce), chunk Requests)."""
    v = minehip.Server(**({} if init_chunk is None else {"init_chunk": init_chunk}))
    v.read(10, minehip.marshal(minehip.NewJoin()))
    req = minehip.NewRequest(MSG, LO, HI) if target is None else minehip.NewTargetRequest(MSG, LO, HI, target)
    v.read(1, minehip.marshal(req), now=time.perf_counter_ns())
    chunks, res = 0, None
    pending = v.writes()
    while pending:
        conn, payload = pending.pop(0)
        if conn == 10:
            chunks += 1
            v.read(10, minehip.miner_handle(payload), now=time.perf_counter_ns())
        else:
            m = minehip.unmarshal(payload)
            res = (m.Hash, m.Nonce)
        pending += v.writes()
    v.close()
    return res, chunks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_cluster.json"))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    size = HI - LO + 1
    direct = lambda T: minehip.search_first(MSG, LO, HI, T)  # noqa: E731
    multi = {"multi_1": lambda T: minehip.search_first_multi(MSG, LO, HI, T, devs=[0]),
             "multi_2": lambda T: minehip.search_first_multi(MSG, LO, HI, T, devs=[0, 0])}
    want, plain_want = {}, minehip.search(MSG, LO, HI)
    for _ in range(2):  # warm: every code object loaded, every kernel of every path run
        for name, T in TARGETS.items():
            want[name] = direct(T)
            for fn in multi.values():
                assert fn(T)[:3] == want[name][:3]
            for c in CHUNKS.values():
                assert serve(T, c)[0] == want[name][1:3]
        for c in CHUNKS.values():
            assert serve(None, c)[0] == plain_want
    t = {name: {k: [] for k in ("direct", *multi, *("job_" + c for c in CHUNKS))} for name in TARGETS}
    sc = {name: {k: [] for k in ("direct", *multi)} for name in TARGETS}
    nchunks = {name: {c: set() for c in CHUNKS} for name in TARGETS}
    t_plain = {c: [] for c in CHUNKS}
    plain_chunks = {c: set() for c in CHUNKS}
    for _ in range(a.rounds):
        for name, T in TARGETS.items():
            for side, fn in (("direct", direct), *multi.items()):
                dt, got = timed(lambda: fn(T))
                assert got[:3] == want[name][:3], (name, side, got, want[name])  # never depends on the timing
                assert (got[2] - LO + 1 if got[0] else size) <= got[3] <= size, (name, side, got)
                t[name][side].append(dt)
                sc[name][side].append(got[3])
            for cname, c in CHUNKS.items():
                dt, (res, k) = timed(lambda: serve(T, c))
                assert res == want[name][1:3], (name, cname, res, want[name])
                t[name]["job_" + cname].append(dt)
                nchunks[name][cname].add(k)
        for cname, c in CHUNKS.items():
            dt, (res, k) = timed(lambda: serve(None, c))
            assert res == plain_want
            t_plain[cname].append(dt)
            plain_chunks[cname].add(k)
    out = {"msg": MSG, "lower": LO, "upper": HI, "rounds": a.rounds, "search_result": list(plain_want),
           "plain_job": {c: dict(quartiles(t_plain[c]), chunks=sorted(plain_chunks[c])) for c in CHUNKS}, "rows": {}}
    for name, T in TARGETS.items():
        found, h, n = want[name][:3]
        row = {"target": T, "found": found, "hash": h, "nonce": n}
        for side in ("direct", *multi):
            row[side] = dict(quartiles(t[name][side]), scanned=[min(sc[name][side]), max(sc[name][side])])
        for c in CHUNKS:
            row["job_" + c] = dict(quartiles(t[name]["job_" + c]), chunks=sorted(nchunks[name][c]))
            row["job_" + c + "_over_direct"] = round(row["job_" + c]["median_ms"] / row["direct"]["median_ms"], 3)
            row["job_" + c + "_over_plain_job"] = round(row["job_" + c]["median_ms"] / out["plain_job"][c]["median_ms"], 3)
        for side in multi:
            row[side + "_over_direct"] = round(row[side]["median_ms"] / row["direct"]["median_ms"], 3)
        out["rows"][name] = row
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
