"""The k smallest hits of many requests: search_first_hits_batch against the two ways to the same
answer that existed before it.

One process, every shape warmed, then shuffled rounds (fixed seed) over three variants of the same
requests:

  a  minehip.search_first_hits_batch(reqs, fuse_fast=F): the new call
  b  a loop of minehip.search_first_hits calls, one per request
  c  minehip.search_hits_batch(reqs, cap=k, fuse_fast=F): every nonce of every request is hashed

64 distinct "cmu440-NN" messages over [0, nonces - 1]: nonces = 10^4, 10^5, 10^6 with fuse_fast off,
3 * 10^6, 10^7, 10^8 with fuse_fast on, and 8 messages over 10^9 with fuse_fast on; per shape the
targets 2^64 // 10^3, 2^64 // 10^6 and 0 (nothing qualifies) and k = 1, 4, 16.  Every answer of
every variant in every round is compared with search_hits' (computed once per row: the first k
entries and, with fewer than k hits, the minimum).  The host clock runs around calls that end in a
synchronise.  Per row: medians and interquartile ranges, the share of the nonces the new call
hashed (its `scanned`, last round) and how many requests were answered from the fused pass, fell
back, or were rebuilt (`path` 0, 1, 2).  The file is rewritten after every row.

    python tools/first_hits_batch_latency.py [--rounds 11] [--out profiles/first_hits_batch_latency.json]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitcoin-miner_amd")]
import minehip  # noqa: E402

# (name, requests, nonces each, fuse_fast)
SHAPES = (("k64_1e4", 64, 10 ** 4, False), ("k64_1e5", 64, 10 ** 5, False), ("k64_1e6", 64, 10 ** 6, False),
          ("k64_3e6", 64, 3 * 10 ** 6, True), ("k64_1e7", 64, 10 ** 7, True), ("k64_1e8", 64, 10 ** 8, True),
          ("k8_1e9", 8, 10 ** 9, True))
TARGETS = (("k3", 2 ** 64 // 10 ** 3), ("k6", 2 ** 64 // 10 ** 6), ("zero", 0))
KS = (1, 4, 16)


def quartiles(ts):
    s = sorted(ts)
    q = lambda f: s[min(len(s) - 1, int(f * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_ms": round(q(0.5) * 1e3, 4), "iqr_ms": round((q(0.75) - q(0.25)) * 1e3, 4),
            "min_ms": round(s[0] * 1e3, 4)}


def run_row(n, nonces, fuse, target, k, rounds):
    ranges = [("cmu440-%02d" % i, 0, nonces - 1) for i in range(n)]
    reqs = [r + (target, k) for r in ranges]
    hreqs = [r + (target,) for r in ranges]
    # search_hits' answers: (entries, minimum of the k entries or, with fewer, of the range)
    want = []
    for r in hreqs:
        count, entries, mn = minehip.search_hits(*r, k)
        want.append((entries, mn if count < k else min((h, x) for x, h in entries)))
    last = {}

    def a():
        res = minehip.search_first_hits_batch(reqs, fuse_fast=fuse)
        last["a"] = res
        return [(g[0], g[1]) for g in res]

    def b():
        return [minehip.search_first_hits(*r)[:2] for r in reqs]

    def c():
        res = minehip.search_hits_batch(hreqs, k, fuse_fast=fuse)
        return [(g[1], g[2] if g[0] < k else min((h, x) for x, h in g[1])) for g in res]

    variants = {"a": a, "b": b, "c": c}
    for name, fn in variants.items():       # warm every path of this shape, checked
        assert fn() == want, "variant %s differs from search_hits" % name
    t = {name: [] for name in variants}
    names, rng = list(variants), random.Random(440)
    for _ in range(rounds):
        rng.shuffle(names)
        for name in names:
            t0 = time.perf_counter()
            got = variants[name]()
            t[name].append(time.perf_counter() - t0)
            assert got == want, "variant %s differs from search_hits" % name
    res = {"requests": n, "nonces_each": nonces, "fuse_fast": fuse, "target": target, "k": k, "rounds": rounds,
           "hits_stored": sum(len(w[0]) for w in want),
           "scanned_share": round(sum(g[2] for g in last["a"]) / (n * nonces), 6),
           "paths": [sum(g[3] == p for g in last["a"]) for p in (0, 1, 2)]}
    for name, ts in t.items():
        res[name] = quartiles(ts)
    res["a"]["speedup_vs_b"] = round(res["b"]["median_ms"] / res["a"]["median_ms"], 3)
    res["a"]["speedup_vs_c"] = round(res["c"]["median_ms"] / res["a"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_hits_batch_latency.json"))
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    out = {"rows": {}}
    for name, n, nonces, fuse in SHAPES:
        if name not in a.shapes.split(","):
            continue
        for tname, target in TARGETS:
            for k in KS:
                row = f"{name}_{tname}_k{k}"
                out["rows"][row] = run_row(n, nonces, fuse, target, k, a.rounds)
                print(row, json.dumps(out["rows"][row]), flush=True)
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
                    f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
