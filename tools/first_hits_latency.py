"""mh_search_first_hits against the two other ways to the same answer, over "cmu440", [0, 2^32 - 1].

One process, every path warmed, then alternating rounds.  Per row (a target and a k):
  first_hits  search_first_hits(target, k): the scan that stops once k hits are known;
  hits        search_hits(target, cap=k): the whole range hashed, whatever k is (every row);
  walk        k calls of search_first, each from the last answer plus 1 (rows with k <= 16).
Rows: target 2^64 // 10^6 with k in {1, 4, 16, 256}; 2^64 // 10^9 with k in {1, 2}; and target 0,
where nothing is found: both scans hash the whole range, so the difference is the cost of the poll
and of the claim's extra word.  Every answer is checked against search_hits' in every round.  The
host clock runs around calls that end in a synchronise.  Medians and interquartile ranges, and the
range of `scanned` per row.  Nothing is required (the call is opt-in): the exit code is 0 once every
answer matched; for the nothing-found row the output states whether the difference lies inside
search_hits' own interquartile range.

    python tools/first_hits_latency.py [--rounds 11] [--out profiles/first_hits_search.json]
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
ROWS = [("T6_k%d" % k, 2 ** 64 // 10 ** 6, k) for k in (1, 4, 16, 256)] + \
       [("T9_k%d" % k, 2 ** 64 // 10 ** 9, k) for k in (1, 2)] + [("nohit", 0, 1)]
WALK_MAX_K = 16


def quartiles(ts):
    s = sorted(ts)
    q = lambda f: s[min(len(s) - 1, int(f * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_ms": round(q(0.5) * 1e3, 4), "iqr_ms": round((q(0.75) - q(0.25)) * 1e3, 4),
            "min_ms": round(s[0] * 1e3, 4)}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def walk(T, k):
    """The k smallest hits by k first-hit searches, each from the last answer plus 1."""
    out, lo = [], LO
    while len(out) < k and lo <= HI:
        found, h, n, _ = minehip.search_first(MSG, lo, HI, T)
        if not found:
            break
        out.append((n, h))
        lo = n + 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_hits_search.json"))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    size = HI - LO + 1
    want = {}
    for name, T, k in ROWS:
        for _ in range(2):  # warm: every code object loaded, every kernel of the plan run
            want[name] = minehip.search_hits(MSG, LO, HI, T, k)
            got = minehip.search_first_hits(MSG, LO, HI, T, k)
            assert got[0] == want[name][1], (name, got[0][:3], want[name][1][:3])
            if k <= WALK_MAX_K:
                assert walk(T, k) == want[name][1], name
    t = {name: {"first_hits": [], "hits": [], "walk": []} for name, _, _ in ROWS}
    sc = {name: [] for name, _, _ in ROWS}
    for _ in range(a.rounds):
        for name, T, k in ROWS:
            count, entries, mn = want[name]
            dt, got = timed(lambda: minehip.search_first_hits(MSG, LO, HI, T, k))
            assert got[0] == entries, (name, got[0][:3])              # the answer never depends on the timing
            if count < k:
                assert got[1] == mn and got[2] == size, (name, got[1:])
            else:
                assert got[1] == min((h, n) for n, h in entries) and entries[-1][0] - LO + 1 <= got[2] <= size, (name, got[1:])
            t[name]["first_hits"].append(dt)
            sc[name].append(got[2])
            dt, ref = timed(lambda: minehip.search_hits(MSG, LO, HI, T, k))
            assert ref == want[name], name
            t[name]["hits"].append(dt)
            if k <= WALK_MAX_K:
                dt, w = timed(lambda: walk(T, k))
                assert w == entries, name
                t[name]["walk"].append(dt)
    out = {"msg": MSG, "lower": LO, "upper": HI, "rounds": a.rounds, "rows": {}}
    for name, T, k in ROWS:
        count, entries, mn = want[name]
        fh, hs = quartiles(t[name]["first_hits"]), quartiles(t[name]["hits"])
        row = {"target": T, "k": k, "count": count, "stored": len(entries),
               "last_nonce": entries[-1][0] if entries else None,
               "first_hits": fh, "hits": hs, "scanned": [min(sc[name]), max(sc[name])],
               "hits_over_first_hits": round(hs["median_ms"] / fh["median_ms"], 3)}
        if t[name]["walk"]:
            row["walk"] = quartiles(t[name]["walk"])
            row["walk_over_first_hits"] = round(row["walk"]["median_ms"] / fh["median_ms"], 3)
        if name == "nohit":
            row["excess_ms"] = round(fh["median_ms"] - hs["median_ms"], 4)
            row["difference_within_hits_iqr"] = abs(fh["median_ms"] - hs["median_ms"]) <= hs["iqr_ms"]
        out["rows"][name] = row
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
