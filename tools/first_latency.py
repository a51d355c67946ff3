"""mh_search_first against mh_search over "cmu440", [0, 2^32 - 1].

One process, every path warmed, then alternating rounds: the full-range search, the first-hit search
that finds nothing (target 0: it must hash what the search hashes), and per target 2^64 // 10^k the
first-hit search and a plain search of [0, answer] -- the cost of a scan that knew where to stop.
The host clock runs around calls that end in a synchronise.  Medians and interquartile ranges.

Required:
  a. no hit: search_first's median is not above search's by more than search's own interquartile
     range in this run (the per-nonce loops are instruction for instruction the same,
     tests/test_first_guards.py);
  b. every hit case is faster than the full-range search of this run.
The ratio of a hit case to its knew-where-to-stop scan is reported, not required.

    python tools/first_latency.py [--rounds 11] [--out profiles/first_search.json]
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
KS = (4, 6, 8, 9)


def quartiles(ts):
    s = sorted(ts)
    q = lambda f: s[min(len(s) - 1, int(f * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_ms": round(q(0.5) * 1e3, 4), "iqr_ms": round((q(0.75) - q(0.25)) * 1e3, 4),
            "min_ms": round(s[0] * 1e3, 4)}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_search.json"))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    full = lambda: minehip.search(MSG, LO, HI)  # noqa: E731
    nohit = lambda: minehip.search_first(MSG, LO, HI, 0)  # noqa: E731
    for _ in range(2):  # warm: both code objects loaded, every kernel of the plan run
        ref, miss = full(), nohit()
    assert miss == (False,) + ref + (HI - LO + 1,), (miss, ref)
    hits = {}
    for k in KS:
        T = 2 ** 64 // 10 ** k
        r = minehip.search_first(MSG, LO, HI, T)
        if not r[0]:
            continue    # nothing in the range meets so low a target
        assert r[1] <= T and r[3] >= r[2] - LO + 1
        minehip.search(MSG, LO, r[2])
        hits[k] = (T, r)
    t = {"search": [], "first_nohit": []}
    scanned = {k: [] for k in hits}
    for k in hits:
        t["first_k%d" % k], t["stop_k%d" % k] = [], []
    for _ in range(a.rounds):
        t["search"].append(timed(full)[0])
        t["first_nohit"].append(timed(nohit)[0])
        for k, (T, r) in hits.items():
            dt, got = timed(lambda: minehip.search_first(MSG, LO, HI, T))
            assert got[:3] == r[:3], (k, got, r)    # the answer never depends on the timing; scanned may
            t["first_k%d" % k].append(dt)
            scanned[k].append(got[3])
            t["stop_k%d" % k].append(timed(lambda: minehip.search(MSG, LO, r[2]))[0])
    out = {"msg": MSG, "lower": LO, "upper": HI, "rounds": a.rounds, "search_result": list(ref)}
    for name, ts in t.items():
        out[name] = quartiles(ts)
    s, f = out["search"], out["first_nohit"]
    out["nohit"] = {"ratio": round(f["median_ms"] / s["median_ms"], 4),
                    "excess_ms": round(f["median_ms"] - s["median_ms"], 4), "search_iqr_ms": s["iqr_ms"],
                    "within_search_iqr": f["median_ms"] <= s["median_ms"] + s["iqr_ms"]}
    out["hits"] = {}
    ok_b = True
    for k, (T, r) in hits.items():
        fk, sk = out["first_k%d" % k], out["stop_k%d" % k]
        faster = fk["median_ms"] < s["median_ms"]
        ok_b = ok_b and faster
        out["hits"]["k%d" % k] = {"target": T, "hash": r[1], "nonce": r[2], "scanned_min": min(scanned[k]),
                                  "scanned_max": max(scanned[k]), "scanned_over_needed": round(max(scanned[k]) / (r[2] - LO + 1), 3),
                                  "first_ms": fk["median_ms"], "stop_scan_ms": sk["median_ms"],
                                  "ratio_to_stop_scan": round(fk["median_ms"] / sk["median_ms"], 3),
                                  "speedup_over_full": round(s["median_ms"] / fk["median_ms"], 2),
                                  "faster_than_full_search": faster}
    out["required_ok"] = {"a_nohit_within_search_iqr": out["nohit"]["within_search_iqr"], "b_every_hit_faster": ok_b}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0 if all(out["required_ok"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
