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

--stop: mh_search_first_ex(MH_FIRST_STOP_RUNNING) against mh_search_first (flags 0, whose code
objects are the ones from before the flag existed: the yardstick, on the same device in the same run).
Per target 2^64 // 10^k, k in {4, 6, 8, 9}, and target 0 (nothing qualifies: the whole range, the
poll's cost), alternating rounds of flags 0 and the flag; medians, interquartile ranges and the range
of `scanned` on both sides.  Reported per row: whether the flag's median is below flags 0's by more
than both interquartile ranges (k = 6 is the case the flag is for), and for target 0 whether it is
slower by more than the flags-0 spread.  Nothing is required: the exit code is 0 once every answer
matched.

    python tools/first_latency.py --stop [--rounds 11] [--out profiles/first_stop_search.json]
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


def stop_main(a):
    """--stop: flags 0 against MH_FIRST_STOP_RUNNING, one process, alternating rounds."""
    plain = lambda T: minehip.search_first(MSG, LO, HI, T)  # noqa: E731
    stop = lambda T: minehip.search_first(MSG, LO, HI, T, stop_running=True)  # noqa: E731
    rows = {"k%d" % k: 2 ** 64 // 10 ** k for k in KS}
    rows["nohit"] = 0
    want = {}
    for name, T in rows.items():
        for _ in range(2):  # warm: both code objects loaded, every kernel of the plan run
            want[name] = plain(T)
            got = stop(T)
            assert got[:3] == want[name][:3], (name, got, want[name])
    size = HI - LO + 1
    t = {name: {"flags0": [], "stop": []} for name in rows}
    sc = {name: {"flags0": [], "stop": []} for name in rows}
    for _ in range(a.rounds):
        for name, T in rows.items():
            for side, fn in (("flags0", plain), ("stop", stop)):
                dt, got = timed(lambda: fn(T))
                assert got[:3] == want[name][:3], (name, side, got, want[name])   # the answer never depends on the timing
                assert (got[2] - LO + 1 if got[0] else size) <= got[3] <= size, (name, side, got)
                t[name][side].append(dt)
                sc[name][side].append(got[3])
    out = {"msg": MSG, "lower": LO, "upper": HI, "rounds": a.rounds, "rows": {}}
    for name, T in rows.items():
        f0, st = quartiles(t[name]["flags0"]), quartiles(t[name]["stop"])
        found, h, n = want[name][:3]
        row = {"target": T, "found": found, "hash": h, "nonce": n, "flags0": f0, "stop": st,
               "flags0_scanned": [min(sc[name]["flags0"]), max(sc[name]["flags0"])],
               "stop_scanned": [min(sc[name]["stop"]), max(sc[name]["stop"])],
               "stop_over_flags0": round(st["median_ms"] / f0["median_ms"], 4),
               "stop_below_flags0_by_more_than_both_iqr":
                   f0["median_ms"] - st["median_ms"] > max(f0["iqr_ms"], st["iqr_ms"]),
               "stop_above_flags0_by_more_than_flags0_iqr": st["median_ms"] - f0["median_ms"] > f0["iqr_ms"]}
        out["rows"][name] = row
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--stop", action="store_true", help="flags 0 against MH_FIRST_STOP_RUNNING (see above)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "first_stop_search.json" if a.stop else "first_search.json")
    if a.stop:
        return stop_main(a)
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
