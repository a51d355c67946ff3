"""What mh_search_hits costs over mh_search, and against the walk it replaces.

"cmu440" over [0, 2^32), one process, every path warmed, then alternating rounds
search, hits at 2^64 // 10^9, hits at 2^64 // 10^6 (cap 4,096), search, ...: the host clock runs
around calls that end in a synchronise, so every path sees the same clock and the same neighbours.
The existing alternative -- minehip.search_first from the last answer plus 1 until the end of the
range, one whole search per hit -- runs fewer rounds (it takes seconds at 10^-6), between the others.
Per path: median, interquartile range, min and max of the wall time, the rounds, and the kernels'
time from the library's HIP events (summed over the launches of one call, in a run of its own).

What the numbers are read for (DESIGN.md §3 "Every hit"): hits / search at the sparse target,
beside the run-to-run spread of the search timings of the same run -- (max - min) / median and
IQR / median; a ratio whose distance from 1 is below that spread is not resolved by this run.

    python tools/hits_search.py [--rounds 15] [--walk-rounds 3] [--out profiles/hits_search.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitcoin-miner_amd")]
import minehip  # noqa: E402

MSG, LO, HI, CAP = b"cmu440", 0, 2 ** 32 - 1, 4096
TARGETS = (("sparse_1e9", 2 ** 64 // 10 ** 9), ("k6_1e6", 2 ** 64 // 10 ** 6))


def stats(ts):
    s = sorted(ts)
    q = lambda f: s[min(len(s) - 1, int(f * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_ms": round(q(0.5) * 1e3, 3), "iqr_ms": round((q(0.75) - q(0.25)) * 1e3, 3),
            "min_ms": round(s[0] * 1e3, 3), "max_ms": round(s[-1] * 1e3, 3), "rounds": len(s)}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def kernel_ms(fn):
    minehip.profile_enable(0, True)
    fn()
    p = minehip.profile_read(0)
    minehip.profile_enable(0, False)
    return round((p["fast_ns"] + p["generic_ns"]) / 1e6, 3)


def walk(target):
    """Every hit of the range by repeated first-hit searches; returns (hits, calls)."""
    hits, calls, lo = [], 0, LO
    while lo <= HI:
        found, h, n, _ = minehip.search_first(MSG, lo, HI, target)
        calls += 1
        if not found:
            break
        hits.append((n, h))
        lo = n + 1
    return hits, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--walk-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits_search.json"))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    paths = {"search": lambda: minehip.search(MSG, LO, HI)}
    for name, t in TARGETS:
        paths["hits_" + name] = lambda t=t: minehip.search_hits(MSG, LO, HI, t, CAP)
    walks = {"walk_" + name: (lambda t=t: walk(t)) for name, t in TARGETS}
    for _ in range(2):  # warm every path (code objects, buffers)
        got = {name: fn() for name, fn in paths.items()}
    got.update({name: fn() for name, fn in walks.items()})
    out = {"msg": MSG.decode(), "lower": LO, "upper": HI, "cap": CAP, "paths": {}}
    for name, t in TARGETS:  # the paths agree before anything is timed
        count, hits, mn = got["hits_" + name]
        assert mn == got["search"] and (count > CAP or (hits, count) == (got["walk_" + name][0], len(hits))), name
        out["paths"]["hits_" + name] = {"target": t, "count": count, "stored": len(hits)}
        out["paths"]["walk_" + name] = {"target": t, "search_first_calls": got["walk_" + name][1]}
    out["paths"]["search"] = {}
    t = {name: [] for name in list(paths) + list(walks)}
    for r in range(a.rounds):
        for name, fn in paths.items():
            t[name].append(timed(fn)[0])
        if r < a.walk_rounds:
            for name, fn in walks.items():
                t[name].append(timed(fn)[0])
    for name, ts in t.items():
        out["paths"][name].update(stats(ts))
        out["paths"][name]["kernel_ms"] = kernel_ms(paths.get(name) or walks[name])
    s = out["paths"]["search"]
    out["search_spread"] = {"range_over_median": round((s["max_ms"] - s["min_ms"]) / s["median_ms"], 4),
                            "iqr_over_median": round(s["iqr_ms"] / s["median_ms"], 4)}
    for name, _ in TARGETS:
        h, w = out["paths"]["hits_" + name], out["paths"]["walk_" + name]
        h["over_search"] = round(h["median_ms"] / s["median_ms"], 4)
        h["over_search_kernel"] = round(h["kernel_ms"] / s["kernel_ms"], 4)
        h["inside_search_spread"] = abs(h["over_search"] - 1.0) <= out["search_spread"]["range_over_median"]
        w["over_hits"] = round(w["median_ms"] / h["median_ms"], 2)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
