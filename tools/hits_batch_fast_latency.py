"""Hits requests with fast pieces in a batch: search_hits_batch(fuse_fast=True) against the
fallback loop it replaces.

One process, every path warmed, then alternating rounds (each round in a shuffled order, fixed seed)
over three variants of the same requests:

  a  minehip.search_hits_batch(reqs): fuse_fast off -- a request with a fast piece is a fallback,
     one mh_search_hits after the other (the behaviour before mh_search_hits_batch_ex); the baseline
  b  minehip.search_batch(ranges, fuse_fast=True): the plain minimum scan of the same ranges, i.e.
     the cost of the append with nothing to append where the target is 0
  c  minehip.search_hits_batch(reqs, fuse_fast=True)

64 distinct "cmu440-NN" messages over [0, nonces - 1] with nonces = 3 * 10^6, 10^7, 10^8, and 8 over
10^9; per size the targets 2^64 // 10^3, 2^64 // 10^6 and 0 (nothing qualifies); cap = 4096 per
request.  Where a request has more hits than its cap (`truncated`), both a and c scan it a second
time to rebuild the list, as the calls document.  One more case: a single request of 10^7 nonces,
search_hits against search_hits_batch(fuse_fast=True) of that one request.  The host clock runs
around calls that end in a synchronise.  Per case: medians and interquartile ranges and the kernels'
summed time of each variant from the library's HIP events.  MINEHIP_BATCH_FAST_MAX is lifted for the
run, so every size is measured fused whatever the cap.

What the numbers are read for (DESIGN.md §3 "Batched hits with fused fast pieces"):
  fixed cost   c against a: the fallback loop pays every call's reset, launches, merge, copy-back
               and synchronise
  append       c against b at target 0
  cap          a size at which c is slower than a by more than a's own interquartile range gives the
               hits call a lower cap of its own, at the largest size below it (`cap_rule`)

    python tools/hits_batch_fast_latency.py [--rounds 15] [--out profiles/hits_batch_fast_latency.json]
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

# (name, requests, nonces each)
SIZES = (("k64_3e6", 64, 3 * 10 ** 6), ("k64_1e7", 64, 10 ** 7), ("k64_1e8", 64, 10 ** 8), ("k8_1e9", 8, 10 ** 9))
TARGETS = (("k3", 2 ** 64 // 10 ** 3), ("k6", 2 ** 64 // 10 ** 6), ("zero", 0))
CAP = 4096


def quartiles(ts):
    s = sorted(ts)
    q = lambda f: s[min(len(s) - 1, int(f * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_ms": round(q(0.5) * 1e3, 4), "iqr_ms": round((q(0.75) - q(0.25)) * 1e3, 4),
            "min_ms": round(s[0] * 1e3, 4)}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def kernel_ms(fn):
    minehip.profile_enable(0, True)
    before = minehip.profile_read(0)
    fn()
    p = minehip.profile_read(0)
    minehip.profile_enable(0, False)
    return round((p["fast_ns"] + p["generic_ns"] - before["fast_ns"] - before["generic_ns"]) / 1e6, 4)


def plan_summary(ranges):
    plan = minehip.batch_plan_ex(ranges)
    fast = [p for p in plan if p["kind"] == 2]
    return {"fused_requests": len({p["req"] for p in plan if p["kind"] != 1}),
            "fallbacks": sum(p["kind"] == 1 for p in plan), "passes": 1 + max(p["pass"] for p in plan),
            "chunks": sum(p["slots"] for p in fast), "tiles": sum(p["slots"] for p in plan if p["kind"] == 0),
            "lo_digits": sorted({p["lo_digits"] for p in fast}),
            "launches": len({(p["pass"], p["launch"]) for p in fast})}


def measure(variants, rounds):
    """Alternating rounds over the variants, each round in a shuffled order: none always follows the
    same one.  {name: quartiles + kernel_ms}."""
    t = {name: [] for name in variants}
    names, rng = list(variants), random.Random(440)
    for _ in range(rounds):
        rng.shuffle(names)
        for name in names:
            dt, _ = timed(variants[name])
            t[name].append(dt)
    res = {}
    for name, ts in t.items():
        res[name] = quartiles(ts)
        res[name]["kernel_ms"] = kernel_ms(variants[name])
    return res


def run_case(k, nonces, target, rounds):
    ranges = [("cmu440-%02d" % i, 0, nonces - 1) for i in range(k)]
    reqs = [r + (target,) for r in ranges]
    variants = {"a": lambda: minehip.search_hits_batch(reqs, CAP),
                "b": lambda: minehip.search_batch(ranges, fuse_fast=True),
                "c": lambda: minehip.search_hits_batch(reqs, CAP, fuse_fast=True)}
    got = {}
    for _ in range(3):  # warm every path
        for name, fn in variants.items():
            got[name] = fn()
    assert got["a"] == got["c"], "the variants differ"
    assert all(g[2] == m for g, m in zip(got["c"], got["b"])), "the minimum differs from search_batch's"
    res = {"requests": k, "nonces_each": nonces, "target": target, "cap": CAP, "rounds": rounds,
           "hits": sum(g[0] for g in got["c"]), "truncated": sum(g[0] > CAP for g in got["c"]),
           "plan": plan_summary(ranges)}
    res.update(measure(variants, rounds))
    res["c"]["speedup_vs_a"] = round(res["a"]["median_ms"] / res["c"]["median_ms"], 3)
    res["c"]["over_b"] = round(res["c"]["median_ms"] / res["b"]["median_ms"], 3)
    res["c"]["not_slower_than_a"] = res["c"]["median_ms"] <= res["a"]["median_ms"] + res["a"]["iqr_ms"]
    return res


def run_single(nonces, target, rounds):
    req = ("cmu440-00", 0, nonces - 1, target)
    variants = {"single": lambda: minehip.search_hits(*req, CAP),
                "batch_of_one": lambda: minehip.search_hits_batch([req], CAP, fuse_fast=True)}
    got = {}
    for _ in range(3):
        for name, fn in variants.items():
            got[name] = fn()
    assert [got["single"]] == got["batch_of_one"], "the variants differ"
    res = {"requests": 1, "nonces_each": nonces, "target": target, "cap": CAP, "rounds": rounds,
           "hits": got["single"][0], "plan": plan_summary([req[:3]])}
    res.update(measure(variants, rounds))
    res["batch_of_one"]["over_single"] = round(res["batch_of_one"]["median_ms"] / res["single"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits_batch_fast_latency.json"))
    ap.add_argument("--cases", default=",".join(s[0] for s in SIZES) + ",single")
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    os.environ["MINEHIP_BATCH_FAST_MAX"] = str((1 << 64) - 1)
    out = {"cases": {}, "single": {}}
    for size, k, nonces in SIZES:
        if size not in a.cases.split(","):
            continue
        for tname, target in TARGETS:
            name = f"{size}_{tname}"
            out["cases"][name] = run_case(k, nonces, target, a.rounds)
            print(name, json.dumps(out["cases"][name]), flush=True)
    if "single" in a.cases.split(","):
        for tname, target in TARGETS:
            out["single"][f"k1_1e7_{tname}"] = run_single(10 ** 7, target, a.rounds)
            print(f"k1_1e7_{tname}", json.dumps(out["single"][f"k1_1e7_{tname}"]), flush=True)
    c = out["cases"]
    # the cap: the sizes at which the fused call is not slower than the fallback loop, at every target
    by_size = {}
    for r in c.values():
        by_size.setdefault(r["nonces_each"], []).append(r["c"]["not_slower_than_a"])
    ok = {n: all(v) for n, v in by_size.items()}
    out["cap_rule"] = {"c_not_slower_than_a": {n: r["c"]["not_slower_than_a"] for n, r in c.items()},
                       "largest_size_meeting_it": max((n for n, v in ok.items() if v), default=0),
                       "smallest_size_failing_it": min((n for n, v in ok.items() if not v), default=None)}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
