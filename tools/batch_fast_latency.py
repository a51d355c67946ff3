"""Requests with fast pieces in a batch: search_batch(fuse_fast=True) against the parent behaviour.

One process, every path warmed, then alternating rounds (each round in a shuffled order, fixed seed:
a call that follows the loop of single searches starts 0.03 ms later than one that follows a batch)
over four variants of the same requests:

  fused         minehip.search_batch(reqs, fuse_fast=True): every request keeps its own plan's lanes
  fused_shared  the same with MINEHIP_BATCH_FAST_LANES=shared: the batch-aware lane rule
  batch      minehip.search_batch(reqs): fuse_fast off -- a request with a fast piece is a fallback,
             one mh_search after the other (the behaviour before mh_search_batch_ex)
  loop       a loop of minehip.search

The host clock runs around calls that end in a synchronise.  Per workload the medians and
interquartile ranges of all four, and the kernels' summed time of each from the library's HIP events.
MINEHIP_BATCH_FAST_MAX is lifted for the run, so every size is measured fused whatever the cap.

Conditions: at no workload may `fused` be slower than `batch` by more than `batch`'s
own interquartile range, and a single request not slower than `loop` by more than `loop`'s; the
size cap is the largest measured size that still meets the first; the lane rule is the batch-aware
one only if `fused_shared` beats `fused` at 64 x 10^7 without losing at 1 x 10^7.

    python tools/batch_fast_latency.py [--rounds 15] [--out profiles/batch_fast_latency.json]
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
CASES = (("k64_3e6", 64, 3 * 10 ** 6), ("k64_1e7", 64, 10 ** 7), ("k64_1e8", 64, 10 ** 8),
         ("k8_1e9", 8, 10 ** 9), ("k8_1e10", 8, 10 ** 10), ("k1_1e7", 1, 10 ** 7),
         ("k64_1e6_generic", 64, 10 ** 6))


def quartiles(ts):
    s = sorted(ts)
    q = lambda f: s[min(len(s) - 1, int(f * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_ms": round(q(0.5) * 1e3, 4), "iqr_ms": round((q(0.75) - q(0.25)) * 1e3, 4),
            "min_ms": round(s[0] * 1e3, 4)}


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def kernel_ns(fn):
    minehip.profile_enable(0, True)
    before = minehip.profile_read(0)
    fn()
    p = minehip.profile_read(0)
    minehip.profile_enable(0, False)
    return p["fast_ns"] + p["generic_ns"] - before["fast_ns"] - before["generic_ns"]


def shared_lanes(fn):
    def run():
        os.environ["MINEHIP_BATCH_FAST_LANES"] = "shared"
        try:
            return fn()
        finally:
            del os.environ["MINEHIP_BATCH_FAST_LANES"]
    return run


def plan_summary(reqs):
    plan = minehip.batch_plan_ex(reqs)
    fast = [p for p in plan if p["kind"] == 2]
    return {"fused_requests": len({p["req"] for p in plan if p["kind"] != 1}),
            "fallbacks": sum(p["kind"] == 1 for p in plan), "passes": 1 + max(p["pass"] for p in plan),
            "chunks": sum(p["slots"] for p in fast), "tiles": sum(p["slots"] for p in plan if p["kind"] == 0),
            "lo_digits": sorted({p["lo_digits"] for p in fast}),
            "launches": len({(p["pass"], p["launch"]) for p in fast})}


def run_case(k, nonces, rounds):
    reqs = [("cmu440-%02d" % i, 0, nonces - 1) for i in range(k)]
    fused = lambda: minehip.search_batch(reqs, fuse_fast=True)  # noqa: E731
    variants = {"fused": fused, "fused_shared": shared_lanes(fused), "batch": lambda: minehip.search_batch(reqs),
                "loop": lambda: [minehip.search(*r) for r in reqs]}
    got = {}
    for _ in range(3):  # warm every path
        for name, fn in variants.items():
            got[name] = fn()
    assert got["fused"] == got["fused_shared"] == got["batch"] == got["loop"], "the variants differ"
    t = {name: [] for name in variants}
    names, rng = list(variants), random.Random(440)
    for _ in range(rounds):  # every variant once per round, in a shuffled order: none always follows the same one
        rng.shuffle(names)
        for name in names:
            t[name].append(timed(variants[name])[0])
    res = {"requests": k, "nonces_each": nonces, "rounds": rounds, "plan": plan_summary(reqs),
           "plan_shared": shared_lanes(lambda: plan_summary(reqs))()}
    for name, ts in t.items():
        res[name] = quartiles(ts)
        res[name]["kernel_ms"] = round(kernel_ns(variants[name]) / 1e6, 4)
        res[name]["ghs"] = round(k * nonces / res[name]["median_ms"] / 1e6, 2)
    for v in ("fused", "fused_shared"):
        res[v]["speedup_vs_batch"] = round(res["batch"]["median_ms"] / res[v]["median_ms"], 3)
        res[v]["not_slower_than_batch"] = res[v]["median_ms"] <= res["batch"]["median_ms"] + res["batch"]["iqr_ms"]
        res[v]["not_slower_than_loop"] = res[v]["median_ms"] <= res["loop"]["median_ms"] + res["loop"]["iqr_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_fast_latency.json"))
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    os.environ["MINEHIP_BATCH_FAST_MAX"] = str((1 << 64) - 1)
    out = {"cases": {}}
    for name, k, nonces in CASES:
        if name in a.cases.split(","):
            out["cases"][name] = run_case(k, nonces, a.rounds)
            print(name, json.dumps(out["cases"][name]), flush=True)
    c = out["cases"]
    out["fused_not_slower_than_batch"] = {n: r["fused"]["not_slower_than_batch"] for n, r in c.items()}
    if "k1_1e7" in c:
        out["single_not_slower_than_search"] = c["k1_1e7"]["fused"]["not_slower_than_loop"]
    if "k64_1e7" in c and "k1_1e7" in c:
        a64, a1 = c["k64_1e7"], c["k1_1e7"]
        out["lane_rule"] = "shared" if (a64["fused_shared"]["median_ms"] < a64["fused"]["median_ms"] and
                                        a1["fused_shared"]["median_ms"] <= a1["fused"]["median_ms"] + a1["fused"]["iqr_ms"]) \
            else "own"
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
