"""First-hit requests with fast pieces in a batch: search_first_batch(fuse_fast=True) against the
fallback loop it replaces.

One process, every path warmed, then alternating rounds (each round in a shuffled order, fixed seed)
over four variants of the same requests:

  a  minehip.search_first_batch(reqs): fuse_fast off -- a request with a fast piece is a fallback,
     one mh_search_first after the other (the behaviour before mh_search_first_batch_ex); the baseline
  b  minehip.search_batch(ranges, fuse_fast=True): the full scan of the same ranges
  c  minehip.search_first_batch(reqs, fuse_fast=True)
  d  the same as c under MINEHIP_FIRST_BATCH_ORDER=request, the identity dispatch order

64 distinct "cmu440-NN" messages over [0, nonces - 1] with nonces = 3 * 10^6, 10^7, 10^8, and 8 over
10^9; per size the targets 2^64 // 10^3, 2^64 // 10^6 and 0 (nothing qualifies).  The host clock
runs around calls that end in a synchronise.  Per case: medians and interquartile ranges, the
kernels' summed time of each variant from the library's HIP events, and the summed `scanned` of c
and d as a share of the nonces.  MINEHIP_BATCH_FAST_MAX is lifted for the run, so every size is
measured fused whatever the cap.

What the numbers are read for (DESIGN.md §3 "Batched first-hit search with fused fast pieces"):
  fixed cost   c against a with hits, where the fallback loop pays every call's fixed cost
  cap          c against a at target 0, where nothing can be skipped: a size at which c is slower
               than a by more than a's own interquartile range gives the first-hit call a lower cap of
               its own, at the largest size below it (`cap_rule`)
  order        c against d with hits, in time and in scanned share

    python tools/first_batch_fast_latency.py [--rounds 15] [--out profiles/first_batch_fast_latency.json]

--stop measures mh_search_first_batch_stop instead (DESIGN.md §3 "Batched first-hit search whose running
chunks stop"): the same sizes and targets, two variants in alternating rounds of one process,

  c  minehip.search_first_batch(reqs, fuse_fast=True): the yardstick, the code objects every earlier
     commit ships
  s  the same call with stop_running=True: batch_stop<J, MODE> for the fast launches

with medians, interquartile ranges, kernel time and the `scanned` share of both.  At target 0
nothing can be skipped, so s against c there is what the poll costs: `poll_rule` says per size
whether s is slower than c by more than c's own interquartile range.

    python tools/first_batch_fast_latency.py --stop [--rounds 15] [--out profiles/first_batch_stop_latency.json]
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


def request_order(fn):
    def run():
        os.environ["MINEHIP_FIRST_BATCH_ORDER"] = "request"  # read per call
        try:
            return fn()
        finally:
            del os.environ["MINEHIP_FIRST_BATCH_ORDER"]
    return run


def plan_summary(ranges):
    plan = minehip.batch_plan_ex(ranges)
    fast = [p for p in plan if p["kind"] == 2]
    return {"fused_requests": len({p["req"] for p in plan if p["kind"] != 1}),
            "fallbacks": sum(p["kind"] == 1 for p in plan), "passes": 1 + max(p["pass"] for p in plan),
            "chunks": sum(p["slots"] for p in fast), "tiles": sum(p["slots"] for p in plan if p["kind"] == 0),
            "lo_digits": sorted({p["lo_digits"] for p in fast}),
            "launches": len({(p["pass"], p["launch"]) for p in fast})}


def run_case(k, nonces, target, rounds):
    ranges = [("cmu440-%02d" % i, 0, nonces - 1) for i in range(k)]
    reqs = [r + (target,) for r in ranges]
    fused = lambda: minehip.search_first_batch(reqs, fuse_fast=True)  # noqa: E731
    variants = {"a": lambda: minehip.search_first_batch(reqs), "b": lambda: minehip.search_batch(ranges, fuse_fast=True),
                "c": fused, "d": request_order(fused)}
    got = {}
    for _ in range(3):  # warm every path
        for name, fn in variants.items():
            got[name] = fn()
    assert [g[:3] for g in got["a"]] == [g[:3] for g in got["c"]] == [g[:3] for g in got["d"]], "the variants differ"
    assert all(g[0] or g[1:3] == m for g, m in zip(got["c"], got["b"])), "not found, yet not the minimum"
    t = {name: [] for name in variants}
    scanned = {"c": [], "d": []}
    names, rng = list(variants), random.Random(440)
    for _ in range(rounds):  # every variant once per round, in a shuffled order: none always follows the same one
        rng.shuffle(names)
        for name in names:
            dt, r = timed(variants[name])
            t[name].append(dt)
            if name in scanned:
                scanned[name].append(sum(g[3] for g in r))
    res = {"requests": k, "nonces_each": nonces, "target": target, "rounds": rounds,
           "found": sum(g[0] for g in got["c"]), "plan": plan_summary(ranges)}
    for name, ts in t.items():
        res[name] = quartiles(ts)
        res[name]["kernel_ms"] = kernel_ms(variants[name])
    for name, ss in scanned.items():
        ss = sorted(ss)
        res[name]["scanned_median"] = ss[len(ss) // 2]
        res[name]["scanned_share"] = round(ss[len(ss) // 2] / (k * nonces), 6)
    res["a"]["scanned_share"] = round(sum(g[3] for g in got["a"]) / (k * nonces), 6)
    res["c"]["speedup_vs_a"] = round(res["a"]["median_ms"] / res["c"]["median_ms"], 3)
    res["d"]["speedup_vs_a"] = round(res["a"]["median_ms"] / res["d"]["median_ms"], 3)
    res["c"]["not_slower_than_a"] = res["c"]["median_ms"] <= res["a"]["median_ms"] + res["a"]["iqr_ms"]
    return res


def run_stop_case(k, nonces, target, rounds):
    """--stop: search_first_batch(fuse_fast=True) against the same call with stop_running=True."""
    ranges = [("cmu440-%02d" % i, 0, nonces - 1) for i in range(k)]
    reqs = [r + (target,) for r in ranges]
    variants = {"c": lambda: minehip.search_first_batch(reqs, fuse_fast=True),
                "s": lambda: minehip.search_first_batch(reqs, fuse_fast=True, stop_running=True)}
    got = {}
    for _ in range(3):  # warm both paths
        for name, fn in variants.items():
            got[name] = fn()
    assert [g[:3] for g in got["c"]] == [g[:3] for g in got["s"]], "the variants differ"
    t = {name: [] for name in variants}
    scanned = {name: [] for name in variants}
    names, rng = list(variants), random.Random(440)
    for _ in range(rounds):  # both once per round, in a shuffled order
        rng.shuffle(names)
        for name in names:
            dt, r = timed(variants[name])
            t[name].append(dt)
            scanned[name].append(sum(g[3] for g in r))
    res = {"requests": k, "nonces_each": nonces, "target": target, "rounds": rounds,
           "found": sum(g[0] for g in got["c"]), "plan": plan_summary(ranges)}
    if res["found"]:  # the nonces a sequential scan would need: up to each request's first hit
        res["needed_share"] = round(sum(g[2] + 1 if g[0] else nonces for g in got["c"]) / (k * nonces), 6)
    for name, ts in t.items():
        res[name] = quartiles(ts)
        res[name]["kernel_ms"] = kernel_ms(variants[name])
        ss = sorted(scanned[name])
        res[name]["scanned_median"] = ss[len(ss) // 2]
        res[name]["scanned_share"] = round(ss[len(ss) // 2] / (k * nonces), 6)
    res["s"]["speedup_vs_c"] = round(res["c"]["median_ms"] / res["s"]["median_ms"], 3)
    res["s"]["not_slower_than_c"] = res["s"]["median_ms"] <= res["c"]["median_ms"] + res["c"]["iqr_ms"]
    return res


def main_stop(a):
    out = {"cases": {}}
    for size, k, nonces in SIZES:
        if size not in a.cases.split(","):
            continue
        for tname, target in TARGETS:
            name = f"{size}_{tname}"
            out["cases"][name] = run_stop_case(k, nonces, target, a.rounds)
            print(name, json.dumps(out["cases"][name]), flush=True)
    zero = {n: r for n, r in out["cases"].items() if n.endswith("_zero")}
    out["poll_rule"] = {"s_not_slower_than_c_at_zero": {n: r["s"]["not_slower_than_c"] for n, r in zero.items()},
                        "s_over_c_at_zero": {n: round(r["s"]["median_ms"] / r["c"]["median_ms"], 4) for n, r in zero.items()}}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default=",".join(s[0] for s in SIZES))
    ap.add_argument("--stop", action="store_true", help="measure search_first_batch(stop_running=True) against fuse_fast=True")
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "first_batch_stop_latency.json" if a.stop else "first_batch_fast_latency.json")
    os.environ["MINEHIP_BATCH_FAST_MAX"] = str((1 << 64) - 1)
    if a.stop:
        return main_stop(a)
    out = {"cases": {}}
    for size, k, nonces in SIZES:
        if size not in a.cases.split(","):
            continue
        for tname, target in TARGETS:
            name = f"{size}_{tname}"
            out["cases"][name] = run_case(k, nonces, target, a.rounds)
            print(name, json.dumps(out["cases"][name]), flush=True)
    c = out["cases"]
    # the cap: the sizes at which, with nothing to skip, the fused call is not slower than the fallback loop
    zero = {n: r for n, r in c.items() if n.endswith("_zero")}
    out["cap_rule"] = {"c_not_slower_than_a_at_zero": {n: r["c"]["not_slower_than_a"] for n, r in zero.items()},
                       "largest_size_meeting_it": max((r["nonces_each"] for r in zero.values()
                                                       if r["c"]["not_slower_than_a"]), default=0),
                       "smallest_size_failing_it": min((r["nonces_each"] for r in zero.values()
                                                        if not r["c"]["not_slower_than_a"]), default=None)}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
