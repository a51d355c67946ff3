"""Many small first-hit searches: a loop of minehip.search_first (a), one minehip.search_batch of
the same ranges -- the full scan -- (b), one minehip.search_first_batch (c), and the same under
MINEHIP_FIRST_BATCH_ORDER=request, the identity dispatch order (d).

One process, every path warmed, then alternating rounds a, b, c, d, a, ...: the host clock runs
around calls that end in a synchronise.  64 distinct "cmu440-NN" messages over [0, nonces - 1] with
nonces = 10^4, 10^5, 10^6, and per size the targets 2^64 // 10^k for k = 3, 4, 6 and 0 (nothing
found).  Per case: medians and interquartile ranges, the kernel time of b, c and d from the
library's HIP events (generic class), and the summed `scanned` of c and d as a share of the nonces.
The `b_abi` / `c_abi` rows time b and c through the C-ABI with the arguments built beforehand, i.e.
without the Python wrapper's per-request work.

What the numbers are read for (DESIGN.md §3 "Batched first-hit search"):
  fixed cost      c against a at 64 x 10^4 and 64 x 10^5, every target (reported, `c_faster_than_a`)
  first-hit cost  c against b at target 0, where nothing can be skipped
  dispatch order  c against d with hits, in time and in scanned share

    python tools/first_batch_latency.py [--rounds 15] [--out profiles/first_batch_latency.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitcoin-miner_amd")]
import minehip  # noqa: E402

K = 64
SIZES = (("k64_1e4", 10 ** 4), ("k64_1e5", 10 ** 5), ("k64_1e6", 10 ** 6))
TARGETS = (("k3", 2 ** 64 // 10 ** 3), ("k4", 2 ** 64 // 10 ** 4), ("k6", 2 ** 64 // 10 ** 6), ("zero", 0))


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
    fn()
    p = minehip.profile_read(0)
    minehip.profile_enable(0, False)
    return round((p["fast_ns"] + p["generic_ns"]) / 1e6, 4)


def request_order(fn):
    def run():
        os.environ["MINEHIP_FIRST_BATCH_ORDER"] = "request"  # read per call
        try:
            return fn()
        finally:
            del os.environ["MINEHIP_FIRST_BATCH_ORDER"]
    return run


def run_case(nonces, target, rounds):
    reqs = [("cmu440-%02d" % i, 0, nonces - 1, target) for i in range(K)]
    plain = [r[:3] for r in reqs]
    paths = {"a_loop_first": lambda: [minehip.search_first(*r) for r in reqs],
             "b_batch_full": lambda: minehip.search_batch(plain),
             "c_first_batch": lambda: minehip.search_first_batch(reqs)}
    paths["d_first_batch_request_order"] = request_order(paths["c_first_batch"])
    # b and c through the C-ABI alone, the arguments built beforehand: without the Python wrapper's
    # per-request work (tools/batch_latency.py's `abi` rows)
    arr_b, keep_b = minehip._requests(plain)
    out_b = (minehip.mh_result * K)()
    arr_c = (minehip.mh_first_request * K)()
    for i, (m, lo, hi, tg) in enumerate(reqs):
        arr_c[i].msg, arr_c[i].len, arr_c[i].lower, arr_c[i].upper, arr_c[i].target = keep_b[i], len(keep_b[i]), lo, hi, tg
    out_c = (minehip.mh_first_result * K)()
    paths["b_abi"] = lambda: minehip._check(minehip.lib.mh_search_batch(0, arr_b, K, out_b))
    paths["c_abi"] = lambda: minehip._check(minehip.lib.mh_search_first_batch(0, arr_c, K, out_c))
    for _ in range(3):  # warm every path
        got = {name: fn() for name, fn in paths.items()}
    key = lambda rs: [r[:3] for r in rs]  # noqa: E731
    assert key(got["a_loop_first"]) == key(got["c_first_batch"]) == key(got["d_first_batch_request_order"]), \
        "search_first_batch differs from search_first"
    t = {name: [] for name in paths}
    scanned = {"c_first_batch": [], "d_first_batch_request_order": []}
    for _ in range(rounds):
        for name, fn in paths.items():
            dt, r = timed(fn)
            t[name].append(dt)
            if name in scanned:
                scanned[name].append(sum(x[3] for x in r))
    res = {"requests": K, "nonces_each": nonces, "target": target, "rounds": rounds,
           "found": sum(1 for r in got["c_first_batch"] if r[0]),
           "fused": all(it["kind"] == 0 for it in minehip.batch_plan(plain))}
    for name, ts in t.items():
        res[name] = quartiles(ts)
        if name[0] in "bcd" and not name.endswith("_abi"):
            res[name]["kernel_ms"] = kernel_ms(paths[name])
    for name, ss in scanned.items():
        res[name]["scanned_share"] = round(sorted(ss)[len(ss) // 2] / (K * nonces), 4)
    a, b, c, d = (res[n] for n in list(paths)[:4])
    res["c_over_b_abi"] = round(res["c_abi"]["median_ms"] / res["b_abi"]["median_ms"], 3)
    res["a_over_c"] = round(a["median_ms"] / c["median_ms"], 3)
    res["c_faster_than_a"] = c["median_ms"] < a["median_ms"]
    res["c_over_b"] = round(c["median_ms"] / b["median_ms"], 3)
    res["c_over_b_kernel"] = round(c["kernel_ms"] / b["kernel_ms"], 3)
    res["d_over_c"] = round(d["median_ms"] / c["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_batch_latency.json"))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    out = {"cases": {}}
    for sname, nonces in SIZES:
        for tname, target in TARGETS:
            out["cases"][sname + "_" + tname] = run_case(nonces, target, a.rounds)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
