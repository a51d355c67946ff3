"""Many small hit searches: a loop of minehip.search_hits (a), one minehip.search_batch of the same
ranges -- the minimum alone, the same scan without the append -- (b), and one
minehip.search_hits_batch (c).

One process, every path warmed, then alternating rounds a, b, c, a, ...: the host clock runs around
calls that end in a synchronise.  64 distinct "cmu440-NN" messages over [0, nonces - 1] with
nonces = 10^4, 10^5, 10^6, and per size the targets 2^64 // 10^3, 2^64 // 10^6 and 0 (no hit).
Per case: medians and interquartile ranges, and the kernel time of b and c from the library's HIP
events (generic class): batch_scan against batch_scan_hits.  The `b_abi` / `c_abi` rows time b and
c through the C-ABI with the arguments built beforehand, i.e. without the Python wrapper's
per-request work.

What the numbers are read for (DESIGN.md §3 "Every hit, batched"):
  fixed cost       c against a, every row (`a_over_c`)
  cost of the hits c against b at target 0, where nothing is ever appended: `c_minus_b_ms` against
                   `zero_target_bound_ms`, the larger of the two interquartile ranges plus b's
                   median times (the hits loop's instructions / batch_scan's loop's - 1)

    python tools/hits_batch_latency.py [--rounds 15] [--out profiles/hits_batch_latency.json]
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
CAP = 4096
SIZES = (("k64_1e4", 10 ** 4), ("k64_1e5", 10 ** 5), ("k64_1e6", 10 ** 6))
TARGETS = (("k3", 2 ** 64 // 10 ** 3), ("k6", 2 ** 64 // 10 ** 6), ("zero", 0))
# per-nonce loop, instructions, read from build/search_kernels.s (`make asm`): batch_scan_hits, batch_scan
LOOP_INSTRUCTIONS = (1443, 1433)


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


def run_case(nonces, target, rounds):
    reqs = [("cmu440-%02d" % i, 0, nonces - 1, target) for i in range(K)]
    plain = [r[:3] for r in reqs]
    paths = {"a_loop_hits": lambda: [minehip.search_hits(*r, CAP) for r in reqs],
             "b_batch_min": lambda: minehip.search_batch(plain),
             "c_hits_batch": lambda: minehip.search_hits_batch(reqs, CAP)}
    arr_b, keep_b = minehip._requests(plain)
    out_b = (minehip.mh_result * K)()
    arr_c, keep_c, _, total = minehip._hits_requests(reqs, CAP)
    buf_c = (minehip.mh_hit * total)()
    out_c = (minehip.mh_hits_result * K)()
    paths["b_abi"] = lambda: minehip._check(minehip.lib.mh_search_batch(0, arr_b, K, out_b))
    paths["c_abi"] = lambda: minehip._check(minehip.lib.mh_search_hits_batch(0, arr_c, K, buf_c, total, out_c))
    for _ in range(3):  # warm every path
        got = {name: fn() for name, fn in paths.items()}
    assert got["a_loop_hits"] == got["c_hits_batch"], "search_hits_batch differs from search_hits"
    assert [g[2] for g in got["c_hits_batch"]] == got["b_batch_min"], "minimum differs from search_batch"
    t = {name: [] for name in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            t[name].append(timed(fn)[0])
    regs = minehip.hits_batch_regions(reqs, CAP)
    res = {"requests": K, "nonces_each": nonces, "target": target, "cap": CAP, "rounds": rounds,
           "hits": sum(g[0] for g in got["c_hits_batch"]),
           "rebuilt": sum(1 for g in got["c_hits_batch"] if g[0] > CAP),
           "fused": all(g["kind"] == 0 for g in regs), "windows": 1 + max(g["window"] for g in regs)}
    for name, ts in t.items():
        res[name] = quartiles(ts)
        if name[0] in "bc" and not name.endswith("_abi"):
            res[name]["kernel_ms"] = kernel_ms(paths[name])
    a, b, c = (res[n] for n in list(paths)[:3])
    res["a_over_c"] = round(a["median_ms"] / c["median_ms"], 2)
    res["c_over_b"] = round(c["median_ms"] / b["median_ms"], 3)
    res["c_over_b_abi"] = round(res["c_abi"]["median_ms"] / res["b_abi"]["median_ms"], 3)
    res["c_over_b_kernel"] = round(c["kernel_ms"] / b["kernel_ms"], 3)
    if target == 0:  # the cost of the feature: nothing is appended, the scan and the tables are what differs
        ratio = LOOP_INSTRUCTIONS[0] / LOOP_INSTRUCTIONS[1]
        for x, y, tag in ((c, b, ""), (res["c_abi"], res["b_abi"], "_abi")):
            res["c_minus_b_ms" + tag] = round(x["median_ms"] - y["median_ms"], 4)
            res["zero_target_bound_ms" + tag] = round(max(x["iqr_ms"], y["iqr_ms"]) + y["median_ms"] * (ratio - 1.0), 4)
            res["within_bound" + tag] = res["c_minus_b_ms" + tag] <= res["zero_target_bound_ms" + tag]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits_batch_latency.json"))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    out = {"loop_instructions": {"batch_scan_hits": LOOP_INSTRUCTIONS[0], "batch_scan": LOOP_INSTRUCTIONS[1]},
           "cases": {}}
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
