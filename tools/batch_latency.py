"""Many small Requests: a loop of minehip.search (A) against one minehip.search_batch (B).

One process, both paths warmed, then alternating rounds A, B, A, B, ...: the host clock runs around
calls that end in a synchronise (every search, and the batch call).  Per case the medians and
interquartile ranges of both, B's speed-up, and the kernel time of each side from the library's HIP
events (generic class: generic_scan for A, batch_scan for B).  The `abi` rows time the same two
paths through the C-ABI with the arguments built beforehand, i.e. without the Python wrapper's
per-request work.

Required: at K = 64 with 10^4 and 10^5 nonces B's median is below A's by more than
the two interquartile ranges together, and at K = 1 B is not above A by more than that spread.  The
10^6 case is reported whatever it shows.

    python tools/batch_latency.py [--rounds 11] [--out profiles/batch_latency.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitcoin-miner_amd")]
import minehip  # noqa: E402

CASES = (("k64_1e4", 64, 10 ** 4, True), ("k64_1e5", 64, 10 ** 5, True), ("k64_1e6", 64, 10 ** 6, False),
         ("k1_1e6", 1, 10 ** 6, True))


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
    fn()
    p = minehip.profile_read(0)
    minehip.profile_enable(0, False)
    return p["fast_ns"] + p["generic_ns"]


def run_case(k, nonces, rounds):
    reqs = [("cmu440-%02d" % i, 0, nonces - 1) for i in range(k)]
    loop = lambda: [minehip.search(*r) for r in reqs]  # noqa: E731
    batch = lambda: minehip.search_batch(reqs)  # noqa: E731
    # the same through the C-ABI alone
    arr, keep = minehip._requests(reqs)
    out = (minehip.mh_result * k)()
    h, n = ctypes.c_uint64(), ctypes.c_uint64()
    msgs = [minehip._b(r[0]) for r in reqs]

    def abi_loop():
        for m in msgs:
            minehip._check(minehip.lib.mh_search(0, m, len(m), 0, nonces - 1, ctypes.byref(h), ctypes.byref(n)))

    def abi_batch():
        minehip._check(minehip.lib.mh_search_batch(0, arr, k, out))

    for _ in range(3):  # warm both paths
        ra, rb = loop(), batch()
        abi_loop(), abi_batch()
    assert ra == rb, "search_batch differs from search"
    t = {"loop": [], "batch": [], "abi_loop": [], "abi_batch": []}
    for _ in range(rounds):
        t["loop"].append(timed(loop)[0])
        t["batch"].append(timed(batch)[0])
        t["abi_loop"].append(timed(abi_loop)[0])
        t["abi_batch"].append(timed(abi_batch)[0])
    res = {"requests": k, "nonces_each": nonces, "rounds": rounds,
           "fused": all(it["kind"] == 0 for it in minehip.batch_plan(reqs))}
    for name, ts in t.items():
        res[name] = quartiles(ts)
    res["loop"]["kernel_ms"] = round(kernel_ns(loop) / 1e6, 4)
    res["batch"]["kernel_ms"] = round(kernel_ns(batch) / 1e6, 4)
    for a, b, key in (("loop", "batch", "python"), ("abi_loop", "abi_batch", "abi")):
        spread = res[a]["iqr_ms"] + res[b]["iqr_ms"]
        res[key] = {"speedup": round(res[a]["median_ms"] / res[b]["median_ms"], 3), "spread_ms": round(spread, 4),
                    "batch_faster_beyond_spread": res[b]["median_ms"] < res[a]["median_ms"] - spread,
                    "batch_not_slower_beyond_spread": res[b]["median_ms"] <= res[a]["median_ms"] + spread}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_latency.json"))
    a = ap.parse_args()
    if a.rounds < 11:
        ap.error("--rounds: at least 11")
    out = {"cases": {}}
    ok = True
    for name, k, nonces, required in CASES:
        r = run_case(k, nonces, a.rounds)
        if required:
            key = "batch_faster_beyond_spread" if k > 1 else "batch_not_slower_beyond_spread"
            r["required"] = key
            r["required_ok"] = bool(r["python"][key])
            ok = ok and r["required_ok"]
        out["cases"][name] = r
    out["required_ok"] = ok
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
