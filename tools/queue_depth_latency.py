"""What a deep per-miner queue is worth end to end: N small client Requests through the server
loop, timed from the first submit to the last client Result, at queue depth 1, 8 and 64.

At depth 1 (the default, and all there was before mh_server_create_ex) every Request costs one
server -> miner -> server round trip and one search of its own; at depth d a miner holds up to d
chunks and answers what it holds with one mh_miner_handle_batch call (one fused GPU pass).

  in process   minehip.Server and one miner that answers every payload pending for it
               (miner_handle for one, miner_handle_batch for several); N = 64 and 1,024 Requests of
               10^4, 10^5 and 10^6 nonces, and of 10^7 with fuse_fast, at depth 1, 8 and 64
  over LSP     bin/minehip-server, one bin/minehip-miner and 64 bin/minehip-client processes of
               10^5 nonces on 127.0.0.1, at depth 1 and 64 (MINEHIP_QUEUE_DEPTH)
  large job    one Request of 2^36 nonces through the in-process loop with 4 miners at depth 1 and
               64 against a direct search: the budget rule must leave it alone (the 4 miners are
               served in turn by one thread here, so this shows the fixed cost per chunk, not
               how the job's tail balances over miners that run in parallel)

One process, every path warmed, then alternating rounds (depth 1, 8, 64, 1, 8, 64, ...); medians
and interquartile ranges as profiles/batch_latency.json.  The depth-1 legs use only calls that
exist without the queue (Server() without depth, miner_handle, minehip-server without
MINEHIP_QUEUE_DEPTH), so `--leg parent` runs them unchanged on a checkout of the parent commit
(copy this file there); `--parent FILE` stores that run as "parent" and compares:
  depth_1_agrees_with_parent      |median - parent median| <= the parent's interquartile range
  depth_64_not_slower_than_parent median <= parent median + the parent's interquartile range

    python tools/queue_depth_latency.py --leg parent --out parent.json        # on the parent commit
    python tools/queue_depth_latency.py --parent parent.json [--out profiles/queue_depth_latency.json]
"""
import argparse
import json
import os
import select
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bitcoin-miner_amd")]
import minehip  # noqa: E402

BIN = os.path.join(ROOT, "bitcoin-miner_amd", "bin")
MINER = 1_000_000
INPROC = [(n, size, size == 10 ** 7) for n in (64, 1024) for size in (10 ** 4, 10 ** 5, 10 ** 6, 10 ** 7)]
DEPTHS = (1, 8, 64)
LSP_CLIENTS, LSP_NONCES, LSP_DEPTHS = 64, 10 ** 5, (1, 64)


def quartiles(ts):
    s = sorted(ts)
    q = lambda f: s[min(len(s) - 1, int(f * (len(s) - 1) + 0.5))]  # noqa: E731
    return {"median_ms": round(q(0.5) * 1e3, 4), "iqr_ms": round((q(0.75) - q(0.25)) * 1e3, 4),
            "min_ms": round(s[0] * 1e3, 4)}


def serve(payloads, depth, fuse_fast=False, miners=(MINER,)):
    """Submit the clients' Request payloads [(conn, payload)] to a fresh Server and let the miners
    answer until every client has its Result.  Returns (seconds from the first submit to the last
    Result, {conn: Result payload}, the largest batch a miner answered)."""
    v = minehip.Server() if depth == 1 else minehip.Server(depth=depth)
    for m in miners:
        v.read(m, JOIN, time.monotonic_ns())
    inbox = {m: [] for m in miners}
    results, largest = {}, 0

    def route():
        for conn, p in v.writes():
            if conn in inbox:
                inbox[conn].append(p)
            else:
                results[conn] = p

    t0 = time.perf_counter()
    for conn, p in payloads:
        v.read(conn, p, time.monotonic_ns())
    route()
    while len(results) < len(payloads):
        for m in miners:
            batch, inbox[m] = inbox[m], []
            if not batch:
                continue
            largest = max(largest, len(batch))
            if len(batch) == 1:
                outs = [minehip.miner_handle(batch[0])]
            elif fuse_fast:
                outs = minehip.miner_handle_batch(batch, errors="raise", fuse_fast=True)
            else:
                outs = minehip.miner_handle_batch(batch, errors="raise")
            for r in outs:
                v.read(m, r, time.monotonic_ns())
            route()
    dt = time.perf_counter() - t0
    v.close()
    return dt, results, largest


def inproc_case(n, size, fuse_fast, depths, rounds):
    payloads = [(c, minehip.marshal(minehip.NewRequest("cmu440-%04d" % c, 0, size - 1))) for c in range(n)]
    ref = None
    for d in depths:  # warm every path, and the answers do not depend on the depth
        _, res, _ = serve(payloads, d, fuse_fast)
        assert ref is None or res == ref, "Results differ between depths"
        ref = res
    ts, largest = {d: [] for d in depths}, {}
    for _ in range(rounds):
        for d in depths:
            dt, _, largest[d] = serve(payloads, d, fuse_fast)
            ts[d].append(dt)
    out = {"requests": n, "nonces_each": size, "fuse_fast": fuse_fast, "rounds": rounds}
    for d in depths:
        out["depth_%d" % d] = dict(quartiles(ts[d]), largest_batch=largest[d])
    return out


class Cluster:
    """minehip-server (at `depth`: MINEHIP_QUEUE_DEPTH, unset for 1) and one minehip-miner."""

    def __init__(self, depth):
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        self.hp = f"127.0.0.1:{port}"
        self.env = dict(os.environ, LSP_EPOCH_MILLIS="200", LSP_EPOCH_LIMIT="5")
        senv = self.env if depth == 1 else dict(self.env, MINEHIP_QUEUE_DEPTH=str(depth))
        self.procs = [subprocess.Popen([os.path.join(BIN, "minehip-server"), str(port)], stdout=subprocess.PIPE,
                                       stderr=subprocess.DEVNULL, env=senv, text=True)]
        ready, _, _ = select.select([self.procs[0].stdout], [], [], 20.0)  # its listening line
        if not ready or not self.procs[0].stdout.readline().startswith("Server listening"):
            self.close()
            raise RuntimeError("minehip-server did not start")
        self.procs.append(subprocess.Popen([os.path.join(BIN, "minehip-miner"), self.hp], stdout=subprocess.DEVNULL,
                                           stderr=subprocess.DEVNULL, env=self.env))

    def clients(self, jobs):
        """Start one client per (msg, max_nonce), all at once; seconds until the last printed Result,
        and the printed lines -- or (None, None) when a client is still waiting after 20 s.  That
        is a stall, not a slow round, and no matter of the queue: when a new client process gets
        the UDP port of one that exited less than EpochLimit epochs ago, liblsp440's server takes
        its Connect for a resent one, acks it with the old connID and drops its Request as a
        duplicate.  Such rounds are counted (stalled_rounds) and run again."""
        t0 = time.perf_counter()
        cl = [subprocess.Popen([os.path.join(BIN, "minehip-client"), self.hp, msg, str(hi)], stdout=subprocess.PIPE,
                               env=self.env, text=True) for msg, hi in jobs]
        try:
            out = [c.communicate(timeout=max(1.0, 20.0 - (time.perf_counter() - t0)))[0].strip() for c in cl]
        except subprocess.TimeoutExpired:
            return None, None
        finally:
            for c in cl:
                if c.poll() is None:
                    c.kill()
                c.wait()
        return time.perf_counter() - t0, out

    def close(self):
        for p in self.procs:
            if p.poll() is None:
                p.kill()
            p.wait()


def lsp_case(depths, rounds):
    jobs = [("lsp-%02d" % k, LSP_NONCES - 1) for k in range(LSP_CLIENTS)]
    clusters = {}
    try:
        for d in depths:
            clusters[d] = Cluster(d)
        time.sleep(3.0)  # miners joined and their GPU contexts up
        ref = None
        ts, stalled = {d: [] for d in depths}, {d: 0 for d in depths}
        for d in depths:  # warm: the first search of each miner process
            for _ in range(4):
                _, out = clusters[d].clients(jobs)
                if out is not None:
                    break
                stalled[d] += 1
            assert out and all(o.startswith("Result ") for o in out) and (ref is None or out == ref), out
            ref = out
        for _ in range(4 * rounds):  # a stalled round is counted and run again
            for d in depths:
                if len(ts[d]) < rounds:
                    dt, _ = clusters[d].clients(jobs)
                    if dt is None:
                        stalled[d] += 1
                    else:
                        ts[d].append(dt)
        assert all(len(ts[d]) == rounds for d in depths), stalled
    finally:
        for c in clusters.values():
            c.close()
    out = {"clients": LSP_CLIENTS, "nonces_each": LSP_NONCES, "rounds": rounds}
    for d in depths:
        out["depth_%d" % d] = dict(quartiles(ts[d]), stalled_rounds=stalled[d])
    return out


def large_case(depths, rounds, bits=36):
    hi = (1 << bits) - 1
    payloads = [(1, minehip.marshal(minehip.NewRequest("cmu440", 0, hi)))]
    miners = tuple(MINER + k for k in range(4))
    direct = minehip.search("cmu440", 0, hi)
    want = minehip.marshal(minehip.NewResult(*direct))
    td, ts, largest = [], {d: [] for d in depths}, {d: 0 for d in depths}
    for _ in range(rounds):
        t0 = time.perf_counter()
        minehip.search("cmu440", 0, hi)
        td.append(time.perf_counter() - t0)
        for d in depths:
            dt, res, k = serve(payloads, d, miners=miners)
            assert res == {1: want}, d
            ts[d].append(dt)
            largest[d] = max(largest[d], k)
    out = {"nonces": hi + 1, "miners": 4, "rounds": rounds, "direct": quartiles(td)}
    for d in depths:
        q = quartiles(ts[d])
        # largest_batch: one chunk per miner while chunks are rate x target_ns; the fair-share cap
        # cuts the job's last chunks smaller than the budget, and those do stack up
        out["depth_%d" % d] = dict(q, server_over_direct=round(out["direct"]["median_ms"] / q["median_ms"], 4),
                                   largest_batch=largest[d])
    return out


def compare(new, parent):
    """The two acceptance rows for one shape: `new` holds depth_1 / depth_64, `parent` the parent's depth_1."""
    p, iqr = parent["median_ms"], parent["iqr_ms"]
    return {"parent_median_ms": p, "parent_iqr_ms": iqr,
            "depth_1_over_parent": round(new["depth_1"]["median_ms"] / p, 4),
            "depth_64_speedup_over_parent": round(p / new["depth_64"]["median_ms"], 3),
            "depth_1_agrees_with_parent": abs(new["depth_1"]["median_ms"] - p) <= iqr,
            "depth_64_not_slower_than_parent": new["depth_64"]["median_ms"] <= p + iqr}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("all", "parent"), default="all")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--lsp-rounds", type=int, default=7)
    ap.add_argument("--large-rounds", type=int, default=3)
    ap.add_argument("--parent", help="the JSON that --leg parent wrote on the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_depth_latency.json"))
    a = ap.parse_args()
    if a.rounds < 11 or a.lsp_rounds < 5:
        ap.error("--rounds: at least 11, --lsp-rounds: at least 5")
    global JOIN
    JOIN = minehip.marshal(minehip.NewJoin())
    depths = (1,) if a.leg == "parent" else DEPTHS
    out = {"leg": a.leg, "inproc": {}}
    for n, size, fuse_fast in INPROC:
        name = "n%d_1e%d" % (n, len(str(size)) - 1)
        out["inproc"][name] = inproc_case(n, size, fuse_fast, depths, a.rounds)
        print(name, json.dumps(out["inproc"][name]), file=sys.stderr, flush=True)
    out["lsp"] = lsp_case((1,) if a.leg == "parent" else LSP_DEPTHS, a.lsp_rounds)
    print("lsp", json.dumps(out["lsp"]), file=sys.stderr, flush=True)
    if a.leg == "all":
        out["large_job"] = large_case((1, 64), a.large_rounds)
        print("large_job", json.dumps(out["large_job"]), file=sys.stderr, flush=True)
    if a.parent:
        with open(a.parent) as f:
            par = json.load(f)
        out["parent"] = par
        cmp_ = {name: compare(c, par["inproc"][name]["depth_1"]) for name, c in out["inproc"].items()}
        cmp_["lsp"] = compare(out["lsp"], par["lsp"]["depth_1"])
        out["vs_parent"] = cmp_
        out["depth_1_agrees_with_parent"] = all(c["depth_1_agrees_with_parent"] for c in cmp_.values())
        out["depth_64_not_slower_than_parent"] = all(c["depth_64_not_slower_than_parent"] for c in cmp_.values())
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
