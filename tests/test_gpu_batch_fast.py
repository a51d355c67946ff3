"""GPU tests of the batched search with fused fast pieces: mh_search_batch_ex(MH_BATCH_FUSE_FAST),
the batch_fast<J, MODE> kernels of the fourth embedded code object and batch_scan_slots.

Every result is compared with the CPU oracle (oracle.search on 8 threads, computed once per request
and shared by the tests) and with mh_search of the same request under the same environment.  The
shapes are the smallest that still plan a fast piece, about 3 * 10^6 nonces or less each:

  ("cmu440", 1_048_000, 2_200_000)      one <3, One> piece of 115,200 runs (450 chunks exactly) + 1 nonce
  ("cmu440", 0, 3_000_000)              10^6 generic + <3, One> with 200,000 runs (781 chunks and a
                                        last one of 64 lanes) + 1 nonce
  ("a" * 51, 0, 3_000_000)              <13, TwoEarly>
  ("a" * 60, 0, 3_000_000)              <0, Pre>
  ("a" * 47, 900_000, 3_000_000)        <13, One>
  ("cmu440", 5 * 10^8, 5 * 10^8 + 3 * 10^6)   9 digits
  ("cmu440", 2^64 - 1 - 3 * 10^6, 2^64 - 1)   20 digits, <6, One>, ends at the top of u64

The probes use the dev build's MINEHIP_DEV_HASH_XOR hook with build/fast_batch_keep.hsaco as the
batch code object (MINEHIP_DEV_BATCH_CODE_OBJECT), in the manner of tests/test_gpu_probe.py: with
x = Hash(msg, n*) the request of msg must return (0, n*) for n* inside its range and a non-zero
minimum for n* just outside it, and every other request of the call the first minimum of Hash ^ x
over its own range (test_gpu_ties.masked_min, from the oracle's hashes, bit-exact).  One child
process per GPU test.
"""
import concurrent.futures
import functools
import json
import os
import subprocess
import sys

import pytest

from oracle import oracle
from conftest import ROOT, PKG, run_dev
from test_gpu_ties import KEEP_CO, U64, masked_min

pytestmark = pytest.mark.gpu

BATCH_KEEP_CO = os.path.join(ROOT, "build", "fast_batch_keep.hsaco")

SHAPES = [
    (b"cmu440", 1_048_000, 2_200_000),
    (b"cmu440", 0, 3_000_000),
    (b"a" * 51, 0, 3_000_000),
    (b"a" * 60, 0, 3_000_000),
    (b"a" * 47, 900_000, 3_000_000),
    (b"cmu440", 5 * 10 ** 8, 5 * 10 ** 8 + 3 * 10 ** 6),
    (b"cmu440", U64 - 3 * 10 ** 6, U64),
]
# generic-only requests beside them, and a second message of the layout <3, One> (a shared launch)
EXTRA = [(b"cmu440", 0, 199_999), (b"x", 5, 5), (b"", 0, 1000), (b"cmu441", 1_048_000, 2_200_000)]
ALL = SHAPES + EXTRA

L3 = dict(MINEHIP_LOWER_DIGITS=3, MINEHIP_MIN_LANES=16)   # [0, 3 * 10^6]: L = 3, 2,000 runs, 7.8 chunks
L2 = dict(MINEHIP_LOWER_DIGITS=2, MINEHIP_MIN_LANES=16)
SLOTS = dict(MINEHIP_BATCH_SLOTS=1000)   # several passes; the requests of 1,174 slots and more fall back
NO_EARLY = dict(MINEHIP_EARLY=0)


@functools.lru_cache(maxsize=None)
def expected(req):
    return oracle.search(*req, threads=8)


CHILD = """
import json, os, minehip
spec = json.load(open({path!r}))
if spec.get("dev"):
    assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
out = []
for j in spec["jobs"]:
    kv = {{k: str(v) for k, v in j["env"].items()}}
    os.environ.update(kv)
    try:
        reqs = [(bytes.fromhex(m), lo, hi) for m, lo, hi in j["reqs"]]
        if j.get("profile"):
            minehip.profile_enable(0, True)
            before = minehip.profile_read(0)
        plan = minehip.batch_plan_ex(reqs) if j.get("plan", True) else None
        res = minehip.search_batch(reqs, fuse_fast=True, errors="return")
        res = [r if isinstance(r, tuple) else ["error", r.code] for r in res]
        d = dict(results=res, plan=plan)
        if j.get("profile"):
            after = minehip.profile_read(0)
            d["profile"] = {{k: after[k] - before[k] for k in after}}
            d["kernels"] = [[k["word"], k["mode"], k["lo_digits"], k["nonces"], k["launches"]]
                            for k in minehip.profile_kernels(0)]
            minehip.profile_enable(0, False)
        if j.get("singles"):
            d["singles"] = [minehip.search(*r) for r in reqs]
    finally:
        for k in kv:
            del os.environ[k]
    out.append(d)
print(json.dumps(out))
"""


def run_jobs(tmp_path, jobs, dev=False, timeout=120):
    """The jobs in one child process: on the product library, or (dev) on the dev build with the
    variant code objects of both the single search and the batch."""
    path = str(tmp_path / "jobs.json")
    with open(path, "w") as f:
        json.dump(dict(jobs=jobs, dev=dev), f)
    code = CHILD.format(path=path)
    if dev:
        assert os.path.exists(BATCH_KEEP_CO) and os.path.exists(KEEP_CO), "make all builds them"
        r = run_dev(code, timeout=timeout, MINEHIP_DEV_CODE_OBJECT=KEEP_CO, MINEHIP_DEV_BATCH_CODE_OBJECT=BATCH_KEEP_CO)
    else:
        pre = f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]\n"
        r = subprocess.run([sys.executable, "-c", pre + code], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def job(reqs, env=None, **kw):
    return dict(reqs=[(m.hex(), lo, hi) for m, lo, hi in reqs], env=env or {}, **kw)


def test_all_shapes_in_one_call(gpu, tmp_path):
    """Every shape, generic-only requests and a second message of one layout in one call, under the
    default plan, L = 3, L = 2, a slot capacity that forces passes and fallbacks, and without the
    Early layouts: the oracle's result and mh_search's, whatever the plan."""
    envs = [{}, L3, L2, SLOTS, NO_EARLY]
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        exp = ex.submit(lambda: [expected(r) for r in ALL])
        out = run_jobs(tmp_path, [job(ALL, env, singles=True) for env in envs])
        exp = exp.result()
    for env, d in zip(envs, out):
        assert [tuple(r) for r in d["results"]] == exp, env
        assert [tuple(r) for r in d["singles"]] == exp, env
    plans = [d["plan"] for d in out]
    fast = [[p for p in plan if p["kind"] == 2] for plan in plans]
    # the plans are the ones the cases are about
    assert {p["req"] for p in fast[0]} == {0, 1, 2, 3, 4, 5, 6, 10} and not [p for p in plans[0] if p["kind"] == 1]
    assert [p["launch"] for p in fast[0] if p["req"] in (0, 1, 5, 10)] == [0, 0, 0, 0]   # <3, One>: one launch
    assert {(p["word"], p["mode"]) for p in fast[0]} == {(3, 0), (13, 5), (0, 1), (13, 0), (6, 0)}
    assert {p["lo_digits"] for p in fast[0]} == {1} and max(p["pass"] for p in plans[0]) == 0
    assert {p["lo_digits"] for p in fast[1]} == {3} and [p["slots"] for p in fast[1] if p["req"] == 1] == [8]
    assert {p["lo_digits"] for p in fast[2]} == {2}
    assert {p["kind"] for p in plans[3]} == {0, 1, 2} and max(p["pass"] for p in plans[3]) >= 1
    assert not [p for p in fast[4] if p["mode"] >= 3] and [p for p in fast[0] if p["mode"] >= 3]


def test_one_request_alone_and_twice(gpu, tmp_path):
    reqs = [SHAPES[1], SHAPES[2]]
    jobs = [job([r]) for r in reqs] + [job([r, r]) for r in reqs] + [job([SHAPES[0]], L3)]
    out = run_jobs(tmp_path, jobs)
    for r, d in zip(reqs + reqs + [SHAPES[0]], out):
        assert [tuple(x) for x in d["results"]] == [expected(r)] * len(d["results"])
        assert {p["kind"] for p in d["plan"]} >= {2} and 1 not in {p["kind"] for p in d["plan"]}
    assert len(out[2]["results"]) == 2 and [p["launch"] for p in out[2]["plan"] if p["kind"] == 2] == [0, 0]


def test_request_errors_leave_the_others_intact(gpu, tmp_path):
    reqs = [SHAPES[0], (b"x", 5, 4), SHAPES[3], (b"y" * ((1 << 20) + 1), 0, 10), EXTRA[0], (b"z", U64, 0)]
    out = run_jobs(tmp_path, [job(reqs, plan=False)])[0]["results"]
    assert [tuple(out[i]) for i in (0, 2, 4)] == [expected(reqs[i]) for i in (0, 2, 4)]
    assert [out[i] for i in (1, 3, 5)] == [["error", -2], ["error", -3], ["error", -2]]


def test_profile_counts_the_fused_fast_pieces(gpu, tmp_path):
    d = run_jobs(tmp_path, [job(ALL, profile=True)])[0]
    assert [tuple(r) for r in d["results"]] == [expected(r) for r in ALL]
    fast = [p for p in d["plan"] if p["kind"] == 2]
    assert d["profile"]["fast_nonces"] == sum(p["count"] for p in fast) > 10 ** 7
    assert d["profile"]["generic_nonces"] == sum(p["count"] for p in d["plan"] if p["kind"] == 0)
    assert d["profile"]["fast_launches"] == len({p["launch"] for p in fast}) == 5
    assert d["profile"]["fast_ns"] > 0 and d["profile"]["fast_ops"] > 0 and d["profile"]["fast_slots"] > 0
    per = {}
    for p in fast:
        k = (p["word"], p["mode"], p["lo_digits"])
        per[k] = per.get(k, 0) + p["count"]
    assert {(w, m, L): n for w, m, L, n, _ in d["kernels"] if n} == per
    assert sum(k[4] for k in d["kernels"]) == 5


# ---- XOR probes (dev build) ----------------------------------------------------------------------

# one request per layout class, and two messages of <3, One> that share a launch (the second is
# the launch's second item: pieces of equal L keep request order)
PROBED = [SHAPES[0], (b"cmu441", 0, 3_000_000), SHAPES[2], SHAPES[3]]
LANES = (63, 64, 255, 256)


def probe_nonces(req, plan, idx):
    """(inside, outside) probes of request idx: its range's edges, every piece's first and last
    nonce (the seams between tiles and chunks), and per fast piece the first and last nonce of
    lanes 63, 64, 255 and 256, of the last lane -- the last valid one of a partial last chunk --
    and of the lane before it."""
    msg, lo, hi = req
    pos, neg = {lo, hi}, ({lo - 1} if lo else set()) | ({hi + 1} if hi < U64 else set())
    for p in plan:
        if p["req"] != idx:
            continue
        first, last = p["first"], p["first"] + p["count"] - 1
        pos |= {first, last}
        if p["kind"] == 2:
            R = 10 ** p["lo_digits"]
            runs = p["count"] // R
            for k in LANES + (runs - 2, runs - 1):
                if 0 <= k < runs:
                    pos |= {first + k * R, first + k * R + R - 1}
    return sorted(pos), sorted(neg)


@pytest.mark.parametrize("env", [{}, L3], ids=["L1", "L3"])
def test_xor_probes(gpu, tmp_path, env):
    """Every probe is one call of the four requests: the probed nonce's request must return
    (0, n*), or a non-zero minimum inside its range for a probe just outside it, and every request
    of the call its masked_min under that constant."""
    import numpy as np
    import minehip
    from test_gpu_parity import env as setenv
    from test_gpu_ties import full_hashes
    with setenv(**env):
        plan = minehip.batch_plan_ex(PROBED)
    fast = [p for p in plan if p["kind"] == 2]
    assert [p["req"] for p in fast] == [0, 1, 2, 3] and [p["launch"] for p in fast] == [0, 0, 1, 2]
    assert {p["lo_digits"] for p in fast} == ({3} if env else {1})
    if not env:  # 450 chunks exactly, and 781 chunks with a last one of 64 lanes
        assert [(p["count"] // 10 // 256, p["count"] // 10 % 256) for p in fast[:2]] == [(450, 0), (781, 64)]
    probes = []   # (request, nonce, inside)
    for i, r in enumerate(PROBED):
        pos, neg = probe_nonces(r, plan, i)
        probes += [(i, n, True) for n in pos] + [(i, n, False) for n in neg]
    assert len(probes) >= 60 and sum(not inside for _, _, inside in probes) == 5
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        list(ex.map(lambda r: full_hashes(*r), PROBED))
    xs = [int(full_hashes(*PROBED[i])[n - PROBED[i][1]]) if inside
          else int(oracle.hash_batch(PROBED[i][0], np.array([n], dtype=np.uint64))[0]) for i, n, inside in probes]
    jobs = [job(PROBED, dict(env, MINEHIP_DEV_HASH_XOR="%016x" % x), plan=False) for x in xs]
    # one more call under a coarse-hash pair: many ties, so the (hash, nonce) order decides across chunks
    jobs.append(job(PROBED, dict(env, MINEHIP_DEV_HASH_KEEP="2,0"), plan=False))
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        refs = ex.map(lambda x: [masked_min(*r, 32, 32, x) for r in PROBED], xs)
        out = run_jobs(tmp_path, jobs, dev=True)
        refs = list(refs)
    for (i, n, inside), x, ref, d in zip(probes, xs, refs, out):
        got = [tuple(r) for r in d["results"]]
        assert got == [(t.hash, t.nonce) for t in ref], (i, n, inside, "%016x" % x)
        if inside:
            assert got[i] == (0, n), (i, n, got[i])
        else:
            assert got[i][0] != 0 and PROBED[i][1] <= got[i][1] <= PROBED[i][2], (i, n, got[i])
    ties = [masked_min(*r, 2, 0) for r in PROBED]
    assert [tuple(r) for r in out[-1]["results"]] == [(t.hash, t.nonce) for t in ties]
    assert all(t.count > 1000 for t in ties)
