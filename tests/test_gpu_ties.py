"""First-minimum tie-breaking on the GPU.

The product promises the lexicographic minimum of (hash, nonce).  With real SHA-256 output no two
nonces of a test share a 64-bit hash, so the second half of that order never decides anything.  The
dev build's MINEHIP_DEV_HASH_KEEP=k0,k1 hook keeps only the top k0 bits of H0 and the
top k1 bits of H1 of every nonce's hash before it enters any comparison: many nonces then tie, and
the unchanged comparison code of every kernel and merge -- fast_search's candidate selection,
block_min / wave_step / lex_less, scan_decade's fold, merge_partials, merge_segments, the host
merges of search_multi -- decides which nonce is returned.  The fast kernels mask in the variant
code object build/fast_search_keep.hsaco (the product's source with -DMH_HASH_KEEP, through the
same passes), loaded through MINEHIP_DEV_CODE_OBJECT.

The reference and the child process also take MINEHIP_DEV_HASH_XOR values (a constant XORed into
every hash before the mask), default none: tests/test_gpu_probe.py probes single nonces with them.

Reference: masked_min -- the oracle's full hashes of every nonce of the range, masked in numpy;
the expected result is (min key, first nonce attaining it), bit-exact.  Every GPU test asserts from
that reference alone that its ties are live: how many nonces attain the minimum and how far apart
they lie.  One child process (conftest.run_dev) per test function.
"""
import collections
import concurrent.futures
import functools
import json
import os
import random
import re

import numpy as np
import pytest

from oracle import oracle
from conftest import ROOT, run_dev

U64 = (1 << 64) - 1
KEEP_CO = os.path.join(ROOT, "build", "fast_search_keep.hsaco")

# (k0, k1): what the pair exercises
KEEP_PAIRS = (
    (0, 0),     # every hash equal: the answer is (0, lo)
    (2, 0),     # massive H0 ties: the nonce decides across lanes, waves, chunks and launches
    (2, 32),    # H0 ties, H1 decides: the <= admission and the c1 < wbh1 arm
    (3, 3),
    (12, 0),    # a handful of tied nonces scattered over the range: the winner is not near lo,
    (16, 0),    # and the ties sit in different chunks and partial buffers
    (32, 32),   # the identity: the product's answer
)
DENSE = tuple(p for p in KEEP_PAIRS if sum(p) <= 8)   # pairs under which every case must tie
SPARSE = ((12, 0), (16, 0))                           # ... at least two thirds of the cases
CHUNK1 = 2560  # nonces of one workgroup's chunk at L = 1 (256 lanes x 10); x 10^(L-1) at lane length L

Tie = collections.namedtuple("Tie", "hash nonce count last")  # last: the largest nonce at the minimum


def keep_mask(k):
    return (0xFFFFFFFF << (32 - k)) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def full_hashes(msg, lo, hi):
    """Hash(msg, n) of every n in [lo, hi] from the CPU oracle, computed once per range (eight
    slices on eight threads: the oracle is a C library and ctypes releases the GIL)."""
    nonces = np.uint64(lo) + np.arange(hi - lo + 1, dtype=np.uint64)
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        h = np.concatenate(list(ex.map(lambda a: oracle.hash_batch(msg, a), np.array_split(nonces, 8))))
    h.setflags(write=False)
    return h


def masked_min(msg, lo, hi, k0, k1, x=0):
    """The expected result of a search of [lo, hi] under MINEHIP_DEV_HASH_KEEP=k0,k1 and
    MINEHIP_DEV_HASH_XOR=x (the XOR first): the minimum key (Hash ^ x) & mask, the first nonce
    attaining it, how many nonces attain it, and the last of them."""
    key, mask = full_hashes(msg, lo, hi), (keep_mask(k0) << 32) | keep_mask(k1)
    if x:
        key = key ^ np.uint64(x)
    if mask != U64:
        key = key & np.uint64(mask)
    first = int(key.argmin())       # numpy: the first occurrence of the minimum
    at = key == key[first]
    return Tie(int(key[first]), lo + first, int(np.count_nonzero(at)), lo + at.size - 1 - int(at[::-1].argmax()))


# ---- CPU tests ---------------------------------------------------------------------------------

def test_masked_min_against_brute_force():
    import hashlib
    for msg, lo in ((b"cmu440", 95), (b"x" * 60, 10 ** 19 - 150), (b"", U64 - 299)):
        hi = lo + 299
        hs = [int.from_bytes(hashlib.sha256(msg + b" " + str(n).encode()).digest()[:8], "big")
              for n in range(lo, hi + 1)]
        for k0, k1 in KEEP_PAIRS + ((1, 0), (0, 5), (32, 0), (7, 9)):
            best, cnt, last = None, 0, None
            for n, h in zip(range(lo, hi + 1), hs):
                key = ((h >> 32) >> (32 - k0) << (32 - k0) if k0 else 0) << 32 | \
                      ((h & 0xFFFFFFFF) >> (32 - k1) << (32 - k1) if k1 else 0)
                if best is None or key < best[0]:   # strict <: the first minimum
                    best, cnt = (key, n), 0
                if key == best[0]:
                    cnt, last = cnt + 1, n
            assert masked_min(msg, lo, hi, k0, k1) == Tie(best[0], best[1], cnt, last), (msg[:8], lo, k0, k1)
        assert masked_min(msg, lo, hi, 0, 0) == Tie(0, lo, 300, hi)
        assert masked_min(msg, lo, hi, 32, 32)[:3] == oracle.search(msg, lo, hi) + (1,)
        # MINEHIP_DEV_HASH_XOR: x = H(n) of nonces inside the range (positive probes: the reference
        # is (0, n), attained once) and just outside it (negative ones: a non-zero minimum), and
        # arbitrary constants, alone and under keep pairs
        H = lambda n: int.from_bytes(hashlib.sha256(msg + b" " + str(n).encode()).digest()[:8], "big")  # noqa: E731
        inside = (lo, lo + 1, lo + 137, hi - 1, hi)
        outside = [n for n in (lo - 1, lo - 2, hi + 1, hi + 2) if 0 <= n <= U64]
        assert len(outside) >= 2
        for x in [H(n) for n in inside + tuple(outside)] + [1, U64, 0x8000000000000000, 0x123456789ABCDEF0]:
            for k0, k1 in ((32, 32), (2, 0), (12, 0), (7, 9)):
                m0, m1 = (0xFFFFFFFF << (32 - k0)) & 0xFFFFFFFF, (0xFFFFFFFF << (32 - k1)) & 0xFFFFFFFF
                keys = [(h ^ x) & (m0 << 32 | m1) for h in hs]
                best = min(keys)
                at = [n for n, k in zip(range(lo, hi + 1), keys) if k == best]
                assert masked_min(msg, lo, hi, k0, k1, x) == Tie(best, at[0], len(at), at[-1]), (msg[:8], lo, k0, k1, x)
        for n in inside:
            assert masked_min(msg, lo, hi, 32, 32, H(n)) == Tie(0, n, 1, n)
        for n in outside:
            assert masked_min(msg, lo, hi, 32, 32, H(n)).hash != 0
        assert masked_min(msg, hi, hi, 32, 32, H(hi) ^ U64) == Tie(U64, hi, 1, hi)   # the all-ones hash


def fast_kernels_of(co):
    from minehip import codeobj
    names = {k[".name"] for k in codeobj.metadata(co)["amdhsa.kernels"]}
    return {tuple(int(x) for x in re.match(r"_ZN2mh11fast_searchILi(\d+)ELi(\d+)EE", n).groups())
            for n in names if "fast_search" in n}


def test_variant_code_object_holds_the_kernels_and_the_marker():
    """build/fast_search_keep.hsaco (make all) holds exactly the product's fast kernels, the
    work-queue marker and the coarse-hash marker; the code object embedded in the library holds
    the same kernels and no coarse-hash marker, so the dev build refuses to run it masked."""
    from minehip import codeobj
    from test_abi import KERNELS
    assert os.path.exists(KEEP_CO), "make all builds it"
    keep = open(KEEP_CO, "rb").read()
    assert fast_kernels_of(keep) == KERNELS
    assert b"mh_fast_hash_keep" in keep and b"mh_fast_queue_args" in keep
    emb = codeobj.fast_code_object()
    assert fast_kernels_of(emb) == KERNELS
    assert b"mh_fast_hash_keep" not in emb
    # the hash-XOR word (MINEHIP_DEV_HASH_XOR): the variant's kernels read it, the product's have none
    assert b"mh_dev_hash_xor" in keep and b"mh_dev_hash_xor" not in emb
    fast = [k for k in codeobj.metadata(keep)["amdhsa.kernels"] if "fast_search" in k[".name"]]
    assert {k[".args"][0][".size"] for k in fast} == {520}      # the same FastArgs, by value


# ---- the child process ---------------------------------------------------------------------------

CHILD = """
import json, os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
spec = json.load(open({path!r}))
if spec["profile"]:
    minehip.profile_enable(0, True)
out = []
for j in spec["jobs"]:
    for env in j["envs"]:
        for k0, k1 in j["keeps"]:
          for x in j.get("xors", [0]):
            kv = dict({{k: str(v) for k, v in env.items()}}, MINEHIP_DEV_HASH_KEEP="%d,%d" % (k0, k1),
                      MINEHIP_DEV_HASH_XOR="%016x" % x)
            os.environ.update(kv)
            try:
                if j["call"] == "batch":
                    reqs = [(bytes.fromhex(m), lo, hi) for m, lo, hi in j["reqs"]]
                    kinds = dict((it["req"], it["kind"]) for it in minehip.batch_plan(reqs))
                    assert [kinds[i] for i in range(len(reqs))] == j["kinds"], kinds
                    r = minehip.search_batch(reqs)
                elif j["call"] == "multi":
                    r = minehip.search_multi(bytes.fromhex(j["msg"]), j["lo"], j["hi"], devs=j["devs"], chunk=j["chunk"])
                else:
                    r = minehip.search(bytes.fromhex(j["msg"]), j["lo"], j["hi"])
            finally:
                for k in kv:
                    del os.environ[k]
            out.append(r)
kernels = sorted((k["word"], k["mode"]) for k in minehip.profile_kernels(0)) if spec["profile"] else []
print(json.dumps(dict(results=out, kernels=kernels)))
"""


def job(msg, lo, hi, keeps, envs=({},), call="search", xors=(0,), **kw):
    """One search per (env, keep pair, XOR value), in that order."""
    return dict(msg=msg.hex(), lo=lo, hi=hi, keeps=[list(k) for k in keeps], envs=list(envs), call=call,
                xors=list(xors), **kw)


def run_jobs(tmp_path, jobs, profile=False, timeout=120, **env):
    """Run the jobs in one child process on the dev build with the variant code object; returns
    ([result per (job, env, keep pair, XOR value), in that order], kernel set).  MINEHIP_DEV_HASH_KEEP
    and MINEHIP_DEV_HASH_XOR are read by every search, so one child runs every setting."""
    assert os.path.exists(KEEP_CO), "make all builds it"
    path = str(tmp_path / "jobs.json")
    with open(path, "w") as f:
        json.dump(dict(jobs=jobs, profile=profile), f)
    r = run_dev(CHILD.format(path=path), timeout=timeout, MINEHIP_DEV_CODE_OBJECT=KEEP_CO, **env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    return d["results"], {tuple(k) for k in d["kernels"]}


def check_jobs(jobs, results):
    """Every search result against masked_min.  Returns {keep pair: [Tie per (job, XOR value)]}."""
    ties = collections.defaultdict(list)
    it = iter(results)
    for j in jobs:
        msg = bytes.fromhex(j["msg"])
        xors = j.get("xors", [0])
        exps = {(k0, k1, x): masked_min(msg, j["lo"], j["hi"], k0, k1, x) for k0, k1 in j["keeps"] for x in xors}
        for env in j["envs"]:
            for k0, k1 in j["keeps"]:
                for x in xors:
                    exp = exps[(k0, k1, x)]
                    got = tuple(next(it))
                    assert got == (exp.hash, exp.nonce), (msg[:8], len(msg), j["lo"], j["hi"], (k0, k1), "%016x" % x,
                                                         env, j["call"], got, exp)
        for k0, k1 in j["keeps"]:
            ties[(k0, k1)].extend(exps[(k0, k1, x)] for x in xors)
    assert next(it, None) is None
    return ties


def assert_ties_live(ties, apart):
    """From the reference alone: under the dense pairs every case has >= 2 nonces at the minimum,
    under the sparse ones at least two thirds of the cases, and per pair at least one case has
    tied nonces more than `apart` nonces from each other (in different chunks)."""
    for pair, ts in ties.items():
        if pair in DENSE:
            assert all(t.count >= 2 for t in ts), (pair, [t for t in ts if t.count < 2][:3])
        if pair in SPARSE:
            assert 3 * sum(t.count >= 2 for t in ts) >= 2 * len(ts), (pair, [t.count for t in ts])
        if pair in DENSE or pair in SPARSE:
            assert any(t.last - t.nonce > apart for t in ts), (pair, apart)
    if (2, 32) in ties and (2, 0) in ties:
        # under (2, 32) the minimal H0 is shared (the (2, 0) count) and H1 picks another nonce
        # than the first of them in at least one case
        assert any(a.nonce != b.nonce for a, b in zip(ties[(2, 32)], ties[(2, 0)]))


# ---- GPU tests -------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_every_fast_kernel(gpu, tmp_path):
    """Each of the 26 fast_search<J, MODE> kernels over test_every_kernel_instantiation's range, at
    L = 1 (99 chunks) and the largest L the layout allows, under every keep pair."""
    from test_abi import KERNELS, KERNEL_CASE_NONCES, kernel_cases
    cases = kernel_cases()
    assert set(cases) == KERNELS
    jobs = []
    for (J, mode), (m, lo, _, early) in sorted(cases.items()):
        envs = [dict(MINEHIP_LOWER_DIGITS=Ld, MINEHIP_MIN_LANES=1, MINEHIP_GENERIC_BELOW=0, MINEHIP_EARLY=early)
                for Ld in (1, 3)]
        jobs.append(job(m, lo, lo + KERNEL_CASE_NONCES + 3_456, KEEP_PAIRS, envs))
    results, kernels = run_jobs(tmp_path, jobs, profile=True)
    assert kernels == KERNELS
    ties = check_jobs(jobs, results)
    assert_ties_live(ties, CHUNK1)
    # (32, 32) is the product library's search
    for j in jobs[::5]:
        m = bytes.fromhex(j["msg"])
        assert gpu.search(m, j["lo"], j["hi"]) == masked_min(m, j["lo"], j["hi"], 32, 32)[:2]


def early_tie_cases():
    """A subset of test_gpu_parity.early_position_cases(), among the cases whose blocks of lanes
    (10^(p+L) nonces each) fit twice into 200,000 nonces, each over 203,456 nonces from its first
    nonce (enough for ties under 16 kept bits): per Early kernel one case with contiguous lanes
    (p < L) and one with interleaved lanes (p >= L, lane order is not nonce order), plus one at the
    top of the u64 range.  Each range still plans a whole block of its (kernel, p, L).  Host only."""
    import minehip
    from test_gpu_parity import early_position_cases, env
    picked = {}
    for (J, mode, p, L, top), (m, lo, hi, Ld) in sorted(early_position_cases().items()):
        size = 200_000 + 3_456
        if 2 * 10 ** (p + L) > 200_000:
            continue
        slot = "top" if top else (J, mode, p < L)
        if slot in picked:
            continue
        lo2, hi2 = (U64 - size, U64) if top else (lo, min(hi, lo + size))
        with env(MINEHIP_LOWER_DIGITS=Ld, MINEHIP_MIN_LANES=1, MINEHIP_GENERIC_BELOW=0):
            t = (len(m) + 1) % 64
            for pc in minehip.plan(m, lo2, hi2):
                if pc["kind"] != 0 or (pc["word"], pc["mode"], pc["lo_digits"]) != (J, mode, L):
                    continue
                pl = t + pc["digits"] - 1
                base = 64 if (pc["blocks"] == 2 and pl >= 64) else 0
                if pl - (base + 4 * J + 3) == p and pc["count"] >= 10 ** (p + L):
                    picked[slot] = (m, lo2, hi2, Ld, p, L)
                    break
    return picked


def test_early_tie_cases_cover_both_lane_orders():
    picked = early_tie_cases()
    assert set(picked) == {(J, mode, c) for J, mode in ((0, 3), (8, 3), (0, 4), (13, 5)) for c in (True, False)} | \
        {"top"}, sorted(map(str, picked))
    assert all(hi - lo <= 210_000 for (_, lo, hi, *_r) in picked.values())


@pytest.mark.gpu
def test_early_positions(gpu, tmp_path):
    """The Early layouts, where a candidate's nonce comes from spread(...) and lanes interleave."""
    picked = early_tie_cases()
    jobs = [job(m, lo, hi, ((2, 0), (16, 0)),
                [dict(MINEHIP_LOWER_DIGITS=Ld, MINEHIP_MIN_LANES=1, MINEHIP_GENERIC_BELOW=0)])
            for (m, lo, hi, Ld, _p, _L) in picked.values()]
    results, _ = run_jobs(tmp_path, jobs)
    ties = check_jobs(jobs, results)
    assert_ties_live(ties, CHUNK1 * 10 ** (min(L for *_r, L in picked.values()) - 1))


@pytest.mark.gpu
def test_generic_path_and_edges(gpu, tmp_path):
    """The default plan (generic_scan on these small ranges): test_u64_edges' messages over
    [0, 25000], the top of u64 and straddles of 10^1, 10^5 and 10^19, under every keep pair that
    ties on ranges this small."""
    ranges = [(0, 25_000), (U64 - 30_000, U64), (3, 9_012), (10 ** 5 - 7_000, 10 ** 5 + 9_000),
              (10 ** 19 - 7_000, 10 ** 19 + 9_000)]
    # every pair but (16, 0): its 65,536 classes over 9,010 .. 30,001 nonces leave the minimum
    # untied in most of these ranges, which would make it a second (32, 32) here
    keeps = tuple(p for p in KEEP_PAIRS if p != (16, 0))
    jobs = [job(m, lo, hi, keeps) for m in (b"cmu440", b"", b"q" * 60, b"r" * 119) for lo, hi in ranges]
    results, _ = run_jobs(tmp_path, jobs)
    assert_ties_live(check_jobs(jobs, results), CHUNK1)


def batch_requests():
    """test_gpu_batch's EDGES and 60 of its fuzz requests (at most 3,000 nonces each), 130 requests
    of 20,000 nonces (eight or nine tiles each: under (12, 0) the ~5 nonces per class that tie at
    the minimum lie in different tiles, for merge_segments to order), and one request of 200,000
    nonces, too large for a pass of BATCH_SLOTS tiles."""
    from test_gpu_batch import EDGES, fuzz_requests
    rng = random.Random(441)
    multi = []
    for i in range(130):
        d = rng.randrange(1, 21)
        lo = min(rng.randrange(0 if d == 1 else 10 ** (d - 1), min(U64, 10 ** d - 1) + 1), U64 - 19_999)
        multi.append((b"tiles%d" % i, lo, lo + 19_999))
    return list(EDGES) + fuzz_requests(n=60) + multi + [(b"fallback", 5, 200_004)]


BATCH_PAIRS = ((0, 0), (2, 0), (2, 32), (12, 0))
BATCH_SLOTS = 64   # the 200,000-nonce request takes 79 tiles: a fallback; every other request fits


@pytest.mark.gpu
def test_batch(gpu, tmp_path):
    """search_batch: fused tiles (ties inside a lane's ten nonces, across lanes, across tiles in
    merge_segments, over several passes) and one request that falls back to the single search."""
    reqs = batch_requests()
    kinds = [0] * (len(reqs) - 1) + [1]
    jobs = [dict(call="batch", reqs=[(m.hex(), lo, hi) for m, lo, hi in reqs], kinds=kinds,
                 keeps=[list(p) for p in BATCH_PAIRS], envs=[{}])]
    results, _ = run_jobs(tmp_path, jobs, MINEHIP_BATCH_SLOTS=BATCH_SLOTS)
    assert len(results) == len(BATCH_PAIRS)
    ties = collections.defaultdict(list)
    for (k0, k1), got in zip(BATCH_PAIRS, results):
        assert len(got) == len(reqs)
        for (m, lo, hi), g in zip(reqs, got):
            exp = masked_min(m, lo, hi, k0, k1)
            assert tuple(g) == (exp.hash, exp.nonce), (m[:8], lo, hi, (k0, k1), g, exp)
            ties[(k0, k1)].append((hi - lo + 1, exp))
    # A request is a case.  One of fewer than 64 nonces need not tie under 2 kept bits (a single
    # nonce cannot at all): the few such EDGES and fuzz requests are exempt from "every case".
    for pair in ((0, 0), (2, 0)):
        big = [t for n, t in ties[pair] if n >= 64]
        assert len(big) >= len(reqs) - 12 and all(t.count >= 2 for t in big), pair
        assert any(t.last - t.nonce > CHUNK1 for t in big)            # in different tiles
        assert sum(t.last // 10 == t.nonce // 10 for t in big) < len(big)
    assert all(t.count >= 2 for n, t in ties[(0, 0)] if n >= 2)
    # (12, 0): requests of <= 3,000 nonces over 4,096 classes rarely tie at the minimum; the
    # 20,000-nonce requests and the fallback do, in different tiles
    sparse = [t for _, t in ties[(12, 0)]]
    assert 3 * sum(t.count >= 2 for t in sparse) >= 2 * len(sparse), [t.count for t in sparse]
    assert 2 * sum(t.last - t.nonce > CHUNK1 for t in sparse) >= len(sparse)
    assert sparse[-1].count >= 2 and sparse[-1].last - sparse[-1].nonce > CHUNK1    # the fallback
    assert any(a.nonce != b.nonce for (_, a), (_, b) in zip(ties[(2, 32)], ties[(2, 0)]))


@pytest.mark.gpu
def test_plans_and_host_merges(gpu, tmp_path):
    """The same tied ranges cut into launches, streams, work queues, partial-buffer flushes and
    host-side chunks in many ways: the first minimum does not depend on the cut."""
    keeps = ((2, 0), (16, 0))
    fast = dict(MINEHIP_MIN_LANES=1, MINEHIP_GENERIC_BELOW=0)
    envs = [dict(fast, MINEHIP_LOWER_DIGITS=3, MINEHIP_LAUNCH_NONCES=100_000, MINEHIP_STREAMS=st,
                 MINEHIP_FINE_TAIL=ft, MINEHIP_QUEUE=q)
            for st in (1, 2) for ft in (0, 20_000) for q in (0, 1)]
    envs += [dict(fast, MINEHIP_LOWER_DIGITS=Ld, MINEHIP_MAX_BLOCKS=mb, MINEHIP_QUEUE=q, MINEHIP_STREAMS=2,
                  MINEHIP_FINE_TAIL=20_000)
             for Ld, mb in ((1, 1), (1, 3), (2, 1), (3, 3)) for q in (0, 1)]
    jobs = []
    for m, lo, hi in ((b"cmu440", 5 * 10 ** 8, 5 * 10 ** 8 + 250_000), (b"x" * 60, 10 ** 9 - 120_000, 10 ** 9 + 130_000)):
        jobs.append(job(m, lo, hi, keeps, envs))
        jobs.append(job(m, lo, hi, keeps, [fast, {}], call="multi", devs=[0, 0, 0], chunk=12_345))
        jobs.append(job(m, lo, hi, keeps, [fast], call="multi", devs=[0, 0, 0], chunk=0))   # rate-weighted shards
    results, _ = run_jobs(tmp_path, jobs)
    ties = check_jobs(jobs, results)
    assert_ties_live(ties, CHUNK1 * 10)   # further apart than a chunk at L = 2 and than a host chunk


@pytest.mark.gpu
def test_guard_refuses_a_code_object_without_the_marker(gpu):
    """MINEHIP_DEV_HASH_KEEP with the embedded code object (its kernels do not mask): a search
    with a fast piece fails loudly instead of mixing masked generic pieces with unmasked fast
    ones, and so does a malformed value; the next search without the variable is the product's."""
    lo, hi = 10 ** 9, 10 ** 9 + 199_999
    r = run_dev(f"""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
assert "MINEHIP_DEV_CODE_OBJECT" not in os.environ
os.environ.update(MINEHIP_GENERIC_BELOW="0", MINEHIP_MIN_LANES="1")
assert any(p["kind"] == 0 for p in minehip.plan(b"cmu440", {lo}, {hi}))
for v in ("2,0", "32,32", "2", "2,33", "2,0,1", "x"):
    os.environ["MINEHIP_DEV_HASH_KEEP"] = v
    try:
        minehip.search(b"cmu440", {lo}, {hi})
        raise SystemExit("searched with MINEHIP_DEV_HASH_KEEP=" + v)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and "MINEHIP_DEV_HASH_KEEP" in str(e), e
del os.environ["MINEHIP_DEV_HASH_KEEP"]
print(*minehip.search(b"cmu440", {lo}, {hi}))
""", timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = tuple(int(x) for x in r.stdout.split()[-2:])
    assert got == masked_min(b"cmu440", lo, hi, 32, 32)[:2] == oracle.search(b"cmu440", lo, hi, threads=4)
