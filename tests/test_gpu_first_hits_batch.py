"""mh_search_first_hits_batch on the GPU: the k smallest hits of many requests in one fused pass --
batch_scan_bound[_slots] for the generic tiles, batch_bound<J, MODE> of the tenth embedded code
object for the fast pieces, merge_segments_bound -- each request stopped by its own bound.

The reference is the oracle's hashes of the whole range in numpy (test_hits.hits_ref; `ref` below
is hits_ref over a range whose hashes are computed once and shared by the requests on it).  The
per-request check is test_gpu_first_hits.check's contract.  Every case asserts from the reference
and the host-only plan alone that it is live before it looks at the GPU: which requests are fused,
that no region can overflow where path == 0 is asserted (so the rebuild path cannot hide a wrong
kernel), where the hits lie.

MINEHIP_EARLY, like every planner knob, is read per call, so test 2 puts the cases of one
(MINEHIP_LOWER_DIGITS, MINEHIP_EARLY) pair -- not of one MINEHIP_LOWER_DIGITS value -- in one batch."""
import functools

import numpy as np
import pytest

from test_first import kth_smallest_hash
from test_first_hits import bound_of, slices_of
from test_gpu_parity import env
from test_gpu_ties import full_hashes
from test_hits import hits_ref

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CMU = (b"cmu440", 0, 1_999_999)
CMU_MIN = (1228377698034, 1_067_492)
FAST = dict(MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1)
BOTH = (False, True)


def T10(j):
    return 2 ** 64 // 10 ** j


def want(k):
    return max(4 * k, 256)       # the region a request of k asks for (include/minehip.h)


@functools.lru_cache(maxsize=4)
def hashes(msg, lo, hi):
    return full_hashes(msg, lo, hi)


def ref(msg, lo, hi, T, k, h=None):
    """hits_ref(msg, lo, hi, T, k) from hashes computed once per range."""
    h = hashes(msg, lo, hi) if h is None else h
    idx = np.flatnonzero(h <= np.uint64(T))
    i = int(h.argmin())
    return int(idx.size), [(lo + int(j), int(h[j])) for j in idx[:k]], (int(h[i]), lo + i)


def check(r, got, exp=None, what=None):
    """One request's answer against the reference and mh_search_first_hits' contract."""
    msg, lo, hi, T, k = r
    count, entries, mn = exp if exp is not None else ref(*r)
    assert not isinstance(got, Exception), (what, got)
    ents, hn, scanned, path = got
    size = hi - lo + 1
    assert ents == entries, (what, msg[:8], lo, hi, T, k, path, ents[:3], len(ents), entries[:3], len(entries))
    assert len(ents) == min(count, k)
    assert all(a[0] < b[0] for a, b in zip(ents, ents[1:]))
    if count < k:
        assert hn == mn and scanned == size, (what, hn, scanned, mn, size)
    else:
        assert hn == min((h, n) for n, h in entries), (what, hn)
        assert entries[-1][0] - lo + 1 <= scanned <= size, (what, scanned, entries[-1][0], size)
    assert path in (0, 1, 2)
    return got


def fused(gpu, reqs, fuse):
    """Per request whether the plan of its flags fuses it (host only)."""
    plan = gpu.batch_plan_ex([r[:3] for r in reqs], fuse_fast=fuse)
    kinds = {}
    for p in plan:
        kinds.setdefault(p["req"], set()).add(p["kind"])
    assert set(kinds) == set(range(len(reqs)))
    return [1 not in kinds[i] for i in range(len(reqs))], plan


def parity_requests():
    msg, lo, hi = CMU
    targets = {T10(6): 4, T10(5): 17, T10(4): 192, CMU_MIN[0]: 1, CMU_MIN[0] - 1: 0, 0: 0}
    reqs = []
    for T, count in targets.items():
        assert ref(msg, lo, hi, T, 1)[0] == count, (T, count)
        for k in sorted({1, 2, 16, count - 1, count, count + 1}):
            if k >= 1:
                reqs.append((msg, lo, hi, T, k))
    second, third = (b"cmu441", 0, 999_999), (b"x" * 60, 1_000_000, 1_499_999)
    reqs[7:7] = [second + (T10(5), 4), third + (T10(4), 300)]
    reqs += [second + (T10(4), 2), third + (0, 1)]
    for r in reqs:                        # no range holds more hits than its region: overflow is impossible
        assert ref(*r[:4], 1)[0] <= 256 <= want(r[4]), r
    return reqs


def test_parity_small_shapes_one_call(gpu):
    reqs = parity_requests()
    assert len(reqs) >= 30 and len({r[0] for r in reqs}) == 3
    singles = {}
    for r in reqs:
        msg, lo, hi, T, k = r
        count = ref(*r)[0]
        if k == 1:
            f = gpu.search_first(msg, lo, hi, T)
            singles[r] = ("first", f)
        elif k >= count:
            singles[r] = ("hits", gpu.search_hits(msg, lo, hi, T, k))
    answers = {}
    for fuse in BOTH:
        ok, plan = fused(gpu, reqs, fuse)
        assert all(ok) and {p["pass"] for p in plan} == {0}          # every request is fused, one pass
        for kv in ({}, dict(MINEHIP_FIRST_BATCH_ORDER="request"), dict(MINEHIP_BATCH_SLOTS=4000)):
            with env(**kv):
                ok, plan = fused(gpu, reqs, fuse)
                assert all(ok), kv
                if "MINEHIP_BATCH_SLOTS" in kv:
                    assert max(p["pass"] for p in plan) >= 3             # the batch spans several passes
                res = gpu.search_first_hits_batch(reqs, fuse_fast=fuse)
            for i, (r, g) in enumerate(zip(reqs, res)):
                check(r, g, what=(fuse, kv, i))
                assert g[3] == 0, (fuse, kv, i, g[3])                    # answered from the fused pass
                answers.setdefault(i, set()).add((tuple(g[0]), g[1]))
                if r in singles and singles[r][0] == "first":
                    assert (len(g[0]) == 1,) + g[1] == singles[r][1][:3], (i, g, singles[r])
                if r in singles and singles[r][0] == "hits":
                    assert (len(g[0]), g[0], g[1]) == singles[r][1], (i, g[:2])
    assert all(len(v) == 1 for v in answers.values())                    # identical across orders, passes and flags


def test_every_fast_layout(gpu):
    from test_abi import KERNELS, KERNEL_CASE_NONCES, kernel_cases
    cases = kernel_cases()
    assert set(cases) == KERNELS and len(KERNELS) == 26
    planned = set()
    for Ld in (1, 3):
        for early in (1, 0):
            reqs, exps, layout = [], [], []
            for (J, mode), (m, lo, _, e) in sorted(cases.items()):
                if e != early:
                    continue
                hi = lo + KERNEL_CASE_NONCES + 3_456
                h = full_hashes(m, lo, hi)
                T5, T1 = int(np.sort(h)[4]), int(h.min())
                assert T5 == kth_smallest_hash(m, lo, hi, 5) if (J, mode) == (0, 0) else True
                five = ref(m, lo, hi, T5, 16, h)
                assert five[0] == 5 and five[1][-1][0] - five[1][0][0] > 2560, (J, mode)      # over more than one chunk
                assert ref(m, lo, hi, T1 - 1, 16, h)[:2] == (0, [])
                for k, T in ((1, T5), (3, T5), (5, T5), (6, T5), (3, T1 - 1)):
                    reqs.append((m, lo, hi, T, k))
                    exps.append(ref(m, lo, hi, T, k, h))
                    layout.append((J, mode))
            with env(**FAST, MINEHIP_LOWER_DIGITS=Ld, MINEHIP_EARLY=early):
                ok, plan = fused(gpu, reqs, True)
                assert all(ok)
                for p in plan:
                    if p["kind"] == 2 and (p["word"], p["mode"]) == layout[p["req"]]:
                        planned.add(layout[p["req"]])
                res = gpu.search_first_hits_batch(reqs, fuse_fast=True)
            for i, (r, g, x) in enumerate(zip(reqs, res, exps)):
                check(r, g, x, what=(Ld, early, layout[i], r[4]))
                assert g[3] == 0, (Ld, early, layout[i], g[3])           # five hits at most, regions of 256
    assert planned == KERNELS, KERNELS - planned                        # all 26 layouts ran as fused fast pieces


def test_the_stop_is_live_and_is_per_request(gpu):
    msg, lo, hi = b"cmu440", 1_000_000, 1_999_999
    shift, n_slices = slices_of(lo, hi)
    assert (shift, n_slices) == (10, 977)

    def settled(hits, k):
        counts = [0] * n_slices
        for n in hits[:k]:
            counts[(n - lo) >> shift] += 1
        return bound_of(lo, hi, k, counts)

    floors = [lo + c * 256_000 for c in range(4)]
    hits6 = [n for n, _ in ref(msg, lo, hi, T10(6), 16)[1]]
    assert hits6 == [1_067_492, 1_456_236, 1_999_610]
    assert settled(hits6, 2) == 1_456_703 < floors[2]                    # below chunks 2 and 3
    hits5 = [n for n, _ in ref(msg, lo, hi, T10(5), 16)[1]]
    assert hits5[:4] == [1_067_492, 1_099_412, 1_120_285, 1_203_279] and hits5[4] >= floors[1]
    assert settled(hits5, 4) == 1_203_775 < floors[1]                    # all four in chunk 0
    D, E = (b"cmu441", lo, hi), (b"x" * 60, lo, hi)
    reqs = [(msg, lo, hi, T10(6), 2), (msg, lo, hi, T10(6), 4), (msg, lo, hi, T10(5), 4), D + (0, 3), E + (0, 1)]
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        ok, plan = fused(gpu, reqs, True)
        assert all(ok) and len(plan) == 5
        for p in plan:                   # one fast piece of four 256,000-nonce chunks each
            assert (p["kind"], p["first"], p["count"], p["slots"], p["lo_digits"]) == (2, lo, 1_000_000, 4, 3), p
        res = gpu.search_first_hits_batch(reqs, fuse_fast=True)
        mn = gpu.search(msg, lo, hi)
    a, b, c, d, e = [check(r, g, what=i) for i, (r, g) in enumerate(zip(reqs, res))]
    print("scanned of 1,000,000: A %d, B %d, C %d, D %d, E %d" % (a[2], b[2], c[2], d[2], e[2]))
    assert [g[3] for g in res] == [0] * 5
    assert [n for n, _ in a[0]] == hits6[:2] and 456_237 <= a[2] < 1_000_000, a
    assert len(b[0]) == 3 and b[2] == 1_000_000 and b[1] == mn, b       # A's bound did not stop B
    assert [n for n, _ in c[0]] == hits5[:4] and 203_280 <= c[2] < 1_000_000, c
    assert d[0] == [] and d[2] == 1_000_000 and e[0] == [] and e[2] == 1_000_000   # ... nor D, nor E


def test_generic_tiles_skip(gpu):
    ranges = [(b"cmu440-%02d" % i, 0, 999_999) for i in range(64)]
    dense = [r + (T10(3), 4) for r in ranges]
    sparse = [r + (T10(4), 2) for r in ranges]
    exp_dense, exp_sparse = [], []
    for r in ranges:
        h = full_hashes(*r)
        exp_dense.append(ref(*r, T10(3), 4, h))
        exp_sparse.append(ref(*r, T10(4), 2, h))
    assert all(800 < x[0] < 1_200 for x in exp_dense)                    # about 1,000 hits per range
    assert all(2 <= x[0] <= 256 for x in exp_sparse)                     # within a region of 256: no overflow
    ok, plan = fused(gpu, dense, False)
    assert all(ok) and {p["kind"] for p in plan} == {0} and {p["pass"] for p in plan} == {0}
    res = gpu.search_first_hits_batch(dense, fuse_fast=False)
    for i, (r, g, x) in enumerate(zip(dense, res, exp_dense)):
        check(r, g, x, what=i)
    scanned = sum(g[2] for g in res)
    print("dense: scanned %d of %d, paths %s" % (scanned, 64 * 1_000_000, sorted({g[3] for g in res})))
    assert scanned < 64 * 1_000_000
    res = gpu.search_first_hits_batch(sparse, fuse_fast=False)
    for i, (r, g, x) in enumerate(zip(sparse, res, exp_sparse)):
        check(r, g, x, what=i)
    print("sparse: scanned %d of %d" % (sum(g[2] for g in res), 64 * 1_000_000))
    assert [g[3] for g in res] == [0] * 64


def test_rebuild_and_small_buffer(gpu):
    # Every nonce of 10,124 hits; the region is 400 entries.  The range is one entry of four tiles
    # (decades 9,500 .. 10,512: 2,560, 2,560, 2,560 and 2,444 nonces).  A tile is skipped only above
    # a published bound, a bound needs k = 100 counted hits, and there is no stop inside a tile: the
    # first tile to run appends all of its 2,444 or more hits, so more than 400 appends are certain
    # whatever the timing: path 2.
    r = (b"cmu440", 95_000, 105_123, U64, 100)
    exp = hits_ref(*r)
    assert exp[0] == 10_124 and [n for n, _ in exp[1]] == list(range(95_000, 95_100)) and want(100) == 400 < 2_560
    for fuse in BOTH:
        ok, _ = fused(gpu, [r], fuse)
        assert ok == [True]
        regs = gpu.first_hits_batch_regions([r], fuse_fast=fuse)
        assert (regs[0]["kind"], regs[0]["slots"]) == (0, 400)
        (g,) = gpu.search_first_hits_batch([r], fuse_fast=fuse)
        check(r, g, exp, what=fuse)
        assert g[3] == 2, g[3]
    reqs = parity_requests()
    default = gpu.search_first_hits_batch(reqs)
    for slots in (64, 1):
        with env(MINEHIP_HITS_SLOTS=slots):
            for fuse in BOTH:
                res = gpu.search_first_hits_batch(reqs, fuse_fast=fuse)
                for i, (q, g, d) in enumerate(zip(reqs, res, default)):
                    check(q, g, what=(slots, fuse, i))
                    assert g[:2] == d[:2], (slots, fuse, i)
                print("MINEHIP_HITS_SLOTS=%d fuse=%s: paths %s" % (slots, fuse, [g[3] for g in res]))
                assert all(g[3] in (0, 2) for g in res)


def test_edges_and_errors_beside_fused_requests(gpu):
    H = lambda m, n: hits_ref(m, n, n, U64, 1)[1][0][1]    # noqa: E731  (the oracle's Hash(m, n))
    top = (b"q" * 60, U64 - 30_000, U64)
    T3 = kth_smallest_hash(*top, 3)
    assert hits_ref(*top, T3, 8)[0] == 3
    h0, h1 = H(b"cmu440", 123_456_789), H(b"", U64)
    big = (b"cmu440", 0, 2 * 10 ** 9 - 1, T10(6), 2)                    # more than 10^9 nonces, hits at 393,322 and 1,067,492
    assert [n for n, _ in ref(*CMU, T10(6), 2)[1]] == [393_322, 1_067_492]
    reqs = [(b"cmu440", 123_456_789, 123_456_789, h0, 4), (b"cmu440", 123_456_789, 123_456_789, h0 - 1, 4),
            (b"x", 5, 4, 7, 2),                                          # lower > upper
            (b"", U64, U64, h1, 1), top + (T3, 2), (b"k0", 0, 1000, U64, 0),      # k == 0
            top + (T3, 3), (b"big", 0, 1000, U64, (1 << 20) + 1),       # oversized k
            top + (T3, 4), (b"y" * ((1 << 20) + 1), 0, 10, 7, 2),       # over-long message
            (b"cmu440", 0, 2_999, T10(3), 3), big]
    bad = {2: gpu.MH_ERANGE, 5: gpu.MH_EINVAL, 7: gpu.MH_EINVAL, 9: gpu.MH_ETOOLONG}
    offsets, total = [], 0
    for r in reqs:
        offsets.append(total)
        total += r[4] if r[4] <= gpu.MH_HITS_MAX_CAP else 0
    single_big = gpu.search_first_hits(*big)
    for fuse in BOTH:
        res = gpu.search_first_hits_batch(reqs, fuse_fast=fuse, errors="return")
        for i, (r, g) in enumerate(zip(reqs, res)):
            if i in bad:
                assert isinstance(g, gpu.MinehipError) and g.code == bad[i], (i, g)
            elif i == len(reqs) - 1:
                assert g[3] == 1 and g[:2] == single_big[:2], (g[1:], single_big[1:])       # the single call's answer
                assert [n for n, _ in g[0]] == [393_322, 1_067_492] and 1_067_493 <= g[2] <= 2 * 10 ** 9
            else:
                check(r, g, hits_ref(*r), what=(fuse, i))
                assert g[3] == 0, (fuse, i, g[3])
        assert res[0][:3] == ([(123_456_789, h0)], (h0, 123_456_789), 1) and res[1][:3] == ([], (h0, 123_456_789), 1)
        # the offsets follow the rule (the binding asserts each against the sum of k as the library counts it)
        import ctypes
        arr, keep, offs, tot = gpu._first_hits_requests(reqs)
        assert offs == offsets and tot == total
        out = (gpu.mh_first_hits_result * len(reqs))()
        buf = (gpu.mh_hit * total)()
        rc = gpu.lib.mh_search_first_hits_batch(0, arr, len(reqs), 1 if fuse else 0, buf, total, out)
        assert rc == gpu.MH_OK and [o.offset for o in out] == offsets
        assert [o.status for o in out] == [bad.get(i, gpu.MH_OK) for i in range(len(reqs))]
        del ctypes
    # flags == 0 on a request with fast pieces: a fallback
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        r = (b"cmu440", 1_000_000, 1_999_999, T10(6), 2)
        assert fused(gpu, [r], False)[0] == [False] and fused(gpu, [r], True)[0] == [True]
        (g,) = gpu.search_first_hits_batch([r], fuse_fast=False)
        check(r, g)
        assert g[3] == 1
        (g,) = gpu.search_first_hits_batch([r], fuse_fast=True)
        check(r, g)
        assert g[3] == 0


def test_profile_counts_the_fused_tiles_and_fast_pieces(gpu):
    lo, hi = 1_000_000, 1_999_999
    reqs = [(b"cmu440", lo, hi, T10(6), 4), (b"cmu441", lo, hi, 0, 1), (b"cmu440", 0, 99_999, T10(4), 2)]
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        ok, plan = fused(gpu, reqs, True)
        assert all(ok)
        fast = [p for p in plan if p["kind"] == 2]
        gen = [p for p in plan if p["kind"] == 0]
        assert len(fast) >= 2 and gen
        gpu.profile_enable(0, True)
        try:
            before = gpu.profile_read(0)
            res = gpu.search_first_hits_batch(reqs, fuse_fast=True)
            after = gpu.profile_read(0)
            kernels = gpu.profile_kernels(0)
        finally:
            gpu.profile_enable(0, False)
    for r, g in zip(reqs, res):
        check(r, g)
    d = {k: after[k] - before[k] for k in after}
    assert d["fast_launches"] == len({(p["pass"], p["launch"]) for p in fast})
    assert d["fast_nonces"] == sum(p["count"] for p in fast) >= 2_000_000
    assert d["generic_nonces"] == sum(p["count"] for p in gen)
    assert d["fast_ns"] > 0 and d["fast_ops"] > 0 and d["fast_slots"] > 0
    assert {(p["word"], p["mode"], p["lo_digits"]) for p in fast} <= {(k["word"], k["mode"], k["lo_digits"]) for k in kernels if k["nonces"]}
