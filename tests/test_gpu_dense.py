"""Every nonce of every layout through the four hits builds of fast_search.hip.

csrc/fast_search.hip is compiled once per embedded code object, each with its own -DMH_FIRST /
-DMH_HITS / -DMH_BATCH / -DMH_STOP combination, and the per-nonce loop differs between the builds
(the kwg[] hoist, the form of round J, the operand selection of round_kw, laundered kernarg
pointers); the append paths also rebuild a nonce per hit, which the product kernel does not.  The
dev build's hash hooks verify fast_search and batch_fast per nonce (tests/test_gpu_probe.py,
tests/test_gpu_batch_fast.py); the other builds refuse those hooks.  The hits family needs none:
with target 2^64 - 1 every nonce of the range is a hit, so the product library itself hands back
(hash, nonce) of every nonce -- one search per layout, through the shipped code objects:

  hits_scan    mh_search_hits                       cap = N
  hits_stop    mh_search_first_hits                 k = N and k = N // 2
  batch_hits   mh_search_hits_batch_ex(FUSE_FAST)   three layouts' requests per call, cap = N each
  batch_bound  mh_search_first_hits_batch(FUSE_FAST) the same, k = N and k = N // 2

over test_abi.kernel_cases()' range of each of the 26 layouts plus 3,456 nonces (N = 253,457), at
MINEHIP_LOWER_DIGITS 1 (one group, 99 chunks, ragged waves) and 3 (100 groups, 253 lanes in one
chunk).  k = N // 2 is the case where every wave step counts 64 hits into the slice counters and
the bound is published while every chunk is appending; its region min(N, max(4 k, 256)) is still
N, so nothing overflows and no list is rebuilt through another path (asserted on the host).  The
device hit buffer holds 2^20 >= 3 N entries, so no window walk replaces the kernels' own entries.

Reference: test_gpu_ties.full_hashes (the CPU oracle's hash of every nonce, once per range),
compared bit for bit with np.array_equal.  The C ABI is called directly with a numpy buffer as
mh_hit*, poisoned with 2^64 - 1 before each call: the bindings' Python lists would take 0.1-0.25 s
per 253,457 entries.  On a mismatch dense_diff names the layout, L, the first differing index, the
plan piece it lies in, its lane, group and digit and how many entries differ.

Each test first asserts from the plans alone that the layouts run as fast pieces (dense_plans).
test_generic_dense does the same for generic_scan_hits and generic_scan_hits_stop on the default
plan at the u64 edges and the powers of ten.

Measured on an MI355X (one run each), seconds.  The first test to run also computes the reference
of the 26 ranges (0.7 s, shared by the others):
  hits_scan    L = 1: 1.1   L = 3: 1.5        batch_hits   L = 1: 0.2   L = 3: 0.6
  hits_stop    L = 1: 1.2   L = 3: 3.6        batch_bound  L = 1: 0.4   L = 3: 2.7
  generic: 0.07
So a dense search of 253,457 hits, with its copy-back and the comparison here, takes about 15 ms
at L = 1 and 55 ms at L = 3 through hits_scan, and about 70 ms at L = 3 through hits_stop.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_parity import env
from test_gpu_ties import full_hashes

U64 = (1 << 64) - 1
FAST = dict(MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1)
LDS = (1, 3)
GROUP = 3           # layouts per batch call: 3 N <= 2^20 entries of the device hit buffer


def case_env(Ld, early):
    return dict(FAST, MINEHIP_LOWER_DIGITS=Ld, MINEHIP_EARLY=early)


@functools.lru_cache(maxsize=None)
def dense_cases():
    """[((J, mode), msg, lo, hi, early)] sorted by layout: test_abi.kernel_cases()' ranges plus 3,456
    nonces, the ranges of test_every_fast_layout and test_gpu_probe.fast_kernel_cases."""
    from test_abi import KERNELS, KERNEL_CASE_NONCES, kernel_cases
    cases = kernel_cases()
    assert set(cases) == KERNELS and len(KERNELS) == 26
    return [(k, m, lo, lo + KERNEL_CASE_NONCES + 3_456, early) for k, (m, lo, _, early) in sorted(cases.items())]


def N_of(lo, hi):
    return hi - lo + 1


def groups():
    cases = dense_cases()
    return [cases[i:i + GROUP] for i in range(0, len(cases), GROUP)]


@functools.lru_cache(maxsize=None)
def dense_plans(batch):
    """{(layout, Ld): pieces}: minehip.plan of each case (batch False), or the case's pieces of
    batch_plan_ex over its group of three (batch True), under the search's environment.  Asserts
    what the tests rest on, from the plans alone: every layout runs as a fast piece (kind 0; of a
    fused request: kind 2) of its own kernel at one of the two L at least -- at L = 3 all but
    <0, OneEarly>, whose range then runs <1, One> -- and those pieces hold at least 60 nonces:
    <0, One>'s hold 990 of its range (the buckets [10, 99] and [100, 999]), every other layout's
    3,460 or more."""
    import minehip
    from test_abi import KERNELS
    fast_kind = 2 if batch else 0
    out, own_count = {}, {}
    for Ld in LDS:
        for grp in groups():
            early = grp[0][4]
            assert all(c[4] == early for c in grp)          # one MINEHIP_EARLY per call (read per call)
            with env(**case_env(Ld, early)):
                if batch:
                    plan = minehip.batch_plan_ex([c[1:4] for c in grp], fuse_fast=True)
                    per = [[p for p in plan if p["req"] == i] for i in range(len(grp))]
                else:
                    per = [minehip.plan(*c[1:4]) for c in grp]
            for (k, m, lo, hi, _), pieces in zip(grp, per):
                assert {p["kind"] for p in pieces} <= {fast_kind, 0 if batch else 1}, (k, Ld, pieces)   # fused / no fallback
                assert sum(p["count"] for p in pieces) == N_of(lo, hi), (k, Ld)
                out[(k, Ld)] = pieces
                own_count[(k, Ld)] = sum(p["count"] for p in pieces
                                         if p["kind"] == fast_kind and (p["word"], p["mode"]) == k)
                assert any(p["kind"] == fast_kind for p in pieces), (k, Ld)
    for k in KERNELS:
        assert own_count[(k, 1)] >= 60, (k, own_count[(k, 1)])                  # every layout is planned at L = 1
        assert (own_count[(k, 3)] >= 60) == (k != (0, 3)), (k, own_count[(k, 3)])
    assert own_count[((0, 0), 1)] == own_count[((0, 0), 3)] == 990 and own_count[((0, 3), 3)] == 0
    assert min(v for (k, _), v in own_count.items() if k != (0, 0) and v) >= 3_460
    return out


def piece_of(pieces, n):
    for p in pieces:
        if p["first"] <= n < p["first"] + p["count"]:
            return p
    return None


def dense_diff(got, h, lo, pieces=(), what=None):
    """None when the rows (hash, nonce) of `got` are exactly (h[i], lo + i); otherwise a report for
    the next reader: the case, the first differing index and its nonce, the plan piece it lies in,
    its lane, group and digit there (n // 10^L - first // 10^L, n % 10^L // 10, n % 10; of an Early
    piece the lane is by value, not by launch order), how many entries differ, and both rows."""
    exp = np.stack([np.asarray(h, dtype=np.uint64), np.uint64(lo) + np.arange(len(h), dtype=np.uint64)], axis=1)
    if got.shape == exp.shape and np.array_equal(got, exp):
        return None
    n_cmp = min(len(got), len(exp))
    bad = (got[:n_cmp] != exp[:n_cmp]).any(axis=1)
    if not bad.any():
        return "%s: %d entries where %d are expected (the common prefix agrees)" % (what, len(got), len(exp))
    i = int(bad.argmax())
    n = lo + i
    p = piece_of(pieces, n)
    where = "no plan piece"
    if p is not None:
        R = 10 ** max(p.get("lo_digits", 0), 0)
        where = "piece kind %d <%d, %d> L = %d first %d count %d: lane %d, group %d, digit %d" % (
            p["kind"], p.get("word", 0), p.get("mode", 0), p.get("lo_digits", 0), p["first"], p["count"],
            n // R - p["first"] // R, n % R // 10, n % 10)
    return ("%s: %d of %d entries differ (%d rows for %d), the first at index %d, nonce %d (%s): "
            "got (%016x, %d), expected (%016x, %d)") % (
        what, int(np.count_nonzero(bad)), n_cmp, len(got), len(exp), i, n, where,
        int(got[i, 0]), int(got[i, 1]), int(exp[i, 0]), int(exp[i, 1]))


def first_min(h, lo):
    """(hash, nonce) of the first minimum of h."""
    i = int(np.asarray(h).argmin())
    return int(h[i]), lo + i


def hit_buffer(entries):
    """A (entries, 2) uint64 array to pass as mh_hit*, poisoned: an entry the library does not write
    cannot equal the reference (nor what an earlier call left in recycled memory)."""
    import minehip
    buf = np.full((max(1, entries), 2), U64, dtype=np.uint64)
    return buf, buf.ctypes.data_as(ctypes.POINTER(minehip.mh_hit))


def check_all_hits(rows, count, stored, hn, h, lo, pieces, what):
    """The hits_scan assertions: count == stored == N, the nonce column lo + arange(N) and the hash
    column the reference's, the minimum the reference's first minimum."""
    N = len(h)
    assert count == stored == N, (what, count, stored, N)
    msg = dense_diff(rows, h, lo, pieces, what)
    assert msg is None, msg
    assert np.array_equal(rows[:, 1], np.uint64(lo) + np.arange(N, dtype=np.uint64)) and np.array_equal(rows[:, 0], h)
    assert hn == first_min(h, lo), (what, hn, first_min(h, lo))


def check_first_k(rows, stored, scanned, hn, k, h, lo, pieces, what):
    """The hits_stop assertions for k <= N: exactly the nonces lo .. lo + k - 1 with their hashes,
    the lexicographic minimum of those k entries, k <= scanned <= N (== N for k == N)."""
    N = len(h)
    assert stored == k == len(rows), (what, stored, k)
    msg = dense_diff(rows, h[:k], lo, pieces, what)
    assert msg is None, msg
    assert hn == first_min(h[:k], lo), (what, hn, first_min(h[:k], lo))
    assert k <= scanned <= N, (what, k, scanned, N)


# ---- CPU tests -------------------------------------------------------------------------------------

def test_dense_plans_and_the_comparison():
    """The plans the GPU tests rest on (dense_plans' assertions, both call shapes), the region rules,
    and the comparison helper itself: one flipped bit of one reference hash inside a fast piece, a
    wrong or missing nonce, and a short list are each reported at their index."""
    import minehip
    single, batch = dense_plans(False), dense_plans(True)
    assert len(single) == len(batch) == 52
    assert len(groups()) == 9
    for Ld in LDS:
        for grp in groups():
            with env(**case_env(Ld, grp[0][4])):
                N = N_of(*grp[0][2:4])
                assert N == 253_457 <= minehip.MH_HITS_MAX_CAP and GROUP * N <= minehip.MH_HITS_MAX_CAP
                regs = minehip.hits_batch_regions([c[1:4] + (U64, N) for c in grp], fuse_fast=True)
                assert [(r["kind"], r["window"], r["slots"]) for r in regs] == [(0, 0, N)] * len(grp), (Ld, regs)
                for k in (N, N // 2):
                    assert min(N, max(4 * k, 256)) == N
                    regs = minehip.first_hits_batch_regions([c[1:4] + (U64, k) for c in grp], fuse_fast=True)
                    assert [(r["kind"], r["window"], r["slots"]) for r in regs] == [(0, 0, N)] * len(grp), (Ld, k, regs)
    k, m, lo, hi, early = dense_cases()[7]
    pieces = single[(k, 3)]
    fast = [p for p in pieces if p["kind"] == 0 and (p["word"], p["mode"]) == k]
    h = full_hashes(m, lo, hi)
    good = np.stack([h, np.uint64(lo) + np.arange(len(h), dtype=np.uint64)], axis=1)
    assert dense_diff(good, h, lo, pieces, "same") is None
    n = fast[0]["first"] + 64 * 1000 + 537           # lane 64, group 53, digit 7 of the L = 3 piece
    assert fast[0]["lo_digits"] == 3 and fast[0]["first"] <= n < fast[0]["first"] + fast[0]["count"]
    flipped = h.copy()
    flipped[n - lo] ^= np.uint64(1 << 17)
    rep = dense_diff(good, flipped, lo, pieces, (k, 3))
    assert rep is not None and "1 of %d entries differ" % len(h) in rep and "index %d, nonce %d " % (n - lo, n) in rep, rep
    assert "<%d, %d> L = 3" % k in rep and "lane 64, group 53, digit 7" in rep, rep
    wrong = good.copy()
    wrong[1000:, 1] += np.uint64(1)                  # a dropped nonce: everything after it shifts
    rep = dense_diff(wrong, h, lo, pieces, (k, 3))
    assert "%d of %d entries differ" % (len(h) - 1000, len(h)) in rep and "index 1000," in rep, rep
    assert "entries where" in dense_diff(good[:-1], h, lo, pieces, "short")
    with pytest.raises(AssertionError):
        check_all_hits(good, len(h), len(h), first_min(h, lo), flipped, lo, pieces, "flipped")
    with pytest.raises(AssertionError):
        check_first_k(good[:500], 500, 500, first_min(h[:500], lo), 500, flipped[:500] ^ np.uint64(1), lo, pieces, "flipped")
    check_all_hits(good, len(h), len(h), first_min(h, lo), h, lo, pieces, "good")
    check_first_k(good[:500], 500, 777, first_min(h[:500], lo), 500, h, lo, pieces, "good")


# ---- GPU tests -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_hits_scan_every_nonce(gpu, Ld):
    plans = dense_plans(False)
    for k, m, lo, hi, early in dense_cases():
        h, N = full_hashes(m, lo, hi), N_of(lo, hi)
        buf, ptr = hit_buffer(N)
        out = gpu.mh_hits()
        with env(**case_env(Ld, early)):
            rc = gpu.lib.mh_search_hits(0, m, len(m), lo, hi, U64, ptr, N, ctypes.byref(out))
        assert rc == gpu.MH_OK, (k, Ld, gpu.lib.mh_last_error())
        check_all_hits(buf[:out.stored], out.count, out.stored, (out.hash, out.nonce), h, lo, plans[(k, Ld)],
                       ("hits_scan", k, Ld))


@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_hits_stop_every_nonce(gpu, Ld):
    plans = dense_plans(False)
    for k, m, lo, hi, early in dense_cases():
        h, N = full_hashes(m, lo, hi), N_of(lo, hi)
        assert N <= gpu.MH_HITS_MAX_CAP          # no window walk can replace the kernels' own entries
        for kk in (N, N // 2):
            buf, ptr = hit_buffer(kk)
            out = gpu.mh_first_hits()
            with env(**case_env(Ld, early)):
                rc = gpu.lib.mh_search_first_hits(0, m, len(m), lo, hi, U64, ptr, kk, ctypes.byref(out))
            assert rc == gpu.MH_OK, (k, Ld, kk, gpu.lib.mh_last_error())
            what = ("hits_stop", k, Ld, "k = %d" % kk)
            if kk == N:
                check_all_hits(buf[:out.stored], out.stored, out.stored, (out.hash, out.nonce), h, lo, plans[(k, Ld)], what)
                assert out.scanned == N, (what, out.scanned)
            else:
                check_first_k(buf[:out.stored], out.stored, out.scanned, (out.hash, out.nonce), kk, h, lo,
                              plans[(k, Ld)], what)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_batch_hits_every_nonce(gpu, Ld):
    plans = dense_plans(True)
    for grp in groups():
        N = N_of(*grp[0][2:4])
        reqs = [c[1:4] + (U64, N) for c in grp]
        arr, keep, offsets, total = gpu._hits_requests(reqs, 0)
        assert total == len(grp) * N <= gpu.MH_HITS_MAX_CAP
        buf, ptr = hit_buffer(total)
        out = (gpu.mh_hits_result * len(grp))()
        with env(**case_env(Ld, grp[0][4])):
            regs = gpu.hits_batch_regions(reqs, fuse_fast=True)
            assert [(r["window"], r["slots"]) for r in regs] == [(0, N)] * len(grp), regs
            rc = gpu.lib.mh_search_hits_batch_ex(0, arr, len(grp), gpu.MH_BATCH_FUSE_FAST, ptr, total, out)
        assert rc == gpu.MH_OK, (Ld, gpu.lib.mh_last_error())
        for (k, m, lo, hi, _), o, off in zip(grp, out, offsets):
            assert o.status == gpu.MH_OK and o.offset == off, (k, Ld, o.status, o.offset)
            check_all_hits(buf[off:off + o.stored], o.count, o.stored, (o.hash, o.nonce), full_hashes(m, lo, hi), lo,
                           plans[(k, Ld)], ("batch_hits", k, Ld))


@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_batch_bound_every_nonce(gpu, Ld):
    plans = dense_plans(True)
    for grp in groups():
        N = N_of(*grp[0][2:4])
        for kk in (N, N // 2):
            reqs = [c[1:4] + (U64, kk) for c in grp]
            arr, keep, offsets, total = gpu._first_hits_requests(reqs)
            buf, ptr = hit_buffer(total)
            out = (gpu.mh_first_hits_result * len(grp))()
            with env(**case_env(Ld, grp[0][4])):
                regs = gpu.first_hits_batch_regions(reqs, fuse_fast=True)
                assert [(r["window"], r["slots"]) for r in regs] == [(0, N)] * len(grp), regs      # min(N, max(4 k, 256)) == N
                rc = gpu.lib.mh_search_first_hits_batch(0, arr, len(grp), gpu.MH_BATCH_FUSE_FAST, ptr, total, out)
            assert rc == gpu.MH_OK, (Ld, kk, gpu.lib.mh_last_error())
            for (k, m, lo, hi, _), o, off in zip(grp, out, offsets):
                what = ("batch_bound", k, Ld, "k = %d" % kk)
                assert o.status == gpu.MH_OK and o.offset == off, (what, o.status, o.offset)
                assert o.path == 0, (what, o.path)                  # the fused pass's own entries, not a rebuild
                h, rows = full_hashes(m, lo, hi), buf[off:off + o.stored]
                if kk == N:
                    check_all_hits(rows, o.stored, o.stored, (o.hash, o.nonce), h, lo, plans[(k, Ld)], what)
                    assert o.scanned == N, (what, o.scanned)
                else:
                    check_first_k(rows, o.stored, o.scanned, (o.hash, o.nonce), kk, h, lo, plans[(k, Ld)], what)


@pytest.mark.gpu
def test_generic_dense(gpu):
    """generic_scan_hits and generic_scan_hits_stop: every nonce of test_gpu_probe's generic ranges
    (<= 30,001 nonces each, lo = 0, hi = 2^64 - 1, straddles of 10^1, 10^5 and 10^19) on the default
    plan, all generic pieces."""
    from test_gpu_probe import GENERIC_MSGS, GENERIC_RANGES
    assert any(lo == 0 for lo, _ in GENERIC_RANGES) and any(hi == U64 for _, hi in GENERIC_RANGES)
    for m in GENERIC_MSGS:
        for lo, hi in GENERIC_RANGES:
            pieces = gpu.plan(m, lo, hi)
            assert pieces and all(p["kind"] == 1 for p in pieces), (m[:8], lo, hi)
            h, N = full_hashes(m, lo, hi), N_of(lo, hi)
            assert N <= 30_001
            buf, ptr = hit_buffer(N)
            out = gpu.mh_hits()
            rc = gpu.lib.mh_search_hits(0, m, len(m), lo, hi, U64, ptr, N, ctypes.byref(out))
            assert rc == gpu.MH_OK, gpu.lib.mh_last_error()
            check_all_hits(buf[:out.stored], out.count, out.stored, (out.hash, out.nonce), h, lo, pieces,
                           ("generic hits", m[:8], len(m), lo, hi))
            buf, ptr = hit_buffer(N)
            out = gpu.mh_first_hits()
            rc = gpu.lib.mh_search_first_hits(0, m, len(m), lo, hi, U64, ptr, N, ctypes.byref(out))
            assert rc == gpu.MH_OK, gpu.lib.mh_last_error()
            check_all_hits(buf[:out.stored], out.stored, out.stored, (out.hash, out.nonce), h, lo, pieces,
                           ("generic first_hits", m[:8], len(m), lo, hi))
            assert out.scanned == N
