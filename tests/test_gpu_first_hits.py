"""mh_search_first_hits on the GPU: the k smallest nonces whose hash is <= a target, from kernels
that stop once k of them are known (hits_stop<J, MODE>, generic_scan_hits_stop).  The entries are
bit for bit the first k of test_hits.hits_ref (the oracle's hashes of the whole range, in numpy)
under every plan and for every fast layout; stored, hash and nonce follow the contract; `scanned`
is the range's size when fewer than k nonces qualify and lies within [k-th hit - lower + 1, size]
otherwise; and the stop is shown live where the reference says chunks lie above the bound.

Every case asserts from the reference alone that it is live before it looks at the GPU."""
import os
import subprocess

import pytest

from conftest import PKG
from test_first import first_ref, kth_smallest_hash
from test_first_hits import bound_of, slices_of
from test_gpu_first import plans
from test_gpu_parity import env
from test_hits import hits_ref

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CMU = (b"cmu440", 0, 1_999_999)
CMU_MIN = (1228377698034, 1_067_492)          # the range's minimum (tests/test_cli.py, tests/test_abi.py)
CMU_HITS = {6: 4, 5: 17, 4: 192, 3: 2_003}    # target 2^64 // 10^j: hits of the range
CMU_K6 = [393_322, 1_067_492, 1_456_236, 1_999_610]
FAST = dict(MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1)
CHUNK1 = 2560  # nonces of one workgroup's chunk at L = 1 (256 lanes x 10)


def T10(j):
    return 2 ** 64 // 10 ** j


def check(gpu, msg, lo, hi, T, k, what=None):
    """One call against the reference and the contract; returns (entries, (hash, nonce), scanned)."""
    count, entries, mn = hits_ref(msg, lo, hi, T, k)
    got = gpu.search_first_hits(msg, lo, hi, T, k)
    size = hi - lo + 1
    assert got[0] == entries, (what, msg[:8], lo, hi, T, k, got[0][:3], len(got[0]), entries[:3], len(entries))
    assert len(got[0]) == min(count, k)
    assert all(a[0] < b[0] for a, b in zip(got[0], got[0][1:]))          # strictly increasing nonces
    if count < k:                     # the whole range was hashed, and the minimum is mh_search's
        assert got[1] == mn and got[2] == size, (what, got[1:], mn, size)
    else:                             # the lexicographic minimum (hash, nonce) of the k entries
        assert got[1] == min((h, n) for n, h in entries), (what, got[1])
        assert entries[-1][0] - lo + 1 <= got[2] <= size, (what, got[2], entries[-1][0], size)
    return got


def test_cmu440_under_every_plan(gpu):
    msg, lo, hi = CMU
    targets = {}
    for j, n in CMU_HITS.items():
        ref = hits_ref(msg, lo, hi, T10(j), 1 << 20)
        assert ref[0] == n == len(ref[1]) and ref[2] == CMU_MIN, j
        targets[T10(j)] = (n, "j=%d" % j)
    full3, full4 = hits_ref(msg, lo, hi, T10(3), 1 << 20)[1], hits_ref(msg, lo, hi, T10(4), 1 << 20)[1]
    assert full3[15][0] == 15_370 and full3[99][0] == 122_839 and full4[15][0] == 169_729          # the anchors
    assert [n for n, _ in hits_ref(msg, lo, hi, T10(6), 16)[1]] == CMU_K6
    assert hits_ref(msg, lo, hi, CMU_MIN[0], 16) == (1, [(CMU_MIN[1], CMU_MIN[0])], CMU_MIN)
    assert hits_ref(msg, lo, hi, CMU_MIN[0] - 1, 16) == (0, [], CMU_MIN) == hits_ref(msg, lo, hi, 0, 16)
    assert hits_ref(msg, lo, hi, U64, 2)[:2] == (2_000_000, [(0, first_ref(msg, 0, 0, U64)[1]), (1, first_ref(msg, 1, 1, U64)[1])])
    targets.update({CMU_MIN[0]: (1, "min"), CMU_MIN[0] - 1: (0, "min-1"), 0: (0, "zero"), U64: (2_000_000, "all")})
    assert len(targets) == 8
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        assert any(p["kind"] == 0 for p in gpu.plan(msg, lo, hi))       # those plans do run fast kernels
    results = {}
    for kv in plans():
        with env(**kv):
            for T, (count, name) in targets.items():
                ks = sorted(k for k in {1, 2, 16, count - 1, count, count + 1, 4_096} if 1 <= k <= gpu.MH_HITS_MAX_CAP)
                first = gpu.search_first(msg, lo, hi, T)
                every = gpu.search_hits(msg, lo, hi, T, 4_096) if count <= 4_096 else None
                for k in ks:
                    got = check(gpu, msg, lo, hi, T, k, (name, k, kv))
                    results.setdefault((name, k), set()).add((tuple(got[0]), got[1]))
                    if k == 1:        # stored, hash and nonce are mh_search_first's found, hash and nonce
                        assert (len(got[0]) == 1,) + got[1] == first[:3], (name, kv, got, first)
                    if every is not None and k >= count:  # ... and mh_search_hits' count, entries and minimum
                        assert (len(got[0]), got[0], got[1]) == every, (name, k, kv)
    assert len(plans()) == 9 and all(len(v) == 1 for v in results.values())          # identical across plans


def test_every_fast_layout(gpu):
    """Each of the 26 layouts over test_abi.kernel_cases()' range plus 3,456 nonces, at
    MINEHIP_LOWER_DIGITS in {1, 3} (each layout is planned at one of the two at least): exactly
    five hits spread over more than one chunk, k below, at and above five; and no hit."""
    from test_abi import KERNELS, KERNEL_CASE_NONCES, kernel_cases
    cases = kernel_cases()
    assert set(cases) == KERNELS and len(KERNELS) == 26
    interleaved, planned = set(), set()
    for (J, mode), (m, lo, _, early) in sorted(cases.items()):
        hi = lo + KERNEL_CASE_NONCES + 3_456
        T5, T1 = kth_smallest_hash(m, lo, hi, 5), kth_smallest_hash(m, lo, hi, 1)
        hits = [n for n, _ in hits_ref(m, lo, hi, T5, 16)[1]]
        assert hits_ref(m, lo, hi, T5, 16)[0] == 5 == len(hits) and hits[-1] - hits[0] > CHUNK1, (J, mode, hits)
        assert hits_ref(m, lo, hi, T1 - 1, 16)[:2] == (0, [])
        for Ld in (1, 3):
            with env(**FAST, MINEHIP_LOWER_DIGITS=Ld, MINEHIP_EARLY=early):
                pieces = [p for p in gpu.plan(m, lo, hi) if p["kind"] == 0 and (p["word"], p["mode"]) == (J, mode)]
                if pieces:
                    planned.add((J, mode))
                if mode >= 3:   # an Early piece at innermost position p >= L: its lanes interleave
                    t = (len(m) + 1) % 64
                    for pc in pieces:
                        pl = t + pc["digits"] - 1
                        base = 64 if (pc["blocks"] == 2 and pl >= 64) else 0
                        p = pl - (base + 4 * J + 3)
                        if p >= pc["lo_digits"] and any(pc["first"] <= n < pc["first"] + pc["count"] for n in hits):
                            interleaved.add((J, mode))
                for k in (1, 3, 5, 6):
                    check(gpu, m, lo, hi, T5, k, (J, mode, Ld, k))
                got = check(gpu, m, lo, hi, T1 - 1, 3, (J, mode, Ld, "none"))
                assert got == ([], gpu.search(m, lo, hi), hi - lo + 1), (J, mode, Ld, got)
    assert planned == KERNELS, KERNELS - planned
    assert interleaved == {k for k in KERNELS if k[1] >= 3}, interleaved


def test_the_stop_is_live_at_a_small_shape(gpu):
    """One fast piece of 1,000 runs x 1,000 nonces: four chunks of 256,000 nonces, all claimed at
    once, slices of 2^10 nonces.  The reference says where the hits lie, hence which slice end the
    bound settles at and which chunks lie wholly above it; those chunks are left at their next group."""
    msg, lo, hi = b"cmu440", 1_000_000, 1_999_999
    where = lambda n: ((n - lo) // 256_000, ((n - lo) % 1000) // 10)      # noqa: E731  (chunk, group) of a nonce
    floors = [lo + c * 256_000 for c in range(4)]
    shift, n_slices = slices_of(lo, hi)
    assert (shift, n_slices) == (10, 977)

    def settled(hits, k):             # the bound once the k smallest hits are counted
        counts = [0] * n_slices
        for n in hits[:k]:
            counts[(n - lo) >> shift] += 1
        return bound_of(lo, hi, k, counts)

    hits6 = [n for n, _ in hits_ref(msg, lo, hi, T10(6), 16)[1]]
    assert hits6 == [1_067_492, 1_456_236, 1_999_610] and [where(n) for n in hits6] == [(0, 49), (1, 23), (3, 61)]
    assert settled(hits6, 2) == 1_456_703 < floors[2]                    # below the floors of chunks 2 and 3
    hits5 = [n for n, _ in hits_ref(msg, lo, hi, T10(5), 16)[1]]
    assert len(hits5) == 10 and hits5[:4] == [1_067_492, 1_099_412, 1_120_285, 1_203_279]
    assert all(where(n)[0] == 0 and where(n)[1] <= 49 for n in hits5[:4]) and where(hits5[4])[0] > 0
    assert settled(hits5, 4) == 1_203_775 < floors[1]                    # below chunk 1's floor
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        pieces = gpu.plan(msg, lo, hi)
        assert len(pieces) == 1 and pieces[0]["kind"] == 0 and pieces[0]["mode"] < 3, pieces
        assert (pieces[0]["first"], pieces[0]["count"], pieces[0]["lo_digits"]) == (lo, 1_000_000, 3), pieces
        assert -(-(pieces[0]["count"] // 1000) // 256) == 4             # 1,000 runs: four chunks
        k2 = check(gpu, msg, lo, hi, T10(6), 2, "k=2")
        k3 = check(gpu, msg, lo, hi, T10(6), 3, "k=3")
        k4 = check(gpu, msg, lo, hi, T10(6), 4, "k=4")
        k4_5 = check(gpu, msg, lo, hi, T10(5), 4, "10^5, k=4")
        every = gpu.search_hits(msg, lo, hi, T10(6), 16)                # no early end there: the contrast
        assert k4[1] == gpu.search(msg, lo, hi)
    print("scanned of 1,000,000: k=2 %d, k=3 %d, k=4 %d; target 2^64//10^5, k=4 %d" % (k2[2], k3[2], k4[2], k4_5[2]))
    assert [n for n, _ in k2[0]] == hits6[:2] and 456_237 <= k2[2] < 1_000_000, k2
    assert [n for n, _ in k3[0]] == hits6 and k3[0] == every[1], k3
    assert len(k4[0]) == 3 and k4[2] == 1_000_000 and k4[0] == every[1] and k4[1] == every[2], k4
    assert [n for n, _ in k4_5[0]] == hits5[:4] and 203_280 <= k4_5[2] < 1_000_000, k4_5


def test_two_streams_default_plan(gpu):
    """The default plan over [0, 2^32): the small pieces that hold the four hits run beside a coarse
    launch whose later generations start after the bound is published."""
    msg, lo, hi = b"cmu440", 0, 2 ** 32 - 1
    ref = hits_ref(*CMU, T10(6), 4)           # the four hits of [0, 1,999,999] are the first four of any longer range
    assert ref[0] == 4 and [n for n, _ in ref[1]] == CMU_K6
    got = gpu.search_first_hits(msg, lo, hi, T10(6), 4)
    print("scanned of 2^32: %d" % got[2])
    assert got[0] == ref[1] and got[1] == min((h, n) for n, h in ref[1]) == CMU_MIN, got
    assert CMU_K6[-1] + 1 <= got[2] < 2 ** 32, got


def test_generic_only(gpu):
    msg, lo, hi = CMU
    assert all(p["kind"] == 1 for p in gpu.plan(msg, lo, hi))           # the default plan: generic tiles only
    assert hits_ref(msg, lo, hi, T10(3), 16)[1][15][0] == 15_370
    got = check(gpu, msg, lo, hi, T10(3), 16, "generic")
    print("scanned of 2,000,000: %d" % got[2])                          # which tiles had started is timing
    assert 15_371 <= got[2] <= 2_000_000


def test_overflow_walk(gpu):
    msg, lo, hi = CMU
    full = hits_ref(msg, lo, hi, T10(3), 1 << 20)
    assert full[0] == 2_003 and full[1][99][0] == 122_839
    for kv in ({}, dict(FAST, MINEHIP_LOWER_DIGITS=3), dict(FAST, MINEHIP_LOWER_DIGITS=1, MINEHIP_QUEUE=0)):
        with env(**kv):
            for k in (100, 64):
                default = check(gpu, msg, lo, hi, T10(3), k, kv)
                with env(MINEHIP_HITS_SLOTS=64):
                    got = check(gpu, msg, lo, hi, T10(3), k, kv)
                assert got[:2] == default[:2] and len(got[0]) == k, (kv, k)
            assert [n for n, _ in hits_ref(msg, 0, 3_000, T10(3), 3)[1]] == [1_081, 1_329, 2_080]
            default = check(gpu, msg, 0, 3_000, T10(3), 3, kv)
            with env(MINEHIP_HITS_SLOTS=1):
                assert check(gpu, msg, 0, 3_000, T10(3), 3, kv)[:2] == default[:2]


def test_edges(gpu):
    msg, lo, hi = b"cmu440", 95_000, 105_123
    ref = hits_ref(msg, lo, hi, U64, 100)
    assert ref[0] == 10_124 and [n for n, _ in ref[1]] == list(range(95_000, 95_100))   # every step of every lane hits
    for q in (0, 1):
        with env(**FAST, MINEHIP_LOWER_DIGITS=1, MINEHIP_QUEUE=q):
            pieces = gpu.plan(msg, lo, hi)
            assert any(p["kind"] == 0 for p in pieces) and any(p["kind"] == 1 for p in pieces)
            assert any(p["kind"] == 0 and (p["count"] // 10) % 64 for p in pieces), pieces    # partly filled waves
            check(gpu, msg, lo, hi, U64, 100, q)
    H = lambda m, n: hits_ref(m, n, n, U64, 1)[1][0][1]    # noqa: E731  (the oracle's Hash(m, n))
    for m, n in ((b"cmu440", 0), (b"cmu440", 123_456_789), (b"", U64), (b"r" * 119, 10 ** 19)):
        h = H(m, n)
        for kv in ({}, FAST):
            with env(**kv):
                assert check(gpu, m, n, n, h, 4) == ([(n, h)], (h, n), 1)            # lower == upper, a hit
                assert check(gpu, m, n, n, h, 1) == ([(n, h)], (h, n), 1)
                assert check(gpu, m, n, n, h - 1, 4) == ([], (h, n), 1)              # ... and a miss
    for m, lo, hi in ((b"cmu440", U64 - 30_000, U64), (b"q" * 60, U64 - 30_000, U64)):     # ends at 2^64 - 1
        T3 = kth_smallest_hash(m, lo, hi, 3)
        assert hits_ref(m, lo, hi, T3, 8)[0] == 3
        for kv in ({}, dict(FAST, MINEHIP_LOWER_DIGITS=1), dict(FAST, MINEHIP_LOWER_DIGITS=3)):
            with env(**kv):
                for k in (2, 3, 4):
                    check(gpu, m, lo, hi, T3, k, (kv, k))


def test_cli_and_binding(gpu):
    exe = os.path.join(PKG, "bin", "minehip-search")
    ref = hits_ref(*CMU, T10(6), 2)
    assert [n for n, _ in ref[1]] == CMU_K6[:2]
    mn = min((h, n) for n, h in ref[1])
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(T10(6)), "2", "first"], capture_output=True, text=True, timeout=120)
    want = "FirstHits 2 %d %d\n" % mn + "".join("%d %d\n" % (h, n) for n, h in ref[1])
    assert r.returncode == 0 and r.stdout == want, (r.stdout, r.stderr)
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(T10(6)), "0", "first"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout == "k is 1 to 1048576.\n", (r.stdout, r.stderr)
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(T10(6)), "1x", "first"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout == "1x is not a number.\n"
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(T10(6)), "2", "frist"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout.startswith("Usage: ")
    with pytest.raises(gpu.MinehipError) as e:
        gpu.search_first_hits(b"cmu440", 0, 1_000, T10(3), 0)
    assert e.value.code == gpu.MH_EINVAL
    assert gpu.search_first_hits("cmu440", 0, 1_999_999, T10(6), 2)[:2] == (ref[1], mn)     # a str message
