"""mh_search_hits on the GPU: every nonce whose hash is <= a target, bit-exact against
test_hits.hits_ref (the oracle's hashes of the whole range, in numpy) under every plan, for every
fast layout, with dense wave steps, at the range edges, truncated by `cap`, rebuilt after the
device buffer overflowed, through the Python binding and the command line.

Every case asserts from the reference alone that it is live -- how many nonces qualify and where
they lie -- before it looks at the GPU, then compares the count, the list and the minimum with the
reference, and the minimum with mh_search's."""
import os
import subprocess

import pytest

from conftest import PKG
from test_first import kth_smallest_hash
from test_gpu_first import plans
from test_gpu_parity import env
from test_hits import hits_ref

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CMU = (b"cmu440", 0, 1_999_999)
CMU_MIN = (1228377698034, 1_067_492)          # the range's minimum (tests/test_cli.py, tests/test_abi.py)
CMU_HITS = {6: 4, 5: 17, 4: 192, 3: 2_003, 2: 19_798}        # target 2^64 // 10^k: hits of the range
CMU_FIRST = {4: 19_411, 3: 1_081, 2: 111}
CMU_K6 = [393_322, 1_067_492, 1_456_236, 1_999_610]
FAST = dict(MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1)
CHUNK1 = 2560  # nonces of one workgroup's chunk at L = 1 (256 lanes x 10)


def T10(k):
    return 2 ** 64 // 10 ** k


def check(gpu, msg, lo, hi, T, cap, what=None):
    """One search against the reference; returns (count, list, minimum)."""
    exp = hits_ref(msg, lo, hi, T, cap)
    got = gpu.search_hits(msg, lo, hi, T, cap)
    assert got == exp, (what, msg[:8], len(msg), lo, hi, T, cap, got[0], got[1][:3], got[2], exp[0], exp[1][:3], exp[2])
    assert got[2] == gpu.search(msg, lo, hi), (what, got[2])
    assert all(a[0] < b[0] for a, b in zip(got[1], got[1][1:]))          # strictly increasing nonces
    return got


def test_cmu440_targets_under_every_plan(gpu):
    msg, lo, hi = CMU
    targets = {}
    for k, n in CMU_HITS.items():
        ref = hits_ref(msg, lo, hi, T10(k), 1 << 20)
        assert ref[0] == n == len(ref[1]) and ref[2] == CMU_MIN, k
        assert k not in CMU_FIRST or ref[1][0][0] == CMU_FIRST[k], k
        targets[T10(k)] = "k=%d" % k
    assert [n for n, _ in hits_ref(msg, lo, hi, T10(6), 16)[1]] == CMU_K6
    assert hits_ref(msg, lo, hi, CMU_MIN[0], 16) == (1, [(CMU_MIN[1], CMU_MIN[0])], CMU_MIN)
    assert hits_ref(msg, lo, hi, CMU_MIN[0] - 1, 16) == (0, [], CMU_MIN)       # no hit, the minimum all the same
    assert hits_ref(msg, lo, hi, 0, 16) == (0, [], CMU_MIN)
    targets.update({CMU_MIN[0]: "min", CMU_MIN[0] - 1: "min-1", 0: "zero"})
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        assert any(p["kind"] == 0 for p in gpu.plan(msg, lo, hi))       # those plans do run fast kernels
    results = {}
    for kv in plans():
        with env(**kv):
            for T, name in targets.items():
                got = check(gpu, msg, lo, hi, T, 1 << 15, (name, kv))
                results.setdefault(name, set()).add((got[0], tuple(got[1]), got[2]))
    assert all(len(v) == 1 for v in results.values())                   # identical throughout


def test_every_fast_layout(gpu):
    """Each of the 26 layouts over test_abi.kernel_cases()' range plus 3,456 nonces, at
    MINEHIP_LOWER_DIGITS in {1, 3} (each layout is planned at one of the two at least): exactly
    five hits spread over more than one chunk, and no hit."""
    from test_abi import KERNELS, KERNEL_CASE_NONCES, kernel_cases
    cases = kernel_cases()
    assert set(cases) == KERNELS
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
                for T in (T5, T1 - 1):
                    check(gpu, m, lo, hi, T, 16, (J, mode, Ld))
    assert planned == KERNELS, KERNELS - planned
    assert interleaved == {k for k in KERNELS if k[1] >= 3}, interleaved


def test_dense_wave_steps_and_edges(gpu):
    msg, lo, hi = b"cmu440", 95_000, 105_123
    ref = hits_ref(msg, lo, hi, U64, 16_384)
    assert ref[0] == 10_124 and [n for n, _ in ref[1]] == list(range(lo, hi + 1))   # every step of every lane hits
    for q in (0, 1):
        with env(**FAST, MINEHIP_LOWER_DIGITS=1, MINEHIP_QUEUE=q):
            pieces = gpu.plan(msg, lo, hi)
            assert any(p["kind"] == 0 for p in pieces) and any(p["kind"] == 1 for p in pieces)
            # partly filled waves and chunks: nothing of an invalid lane or outside the range appears
            assert any(p["kind"] == 0 and (p["count"] // 10) % 64 for p in pieces), pieces
            check(gpu, msg, lo, hi, U64, 16_384, q)
    H = lambda m, n: hits_ref(m, n, n, U64, 1)[1][0][1]    # noqa: E731  (the oracle's Hash(m, n))
    for m, n in ((b"cmu440", 0), (b"cmu440", 123_456_789), (b"", U64), (b"r" * 119, 10 ** 19)):
        h = H(m, n)
        for kv in ({}, FAST):
            with env(**kv):
                assert check(gpu, m, n, n, h, 4) == (1, [(n, h)], (h, n))            # lower == upper, a hit
                assert check(gpu, m, n, n, h - 1, 4) == (0, [], (h, n))              # ... and a miss
    for m, lo, hi in ((b"cmu440", U64 - 30_000, U64), (b"q" * 60, U64 - 30_000, U64)):     # ends at 2^64 - 1
        T3 = kth_smallest_hash(m, lo, hi, 3)
        assert hits_ref(m, lo, hi, T3, 8)[0] == 3
        for kv in ({}, dict(FAST, MINEHIP_LOWER_DIGITS=1), dict(FAST, MINEHIP_LOWER_DIGITS=3)):
            with env(**kv):
                check(gpu, m, lo, hi, T3, 8, kv)
                assert check(gpu, m, lo, hi, U64, 1 << 15, kv)[0] == 30_001


def test_truncation(gpu):
    msg, lo, hi = CMU
    full = hits_ref(msg, lo, hi, T10(3), 1 << 20)
    assert full[0] == 2_003 == len(full[1])
    for kv in ({}, dict(FAST, MINEHIP_LOWER_DIGITS=3)):
        with env(**kv):
            assert check(gpu, msg, lo, hi, T10(3), 0, kv) == (2_003, [], CMU_MIN)       # count only
            for cap in (1, 100):
                got = check(gpu, msg, lo, hi, T10(3), cap, kv)
                assert got[0] == 2_003 and got[1] == full[1][:cap]


def test_overflow_walk(gpu):
    msg, lo, hi = CMU
    full = hits_ref(msg, lo, hi, T10(3), 1 << 20)
    assert full[0] == 2_003 and full[1][99][0] == 122_839
    for kv in ({}, dict(FAST, MINEHIP_LOWER_DIGITS=3), dict(FAST, MINEHIP_LOWER_DIGITS=1, MINEHIP_QUEUE=0)):
        with env(**kv):
            for cap in (100, 64):
                default = check(gpu, msg, lo, hi, T10(3), cap, kv)
                with env(MINEHIP_HITS_SLOTS=64):
                    got = check(gpu, msg, lo, hi, T10(3), cap, kv)
                assert got == default and got[0] == 2_003 and len(got[1]) == cap, (kv, cap)
            assert got[1] == full[1][:64]
            with env(MINEHIP_HITS_SLOTS=64):
                assert check(gpu, msg, lo, hi, T10(3), 0, kv) == (2_003, [], CMU_MIN)   # count only: no walk needed
            assert [n for n, _ in hits_ref(msg, 0, 3_000, T10(3), 3)[1]] == [1_081, 1_329, 2_080]
            default = check(gpu, msg, 0, 3_000, T10(3), 3, kv)
            with env(MINEHIP_HITS_SLOTS=1):
                assert check(gpu, msg, 0, 3_000, T10(3), 3, kv) == default


def test_cli_and_binding(gpu):
    exe = os.path.join(PKG, "bin", "minehip-search")
    ref = hits_ref(*CMU, T10(6), 16)
    assert [n for n, _ in ref[1]] == CMU_K6
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(T10(6)), "16"], capture_output=True, text=True, timeout=120)
    want = "Hits 4 %d %d\n" % CMU_MIN + "".join("%d %d\n" % (h, n) for n, h in ref[1])
    assert r.returncode == 0 and r.stdout == want, (r.stdout, r.stderr)
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(T10(6)), "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "".join(want.splitlines(True)[:3]), (r.stdout, r.stderr)
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(T10(6)), "1x"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout == "1x is not a number.\n"
    with pytest.raises(gpu.MinehipError) as e:
        gpu.search_hits(b"cmu440", 0, 1_000, T10(3), gpu.MH_HITS_MAX_CAP + 1)
    assert e.value.code == gpu.MH_EINVAL
    assert gpu.search_hits("cmu440", 0, 1_999_999, T10(6)) == (4, ref[1], CMU_MIN)      # str message, default cap
