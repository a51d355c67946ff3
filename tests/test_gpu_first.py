"""mh_search_first on the GPU: the smallest nonce whose hash is <= a target, bit-exact against
test_first.first_ref (the oracle's hashes of the whole range, in numpy) under every plan, for every
fast layout, at the range edges, through the Python binding and the command line.

Every case asserts from the reference alone that it is live -- how many nonces qualify, where they
lie, that the first of them is not the range's minimum where that matters -- before it looks at the
GPU.  `scanned` (counted on the device) is checked in every case: the whole range when nothing
qualifies, never less than nonce - lower + 1 when something does."""
import os
import subprocess

import pytest

from conftest import PKG
from test_first import first_ref, hits_of, kth_smallest_hash
from test_gpu_parity import env

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CMU = (b"cmu440", 0, 1_999_999)
CMU_MIN = (1228377698034, 1_067_492)          # the range's minimum (tests/test_cli.py, tests/test_abi.py)
CMU_FIRST = {2: 111, 3: 1_081, 4: 19_411, 5: 114_702, 6: 393_322}    # target 2^64 // 10^k: first hit
FAST = dict(MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1)
CHUNK1 = 2560  # nonces of one workgroup's chunk at L = 1 (256 lanes x 10)


def check(gpu, msg, lo, hi, T, what=None):
    """One search against the reference, scanned included; returns (found, hash, nonce, scanned)."""
    exp = first_ref(msg, lo, hi, T)
    got = gpu.search_first(msg, lo, hi, T)
    assert got[:3] == exp, (what, msg[:8], len(msg), lo, hi, T, got, exp)
    if exp[0]:
        assert got[2] - lo + 1 <= got[3] <= hi - lo + 1, (what, got)
    else:
        assert got[3] == hi - lo + 1, (what, got)
        assert got[1:3] == gpu.search(msg, lo, hi), (what, got)
    return got


def plans():
    """The default plan, and the fast kernels with L in {1, 3}, work queue or static, one or two streams."""
    return [{}] + [dict(FAST, MINEHIP_LOWER_DIGITS=L, MINEHIP_QUEUE=q, MINEHIP_STREAMS=s)
                   for L in (1, 3) for q in (0, 1) for s in (1, 2)]


def test_cmu440_first_hits_under_every_plan(gpu):
    msg, lo, hi = CMU
    targets = {}
    for k, n in CMU_FIRST.items():
        T = 2 ** 64 // 10 ** k
        assert first_ref(msg, lo, hi, T)[0] and first_ref(msg, lo, hi, T)[2] == n, k
        targets[T] = "k=%d" % k
    T6 = 2 ** 64 // 10 ** 6
    hits = hits_of(msg, lo, hi, T6)
    assert len(hits) == 4 and hits[0] == 393_322 != CMU_MIN[1] and CMU_MIN[1] in hits   # first hit != argmin
    assert first_ref(msg, lo, hi, CMU_MIN[0]) == (True,) + CMU_MIN and hits_of(msg, lo, hi, CMU_MIN[0]) == [CMU_MIN[1]]
    assert first_ref(msg, lo, hi, CMU_MIN[0] - 1) == (False,) + CMU_MIN
    assert first_ref(msg, lo, hi, U64)[2] == lo and first_ref(msg, lo, hi, 0) == (False,) + CMU_MIN
    targets.update({CMU_MIN[0]: "min", CMU_MIN[0] - 1: "min-1", U64: "all", 0: "zero"})
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        assert any(p["kind"] == 0 for p in gpu.plan(msg, lo, hi))       # those plans do run fast kernels
    results = {}
    for kv in plans():
        with env(**kv):
            for T, name in targets.items():
                got = check(gpu, msg, lo, hi, T, (name, kv))
                results.setdefault(name, set()).add(got[:3])
    assert all(len(v) == 1 for v in results.values()), results           # identical throughout


def test_every_fast_layout(gpu):
    """Each of the 26 layouts over test_abi.kernel_cases()' range (as tests/test_gpu_ties.py: 253,457
    nonces), at MINEHIP_LOWER_DIGITS in {1, 3} (a layout that cannot enumerate three digits runs its
    largest L there, or leaves the range to a neighbouring layout: each is planned at one of the
    two at least): exactly five hits spread over more than one chunk, the minimum alone, and no hit."""
    from test_abi import KERNELS, KERNEL_CASE_NONCES, kernel_cases
    cases = kernel_cases()
    assert set(cases) == KERNELS
    interleaved, planned = set(), set()
    for (J, mode), (m, lo, _, early) in sorted(cases.items()):
        hi = lo + KERNEL_CASE_NONCES + 3_456
        T5, T1 = kth_smallest_hash(m, lo, hi, 5), kth_smallest_hash(m, lo, hi, 1)
        hits = hits_of(m, lo, hi, T5)
        assert len(hits) == 5 and hits[-1] - hits[0] > CHUNK1, (J, mode, hits)
        assert len(hits_of(m, lo, hi, T1)) == 1 and not hits_of(m, lo, hi, T1 - 1)
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
                for T in (T5, T1, T1 - 1):
                    check(gpu, m, lo, hi, T, (J, mode, Ld))
    assert planned == KERNELS, KERNELS - planned
    assert interleaved == {k for k in KERNELS if k[1] >= 3}, interleaved


def test_early_exit_is_deterministic_on_one_stream(gpu):
    msg, lo, hi = CMU
    with env(MINEHIP_STREAMS=1, MINEHIP_LAUNCH_NONCES=100_000, MINEHIP_GENERIC_BELOW=0):
        pieces = gpu.plan(msg, lo, hi)
        assert len(pieces) > 10 and pieces[0]["first"] == 0
        # every nonce qualifies: the first piece records nonce 0, and every later launch -- queued
        # behind it on the one stream -- skips all of its work
        got = check(gpu, msg, lo, hi, U64)
        assert got[2] == 0 and got[3] <= pieces[0]["count"], (got, pieces[0])
        # four hits from 393,322 on: everything up to the first is hashed, and not everything
        got = check(gpu, msg, lo, hi, 2 ** 64 // 10 ** 6)
        assert got[2] == 393_322 and 393_323 <= got[3] < hi - lo + 1, got


def test_edges(gpu):
    H = lambda m, n: first_ref(m, n, n, U64)[1]    # noqa: E731  (the oracle's Hash(m, n))
    for m, n in ((b"cmu440", 0), (b"cmu440", 123_456_789), (b"", U64), (b"r" * 119, 10 ** 19)):
        h = H(m, n)
        for kv in ({}, FAST):
            with env(**kv):
                assert check(gpu, m, n, n, h) == (True, h, n, 1)            # lower == upper, a hit
                assert check(gpu, m, n, n, h - 1) == (False, h, n, 1)       # ... and a miss
    ranges = [(b"cmu440", U64 - 30_000, U64),                       # ends at 2^64 - 1
              (b"q" * 60, U64 - 30_000, U64),
              (b"cmu440", 10 ** 5 - 7_000, 10 ** 5 + 9_000),        # straddles 10^5
              (b"cmu440", 10 ** 19 - 7_000, 10 ** 19 + 9_000),      # ... and 10^19
              (b"r" * 119, 3, 40_000),                              # 119 bytes: two tail blocks
              (b"r" * 119, 10 ** 9 - 20_000, 10 ** 9 + 20_000)]
    for m, lo, hi in ranges:
        T3, T1 = kth_smallest_hash(m, lo, hi, 3), kth_smallest_hash(m, lo, hi, 1)
        assert len(hits_of(m, lo, hi, T3)) == 3
        for kv in ({}, dict(FAST, MINEHIP_LOWER_DIGITS=1), dict(FAST, MINEHIP_LOWER_DIGITS=3)):
            with env(**kv):
                for T in (T3, T1, T1 - 1, U64):
                    check(gpu, m, lo, hi, T, kv)


def test_hit_in_a_generic_edge_before_and_after_the_fast_pieces(gpu):
    msg = b"cmu440"
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        # leading edge: the first hit lies in the generic piece before the first fast piece
        lo, hi = 10 ** 6 + 337, 10 ** 6 + 250_450
        pieces = gpu.plan(msg, lo, hi)
        assert [p["kind"] for p in pieces][:2] == [1, 0] and pieces[-1]["kind"] == 1, pieces
        lead = pieces[0]
        T = kth_smallest_hash(msg, lead["first"], lead["first"] + lead["count"] - 1, 1)
        exp = first_ref(msg, lo, hi, T)
        assert exp[0] and lead["first"] <= exp[2] < lead["first"] + lead["count"]
        assert len(hits_of(msg, lo, hi, T)) > 1            # later pieces hold hits too: the first one wins
        check(gpu, msg, lo, hi, T)
        # trailing edge: the only hit is the range's minimum, in the generic piece after the last fast one
        lo, hi = 10 ** 6, CMU_MIN[1] + 7
        pieces = gpu.plan(msg, lo, hi)
        assert pieces[-1]["kind"] == 1 and pieces[-2]["kind"] == 0 and pieces[-1]["first"] <= CMU_MIN[1], pieces
        assert hits_of(msg, lo, hi, CMU_MIN[0]) == [CMU_MIN[1]]
        assert check(gpu, msg, lo, hi, CMU_MIN[0])[:3] == (True,) + CMU_MIN


def test_cli_prints_first_and_none(gpu):
    exe = os.path.join(PKG, "bin", "minehip-search")
    h, n = first_ref(*CMU, 2 ** 64 // 10 ** 6)[1:]
    assert n == 393_322
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(2 ** 64 // 10 ** 6)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "First %d %d\n" % (h, n), (r.stdout, r.stderr)
    r = subprocess.run([exe, "cmu440", "1999999", "0", str(CMU_MIN[0] - 1)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "None %d %d\n" % CMU_MIN, (r.stdout, r.stderr)
    r = subprocess.run([exe, "cmu440", "1999999", "0", "12x"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout == "12x is not a number.\n"
