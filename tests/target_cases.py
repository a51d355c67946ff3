"""Brute-force expectations for the target-job tests (test_target_*.py, test_gpu_target.py): the
proof-of-work answer of a range, from oracle.hash_batch -- the first nonce whose hash is <= target
and its hash, otherwise oracle.search's minimum -- and the fixture ranges those tests share.

The hashes of a range are computed once per (msg, lower, upper) and kept; an answer for a sub-range
of a kept range (a simulated miner's chunk) is read from them."""
import numpy as np

from oracle import oracle

U64 = (1 << 64) - 1
T3, T6, T9 = (1 << 64) // 10 ** 3, (1 << 64) // 10 ** 6, (1 << 64) // 10 ** 9

# (msg, lower, upper, target) and, checked with hashlib when they were chosen, what each must give
FIXTURES = [
    (b"cmu440", 0, 1_999_999, T6),   # hits at 393,322; 1,067,492; 1,456,236; 1,999,610
    (b"cmu440", 0, 1_999_999, T9),   # no hit: the minimum
    (b"cmu440", 0, 299_999, T3),     # 285 hits, the first at 1,081
]
FIXTURE_ANSWERS = [(14415379299797, 393_322), (1228377698034, 1_067_492), (8602862364711503, 1_081)]
FIXTURE_MINIMA = [(1228377698034, 1_067_492), (1228377698034, 1_067_492), (50287055093129, 138_932)]
# further ranges of the cluster tests: digits change inside, and the top of uint64
EXTRA = [
    (b"x" * 60, 10 ** 9 - 5_000, 10 ** 9 + 300_000, T3),
    (b"a" * 100, U64 - 200_000, U64, T3),
]

_hashes = {}


def hashes(msg, lower, upper):
    """Hash(msg, n) for n in [lower, upper] as a uint64 array, from the kept range that holds it."""
    msg = bytes(msg)
    for (m, lo, hi), h in _hashes.items():
        if m == msg and lo <= lower and upper <= hi:
            return h[lower - lo:upper - lo + 1]
    n = upper - lower + 1
    h = oracle.hash_batch(msg, np.uint64(lower) + np.arange(n, dtype=np.uint64))
    h.setflags(write=False)
    _hashes[(msg, lower, upper)] = h
    return h


def first_hit(msg, lower, upper, target):
    """(hash, nonce) of the smallest nonce of [lower, upper] with hash <= target, or None."""
    h = hashes(msg, lower, upper)
    idx = np.flatnonzero(h <= np.uint64(target))
    return (int(h[idx[0]]), lower + int(idx[0])) if idx.size else None


def brute_first(msg, lower, upper, target):
    """(hash, nonce): the first hit, otherwise oracle.search's minimum of the range."""
    return first_hit(msg, lower, upper, target) or oracle.search(msg, lower, upper, threads=4)


def chunk_answer(msg, lower, upper, target=None):
    """What a miner answers for the chunk [lower, upper] of a kept range: with a target the chunk's
    first hit, else (and when nothing qualifies) its lexicographic minimum."""
    if target is not None:
        f = first_hit(msg, lower, upper, target)
        if f:
            return f
    h = hashes(msg, lower, upper)
    i = int(np.argmin(h))  # the first occurrence: the smallest nonce among equal hashes
    return int(h[i]), lower + i
