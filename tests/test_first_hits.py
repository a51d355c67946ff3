"""mh_search_first_hits on the CPU: the symbols and the binding, the C-ABI's argument handling, the
dev build's refusal of the hooks, and the invariant of the bound the kernels stop by, fuzzed through
the host-only exports mh_first_hits_slices and mh_first_hits_bound (layout.hpp's inline functions,
the ones the kernels publish with).  No GPU compute is called here.

The invariant: whenever the bound word holds B < 2^64-1, at least k qualifying nonces of the range
are <= B.  The word is lowered to mh_first_hits_bound of slice counters that may lag behind the
hits found so far, so the fuzz builds the counters from an arbitrary subset of a random hit set."""
import ctypes
import random

import minehip
from minehip import _lib
from conftest import run_dev

U64 = (1 << 64) - 1


def slices_of(lo, hi):
    shift, n = ctypes.c_uint32(), ctypes.c_uint32()
    assert minehip.lib.mh_first_hits_slices(lo, hi, ctypes.byref(shift), ctypes.byref(n)) == minehip.MH_OK
    return shift.value, n.value


def bound_of(lo, hi, k, counts):
    return minehip.lib.mh_first_hits_bound(lo, hi, k, (ctypes.c_uint32 * len(counts))(*counts))


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mh_search_first_hits", "mh_first_hits_slices", "mh_first_hits_bound"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    fn = minehip.lib.mh_search_first_hits
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[5] is ctypes.c_uint64 and fn.argtypes[6]._type_ is _lib.mh_hit
    assert fn.argtypes[7] is ctypes.c_size_t and fn.argtypes[8]._type_ is _lib.mh_first_hits
    assert [f for f, _ in _lib.mh_first_hits._fields_] == ["stored", "scanned", "hash", "nonce"]
    assert ctypes.sizeof(_lib.mh_first_hits) == 32 and ctypes.sizeof(_lib.mh_hit) == 16
    assert minehip.lib.mh_first_hits_slices.restype is ctypes.c_int
    assert minehip.lib.mh_first_hits_bound.restype is ctypes.c_uint64
    assert callable(minehip.search_first_hits) and minehip.mh_first_hits is _lib.mh_first_hits
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed
    from minehip import codeobj
    assert codeobj.hits_stop_code_object()[:4] == b"\x7fELF"


def test_argument_errors_come_before_the_device():
    out = _lib.mh_first_hits()
    buf = (_lib.mh_hit * 4)()
    f = minehip.lib.mh_search_first_hits
    err = minehip.lib.mh_last_error
    assert f(0, b"x", 1, 0, 4, 7, buf, 4, None) == minehip.MH_EINVAL
    assert b"NULL" in err()
    assert f(0, b"x", 1, 5, 4, 7, buf, 4, None) == minehip.MH_EINVAL                    # out == NULL first
    assert f(0, b"x", 1, 0, 4, 7, None, 4, ctypes.byref(out)) == minehip.MH_EINVAL
    assert b"hits is NULL" in err()
    assert f(0, b"x", 1, 0, 4, 7, buf, 0, ctypes.byref(out)) == minehip.MH_EINVAL
    assert b"k is 0" in err()
    assert f(0, b"x", 1, 0, 4, 7, buf, (1 << 20) + 1, ctypes.byref(out)) == minehip.MH_EINVAL
    assert b"MH_HITS_MAX_CAP" in err()
    assert f(0, b"x", 1, 5, 4, 7, buf, (1 << 20) + 1, ctypes.byref(out)) == minehip.MH_EINVAL   # before the range
    assert f(0, b"x", 1, 5, 4, 7, buf, 4, ctypes.byref(out)) == minehip.MH_ERANGE
    assert b"lower > upper" in err()
    assert f(0, None, 3, 0, 4, 7, buf, 4, ctypes.byref(out)) == minehip.MH_EINVAL
    assert b"msg is NULL" in err()
    big = b"y" * ((1 << 20) + 1)
    assert f(0, big, len(big), 0, 4, 7, buf, 4, ctypes.byref(out)) == minehip.MH_ETOOLONG
    for args in (("x", 9, 3, 1, 2), ("x", 0, 3, 1, 0), ("x", 0, 3, 1, (1 << 20) + 1), ("x", 0, 3, 1, -1)):
        try:
            minehip.search_first_hits(*args)
            raise AssertionError("searched %r" % (args,))
        except minehip.MinehipError as e:
            assert e.code == (minehip.MH_ERANGE if args[1] > args[2] else minehip.MH_EINVAL)
    if minehip.device_count() == 0:               # every error above was returned without a device
        try:
            minehip.search_first_hits("cmu440", 0, 10, U64, 3)
            raise AssertionError("searched without a device")
        except minehip.MinehipError as e:
            assert e.code == minehip.MH_ENODEV
    # the host-only exports
    s, n = ctypes.c_uint32(), ctypes.c_uint32()
    g = minehip.lib.mh_first_hits_slices
    assert g(5, 4, ctypes.byref(s), ctypes.byref(n)) == minehip.MH_ERANGE
    assert g(0, 4, None, ctypes.byref(n)) == minehip.MH_EINVAL and g(0, 4, ctypes.byref(s), None) == minehip.MH_EINVAL
    assert minehip.lib.mh_first_hits_bound(0, 4, 1, None) == U64
    assert bound_of(0, 4, 0, [1] * 5) == U64 and bound_of(5, 4, 1, [1] * 5) == U64


def test_dev_build_refuses_the_hash_and_code_object_hooks():
    """As mh_search_hits: hits_stop has no variants of the dev build's hash and code-object hooks, so
    with one set the call fails with MH_EINVAL before it touches a device."""
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    try:
        minehip.search_first_hits(b"cmu440", 0, 1000, 5, 2)
        raise SystemExit("searched with " + k)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and k in str(e) and "mh_search_first_hits" in str(e), e
    del os.environ[k]
print("refused")
""", timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:] + r.stdout[-500:]


def test_slicing():
    """shift is the smallest value with 1024 << shift >= size; the slices cover the range exactly."""
    for lo, hi in ((0, 0), (7, 7), (0, 1022), (0, 1023), (0, 1024), (5, 1028), (5, 1029), (0, (1 << 20) - 2),
                   (0, (1 << 20) - 1), (0, 1 << 20), (1_000_000, 1_999_999), (0, (1 << 32) - 1), (0, U64),
                   (U64, U64), (U64 - 30_000, U64), (1, U64), (1 << 63, U64)):
        size = hi - lo + 1
        shift, n = slices_of(lo, hi)
        assert (1024 << shift) >= size and (shift == 0 or (1024 << (shift - 1)) < size), (lo, hi, shift)
        assert 1 <= n <= 1024 and n == ((hi - lo) >> shift) + 1, (lo, hi, shift, n)
        # the bound of one hit in slice s, k = 1: the slice's last nonce, cut to the range's
        for s in {0, n // 2, n - 1}:
            counts = [0] * n
            counts[s] = 1
            want = min(hi, lo + ((s + 1) << shift) - 1)
            assert bound_of(lo, hi, 1, counts) == want and lo + (s << shift) <= want, (lo, hi, s)
            assert bound_of(lo, hi, 2, counts) == U64
    assert slices_of(1_000_000, 1_999_999) == (10, 977) and slices_of(0, (1 << 32) - 1) == (22, 1024)
    assert slices_of(0, U64) == (54, 1024) and bound_of(0, U64, 1, [0] * 1023 + [1]) == U64     # no 2^64 overflow


def random_range(rng):
    size = rng.choice([1, 2, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, rng.randrange(1, 5000),
                       rng.randrange(1, 1 << 24), rng.randrange(1, 1 << 40), rng.randrange(1, 1 << 64)])
    if rng.random() < 0.3:
        hi = U64                                      # ranges that end at 2^64 - 1
        lo = hi - size + 1
    else:
        lo = rng.randrange(0, U64 - size + 2)
        hi = lo + size - 1
    return lo, hi


def test_invariant_fuzz():
    rng = random.Random(440)
    lowered = loose = 0
    for _ in range(600):
        lo, hi = random_range(rng)
        size = hi - lo + 1
        shift, n = slices_of(lo, hi)
        nh = min(size, rng.choice([0, 1, 2, 5, 40, 300]))
        if rng.random() < 0.5:                        # clustered low, as the hits of a range scanned upward are
            span = max(1, min(size, (size >> rng.randrange(0, 12)) or 1))
            hits = sorted({lo + rng.randrange(0, span) for _ in range(nh)})
        else:
            hits = sorted({lo + rng.randrange(0, size) for _ in range(nh)})
        for k in {1, 2, max(1, len(hits) - 1), max(1, len(hits)), len(hits) + 1, rng.randrange(1, 400)}:
            order = hits[:]
            rng.shuffle(order)                        # an arbitrary subset of the true hits, grown one by one
            counts = [0] * n
            prev = U64
            assert bound_of(lo, hi, k, counts) == U64
            for j, x in enumerate(order):
                counts[(x - lo) >> shift] += 1
                b = bound_of(lo, hi, k, counts)
                assert (b == U64) == (j + 1 < k) or (b == hi == U64 and j + 1 >= k), (lo, hi, k, j, b)
                if j + 1 >= k:
                    assert b <= hi and sum(1 for y in hits if y <= b) >= k, (lo, hi, k, j, b)
                    lowered += 1
                assert b <= prev, (lo, hi, k, j, b, prev)         # growing the subset never raises it
                prev = b
            if len(hits) >= k:                        # all counted: the bound lies in the k-th smallest hit's slice
                kth = hits[k - 1]
                assert (prev - lo) >> shift == (kth - lo) >> shift and prev >= kth, (lo, hi, k, prev, kth)
                loose += prev > kth
    assert lowered > 2000 and loose > 100             # the fuzz did lower bounds, mostly to a slice end past the hit
