"""mh_search_first on the CPU: the reference the GPU tests use, the C-ABI's argument handling and
the binding.  No GPU compute is called here.

Reference: first_ref -- the oracle's hashes of every nonce of the range (test_gpu_ties.full_hashes),
in numpy: the first index with Hash <= target, or without one the range's (hash, nonce) minimum,
which is what mh_search returns."""
import ctypes
import hashlib

import numpy as np

import minehip
from minehip import _lib
from oracle import oracle
from conftest import run_dev
from test_gpu_ties import full_hashes

U64 = (1 << 64) - 1


def first_ref(msg, lo, hi, target):
    """(found, hash, nonce) of mh_search_first(msg, [lo, hi], target)."""
    h = full_hashes(msg, lo, hi)
    hits = np.flatnonzero(h <= np.uint64(target))
    i = int(hits[0]) if hits.size else int(h.argmin())      # argmin: the first occurrence of the minimum
    return bool(hits.size), int(h[i]), lo + i


def hits_of(msg, lo, hi, target):
    """The qualifying nonces of the range, in order."""
    return [lo + int(i) for i in np.flatnonzero(full_hashes(msg, lo, hi) <= np.uint64(target))]


def kth_smallest_hash(msg, lo, hi, k):
    """The k-th smallest hash of the range (k = 1: the minimum)."""
    return int(np.partition(full_hashes(msg, lo, hi), k - 1)[k - 1])


def test_first_ref_against_brute_force():
    for msg, lo in ((b"cmu440", 95), (b"x" * 60, 10 ** 19 - 150), (b"", U64 - 299), (b"r" * 119, 999_900)):
        hi = lo + 299
        hs = [int.from_bytes(hashlib.sha256(msg + b" " + str(n).encode()).digest()[:8], "big")
              for n in range(lo, hi + 1)]
        mn = min(hs)
        assert kth_smallest_hash(msg, lo, hi, 1) == mn and kth_smallest_hash(msg, lo, hi, 5) == sorted(hs)[4]
        for T in (0, mn - 1, mn, U64, sorted(hs)[4], sorted(hs)[150], hs[0], hs[0] - 1, hs[-1]):
            exp = None
            for n, h in zip(range(lo, hi + 1), hs):     # the proof-of-work loop: stop at the first hit
                if h <= T:
                    exp = (True, h, n)
                    break
            if exp is None:                              # the miner's loop: strict <, the first minimum
                best = None
                for n, h in zip(range(lo, hi + 1), hs):
                    if best is None or h < best[0]:
                        best = (h, n)
                exp = (False,) + best
            assert first_ref(msg, lo, hi, T) == exp, (msg[:8], lo, T)
            assert hits_of(msg, lo, hi, T) == [n for n, h in zip(range(lo, hi + 1), hs) if h <= T]
        assert first_ref(msg, lo, hi, U64) == (True, hs[0], lo)
        assert first_ref(msg, lo, hi, mn - 1) == (False,) + oracle.search(msg, lo, hi)
        assert first_ref(msg, lo, hi, mn)[0] and first_ref(msg, lo, hi, mn)[1:] == oracle.search(msg, lo, hi)


def test_issue_example_first_hit_is_not_the_minimum():
    """"cmu440" over [0, 1,999,999] with target 2^64 // 10^6: four hits, the first at 393,322, the
    minimum at 1,067,492 (hashlib, independent of the oracle)."""
    T = 2 ** 64 // 10 ** 6
    H = lambda n: int.from_bytes(hashlib.sha256(b"cmu440 " + str(n).encode()).digest()[:8], "big")  # noqa: E731
    assert H(393_322) <= T and H(1_067_492) == 1228377698034 <= T
    hits = hits_of(b"cmu440", 0, 1_999_999, T)
    assert len(hits) == 4 and hits[0] == 393_322 and 1_067_492 in hits
    assert first_ref(b"cmu440", 0, 1_999_999, T) == (True, H(393_322), 393_322)
    assert oracle.search(b"cmu440", 0, 1_999_999) == (1228377698034, 1_067_492)


def test_symbol_exported_and_bound():
    assert "mh_search_first" in _lib.EXPORTS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "mh_search_first")
    fn = minehip.lib.mh_search_first
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7
    assert fn.argtypes[5] is ctypes.c_uint64 and fn.argtypes[6]._type_ is _lib.mh_first
    assert [f for f, _ in _lib.mh_first._fields_] == ["found", "reserved", "hash", "nonce", "scanned"]
    assert ctypes.sizeof(_lib.mh_first) == 32
    assert callable(minehip.search_first)
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed


def test_argument_errors():
    out = _lib.mh_first()
    f = minehip.lib.mh_search_first
    assert f(0, b"x", 1, 5, 4, 7, ctypes.byref(out)) == minehip.MH_ERANGE
    assert b"lower > upper" in minehip.lib.mh_last_error()
    assert f(0, b"x", 1, 0, 4, 7, None) == minehip.MH_EINVAL
    assert b"NULL" in minehip.lib.mh_last_error()
    assert f(0, b"x", 1, 5, 4, 7, None) == minehip.MH_EINVAL         # out == NULL first, as mh_search
    assert f(0, None, 3, 0, 4, 7, ctypes.byref(out)) == minehip.MH_EINVAL
    big = b"y" * ((1 << 20) + 1)
    assert f(0, big, len(big), 0, 4, 7, ctypes.byref(out)) == minehip.MH_ETOOLONG
    try:
        minehip.search_first("x", 9, 3, 1)
        raise AssertionError("searched lower > upper")
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_ERANGE
    if minehip.device_count() == 0:               # no CPU fallback here either
        try:
            minehip.search_first("cmu440", 0, 10, U64)
            raise AssertionError("searched without a device")
        except minehip.MinehipError as e:
            assert e.code == minehip.MH_ENODEV


def test_dev_build_refuses_the_hash_and_code_object_hooks():
    """mh_search_first has no variants of the dev build's hash and code-object hooks: with one set
    it fails with MH_EINVAL before it touches a device, instead of silently ignoring it."""
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    try:
        minehip.search_first(b"cmu440", 0, 1000, 5)
        raise SystemExit("searched with " + k)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and k in str(e), e
    del os.environ[k]
print("refused")
""", timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:] + r.stdout[-500:]
