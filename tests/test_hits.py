"""mh_search_hits on the CPU: the reference the GPU tests use, the C-ABI's argument handling and
the binding.  No GPU compute is called here.

Reference: hits_ref -- the oracle's hashes of every nonce of the range (test_gpu_ties.full_hashes),
in numpy: how many are <= target, the first `cap` of them in nonce order with their hashes, and
the range's (hash, nonce) minimum, which is what mh_search returns."""
import ctypes
import hashlib

import numpy as np

import minehip
from minehip import _lib
from conftest import run_dev
from test_gpu_ties import full_hashes

U64 = (1 << 64) - 1


def hits_ref(msg, lo, hi, target, cap):
    """(count, [(nonce, hash), ...], (min_hash, min_nonce)) of mh_search_hits(msg, [lo, hi], target, cap)."""
    h = full_hashes(msg, lo, hi)
    idx = np.flatnonzero(h <= np.uint64(target))
    i = int(h.argmin())                                      # argmin: the first occurrence of the minimum
    return int(idx.size), [(lo + int(j), int(h[j])) for j in idx[:cap]], (int(h[i]), lo + i)


def test_hits_ref_against_brute_force():
    for msg, lo in ((b"cmu440", 95), (b"x" * 60, 10 ** 19 - 1_500), (b"", U64 - 2_999), (b"r" * 119, 999_000)):
        hi = lo + 2_999
        hs = [int.from_bytes(hashlib.sha256(msg + b" " + str(n).encode()).digest()[:8], "big")
              for n in range(lo, hi + 1)]
        order = sorted(hs)
        best = None
        for n, h in zip(range(lo, hi + 1), hs):              # the miner's loop: strict <, the first minimum
            if best is None or h < best[0]:
                best = (h, n)
        for T in (0, order[0] - 1, order[0], order[4], order[1_500], U64, hs[0], hs[-1]):
            every = [(n, h) for n, h in zip(range(lo, hi + 1), hs) if h <= T]
            for cap in (0, 1, 3, 3_000, 4_096):
                assert hits_ref(msg, lo, hi, T, cap) == (len(every), every[:cap], best), (msg[:8], lo, T, cap)
        assert hits_ref(msg, lo, hi, U64, 3_000)[0] == 3_000
        assert hits_ref(msg, lo, hi, order[4], 10)[0] == 5


def test_symbol_exported_and_bound():
    assert "mh_search_hits" in _lib.EXPORTS
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "mh_search_hits")
    fn = minehip.lib.mh_search_hits
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[5] is ctypes.c_uint64 and fn.argtypes[6]._type_ is _lib.mh_hit
    assert fn.argtypes[7] is ctypes.c_size_t and fn.argtypes[8]._type_ is _lib.mh_hits
    assert [f for f, _ in _lib.mh_hit._fields_] == ["hash", "nonce"]
    assert [f for f, _ in _lib.mh_hits._fields_] == ["count", "stored", "hash", "nonce"]
    assert ctypes.sizeof(_lib.mh_hit) == 16 and ctypes.sizeof(_lib.mh_hits) == 32
    assert minehip.MH_HITS_MAX_CAP == 1 << 20
    assert callable(minehip.search_hits)
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed


def test_argument_errors():
    out = _lib.mh_hits()
    buf = (_lib.mh_hit * 4)()
    f = minehip.lib.mh_search_hits
    err = minehip.lib.mh_last_error
    assert f(0, b"x", 1, 5, 4, 7, buf, 4, ctypes.byref(out)) == minehip.MH_ERANGE
    assert b"lower > upper" in err()
    assert f(0, b"x", 1, 5, 4, 7, None, 0, ctypes.byref(out)) == minehip.MH_ERANGE     # the count-only form too
    assert f(0, b"x", 1, 0, 4, 7, buf, 4, None) == minehip.MH_EINVAL
    assert b"NULL" in err()
    assert f(0, b"x", 1, 5, 4, 7, buf, 4, None) == minehip.MH_EINVAL                   # out == NULL first, as mh_search
    assert f(0, b"x", 1, 0, 4, 7, None, 4, ctypes.byref(out)) == minehip.MH_EINVAL     # hits == NULL with cap > 0
    assert b"hits is NULL" in err()
    assert f(0, b"x", 1, 0, 4, 7, buf, (1 << 20) + 1, ctypes.byref(out)) == minehip.MH_EINVAL
    assert b"MH_HITS_MAX_CAP" in err()
    assert f(0, b"x", 1, 5, 4, 7, buf, (1 << 20) + 1, ctypes.byref(out)) == minehip.MH_EINVAL   # before the range
    assert f(0, None, 3, 0, 4, 7, buf, 4, ctypes.byref(out)) == minehip.MH_EINVAL
    big = b"y" * ((1 << 20) + 1)
    assert f(0, big, len(big), 0, 4, 7, buf, 4, ctypes.byref(out)) == minehip.MH_ETOOLONG
    for args in (("x", 9, 3, 1), ("x", 0, 3, 1, (1 << 20) + 1), ("x", 0, 3, 1, -1)):
        try:
            minehip.search_hits(*args)
            raise AssertionError("searched %r" % (args,))
        except minehip.MinehipError as e:
            assert e.code == (minehip.MH_ERANGE if args[1] > args[2] else minehip.MH_EINVAL)
    if minehip.device_count() == 0:               # no CPU fallback here either
        for cap in (0, 16):
            try:
                minehip.search_hits("cmu440", 0, 10, U64, cap)
                raise AssertionError("searched without a device")
            except minehip.MinehipError as e:
                assert e.code == minehip.MH_ENODEV


def test_dev_build_refuses_the_hash_and_code_object_hooks():
    """mh_search_hits has no variants of the dev build's hash and code-object hooks: with one set
    it fails with MH_EINVAL before it touches a device, instead of silently ignoring it."""
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    try:
        minehip.search_hits(b"cmu440", 0, 1000, 5)
        raise SystemExit("searched with " + k)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and k in str(e), e
    del os.environ[k]
print("refused")
""", timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:] + r.stdout[-500:]
