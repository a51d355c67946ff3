"""mh_search_first_hits_batch / mh_first_hits_batch_regions on the CPU: the ABI surface, the
argument handling up to the device call, the binding, and the host-built schedule of the fused
passes.  No GPU compute is called here.

The schedule (include/minehip.h): fused or fallback and the passes are
mh_batch_plan_ex(flags)'s; in request order a fused request of k wants min(its nonce count,
max(4 k, 256)) entries of the device hit buffer and gets min(that, what the window has left) at the
next free offset, and a pass whose requests want more than the window has left starts a new window."""
import ctypes
import re

import pytest

import minehip
from minehip import _lib
from conftest import ROOT, run_dev
from test_gpu_parity import env

U64 = (1 << 64) - 1
MAXCAP = 1 << 20


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mh_search_first_hits_batch", "mh_first_hits_batch_regions", "mh_batch_bound_co_begin",
                 "mh_batch_bound_co_end"):
        assert hasattr(raw, name), name
    assert "mh_search_first_hits_batch" in _lib.EXPORTS and "mh_first_hits_batch_regions" in _lib.EXPORTS
    fn = minehip.lib.mh_search_first_hits_batch
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7
    assert fn.argtypes[0] is ctypes.c_int and fn.argtypes[1]._type_ is _lib.mh_first_hits_request
    assert fn.argtypes[2] is ctypes.c_size_t and fn.argtypes[3] is ctypes.c_uint32 and fn.argtypes[4]._type_ is _lib.mh_hit
    assert fn.argtypes[5] is ctypes.c_size_t and fn.argtypes[6]._type_ is _lib.mh_first_hits_result
    fr = minehip.lib.mh_first_hits_batch_regions
    assert fr.restype is ctypes.c_int64 and len(fr.argtypes) == 5
    assert fr.argtypes[0]._type_ is _lib.mh_first_hits_request and fr.argtypes[2] is ctypes.c_uint32
    assert fr.argtypes[3]._type_ is _lib.mh_hits_region and fr.argtypes[4] is ctypes.c_int64
    assert [f for f, _ in _lib.mh_first_hits_request._fields_] == ["msg", "len", "lower", "upper", "target", "k"]
    assert [f for f, _ in _lib.mh_first_hits_result._fields_] == ["status", "path", "stored", "scanned", "hash", "nonce",
                                                                  "offset"]
    assert ctypes.sizeof(_lib.mh_first_hits_request) == 48 and ctypes.sizeof(_lib.mh_first_hits_result) == 48
    assert callable(minehip.search_first_hits_batch) and callable(minehip.first_hits_batch_regions)
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed


def test_header_declares_what_the_binding_binds():
    h = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/minehip.h").read(), flags=re.S)
    h = re.sub(r"\s+", " ", h)
    assert ("typedef struct mh_first_hits_request { const uint8_t *msg; size_t len; uint64_t lower, upper, target; "
            "uint64_t k; } mh_first_hits_request;") in h
    assert ("typedef struct mh_first_hits_result { int32_t status; int32_t path; uint64_t stored, scanned, hash, nonce; "
            "uint64_t offset; } mh_first_hits_result;") in h
    assert ("int mh_search_first_hits_batch(int dev, const mh_first_hits_request *reqs, size_t n, uint32_t flags, "
            "mh_hit *hits, size_t hits_cap, mh_first_hits_result *out);") in h
    assert ("int64_t mh_first_hits_batch_regions(const mh_first_hits_request *reqs, size_t n, uint32_t flags, "
            "mh_hits_region *out, int64_t cap);") in h
    assert "#define MH_ABI_VERSION 5" in open(ROOT + "/include/minehip.h").read()
    assert "no batched form" not in open(ROOT + "/include/minehip.h").read()


def _reqs(*rows):
    arr = (_lib.mh_first_hits_request * len(rows))()
    keep = []
    for i, (m, lo, hi, T, k) in enumerate(rows):
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper = m, (len(m) if m is not None else 3), lo, hi
        arr[i].target, arr[i].k = T, k
    return arr, keep


def test_arguments_without_a_device():
    L = minehip.lib
    for flags in (0, 1):
        assert L.mh_search_first_hits_batch(0, None, 0, flags, None, 0, None) == minehip.MH_OK   # n = 0: no device touched
        assert minehip.search_first_hits_batch([], fuse_fast=bool(flags)) == []
        arr, _ = _reqs((b"cmu440", 0, 99, 7, 4))
        out = (_lib.mh_first_hits_result * 1)()
        buf = (_lib.mh_hit * 64)()
        assert L.mh_search_first_hits_batch(0, None, 1, flags, buf, 64, out) == minehip.MH_EINVAL
        assert b"NULL" in L.mh_last_error()
        assert L.mh_search_first_hits_batch(0, arr, 1, flags, buf, 64, None) == minehip.MH_EINVAL
        assert L.mh_search_first_hits_batch(0, arr, 1, flags, buf, 3, out) == minehip.MH_EINVAL        # a short hits_cap
        assert b"hits_cap" in L.mh_last_error()
        assert L.mh_search_first_hits_batch(0, arr, 1, flags, None, 64, out) == minehip.MH_EINVAL      # hits NULL, a positive sum
        assert b"hits is NULL" in L.mh_last_error()
        # every request refused on its own: each has its status, the call is MH_OK, no device needed;
        # the offsets are the prefix sums of k, failed requests included, a k of 0 or out of range as 0
        big = b"y" * ((1 << 20) + 1)
        bad, _ = _reqs((b"x", 9, 3, 5, 7), (None, 0, 9, 5, 2), (big, 0, 4, 5, 3), (b"y", 0, 4, 5, MAXCAP + 1),
                       (b"y", 0, 4, 5, 0), (b"y", U64, 0, U64, 11), (b"z", 4, 1, 0, 1))
        out = (_lib.mh_first_hits_result * 7)()
        assert L.mh_search_first_hits_batch(0, bad, 7, flags, buf, 24, out) == minehip.MH_OK
        assert [o.status for o in out] == [minehip.MH_ERANGE, minehip.MH_EINVAL, minehip.MH_ETOOLONG, minehip.MH_EINVAL,
                                           minehip.MH_EINVAL, minehip.MH_ERANGE, minehip.MH_ERANGE]
        assert [o.offset for o in out] == [0, 7, 9, 12, 12, 12, 23]
        assert [(o.path, o.stored, o.scanned, o.hash, o.nonce) for o in out] == [(0, 0, 0, 0, 0)] * 7
        assert L.mh_search_first_hits_batch(0, bad, 7, flags, buf, 23, out) == minehip.MH_EINVAL       # the k add up to 24
        assert L.mh_search_first_hits_batch(0, bad, 7, flags, None, 24, out) == minehip.MH_EINVAL
    for flags in (2, 3, 4, 1 << 31):               # an unknown flag bit, before anything else
        assert L.mh_search_first_hits_batch(0, None, 0, flags, None, 0, None) == minehip.MH_EINVAL
        assert b"flag" in L.mh_last_error()
        assert L.mh_first_hits_batch_regions(None, 0, flags, None, 0) == minehip.MH_EINVAL
    res = minehip.search_first_hits_batch([("x", 9, 3, 1, 1), ("y", 0, 5, 1, MAXCAP + 1), ("y", 0, 5, 1, 0)], errors="return")
    assert [(r.code, r.index) for r in res] == [(minehip.MH_ERANGE, 0), (minehip.MH_EINVAL, 1), (minehip.MH_EINVAL, 2)]
    assert "MH_HITS_MAX_CAP" in str(res[1]) and "k is 0" in str(res[2])
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_first_hits_batch([("x", 9, 3, 1, 1)])
    assert e.value.code == minehip.MH_ERANGE and e.value.index == 0 and "request 0" in str(e.value)
    if minehip.device_count() == 0:                # no CPU fallback: fused and fallback requests alike
        for r in (("cmu440", 0, 99, U64, 1), ("cmu440", 0, 3 * 10 ** 6, U64, 4)):
            for fuse in (False, True):
                with pytest.raises(minehip.MinehipError) as e:
                    minehip.search_first_hits_batch([r, ("x", 9, 3, 1, 1)], errors="return", fuse_fast=fuse)
                assert e.value.code == minehip.MH_ENODEV


def test_python_argument_checks():
    for bad in (-1, 1 << 64, 0.5, "7", None, True):
        with pytest.raises(ValueError, match="target"):
            minehip.search_first_hits_batch([("x", 0, 1, bad, 1)])
        with pytest.raises(ValueError, match="k ="):
            minehip.search_first_hits_batch([("x", 0, 1, 5, bad)])
    with pytest.raises(ValueError):
        minehip.search_first_hits_batch([("x", 0, 1, 5)])              # no k
    with pytest.raises(ValueError):
        minehip.search_first_hits_batch([("x", 0, 1, 5, 1)], errors="ignore")


def test_dev_build_refuses_the_hash_and_code_object_hooks():
    code = """
import minehip
for fuse in (False, True):
    try:
        minehip.search_first_hits_batch([("cmu440", 0, 99, 7, 1)], fuse_fast=fuse)
        print("ran")
    except minehip.MinehipError as e:
        print(e.code, str(e))
"""
    for hook in (dict(MINEHIP_DEV_HASH_KEEP="8,0"), dict(MINEHIP_DEV_HASH_XOR="1f"),
                 dict(MINEHIP_DEV_CODE_OBJECT="/nonexistent.hsaco")):
        r = run_dev(code, **hook)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 2 and all(l.startswith(str(minehip.MH_EINVAL)) and list(hook)[0] in l for l in lines), r.stdout


SHAPES = [("cmu440", 0, 1_999_999), ("cmu441", 0, 999_999), ("x" * 60, 1_000_000, 1_499_999), ("cmu440", 95_000, 105_123),
          ("cmu440", 1_048_000, 2_200_000), ("cmu440", 0, 3_000_000), ("q", 5, 5), ("", 0, 100), ("cmu440", 0, 2 * 10 ** 9)]
KS = [1, 2, 300, 100, 4, 16, 4, 1000, 2]


def check_regions(reqs, fuse, window_limit=MAXCAP):
    """first_hits_batch_regions against mh_batch_plan_ex and the region rule.  Returns (windows,
    fused, fallbacks, cut)."""
    plan = {}
    for p in minehip.batch_plan_ex([r[:3] for r in reqs], fuse_fast=fuse):
        kind = 1 if p["kind"] == 1 else 0
        assert plan.setdefault(p["req"], (kind, p["pass"])) == (kind, p["pass"])
    regs = minehip.first_hits_batch_regions(reqs, fuse_fast=fuse)
    assert [g["req"] for g in regs] == list(range(len(reqs)))
    assert [(g["kind"], g["pass"]) for g in regs] == [plan[i] for i in range(len(reqs))]
    window, used, last_pass, cut = 0, 0, -1, 0
    for g, r in zip(regs, reqs):
        if g["kind"] == 1:
            assert (g["window"], g["offset"], g["slots"]) == (-1, 0, 0)
            continue
        size = r[2] - r[1] + 1
        want = min(size, max(4 * r[4], 256))
        assert g["pass"] >= last_pass and g["window"] in (window, window + 1), g
        if g["window"] != window:
            assert g["pass"] > last_pass                 # a window starts with a pass
            window, used = g["window"], 0
        last_pass = g["pass"]
        # in order, disjoint, inside the buffer, never larger than the request's nonce count
        assert g["offset"] == used and g["slots"] == min(want, window_limit - used) <= size, (g, want, used)
        cut += g["slots"] < want
        used += g["slots"]
        assert used <= window_limit
    return window + 1, sum(g["kind"] == 0 for g in regs), sum(g["kind"] == 1 for g in regs), cut


def test_regions_follow_the_plan_and_the_rule():
    reqs = [s + (2 ** 64 // 10 ** 6, k) for s, k in zip(SHAPES, KS)]
    for fuse in (False, True):
        windows, fused, fallbacks, cut = check_regions(reqs, fuse)
        assert windows == 1 and cut == 0
        assert (fused, fallbacks) == ((8, 1) if fuse else (6, 3))         # the fast-piece shapes fuse only with the flag
    regs = minehip.first_hits_batch_regions(reqs, fuse_fast=True)
    assert [g["slots"] for g in regs] == [256, 256, 1200, 400, 256, 256, 1, 101, 0]
    # the plan depends on neither targets nor k
    other = [s + (0, 7) for s in SHAPES]
    assert [(g["kind"], g["pass"]) for g in minehip.first_hits_batch_regions(other, fuse_fast=True)] == \
        [(g["kind"], g["pass"]) for g in regs]
    with pytest.raises(minehip.MinehipError) as e:
        minehip.first_hits_batch_regions([("x", 0, 9, 1, 0)])
    assert e.value.code == minehip.MH_EINVAL
    with pytest.raises(minehip.MinehipError) as e:
        minehip.first_hits_batch_regions([("x", 9, 0, 1, 1)], fuse_fast=True)
    assert e.value.code == minehip.MH_ERANGE
    assert minehip.first_hits_batch_regions([]) == []


def test_window_cuts_and_drains_under_a_small_buffer():
    reqs = [s + (5, k) for s, k in zip(SHAPES, KS)] * 3
    with env(MINEHIP_HITS_SLOTS=64):
        for fuse in (False, True):
            windows, fused, _, cut = check_regions(reqs, fuse, 64)
            assert windows == 1 and cut >= fused - 2                      # one pass: no drain inside it, the regions run out
        with env(MINEHIP_BATCH_SLOTS=1500):
            for fuse in (False, True):
                windows, fused, fallbacks, cut = check_regions(reqs, fuse, 64)
                assert windows >= 3 and cut > 0 and fused >= 6 and fallbacks > 0   # several passes: a drain before each
