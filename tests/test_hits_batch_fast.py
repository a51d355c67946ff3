"""mh_search_hits_batch_ex / mh_hits_batch_regions_ex on the CPU: the ABI surface, the argument
handling up to the device call, the binding, and the host-built schedule of passes with fused fast
pieces.  No GPU compute is called here.

The schedule (include/minehip.h): fused or fallback and the passes are
mh_batch_plan_ex's; windows and regions follow mh_search_hits_batch's rule -- in request order a
fused request gets min(cap, its nonce count, slots left in the window) slots at the next free
offset, and a pass whose requests want more than the window has left starts a new window."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import minehip
from minehip import _lib
from conftest import ROOT, PKG, run_dev
from test_gpu_batch_fast import EXTRA, SHAPES
from test_hits_batch import _reqs

U64 = (1 << 64) - 1
MAXCAP = 1 << 20
FUSE = minehip.MH_BATCH_FUSE_FAST
MIXED = SHAPES + EXTRA     # every layout class, generic-only requests, two messages of one layout


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mh_search_hits_batch_ex", "mh_hits_batch_regions_ex"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    for name in ("mh_batch_hits_co_begin", "mh_batch_hits_co_end"):
        assert hasattr(raw, name), name
    fn = minehip.lib.mh_search_hits_batch_ex
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7 and fn.argtypes[3] is ctypes.c_uint32
    assert fn.argtypes[1]._type_ is _lib.mh_hits_request and fn.argtypes[4]._type_ is _lib.mh_hit
    assert fn.argtypes[5] is ctypes.c_size_t and fn.argtypes[6]._type_ is _lib.mh_hits_result
    fr = minehip.lib.mh_hits_batch_regions_ex
    assert fr.restype is ctypes.c_int64 and len(fr.argtypes) == 5 and fr.argtypes[2] is ctypes.c_uint32
    assert fr.argtypes[0]._type_ is _lib.mh_hits_request and fr.argtypes[3]._type_ is _lib.mh_hits_region
    assert ctypes.sizeof(_lib.mh_hits_request) == 48 and ctypes.sizeof(_lib.mh_hits_result) == 48
    assert ctypes.sizeof(_lib.mh_hits_region) == 40
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed
    from minehip import codeobj
    assert callable(codeobj.batch_hits_code_object) and callable(codeobj.batch_hits_kernel_resources)
    assert codeobj.batch_hits_code_object()[:4] == b"\x7fELF"


def test_arguments_without_a_device():
    L = minehip.lib
    arr, _ = _reqs((b"cmu440", 0, 99, 7, 4))
    out = (_lib.mh_hits_result * 1)()
    buf = (_lib.mh_hit * 64)()
    for flags in (2, 3, 1 << 31, 0xFFFFFFFE):                      # an unknown bit, with or without the known one
        assert L.mh_search_hits_batch_ex(0, arr, 1, flags, buf, 64, out) == minehip.MH_EINVAL
        assert b"unknown flag" in L.mh_last_error()
        assert L.mh_search_hits_batch_ex(0, None, 0, flags, None, 0, None) == minehip.MH_EINVAL   # before n == 0
        assert L.mh_hits_batch_regions_ex(arr, 1, flags, None, 16) == minehip.MH_EINVAL
    for flags in (0, FUSE):
        assert L.mh_search_hits_batch_ex(0, None, 0, flags, None, 0, None) == minehip.MH_OK   # n = 0: no device touched
        assert L.mh_search_hits_batch_ex(0, None, 1, flags, buf, 64, out) == minehip.MH_EINVAL
        assert b"NULL" in L.mh_last_error()
        assert L.mh_search_hits_batch_ex(0, arr, 1, flags, buf, 64, None) == minehip.MH_EINVAL
        assert L.mh_search_hits_batch_ex(0, arr, 1, flags, buf, 3, out) == minehip.MH_EINVAL    # a short hits_cap
        assert b"hits_cap" in L.mh_last_error()
        assert L.mh_search_hits_batch_ex(0, arr, 1, flags, None, 64, out) == minehip.MH_EINVAL  # hits NULL, a cap sum > 0
        assert b"hits is NULL" in L.mh_last_error()
        # every request refused on its own: each has its status, the call is MH_OK, no device needed;
        # the offsets are the prefix sums of the caps, failed requests included, an out-of-range cap as 0
        big = b"y" * ((1 << 20) + 1)
        bad, _ = _reqs((b"x", 9, 3, 5, 7), (None, 0, 9, 5, 2), (big, 0, 4, 5, 0), (b"y", 0, 4, 5, MAXCAP + 1),
                       (b"y", U64, 0, U64, 11), (b"z", 4, 1, 0, 1))
        res = (_lib.mh_hits_result * 6)()
        assert L.mh_search_hits_batch_ex(0, bad, 6, flags, buf, 21, res) == minehip.MH_OK
        assert [o.status for o in res] == [minehip.MH_ERANGE, minehip.MH_EINVAL, minehip.MH_ETOOLONG,
                                           minehip.MH_EINVAL, minehip.MH_ERANGE, minehip.MH_ERANGE]
        assert [o.offset for o in res] == [0, 7, 9, 9, 9, 20]
        assert L.mh_search_hits_batch_ex(0, bad, 6, flags, buf, 20, res) == minehip.MH_EINVAL   # the caps add up to 21
        zero, _ = _reqs((b"x", 9, 3, 5, 0), (b"x", 2, 1, 5, 0))
        assert L.mh_search_hits_batch_ex(0, zero, 2, flags, None, 0, res) == minehip.MH_OK      # count only
    assert minehip.search_hits_batch([], fuse_fast=True) == []
    res = minehip.search_hits_batch([("x", 9, 3, 1), ("y", 0, 5, 1, MAXCAP + 1)], errors="return", fuse_fast=True)
    assert [(r.code, r.index) for r in res] == [(minehip.MH_ERANGE, 0), (minehip.MH_EINVAL, 1)]
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_hits_batch([("x", 9, 3, 1)], fuse_fast=True)
    assert e.value.code == minehip.MH_ERANGE and e.value.index == 0
    if minehip.device_count() == 0:                # no CPU fallback: fused and fallback requests alike
        for r in (("cmu440", 0, 99, U64), ("cmu440", 0, 3 * 10 ** 6, U64), ("cmu440", 0, 2 * 10 ** 9, U64, 0)):
            with pytest.raises(minehip.MinehipError) as e:
                minehip.search_hits_batch([r], errors="return", fuse_fast=True)
            assert e.value.code == minehip.MH_ENODEV


def check_regions_ex(reqs, cap, slots_limit=MAXCAP):
    """hits_batch_regions(fuse_fast=True) against mh_batch_plan_ex and the region rule.  Returns
    (windows, fused, fused with a fast piece, fallbacks)."""
    plan = minehip.batch_plan_ex([r[:3] for r in reqs])
    regs = minehip.hits_batch_regions(reqs, cap, fuse_fast=True)
    assert [g["req"] for g in regs] == list(range(len(reqs)))
    fast = 0
    for i, g in enumerate(regs):                       # kind and pass follow the ex plan
        mine = [p for p in plan if p["req"] == i]
        assert mine and {p["pass"] for p in mine} == {g["pass"]}, (i, g)
        assert g["kind"] == (1 if mine[0]["kind"] == 1 else 0) and (g["kind"] == 0 or len(mine) == 1), (i, g)
        fast += any(p["kind"] == 2 for p in mine)
    window, used, last_pass = 0, 0, -1
    for g, r in zip(regs, reqs):
        if g["kind"] == 1:
            assert (g["pass"], g["window"], g["offset"], g["slots"]) == (-1, -1, 0, 0)
            continue
        c = r[4] if len(r) == 5 else cap
        want = min(c, r[2] - r[1] + 1)
        assert g["pass"] >= last_pass and g["window"] in (window, window + 1), g
        if g["window"] != window:
            assert g["pass"] > last_pass                 # a window starts with a pass
            window, used = g["window"], 0
        last_pass = g["pass"]
        assert g["offset"] == used and g["slots"] == min(want, slots_limit - used), (g, want, used)
        used += g["slots"]
        assert used <= slots_limit                       # inside the buffer, disjoint and in order
    return window + 1, sum(1 for g in regs if g["kind"] == 0), fast, sum(1 for g in regs if g["kind"] == 1)


def test_regions_follow_the_ex_plan():
    reqs = [r + (1,) for r in MIXED]
    assert check_regions_ex(reqs, 4096) == (1, 11, 8, 0)
    regs = minehip.hits_batch_regions(reqs, 4096, fuse_fast=True)
    assert [g["slots"] for g in regs] == [min(4096, hi - lo + 1) for _, lo, hi in MIXED]
    # without the flag the requests with a fast piece are fallbacks
    plain = minehip.hits_batch_regions(reqs, 4096)
    assert [g["kind"] for g in plain] == [1] * 7 + [0, 0, 0, 1]
    # a cap of its own, a count-only request; the target plays no part
    mixed = [SHAPES[0] + (0, 0), SHAPES[0] + (U64, 3), SHAPES[0] + (7,)]
    assert [(g["offset"], g["slots"]) for g in minehip.hits_batch_regions(mixed, 16, fuse_fast=True)] == \
        [(0, 0), (0, 3), (3, 16)]
    # above MH_BATCH_FAST_MAX_NONCES: a fallback, beside fused requests
    big = [(b"cmu440", 0, minehip.MH_BATCH_FAST_MAX_NONCES, 1), (b"cmu440", 0, minehip.MH_BATCH_FAST_MAX_NONCES - 1, 1),
           SHAPES[0] + (1,)]
    regs = minehip.hits_batch_regions(big, 64, fuse_fast=True)
    assert [g["kind"] for g in regs] == [1, 0, 0] and (regs[0]["pass"], regs[0]["window"]) == (-1, -1)
    check_regions_ex(big, 64)


def test_flag_zero_is_hits_batch_regions():
    from test_gpu_batch import fuzz_requests
    reqs = [r + (1,) for r in fuzz_requests()[:60]] + [SHAPES[0] + (1,)]
    assert minehip.hits_batch_regions(reqs, 16, flags=0) == minehip.hits_batch_regions(reqs, 16)
    L = minehip.lib
    arr, _ = _reqs((b"tile", 0, 2560, 1, 4), (b"tile", 0, 2559, 1, 9))
    buf = (_lib.mh_hits_region * 2)()
    for flags in (0, FUSE):
        assert L.mh_hits_batch_regions_ex(None, 0, flags, None, 0) == 0
        assert L.mh_hits_batch_regions_ex(arr, 2, flags, None, 16) == 2             # counting only
        assert L.mh_hits_batch_regions_ex(arr, 2, flags, buf, 1) == 2               # cap + 1: the first cap written
        assert (buf[0].req, buf[0].offset, buf[0].slots) == (0, 0, 4)
        assert L.mh_hits_batch_regions_ex(arr, 2, flags, buf, 2) == 2
        assert (buf[1].req, buf[1].offset, buf[1].slots) == (1, 4, 9)
        assert L.mh_hits_batch_regions_ex(arr, 2, flags, None, -1) == minehip.MH_EINVAL
        assert L.mh_hits_batch_regions_ex(None, 2, flags, None, 16) == minehip.MH_EINVAL
        bad, _ = _reqs((b"cmu440", 0, 99, 1, 4), (b"x", 9, 3, 1, 4))
        assert L.mh_hits_batch_regions_ex(bad, 2, flags, None, 16) == minehip.MH_ERANGE
        bad, _ = _reqs((b"cmu440", 0, 99, 1, MAXCAP + 1))
        assert L.mh_hits_batch_regions_ex(bad, 1, flags, None, 16) == minehip.MH_EINVAL
        assert b"MH_HITS_MAX_CAP" in L.mh_last_error()


def _child(code, **env):
    pre = f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}, {os.path.join(ROOT, 'tests')!r}]\n"
    r = subprocess.run([sys.executable, "-c", pre + code], env=dict(os.environ, **{k: str(v) for k, v in env.items()}),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_regions_with_a_small_hit_buffer_and_pass_capacity():
    """MINEHIP_HITS_SLOTS small (child processes): regions are cut short by the window; with
    MINEHIP_BATCH_SLOTS as well the passes multiply, the large requests fall back and windows
    advance; the regions of one window stay disjoint, in order and inside the buffer."""
    code = ("import json, minehip, test_hits_batch_fast as t\n"
            "reqs = [r + (1,) for r in t.MIXED]\n"
            "w = t.check_regions_ex(reqs, 4096, {slots})\n"
            "print(json.dumps([w, minehip.hits_batch_regions(reqs, 4096, fuse_fast=True)]))\n")
    (windows, fused, fast, fallbacks), regs = _child(code.format(slots=5000), MINEHIP_HITS_SLOTS=5000)
    assert (windows, fused, fast, fallbacks) == (1, 11, 8, 0)       # one pass: one window, cut short
    assert [g["slots"] for g in regs[:3]] == [4096, 904, 0] and sum(g["slots"] for g in regs) == 5000
    (windows, fused, fast, fallbacks), regs = _child(code.format(slots=1500), MINEHIP_HITS_SLOTS=1500,
                                                    MINEHIP_BATCH_SLOTS=1000)
    assert windows >= 2 and fallbacks >= 1 and fast >= 2 and fused + fallbacks == 11
    assert all(g["offset"] + g["slots"] <= 1500 for g in regs)
    by_window = {}
    for g in regs:
        if g["kind"] == 0:
            by_window.setdefault(g["window"], []).append((g["offset"], g["offset"] + g["slots"]))
    for spans in by_window.values():
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans       # disjoint, in order


def test_dev_build_refuses_the_hash_hooks():
    """As mh_search_hits_batch: with a hash or code-object hook set the dev build fails with
    MH_EINVAL before it touches a device, instead of silently ignoring the hook."""
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    try:
        minehip.search_hits_batch([(b"cmu440", 0, 3000000, 5)], fuse_fast=True)
        raise SystemExit("searched with " + k)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and k in str(e), e
    del os.environ[k]
print("refused")
""", timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:] + r.stdout[-500:]
