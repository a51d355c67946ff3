"""mh_search_hits_batch / mh_hits_batch_regions on the CPU: the ABI surface, the argument handling
up to the device call, the binding, and the host-built schedule of the fused passes -- which request
gets which region of the device hit buffer, and which passes start after a drain.  No GPU compute
is called here.

The schedule (include/minehip.h): fused or fallback and the passes are
mh_batch_plan's; in request order a fused request gets min(cap, its nonce count, slots left in the
window) slots at the next free offset, and a pass whose requests want more than the window has
left starts a new window."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

import minehip
from minehip import _lib
from conftest import ROOT, PKG, run_dev

U64 = (1 << 64) - 1
MAXCAP = 1 << 20


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mh_search_hits_batch", "mh_hits_batch_regions"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    fn = minehip.lib.mh_search_hits_batch
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 6
    assert fn.argtypes[1]._type_ is _lib.mh_hits_request and fn.argtypes[3]._type_ is _lib.mh_hit
    assert fn.argtypes[4] is ctypes.c_size_t and fn.argtypes[5]._type_ is _lib.mh_hits_result
    fr = minehip.lib.mh_hits_batch_regions
    assert fr.restype is ctypes.c_int64 and len(fr.argtypes) == 4
    assert fr.argtypes[0]._type_ is _lib.mh_hits_request and fr.argtypes[2]._type_ is _lib.mh_hits_region
    assert [f for f, _ in _lib.mh_hits_request._fields_] == ["msg", "len", "lower", "upper", "target", "cap"]
    assert [f for f, _ in _lib.mh_hits_result._fields_] == ["status", "reserved", "count", "stored", "hash", "nonce",
                                                            "offset"]
    assert [f for f, _ in _lib.mh_hits_region._fields_] == ["req", "kind", "pass", "window", "reserved", "offset",
                                                            "slots"]
    assert ctypes.sizeof(_lib.mh_hits_request) == 48 and ctypes.sizeof(_lib.mh_hits_result) == 48
    assert ctypes.sizeof(_lib.mh_hits_region) == 40
    assert callable(minehip.search_hits_batch) and callable(minehip.hits_batch_regions)
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed


def _reqs(*rows):
    arr = (_lib.mh_hits_request * len(rows))()
    keep = []
    for i, (m, lo, hi, T, cap) in enumerate(rows):
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper = m, (len(m) if m is not None else 3), lo, hi
        arr[i].target, arr[i].cap = T, cap
    return arr, keep


def test_arguments_without_a_device():
    L = minehip.lib
    assert L.mh_search_hits_batch(0, None, 0, None, 0, None) == minehip.MH_OK   # n = 0: no device touched
    assert minehip.search_hits_batch([]) == []
    arr, _ = _reqs((b"cmu440", 0, 99, 7, 4))
    out = (_lib.mh_hits_result * 1)()
    buf = (_lib.mh_hit * 64)()
    assert L.mh_search_hits_batch(0, None, 1, buf, 64, out) == minehip.MH_EINVAL
    assert b"NULL" in L.mh_last_error()
    assert L.mh_search_hits_batch(0, arr, 1, buf, 64, None) == minehip.MH_EINVAL
    assert L.mh_search_hits_batch(0, arr, 1, buf, 3, out) == minehip.MH_EINVAL        # a short hits_cap
    assert b"hits_cap" in L.mh_last_error()
    assert L.mh_search_hits_batch(0, arr, 1, None, 64, out) == minehip.MH_EINVAL      # hits NULL, a positive cap sum
    assert b"hits is NULL" in L.mh_last_error()
    # every request refused on its own: each has its status, the call is MH_OK, no device needed;
    # the offsets are the prefix sums of the caps, failed requests included, an out-of-range cap as 0
    big = b"y" * ((1 << 20) + 1)
    bad, _ = _reqs((b"x", 9, 3, 5, 7), (None, 0, 9, 5, 2), (big, 0, 4, 5, 0), (b"y", 0, 4, 5, MAXCAP + 1),
                   (b"y", U64, 0, U64, 11), (b"z", 4, 1, 0, 1))
    out = (_lib.mh_hits_result * 6)()
    assert L.mh_search_hits_batch(0, bad, 6, buf, 21, out) == minehip.MH_OK
    assert [o.status for o in out] == [minehip.MH_ERANGE, minehip.MH_EINVAL, minehip.MH_ETOOLONG, minehip.MH_EINVAL,
                                       minehip.MH_ERANGE, minehip.MH_ERANGE]
    assert [o.offset for o in out] == [0, 7, 9, 9, 9, 20]
    assert L.mh_search_hits_batch(0, bad, 6, buf, 20, out) == minehip.MH_EINVAL       # the caps add up to 21
    assert L.mh_search_hits_batch(0, bad, 6, None, 21, out) == minehip.MH_EINVAL
    zero, _ = _reqs((b"x", 9, 3, 5, 0), (b"x", 2, 1, 5, 0))
    assert L.mh_search_hits_batch(0, zero, 2, None, 0, out) == minehip.MH_OK          # count only: hits may be NULL
    res = minehip.search_hits_batch([("x", 9, 3, 1), ("y", 0, 5, 1, MAXCAP + 1), ("y", 2, 1, 1, 0)], errors="return")
    assert [type(r) for r in res] == [minehip.MinehipError] * 3
    assert [(r.code, r.index) for r in res] == [(minehip.MH_ERANGE, 0), (minehip.MH_EINVAL, 1), (minehip.MH_ERANGE, 2)]
    assert "MH_HITS_MAX_CAP" in str(res[1])
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_hits_batch([("x", 9, 3, 1)])
    assert e.value.code == minehip.MH_ERANGE and e.value.index == 0 and "request 0" in str(e.value)
    if minehip.device_count() == 0:                # no CPU fallback: fused and fallback requests alike
        for r in (("cmu440", 0, 99, U64), ("cmu440", 0, 3 * 10 ** 6, U64), ("cmu440", 0, 99, U64, 0)):
            with pytest.raises(minehip.MinehipError) as e:
                minehip.search_hits_batch([r, ("x", 9, 3, 1)], errors="return")
            assert e.value.code == minehip.MH_ENODEV


def test_python_argument_checks():
    for bad in (-1, 1 << 64, 0.5, "7", None, True):
        with pytest.raises(ValueError, match="target"):
            minehip.search_hits_batch([("x", 0, 1, bad)])
        with pytest.raises(ValueError, match="cap"):
            minehip.search_hits_batch([("x", 0, 1, 5, bad)])
        with pytest.raises(ValueError, match="cap"):
            minehip.search_hits_batch([("x", 0, 1, 5)], cap=bad)
    with pytest.raises(ValueError):
        minehip.search_hits_batch([("x", 0, 1)])              # no target
    with pytest.raises(ValueError):
        minehip.search_hits_batch([("x", -1, 1, 5)])
    with pytest.raises(ValueError):
        minehip.search_hits_batch([("x", 0, 1, 5)], errors="ignore")


def check_regions(reqs, cap, slots_limit=MAXCAP):
    """hits_batch_regions against mh_batch_plan and the region rule.  Returns (windows, fused,
    fallbacks)."""
    plan = {}
    for it in minehip.batch_plan([r[:3] for r in reqs]):
        plan.setdefault(it["req"], (it["kind"], it["pass"]))
    regs = minehip.hits_batch_regions(reqs, cap)
    assert [g["req"] for g in regs] == list(range(len(reqs)))
    assert [(g["kind"], g["pass"]) for g in regs] == [plan[i] for i in range(len(reqs))]
    window, used, last_pass = 0, 0, -1
    for g, r in zip(regs, reqs):
        if g["kind"] == 1:
            assert (g["window"], g["offset"], g["slots"]) == (-1, 0, 0)
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
        assert used <= slots_limit
    return window + 1, sum(1 for g in regs if g["kind"] == 0), sum(1 for g in regs if g["kind"] == 1)


def test_regions_of_the_edges():
    from test_gpu_batch import EDGES
    reqs = [r + (5,) for r in EDGES]
    regs = minehip.hits_batch_regions(reqs, 16)
    assert all((g["kind"], g["pass"], g["window"]) == (0, 0, 0) for g in regs)       # all fused, one pass, no drain
    assert [g["slots"] for g in regs] == [min(16, hi - lo + 1) for _, lo, hi in EDGES]
    assert [g["offset"] for g in regs] == [sum(g["slots"] for g in regs[:i]) for i in range(len(regs))]
    assert check_regions(reqs, 16) == (1, len(EDGES), 0)
    # a cap of its own, a count-only request, and a target plays no part
    mixed = [EDGES[3] + (0, 0), EDGES[3] + (U64, 3), EDGES[3] + (7,)]
    assert [(g["offset"], g["slots"]) for g in minehip.hits_batch_regions(mixed, 16)] == [(0, 0), (0, 3), (3, 16)]


def test_regions_arguments():
    L = minehip.lib
    arr, _ = _reqs((b"tile", 0, 2560, 1, 4), (b"tile", 0, 2559, 1, 9))
    buf = (_lib.mh_hits_region * 2)()
    assert L.mh_hits_batch_regions(None, 0, None, 0) == 0
    assert L.mh_hits_batch_regions(arr, 2, None, 16) == 2             # counting only
    assert L.mh_hits_batch_regions(arr, 2, buf, 1) == 2               # cap + 1: truncated, the first cap written
    assert (buf[0].req, buf[0].offset, buf[0].slots) == (0, 0, 4)
    assert L.mh_hits_batch_regions(arr, 2, buf, 2) == 2 and (buf[1].req, buf[1].offset, buf[1].slots) == (1, 4, 9)
    assert L.mh_hits_batch_regions(arr, 2, None, -1) == minehip.MH_EINVAL
    assert L.mh_hits_batch_regions(None, 2, None, 16) == minehip.MH_EINVAL
    bad, _ = _reqs((b"cmu440", 0, 99, 1, 4), (b"x", 9, 3, 1, 4))
    assert L.mh_hits_batch_regions(bad, 2, None, 16) == minehip.MH_ERANGE
    bad, _ = _reqs((b"cmu440", 0, 99, 1, MAXCAP + 1))
    assert L.mh_hits_batch_regions(bad, 1, None, 16) == minehip.MH_EINVAL
    assert b"MH_HITS_MAX_CAP" in L.mh_last_error()


def test_regions_follow_the_batch_plan():
    from test_gpu_batch import fuzz_requests, capacity_requests
    assert check_regions([r + (1,) for r in fuzz_requests()], 4096) == (1, 200, 0)
    assert check_regions([r + (1,) for r in capacity_requests()], 4096) == (1, 41, 0)
    mixed = [(b"cmu440", 10, 500, 1), (b"cmu440", 0, 3 * 10 ** 6, 1), (b"abc", 0, 999, 1)]
    assert check_regions(mixed, 64) == (1, 2, 1)


def _child(code, **env):
    pre = f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}, {os.path.join(ROOT, 'tests')!r}]\n"
    r = subprocess.run([sys.executable, "-c", pre + code], env=dict(os.environ, **{k: str(v) for k, v in env.items()}),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_regions_with_a_small_hit_buffer():
    """MINEHIP_HITS_SLOTS=8 (a child process): the edges with cap 16 no longer fit one window, so
    windows advance; every region lies inside 8 slots and the regions of one window are disjoint."""
    code = ("import json, minehip, test_hits_batch as t\n"
            "from test_gpu_batch import EDGES\n"
            "reqs = [r + (5,) for r in EDGES]\n"
            "w = t.check_regions(reqs, 16, 8)\n"
            "print(json.dumps([w, minehip.hits_batch_regions(reqs, 16)]))\n")
    (windows, fused, fallbacks), regs = _child(code, MINEHIP_HITS_SLOTS=8)
    assert fused == 19 and fallbacks == 0
    # all in one pass: a window starts with a pass, so there is still one window, cut short
    assert windows == 1 and all(g["offset"] + g["slots"] <= 8 for g in regs)
    assert sum(g["slots"] for g in regs) == 8 and [g["slots"] for g in regs[:4]] == [1, 1, 6, 0]
    # and with a pass per two requests (MINEHIP_BATCH_SLOTS=2: the one-tile edges) windows advance
    code = ("import json, minehip, test_hits_batch as t\n"
            "from test_gpu_batch import EDGES\n"
            "reqs = [r + (5,) for r in EDGES if r[2] - r[1] < 1000]\n"
            "w = t.check_regions(reqs, 16, 8)\n"
            "print(json.dumps([w, minehip.hits_batch_regions(reqs, 16)]))\n")
    (windows, fused, fallbacks), regs = _child(code, MINEHIP_HITS_SLOTS=8, MINEHIP_BATCH_SLOTS=2)
    assert windows > 2 and fallbacks == 0
    assert all(g["offset"] + g["slots"] <= 8 for g in regs)
    by_window = {}
    for g in regs:
        by_window.setdefault(g["window"], []).append((g["offset"], g["offset"] + g["slots"]))
    for spans in by_window.values():
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans       # disjoint, in order


def test_regions_under_a_small_pass_capacity():
    """MINEHIP_BATCH_SLOTS=32 (a child process): kind and pass are still mh_batch_plan's -- the
    capacity requests take 20 passes and the last request is a fallback."""
    code = ("import json, minehip, test_hits_batch as t\n"
            "from test_gpu_batch import capacity_requests\n"
            "reqs = [r + (1,) for r in capacity_requests()]\n"
            "w = t.check_regions(reqs, 4096)\n"
            "regs = minehip.hits_batch_regions(reqs, 4096)\n"
            "print(json.dumps([w, max(g['pass'] for g in regs) + 1, regs[-1]['kind']]))\n")
    (windows, fused, fallbacks), passes, last_kind = _child(code, MINEHIP_BATCH_SLOTS=32)
    assert (windows, fused, fallbacks, passes, last_kind) == (1, 40, 1, 20, 1)


def test_schedule_under_sanitizers(tmp_path):
    """plan_hits_batch_pass and hits_batch_tables_ok (csrc/plan.cpp) under AddressSanitizer and
    UndefinedBehaviorSanitizer: the stand-alone tests/host/hits_batch_host.cpp over random batches,
    caps, pass capacities and hit-buffer sizes, ranges at the top of u64 included, and tables
    corrupted on purpose."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "hits_batch_host")
    csrc = os.path.join(PKG, "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out,
           os.path.join(ROOT, "tests", "host", "hits_batch_host.cpp"), os.path.join(csrc, "plan.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out, "440", "30"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_dev_build_refuses_the_hash_hooks():
    """As mh_search_hits: with a hash or code-object hook set the dev build fails with MH_EINVAL
    before it touches a device, instead of silently ignoring the hook."""
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    try:
        minehip.search_hits_batch([(b"cmu440", 0, 1000, 5)])
        raise SystemExit("searched with " + k)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and k in str(e), e
    del os.environ[k]
print("refused")
""", timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:] + r.stdout[-500:]
