"""mh_search_first_batch / mh_first_batch_order on the CPU: the ABI surface, the argument handling
up to the device call, the binding, and the host-built dispatch order of batch_scan_first.  No GPU
compute is called here.

The order (include/minehip.h): workgroup b runs the tile of partial slot order[b];
rank-major means slot seg[r] + k of every request r that has k + 1 tiles, for k = 0, 1, ..., in
request order within a rank."""
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


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mh_search_first_batch", "mh_first_batch_order"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    fn = minehip.lib.mh_search_first_batch
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 4
    assert fn.argtypes[1]._type_ is _lib.mh_first_request and fn.argtypes[3]._type_ is _lib.mh_first_result
    fo = minehip.lib.mh_first_batch_order
    assert fo.restype is ctypes.c_int64 and len(fo.argtypes) == 5
    assert fo.argtypes[0]._type_ is _lib.mh_request and fo.argtypes[3]._type_ is ctypes.c_uint32
    assert ctypes.sizeof(_lib.mh_first_request) == 40 and ctypes.sizeof(_lib.mh_first_result) == 32
    assert [f for f, _ in _lib.mh_first_request._fields_] == ["msg", "len", "lower", "upper", "target"]
    assert [f for f, _ in _lib.mh_first_result._fields_] == ["status", "found", "hash", "nonce", "scanned"]
    assert callable(minehip.search_first_batch) and callable(minehip.first_batch_order)
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed


def _reqs(*quads):
    arr = (_lib.mh_first_request * len(quads))()
    keep = []
    for i, (m, lo, hi, T) in enumerate(quads):
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper, arr[i].target = m, (len(m) if m is not None else 3), lo, hi, T
    return arr, keep


def test_arguments_without_a_device():
    L = minehip.lib
    assert L.mh_search_first_batch(0, None, 0, None) == minehip.MH_OK   # n = 0: no device touched
    assert minehip.search_first_batch([]) == []
    arr, _ = _reqs((b"cmu440", 0, 99, 7))
    out = (_lib.mh_first_result * 1)()
    assert L.mh_search_first_batch(0, None, 1, out) == minehip.MH_EINVAL
    assert b"NULL" in L.mh_last_error()
    assert L.mh_search_first_batch(0, arr, 1, None) == minehip.MH_EINVAL
    # every request refused on its own: each has its status, the call is MH_OK, no device needed
    big = b"y" * ((1 << 20) + 1)
    bad, _ = _reqs((b"x", 9, 3, 5), (None, 0, 9, 5), (big, 0, 4, 5), (b"y", U64, 0, U64))
    out = (_lib.mh_first_result * 4)()
    assert L.mh_search_first_batch(0, bad, 4, out) == minehip.MH_OK
    assert [o.status for o in out] == [minehip.MH_ERANGE, minehip.MH_EINVAL, minehip.MH_ETOOLONG, minehip.MH_ERANGE]
    res = minehip.search_first_batch([("x", 9, 3, 1), ("y", 2, 1, 1)], errors="return")
    assert [type(r) for r in res] == [minehip.MinehipError] * 2
    assert [(r.code, r.index) for r in res] == [(minehip.MH_ERANGE, 0), (minehip.MH_ERANGE, 1)]
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_first_batch([("x", 9, 3, 1)])
    assert e.value.code == minehip.MH_ERANGE and e.value.index == 0 and "request 0" in str(e.value)
    if minehip.device_count() == 0:                # no CPU fallback: fused and fallback requests alike
        for r in (("cmu440", 0, 99, U64), ("cmu440", 0, 3 * 10 ** 6, U64)):
            with pytest.raises(minehip.MinehipError) as e:
                minehip.search_first_batch([r], errors="return")
            assert e.value.code == minehip.MH_ENODEV


def test_python_argument_checks():
    for bad in (-1, 1 << 64, 0.5, "7", None, True):
        with pytest.raises(ValueError, match="target"):
            minehip.search_first_batch([("x", 0, 1, bad)])
    with pytest.raises(ValueError):
        minehip.search_first_batch([("x", 0, 1)])              # no target
    with pytest.raises(ValueError):
        minehip.search_first_batch([("x", -1, 1, 5)])
    with pytest.raises(ValueError):
        minehip.search_first_batch([("x", 0, 1, 5)], errors="ignore")


def test_order_of_the_last_three_edges():
    """One, two and two tiles: slots 0 | 1, 2 | 3, 4."""
    from test_gpu_batch import EDGES
    reqs = EDGES[-3:]
    assert [(it["slot"], it["slots"]) for it in minehip.batch_plan(reqs)] == [(0, 1), (1, 2), (3, 2)]
    assert minehip.first_batch_order(reqs) == [0, 1, 3, 2, 4]
    assert minehip.first_batch_order([r + (5,) for r in reqs]) == [0, 1, 3, 2, 4]   # a target plays no part
    os.environ["MINEHIP_FIRST_BATCH_ORDER"] = "request"      # read per call
    try:
        assert minehip.first_batch_order(reqs) == [0, 1, 2, 3, 4]
    finally:
        del os.environ["MINEHIP_FIRST_BATCH_ORDER"]
    assert minehip.first_batch_order(reqs) == [0, 1, 3, 2, 4]


def test_order_arguments():
    L = minehip.lib
    arr, _ = minehip._requests([(b"tile", 0, 2560), (b"tile", 0, 2559)])
    buf = (ctypes.c_uint32 * 2)()
    assert L.mh_first_batch_order(arr, 2, 0, None, 16) == 3           # counting only
    assert L.mh_first_batch_order(arr, 2, 0, buf, 2) == 3             # cap + 1: truncated, the first cap written
    assert list(buf) == [0, 2]
    assert L.mh_first_batch_order(arr, 2, 1, None, 16) == minehip.MH_EINVAL   # no such pass
    assert L.mh_first_batch_order(arr, 2, -1, None, 16) == minehip.MH_EINVAL
    assert L.mh_first_batch_order(arr, 2, 0, None, -1) == minehip.MH_EINVAL
    assert L.mh_first_batch_order(None, 2, 0, None, 16) == minehip.MH_EINVAL
    bad, _ = minehip._requests([(b"cmu440", 0, 99), (b"x", 9, 3)])
    assert L.mh_first_batch_order(bad, 2, 0, None, 16) == minehip.MH_ERANGE
    with pytest.raises(minehip.MinehipError) as e:
        minehip.first_batch_order([("cmu440", 0, 3 * 10 ** 6)])        # a fallback alone: no pass at all
    assert e.value.code == minehip.MH_EINVAL


def check_orders(reqs):
    """Every pass of the plan: its order is a permutation of the pass's slots, every request's
    slots appear in increasing order, and no request's rank-k tile comes before another request's
    rank-j tile for j < k.  Returns (passes, tiles)."""
    plan = [it for it in minehip.batch_plan(reqs) if it["kind"] == 0]
    passes = 1 + max(it["pass"] for it in plan)
    total = 0
    for p in range(passes):
        seg = {}                                   # request -> (first slot, slots) of this pass
        for it in plan:
            if it["pass"] == p:
                a, n = seg.get(it["req"], (it["slot"], 0))
                assert a + n == it["slot"]          # a request's entries are contiguous
                seg[it["req"]] = (a, n + it["slots"])
        tiles = sum(n for _, n in seg.values())
        order = minehip.first_batch_order(reqs, p)
        assert sorted(order) == list(range(tiles)), p
        owner = {}
        for r, (a, n) in seg.items():
            for k in range(n):
                owner[a + k] = (r, k)
        last_slot, ranks = {}, []
        for s in order:
            r, k = owner[s]
            assert last_slot.get(r, -1) < s, (p, r, s)
            last_slot[r] = s
            ranks.append(k)
        assert ranks == sorted(ranks), p            # rank-major: ranks never decrease along the order
        total += tiles
    return passes, total


def test_order_properties_default_capacity():
    from test_gpu_batch import fuzz_requests, capacity_requests
    assert check_orders(fuzz_requests())[0] == 1
    passes, tiles = check_orders(capacity_requests())
    assert (passes, tiles) == (1, 40 * 12 + 79)


def test_order_properties_small_capacity():
    """The same under MINEHIP_BATCH_SLOTS=32, in a child process that has it from the start: the
    capacity requests then take 20 passes of two requests each."""
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import json, test_first_batch as t\n"
            "from test_gpu_batch import fuzz_requests, capacity_requests\n"
            "print(json.dumps([t.check_orders(fuzz_requests()), t.check_orders(capacity_requests())]))\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MINEHIP_BATCH_SLOTS="32"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    fuzz, cap = json.loads(r.stdout.strip().splitlines()[-1])
    assert fuzz[0] > 1 and cap == [20, 40 * 12]


def test_tables_under_sanitizers(tmp_path):
    """build_first_batch_tables and first_batch_tables_ok (csrc/plan.cpp) and the per-tile nonce count
    and floor of batch_scan_first, replayed on the host, under AddressSanitizer and
    UndefinedBehaviorSanitizer: the stand-alone tests/host/first_batch_host.cpp over random batches
    at random capacities, ranges at the top of u64 included, and tables corrupted on purpose."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "first_batch_host")
    csrc = os.path.join(PKG, "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out,
           os.path.join(ROOT, "tests", "host", "first_batch_host.cpp"), os.path.join(csrc, "plan.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out, "440", "30"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_dev_build_refuses_the_hash_hooks():
    """As mh_search_first: with a hash or code-object hook set the dev build fails with MH_EINVAL
    before it touches a device, instead of silently ignoring the hook."""
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    try:
        minehip.search_first_batch([(b"cmu440", 0, 1000, 5)])
        raise SystemExit("searched with " + k)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and k in str(e), e
    del os.environ[k]
print("refused")
""", timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:] + r.stdout[-500:]
