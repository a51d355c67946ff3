"""CPU tests of the batched search (mh_search_batch / mh_batch_plan / mh_miner_handle_batch): the
host planner that packs many small Requests into passes of batch_scan tiles, and the argument and
error behaviour of the entry points up to the device call.  No GPU compute is called here.

The tile rule (include/minehip.h): an entry's nonces [first, first+count-1] are the
aligned decades first//10 .. last//10, and a tile is 256 decades (256 lanes x 1), so an entry
takes ceil(decades / 256) partial slots."""
import ctypes
import os
import random
import shutil
import subprocess
import sys

import pytest

import minehip
from minehip import _lib
from conftest import ROOT, PKG

U64 = (1 << 64) - 1
TILE_DECADES = 256
MAX_SLOTS = 1 << 18     # kMaxBlocksPerLaunch: the partials buffer
MAX_REQUESTS = 4096     # kBatchMaxRequests


def tiles_of(first, count):
    last = first + count - 1
    return -(-(last // 10 - first // 10 + 1) // TILE_DECADES)


def random_batch(rng):
    reqs = []
    for _ in range(rng.randrange(1, 301)):
        msg = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 131)))
        d = rng.randrange(1, 21)
        lo = rng.randrange(0 if d == 1 else 10 ** (d - 1), min(U64, 10 ** d - 1) + 1)
        hi = min(U64, lo + rng.choice((rng.randrange(1, 3 * 10 ** 6 + 1), rng.randrange(1, 3001), 1)) - 1)
        reqs.append((msg, lo, hi))
    return reqs


def check_batch(reqs, cap):
    """Every property of one batch plan under a slot capacity of `cap`."""
    items = minehip.batch_plan(reqs)
    by_req = {}
    for it in items:
        by_req.setdefault(it["req"], []).append(it)
    assert sorted(by_req) == list(range(len(reqs)))
    assert [it["req"] for it in items] == sorted(it["req"] for it in items)  # request order
    cur_pass, used, in_pass = 0, 0, 0
    totals = {}
    for i, (msg, lo, hi) in enumerate(reqs):
        mine = by_req[i]
        pieces = minehip.plan(msg, lo, hi)
        generic_tiles = sum(tiles_of(p["first"], p["count"]) for p in pieces if p["kind"] == 1)
        has_fast = any(p["kind"] == 0 for p in pieces)
        if mine[0]["kind"] == 1:  # fallback: one item, no slots; it has a fast piece or exceeds a pass
            assert len(mine) == 1
            it = mine[0]
            assert (it["first"], it["count"], it["pass"], it["slot"], it["slots"]) == \
                (lo, (hi - lo + 1) & U64, -1, 0, 0)
            assert has_fast or generic_tiles > cap, (i, lo, hi, cap)
            continue
        # fused: only generic pieces, one item per piece, tiling [lo, hi] exactly once and in order
        assert not has_fast and generic_tiles <= cap
        assert [(it["first"], it["count"]) for it in mine] == [(p["first"], p["count"]) for p in pieces]
        nxt = lo
        for it in mine:
            assert it["kind"] == 0 and it["first"] == nxt and it["count"] >= 1
            assert it["slots"] == tiles_of(it["first"], it["count"])
            nxt = it["first"] + it["count"]
        assert nxt - 1 == hi
        # its slot segment: contiguous, after the previous request's of the same pass, within capacity
        p = mine[0]["pass"]
        assert all(it["pass"] == p for it in mine)
        assert p in (cur_pass, cur_pass + 1)
        if p != cur_pass:  # a new pass only because the request did not fit the old one
            assert used + generic_tiles > cap or in_pass == MAX_REQUESTS
            cur_pass, used, in_pass = p, 0, 0
        for it in mine:
            assert it["slot"] == used
            used += it["slots"]
        in_pass += 1
        totals[p] = used
        assert used <= cap and in_pass <= MAX_REQUESTS
    assert all(0 < t <= cap for t in totals.values())
    return items


def check_batches(cap, seed=440, batches=10):
    rng = random.Random(seed)
    kinds = set()
    passes = 0
    for _ in range(batches):
        items = check_batch(random_batch(rng), cap)
        kinds |= {it["kind"] for it in items}
        passes = max(passes, 1 + max(it["pass"] for it in items))
    return kinds, passes


def test_tiling_property():
    kinds, passes = check_batches(MAX_SLOTS)
    assert kinds == {0, 1} and passes == 1  # 300 small requests fit one pass


def test_tiling_property_small_capacity():
    """The same checks with MINEHIP_BATCH_SLOTS=8 (read per call, so in a child process that has it
    from the start): many passes, and requests of more than 8 tiles become fallbacks."""
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import test_batch_plan as t\n"
            "kinds, passes = t.check_batches(8)\n"
            "assert kinds == {0, 1} and passes > 5, (kinds, passes)\n"
            "print('ok', passes)\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MINEHIP_BATCH_SLOTS="8"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])


def test_fused_and_fallback_boundaries():
    """The sizes the documents name: for "cmu440", [0, 2*10^6] is one generic piece (fused, 782
    tiles) and [0, 3*10^6] plans a fast piece (fallback); a range of exactly one tile, and one
    nonce more."""
    items = minehip.batch_plan([("cmu440", 0, 2 * 10 ** 6), ("cmu440", 0, 3 * 10 ** 6), ("cmu440", 0, 2559),
                                ("cmu440", 0, 2560), ("cmu440", 7, 7), ("", U64 - 5000, U64)])
    got = [(it["req"], it["kind"], it["pass"], it["slot"], it["slots"]) for it in items]
    assert got == [(0, 0, 0, 0, 782), (1, 1, -1, 0, 0), (2, 0, 0, 782, 1), (3, 0, 0, 783, 2), (4, 0, 0, 785, 1),
                   (5, 0, 0, 786, 2)]
    assert any(p["kind"] == 0 for p in minehip.plan("cmu440", 0, 3 * 10 ** 6))


def _reqs(*triples):
    arr = (_lib.mh_request * len(triples))()
    keep = []
    for i, (m, lo, hi) in enumerate(triples):
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper = m, (len(m) if m is not None else 3), lo, hi
    return arr, keep


def test_batch_plan_arguments():
    L = minehip.lib
    assert L.mh_batch_plan(None, 0, None, 0) == 0
    assert minehip.batch_plan([]) == []
    arr, _ = _reqs((b"cmu440", 0, 99), (b"x", 5, 5))
    assert L.mh_batch_plan(None, 2, None, 16) == minehip.MH_EINVAL
    assert L.mh_batch_plan(arr, 2, None, -1) == minehip.MH_EINVAL
    assert L.mh_batch_plan(arr, 2, None, 16) == 2          # counting only
    buf = (_lib.mh_batch_item * 1)()
    assert L.mh_batch_plan(arr, 2, buf, 1) == 2            # cap + 1: truncated, the first written
    assert (buf[0].req, buf[0].first, buf[0].count, buf[0].slots) == (0, 0, 100, 1)
    bad, _ = _reqs((b"cmu440", 0, 99), (b"x", 9, 3))
    assert L.mh_batch_plan(bad, 2, None, 16) == minehip.MH_ERANGE
    null, _ = _reqs((None, 0, 9))
    assert L.mh_batch_plan(null, 1, None, 16) == minehip.MH_EINVAL
    with pytest.raises(minehip.MinehipError) as e:
        minehip.batch_plan([("x", 9, 3)])
    assert e.value.code == minehip.MH_ERANGE


def test_search_batch_arguments_without_a_device():
    L = minehip.lib
    assert L.mh_search_batch(0, None, 0, None) == minehip.MH_OK  # n = 0: no device touched
    assert minehip.search_batch([]) == []
    arr, _ = _reqs((b"cmu440", 0, 99))
    out = (_lib.mh_result * 1)()
    assert L.mh_search_batch(0, None, 1, out) == minehip.MH_EINVAL
    assert L.mh_search_batch(0, arr, 1, None) == minehip.MH_EINVAL
    # every request refused on its own: each has its status, the call is MH_OK, no device needed
    bad, _ = _reqs((b"x", 9, 3), (None, 0, 9), (b"y", U64, 0))
    out = (_lib.mh_result * 3)()
    assert L.mh_search_batch(0, bad, 3, out) == minehip.MH_OK
    assert [o.status for o in out] == [minehip.MH_ERANGE, minehip.MH_EINVAL, minehip.MH_ERANGE]
    res = minehip.search_batch([("x", 9, 3), ("y", 2, 1)], errors="return")
    assert [type(r) for r in res] == [minehip.MinehipError] * 2
    assert [(r.code, r.index) for r in res] == [(minehip.MH_ERANGE, 0), (minehip.MH_ERANGE, 1)]
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_batch([("x", 9, 3)])
    assert e.value.code == minehip.MH_ERANGE and e.value.index == 0 and "request 0" in str(e.value)


def test_search_batch_python_argument_checks():
    with pytest.raises(ValueError):
        minehip.search_batch([("x", 0, 1)], errors="ignore")
    with pytest.raises(ValueError):
        minehip.search_batch([("x", 0)])
    with pytest.raises(ValueError):
        minehip.search_batch([("x", -1, 5)])
    with pytest.raises(ValueError):
        minehip.search_batch([("x", 0, 1 << 64)])
    with pytest.raises(ValueError):
        minehip.batch_plan([("x", 0.5, 3)])
    with pytest.raises(ValueError):
        minehip.miner_handle_batch([b"{}"], errors="ignore")


def test_valid_batch_without_a_device_is_enodev():
    if minehip.device_count() > 0:
        pytest.skip("a device is visible")
    arr, _ = _reqs((b"x", 9, 3), (b"cmu440", 0, 99))
    out = (_lib.mh_result * 2)()
    assert minehip.lib.mh_search_batch(0, arr, 2, out) == minehip.MH_ENODEV
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_batch([("cmu440", 0, 99)], errors="return")  # a device failure is the call's
    assert e.value.code == minehip.MH_ENODEV
    big, _ = _reqs((b"cmu440", 0, 3 * 10 ** 6))  # a fallback alone
    assert minehip.lib.mh_search_batch(0, big, 1, out) == minehip.MH_ENODEV
    with pytest.raises(minehip.MinehipError) as e:
        minehip.miner_handle_batch([minehip.marshal(minehip.NewRequest("cmu440", 0, 99))])
    assert e.value.code == minehip.MH_ENODEV


def test_miner_handle_batch_skips_without_a_device():
    """Payloads a miner skips get mh_miner_handle's own codes, and need no device."""
    payloads = [minehip.marshal(minehip.NewJoin()), b"not json", minehip.marshal(minehip.NewRequest("x", 9, 1))]
    res = minehip.miner_handle_batch(payloads)
    assert [r.code for r in res] == [minehip.MH_ENOTREQ, minehip.MH_ENOTREQ, minehip.MH_ERANGE]
    for p, r in zip(payloads, res):
        with pytest.raises(minehip.MinehipError) as e:
            minehip.miner_handle(p)
        assert e.value.code == r.code
    with pytest.raises(minehip.MinehipError) as e:
        minehip.miner_handle_batch(payloads, errors="raise")
    assert e.value.code == minehip.MH_ENOTREQ and e.value.index == 0
    assert minehip.miner_handle_batch([]) == []
    n = ctypes.c_size_t()
    assert minehip.lib.mh_miner_handle_batch(None, 1, None, None, 1, None, 0, ctypes.byref(n), None) == \
        minehip.MH_EINVAL


def test_struct_layouts():
    assert ctypes.sizeof(_lib.mh_request) == 32 and ctypes.sizeof(_lib.mh_result) == 24
    assert ctypes.sizeof(_lib.mh_batch_item) == 40


def test_planner_under_sanitizers(tmp_path):
    """plan_batch, build_batch_tables and batch_tables_ok (csrc/plan.cpp) under AddressSanitizer and
    UndefinedBehaviorSanitizer, driven by the stand-alone tests/host/batch_plan_host.cpp: random
    batches at random capacities, the tile walk batch_scan does replayed on the host, and tables
    corrupted on purpose, which the check must refuse."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "batch_plan_host")
    csrc = os.path.join(PKG, "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out,
           os.path.join(ROOT, "tests", "host", "batch_plan_host.cpp"), os.path.join(csrc, "plan.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out, "440", "40"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "failures=0" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
