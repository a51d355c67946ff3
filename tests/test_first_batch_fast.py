"""mh_search_first_batch_ex / mh_first_batch_order_ex on the CPU: the ABI surface, the argument
handling up to the device call, the binding, and the host-built dispatch orders of a pass with
fused fast pieces.  No GPU compute is called here.

The orders (include/minehip.h): workgroup b of the pass's generic launch runs the tile
of partial slot order(-1)[b]; workgroup b of batch_first launch l runs the chunk of partial slot
order(l)[b].  Rank-major means chunk k of every item of the launch that has k + 1 chunks, for
k = 0, 1, ..., in item order within a rank; likewise tile k of every request."""
import ctypes
import os

import pytest

import minehip
from minehip import _lib
from conftest import run_dev
from test_gpu_batch_fast import EXTRA, SHAPES
from test_gpu_parity import env

U64 = (1 << 64) - 1
FUSE = minehip.MH_BATCH_FUSE_FAST
MIXED = SHAPES + EXTRA     # every layout class, generic-only requests, two messages of one layout


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mh_search_first_batch_ex", "mh_first_batch_order_ex"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    for name in ("mh_batch_first_co_begin", "mh_batch_first_co_end"):
        assert hasattr(raw, name), name
    fn = minehip.lib.mh_search_first_batch_ex
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 5 and fn.argtypes[3] is ctypes.c_uint32
    assert fn.argtypes[1]._type_ is _lib.mh_first_request and fn.argtypes[4]._type_ is _lib.mh_first_result
    fo = minehip.lib.mh_first_batch_order_ex
    assert fo.restype is ctypes.c_int64 and len(fo.argtypes) == 7
    assert fo.argtypes[0]._type_ is _lib.mh_request and fo.argtypes[2] is ctypes.c_uint32
    assert fo.argtypes[3] is ctypes.c_int32 and fo.argtypes[4] is ctypes.c_int32
    assert fo.argtypes[5]._type_ is ctypes.c_uint32
    assert ctypes.sizeof(_lib.mh_first_request) == 40 and ctypes.sizeof(_lib.mh_first_result) == 32
    assert minehip.lib.mh_abi_version() == 5      # additive: no existing struct changed
    from minehip import codeobj
    assert callable(codeobj.batch_first_code_object) and callable(codeobj.batch_first_kernel_resources)
    assert codeobj.batch_first_code_object()[:4] == b"\x7fELF"


def _reqs(*quads):
    arr = (_lib.mh_first_request * len(quads))()
    keep = []
    for i, (m, lo, hi, T) in enumerate(quads):
        keep.append(m)
        arr[i].msg, arr[i].len, arr[i].lower, arr[i].upper, arr[i].target = m, (len(m) if m is not None else 3), lo, hi, T
    return arr, keep


def test_arguments_without_a_device():
    L = minehip.lib
    arr, _ = _reqs((b"cmu440", 0, 99, 7))
    out = (_lib.mh_first_result * 1)()
    for flags in (2, 3, 1 << 31, 0xFFFFFFFE):                      # an unknown bit, with or without the known one
        assert L.mh_search_first_batch_ex(0, arr, 1, flags, out) == minehip.MH_EINVAL
        assert b"unknown flag" in L.mh_last_error()
        assert L.mh_search_first_batch_ex(0, None, 0, flags, None) == minehip.MH_EINVAL   # before n == 0
    for flags in (0, FUSE):
        assert L.mh_search_first_batch_ex(0, None, 0, flags, None) == minehip.MH_OK       # n = 0: no device touched
        assert L.mh_search_first_batch_ex(0, None, 1, flags, out) == minehip.MH_EINVAL
        assert b"NULL" in L.mh_last_error()
        assert L.mh_search_first_batch_ex(0, arr, 1, flags, None) == minehip.MH_EINVAL
        # every request refused on its own: each has its status, the call is MH_OK, no device needed
        big = b"y" * ((1 << 20) + 1)
        bad, _ = _reqs((b"x", 9, 3, 5), (None, 0, 9, 5), (big, 0, 4, 5), (b"y", U64, 0, U64))
        res = (_lib.mh_first_result * 4)()
        assert L.mh_search_first_batch_ex(0, bad, 4, flags, res) == minehip.MH_OK
        assert [o.status for o in res] == [minehip.MH_ERANGE, minehip.MH_EINVAL, minehip.MH_ETOOLONG, minehip.MH_ERANGE]
    assert minehip.search_first_batch([], fuse_fast=True) == []
    res = minehip.search_first_batch([("x", 9, 3, 1), ("y", 2, 1, 1)], errors="return", fuse_fast=True)
    assert [(r.code, r.index) for r in res] == [(minehip.MH_ERANGE, 0), (minehip.MH_ERANGE, 1)]
    with pytest.raises(minehip.MinehipError) as e:
        minehip.search_first_batch([("x", 9, 3, 1)], fuse_fast=True)
    assert e.value.code == minehip.MH_ERANGE and e.value.index == 0
    if minehip.device_count() == 0:                # no CPU fallback: fused and fallback requests alike
        for r in (("cmu440", 0, 99, U64), ("cmu440", 0, 3 * 10 ** 6, U64), ("cmu440", 0, 2 * 10 ** 9, U64)):
            with pytest.raises(minehip.MinehipError) as e:
                minehip.search_first_batch([r], errors="return", fuse_fast=True)
            assert e.value.code == minehip.MH_ENODEV


def launches_of(plan, p):
    """{launch: [fast pieces in chunk order]} of pass p of a batch_plan_ex plan."""
    out = {}
    for it in plan:
        if it["kind"] == 2 and it["pass"] == p:
            out.setdefault(it["launch"], []).append(it)
    # inside a launch the pieces are ordered longest lanes first, then request order
    return {l: sorted(v, key=lambda it: (-it["lo_digits"], it["req"], it["first"])) for l, v in out.items()}


def check_orders(reqs, rank_major=True):
    """Every pass and every launch of the plan: the order is a permutation of exactly that launch's
    slots; rank-major, chunk k of an item precedes its chunk k + 1, ranks never decrease along the
    order and all chunks 0 come first; otherwise it is the identity in launch order.  Returns
    (passes, fast launches, slots)."""
    plan = minehip.batch_plan_ex(reqs)
    fused = [it for it in plan if it["kind"] != 1]
    passes = 1 + max(it["pass"] for it in fused)
    n_launches = total = 0
    for p in range(passes):
        tiles = [it for it in fused if it["pass"] == p and it["kind"] == 0]
        order = minehip.first_batch_order(reqs, p, fuse_fast=True)
        tile_slots = [s for it in tiles for s in range(it["slot"], it["slot"] + it["slots"])]
        assert sorted(order) == sorted(tile_slots), p
        rank, seen = {}, {}
        for it in tiles:                              # a request's tiles across its entries, in nonce order
            for s in range(it["slot"], it["slot"] + it["slots"]):
                rank[s] = seen[it["req"]] = seen.get(it["req"], -1) + 1
        if rank_major:
            assert [rank[s] for s in order] == sorted(rank[s] for s in order), p
            last = {}
            for s in order:
                r = next(it["req"] for it in tiles if it["slot"] <= s < it["slot"] + it["slots"])
                assert last.get(r, -1) < s
                last[r] = s
        else:
            assert order == tile_slots, p
        total += len(order)
        launches = launches_of(plan, p)
        assert sorted(launches) == list(range(len(launches)))
        for l, items in launches.items():
            order = minehip.first_batch_order(reqs, p, fuse_fast=True, launch=l)
            slots = [s for it in items for s in range(it["slot"], it["slot"] + it["slots"])]
            assert sorted(order) == sorted(slots) and len(set(order)) == len(order), (p, l)
            rank = {s: s - it["slot"] for it in items for s in range(it["slot"], it["slot"] + it["slots"])}
            if rank_major:
                ranks = [rank[s] for s in order]
                assert ranks == sorted(ranks), (p, l)                       # chunk k before chunk k + 1
                assert set(order[:len(items)]) == {it["slot"] for it in items}   # all chunks 0 come first
                assert order[:len(items)] == [it["slot"] for it in items]        # ... in item order
            else:
                assert order == slots, (p, l)
            total += len(order)
            n_launches += 1
        with pytest.raises(minehip.MinehipError) as e:                       # a launch the plan lacks
            minehip.first_batch_order(reqs, p, fuse_fast=True, launch=len(launches))
        assert e.value.code == minehip.MH_EINVAL
    with pytest.raises(minehip.MinehipError) as e:
        minehip.first_batch_order(reqs, passes, fuse_fast=True)
    assert e.value.code == minehip.MH_EINVAL
    return passes, n_launches, total


def test_orders_of_a_mixed_call():
    passes, launches, slots = check_orders(MIXED)
    plan = minehip.batch_plan_ex(MIXED)
    assert passes == 1 and launches == 5 and slots == sum(it["slots"] for it in plan)
    # two messages and two ranges of <3, One> share launch 0: four items, their chunks 0 first
    assert len(launches_of(plan, 0)[0]) == 4
    with env(MINEHIP_FIRST_BATCH_ORDER="request"):
        assert check_orders(MIXED, rank_major=False) == (passes, launches, slots)
    with env(MINEHIP_LOWER_DIGITS=3, MINEHIP_MIN_LANES=16):
        check_orders(MIXED)
    with env(MINEHIP_BATCH_SLOTS=1000):
        p2, l2, _ = check_orders(MIXED)
        assert p2 >= 2 and l2 >= 2


def test_order_of_one_piece_and_of_generic_requests():
    # 450 chunks and one tile: the tile's slot is 450
    one = [(b"cmu441", 1_048_000, 2_200_000)]
    assert minehip.first_batch_order(one, fuse_fast=True) == [450]
    assert minehip.first_batch_order(one, fuse_fast=True, launch=0) == list(range(450))
    # the same request three times: chunk 0 of each item, then chunk 1 of each, ...
    order = minehip.first_batch_order(one * 3, fuse_fast=True, launch=0)
    assert order[:7] == [0, 451, 902, 1, 452, 903, 2] and sorted(order) == sorted(
        s for b in (0, 451, 902) for s in range(b, b + 450))
    assert minehip.first_batch_order(one * 3, fuse_fast=True) == [450, 901, 1352]
    # generic-only requests: the pass has no fast launch, and its order is mh_first_batch_order's
    from test_gpu_batch import EDGES
    reqs = EDGES[-3:]
    assert minehip.first_batch_order(reqs, fuse_fast=True) == minehip.first_batch_order(reqs) == [0, 1, 3, 2, 4]
    with pytest.raises(minehip.MinehipError):
        minehip.first_batch_order(reqs, fuse_fast=True, launch=0)


def test_flag_zero_is_first_batch_order():
    from test_gpu_batch import fuzz_requests
    reqs = fuzz_requests()[:60]
    assert minehip.first_batch_order(reqs, flags=0) == minehip.first_batch_order(reqs)
    L = minehip.lib
    arr, _ = minehip._requests([(b"tile", 0, 2560), (b"tile", 0, 2559)])
    buf = (ctypes.c_uint32 * 2)()
    assert L.mh_first_batch_order_ex(arr, 2, 0, 0, -1, None, 16) == 3            # counting only
    assert L.mh_first_batch_order_ex(arr, 2, FUSE, 0, -1, None, 16) == 3
    assert L.mh_first_batch_order_ex(arr, 2, FUSE, 0, -1, buf, 2) == 3           # cap + 1: the first cap written
    assert list(buf) == [0, 2]
    assert L.mh_first_batch_order_ex(arr, 2, 0, 0, 0, None, 16) == minehip.MH_EINVAL      # flags 0 has no fast launch
    assert L.mh_first_batch_order_ex(arr, 2, FUSE, 0, 0, None, 16) == minehip.MH_EINVAL   # nor has this plan
    assert L.mh_first_batch_order_ex(arr, 2, FUSE, 0, -2, None, 16) == minehip.MH_EINVAL
    assert L.mh_first_batch_order_ex(arr, 2, FUSE, 1, -1, None, 16) == minehip.MH_EINVAL  # no such pass
    assert L.mh_first_batch_order_ex(arr, 2, 2, 0, -1, None, 16) == minehip.MH_EINVAL     # unknown flag
    assert L.mh_first_batch_order_ex(arr, 2, FUSE, 0, -1, None, -1) == minehip.MH_EINVAL
    assert L.mh_first_batch_order_ex(None, 2, FUSE, 0, -1, None, 16) == minehip.MH_EINVAL
    bad, _ = minehip._requests([(b"cmu440", 0, 99), (b"x", 9, 3)])
    assert L.mh_first_batch_order_ex(bad, 2, FUSE, 0, -1, None, 16) == minehip.MH_ERANGE
    with pytest.raises(minehip.MinehipError) as e:      # larger than the cap: a fallback alone, no pass at all
        minehip.first_batch_order([("cmu440", 0, 2 * 10 ** 9)], fuse_fast=True)
    assert e.value.code == minehip.MH_EINVAL


def test_dev_build_refuses_the_hash_hooks():
    """As mh_search_first_batch: with a hash or code-object hook set the dev build fails with
    MH_EINVAL before it touches a device, instead of silently ignoring the hook."""
    r = run_dev("""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
for k, v in (("MINEHIP_DEV_HASH_KEEP", "2,0"), ("MINEHIP_DEV_HASH_XOR", "1f"),
             ("MINEHIP_DEV_CODE_OBJECT", "build/fast_search_keep.hsaco")):
    os.environ[k] = v
    try:
        minehip.search_first_batch([(b"cmu440", 0, 3000000, 5)], fuse_fast=True)
        raise SystemExit("searched with " + k)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and k in str(e), e
    del os.environ[k]
print("refused")
""", timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "refused", r.stderr[-2000:] + r.stdout[-500:]
