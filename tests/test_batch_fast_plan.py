"""CPU tests of the batched search with fused fast pieces (mh_search_batch_ex / mh_batch_plan_ex
with MH_BATCH_FUSE_FAST): the host plan that packs generic entries and fast pieces of many requests
into passes, and the argument behaviour of the entry points up to the device call.  No GPU compute.

The rules (include/minehip.h): a generic entry takes one slot per tile of 256 aligned
decades, a fast piece one slot per chunk of 256 runs of 10^L nonces; a fused request's pieces fill
one contiguous slot segment in nonce order; the fast pieces of one layout of a pass share a launch,
ordered by L descending, then request order.  Lanes: every request keeps its own plan's; with
MINEHIP_BATCH_FAST_LANES=shared the requests of the call whose own plan holds a fast piece (and
which pass the size cap) are planned with min_lanes = min(m, max(256, pow2floor(m / k))) for k >= 2
of them, m = MINEHIP_MIN_LANES (2^19)."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

import minehip
from minehip import _lib
from conftest import ROOT, PKG

U64 = (1 << 64) - 1
TILE_DECADES = 256
CHUNK_RUNS = 256
MAX_SLOTS = 1 << 18        # kMaxBlocksPerLaunch: the partials buffer
MAX_REQUESTS = 4096        # kBatchMaxRequests
MAX_FAST_ITEMS = 1024      # kBatchMaxFastItems
MIN_LANES = 1 << 19        # PlanOpts::min_lanes

# the shapes of tests/test_gpu_batch_fast.py: the smallest ranges that still plan a fast piece
SHAPES = [
    ("cmu440", 1_048_000, 2_200_000),
    ("cmu440", 0, 3_000_000),
    ("a" * 51, 0, 3_000_000),
    ("a" * 60, 0, 3_000_000),
    ("a" * 47, 900_000, 3_000_000),
    ("cmu440", 5 * 10 ** 8, 5 * 10 ** 8 + 3 * 10 ** 6),
    ("cmu440", U64 - 3 * 10 ** 6, U64),
]


def tiles_of(first, count):
    last = first + count - 1
    return -(-(last // 10 - first // 10 + 1) // TILE_DECADES)


def shared_min_lanes(m, k):
    if k < 2:
        return m
    share, p = m // k, 1
    while p <= share // 2:
        p *= 2
    return min(m, max(p, CHUNK_RUNS))


def own_plan(req, monkeypatch, min_lanes=None):
    if min_lanes is not None:
        monkeypatch.setenv("MINEHIP_MIN_LANES", str(min_lanes))
    try:
        return minehip.plan(*req)
    finally:
        if min_lanes is not None:
            monkeypatch.delenv("MINEHIP_MIN_LANES")


def check_plan(reqs, monkeypatch, cap=MAX_SLOTS, max_nonces=minehip.MH_BATCH_FAST_MAX_NONCES, min_lanes=MIN_LANES,
               shared=False):
    """Every property of one fused-fast plan (shared: under the batch-aware lane rule); returns it."""
    if shared:
        monkeypatch.setenv("MINEHIP_BATCH_FAST_LANES", "shared")
    try:
        pieces = minehip.batch_plan_ex(reqs)
    finally:
        if shared:
            monkeypatch.delenv("MINEHIP_BATCH_FAST_LANES")
    by_req = {}
    for p in pieces:
        by_req.setdefault(p["req"], []).append(p)
    assert sorted(by_req) == list(range(len(reqs)))
    assert [p["req"] for p in pieces] == sorted(p["req"] for p in pieces)  # request order
    own = [minehip.plan(*r) for r in reqs]
    cand = [any(p["kind"] == 0 for p in own[i]) and reqs[i][2] - reqs[i][1] + 1 <= max_nonces
            for i in range(len(reqs))]
    lanes = shared_min_lanes(min_lanes, sum(cand)) if shared else min_lanes
    cur_pass, used, in_pass, fast_in_pass = 0, 0, 0, 0
    launches = {}   # (pass, launch) -> [(piece, position in the plan)]
    for i, (msg, lo, hi) in enumerate(reqs):
        mine = by_req[i]
        want = own_plan(reqs[i], monkeypatch, lanes) if cand[i] and lanes != min_lanes else own[i]
        slots = sum(tiles_of(p["first"], p["count"]) if p["kind"] == 1
                    else -(-(p["count"] // 10 ** p["lo_digits"]) // CHUNK_RUNS) for p in want)
        has_fast = any(p["kind"] == 0 for p in want)
        n_fast = sum(p["kind"] == 0 for p in want)
        if mine[0]["kind"] == 1:  # fallback: one piece, no slots; over the size cap or more than a pass holds
            assert len(mine) == 1
            p = mine[0]
            assert (p["first"], p["count"], p["pass"], p["slot"], p["slots"], p["launch"]) == \
                (lo, (hi - lo + 1) & U64, -1, 0, 0, -1)
            assert (has_fast and not cand[i]) or slots > cap or n_fast > MAX_FAST_ITEMS, (i, lo, hi, cap)
            continue
        assert slots <= cap and (cand[i] or not has_fast)
        # one piece per piece of the documented plan, tiling [lo, hi] exactly once and in nonce order
        assert [(p["first"], p["count"], p["kind"]) for p in mine] == \
            [(q["first"], q["count"], 2 if q["kind"] == 0 else 0) for q in want]
        nxt = lo
        for p, q in zip(mine, want):
            assert p["first"] == nxt and p["count"] >= 1
            nxt = p["first"] + p["count"]
            if p["kind"] == 0:
                assert p["slots"] == tiles_of(p["first"], p["count"])
                assert (p["word"], p["mode"], p["lo_digits"], p["launch"]) == (0, 0, 0, -1)
            else:  # L, J and MODE as the documented rule plans them
                assert (p["word"], p["mode"], p["lo_digits"]) == (q["word"], q["mode"], q["lo_digits"])
                assert p["count"] % 10 ** p["lo_digits"] == 0
                assert p["slots"] == -(-(p["count"] // 10 ** p["lo_digits"]) // CHUNK_RUNS) and p["launch"] >= 0
        assert nxt - 1 == hi
        # its slot segment: contiguous, in nonce order, after the previous request's of the same pass
        ps = mine[0]["pass"]
        assert all(p["pass"] == ps for p in mine) and ps in (cur_pass, cur_pass + 1)
        if ps != cur_pass:  # a new pass only because the request did not fit the old one
            assert used + slots > cap or in_pass == MAX_REQUESTS or fast_in_pass + n_fast > MAX_FAST_ITEMS
            cur_pass, used, in_pass, fast_in_pass = ps, 0, 0, 0
        for p in mine:
            assert p["slot"] == used
            used += p["slots"]
            if p["kind"] == 2:
                launches.setdefault((ps, p["launch"]), []).append(p)
        in_pass += 1
        fast_in_pass += n_fast
        assert used <= cap and in_pass <= MAX_REQUESTS and fast_in_pass <= MAX_FAST_ITEMS
    # launches: one per layout of a pass, numbered from 0 in order of first appearance
    by_pass = {}
    for (ps, l), ps_pieces in launches.items():
        assert len({(p["word"], p["mode"]) for p in ps_pieces}) == 1
        by_pass.setdefault(ps, {})[l] = (ps_pieces[0]["word"], ps_pieces[0]["mode"])
    for ps, ls in by_pass.items():
        assert sorted(ls) == list(range(len(ls))) and len(set(ls.values())) == len(ls)
        firsts = [min(k for k, p in enumerate(pieces) if p["pass"] == ps and p["launch"] == l) for l in sorted(ls)]
        assert firsts == sorted(firsts)
    return pieces


def test_exports_and_struct():
    raw = ctypes.CDLL(_lib.PRODUCT_LIB_PATH)
    for name in ("mh_search_batch_ex", "mh_batch_plan_ex"):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
    assert ctypes.sizeof(_lib.mh_batch_piece) == 56
    assert minehip.MH_BATCH_FUSE_FAST == 1


def test_shapes_plan_as_documented(monkeypatch):
    pieces = check_plan(SHAPES, monkeypatch)
    fast = [p for p in pieces if p["kind"] == 2]
    assert not [p for p in pieces if p["kind"] == 1] and {p["pass"] for p in pieces} == {0}
    assert [(p["req"], p["word"], p["mode"]) for p in fast] == \
        [(0, 3, 0), (1, 3, 0), (2, 13, 5), (3, 0, 1), (4, 13, 0), (5, 3, 0), (6, 6, 0)]
    # 115,200 runs are 450 chunks exactly; 200,000 runs are 781 chunks and a last one of 64 lanes
    assert (fast[0]["count"], fast[0]["lo_digits"], fast[0]["slots"]) == (1_152_000, 1, 450)
    assert (fast[1]["count"], fast[1]["lo_digits"], fast[1]["slots"]) == (2_000_000, 1, 782)
    assert fast[6]["first"] + fast[6]["count"] + 5 == U64  # up to the last whole run below 2^64
    # <3, One> of three requests shares launch 0; the other layouts follow in order of appearance
    assert [p["launch"] for p in fast] == [0, 0, 1, 2, 3, 0, 4]


def test_flags_zero_is_batch_plan():
    rng = random.Random(440)
    reqs = SHAPES + [("m%d" % i, rng.randrange(0, 10 ** 6), 10 ** 6 + rng.randrange(0, 10 ** 6)) for i in range(40)]
    old = minehip.batch_plan(reqs)
    new = minehip.batch_plan_ex(reqs, fuse_fast=False)
    assert new == [dict(it, word=0, mode=0, lo_digits=0, launch=-1) for it in old]
    assert {it["kind"] for it in old} == {0, 1}
    # and the old plan still sends [0, 3 * 10^6] to the fallback path
    assert [it["kind"] for it in minehip.batch_plan([("cmu440", 0, 3_000_000)])] == [1]


def test_unknown_flags_are_refused():
    arr, keep = minehip._requests([("cmu440", 0, 10)])
    out = (_lib.mh_result * 1)()
    buf = (_lib.mh_batch_piece * 4)()
    for flags in (2, 3, 1 << 31):
        assert _lib.lib.mh_batch_plan_ex(arr, 1, flags, buf, 4) == _lib.MH_EINVAL
        assert _lib.lib.mh_search_batch_ex(0, arr, 1, flags, out) == _lib.MH_EINVAL  # before any device call
    with pytest.raises(minehip.MinehipError) as e:
        minehip.batch_plan_ex([("cmu440", 0, 10)], flags=4)
    assert e.value.code == _lib.MH_EINVAL
    assert _lib.lib.mh_batch_plan_ex(arr, 0, 1, buf, 4) == 0
    assert _lib.lib.mh_search_batch_ex(0, arr, 0, 1, out) == _lib.MH_OK  # n == 0 touches no device
    assert _lib.lib.mh_search_batch_ex(0, None, 1, 1, out) == _lib.MH_EINVAL
    # per-request refusals are the plan call's return code, as mh_batch_plan's
    with pytest.raises(minehip.MinehipError) as e:
        minehip.batch_plan_ex([("cmu440", 0, 10), ("cmu440", 5, 4)])
    assert e.value.code == _lib.MH_ERANGE
    assert _lib.lib.mh_batch_plan_ex(arr, 1, 1, buf, 0) == 1  # cap + 1: truncated


def test_lanes_follow_the_rule(monkeypatch):
    # by default every request keeps its own plan's lanes, alone or among 64
    one = check_plan([("cmu440", 0, 10 ** 7)], monkeypatch)
    assert [p["lo_digits"] for p in one if p["kind"] == 2] == \
        [p["lo_digits"] for p in minehip.plan("cmu440", 0, 10 ** 7) if p["kind"] == 0] == [1]
    reqs64 = [("m%d" % i, 0, 10 ** 7) for i in range(64)]
    many = check_plan(reqs64, monkeypatch)
    fast = [p for p in many if p["kind"] == 2]
    assert len(fast) == 64 and {(p["lo_digits"], p["count"], p["slots"]) for p in fast} == {(1, 9_000_000, 3516)}
    assert sum(p["slots"] for p in many) <= MAX_SLOTS and {p["pass"] for p in many} == {0}
    # the batch-aware rule: one request alone is unchanged, 64 share 2^19 lanes: 2^13 each, so L = 3
    assert check_plan([("cmu440", 0, 10 ** 7)], monkeypatch, shared=True) == one
    fast = [p for p in check_plan(reqs64, monkeypatch, shared=True) if p["kind"] == 2]
    assert len(fast) == 64 and {(p["lo_digits"], p["count"], p["slots"]) for p in fast} == {(3, 9_000_000, 36)}
    assert shared_min_lanes(MIN_LANES, 64) == 1 << 13 and shared_min_lanes(MIN_LANES, 3) == 1 << 17
    assert shared_min_lanes(MIN_LANES, 10 ** 6) == 256 and shared_min_lanes(100, 8) == 100
    # generic-only requests do not count: two fast requests among 30 small ones share 2^18 each
    mixed = [("s%d" % i, 0, 50_000) for i in range(30)] + [("cmu440", 0, 4 * 10 ** 8), ("x", 0, 4 * 10 ** 8)]
    check_plan(mixed, monkeypatch, shared=True)
    check_plan(mixed, monkeypatch)
    check_plan(SHAPES, monkeypatch, shared=True)
    # the planning variables keep their meaning
    monkeypatch.setenv("MINEHIP_LOWER_DIGITS", "2")
    monkeypatch.setenv("MINEHIP_MIN_LANES", "16")
    assert {p["lo_digits"] for p in minehip.batch_plan_ex(reqs64) if p["kind"] == 2} == {2}
    monkeypatch.setenv("MINEHIP_LOWER_DIGITS", "3")
    small = [p for p in check_plan(SHAPES, monkeypatch, min_lanes=16) if p["req"] == 1]
    # [0, 3 * 10^6] at L = 3: 2,000 runs, 7.8 chunks
    assert (small[0]["kind"], small[1]["lo_digits"], small[1]["count"], small[1]["slots"]) == (0, 3, 2_000_000, 8)
    monkeypatch.setenv("MINEHIP_EARLY", "0")
    assert not [p for p in check_plan(SHAPES, monkeypatch, min_lanes=16) if p["mode"] >= 3]
    monkeypatch.setenv("MINEHIP_GENERIC_BELOW", str(10 ** 7))
    assert {p["kind"] for p in minehip.batch_plan_ex(SHAPES[:5])} == {0}


def test_size_cap(monkeypatch):
    reqs = [("cmu440", 0, 10 ** 7), ("x", 0, 2 * 10 ** 7), ("y", 0, 1000)]
    monkeypatch.setenv("MINEHIP_BATCH_FAST_MAX", str(10 ** 7 + 1))
    pieces = check_plan(reqs, monkeypatch, max_nonces=10 ** 7 + 1)
    assert [p["kind"] for p in pieces if p["req"] == 1] == [1] and {p["kind"] for p in pieces if p["req"] == 0} == {0, 2}
    monkeypatch.setenv("MINEHIP_BATCH_FAST_MAX", str(10 ** 7))
    assert [p["kind"] for p in minehip.batch_plan_ex(reqs)] == [1, 1, 0]
    monkeypatch.delenv("MINEHIP_BATCH_FAST_MAX")
    assert minehip.MH_BATCH_FAST_MAX_NONCES == 10 ** 9   # at most 10^9 nonces: [0, 10^9 - 1] is fused
    big = minehip.batch_plan_ex([("cmu440", 0, 10 ** 9 - 1), ("cmu440", 0, 10 ** 9), ("cmu440", 0, U64)])
    assert [p["kind"] for p in big if p["req"] == 1] == [1] and [p["kind"] for p in big if p["req"] == 2] == [1]
    assert 2 in {p["kind"] for p in big if p["req"] == 0}


@pytest.mark.parametrize("cap", [3000, 500])
def test_capacity_fallbacks_and_passes(monkeypatch, cap):
    """MINEHIP_BATCH_SLOTS lowers the slots of a pass: more passes, and a request whose tiles and
    chunks exceed one pass falls back."""
    monkeypatch.setenv("MINEHIP_BATCH_SLOTS", str(cap))
    reqs = SHAPES + [("g%d" % i, 0, 200_000) for i in range(5)]
    pieces = check_plan(reqs, monkeypatch, cap=cap)
    assert max(p["pass"] for p in pieces) >= 1
    kinds = {p["req"]: p["kind"] for p in pieces}
    if cap == 500:  # only the 450-chunk request and the small ones fit
        assert [r for r in range(7) if kinds[r] != 1] == [0]
    else:
        assert 1 not in kinds.values()


def test_seeded_fuzz(monkeypatch):
    rng = random.Random(4400)
    seen = set()
    for _ in range(6):
        reqs = []
        for _ in range(rng.randrange(1, 40)):
            msg = bytes(rng.randrange(1, 256) for _ in range(rng.randrange(0, 131)))
            d = rng.randrange(1, 21)
            lo = rng.randrange(0 if d == 1 else 10 ** (d - 1), min(U64, 10 ** d - 1) + 1)
            hi = min(U64, lo + rng.choice((rng.randrange(1, 6 * 10 ** 6), rng.randrange(1, 3001), 1,
                                           rng.randrange(10 ** 6, 4 * 10 ** 8))) - 1)
            reqs.append((msg, lo, hi))
        seen |= {p["kind"] for p in check_plan(reqs, monkeypatch)}
    assert seen >= {0, 2}
    monkeypatch.setenv("MINEHIP_BATCH_SLOTS", "1000")  # a piece of 2.56 * 10^6 nonces at L = 1 no longer fits a pass
    rng = random.Random(4401)
    reqs = []
    for i in range(60):
        lo = rng.randrange(0, 2 * 10 ** 6)
        reqs.append((bytes([65 + i % 26]) * rng.randrange(1, 120), lo, lo + rng.randrange(1, 5 * 10 ** 6)))
    for shared in (False, True):
        pieces = check_plan(reqs, monkeypatch, cap=1000, shared=shared)
        assert {p["kind"] for p in pieces} == {0, 1, 2} and max(p["pass"] for p in pieces) >= 2


def test_host_plan_and_table_checks_under_sanitizers(tmp_path):
    """plan_batch_ex, build_batch_tables_ex and batch_tables_ex_ok under AddressSanitizer and
    UndefinedBehaviorSanitizer: the stand-alone tests/host/batch_fast_host.cpp over random batches,
    both lane rules and small capacities, ranges at the top of u64 included, and tables corrupted
    on purpose."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path / "batch_fast_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-Wall", "-o", out,
           os.path.join(ROOT, "tests", "host", "batch_fast_host.cpp"), os.path.join(PKG, "csrc", "plan.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out, "440", "40"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "failures=0" in r.stdout and "items=0" not in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
