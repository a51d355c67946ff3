"""mh_search_hits_batch on the GPU: every hit of many small Requests, fused into passes of
batch_scan_hits (batch_scan with an append of every hit through a per-request cursor into the
request's region of the device hit buffer) and merge_segments_hits, the others through the
mh_search_hits path.  Bit-exact: every expected value comes from test_hits.hits_ref (the oracle's
hashes of the whole range, in numpy), and every result is also what minehip.search_hits gives for
the same request, its minimum what minehip.search gives.

Every case first asserts from the reference alone that it is live -- how many nonces qualify and
where they lie -- before it looks at the GPU."""
import json
import os
import random
import subprocess
import sys

import pytest

from conftest import PKG, ROOT
from test_first import hits_of, kth_smallest_hash
from test_gpu_batch import EDGES, TILE, capacity_requests, fuzz_requests
from test_gpu_parity import env
from test_hits import hits_ref

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CMU = (b"cmu440", 0, 1_999_999)
CMU_MIN = (1228377698034, 1_067_492)          # the range's minimum (tests/test_gpu_hits.py)
CMU_HITS = {6: 4, 5: 17, 4: 192, 3: 2_003}    # target 2^64 // 10^k: hits of the range
CMU_K6 = [393_322, 1_067_492, 1_456_236, 1_999_610]


def T10(k):
    return 2 ** 64 // 10 ** k


def with_cap(r, cap):
    return tuple(r) if len(r) == 5 else tuple(r) + (cap,)


def check(gpu, reqs, cap=4096, got=None):
    """search_hits_batch(reqs, cap) against the reference, against search_hits() of every request,
    and every minimum against search()."""
    if got is None:
        got = gpu.search_hits_batch(reqs, cap)
    assert len(got) == len(reqs)
    for i, (r, g) in enumerate(zip(reqs, got)):
        msg, lo, hi, T, c = with_cap(r, cap)
        exp = hits_ref(msg, lo, hi, T, c)
        assert g == exp, (i, msg[:8], len(msg), lo, hi, T, c, g[0], g[1][:3], g[2], exp[0], exp[1][:3], exp[2])
        assert g == gpu.search_hits(msg, lo, hi, T, c), (i, msg[:8], lo, hi, T, c)
        assert g[2] == gpu.search(msg, lo, hi), (i, g[2])
        assert all(a[0] < b[0] for a, b in zip(g[1], g[1][1:]))          # strictly increasing nonces
    return got


def test_edges_in_one_call(gpu):
    assert (b"cmu440", 0, 0) in EDGES and (b"cmu440", 9, 10) in EDGES and (b"cmu440", U64 - 5000, U64) in EDGES
    assert [r[2] - r[1] + 1 for r in EDGES[-3:]] == [TILE, TILE + 1, TILE]
    reqs = []
    for msg, lo, hi in EDGES:
        size = hi - lo + 1
        mn = kth_smallest_hash(msg, lo, hi, 1)
        targets = [mn, mn - 1, U64, 0]
        assert mn > 0 and hits_ref(msg, lo, hi, mn, 16)[0] == 1 and hits_ref(msg, lo, hi, mn - 1, 16)[:2] == (0, [])
        every = hits_ref(msg, lo, hi, U64, 16)
        assert every[0] == size and [n for n, _ in every[1]] == list(range(lo, lo + min(16, size)))
        assert hits_ref(msg, lo, hi, 0, 16)[:2] == (0, [])
        if size >= 3:
            T3 = kth_smallest_hash(msg, lo, hi, 3)
            assert hits_ref(msg, lo, hi, T3, 16)[0] == 3
            targets.insert(2, T3)
        reqs += [(msg, lo, hi, T) for T in targets]
    assert len(reqs) == 5 * len(EDGES) - 4          # [0, 0], 7, 9..10 and 2^64 - 1 have fewer than 3 nonces
    regs = gpu.hits_batch_regions(reqs, 16)
    assert all((g["kind"], g["pass"], g["window"]) == (0, 0, 0) for g in regs)     # all fused, one pass, one window
    check(gpu, reqs, 16)


def test_one_message_many_targets(gpu):
    msg, lo, hi = CMU
    reqs = [(msg, lo, hi, T10(k)) for k in (6, 5, 4, 3)]
    reqs += [(msg, lo, hi, CMU_MIN[0]), (msg, lo, hi, CMU_MIN[0] - 1), (msg, lo, hi, 0), (msg, lo, hi, T10(3), 0)]
    exp = [hits_ref(*with_cap(r, 4096)) for r in reqs]
    assert [e[0] for e in exp[:4]] == [CMU_HITS[k] for k in (6, 5, 4, 3)] == [len(e[1]) for e in exp[:4]]
    assert [n for n, _ in exp[0][1]] == CMU_K6 and all(e[2] == CMU_MIN for e in exp)
    assert exp[4] == (1, [(CMU_MIN[1], CMU_MIN[0])], CMU_MIN)
    assert exp[5] == (0, [], CMU_MIN) == exp[6] and exp[7] == (2_003, [], CMU_MIN)     # cap 0: the count alone
    regs = gpu.hits_batch_regions(reqs)
    assert all((g["kind"], g["pass"], g["window"]) == (0, 0, 0) for g in regs)
    # one message and range, yet a cursor and a region per request
    assert [(g["offset"], g["slots"]) for g in regs] == [(4096 * i, 4096) for i in range(7)] + [(4096 * 7, 0)]
    assert check(gpu, reqs) == exp


def truncation_requests():
    msg, lo, hi = CMU
    return [(b"abc", 0, 999, kth_smallest_hash(b"abc", 0, 999, 2), 16),
            (msg, 0, 3_000, T10(3), 3),
            (msg, 2_000, 9_000, T10(3), 16),
            (msg, lo, hi, T10(3), 100),
            (b"x" * 60, 0, 9_999, kth_smallest_hash(b"x" * 60, 0, 9_999, 5), 16),
            (msg, lo, hi, T10(3), 64),
            (b"tile", 5, TILE + 4, U64, 4_096)]


TRUNCATED = (1, 3, 5)


def test_truncation_and_rebuild(gpu):
    reqs = truncation_requests()
    full = hits_ref(*CMU, T10(3), 1 << 20)
    small = hits_ref(b"cmu440", 0, 3_000, T10(3), 3)
    assert [n for n, _ in small[1]] == [1_081, 1_329, 2_080] and small[0] > 3          # more qualify than the cap
    assert full[0] == 2_003 and full[1][99][0] == 122_839
    for i in range(len(reqs)):                       # the truncated ones drop entries, the neighbours none
        r = reqs[i]
        assert (hits_ref(*r[:4], 1 << 20)[0] > r[4]) == (i in TRUNCATED), i
        assert hits_ref(*r[:4], 1 << 20)[0] > 0
    regs = gpu.hits_batch_regions(reqs)
    assert all(g["kind"] == 0 and g["slots"] == min(r[4], r[2] - r[1] + 1) for g, r in zip(regs, reqs))
    got = check(gpu, reqs)
    assert got[3][1] == full[1][:100] and got[5][1] == full[1][:64] and got[1][1] == small[1]
    assert got[3][0] == got[5][0] == 2_003
    neighbours = [r for i, r in enumerate(reqs) if i not in TRUNCATED]
    alone = gpu.search_hits_batch(neighbours)
    assert alone == [g for i, g in enumerate(got) if i not in TRUNCATED]


def fuzz_hit_requests():
    """fuzz_requests(seed=440, n=200), each with a target drawn with a fixed seed from: the k-th
    smallest hash of its range for k in {1, 2, 5} (the largest hash where the range has fewer than
    k nonces), the minimum minus 1, 2^64 - 1, and 2^64 // size; and a cap from {0, 1, 4, 4096}."""
    rng = random.Random(4402)
    reqs = []
    for msg, lo, hi in fuzz_requests(seed=440, n=200):
        size = hi - lo + 1
        kind = rng.randrange(6)
        if kind < 3:
            T = kth_smallest_hash(msg, lo, hi, min((1, 2, 5)[kind], size))
        elif kind == 3:
            T = kth_smallest_hash(msg, lo, hi, 1) - 1
        elif kind == 4:
            T = U64
        else:
            T = 2 ** 64 // size
        reqs.append((msg, lo, hi, T, rng.choice((0, 1, 4, 4096))))
    return reqs


def test_fuzz_seed440_one_call(gpu):
    reqs = fuzz_hit_requests()
    exp = [hits_ref(*r) for r in reqs]
    assert sum(1 for e, r in zip(exp, reqs) if e[0] > r[4] > 0) >= 40         # truncated: rebuilt
    assert sum(1 for e in exp if e[0] == 0) >= 20
    assert sum(1 for e, r in zip(exp, reqs) if 0 < e[0] <= r[4]) >= 40        # and lists that fit their region
    assert all(g["kind"] == 0 and g["pass"] == 0 for g in gpu.hits_batch_regions(reqs))
    assert check(gpu, reqs) == exp


@pytest.mark.parametrize("slots,batch_slots", [(1, None), (64, None), (64, 64)])
def test_small_device_buffer(gpu, slots, batch_slots):
    """MINEHIP_HITS_SLOTS (a child process) against the default buffer: the fuzz and the truncation
    case give identical results.  The windows of the device hit buffer advance between passes (a
    drain is what a full table or result buffer forces, too), so with the fuzz's one pass there is
    one window, cut short; MINEHIP_BATCH_SLOTS=64 beside 64 hit slots makes several passes, and
    hits_batch_regions then shows more than one window."""
    fuzz, trunc = fuzz_hit_requests(), truncation_requests()
    default = [gpu.search_hits_batch(fuzz), gpu.search_hits_batch(trunc)]
    assert default[0] == [hits_ref(*r) for r in fuzz] and default[1] == [hits_ref(*r) for r in trunc]
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import json, minehip, test_gpu_hits_batch as t\n"
            "fuzz, trunc = t.fuzz_hit_requests(), t.truncation_requests()\n"
            "regs = minehip.hits_batch_regions(fuzz) + minehip.hits_batch_regions(trunc)\n"
            f"assert all(g['offset'] + g['slots'] <= {slots} for g in regs)\n"
            "windows = 1 + max(g['window'] for g in minehip.hits_batch_regions(fuzz))\n"
            "print(json.dumps([minehip.search_hits_batch(fuzz), minehip.search_hits_batch(trunc), windows]))\n")
    e = dict(os.environ, MINEHIP_HITS_SLOTS=str(slots))
    if batch_slots:
        e["MINEHIP_BATCH_SLOTS"] = str(batch_slots)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    assert child[:2] == json.loads(json.dumps(default))
    assert (child[2] > 1) == bool(batch_slots), child[2]


def test_several_entries_per_request(gpu):
    """MINEHIP_MAX_BLOCKS=16 cuts a request of 30,000 nonces into generic pieces of 4,096: eight
    entries, whose tiles share the request's cursor and region."""
    msg, lo, hi = b"cmu440", 340_000, 369_999
    with env(MINEHIP_MAX_BLOCKS=16):
        plan = gpu.batch_plan([(msg, lo, hi)])
        assert len(plan) >= 3 and all(it["kind"] == 0 and it["count"] <= 4096 for it in plan)
        first_e, last_e = plan[0], plan[-1]
        in_first = lambda n: first_e["first"] <= n < first_e["first"] + first_e["count"]   # noqa: E731
        in_last = lambda n: last_e["first"] <= n <= hi                                      # noqa: E731
        mn = kth_smallest_hash(msg, lo, hi, 1)
        T2 = max(kth_smallest_hash(msg, first_e["first"], first_e["first"] + first_e["count"] - 1, 1), mn)
        hits = hits_of(msg, lo, hi, T2)
        assert len(hits) >= 2 and in_first(hits[0]) and in_last(hits[-1])       # hits in the first and the last entry
        reqs = [(msg, lo, hi, T2), (msg, lo, hi, mn), (msg, lo, hi, mn - 1), (msg, lo, hi, T2, 1)]
        assert all(g["kind"] == 0 and g["pass"] == 0 for g in gpu.hits_batch_regions(reqs, 64))
        got = check(gpu, reqs, 64)
        assert [n for n, _ in got[0][1]] == hits and got[3][1] == got[0][1][:1]


@pytest.mark.parametrize("slots,passes", [(8, 0), (32, 20)])
def test_passes_and_fallback_by_capacity(gpu, slots, passes):
    """MINEHIP_BATCH_SLOTS (a child process) against the default capacity: with 8 slots every
    request is a fallback, with 32 there are 20 passes and one fallback.  The results are the same
    and the reference's."""
    reqs = [(m, lo, hi, kth_smallest_hash(m, lo, hi, 2)) for m, lo, hi in capacity_requests()]
    assert all(hits_ref(*r, 16)[0] == 2 for r in reqs)
    got = check(gpu, reqs, 16)
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import json, minehip\n"
            "reqs = [(bytes.fromhex(m), lo, hi, T) for m, lo, hi, T in json.loads(sys.argv[1])]\n"
            "regs = minehip.hits_batch_regions(reqs, 16)\n"
            f"assert 1 + max(g['pass'] for g in regs) == {passes} and regs[-1]['kind'] == 1, regs[-3:]\n"
            "print(json.dumps(minehip.search_hits_batch(reqs, 16)))\n")
    arg = json.dumps([(m.hex(), lo, hi, T) for m, lo, hi, T in reqs])
    r = subprocess.run([sys.executable, "-c", code, arg], env=dict(os.environ, MINEHIP_BATCH_SLOTS=str(slots)),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == json.loads(json.dumps(got))


def test_mixed_sizes_and_order(gpu):
    """[0, 3*10^6] plans a fast piece (a fallback, through the mh_search_hits path) between fused requests."""
    T6 = T10(6)
    reqs = [(b"cmu440", 10, 500, kth_smallest_hash(b"cmu440", 10, 500, 2)), (b"cmu440", 0, 3 * 10 ** 6, T6),
            (b"abc", 0, 999, 0), (b"cmu440", 0, 2 * 10 ** 6, T6), (b"cmu440", 123, 456, U64)]
    assert [g["kind"] for g in gpu.hits_batch_regions(reqs, 512)] == [0, 1, 0, 0, 0]
    assert [n for n, _ in hits_ref(*reqs[3], 512)[1]] == CMU_K6
    big = hits_ref(*reqs[1], 512)
    assert big[0] > 4 and [n for n, _ in big[1][:4]] == CMU_K6 and big[1][4][0] > 2 * 10 ** 6
    got = check(gpu, reqs, 512)
    assert got[0][0] == 2 and got[2][:2] == (0, []) and [n for n, _ in got[4][1]] == list(range(123, 457))


def test_dense(gpu):
    """Target 2^64 - 1 over partly filled tiles: every lane appends at every step."""
    msg, lo, hi = b"cmu440", 95_000, 105_123
    ref = hits_ref(msg, lo, hi, U64, 16_384)
    assert ref[0] == 10_124 and [n for n, _ in ref[1]] == list(range(lo, hi + 1))
    regs = gpu.hits_batch_regions([(msg, lo, hi, U64)], 16_384)
    assert [(g["kind"], g["slots"]) for g in regs] == [(0, 10_124)]
    assert (hi // 10 - lo // 10 + 1) % 256 != 0                        # the last tile is partly filled
    assert check(gpu, [(msg, lo, hi, U64)], 16_384) == [ref]


def test_per_request_errors(gpu):
    T = kth_smallest_hash(b"cmu440", 0, 999, 2)
    reqs = [(b"cmu440", 0, 999, T), (b"cmu440", 9, 3, T), (b"cmu440", 1000, 1999, T, gpu.MH_HITS_MAX_CAP + 1),
            (b"cmu440", 1000, 1999, T)]
    assert hits_ref(*reqs[0], 8)[0] == 2
    got = gpu.search_hits_batch(reqs, 8, errors="return")
    assert isinstance(got[1], gpu.MinehipError) and got[1].code == gpu.MH_ERANGE and got[1].index == 1
    assert isinstance(got[2], gpu.MinehipError) and got[2].code == gpu.MH_EINVAL and got[2].index == 2
    check(gpu, [reqs[0], reqs[3]], 8, [got[0], got[3]])
    with pytest.raises(gpu.MinehipError) as e:
        gpu.search_hits_batch(reqs, 8)
    assert e.value.code == gpu.MH_ERANGE and e.value.index == 1


def test_profile_counts_in_generic_class(gpu):
    reqs = [r + (kth_smallest_hash(*r, 1),) for r in EDGES[:6]]
    gpu.profile_enable(0, True)
    got = gpu.search_hits_batch(reqs, 4)
    p = gpu.profile_read(0)
    gpu.profile_enable(0, False)
    assert [g[0] for g in got] == [1] * 6
    assert p["generic_nonces"] == sum(hi - lo + 1 for _, lo, hi, _ in reqs) and p["generic_ns"] > 0
    assert p["fast_launches"] == 0
