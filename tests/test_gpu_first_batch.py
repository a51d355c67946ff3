"""mh_search_first_batch on the GPU: many first-hit searches fused into passes of batch_scan_first
(first-hit keys, per-request device words, tiles dispatched rank-major) and merge_segments_first,
the others through the mh_search_first path.  Bit-exact: every expected value comes from
test_first.first_ref / hits_of / kth_smallest_hash (the oracle's hashes of the whole range, in
numpy), and every result is also what minehip.search_first gives for the same request.

Every case first asserts from the reference alone that it is live -- how many nonces qualify and
where they lie.  `scanned` is only held to its bounds: the whole range when nothing qualifies,
nonce - lower + 1 <= scanned <= the range's size otherwise.  No test asserts a skip."""
import json
import os
import random
import subprocess
import sys

import pytest

from conftest import PKG, ROOT
from test_first import first_ref, hits_of, kth_smallest_hash
from test_gpu_batch import EDGES, TILE, capacity_requests, fuzz_requests
from test_gpu_parity import env

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CMU = (b"cmu440", 0, 1_999_999)
CMU_MIN = (1228377698034, 1_067_492)          # the range's minimum (tests/test_gpu_first.py)
CMU_FIRST = {2: 111, 3: 1_081, 4: 19_411, 5: 114_702, 6: 393_322}    # target 2^64 // 10^k: first hit


def check_scanned(r, g):
    msg, lo, hi, T = r
    if g[0]:
        assert g[2] - lo + 1 <= g[3] <= hi - lo + 1, (msg[:8], lo, hi, T, g)
    else:
        assert g[3] == hi - lo + 1, (msg[:8], lo, hi, T, g)


def check(gpu, reqs, got=None):
    """search_first_batch(reqs) against the reference, against search_first() of every request and,
    where nothing qualifies, against search(); scanned within its bounds."""
    if got is None:
        got = gpu.search_first_batch(reqs)
    assert len(got) == len(reqs)
    for r, g in zip(reqs, got):
        msg, lo, hi, T = r
        assert g[:3] == first_ref(msg, lo, hi, T), (msg[:8], len(msg), lo, hi, T, g)
        assert g[:3] == gpu.search_first(msg, lo, hi, T)[:3], (msg[:8], lo, hi, T, g)
        check_scanned(r, g)
        if not g[0]:
            assert g[1:3] == gpu.search(msg, lo, hi), (msg[:8], lo, hi, T, g)
    return got


def test_edges_in_one_call(gpu):
    assert (b"cmu440", 0, 0) in EDGES and (b"cmu440", 9, 10) in EDGES and (b"cmu440", U64 - 5000, U64) in EDGES
    assert [r[2] - r[1] + 1 for r in EDGES[-3:]] == [TILE, TILE + 1, TILE]
    reqs = []
    for msg, lo, hi in EDGES:
        mn = kth_smallest_hash(msg, lo, hi, 1)
        targets = [mn, mn - 1, U64, 0]
        assert mn > 0 and len(hits_of(msg, lo, hi, mn)) == 1 and not hits_of(msg, lo, hi, mn - 1)
        assert first_ref(msg, lo, hi, U64)[2] == lo and not first_ref(msg, lo, hi, 0)[0]
        if hi - lo + 1 >= 3:
            T3 = kth_smallest_hash(msg, lo, hi, 3)
            assert len(hits_of(msg, lo, hi, T3)) == 3
            targets.insert(0, T3)
        reqs += [(msg, lo, hi, T) for T in targets]
    assert len(reqs) == 5 * len(EDGES) - 4          # [0, 0], 7, 9..10 and 2^64 - 1 have fewer than 3 nonces
    # a first hit that is not the minimum's nonce is among them
    assert sum(1 for m, lo, hi, T in reqs if first_ref(m, lo, hi, T)[0] and
               first_ref(m, lo, hi, T)[2] != first_ref(m, lo, hi, 0)[2]) >= 10
    plan = gpu.batch_plan([r[:3] for r in reqs])
    assert all(it["kind"] == 0 and it["pass"] == 0 for it in plan)     # all fused, one pass
    check(gpu, reqs)


def test_one_message_many_targets(gpu):
    msg, lo, hi = CMU
    targets = [2 ** 64 // 10 ** k for k in (2, 3, 4, 5, 6)] + [CMU_MIN[0], CMU_MIN[0] - 1, U64, 0]
    exp = [first_ref(msg, lo, hi, T) for T in targets]
    assert [e[2] for e in exp[:5]] == [CMU_FIRST[k] for k in (2, 3, 4, 5, 6)] and all(e[0] for e in exp[:5])
    assert exp[5] == (True,) + CMU_MIN and exp[6] == (False,) + CMU_MIN and exp[8] == (False,) + CMU_MIN
    assert exp[7][0] and exp[7][2] == 0
    # nine targets, eight different results: the two targets below the minimum both give (False, min)
    assert len(set(exp)) == 8 and len(set(exp[:6] + exp[7:8])) == 7 and exp[6] == exp[8]
    reqs = [(msg, lo, hi, T) for T in targets]
    plan = gpu.batch_plan([r[:3] for r in reqs])
    assert [it["kind"] for it in plan] == [0] * 9 and {it["pass"] for it in plan} == {0}
    got = check(gpu, reqs)
    with env(MINEHIP_FIRST_BATCH_ORDER="request"):
        assert gpu.first_batch_order(reqs) == list(range(9 * 782))
        again = gpu.search_first_batch(reqs)
    assert [g[:3] for g in again] == [g[:3] for g in got] == exp
    for r, g in zip(reqs, again):
        check_scanned(r, g)


def fuzz_targets():
    """fuzz_requests(seed=440, n=200), each with a target drawn with a fixed seed from: the k-th
    smallest hash of its range for k in {1, 2, 5} (the largest hash where the range has fewer than
    k nonces), the minimum minus 1, 2^64 - 1, and 2^64 // size."""
    rng = random.Random(4401)
    reqs = []
    for msg, lo, hi in fuzz_requests(seed=440, n=200):
        size = hi - lo + 1
        kind = rng.randrange(6)
        k = (1, 2, 5)[kind] if kind < 3 else 0
        if kind < 3:
            T = kth_smallest_hash(msg, lo, hi, min(k, size))
        elif kind == 3:
            T = kth_smallest_hash(msg, lo, hi, 1) - 1
        elif kind == 4:
            T = U64
        else:
            T = 2 ** 64 // size
        reqs.append((msg, lo, hi, T))
    return reqs


def test_fuzz_seed440_one_call(gpu):
    reqs = fuzz_targets()
    exp = [first_ref(*r) for r in reqs]
    argmin = [first_ref(m, lo, hi, 0)[2] for m, lo, hi, _ in reqs]
    assert sum(1 for e, a in zip(exp, argmin) if e[0] and e[2] != a) >= 40
    assert sum(1 for e in exp if not e[0]) >= 20
    check(gpu, reqs)


def test_several_entries_per_request(gpu):
    """MINEHIP_MAX_BLOCKS=16 cuts a request of 30,000 nonces into generic pieces of 4,096: eight
    entries, whose tiles share the request's three device words and its rank order."""
    msg, lo, hi = b"cmu440", 340_000, 369_999
    with env(MINEHIP_MAX_BLOCKS=16):
        plan = gpu.batch_plan([(msg, lo, hi)])
        assert len(plan) >= 3 and all(it["kind"] == 0 and it["count"] <= 4096 for it in plan)
        first_e, last_e = plan[0], plan[-1]
        in_first = lambda n: first_e["first"] <= n < first_e["first"] + first_e["count"]   # noqa: E731
        in_last = lambda n: last_e["first"] <= n <= hi                                      # noqa: E731
        mn = kth_smallest_hash(msg, lo, hi, 1)
        assert [in_last(n) for n in hits_of(msg, lo, hi, mn)] == [True]       # the only hit: in the last entry
        T2 = max(kth_smallest_hash(msg, first_e["first"], first_e["first"] + first_e["count"] - 1, 1), mn)
        hits = hits_of(msg, lo, hi, T2)
        assert in_first(hits[0]) and in_last(hits[-1]) and first_ref(msg, lo, hi, T2)[2] == hits[0]
        assert not hits_of(msg, lo, hi, mn - 1)
        reqs = [(msg, lo, hi, mn), (msg, lo, hi, T2), (msg, lo, hi, mn - 1)]
        order = gpu.first_batch_order(reqs)
        tiles = sum(it["slots"] for it in plan)
        assert sorted(order) == list(range(3 * tiles)) and order[:4] == [0, tiles, 2 * tiles, 1]
        check(gpu, reqs)


@pytest.mark.parametrize("slots,passes", [(8, 0), (32, 20)])
def test_passes_and_fallback_by_capacity(gpu, slots, passes):
    """MINEHIP_BATCH_SLOTS (a child process) against the default capacity: with 8 slots every
    request is a fallback, with 32 there are 20 passes and one fallback.  found, hash and nonce are
    the same and the reference's; scanned stays within its bounds in each."""
    reqs = [(m, lo, hi, kth_smallest_hash(m, lo, hi, 2)) for m, lo, hi in capacity_requests()]
    assert all(len(hits_of(*r)) == 2 for r in reqs)
    got = check(gpu, reqs)
    code = (f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}, {os.path.join(ROOT, 'tests')!r}]\n"
            "import json, minehip\n"
            "reqs = [(bytes.fromhex(m), lo, hi, T) for m, lo, hi, T in json.loads(sys.argv[1])]\n"
            "plan = minehip.batch_plan([r[:3] for r in reqs])\n"
            f"assert 1 + max(it['pass'] for it in plan) == {passes} and plan[-1]['kind'] == 1, plan[-3:]\n"
            "print(json.dumps(minehip.search_first_batch(reqs)))\n")
    arg = json.dumps([(m.hex(), lo, hi, T) for m, lo, hi, T in reqs])
    r = subprocess.run([sys.executable, "-c", code, arg], env=dict(os.environ, MINEHIP_BATCH_SLOTS=str(slots)),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    child = [tuple(x) for x in json.loads(r.stdout.strip().splitlines()[-1])]
    assert [g[:3] for g in child] == [g[:3] for g in got]
    for q, g in zip(reqs, child):
        check_scanned(q, g)


def test_mixed_sizes_and_order(gpu):
    """[0, 3*10^6] plans a fast piece (a fallback, through the mh_search_first path) between fused requests."""
    T6 = 2 ** 64 // 10 ** 6
    reqs = [(b"cmu440", 10, 500, kth_smallest_hash(b"cmu440", 10, 500, 2)), (b"cmu440", 0, 3 * 10 ** 6, T6),
            (b"abc", 0, 999, 0), (b"cmu440", 0, 2 * 10 ** 6, T6), (b"cmu440", 123, 456, U64)]
    kinds = {it["req"]: it["kind"] for it in gpu.batch_plan([r[:3] for r in reqs])}
    assert kinds == {0: 0, 1: 1, 2: 0, 3: 0, 4: 0}
    assert first_ref(*reqs[1])[2] == 393_322 == first_ref(*reqs[3])[2] and len(hits_of(*reqs[1])) > 1
    got = check(gpu, reqs)
    assert got[1][2] == 393_322 and got[4][2] == 123 and not got[2][0]


def test_per_request_errors(gpu):
    T = kth_smallest_hash(b"cmu440", 0, 999, 2)
    reqs = [(b"cmu440", 0, 999, T), (b"cmu440", 9, 3, T), (b"cmu440", 1000, 1999, T)]
    got = gpu.search_first_batch(reqs, errors="return")
    assert isinstance(got[1], gpu.MinehipError) and got[1].code == gpu.MH_ERANGE and got[1].index == 1
    check(gpu, [reqs[0], reqs[2]], [got[0], got[2]])
    with pytest.raises(gpu.MinehipError) as e:
        gpu.search_first_batch(reqs)
    assert e.value.code == gpu.MH_ERANGE and e.value.index == 1


def test_profile_counts_in_generic_class(gpu):
    reqs = [r + (kth_smallest_hash(*r, 1) - 1,) for r in EDGES[:6]]
    gpu.profile_enable(0, True)
    gpu.search_first_batch(reqs)
    p = gpu.profile_read(0)
    gpu.profile_enable(0, False)
    assert p["generic_nonces"] == sum(hi - lo + 1 for _, lo, hi, _ in reqs) and p["generic_ns"] > 0
    assert p["fast_launches"] == 0
