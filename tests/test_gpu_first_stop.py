"""mh_search_first_ex(MH_FIRST_STOP_RUNNING) on the GPU: stop_scan<J, MODE> publishes a hit when it
finds it and leaves a running chunk that lies wholly above a published hit.  found, hash and nonce
are bit for bit mh_search_first's (test_first.first_ref, and the call with flags 0) under every
plan and for every fast layout; `scanned`, counted by the waves themselves, is the range's size when
nothing qualifies and lies within [nonce - lower + 1, size] otherwise; and the stop is shown live:
fewer nonces hashed than without the flag, where the reference says chunks lie above the first hit.

Every case asserts from the reference alone that it is live before it looks at the GPU."""
import pytest

from test_abi import KERNELS, KERNEL_CASE_NONCES, kernel_cases
from test_first import first_ref, hits_of, kth_smallest_hash
from test_gpu_first import plans
from test_gpu_parity import env

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
CMU = (b"cmu440", 0, 1_999_999)
CMU_MIN = (1228377698034, 1_067_492)          # the range's minimum (tests/test_gpu_first.py)
CMU_FIRST = {2: 111, 3: 1_081, 4: 19_411, 6: 393_322}     # target 2^64 // 10^k: first hit
T6 = 2 ** 64 // 10 ** 6
FAST = dict(MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1)
CHUNK1 = 2560  # nonces of one workgroup's chunk at L = 1 (256 lanes x 10)


def check(gpu, msg, lo, hi, T, what=None):
    """One search with the flag against the reference and against flags 0, scanned included;
    returns ((found, hash, nonce, scanned) with the flag, the same with flags 0)."""
    exp = first_ref(msg, lo, hi, T)
    plain = gpu.search_first(msg, lo, hi, T)
    got = gpu.search_first(msg, lo, hi, T, stop_running=True)
    assert got[:3] == exp == plain[:3], (what, msg[:8], len(msg), lo, hi, T, got, plain, exp)
    size = hi - lo + 1
    if exp[0]:
        assert got[2] - lo + 1 <= got[3] <= size, (what, got)
    else:
        assert got[3] == size == plain[3], (what, got, plain)
        assert got[1:3] == gpu.search(msg, lo, hi), (what, got)
    return got, plain


def test_same_answers_under_every_plan(gpu):
    msg, lo, hi = CMU
    targets = {}
    for k, n in CMU_FIRST.items():
        T = 2 ** 64 // 10 ** k
        assert first_ref(msg, lo, hi, T)[0] and first_ref(msg, lo, hi, T)[2] == n, k
        targets[T] = "k=%d" % k
    hits = hits_of(msg, lo, hi, T6)
    assert len(hits) == 4 and hits[0] == 393_322 != CMU_MIN[1] and CMU_MIN[1] in hits   # first hit != argmin
    assert first_ref(msg, lo, hi, CMU_MIN[0]) == (True,) + CMU_MIN and hits_of(msg, lo, hi, CMU_MIN[0]) == [CMU_MIN[1]]
    assert first_ref(msg, lo, hi, CMU_MIN[0] - 1) == (False,) + CMU_MIN
    assert first_ref(msg, lo, hi, U64)[2] == lo and first_ref(msg, lo, hi, 0) == (False,) + CMU_MIN
    targets.update({CMU_MIN[0]: "min", CMU_MIN[0] - 1: "min-1", 0: "zero", U64: "all"})
    assert len(targets) == 8
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        assert any(p["kind"] == 0 for p in gpu.plan(msg, lo, hi))       # those plans do run fast kernels
    results = {}
    for kv in plans():
        with env(**kv):
            for T, name in targets.items():
                got, _ = check(gpu, msg, lo, hi, T, (name, kv))
                results.setdefault(name, set()).add(got[:3])
    assert len(plans()) == 9 and all(len(v) == 1 for v in results.values()), results    # identical throughout


def test_every_fast_layout(gpu):
    """Each of the 26 layouts over test_abi.kernel_cases()' range plus 3,456 nonces (more than one
    chunk at L = 1), at MINEHIP_LOWER_DIGITS in {1, 3}: exactly five hits spread over more than one
    chunk -- chunks above the first of them may be left -- and no hit at all."""
    cases = kernel_cases()
    assert set(cases) == KERNELS and len(KERNELS) == 26
    interleaved, planned = set(), set()
    for (J, mode), (m, lo, _, early) in sorted(cases.items()):
        hi = lo + KERNEL_CASE_NONCES + 3_456
        T5, T1 = kth_smallest_hash(m, lo, hi, 5), kth_smallest_hash(m, lo, hi, 1)
        hits = hits_of(m, lo, hi, T5)
        assert len(hits) == 5 and hits[-1] - hits[0] > CHUNK1, (J, mode, hits)
        assert not hits_of(m, lo, hi, T1 - 1)
        for Ld in (1, 3):
            with env(**FAST, MINEHIP_LOWER_DIGITS=Ld, MINEHIP_EARLY=early):
                pieces = [p for p in gpu.plan(m, lo, hi) if p["kind"] == 0 and (p["word"], p["mode"]) == (J, mode)]
                if pieces:
                    planned.add((J, mode))
                if mode >= 3:   # an Early piece at innermost position p >= L: its lanes interleave
                    t = (len(m) + 1) % 64
                    for pc in pieces:
                        pl = t + pc["digits"] - 1
                        base = 64 if (pc["blocks"] == 2 and pl >= 64) else 0
                        p = pl - (base + 4 * J + 3)
                        if p >= pc["lo_digits"] and any(pc["first"] <= n < pc["first"] + pc["count"] for n in hits):
                            interleaved.add((J, mode))
                for T in (T5, T1 - 1):
                    check(gpu, m, lo, hi, T, (J, mode, Ld))
    assert planned == KERNELS, KERNELS - planned
    assert interleaved == {k for k in KERNELS if k[1] >= 3}, interleaved


def test_the_stop_is_live_at_a_small_shape(gpu):
    """Four chunks of 256 runs x 1,000 nonces, all claimed at once; the first hit sits in chunk 0 at
    group 49 of 100 and three chunks lie wholly above it.  Without the flag every chunk runs to its
    end (scanned is the range); with it the three chunks are left once the hit is published."""
    msg, lo, hi = b"cmu440", 1_000_000, 1_999_999
    hits = hits_of(msg, lo, hi, T6)
    assert hits == [1_067_492, 1_456_236, 1_999_610]
    run, q = divmod(hits[0] - lo, 1000)
    assert run < 256 and q // 10 == 49                              # chunk 0, group 49 of 100
    assert all(lo + c * 256_000 > hits[0] for c in (1, 2, 3))       # the floors of chunks 1..3
    exp = first_ref(msg, lo, hi, T6)
    assert exp[0] and exp[2] == hits[0]
    with env(**FAST, MINEHIP_LOWER_DIGITS=3):
        pieces = gpu.plan(msg, lo, hi)
        assert len(pieces) == 1 and pieces[0]["kind"] == 0 and pieces[0]["mode"] < 3, pieces
        assert (pieces[0]["first"], pieces[0]["count"], pieces[0]["lo_digits"]) == (lo, 1_000_000, 3), pieces
        assert -(-(pieces[0]["count"] // 1000) // 256) == 4         # 1,000 runs: four chunks
        plain = gpu.search_first(msg, lo, hi, T6)
        got = gpu.search_first(msg, lo, hi, T6, stop_running=True)
    print("scanned: flags 0 %d, MH_FIRST_STOP_RUNNING %d" % (plain[3], got[3]))
    assert plain[:3] == exp and plain[3] == 1_000_000, plain        # all four workgroups claim before chunk 0 ends
    assert got[:3] == exp, (got, exp)
    assert hits[0] - lo + 1 <= got[3] < 1_000_000, got


def test_two_streams_coarse_launch_beside_small_pieces(gpu):
    """The default plan over [0, 2^32): the small pieces that hold the answer run beside a coarse
    launch whose first generation of chunks starts before any hit can be known."""
    msg, lo, hi = b"cmu440", 0, 2 ** 32 - 1
    exp = first_ref(*CMU, T6)                 # the first hit of [0, 1,999,999] is the first of any longer range
    assert exp[0] and exp[2] == 393_322
    plain = gpu.search_first(msg, lo, hi, T6)
    got = gpu.search_first(msg, lo, hi, T6, stop_running=True)
    print("scanned: flags 0 %d, MH_FIRST_STOP_RUNNING %d" % (plain[3], got[3]))
    assert plain[:3] == exp == got[:3], (plain, got, exp)
    assert 393_323 <= got[3] < plain[3] <= hi - lo + 1, (got, plain)


def test_nothing_found(gpu):
    msg, lo, hi = b"cmu440", 0, 99_999_999
    got = gpu.search_first(msg, lo, hi, 0, stop_running=True)
    assert got == (False,) + gpu.search(msg, lo, hi) + (10 ** 8,), got
