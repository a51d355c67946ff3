"""Chosen-nonce probes of the four first-hit builds of fast_search.hip: first_scan (mh_search_first),
stop_scan (mh_search_first_ex, MH_FIRST_STOP_RUNNING), batch_first (mh_search_first_batch_ex,
MH_BATCH_FUSE_FAST) and batch_stop (mh_search_first_batch_stop).

These builds take no hash hook, and a first-hit search returns one nonce.  A test can still choose
which: to probe n* of [lo, hi] take T = Hash(msg, n*), prev = the last n < n* with Hash(msg, n) <= T
and lo' = max(lo, prev + 1); the reference answer of (msg, lo', hi, T) is exactly (True, T, n*).  The
GPU returns it only if it computes all 64 bits of that nonce's hash at its place in the plan,
considers the nonce and rebuilds its value.  The same lo' with T - 1 has the reference's next hit
above n*, or no hit at all -- then the answer is the range's minimum, (False, T, n*), found being
what tells the two apart -- and catches a too-small wrong hash anywhere in [lo', hi].  What the
probes do not show is a too-large wrong hash at an unprobed nonce.

Unlike the record-low tests, which keep lo fixed and so reach about ln N nonces near the start of
the range, n* sits anywhere: the candidates are the 300 nonces with the lowest hashes of each
layout's range (test_gpu_dense.dense_cases), kept where, under minehip.plan(msg, lo', hi) in the
search's environment, n* lies in a fast piece of the layout's own kernel.  <0, One> owns 990 nonces
of its range ([10, 99] and [100, 999]): its candidates are the 60 lowest hashes among those (at
L = 3, where few of them can be probed, all 990).  At MINEHIP_LOWER_DIGITS=3 a search takes 2.9 ms
against 0.12 ms at L = 1 (tests/test_gpu_probe.py), so the kept probes are cut to 60 per layout
there, plus what the digit coverage needs.  Every expected value comes from slices of the one
full_hashes array of [lo, hi].  test_probe_sets_cover asserts the coverage on the host.

Measured on an MI355X (one run each), seconds.  The first test to run also builds the probe sets
(5 s of host work, shared by the others); stop_scan compares with first_scan's cached answers:
  first_scan   L = 1: 4.3 (14,392 searches)   L = 3: 4.6 + 4.6 (3,000 searches in two halves)
  stop_scan    L = 1: 1.8                     L = 3: 4.4 + 4.7
  batch_first  L = 1: 0.11   L = 3: 0.17      batch_stop  L = 1: 0.10   L = 3: 0.17
(a batch call runs its 60 one-chunk requests at L = 3 side by side, which is why it is 50 times
faster there than 60 single searches).
"""
import collections
import functools

import numpy as np
import pytest

from test_gpu_dense import FAST, LDS, dense_cases
from test_gpu_parity import env
from test_gpu_probe import chunk_of, last_of
from test_gpu_ties import full_hashes

CANDIDATES = 300        # lowest hashes of a range
CANDIDATES_0_ONE = 60   # ... among the 990 nonces of <0, One>'s own pieces
CUT_L3 = 60             # probes per layout at L = 3, before the digit top-up

Probe = collections.namedtuple("Probe", "n lower T exp exp_below piece")
# exp, exp_below: (found, hash, nonce) of (msg, lower, hi, T) and of (msg, lower, hi, T - 1)


def expect(h, lo, lower, T):
    """(found, hash, nonce) of mh_search_first(msg, lower, hi, T) from the hashes h of [lo, hi]: the
    first nonce at or above `lower` whose hash is <= T, or the first minimum of [lower, hi]."""
    part = h[lower - lo:]
    hit = np.flatnonzero(part <= np.uint64(T))
    j = int(hit[0]) if hit.size else int(part.argmin())
    return bool(hit.size), int(part[j]), lower + j


def probe_of(h, lo, n):
    """(lower, T, exp, exp_below) of the probe of nonce n from the hashes h of [lo, hi]."""
    i = n - lo
    T = int(h[i])
    before = np.flatnonzero(h[:i] <= np.uint64(T))
    lower = lo + int(before[-1]) + 1 if before.size else lo
    return lower, T, expect(h, lo, lower, T), expect(h, lo, lower, T - 1)


def check_probe(got, exp, lower, hi, what):
    """One answer (found, hash, nonce, scanned) against the reference and the scanned contract."""
    assert tuple(got[:3]) == exp, (what, got, exp)
    size = hi - lower + 1
    if exp[0]:
        assert exp[2] - lower + 1 <= got[3] <= size, (what, got, size)
    else:
        assert got[3] == size, (what, got, size)


def own_piece(pieces, layout, n, kind):
    for p in pieces:
        if p["kind"] == kind and (p["word"], p["mode"]) == layout and p["first"] <= n <= last_of(p):
            return p
    return None


def digits_covered(ns):
    return all({n // 10 ** k % 10 for n in ns} == set(range(10)) for k in (0, 1))


@functools.lru_cache(maxsize=None)
def probe_sets():
    """{(layout, Ld): dict(msg, lo, hi, env, own, probes)}: the kept probes of each layout at
    MINEHIP_LOWER_DIGITS 1 and 3 (host only); own: the layout's fast pieces in the plan of [lo, hi]."""
    import minehip
    out = {}
    for k, m, lo, hi, early in dense_cases():
        h = full_hashes(m, lo, hi)
        probed = {}                         # n: probe_of(h, lo, n), the same at both L
        for Ld in LDS:
            e = dict(FAST, MINEHIP_LOWER_DIGITS=Ld, MINEHIP_EARLY=early)
            with env(**e):
                own = [p for p in minehip.plan(m, lo, hi, cap=256) if p["kind"] == 0 and (p["word"], p["mode"]) == k]
                if k == (0, 0):
                    # at L = 3 its pieces are [10, 99] at L = 1 and [100, 999] at L = 2, whose nine lanes of
                    # 100 nonces start a fast piece only at a multiple of 100: a nonce can be probed there
                    # only if it is the lowest hash of its lane so far, about five per lane, so every
                    # nonce of the pieces is a candidate
                    mine = np.concatenate([np.arange(p["first"] - lo, last_of(p) - lo + 1) for p in own])
                    ranked = mine[np.argsort(h[mine], kind="stable")]
                    cand = [lo + int(i) for i in (ranked[:CANDIDATES_0_ONE] if Ld == 1 else ranked)]
                elif Ld == 1:
                    cand = [lo + int(i) for i in np.argsort(h, kind="stable")[:CANDIDATES]]
                kept = []
                for n in cand:
                    if n not in probed:
                        probed[n] = probe_of(h, lo, n)
                    lower, T, exp, below = probed[n]
                    pc = own_piece(minehip.plan(m, lower, hi, cap=256), k, n, 0)
                    if pc is not None:
                        kept.append(Probe(n, lower, T, exp, below, pc))
            if Ld == 3 and len(kept) > CUT_L3:
                rest = kept[CUT_L3:]
                kept = kept[:CUT_L3]
                while rest and not digits_covered([p.n for p in kept]):     # 60 draws can miss a digit value
                    kept.append(rest.pop(0))
            out[(k, Ld)] = dict(msg=m, lo=lo, hi=hi, env=e, own=own, probes=kept)
    return out


def batch_probes(minehip, s, layout):
    """The probes of one set that mh_batch_plan_ex fuses with a kind-2 piece of the layout holding
    n* (one request per probe, all in one call), and how many it does not."""
    if not s["probes"]:
        return [], 0
    with env(**s["env"]):
        plan = minehip.batch_plan_ex([(s["msg"], p.lower, s["hi"]) for p in s["probes"]], fuse_fast=True, cap=1 << 14)
    per = collections.defaultdict(list)
    for pc in plan:
        per[pc["req"]].append(pc)
    ok = [p for i, p in enumerate(s["probes"])
          if all(pc["kind"] != 1 for pc in per[i]) and own_piece(per[i], layout, p.n, 2) is not None]
    return ok, len(s["probes"]) - len(ok)


def check_cover(k, Ld, s, probes):
    """The floors of one probe set: how many probes, in how many chunks, with which digits."""
    if Ld == 3 and not s["own"]:
        assert k == (0, 3) and not probes      # at L = 3 <0, OneEarly>'s range runs <1, One>
        return
    if Ld == 1:
        floor = 50 if k == (0, 0) else 100     # 53 of <0, One>'s 60 candidates; 129 .. 300 of 300 elsewhere
    else:
        floor = 60                             # more than 60 are kept everywhere, cut to 60
    assert len(probes) >= floor, (k, Ld, len(probes))
    assert all(s["lo"] <= p.lower <= p.n <= s["hi"] for p in probes)
    have = sum(-(-pc["count"] // 10 ** pc["lo_digits"] // 256) for pc in s["own"])
    # a chunk as the probe's own search sees it: which piece (by its end: lower moves its start) and
    # which 256 lanes of it
    chunks = {(last_of(p.piece), chunk_of(s["msg"], p.piece, p.n)) for p in probes}
    assert len(chunks) >= min(3, have), (k, Ld, chunks, have)
    assert digits_covered([p.n for p in probes]), (k, Ld)


# ---- CPU tests -------------------------------------------------------------------------------------

def test_probe_sets_cover():
    """Per layout at least 100 kept probes at L = 1 (129 .. 300 of the 300 candidates are kept; 53
    of <0, One>'s 60, floor 50) and at least 60 at L = 3 where the layout is planned (more than 60
    are kept of each and cut to 60; of <0, One> only 33 of its 60, so every nonce of its 990 is a
    candidate there); in at least three different 256-lane chunks where the layout's pieces have
    three; every digit value at each of the low two decimal places.  The same floors for what
    mh_batch_plan_ex keeps of them, which is all of them.  And the expectation helper itself: a
    flipped bit of the reference's hash of a probed n* changes that probe's expectation, and the
    unflipped answer then fails the check."""
    import minehip
    from test_abi import KERNELS
    sets = probe_sets()
    assert {k for k, _ in sets} == KERNELS and len(sets) == 52
    counts = {}
    for (k, Ld), s in sets.items():
        check_cover(k, Ld, s, s["probes"])
        ok, dropped = batch_probes(minehip, s, k)
        assert dropped == 0, (k, Ld, dropped)
        check_cover(k, Ld, s, ok)
        counts[(k, Ld)] = len(s["probes"])
        for p in s["probes"]:
            assert p.exp == (True, p.T, p.n)
            assert p.exp_below[2] > p.n if p.exp_below[0] else p.exp_below == (False, p.T, p.n), (k, Ld, p)
    print(sorted(counts.items()))
    # some T - 1 probes hit further up and some miss: both arms of the reference are live
    below = [p.exp_below[0] for s in sets.values() for p in s["probes"]]
    assert sum(below) > 1_000 and len(below) - sum(below) >= 26
    s = sets[((3, 0), 1)]
    h, p = full_hashes(s["msg"], s["lo"], s["hi"]), s["probes"][40]
    assert probe_of(h, s["lo"], p.n) == (p.lower, p.T, p.exp, p.exp_below)
    flipped = h.copy()
    flipped[p.n - s["lo"]] ^= np.uint64(1 << 40)
    wrong = probe_of(flipped, s["lo"], p.n)
    assert wrong[2] != p.exp and wrong[1] != p.T
    check_probe(p.exp + (p.n - p.lower + 1,), p.exp, p.lower, s["hi"], "good")
    with pytest.raises(AssertionError):
        check_probe(p.exp + (p.n - p.lower + 1,), expect(flipped, s["lo"], p.lower, p.T), p.lower, s["hi"], "flipped")
    with pytest.raises(AssertionError):
        check_probe(p.exp + (p.n - p.lower,), p.exp, p.lower, s["hi"], "scanned too small")


# ---- GPU tests -------------------------------------------------------------------------------------

# (L, part, parts): at L = 3 every search runs a whole 253-lane chunk of 1,000-nonce lanes, so the
# single-request builds take the layouts there in two halves of about 4.6 s each
PARTS = ((1, 0, 1), (3, 0, 2), (3, 1, 2))
PART_IDS = ("L1", "L3a", "L3b")


def sets_of(Ld, part=0, parts=1):
    """[(layout, set)] of this L, every parts-th layout from the part-th."""
    return [(k, s) for (k, L), s in probe_sets().items() if L == Ld][part::parts]


@functools.lru_cache(maxsize=None)
def single_probes(gpu, Ld, part, parts, stop_running):
    """Every kept probe of these layouts through search_first: target T and T - 1.  Run once per
    build: the stop_scan test compares with what the first_scan test got."""
    res = {}
    for k, s in sets_of(Ld, part, parts):
        with env(**s["env"]):
            for p in s["probes"]:
                for T, exp in ((p.T, p.exp), (p.T - 1, p.exp_below)):
                    got = gpu.search_first(s["msg"], p.lower, s["hi"], T, stop_running=stop_running)
                    check_probe(got, exp, p.lower, s["hi"], (k, Ld, "stop" if stop_running else "scan", p.n, p.lower, T))
                    res[(k, p.n, T)] = got
    assert len(res) == 2 * sum(len(s["probes"]) for _, s in sets_of(Ld, part, parts)) >= 1_300
    return res


def batch_probe_calls(gpu, Ld, stop_running):
    """Every probe of one layout as one call of one request per probe, target T, then T - 1."""
    done = 0
    for k, s in sets_of(Ld):
        probes, dropped = batch_probes(gpu, s, k)
        assert dropped == 0
        check_cover(k, Ld, s, probes)
        if not probes:
            continue
        with env(**s["env"]):
            for below in (False, True):
                reqs = [(s["msg"], p.lower, s["hi"], p.T - 1 if below else p.T) for p in probes]
                res = gpu.search_first_batch(reqs, fuse_fast=True, stop_running=stop_running)
                assert len(res) == len(probes)
                for p, r, got in zip(probes, reqs, res):
                    check_probe(got, p.exp_below if below else p.exp, p.lower, s["hi"],
                                (k, Ld, "batch_stop" if stop_running else "batch_first", p.n, p.lower, r[3]))
                done += len(reqs)
    assert done == 2 * sum(len(s["probes"]) for _, s in sets_of(Ld)) >= 2_900
    return done


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", PARTS, ids=PART_IDS)
def test_first_scan_probes(gpu, Ld, part, parts):
    single_probes(gpu, Ld, part, parts, False)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", PARTS, ids=PART_IDS)
def test_stop_scan_probes(gpu, Ld, part, parts):
    """... and found, hash and nonce bit for bit first_scan's."""
    stop, scan = single_probes(gpu, Ld, part, parts, True), single_probes(gpu, Ld, part, parts, False)
    assert stop.keys() == scan.keys() and all(stop[key][:3] == scan[key][:3] for key in stop)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_batch_first_probes(gpu, Ld):
    batch_probe_calls(gpu, Ld, False)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_batch_stop_probes(gpu, Ld):
    batch_probe_calls(gpu, Ld, True)
