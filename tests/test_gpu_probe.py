"""Per-nonce hash values and range coverage on the GPU.

A search returns one (hash, nonce), so comparing it with the oracle verifies one nonce's hash per
search: of every other nonce it shows only that whatever the kernel computed for it was not
smaller.  A defect that corrupts a fraction f of the nonces (one (g, i) pair of fast_search, one
digit position of U, one lane), scans hi + 1, or drops a nonce at a seam between plan pieces,
launches, chunks, tiles or host chunks is noticed with probability f or 1 / N per search.

The dev build's MINEHIP_DEV_HASH_XOR=x hook XORs every nonce's (H0, H1) with a
64-bit constant before the keep mask and before any comparison, which lets a test choose the
winner.  With x = Hash(msg, n*) from the CPU oracle:
  positive probe  n* inside [lo, hi]: the search must return exactly (0, n*) -- iff the GPU computes
                  all 64 bits of Hash(msg, n*) at that nonce's place in the plan, considers the
                  nonce and rebuilds its value;
  negative probe  n* = lo - 1 or hi + 1: the search must return the reference's non-zero minimum,
                  and returns (0, n*) if anything scans past an edge.
One small search per probed nonce, the comparison code the product's.  Reference:
test_gpu_ties.masked_min(..., x), the first minimum of Hash(msg, n) ^ x over the oracle's hashes
of the whole range, bit-exact.  Probe sets come from random.Random with fixed seeds and from
minehip.plan under the search's own environment; their coverage conditions (digit values, chunk
spread, edges) are asserted on the host (test_probe_sets_cover).  One child process per GPU test.
"""
import collections
import concurrent.futures
import functools
import random

import numpy as np
import pytest

from oracle import oracle
from conftest import run_dev
from test_gpu_ties import BATCH_SLOTS, U64, check_jobs, early_tie_cases, full_hashes, job, masked_min, run_jobs

FULL = ((32, 32),)      # the identity keep pair: every probe compares full 64-bit hashes
# random probes per fast kernel at MINEHIP_LOWER_DIGITS 1 and 3.  At L = 3 the 253,456 nonces are 253
# lanes of 1,000 nonces in one workgroup, 2.9 ms a search on an MI355X against 0.12 ms at L = 1, so
# the draws there are cut to the floor of 60 that the digit coverage below needs (every structural
# probe stays): the test then takes 12.5 s instead of 21 s
RANDOM_FAST = {1: 150, 3: 60}
RANDOM_EARLY = 100      # ... per Early position case
RANDOM_GENERIC = 40     # ... per generic-path range
RANDOM_TILES = 10       # ... per multi-tile batch request
LANE_KS = (1, 63, 64, 65, 255, 256, 257)   # lane, wave and chunk boundaries of the last-digit layouts (and n_runs - 1)


def hashes_of(msg, lo, hi, nonces):
    """Hash(msg, n) of each n from the oracle: out of full_hashes(msg, lo, hi) where n lies inside."""
    full = full_hashes(msg, lo, hi)
    rest = [n for n in nonces if not lo <= n <= hi]
    extra = dict(zip(rest, oracle.hash_batch(msg, np.array(rest, dtype=np.uint64)).tolist())) if rest else {}
    return [int(full[n - lo]) if lo <= n <= hi else int(extra[n]) for n in nonces]


def planned(msg, lo, hi, env):
    """minehip.plan under the search's environment (host only)."""
    import minehip
    from test_gpu_parity import env as setenv
    with setenv(**env):
        return minehip.plan(msg, lo, hi)


def last_of(pc):
    return pc["first"] + pc["count"] - 1


def early_pos(msg, pc):
    """Decimal position p of the innermost digit of an Early piece (test_abi.check_plan)."""
    pl = (len(msg) + 1) % 64 + pc["digits"] - 1
    base = 64 if (pc["blocks"] == 2 and pl >= 64) else 0
    return pl - (base + 4 * pc["word"] + 3)


def chunk_of(msg, pc, n):
    """The workgroup chunk (256 lanes) of nonce n inside fast piece pc: lane U is n without its L
    lower digits; Early layouts: without the L digits at decimal positions p .. p + L - 1."""
    L = pc["lo_digits"]
    if pc["mode"] < 3:
        return (n // 10 ** L - pc["first"] // 10 ** L) // 256
    p = early_pos(msg, pc)
    return (n // 10 ** (p + L) * 10 ** p + n % 10 ** p - pc["first"] // 10 ** L) // 256


def edges(lo, hi):
    """(positive, negative) edge probes of a range."""
    return {lo, hi}, ({lo - 1} if lo > 0 else set()) | ({hi + 1} if hi < U64 else set())


def draw(rng, pieces, k):
    """k nonces drawn uniformly from the pieces."""
    total = sum(pc["count"] for pc in pieces)
    out = set()
    for _ in range(k):
        r = rng.randrange(total)
        for pc in pieces:
            if r < pc["count"]:
                out.add(pc["first"] + r)
                break
            r -= pc["count"]
    return out


class Case(dict):
    """msg, lo, hi, env, pieces, pos (probed nonces inside the range), neg (outside)."""
    __getattr__ = dict.__getitem__

    @property
    def probes(self):
        return sorted(self.pos) + sorted(self.neg)

    def job(self, **kw):
        xs = hashes_of(self.msg, self.lo, self.hi, self.probes)
        return job(self.msg, self.lo, self.hi, FULL, [self.env], xors=xs, **kw)


def seam_probes(pieces):
    return {n for pc in pieces for n in (pc["first"], last_of(pc))}


def run_cases(tmp_path, cases, profile=False, **kw):
    """One search per probe of every case; every result against masked_min(..., x), and from the
    probes alone: a positive probe returns (0, n*), a negative one a non-zero hash.  The reference
    is computed on four threads while the child process searches."""
    jobs = [c.job(**kw) for c in cases]
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        refs = ex.map(lambda cj: [masked_min(cj[0].msg, cj[0].lo, cj[0].hi, 32, 32, x) for x in cj[1]["xors"]],
                      list(zip(cases, jobs)))
        results, kernels = run_jobs(tmp_path, jobs, profile=profile)
        refs = list(refs)
    assert len(results) == sum(len(c.probes) for c in cases)
    it = iter(results)
    for c, j, exps in zip(cases, jobs, refs):
        for n, x, exp in zip(c.probes, j["xors"], exps):
            got = tuple(next(it))
            assert got == (exp.hash, exp.nonce), (c.msg[:8], len(c.msg), c.lo, c.hi, c.env, n, "%016x" % x, got, exp)
            if c.lo <= n <= c.hi:
                assert got == (0, n), (c.msg[:8], len(c.msg), c.lo, c.hi, c.env, n, got)
            else:
                assert got[0] != 0 and c.lo <= got[1] <= c.hi, (c.msg[:8], c.lo, c.hi, c.env, n, got)
    return kernels


# ---- probe sets (host only) ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fast_kernel_cases():
    """{(J, mode, L env): Case}: test_every_kernel_instantiation's range of every fast kernel at
    MINEHIP_LOWER_DIGITS 1 and 3.  Probes: the range's edges, each plan piece's first and last
    nonce, per fast piece first + k 10^L - 1 and first + k 10^L for the lane, wave, chunk and
    ragged-last-lane boundaries k of the last-digit layouts (more samples of the Early ones), and
    RANDOM_FAST[L] nonces of the fast pieces."""
    from test_abi import KERNEL_CASE_NONCES, kernel_cases
    rng = random.Random(4401)
    out = {}
    for (J, mode), (m, lo, _, early) in sorted(kernel_cases().items()):
        hi = lo + KERNEL_CASE_NONCES + 3_456
        for Ld in (1, 3):
            env = dict(MINEHIP_LOWER_DIGITS=Ld, MINEHIP_MIN_LANES=1, MINEHIP_GENERIC_BELOW=0, MINEHIP_EARLY=early)
            pieces = planned(m, lo, hi, env)
            fast = [pc for pc in pieces if pc["kind"] == 0]
            pos, neg = edges(lo, hi)
            pos |= seam_probes(pieces)
            for pc in fast:
                R = 10 ** pc["lo_digits"]
                for k in LANE_KS + (pc["count"] // R - 1,):
                    pos |= {n for n in (pc["first"] + k * R - 1, pc["first"] + k * R) if pc["first"] <= n <= last_of(pc)}
            pos |= draw(rng, fast, RANDOM_FAST[Ld])
            # the case's own kernel may hold a small bucket of the range only: at least 60 probes in its pieces
            own = [pc for pc in fast if (pc["word"], pc["mode"]) == (J, mode)]
            while sum(pc["first"] <= n <= last_of(pc) for n in pos for pc in own) < min(60, sum(pc["count"] for pc in own)):
                pos |= draw(rng, own, 1)
            # ... and every digit value at each of the low L + 2 decimal places (60 draws can miss one)
            Lmax = max(pc["lo_digits"] for pc in fast)
            while any({n // 10 ** k % 10 for n in pos if any(pc["first"] <= n <= last_of(pc) for pc in fast)} != set(range(10))
                      for k in range(Lmax + 2)):
                pos |= draw(rng, fast, 1)
            out[(J, mode, Ld)] = Case(msg=m, lo=lo, hi=hi, env=env, pieces=pieces, pos=pos, neg=neg)
    return out


@functools.lru_cache(maxsize=None)
def lane_cases():
    """{(J, mode): Case}: the same ranges at MINEHIP_LOWER_DIGITS=2, where a lane enumerates 100
    nonces: every (g, i) pair of one lane of the case's kernel (drawn at random), so a defect in one
    pair, which the random draws above meet with probability 1 / 10^L each, is met for certain
    where g has one digit.  A last-digit lane is 100 consecutive nonces; an Early lane's are 10^p
    apart (g and i are the digits at decimal positions p + 1 and p)."""
    from test_abi import KERNEL_CASE_NONCES, kernel_cases
    rng = random.Random(4405)
    out = {}
    for (J, mode), (m, lo, _, early) in sorted(kernel_cases().items()):
        hi = lo + KERNEL_CASE_NONCES + 3_456
        env = dict(MINEHIP_LOWER_DIGITS=2, MINEHIP_MIN_LANES=1, MINEHIP_GENERIC_BELOW=0, MINEHIP_EARLY=early)
        pieces = planned(m, lo, hi, env)
        own = [pc for pc in pieces if pc["kind"] == 0 and (pc["word"], pc["mode"], pc["lo_digits"]) == (J, mode, 2)]
        if not own:
            continue
        pc = max(own, key=lambda pc: pc["count"])
        p = early_pos(m, pc) if mode >= 3 else 0
        block = 10 ** (p + 2)
        base = pc["first"] + rng.randrange(pc["count"] // block) * block + rng.randrange(10 ** p)
        pos, neg = edges(lo, hi)
        out[(J, mode)] = Case(msg=m, lo=lo, hi=hi, env=env, pieces=pieces, pos=pos | {base + q * 10 ** p for q in range(100)},
                              neg=neg, piece=pc, p=p)
    return out


@functools.lru_cache(maxsize=None)
def early_cases():
    """{slot: Case} over test_gpu_ties.early_tie_cases(): each Early kernel with contiguous and
    interleaved lanes, plus the top of u64 (hi = 2^64 - 1: no hi + 1 probe).  Probes: edges, piece
    seams, RANDOM_EARLY nonces of the range."""
    rng = random.Random(4402)
    out = {}
    for slot, (m, lo, hi, Ld, p, L) in sorted(early_tie_cases().items(), key=str):
        env = dict(MINEHIP_LOWER_DIGITS=Ld, MINEHIP_MIN_LANES=1, MINEHIP_GENERIC_BELOW=0)
        pieces = planned(m, lo, hi, env)
        pos, neg = edges(lo, hi)
        pos |= seam_probes(pieces) | {rng.randrange(lo, hi + 1) for _ in range(RANDOM_EARLY)}
        out[slot] = Case(msg=m, lo=lo, hi=hi, env=env, pieces=pieces, pos=pos, neg=neg, p=p, L=L)
    return out


@functools.lru_cache(maxsize=None)
def batch_calls():
    """(requests, kinds, probes): test_gpu_batch's EDGES, 60 fuzz requests, ten multi-tile requests of
    20,000 nonces and the 200,000-nonce fallback of test_gpu_ties.batch_requests(); probes are
    (request index, nonce): per request lo, hi, lo - 1, hi + 1 (the partial first and last decade),
    per multi-tile request both sides of every tile seam and RANDOM_TILES nonces."""
    from test_gpu_batch import EDGES, fuzz_requests
    from test_gpu_ties import batch_requests
    allreqs = batch_requests()
    multi = [r for r in allreqs if r[0].startswith(b"tiles")][:10]
    reqs = list(EDGES) + fuzz_requests(n=60) + multi + [allreqs[-1]]
    assert reqs[-1] == (b"fallback", 5, 200_004) and len(multi) == 10
    rng = random.Random(4404)
    probes = []
    for i, (m, lo, hi) in enumerate(reqs):
        pos, neg = edges(lo, hi)
        if (m, lo, hi) in multi:
            u0 = lo // 10
            seams = [(u0 + 256 * k) * 10 for k in range(1, (hi // 10 - u0) // 256 + 1)]
            pos |= {n for s in seams for n in (s - 1, s)} | {rng.randrange(lo, hi + 1) for _ in range(RANDOM_TILES)}
        probes += [(i, n) for n in sorted(pos) + sorted(neg)]
    return reqs, [0] * (len(reqs) - 1) + [1], probes


# ---- CPU tests -------------------------------------------------------------------------------------

def test_probe_sets_cover():
    """The coverage conditions of the probe sets, from the sets alone (no GPU, no hashes).
    Digits: a fast kernel places the L enumerated digits and the lowest digits of U by byte
    position, so every value 0-9 must be probed at each of the low L + 2 decimal digits (Early
    cases: the low p + L, the enumerated digits and the U digits below them); with >= 60 random
    draws a value is missed at a position with probability 10 x 0.9^60 < 2%, and the seeds are
    fixed.  Chunks: probes in three different chunks wherever the fast pieces have three (at L = 1
    the 253,456 nonces are 99 chunks; at L = 3 they are one, and the range cannot hold more)."""
    from test_abi import KERNELS
    cases = fast_kernel_cases()
    assert {k[:2] for k in cases} == KERNELS and len(cases) == 2 * len(KERNELS)
    for (J, mode, Ld), c in cases.items():
        fast = [pc for pc in c.pieces if pc["kind"] == 0]
        # the case's kernel runs at L = 1; at MINEHIP_LOWER_DIGITS=3 <0, OneEarly> has no plan (its
        # range then runs <1, One>), as in test_every_kernel_instantiation
        assert any((pc["word"], pc["mode"]) == (J, mode) for pc in fast) or (Ld == 3 and (J, mode) == (0, 3)), (J, mode, Ld)
        assert c.neg == {c.lo - 1, c.hi + 1} and {c.lo, c.hi} <= c.pos
        assert seam_probes(c.pieces) <= c.pos
        infast = [(pc, n) for n in c.pos for pc in fast if pc["first"] <= n <= last_of(pc)]
        own = [n for pc, n in infast if (pc["word"], pc["mode"]) == (J, mode)]
        assert len(own) >= min(60, sum(pc["count"] for pc in fast if (pc["word"], pc["mode"]) == (J, mode))), (J, mode, Ld)
        L = max(pc["lo_digits"] for pc in fast)
        for k in range(L + 2):
            assert {n // 10 ** k % 10 for _, n in infast} == set(range(10)), (J, mode, Ld, k)
        have = sum(-(-pc["count"] // 10 ** pc["lo_digits"] // 256) for pc in fast)
        assert Ld != 1 or have >= 3
        assert len({(pc["first"], chunk_of(c.msg, pc, n)) for pc, n in infast}) >= min(3, have), (J, mode, Ld)
        # the ragged last chunk's last valid lane, and the lane after a full wave and a full chunk
        for pc in fast:
            R = 10 ** pc["lo_digits"]
            assert last_of(pc) in c.pos and last_of(pc) - R + 1 in c.pos
            assert all(pc["first"] + k * R in c.pos for k in (64, 256) if k * R < pc["count"])
    lc = lane_cases()
    # <0, One> holds the buckets d <= 4 and <0, OneEarly> d <= 5 of their range: lanes of 100 nonces
    # only in pieces of 900 and 90,000 nonces, which is enough; <0, Pre>'s range plans no lane of 100
    assert set(lc) == KERNELS - {(0, 1)}, sorted(KERNELS - set(lc))
    for (J, mode), c in lc.items():
        pc, inpc = c.piece, [n for n in c.pos if c.piece["first"] <= n <= last_of(c.piece)]
        lanes = collections.Counter((n // 10 ** (c.p + 2), n % 10 ** c.p) for n in inpc)
        (lane, cnt), = lanes.most_common(1)
        assert cnt >= 100 and {n // 10 ** c.p % 100 for n in inpc
                               if (n // 10 ** (c.p + 2), n % 10 ** c.p) == lane} == set(range(100)), (J, mode)
    ec = early_cases()
    assert sum(c.hi == U64 for c in ec.values()) >= 1
    for slot, c in ec.items():
        assert {c.lo, c.hi} <= c.pos and seam_probes(c.pieces) <= c.pos
        assert c.neg == ({c.lo - 1} | ({c.hi + 1} if c.hi < U64 else set())), slot
        fast = [pc for pc in c.pieces if pc["kind"] == 0 and pc["mode"] >= 3]
        infast = [(pc, n) for n in c.pos for pc in fast if pc["first"] <= n <= last_of(pc)]
        for k in range(c.p + c.L):
            assert {n // 10 ** k % 10 for _, n in infast} == set(range(10)), (slot, k)
        have = sum(-(-pc["count"] // 10 ** pc["lo_digits"] // 256) for pc in fast)
        assert have >= 1
        assert len({(pc["first"], chunk_of(c.msg, pc, n)) for pc, n in infast}) >= min(3, have), slot
    reqs, kinds, probes = batch_calls()
    by_req = {}
    for i, n in probes:
        by_req.setdefault(i, set()).add(n)
    assert any(lo == 0 for _, lo, _ in reqs) and any(hi == U64 for _, _, hi in reqs)
    for i, (m, lo, hi) in enumerate(reqs):
        pos, neg = edges(lo, hi)
        assert pos | neg <= by_req[i], (i, lo, hi)
        assert (lo == 0) == (lo - 1 not in by_req[i]) and (hi == U64) == (hi + 1 not in by_req[i])
        if m.startswith(b"tiles"):     # 20,000 nonces: eight or nine tiles, both sides of every seam
            inside = sorted(n for n in by_req[i] if lo <= n <= hi)
            tiles = {(n // 10 - lo // 10) // 256 for n in inside}
            assert tiles == set(range((hi // 10 - lo // 10) // 256 + 1)) and len(tiles) >= 8
            assert sum(b - a == 1 and (b // 10 - lo // 10) % 256 == 0 and b % 10 == 0
                       for a, b in zip(inside, inside[1:])) == len(tiles) - 1
    # partial first and last decades are exercised: some lo is no multiple of ten, some hi not 9 mod 10
    assert sum(lo % 10 != 0 for _, lo, _ in reqs) > 20 and sum(hi % 10 != 9 for _, _, hi in reqs) > 20


# ---- GPU tests -------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_every_fast_kernel_probes(gpu, tmp_path):
    """Each of the 26 fast_search<J, MODE> kernels at L = 1 and 3: edges, seams, lane / wave / chunk
    boundaries, the ragged last lane and random nonces, each hashed right, considered and rebuilt;
    at L = 2 every (g, i) pair of one lane."""
    from test_abi import KERNELS
    kernels = run_cases(tmp_path, list(fast_kernel_cases().values()) + list(lane_cases().values()), profile=True)
    assert kernels == KERNELS


@pytest.mark.gpu
def test_early_positions_probes(gpu, tmp_path):
    """The Early layouts, where spread(...) rebuilds a candidate's nonce and lanes interleave."""
    run_cases(tmp_path, list(early_cases().values()))


# test_gpu_ties.test_generic_path_and_edges' messages and ranges
GENERIC_MSGS = (b"cmu440", b"", b"q" * 60, b"r" * 119)
GENERIC_RANGES = ((0, 25_000), (U64 - 30_000, U64), (3, 9_012), (10 ** 5 - 7_000, 10 ** 5 + 9_000),
                  (10 ** 19 - 7_000, 10 ** 19 + 9_000))


def generic_cases():
    rng = random.Random(4403)
    out = []
    for m in GENERIC_MSGS:
        for lo, hi in GENERIC_RANGES:
            pieces = planned(m, lo, hi, {})
            pos, neg = edges(lo, hi)
            pos |= seam_probes(pieces)
            pos |= {n for k in range(20) for n in (10 ** k - 1, 10 ** k) if lo <= n <= hi}
            for pc in pieces:   # generic_scan: one nonce per lane, 256-lane blocks from the piece's first
                pos |= {pc["first"] + 256 * b - d for b in range(1, pc["count"] // 256 + 1) for d in (1, 0)
                        if pc["first"] + 256 * b - d <= last_of(pc)}
            pos |= {rng.randrange(lo, hi + 1) for _ in range(RANDOM_GENERIC)}
            out.append(Case(msg=m, lo=lo, hi=hi, env={}, pieces=pieces, pos=pos, neg=neg))
    return out


@pytest.mark.gpu
def test_generic_and_edges_probes(gpu, tmp_path):
    """The default plan (generic_scan on these ranges): edges, every 10^k - 1 | 10^k, the last lane
    of each full 256-lane block and the first of the next, random nonces.  And single-nonce ranges
    [n, n] under x = ~Hash(msg, n): the all-ones hash equals the kernels' empty-lane sentinel and
    must still come back with its nonce."""
    cases = generic_cases()
    assert all(pc["kind"] == 1 for c in cases for pc in c.pieces)
    assert sum(len(c.pos) for c in cases) > 2_000
    run_cases(tmp_path, cases)
    singles = [0, 7, 9, 10, 255, 256, 99_999, 10 ** 19 - 1, 10 ** 19, U64 - 1, U64]
    jobs = [job(m, n, n, FULL, xors=[hashes_of(m, n, n, [n])[0] ^ U64]) for m in GENERIC_MSGS for n in singles]
    results, _ = run_jobs(tmp_path, jobs)
    check_jobs(jobs, results)
    assert [tuple(r) for r in results] == [(U64, n) for _ in GENERIC_MSGS for n in singles]


@pytest.mark.gpu
def test_batch_probes(gpu, tmp_path):
    """search_batch: one call per probe, x the hash of one nonce of one request; that request must
    return (0, n*) (or, probed just outside, its non-zero minimum) and every other request of the
    call its own minimum under x.  Partial first and last decades, tile seams, decade 0, the top of
    u64, several passes and the fallback search."""
    reqs, kinds, probes = batch_calls()
    xs = [hashes_of(reqs[i][0], reqs[i][1], reqs[i][2], [n])[0] for i, n in probes]
    jobs = [dict(call="batch", reqs=[(m.hex(), lo, hi) for m, lo, hi in reqs], kinds=kinds,
                 keeps=[list(p) for p in FULL], envs=[{}], xors=xs)]
    results, _ = run_jobs(tmp_path, jobs, MINEHIP_BATCH_SLOTS=BATCH_SLOTS)
    assert len(results) == len(probes)
    for (i, n), x, got in zip(probes, xs, results):
        assert len(got) == len(reqs)
        for r, ((m, lo, hi), g) in enumerate(zip(reqs, got)):
            exp = masked_min(m, lo, hi, 32, 32, x)
            assert tuple(g) == (exp.hash, exp.nonce), (r, m[:8], lo, hi, "probe", i, n, g, exp)
        lo, hi = reqs[i][1:]
        if lo <= n <= hi:
            assert tuple(got[i]) == (0, n), (i, n, got[i])
        else:
            assert got[i][0] != 0 and lo <= got[i][1] <= hi, (i, n, got[i])


def seam_cases():
    """test_gpu_ties.test_plans_and_host_merges' two ranges under four of its cut environments.
    Probes: edges, both sides of every plan piece seam and of every MINEHIP_LAUNCH_NONCES multiple
    from a piece's first nonce."""
    fast = dict(MINEHIP_MIN_LANES=1, MINEHIP_GENERIC_BELOW=0)
    envs = [dict(fast, MINEHIP_LOWER_DIGITS=3, MINEHIP_LAUNCH_NONCES=100_000, MINEHIP_STREAMS=1, MINEHIP_FINE_TAIL=0,
                 MINEHIP_QUEUE=0),
            dict(fast, MINEHIP_LOWER_DIGITS=3, MINEHIP_LAUNCH_NONCES=100_000, MINEHIP_STREAMS=2, MINEHIP_FINE_TAIL=20_000,
                 MINEHIP_QUEUE=1),
            dict(fast, MINEHIP_LOWER_DIGITS=1, MINEHIP_MAX_BLOCKS=1, MINEHIP_QUEUE=0, MINEHIP_STREAMS=2,
                 MINEHIP_FINE_TAIL=20_000),
            dict(fast, MINEHIP_LOWER_DIGITS=2, MINEHIP_MAX_BLOCKS=1, MINEHIP_QUEUE=1, MINEHIP_STREAMS=2,
                 MINEHIP_FINE_TAIL=20_000)]
    ranges = ((b"cmu440", 5 * 10 ** 8, 5 * 10 ** 8 + 250_000), (b"x" * 60, 10 ** 9 - 120_000, 10 ** 9 + 130_000))
    cases, multi = [], []
    for m, lo, hi in ranges:
        for env in envs:
            pieces = planned(m, lo, hi, env)
            pos, neg = edges(lo, hi)
            for pc in pieces:
                cuts = {pc["first"], last_of(pc) + 1}
                cuts |= set(range(pc["first"], last_of(pc) + 1, env.get("MINEHIP_LAUNCH_NONCES", pc["count"])))
                pos |= {n for s in cuts for n in (s - 1, s) if lo <= n <= hi}
            cases.append(Case(msg=m, lo=lo, hi=hi, env=env, pieces=pieces, pos=pos, neg=neg))
        pos, neg = edges(lo, hi)     # search_multi's host chunks: 12,345 nonces each from lo
        pos |= {n for s in range(lo + 12_345, hi + 1, 12_345) for n in (s - 1, s)}
        # at L = 1 a host chunk is a fast piece between generic edges (at L = 3 its 12 lanes of 1,000
        # nonces would take 2.9 ms per chunk, 60 ms per search)
        multi.append(Case(msg=m, lo=lo, hi=hi, env=dict(fast, MINEHIP_LOWER_DIGITS=1), pieces=[], pos=pos, neg=neg))
    return cases, multi


@pytest.mark.gpu
def test_plan_and_host_seam_probes(gpu, tmp_path):
    """Both sides of every seam between plan pieces, launches and search_multi's host chunks."""
    cases, multi = seam_cases()
    assert max(len(c.pieces) for c in cases) >= 90 and all(len(c.pieces) >= 3 for c in cases)
    assert all(len(c.pos) >= 2 * 20 for c in multi)
    run_cases(tmp_path, cases)
    run_cases(tmp_path, multi, call="multi", devs=[0, 0, 0], chunk=12_345)


@pytest.mark.gpu
def test_guard_refuses_xor_without_the_symbol(gpu):
    """MINEHIP_DEV_HASH_XOR with the embedded code object (its kernels have no mh_dev_hash_xor): a
    search with a fast piece fails loudly instead of mixing XORed generic pieces with plain fast
    ones, and so does a malformed value; the next search without the variable is the product's."""
    lo, hi = 10 ** 9, 10 ** 9 + 199_999
    r = run_dev(f"""
import os, minehip
assert minehip.LIB_PATH.endswith("build/dev/libminehip.so"), minehip.LIB_PATH
assert "MINEHIP_DEV_CODE_OBJECT" not in os.environ
os.environ.update(MINEHIP_GENERIC_BELOW="0", MINEHIP_MIN_LANES="1")
assert any(p["kind"] == 0 for p in minehip.plan(b"cmu440", {lo}, {hi}))
for v in ("1", "8000000000000000", "ffffffffffffffff", "DEADBEEF",        # set, no symbol
          "10000000000000000", "0x12", "12g", "1 ", " 1", "-1", "1,2", "x"):  # malformed
    os.environ["MINEHIP_DEV_HASH_XOR"] = v
    try:
        minehip.search(b"cmu440", {lo}, {hi})
        raise SystemExit("searched with MINEHIP_DEV_HASH_XOR=" + v)
    except minehip.MinehipError as e:
        assert e.code == minehip.MH_EINVAL and "MINEHIP_DEV_HASH_XOR" in str(e), e
os.environ["MINEHIP_DEV_HASH_XOR"] = "0"      # zero is off
print(*minehip.search(b"cmu440", {lo}, {hi}))
del os.environ["MINEHIP_DEV_HASH_XOR"]
print(*minehip.search(b"cmu440", {lo}, {hi}))
""", timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in r.stdout.split()[-4:]]
    exp = oracle.search(b"cmu440", lo, hi, threads=4)
    assert tuple(got[:2]) == tuple(got[2:]) == masked_min(b"cmu440", lo, hi, 32, 32)[:2] == exp
