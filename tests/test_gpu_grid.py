"""Every nonce at every tail offset, digit count and lane length, through all ten builds of
fast_search.hip.

Inside one fast_search<J, MODE> the kernel still works on runtime values -- hi_end, lo_pos, n_hi, L,
inner, hole, g_last, g_hole: the byte of every digit of the lane number U, whether a group digit
goes to word J or word J - 1, and the shift of the per-nonce digit.  The per-layout tests
(test_gpu_probe.py, test_gpu_dense.py, test_gpu_first_probe.py, ...) run each layout over one
message and one range, test_abi.kernel_cases()': 19 of the 26 layouts only with the last digit at
byte 0 of word J, 21 of the 26 with d = 20 and lo = 10^19, where every digit of U above the sixth
place is '0' and a wrong byte position for it adds 0 << shift to a template that already holds '0'.

tests/grid_cases.py builds the grid that closes this: 64 messages x 19 digit counts, ranges of up to
5,201 nonces whose U has non-zero digits at every place, the top of u64 per message, each under
MINEHIP_LOWER_DIGITS 1, 2 and 3, again with MINEHIP_EARLY=0 where an Early layout took the cell, plus
the Early position cases of up to 203,457 nonces.  test_grid_rests_on asserts from the plans alone
what that reaches: every last-digit layout at every byte alignment it can have, both routes of the
group digits, every Early (J, mode, p, L) with p + L <= 5.

  dense       hits_scan, hits_stop, batch_hits, batch_bound: target 2^64 - 1, every (hash, nonce) of
              every cell bit for bit the oracle's (test_gpu_ties.full_hashes), as test_gpu_dense.py
  edge probes first_scan, stop_scan, batch_first, batch_stop: the four lowest hashes of each cell's
              fast pieces, each made the answer by moving the lower edge, target T and T - 1, as
              test_gpu_first_probe.py
  XOR probes  fast_search, batch_fast (dev build): piece ends, random nonces and lo - 1 / hi + 1 of
              each cell, against masked_min(..., x), as test_gpu_probe.py / test_gpu_batch_fast.py

A mismatch names the cell (n, t, d, alignment, range), the environment, the plan piece's layout and L,
lane, group and digit, and the tail byte of each digit of U.  No cell is skipped at run time: what a
test cannot use is left out in grid_cases.py and counted in the host tests -- the Early position
cases run in the dense tests only (the probes take the 1,280 grid cells and their MINEHIP_EARLY=0
reruns); of the grid's moved-edge candidates 15,166 are kept, and mh_batch_plan_ex drops none.

A search at L = 3 runs a lane of 1,000 nonces whatever the range (about 3 ms against 0.15 ms at
L = 1), so the tests take the runs of L = 3, and some of L = 2, in several parts ([part::parts]).

Measured on an MI355X (one run each), seconds per test case.  The first test to run also computes
the oracle's hashes of every cell and Early case (3 s, shared by the others); the host tests take
16 s together, most of it those hashes and the probe sets:
  hits_scan    L1 2.8 (with the hashes)  L2 2.2  L3 2 x 3.0
  hits_stop    L1 2.6   L2 3 x 3.2-3.7   L3 5 x 4.0-4.2
  batch_hits   L1 0.3   L2 0.8   L3 1.8      batch_bound  L1 1.0   L2 3.9   L3 2 x 3.1-3.3
  first_scan   L1 1.9   L2 4.5   L3 6 x 4.0-4.4 (11,012 / 10,408 / 8,912 searches per L)
  stop_scan    L1 1.4   L2 4.0   L3 6 x 4.0-4.2
  batch_first  L1 0.1   L2 0.4   L3 2.1      batch_stop   L1 0.1   L2 0.3   L3 2.0
  fast_search XOR probes  L1 1.6   L2 3.7   L3 8 x 3.0-3.1
  batch_fast XOR probes   L1 2.4   L2 2 x 3.5   L3 10 x 4.3-4.5 (one of them 5.8)
65 GPU cases, 209 s in all.
"""
import collections
import ctypes

import numpy as np
import pytest

import grid_cases as g
from grid_cases import LDS, U64, N_of, cell_env, hashes, name
from test_gpu_dense import check_all_hits, check_first_k, first_min, hit_buffer
from test_gpu_first_probe import check_probe, expect, probe_of
from test_gpu_parity import env
from test_gpu_probe import Case, hashes_of, last_of
from test_gpu_ties import masked_min

MAIN, TOPS = 1_216, 64


def parts_of(parts_by_L):
    """([(Ld, part, parts)], ids) of a test that takes the runs of each L in parts_by_L[L] parts."""
    ps = [(Ld, part, parts_by_L[Ld]) for Ld in LDS for part in range(parts_by_L[Ld])]
    return ps, ["L%d" % Ld if n == 1 else "L%d-%dof%d" % (Ld, part + 1, n) for Ld, part, n in ps]


def where(c, Ld, early, pieces, nonce):
    """The cell, its environment, and the plan piece, lane, group and digit of one nonce."""
    s = name(c, Ld, early)
    p = g.piece_of(pieces, nonce)
    if p is None or p["kind"] == 1:
        return s + ", nonce %d in %s" % (nonce, "a generic piece" if p else "no plan piece")
    R = 10 ** p["lo_digits"]
    return s + ", nonce %d in <%d, %d> L = %d (first %d count %d): lane %d, group %d, digit %d" % (
        nonce, p["word"], p["mode"], p["lo_digits"], p["first"], p["count"], nonce // R - p["first"] // R,
        nonce % R // 10, nonce % 10)


# ---- CPU tests -------------------------------------------------------------------------------------

def test_grid_rests_on():
    """What the GPU tests rest on, from minehip.plan, batch_plan_ex, hits_batch_regions and
    first_hits_batch_regions alone."""
    import minehip
    from test_abi import KERNELS
    main, tops = g.main_cells(), g.top_cells()
    assert (len(main), len(tops)) == (MAIN, TOPS) and sum(map(N_of, main)) == 5_722_048
    assert all(N_of(c) <= 5_201 for c in main + tops) and all(c.hi == U64 and N_of(c) == 5_201 for c in tops)
    assert {g.t_of(c) for c in main if c.d == 9} == set(range(64))
    for c in main:
        assert len(str(c.lo)) == len(str(c.hi)) == c.d
        if c.d >= 6:    # U's places from 10^4 up are non-zero in all but the first 37 nonces, the edges ragged
            assert "0" not in str(c.hi // 10 ** 4) and (c.lo + 37) // 10 ** 4 == c.hi // 10 ** 4, c
            assert c.lo % 1000 not in (0, 999) and c.hi % 1000 not in (0, 999), c
    early_layouts = {k for k in KERNELS if k[1] >= 3}
    assert len(KERNELS) == 26 and len(early_layouts) == 4
    # ---- fast pieces, layouts, alignments, group-digit routes
    reached = {}
    for Ld in LDS:
        for early in (1, 0):
            plans = g.grid_plans(Ld, early)
            assert len(plans) == MAIN + TOPS and all(g.fast_pieces(p) for p in plans.values()), (Ld, early)
            for c, pieces in plans.items():
                assert sum(p["count"] for p in pieces) == N_of(c) and {p["kind"] for p in pieces} <= {0, 1}
            reached[(Ld, early)] = g.coverage(Ld, early)
        assert reached[(Ld, 1)][0] == (KERNELS if Ld < 3 else KERNELS - early_layouts), Ld
        assert reached[(Ld, 0)][0] == KERNELS - early_layouts, Ld
        # MINEHIP_EARLY=0 runs again exactly the cells with an Early piece
        again = g.early_cells(Ld)
        assert len(again) == {1: 111, 2: 54, 3: 0}[Ld], (Ld, len(again))
        assert all(g.early_pieces(g.grid_plans(Ld, 1)[c]) and not g.early_pieces(g.grid_plans(Ld, 0)[c]) for c in again)
    aligns = collections.defaultdict(set)
    for (Ld, early), (_, al, _r) in reached.items():
        for k, v in al.items():
            aligns[k] |= v
    special = {(0, 0): {1, 2, 3}, (4, 1): {0, 1, 2}, (13, 0): {0, 1, 2}, (13, 2): {3}}
    for k in KERNELS:
        assert aligns[k] == ({0, 1} if k in early_layouts else special.get(k, {0, 1, 2, 3})), (k, aligns[k])
    for Ld in LDS:      # every alignment of every last-digit layout at each L on its own, too
        al = collections.defaultdict(set)
        for early in (1, 0):
            for k, v in reached[(Ld, early)][1].items():
                al[k] |= v
        assert all(al[k] == aligns[k] for k in KERNELS - early_layouts), Ld
    # L = 2 and 3: both routes of the group digits (all in word J; one in word J - 1) for every
    # last-digit layout with J > 0.  <13, Two> is the one that has a single route: its last digit
    # sits at byte 3 of word 13 (its only alignment), so up to three group digits stay in word 13
    for Ld in (2, 3):
        routes = collections.defaultdict(set)
        for early in (1, 0):
            for k, v in reached[(Ld, early)][2].items():
                routes[k] |= v
        for k in KERNELS - early_layouts:
            if k[0] == 0:
                assert routes[k] == {frozenset({0})}, (Ld, k, routes[k])
            elif k == (13, 2):
                assert routes[k] == {frozenset({0})}, (Ld, k, routes[k])
            else:
                assert frozenset({0}) in routes[k] and any(-1 in r for r in routes[k]), (Ld, k, routes[k])
    # ---- the Early position cases: every (J, mode, p, L) with p + L <= 5 is kept
    from test_gpu_parity import early_position_cases
    cases, dropped = g.early_cases()
    keys = {k[:4] for k in early_position_cases(Ls=LDS) if k[2] + k[3] <= g.EARLY_MAX}
    assert dropped == g.EARLY_DROPPED == {} and {c.key for c in cases} == keys and len(keys) == 36
    assert len(cases) == 63 and sum(c.hi == U64 for c in cases) == 27       # <0, OneEarly> has d <= 8: no top case
    assert {c.key[:2] for c in cases} == early_layouts and max(map(N_of, cases)) == 203_457 < g.HIT_BUFFER
    assert all("0" not in str(c.lo // 10 ** sum(c.key[2:])) for c in cases if c.hi < U64)   # U's digits above the block
    # ---- the batched calls
    for Ld in LDS:
        single = {(c, early): pieces for c, early, pieces in g.runs(Ld)}
        groups = g.batch_groups(Ld)
        assert sum(len(cs) for _, cs, _ in groups) == len(single)        # every run is in exactly one call
        same = 0
        for early, cs, per in groups:
            assert len({p["pass"] for pieces in per for p in pieces}) == 1, (Ld, early, cs[0].d)     # one pass
            for c, pieces in zip(cs, per):
                assert {p["kind"] for p in pieces} <= {0, 2} and sum(p["count"] for p in pieces) == N_of(c)
                fused = sorted((p["word"], p["mode"], p["lo_digits"], p["first"], p["count"]) for p in pieces if p["kind"] == 2)
                alone = sorted((p["word"], p["mode"], p["lo_digits"], p["first"], p["count"])
                               for p in g.fast_pieces(single[(c, early)]))
                assert fused == alone and fused, (Ld, name(c, Ld, early))
                same += c.kind == "main" and early == 1
            with env(**cell_env(Ld, early)):
                want = [(0, 0, N_of(c)) for c in cs]
                regs = minehip.hits_batch_regions([(c.msg, c.lo, c.hi, U64, N_of(c)) for c in cs], fuse_fast=True)
                assert [(r["kind"], r["window"], r["slots"]) for r in regs] == want, (Ld, early, cs[0].d)
                for half in (False, True):
                    regs = minehip.first_hits_batch_regions(
                        [(c.msg, c.lo, c.hi, U64, N_of(c) // 2 if half else N_of(c)) for c in cs], fuse_fast=True)
                    assert [(r["kind"], r["window"], r["slots"]) for r in regs] == want, (Ld, early, cs[0].d, half)
        assert same == MAIN


def test_edge_probe_sets():
    """The moved-edge probes of the first-hit builds, from the plans and the oracle alone: every cell
    keeps its first minimum, at L = 1 and 2 every main cell keeps at least two probes, the main cells
    keep 4,808 / 4,739 / 4,241 probes at L = 1 / 2 / 3 (floor 4,000), every top cell keeps its first
    minimum, and mh_batch_plan_ex fuses every kept probe's request.  And the expectation itself: a
    flipped bit of the reference's hash of a probed nonce changes what is expected of that probe."""
    total = 0
    for Ld in LDS:
        sets = g.edge_probes(Ld)
        main = [(c, kept, first) for c, early, kept, first in sets if c.kind == "main" and early == 1]
        assert len(main) == MAIN and len([1 for c, early, *_ in sets if c.kind == "top" and early == 1]) == TOPS
        assert len(sets) == MAIN + TOPS + len(g.early_cells(Ld))
        for c, early, kept, first in sets:
            assert kept and kept[0].n == first, name(c, Ld, early)       # the first minimum of its fast pieces
            for p in kept:
                assert c.lo <= p.lower <= p.n <= c.hi and p.exp == (True, p.T, p.n)
                assert p.exp_below[2] > p.n if p.exp_below[0] else p.exp_below == (False, p.T, p.n)
        kept_main = sum(len(kept) for _, kept, _ in main)
        assert kept_main == {1: 4_808, 2: 4_739, 3: 4_241}[Ld] >= 4_000, (Ld, kept_main)
        assert min(len(kept) for _, kept, _ in main) >= (2 if Ld < 3 else 1), Ld
        batches = g.edge_probe_batches(Ld)
        assert sum(dropped for _, _, dropped in batches) == 0
        assert sum(len(ok) for _, ok, _ in batches) == sum(len(kept) for _, _, kept, _ in sets)
        total += sum(len(kept) for _, _, kept, _ in sets)
    assert total == 15_166
    c, early, kept, _ = g.edge_probes(2)[700]
    h, p = hashes(c), kept[-1]
    assert probe_of(h, c.lo, p.n) == (p.lower, p.T, p.exp, p.exp_below)
    flipped = h.copy()
    flipped[p.n - c.lo] ^= np.uint64(1 << 33)
    assert probe_of(flipped, c.lo, p.n)[2] != p.exp
    check_probe(p.exp + (p.n - p.lower + 1,), p.exp, p.lower, c.hi, "good")
    with pytest.raises(AssertionError) as e:
        checked_probe(p.exp + (p.n - p.lower + 1,), expect(flipped, c.lo, p.lower, p.T), c, 2, early, p, "first_scan")
    assert name(c, 2, early) in str(e.value) and "lane" in str(e.value)


def test_xor_probe_sets():
    """The XOR probes: per run the first and last nonce of each fast piece and lo - 1 / hi + 1 where
    they exist, at least two nonces of the fast pieces, and over the grid every digit value at each of
    the low L + 2 decimal places; the batched calls fuse the fast pieces of each of their requests."""
    import minehip
    for Ld in LDS:
        probes = g.xor_probes(Ld)
        assert len(probes) == MAIN + TOPS + len(g.early_cells(Ld))
        assert g.digits_probed(probes, Ld)
        for c, early, pieces, pos, neg in probes:
            fast = g.fast_pieces(pieces)
            assert {n for p in fast for n in (p["first"], last_of(p))} <= pos and len(pos) >= 2
            assert all(g.in_fast(pieces, n) for n in pos)
            assert neg == ({c.lo - 1} if c.lo else set()) | ({c.hi + 1} if c.hi < U64 else set())
        assert sum(len(neg) for *_x, neg in probes) >= 2 * MAIN + TOPS
        for early, cs, _ in xor_batch_groups(Ld):
            for i in range(len(cs)):
                call = batch_call(cs, i)
                with env(**cell_env(Ld, early)):
                    plan = minehip.batch_plan_ex([(c.msg, c.lo, c.hi) for c in call], fuse_fast=True)
                assert {p["kind"] for p in plan} <= {0, 2} and {p["req"] for p in plan if p["kind"] == 2} == set(range(len(call)))


def test_the_comparisons_fail_when_they_should():
    """grid_diff (test_gpu_dense.dense_diff with the cell named) and the check helpers: one flipped
    bit of one reference hash inside a fast piece, a shifted nonce and a short list are each
    reported, with the cell named."""
    Ld = 3
    c, early, pieces = next(r for r in g.runs(Ld) if r[0].kind == "main" and (r[0].n, r[0].d) == (22, 13))
    h = hashes(c)
    good = np.stack([h, np.uint64(c.lo) + np.arange(len(h), dtype=np.uint64)], axis=1)
    assert g.grid_diff(good, h, c, pieces, "same") is None
    fast = g.fast_pieces(pieces)[0]
    assert fast["lo_digits"] == 3 and fast["count"] >= 3_000
    n = fast["first"] + 2 * 1000 + 537           # lane 2, group 53, digit 7
    flipped = h.copy()
    flipped[n - c.lo] ^= np.uint64(1 << 17)
    rep = g.grid_diff(good, flipped, c, pieces, ("hits_scan", Ld, early))
    assert "1 of %d entries differ" % len(h) in rep and "index %d, nonce %d " % (n - c.lo, n) in rep, rep
    assert "<%d, %d> L = 3" % (fast["word"], fast["mode"]) in rep and "lane 2, group 53, digit 7" in rep, rep
    assert "n = 22 (t = 23), d = 13, alignment %d" % ((23 + 12) & 3) in rep and "U = %d" % (n // 1000) in rep, rep
    assert "k = 0: '%d' at byte %d" % (n // 1000 % 10, 23 + 12 - 3) in rep, rep
    wrong = good.copy()
    wrong[1000:, 1] += np.uint64(1)                  # a dropped nonce: everything after it shifts
    rep = g.grid_diff(wrong, h, c, pieces, "shifted")
    assert "%d of %d entries differ" % (len(h) - 1000, len(h)) in rep and "index 1000," in rep and name(c) in rep, rep
    rep = g.grid_diff(good[:-1], h, c, pieces, "short")
    assert "entries where" in rep and name(c) in rep, rep
    for bad_h, rows in ((flipped, good), (h, wrong), (h, good[:-1])):
        with pytest.raises(AssertionError) as e:
            checked_all_hits(rows, len(rows), len(rows), first_min(h, c.lo), bad_h, c, pieces, "hits_scan", Ld, early)
        assert name(c) in str(e.value)
    k = len(h) // 2
    with pytest.raises(AssertionError) as e:
        checked_first_k(good[:k], k, k, first_min(h[:k], c.lo), k, flipped, c, pieces, "hits_stop", Ld, early)
    assert name(c) in str(e.value) and "lane 2, group 53, digit 7" in str(e.value)
    checked_all_hits(good, len(h), len(h), first_min(h, c.lo), h, c, pieces, "hits_scan", Ld, early)
    checked_first_k(good[:k], k, k + 5, first_min(h[:k], c.lo), k, h, c, pieces, "hits_stop", Ld, early)
    assert "lane 2, group 53, digit 7" in where(c, Ld, early, pieces, n) and name(c, Ld, early) in where(c, Ld, early, pieces, n)


# ---- dense: the four hits builds ---------------------------------------------------------------------

def checked_all_hits(rows, count, stored, hn, h, c, pieces, build, Ld, early):
    rep = g.grid_diff(rows, h, c, pieces, (build, "L = %d" % Ld, "MINEHIP_EARLY=%d" % early))
    assert rep is None, rep
    check_all_hits(rows, count, stored, hn, h, c.lo, pieces, (build, name(c, Ld, early)))


def checked_first_k(rows, stored, scanned, hn, k, h, c, pieces, build, Ld, early):
    rep = g.grid_diff(rows, h[:k], c, pieces, (build, "L = %d" % Ld, "MINEHIP_EARLY=%d" % early, "k = %d" % k))
    assert rep is None, rep
    check_first_k(rows, stored, scanned, hn, k, h, c.lo, pieces, (build, name(c, Ld, early), "k = %d" % k))


DENSE_PARTS, DENSE_IDS = parts_of({1: 1, 2: 1, 3: 2})
STOP_PARTS, STOP_IDS = parts_of({1: 1, 2: 3, 3: 5})
BOUND_PARTS, BOUND_IDS = parts_of({1: 1, 2: 1, 3: 2})


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", DENSE_PARTS, ids=DENSE_IDS)
def test_hits_scan_every_nonce(gpu, Ld, part, parts):
    todo = g.runs(Ld)[part::parts]
    for c, early, pieces in todo:
        h, N = hashes(c), N_of(c)
        buf, ptr = hit_buffer(N)
        out = gpu.mh_hits()
        with env(**cell_env(Ld, early)):
            rc = gpu.lib.mh_search_hits(0, c.msg, len(c.msg), c.lo, c.hi, U64, ptr, N, ctypes.byref(out))
        assert rc == gpu.MH_OK, (name(c, Ld, early), gpu.lib.mh_last_error())
        checked_all_hits(buf[:out.stored], out.count, out.stored, (out.hash, out.nonce), h, c, pieces, "hits_scan", Ld, early)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", STOP_PARTS, ids=STOP_IDS)
def test_hits_stop_every_nonce(gpu, Ld, part, parts):
    for c, early, pieces in g.runs(Ld)[part::parts]:
        h, N = hashes(c), N_of(c)
        assert N <= gpu.MH_HITS_MAX_CAP          # no window walk can replace the kernels' own entries
        for k in (N, N // 2):
            buf, ptr = hit_buffer(k)
            out = gpu.mh_first_hits()
            with env(**cell_env(Ld, early)):
                rc = gpu.lib.mh_search_first_hits(0, c.msg, len(c.msg), c.lo, c.hi, U64, ptr, k, ctypes.byref(out))
            assert rc == gpu.MH_OK, (name(c, Ld, early), k, gpu.lib.mh_last_error())
            rows = buf[:out.stored]
            if k == N:
                checked_all_hits(rows, out.stored, out.stored, (out.hash, out.nonce), h, c, pieces, "hits_stop", Ld, early)
                assert out.scanned == N, (name(c, Ld, early), out.scanned)
            else:
                checked_first_k(rows, out.stored, out.scanned, (out.hash, out.nonce), k, h, c, pieces, "hits_stop", Ld, early)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_batch_hits_every_nonce(gpu, Ld):
    for early, cs, per in g.batch_groups(Ld):
        reqs = [(c.msg, c.lo, c.hi, U64, N_of(c)) for c in cs]
        arr, keep, offsets, total = gpu._hits_requests(reqs, 0)
        assert total == sum(map(N_of, cs)) <= gpu.MH_HITS_MAX_CAP
        buf, ptr = hit_buffer(total)
        out = (gpu.mh_hits_result * len(cs))()
        with env(**cell_env(Ld, early)):
            rc = gpu.lib.mh_search_hits_batch_ex(0, arr, len(cs), gpu.MH_BATCH_FUSE_FAST, ptr, total, out)
        assert rc == gpu.MH_OK, (Ld, early, cs[0].d, gpu.lib.mh_last_error())
        for c, pieces, o, off in zip(cs, per, out, offsets):
            assert o.status == gpu.MH_OK and o.offset == off, (name(c, Ld, early), o.status, o.offset)
            checked_all_hits(buf[off:off + o.stored], o.count, o.stored, (o.hash, o.nonce), hashes(c), c, pieces,
                             "batch_hits", Ld, early)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", BOUND_PARTS, ids=BOUND_IDS)
def test_batch_bound_every_nonce(gpu, Ld, part, parts):
    for early, cs, per in g.batch_groups(Ld)[part::parts]:
        for half in (False, True):
            ks = [N_of(c) // 2 if half else N_of(c) for c in cs]
            reqs = [(c.msg, c.lo, c.hi, U64, k) for c, k in zip(cs, ks)]
            arr, keep, offsets, total = gpu._first_hits_requests(reqs)
            buf, ptr = hit_buffer(total)
            out = (gpu.mh_first_hits_result * len(cs))()
            with env(**cell_env(Ld, early)):
                rc = gpu.lib.mh_search_first_hits_batch(0, arr, len(cs), gpu.MH_BATCH_FUSE_FAST, ptr, total, out)
            assert rc == gpu.MH_OK, (Ld, early, cs[0].d, half, gpu.lib.mh_last_error())
            for c, pieces, k, o, off in zip(cs, per, ks, out, offsets):
                assert o.status == gpu.MH_OK and o.offset == off, (name(c, Ld, early), k, o.status, o.offset)
                assert o.path == 0, (name(c, Ld, early), k, o.path)      # the fused pass's own entries, not a rebuild
                h, rows = hashes(c), buf[off:off + o.stored]
                if not half:
                    checked_all_hits(rows, o.stored, o.stored, (o.hash, o.nonce), h, c, pieces, "batch_bound", Ld, early)
                    assert o.scanned == N_of(c), (name(c, Ld, early), o.scanned)
                else:
                    checked_first_k(rows, o.stored, o.scanned, (o.hash, o.nonce), k, h, c, pieces, "batch_bound", Ld, early)


# ---- moved-edge probes: the four first-hit builds ---------------------------------------------------

def checked_probe(got, exp, c, Ld, early, p, build):
    try:
        check_probe(got, exp, p.lower, c.hi, build)
    except AssertionError as e:
        raise AssertionError("%s: %s; lower moved to %d, target %016x: %s" % (
            build, where(c, Ld, early, [p.piece], p.n), p.lower, p.T, e)) from e


FIRST_PARTS, FIRST_IDS = parts_of({1: 1, 2: 1, 3: 6})


def single_edge_probes(gpu, Ld, part, parts, stop_running):
    build, done = "stop_scan" if stop_running else "first_scan", 0
    for c, early, kept, _ in g.edge_probes(Ld)[part::parts]:
        with env(**cell_env(Ld, early)):
            for p in kept:
                for T, exp in ((p.T, p.exp), (p.T - 1, p.exp_below)):
                    got = gpu.search_first(c.msg, p.lower, c.hi, T, stop_running=stop_running)
                    checked_probe(got, exp, c, Ld, early, p, build)
                    done += 1
    assert done >= 2 * 4_000 // parts


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", FIRST_PARTS, ids=FIRST_IDS)
def test_first_scan_edge_probes(gpu, Ld, part, parts):
    single_edge_probes(gpu, Ld, part, parts, False)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", FIRST_PARTS, ids=FIRST_IDS)
def test_stop_scan_edge_probes(gpu, Ld, part, parts):
    single_edge_probes(gpu, Ld, part, parts, True)


def batch_edge_probes(gpu, Ld, stop_running):
    build, done = "batch_stop" if stop_running else "batch_first", 0
    for early, items, dropped in g.edge_probe_batches(Ld):
        assert dropped == 0
        with env(**cell_env(Ld, early)):
            for below in (False, True):
                reqs = [(c.msg, p.lower, c.hi, p.T - 1 if below else p.T) for c, p in items]
                res = gpu.search_first_batch(reqs, fuse_fast=True, stop_running=stop_running)
                assert len(res) == len(items)
                for (c, p), got in zip(items, res):
                    checked_probe(got, p.exp_below if below else p.exp, c, Ld, early, p, build)
                done += len(reqs)
    assert done >= 2 * 4_000


@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_batch_first_edge_probes(gpu, Ld):
    batch_edge_probes(gpu, Ld, False)


@pytest.mark.gpu
@pytest.mark.parametrize("Ld", LDS)
def test_batch_stop_edge_probes(gpu, Ld):
    batch_edge_probes(gpu, Ld, True)


# ---- XOR probes: fast_search and batch_fast (dev build) ---------------------------------------------

XOR_PARTS, XOR_IDS = parts_of({1: 1, 2: 1, 3: 8})
XOR_BATCH_PARTS, XOR_BATCH_IDS = parts_of({1: 1, 2: 2, 3: 10})
BATCH_CALL = 4      # requests per batch_fast call: the probed cell and the next three of its group


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", XOR_PARTS, ids=XOR_IDS)
def test_fast_search_xor_probes(gpu, tmp_path, Ld, part, parts):
    """test_gpu_probe.run_cases' comparison -- every result bit for bit masked_min(..., x); a positive
    probe returns (0, n*), a negative one a non-zero hash inside the range -- with the cell named."""
    from test_gpu_ties import run_jobs
    todo = g.xor_probes(Ld)[part::parts]
    cases = [Case(msg=c.msg, lo=c.lo, hi=c.hi, env=cell_env(Ld, early), pieces=pieces, pos=pos, neg=neg)
             for c, early, pieces, pos, neg in todo]
    jobs = [case.job() for case in cases]
    results, _ = run_jobs(tmp_path, jobs)
    assert len(results) == sum(len(case.probes) for case in cases) >= (len(cases) * 4)
    it = iter(results)
    for (c, early, pieces, _pos, _neg), case, j in zip(todo, cases, jobs):
        for n, x in zip(case.probes, j["xors"]):
            got, exp = tuple(next(it)), masked_min(c.msg, c.lo, c.hi, 32, 32, x)
            assert got == (exp.hash, exp.nonce), ("fast_search", where(c, Ld, early, pieces, n), "%016x" % x, got, exp)
            if c.lo <= n <= c.hi:
                assert got == (0, n), ("fast_search", where(c, Ld, early, pieces, n), got)
            else:
                assert got[0] != 0 and c.lo <= got[1] <= c.hi, ("fast_search", name(c, Ld, early), n, got)


def xor_batch_groups(Ld):
    return [grp for grp in g.batch_groups(Ld) if grp[1][0].kind != "early"]


def batch_call(cs, i):
    """The cells of the batch_fast call that probes cs[i]: it and the next cells of its group."""
    return [cs[(i + k) % len(cs)] for k in range(min(BATCH_CALL, len(cs)))]


@pytest.mark.gpu
@pytest.mark.parametrize("Ld,part,parts", XOR_BATCH_PARTS, ids=XOR_BATCH_IDS)
def test_batch_fast_xor_probes(gpu, tmp_path, Ld, part, parts):
    """The same probes through mh_search_batch_ex(MH_BATCH_FUSE_FAST) on the dev build's batch code
    object (test_gpu_batch_fast.run_jobs): one call per probe, holding the probed cell's request and
    the next three of its group; the probed request returns (0, n*) (probed just outside: a non-zero
    minimum) and every request of the call its masked_min under that constant."""
    from test_gpu_batch_fast import job, run_jobs
    probes = {(c, early): (pieces, pos, neg) for c, early, pieces, pos, neg in g.xor_probes(Ld)}
    calls = []      # (cells, early, probed nonce, x)
    for early, cs, _ in xor_batch_groups(Ld):
        for i, c in enumerate(cs):
            pieces, pos, neg = probes[(c, early)]
            ns = sorted(pos) + sorted(neg)
            calls += [(batch_call(cs, i), early, n, x) for n, x in zip(ns, hashes_of(c.msg, c.lo, c.hi, ns))]
    calls = calls[part::parts]
    jobs = [job([(c.msg, c.lo, c.hi) for c in cs], dict(cell_env(Ld, early), MINEHIP_DEV_HASH_XOR="%016x" % x), plan=False)
            for cs, early, n, x in calls]
    out = run_jobs(tmp_path, jobs, dev=True)
    assert len(out) == len(calls) >= 4 * (MAIN + TOPS) // parts
    for (cs, early, n, x), d in zip(calls, out):
        got = [tuple(r) for r in d["results"]]
        exp = [masked_min(c.msg, c.lo, c.hi, 32, 32, x) for c in cs]
        c = cs[0]
        pieces = probes[(c, early)][0]
        assert got == [(t.hash, t.nonce) for t in exp], ("batch_fast", where(c, Ld, early, pieces, n), "%016x" % x, got, exp)
        if c.lo <= n <= c.hi:
            assert got[0] == (0, n), ("batch_fast", where(c, Ld, early, pieces, n), got[0])
        else:
            assert got[0][0] != 0 and c.lo <= got[0][1] <= c.hi, ("batch_fast", name(c, Ld, early), n, got[0])
