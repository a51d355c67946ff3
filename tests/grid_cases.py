"""Host-only case construction for tests/test_gpu_grid.py: every tail offset x every digit count.

A cell is (n, d): the message b"q" * n, n = 0..63, so that the tail offset t = (n + 1) % 64 takes
every value, and a range of at most 5,201 nonces of d digits, d = 2..20, placed so that every
decimal place of the lane number U = nonce // 10^L is non-zero and both edges are ragged:

  B_d = int("12345678912345678912"[:d])
  lo  = 10^(d-1) for d <= 4, else max(10^(d-1), B_d // 10^4 * 10^4 - 37)
  hi  = min(10^d - 1, lo + 5200)

plus, per n, a top cell [2^64 - 1 - 5200, 2^64 - 1].  1,216 + 64 cells, 5,722,048 nonces in the
main ones.  Every search of a cell runs under MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1,
MINEHIP_LOWER_DIGITS in {1, 2, 3} and MINEHIP_EARLY=1, and again under MINEHIP_EARLY=0 where the
cell's plan holds an Early piece (the last-digit layout it replaces at that offset).

An Early layout needs whole blocks of 10^(p+L) nonces (p: the decimal position of its innermost
digit), which a 5,201-nonce cell holds only for p + L <= 3.  early_cases() adds the cases of
test_gpu_parity.early_position_cases(Ls=(1, 2, 3)) with p + L <= 5 (two blocks plus a ragged edge,
at most 203,457 nonces), moved to B_d rounded down to a multiple of 10^(p+L) so that U's digits are
non-zero; the cases at the top of u64 stay there.

Everything here comes from minehip.plan / batch_plan_ex and the CPU oracle; nothing touches a GPU.
"""
import collections
import functools
import random

import numpy as np

from test_gpu_dense import piece_of
from test_gpu_first_probe import Probe, own_piece, probe_of
from test_gpu_parity import env
from test_gpu_probe import early_pos, last_of
from test_gpu_ties import full_hashes

U64 = (1 << 64) - 1
LDS = (1, 2, 3)
SPAN = 5_200
B = "12345678912345678912"
FAST = dict(MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1)
HIT_BUFFER = 1 << 20        # entries of the device hit buffer (MH_HITS_MAX_CAP): one batch call's sum of caps
LOWEST = 4                  # moved-edge probes per cell and L: the lowest hashes of its fast pieces
RANDOM = 2                  # XOR probes per cell and L: seeded random nonces of its fast pieces

# kind: "main", "top" (grid cells), "early" (an Early position case; key = (J, mode, p, L), Ld its
# MINEHIP_LOWER_DIGITS, top: whether it ends at 2^64 - 1)
Cell = collections.namedtuple("Cell", "kind n d msg lo hi key Ld")


def t_of(c):
    return (c.n + 1) % 64


def align_of(c):
    """Byte of the cell's last digit inside its word: (t + d - 1) & 3."""
    return (t_of(c) + c.d - 1) & 3


def N_of(c):
    return c.hi - c.lo + 1


def name(c, Ld=None, early=None):
    """The cell as a mismatch report names it."""
    s = "%s cell n = %d (t = %d), d = %d, alignment %d, [%d, %d]" % (c.kind, c.n, t_of(c), c.d, align_of(c), c.lo, c.hi)
    if c.key is not None:
        s += ", Early case <%d, %d> p = %d L = %d" % c.key
    if Ld is not None:
        s += ", MINEHIP_LOWER_DIGITS=%d" % Ld
    if early is not None:
        s += ", MINEHIP_EARLY=%d" % early
    return s


def cell_env(Ld, early):
    return dict(FAST, MINEHIP_LOWER_DIGITS=Ld, MINEHIP_EARLY=early)


def B_d(d):
    return int(B[:d])


@functools.lru_cache(maxsize=None)
def main_cells():
    out = []
    for d in range(2, 21):
        low = 10 ** (d - 1)
        lo = low if d <= 4 else max(low, B_d(d) // 10 ** 4 * 10 ** 4 - 37)
        hi = min(10 ** d - 1, U64, lo + SPAN)
        out += [Cell("main", n, d, b"q" * n, lo, hi, None, None) for n in range(64)]
    return out


@functools.lru_cache(maxsize=None)
def top_cells():
    return [Cell("top", n, 20, b"q" * n, U64 - SPAN, U64, None, None) for n in range(64)]


def grid_cells():
    return main_cells() + top_cells()


def fast_pieces(pieces, kind=0):
    return [p for p in pieces if p["kind"] == kind]


def early_pieces(pieces):
    return [p for p in pieces if p["kind"] == 0 and p["mode"] >= 3]


@functools.lru_cache(maxsize=None)
def grid_plans(Ld, early):
    """{cell: minehip.plan of it} of every grid cell under cell_env(Ld, early)."""
    import minehip
    with env(**cell_env(Ld, early)):
        return {c: minehip.plan(c.msg, c.lo, c.hi) for c in grid_cells()}


@functools.lru_cache(maxsize=None)
def early_cells(Ld):
    """The grid cells whose MINEHIP_EARLY=1 plan holds an Early piece: they run again with
    MINEHIP_EARLY=0."""
    return [c for c, pieces in grid_plans(Ld, 1).items() if early_pieces(pieces)]


# ---- the Early position cases ------------------------------------------------------------------------

EARLY_MAX = 5               # p + L <= 5: two blocks are at most 200,000 nonces
# (J, mode, p, L) of test_gpu_parity.early_position_cases with p + L <= 5 that no moved case
# reaches, each with its reason; test_grid_rests_on asserts that every other key is kept
EARLY_DROPPED = {}


@functools.lru_cache(maxsize=None)
def early_cases():
    """([Cell of kind "early"], {dropped key: why}): per key (J, mode, p, L) of
    early_position_cases(Ls=(1, 2, 3)) with p + L <= 5 the case moved to B_d rounded down to a
    multiple of 10^(p+L), two blocks plus 3,456 nonces, kept where minehip.plan still gives an Early
    piece of the same (J, mode, p, L) holding a whole block; its top-of-u64 variant stays at the top."""
    import minehip
    from test_gpu_parity import early_position_cases
    kept, dropped = [], {}
    for (J, mode, p, L, top), (m, lo, hi, Ld) in sorted(early_position_cases(Ls=LDS).items()):
        if p + L > EARLY_MAX:
            continue
        with env(**cell_env(Ld, 1)):     # d: the digit count of the case's Early piece (its range may span buckets)
            d = next(pc["digits"] for pc in early_pieces(minehip.plan(m, lo, hi))
                     if (pc["word"], pc["mode"], pc["lo_digits"]) == (J, mode, L) and early_pos(m, pc) == p)
        block = 10 ** (p + L)
        size = 2 * block + 3_456
        lo2 = U64 - size if top else B_d(d) // block * block
        hi2 = min(U64, 10 ** d - 1, lo2 + size)
        c = Cell("early", len(m), d, m, lo2, hi2, (J, mode, p, L), Ld)
        with env(**cell_env(Ld, 1)):
            pieces = minehip.plan(m, lo2, hi2)
        own = [pc for pc in early_pieces(pieces) if (pc["word"], pc["mode"], pc["lo_digits"]) == (J, mode, L)
               and early_pos(m, pc) == p and pc["count"] >= block]
        if own:
            kept.append(c)
        else:
            dropped[(J, mode, p, L, top)] = "no Early piece of this key in the plan of [%d, %d]" % (lo2, hi2)
    return kept, dropped


# ---- runs: what one search is ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def runs(Ld):
    """[(cell, early, pieces)]: every search of the grid at this MINEHIP_LOWER_DIGITS -- each grid
    cell under MINEHIP_EARLY=1, the cells with an Early piece again under MINEHIP_EARLY=0, and the
    Early position cases of this Ld."""
    import minehip
    out = [(c, 1, grid_plans(Ld, 1)[c]) for c in grid_cells()]
    out += [(c, 0, grid_plans(Ld, 0)[c]) for c in early_cells(Ld)]
    with env(**cell_env(Ld, 1)):
        out += [(c, 1, minehip.plan(c.msg, c.lo, c.hi)) for c in early_cases()[0] if c.Ld == Ld]
    return out


@functools.lru_cache(maxsize=None)
def batch_groups(Ld):
    """[(early, [cell], [pieces of batch_plan_ex per cell])]: the calls of the batched builds -- the
    64 main cells of one d, the 64 top cells, the cells of one d with an Early piece under
    MINEHIP_EARLY=0, and the Early position cases, as many per call as the device hit buffer holds."""
    import minehip
    groups = []
    for d in range(2, 21):
        groups.append((1, [c for c in main_cells() if c.d == d]))
    groups.append((1, top_cells()))
    for d in range(2, 21):
        again = [c for c in early_cells(Ld) if c.d == d]
        if again:
            groups.append((0, again))
    cur = []
    for c in [c for c in early_cases()[0] if c.Ld == Ld]:
        if cur and sum(map(N_of, cur)) + N_of(c) > HIT_BUFFER:
            groups.append((1, cur))
            cur = []
        cur.append(c)
    if cur:
        groups.append((1, cur))
    out = []
    for early, cs in groups:
        assert sum(map(N_of, cs)) <= HIT_BUFFER
        with env(**cell_env(Ld, early)):
            plan = minehip.batch_plan_ex([(c.msg, c.lo, c.hi) for c in cs], fuse_fast=True)
        per = [[] for _ in cs]
        for p in plan:
            per[p["req"]].append(p)
        out.append((early, cs, per))
    return out


def hashes(c):
    return full_hashes(c.msg, c.lo, c.hi)


# ---- the mismatch report ---------------------------------------------------------------------------

def grid_diff(rows, h, c, pieces, what):
    """None when the rows (hash, nonce) are exactly (h[i], c.lo + i); otherwise
    test_gpu_dense.dense_diff's report (the first differing index, its plan piece, lane, group and
    digit, how many differ) with the cell named: n, t, d, the alignment, and the lane number U of
    the first differing nonce with the tail byte of each of its digits (digit index k, least
    significant first, as the kernel places them)."""
    from test_gpu_dense import dense_diff
    rep = dense_diff(rows, h, c.lo, pieces, what)
    if rep is None:
        return None
    rep += " -- " + name(c)
    exp_n = np.uint64(c.lo) + np.arange(len(h), dtype=np.uint64)
    k = min(len(rows), len(h))
    bad = (rows[:k, 0] != np.asarray(h)[:k]) | (rows[:k, 1] != exp_n[:k])
    if bad.any():
        nonce = c.lo + int(bad.argmax())
        p = piece_of(pieces, nonce)
        if p is not None and p["kind"] != 1 and p.get("lo_digits", 0) > 0:
            L = p["lo_digits"]
            last = t_of(c) + c.d - 1                    # tail byte of the last digit
            if p["mode"] < 3:
                U = nonce // 10 ** L
                at = ["k = %d: '%s' at byte %d (word %d, byte %d)" % (k, dg, last - L - k, (last - L - k) >> 2, (last - L - k) & 3)
                      for k, dg in enumerate(reversed(str(U)))]
                rep += "; group digits at bytes %d..%d, last digit at byte %d" % (last - L + 1, last - 1, last)
            else:
                U = nonce // 10 ** L                    # by value: the Early lanes interleave
                at = ["%d digits of the nonce from byte %d" % (c.d, t_of(c))]
            rep += "; U = %d, U's digits: %s" % (U, "; ".join(at))
    return rep


# ---- coverage, from the plans alone ---------------------------------------------------------------

def is_early_layout(k):
    return k[1] >= 3


def group_words(c, p):
    """Of a last-digit fast piece at L >= 2: the set of words (relative to the piece's word J: 0 or
    -1) its L - 1 group digits lie in."""
    last = t_of(c) + c.d - 1
    base = 64 if (p["blocks"] == 2 and last >= 64) else 0
    return {((last - base - k) >> 2) - p["word"] for k in range(1, p["lo_digits"])}


def coverage(Ld, early):
    """(layouts, aligns, routes) of the grid cells under (Ld, early): the set of (J, mode) with a fast
    piece, {(J, mode): set of alignments}, {(J, mode): set of frozenset(group_words)} for pieces of
    lo_digits >= 2."""
    layouts, aligns, routes = set(), collections.defaultdict(set), collections.defaultdict(set)
    for c, pieces in grid_plans(Ld, early).items():
        for p in fast_pieces(pieces):
            k = (p["word"], p["mode"])
            layouts.add(k)
            aligns[k].add(align_of(c))
            if p["mode"] < 3 and p["lo_digits"] >= 2:
                routes[k].add(frozenset(group_words(c, p)))
    return layouts, aligns, routes


# ---- moved-edge probes of the first-hit builds -----------------------------------------------------

def in_fast(pieces, n, kind=0):
    for p in pieces:
        if p["kind"] == kind and p["first"] <= n <= last_of(p):
            return p
    return None


@functools.lru_cache(maxsize=None)
def edge_probes(Ld):
    """[(cell, early, [Probe], first)] per grid run of this L: of the LOWEST lowest hashes among the
    nonces of the cell's fast pieces, in increasing order of hash, those whose n* still lies in a
    fast piece of the same layout under minehip.plan(msg, lo', hi); first: the nonce of the lowest
    of them all, the first minimum of the cell's fast pieces (kept when it is the first Probe's)."""
    import minehip
    out = []
    for c, early, pieces in runs(Ld):
        if c.kind == "early":
            continue
        h = hashes(c)
        fast = fast_pieces(pieces)
        idx = np.concatenate([np.arange(p["first"] - c.lo, last_of(p) - c.lo + 1) for p in fast])
        ranked = idx[np.argsort(h[idx], kind="stable")][:LOWEST]
        kept = []
        with env(**cell_env(Ld, early)):
            for i in ranked:
                n = c.lo + int(i)
                k = in_fast(pieces, n)
                lower, T, exp, below = probe_of(h, c.lo, n)
                pc = own_piece(minehip.plan(c.msg, lower, c.hi), (k["word"], k["mode"]), n, 0)
                if pc is not None:
                    kept.append(Probe(n, lower, T, exp, below, pc))
        out.append((c, early, kept, c.lo + int(ranked[0])))
    return out


@functools.lru_cache(maxsize=None)
def edge_probe_batches(Ld):
    """[(early, [(cell, Probe)], dropped)]: the kept probes of 64 cells (batch_groups' grid groups)
    as one call of one request per probe, kept where mh_batch_plan_ex fuses the request with a kind-2
    piece of the probe's layout holding n*; dropped: how many it does not."""
    import minehip
    by_run = {(c, early): kept for c, early, kept, _ in edge_probes(Ld)}
    out = []
    for early, cs, _ in batch_groups(Ld):
        if cs[0].kind == "early":
            continue
        items = [(c, p) for c in cs for p in by_run[(c, early)]]
        with env(**cell_env(Ld, early)):
            plan = minehip.batch_plan_ex([(c.msg, p.lower, c.hi) for c, p in items], fuse_fast=True, cap=1 << 16)
        per = collections.defaultdict(list)
        for pc in plan:
            per[pc["req"]].append(pc)
        ok = [(c, p) for i, (c, p) in enumerate(items)
              if all(pc["kind"] != 1 for pc in per[i])
              and own_piece(per[i], (p.piece["word"], p.piece["mode"]), p.n, 2) is not None]
        out.append((early, ok, len(items) - len(ok)))
    return out


# ---- XOR probes of fast_search and batch_fast ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def xor_probes(Ld):
    """[(cell, early, pieces, pos, neg)] per grid run of this L.  pos: the first and last nonce of
    each fast piece and RANDOM seeded random nonces of the fast pieces, plus draws until, over the
    whole grid at this L, every digit value has been probed at each of the low L + 2 decimal places;
    neg: lo - 1 and hi + 1 where they exist."""
    rng = random.Random(4410 + Ld)
    out = []
    for c, early, pieces in runs(Ld):
        if c.kind == "early":
            continue
        fast = fast_pieces(pieces)
        pos = {n for p in fast for n in (p["first"], last_of(p))}
        total = sum(p["count"] for p in fast)
        for _ in range(RANDOM):
            pos.add(nth_of(fast, rng.randrange(total)))
        neg = ({c.lo - 1} if c.lo > 0 else set()) | ({c.hi + 1} if c.hi < U64 else set())
        out.append((c, early, pieces, pos, neg))
    while not digits_probed(out, Ld):
        c, early, pieces, pos, neg = out[rng.randrange(len(out))]
        fast = fast_pieces(pieces)
        pos.add(nth_of(fast, rng.randrange(sum(p["count"] for p in fast))))
    return out


def nth_of(pieces, r):
    for p in pieces:
        if r < p["count"]:
            return p["first"] + r
        r -= p["count"]
    raise IndexError(r)


def digits_probed(probes, Ld):
    seen = [set() for _ in range(Ld + 2)]
    for c, early, pieces, pos, neg in probes:
        for n in pos:
            for k in range(min(Ld + 2, c.d)):
                seen[k].add(n // 10 ** k % 10)
    return all(s == set(range(10)) for s in seen)
