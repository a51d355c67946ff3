"""The one pass function of mh_search_hits_batch and mh_search_hits_batch_ex on the CPU: a pass without
fast pieces planned through the fast-piece planner (plan_hits_batch_pass_ex on empty fast tables, what
hits_batch_run_pass and mh_hits_batch_regions_ex run) gets the regions and windows of the plain
planner (plan_hits_batch_pass, what mh_hits_batch_regions runs).  No GPU compute is called here."""
import minehip
from test_hits_batch import MAXCAP, _child, check_regions

# 3 requests of 10^4 nonces: far below the fast kernels' reach, so every pass is without fast pieces
REQS = [(b"cmu440", 0, 9999, 1, 1), (b"abc", 5000, 14999, 1, 16), (b"minehip", 10 ** 12, 10 ** 12 + 9999, 1, 4096)]


def both_probes(reqs, slots_limit=MAXCAP):
    plan = minehip.batch_plan_ex([r[:3] for r in reqs], fuse_fast=True)
    assert plan and all(p["kind"] == 0 for p in plan), plan        # fused, and no fast piece (kind 2)
    plain = minehip.hits_batch_regions(reqs, 0)
    merged = minehip.hits_batch_regions(reqs, 0, fuse_fast=True)
    assert merged == plain
    check_regions(reqs, 0, slots_limit)                             # and both follow the region rule
    return plain


def test_regions_and_windows_of_a_pass_without_fast_pieces():
    regs = both_probes(REQS)
    assert [(g["pass"], g["window"], g["offset"], g["slots"]) for g in regs] == [(0, 0, 0, 1), (0, 0, 1, 16),
                                                                                 (0, 0, 17, 4096)]


def test_the_same_with_a_pass_and_a_window_per_request():
    """A child process with a pass per request (MINEHIP_BATCH_SLOTS = the tiles of one) and a hit
    buffer of 16 entries: the second request starts a window, the third is cut to the buffer."""
    code = ("import json, os, minehip, test_hits_batch_merged_pass as t\n"
            "tiles = max(sum(it['slots'] for it in minehip.batch_plan([r[:3]])) for r in t.REQS)\n"
            "os.environ['MINEHIP_BATCH_SLOTS'] = str(tiles)\n"
            "print(json.dumps(t.both_probes(t.REQS, 16)))\n")
    regs = _child(code, MINEHIP_HITS_SLOTS=16)
    assert [(g["pass"], g["window"], g["offset"], g["slots"]) for g in regs] == [(0, 0, 0, 1), (1, 1, 0, 16),
                                                                                 (2, 2, 0, 16)]
