"""Static guards on the stopping hits code object (CPU, no GPU touched).

mh_search_first_hits runs hits_stop<J, MODE>: fast_search.hip built with -DMH_HITS -DMH_STOP through
the product's passes into build/fast_hits_stop.hsaco, embedded in the library as a ninth blob
(mh_hits_stop_co_begin).  The poll sits outside the per-nonce loop, the slice counts and the
published bound in the rare hit branch, and the feature must leave every other code object alone:

  * the blob holds one hits_stop kernel per entry of layout.hpp's MH_FAST_KERNELS and no other
    kernel; no other blob mentions hits_stop;
  * the per-nonce loops hold no private-memory access and no load, atomic or barrier beyond what
    hits_scan's loops have; the poll is a `global_load_dwordx2 ... sc1` in the group loop's header;
  * per <J, MODE> the register file holds no fewer waves per SIMD than with hits_scan, with no
    fewer LDS bytes;
  * per <J, MODE> the per-nonce loop issues no more VALU instructions and no more half-rate ones
    than the product kernel's loop (csrc/loop_mix.py against build/fast_loop_mix.json), which
    hits_scan and stop_scan each meet -- except the layouts DESIGN.md lists with their excess, at
    most 2 instructions in either count (the excess the file's comments record for the un-remedied
    hits and stop builds);
  * in fast_search.hip, hits_stop appears only under both MH_HITS and MH_STOP.

These are conditions of the build, not measurements.
"""
import json
import os
import re
import sys

from conftest import ROOT

CSRC = os.path.join(ROOT, "bitcoin-miner_amd", "csrc")
BUILD = os.path.join(ROOT, "build")
sys.path.insert(0, CSRC)
import loop_mix  # noqa: E402
from minehip import codeobj  # noqa: E402
from test_abi import KERNELS  # noqa: E402

NAME = r"_ZN2mh9hits_stopILi(\d+)ELi(\d+)EEEvNS_8FastArgsEPNS_7PartialENS_12HitsStopArgsE$"
MAX_EXCESS = 2          # VALU instructions a listed layout's loop may issue above the product's


def test_code_object_holds_one_kernel_per_layout():
    co = codeobj.hits_stop_code_object()
    assert co == open(os.path.join(BUILD, "fast_hits_stop.hsaco"), "rb").read()
    kernels = codeobj.metadata(co)["amdhsa.kernels"]
    got = [tuple(int(x) for x in re.match(NAME, k[".name"]).groups()) for k in kernels]     # every kernel is a hits_stop
    assert len(got) == len(KERNELS) == 26 and set(got) == KERNELS == loop_mix.fast_kernels()
    # FastArgs by value at its product size, then the partials pointer (then HitsStopArgs, 88 bytes)
    assert {tuple(a[".size"] for a in k[".args"][:2]) for k in kernels} == {(520, 8)}
    assert {k[".args"][2][".size"] for k in kernels} == {88}
    assert b"mh_fast_queue_args" in co and b"mh_fast_hash_keep" not in co and b"mh_dev_hash_xor" not in co
    for other in (b"hits_scan", b"stop_scan", b"first_scan", b"fast_search", b"batch_"):
        assert other not in co, other
    # and no existing blob knows anything of it
    blobs = [codeobj.fast_code_object(), codeobj.first_code_object(), codeobj.hits_code_object(),
             codeobj.batch_code_object(), codeobj.batch_first_code_object(), codeobj.batch_hits_code_object(),
             codeobj.first_stop_code_object(), codeobj.batch_first_stop_code_object()]
    assert len({co, *blobs}) == 9
    for other in blobs:
        assert b"hits_stop" not in other
    for f in ("fast_search_keep.hsaco", "fast_batch_keep.hsaco"):
        assert b"hits_stop" not in open(os.path.join(BUILD, f), "rb").read(), f
    assert set(codeobj.hits_stop_kernel_resources()) == KERNELS


def test_kernels_keep_hits_scans_occupancy():
    hs, hits = codeobj.hits_stop_kernel_resources(), codeobj.hits_kernel_resources()
    assert set(hs) == set(hits) == KERNELS
    lower = {k: (hs[k], hits[k]) for k in hits
             if hs[k]["max_waves_per_simd"] < hits[k]["max_waves_per_simd"] or hs[k]["lds_bytes"] < hits[k]["lds_bytes"]}
    assert not lower, lower


def test_the_poll_and_the_per_nonce_loops():
    """Per kernel against hits_scan's: the bound word is read by `global_load_dwordx2 ... sc1` (a
    relaxed agent-scope load, served past the CU's L1) once beside the claim and once in the group
    loop's header block -- hits_scan has no such load -- and the per-nonce loop holds no load, store,
    atomic or barrier of its own, no private-memory access, and no more scalar loads than hits_scan's."""
    text = open(os.path.join(BUILD, "fast_hits_stop_prio.s")).read()
    hits = loop_mix.kernels(open(os.path.join(BUILD, "fast_hits_prio.s")).read())
    hits = {loop_mix.HITS.match(n).groups(): b for n, b in hits.items() if loop_mix.HITS.match(n)}
    poll = r"^\s+global_load_dwordx2 .* sc1\s*$"
    seen = 0
    for name, body in loop_mix.kernels(text).items():
        m = loop_mix.HITS_STOP.match(name)
        if not m:
            continue
        seen += 1
        lines = body.split("\n")
        assert not [l for l in hits[m.groups()].split("\n") if re.match(poll, l)], name
        at = [i for i, l in enumerate(lines) if re.match(poll, l)]
        assert len(at) == 3, (name, len(at))          # claim_below_bound's (inlined twice) and the group loop's
        # exactly one sits in a loop header's block, one with child loops: the group loop's (a claim
        # reads the word behind the branch that ends the claim loop)
        headers = [i for i, l in enumerate(lines) if "Loop Header" in l]
        in_header = []
        for i in at:
            head = max([h for h in headers if h < i], default=None)
            if head is not None and not [l for l in lines[head:i] if l.strip().startswith(("s_cbranch", "s_branch"))]:
                in_header.append(head)
        assert len(in_header) == 1 and "Child Loop" in lines[in_header[0] + 1], (name, in_header)
        inner = loop_mix.per_nonce_loop(body)
        assert sum(o.startswith("v_") for o in inner) > 1000
        assert not [o for o in inner if o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_", "s_barrier"))], name
        hits_inner = loop_mix.per_nonce_loop(hits[m.groups()])
        assert sum(o.startswith("s_load") for o in inner) <= sum(o.startswith("s_load") for o in hits_inner), name
        assert not [o for o in inner if "atomic" in o], name
    assert seen == len(KERNELS)


def listed_excess():
    """{(J, MODE): (valu excess, half excess)} of the layouts DESIGN.md lists for hits_stop."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("hits_stop loops above the product's"):]
    sec = sec[:sec.index("\n\n")]
    return {(int(j), int(m)): (int(v), int(h))
            for j, m, v, h in re.findall(r"<(\d+), (\d)>: \+(\d+) VALU, \+(\d+) half-rate", sec)}


def test_loops_issue_no_more_than_the_products():
    hs = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_hits_stop_prio.s")).read(), loop_mix.HITS_STOP)
    prod = json.load(open(os.path.join(BUILD, "fast_loop_mix.json")))
    assert set(hs) == set(prod) == {f"{j},{m}" for j, m in KERNELS}
    # the product's own file is what its assembly gives (the comparison is like for like), and
    # hits_scan and stop_scan each meet the product's loops
    assert prod == loop_mix.loop_mix(open(os.path.join(BUILD, "fast_search_prio.s")).read())
    for f, pat in (("fast_hits_prio.s", loop_mix.HITS), ("fast_first_stop_prio.s", loop_mix.STOP)):
        other = loop_mix.loop_mix(open(os.path.join(BUILD, f)).read(), pat)
        assert not [k for k in prod if other[k]["valu"] > prod[k]["valu"] or other[k]["half"] > prod[k]["half"]], f
    assert all(v["valu"] > 1000 for v in hs.values())          # a whole per-nonce loop was found
    assert {v["loop_spill_ops"] for v in hs.values()} == {0}
    over = {tuple(int(x) for x in k.split(",")): (max(0, hs[k]["valu"] - prod[k]["valu"]), max(0, hs[k]["half"] - prod[k]["half"]))
            for k in prod if hs[k]["valu"] > prod[k]["valu"] or hs[k]["half"] > prod[k]["half"]}
    for k, (v, h) in sorted(over.items()):
        print("<%d, %d>: +%d VALU, +%d half-rate" % (k + (v, h)))
    assert all(v <= MAX_EXCESS and h <= MAX_EXCESS for v, h in over.values()), over
    assert over == listed_excess(), (over, listed_excess())     # each such layout is listed with its excess


def cut(src, macro, define):
    """fast_search.hip, comments removed, as the preprocessor sees it with `macro` defined or not:
    the lines kept (conditionals on other macros keep both branches)."""
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    keep, stack = [], []
    for line in src.split("\n"):
        s = line.strip()
        if re.match(r"#\s*if", s):
            m = re.match(r"#\s*(ifdef|ifndef)\s+%s\b" % macro, s)
            assert m or macro not in s, s
            stack.append(((m.group(1) == "ifdef") == define, True) if m else (True, False))
        elif re.match(r"#\s*else", s):
            taken, ours = stack.pop()
            stack.append((not taken if ours else taken, ours))
        elif re.match(r"#\s*elif", s):
            assert not stack[-1][1], "no #elif on an %s conditional" % macro
        elif re.match(r"#\s*endif", s):
            stack.pop()
        elif all(t for t, _ in stack):
            keep.append(line)
    assert not stack
    return "\n".join(keep)


def test_hits_stop_appears_only_under_both_macros():
    src = open(os.path.join(CSRC, "fast_search.hip")).read()
    new = r"hits_stop|HitsStop|hits_floor|claim_below_bound|publish_first_hits_bound|first_hits_slice|KHStop|KHits2"
    assert len(re.findall(r"hits_stop<j, m>", src)) == 1 and re.search(new, cut(src, "MH_STOP", True))
    assert not re.search(new, cut(src, "MH_STOP", False))
    assert not re.search(new, cut(src, "MH_HITS", False))
    for line in src.split("\n"):                                # plain #ifdef / #ifndef on the three macros
        if re.match(r"\s*#\s*(if|elif)\b", line):
            assert not re.search(r"MH_FIRST|MH_HITS|MH_STOP", line), line
