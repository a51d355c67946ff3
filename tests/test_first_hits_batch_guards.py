"""Static guards on the stopping hits batch code object (CPU, no GPU touched).

mh_search_first_hits_batch(MH_BATCH_FUSE_FAST) runs batch_bound<J, MODE>: fast_search.hip built with
-DMH_BATCH -DMH_HITS -DMH_STOP through the product's passes into build/fast_batch_bound.hsaco,
embedded in the library as a tenth blob (mh_batch_bound_co_begin).  The wrapper is batch_first's and
the chunk body hits_stop's, so for each of the 26 layouts:

  * the blob holds one batch_bound kernel and nothing else, its own marker (sized as BatchBoundItem)
    and no hook symbols, and no other blob or *_keep.hsaco mentions it;
  * the register file holds no fewer waves per SIMD than with hits_stop, with no fewer LDS bytes;
  * the per-nonce loop holds no load, store, atomic, barrier or private-memory access, and no more
    scalar loads than hits_stop's;
  * the per-nonce loop issues no more VALU instructions and no more half-rate ones than hits_stop's
    own loop for the layout (hits_stop as the same `make` builds it from the parent's sources: its
    bytes are pinned below) -- except the layouts DESIGN.md lists with their excess;
  * every code object that existed before, and build/fast_loop_mix.json, is byte-identical to the
    parent commit's build (tests/golden/parent_code_objects_first_hits_batch.json, per compiler).

These are conditions of the build, not measurements; the assembly is parsed for loop structure and
instruction counts only.
"""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT, GOLDEN

CSRC = os.path.join(ROOT, "bitcoin-miner_amd", "csrc")
BUILD = os.path.join(ROOT, "build")
sys.path.insert(0, CSRC)
import loop_mix  # noqa: E402
from minehip import codeobj  # noqa: E402
from test_abi import KERNELS  # noqa: E402

NAME = r"_ZN2mh11batch_boundILi(\d+)ELi(\d+)EEEvPKNS_14BatchBoundItemEPKjS5_PNS_7PartialE$"
MAX_EXCESS = 3          # VALU instructions a listed layout's loop may issue above hits_stop's


def test_code_object_holds_one_kernel_per_layout():
    co = codeobj.batch_bound_code_object()
    assert co == open(os.path.join(BUILD, "fast_batch_bound.hsaco"), "rb").read()
    kernels = codeobj.metadata(co)["amdhsa.kernels"]
    got = [tuple(int(x) for x in re.match(NAME, k[".name"]).groups()) for k in kernels]    # every kernel is a batch_bound
    assert len(got) == len(KERNELS) == 26 and set(got) == KERNELS == loop_mix.fast_kernels()
    # batch_first's four pointers: the items, the per-chunk item table, the order table, the partials
    assert {tuple(a[".size"] for a in k[".args"][:4]) for k in kernels} == {(8, 8, 8, 8)}
    assert all(len(k[".args"]) == 4 or k[".args"][4].get(".value_kind", "").startswith("hidden") for k in kernels)
    # its own marker, none of the others', no hook symbols, no other kernel family
    assert b"mh_fast_batch_bound_items" in co
    for other in (b"mh_fast_batch_items", b"mh_fast_batch_first_items", b"mh_fast_batch_hits_items", b"mh_fast_batch_stop_items",
                  b"mh_fast_queue_args", b"mh_fast_hash_keep", b"mh_dev_hash_xor", b"stop_scan", b"first_scan", b"batch_fast",
                  b"batch_first", b"batch_hits", b"batch_stop", b"fast_search", b"hits_scan", b"hits_stop"):
        assert other not in co, other
    # no other blob knows anything of it
    blobs = [codeobj.fast_code_object(), codeobj.first_code_object(), codeobj.hits_code_object(),
             codeobj.batch_code_object(), codeobj.batch_first_code_object(), codeobj.batch_hits_code_object(),
             codeobj.first_stop_code_object(), codeobj.batch_first_stop_code_object(), codeobj.hits_stop_code_object()]
    assert len({co, *blobs}) == 10
    for other in blobs:
        assert b"batch_bound" not in other
    for f in ("fast_search_keep.hsaco", "fast_batch_keep.hsaco"):
        assert b"batch_bound" not in open(os.path.join(BUILD, f), "rb").read(), f
    assert set(codeobj.batch_bound_kernel_resources()) == KERNELS


def test_marker_is_sized_as_the_item_struct():
    """layout.hpp BatchBoundItem: FastArgs (520), the unused pointer, HitsStopArgs (88), chunk0, slot0."""
    readelf = os.path.join(os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin"), "llvm-readelf")   # the Makefile's LLVM
    if not os.path.exists(readelf):
        pytest.skip("no llvm-readelf")
    r = subprocess.run([readelf, "-sW", os.path.join(BUILD, "fast_batch_bound.hsaco")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes = {int(l.split()[2]) for l in r.stdout.splitlines() if l.split()[-1:] == ["mh_fast_batch_bound_items"]}
    assert sizes == {520 + 8 + 88 + 8} == {624}     # in .dynsym and .symtab alike


def test_kernels_keep_hits_stops_occupancy():
    bb, hs = codeobj.batch_bound_kernel_resources(), codeobj.hits_stop_kernel_resources()
    assert set(bb) == set(hs) == KERNELS
    lower = {k: (bb[k], hs[k]) for k in hs
             if bb[k]["max_waves_per_simd"] < hs[k]["max_waves_per_simd"] or bb[k]["lds_bytes"] < hs[k]["lds_bytes"]}
    assert not lower, lower


def bodies():
    bb = loop_mix.kernels(open(os.path.join(BUILD, "fast_batch_bound_prio.s")).read(), whole=True)
    hs = loop_mix.kernels(open(os.path.join(BUILD, "fast_hits_stop_prio.s")).read())
    return ({loop_mix.BATCH_BOUND.match(n).groups(): b for n, b in bb.items() if loop_mix.BATCH_BOUND.match(n)},
            {loop_mix.HITS_STOP.match(n).groups(): b for n, b in hs.items() if loop_mix.HITS_STOP.match(n)})


def test_the_poll_and_the_per_nonce_loops():
    """Per kernel: the bound is read by `global_load_dwordx2 ... sc1` (a relaxed agent-scope load,
    served past the CU's L1) once in the wrapper and once in the group loop's header block; the
    per-nonce loop holds no load, store, atomic or barrier of its own, no private-memory access, and
    no more scalar loads than hits_stop's."""
    bb, hs = bodies()
    assert set(bb) == set(hs) == {(str(j), str(m)) for j, m in KERNELS}
    poll = r"^\s+global_load_dwordx2 .* sc1\s*$"
    for key, body in bb.items():
        lines = body.split("\n")
        at = [i for i, l in enumerate(lines) if re.match(poll, l)]
        assert len(at) == 2, (key, len(at))                       # the wrapper's and the group loop's
        headers = [i for i, l in enumerate(lines) if "Loop Header" in l]
        in_header = []
        for i in at:
            head = max([h for h in headers if h < i], default=None)
            if head is not None and not [l for l in lines[head:i] if l.strip().startswith(("s_cbranch", "s_branch"))]:
                in_header.append(head)
        assert len(in_header) == 1 and "Child Loop" in lines[in_header[0] + 1], (key, in_header)
        inner = loop_mix.per_nonce_loop(body)
        assert sum(o.startswith("v_") for o in inner) > 1000
        assert not [o for o in inner if o.startswith(("global_", "flat_", "buffer_", "scratch_", "ds_", "s_barrier"))], key
        assert not [o for o in inner if "atomic" in o], key
        hs_inner = loop_mix.per_nonce_loop(hs[key])
        assert sum(o.startswith("s_load") for o in inner) <= sum(o.startswith("s_load") for o in hs_inner), key


def listed_excess():
    """{(J, MODE): (valu excess, half excess)} of the layouts DESIGN.md lists for batch_bound."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("batch_bound loops above hits_stop's"):]
    sec = sec[:sec.index("\n\n")]
    return {(int(j), int(m)): (int(v), int(h))
            for j, m, v, h in re.findall(r"<(\d+), (\d)>: \+(\d+) VALU, \+(\d+) half-rate", sec)}


def test_loops_issue_no_more_than_hits_stops():
    bb = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_batch_bound_prio.s")).read(), loop_mix.BATCH_BOUND, whole=True)
    hs = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_hits_stop_prio.s")).read(), loop_mix.HITS_STOP)
    assert set(bb) == set(hs) == {f"{j},{m}" for j, m in KERNELS}
    assert all(v["valu"] > 1000 for v in bb.values())          # a whole per-nonce loop was found
    assert {v["loop_spill_ops"] for v in bb.values()} == {0}
    over = {tuple(int(x) for x in k.split(",")): (max(0, bb[k]["valu"] - hs[k]["valu"]), max(0, bb[k]["half"] - hs[k]["half"]))
            for k in hs if bb[k]["valu"] > hs[k]["valu"] or bb[k]["half"] > hs[k]["half"]}
    for k, (v, h) in sorted(over.items()):
        print("<%d, %d>: +%d VALU, +%d half-rate" % (k + (v, h)))
    assert all(v <= MAX_EXCESS and h <= MAX_EXCESS for v, h in over.values()), over
    assert over == listed_excess(), (over, listed_excess())     # each such layout is listed with its excess


def _compiler():
    out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True,
                         text=True).stdout
    return next((l.strip() for l in out.splitlines() if "clang version" in l), "")


def test_existing_code_objects_are_the_parents():
    """The bytes every existing call loads did not change: each code object built from
    fast_search.hip before this feature -- the nine embedded ones, hits_stop (the yardstick above)
    among them, and the two coarse-hash test variants -- and the loop mix bench.py reads, hash as the
    parent commit's build did.  A code object's bytes belong to one compiler, so the recorded hashes
    hold for the recorded compiler only."""
    want = json.load(open(os.path.join(GOLDEN, "parent_code_objects_first_hits_batch.json")))
    if _compiler() != want["compiler"]:
        pytest.skip("another compiler than the recorded hashes': " + _compiler())
    files = [f for f in want if f not in ("comment", "compiler")]
    assert sorted(files) == ["fast_batch.hsaco", "fast_batch_first.hsaco", "fast_batch_first_stop.hsaco",
                             "fast_batch_hits.hsaco", "fast_batch_keep.hsaco", "fast_first.hsaco", "fast_first_stop.hsaco",
                             "fast_hits.hsaco", "fast_hits_stop.hsaco", "fast_loop_mix.json", "fast_search.hsaco",
                             "fast_search_keep.hsaco"]
    for f in files:
        assert hashlib.sha256(open(os.path.join(BUILD, f), "rb").read()).hexdigest() == want[f], f
    before = json.load(open(os.path.join(GOLDEN, "parent_code_objects_batch_stop.json")))
    assert all(before[f] == want[f] for f in before if f not in ("comment", "compiler"))


def test_new_names_appear_only_under_the_three_macros():
    """In fast_search.hip, batch_bound and BatchBoundItem appear only where MH_BATCH, MH_HITS and
    MH_STOP are all defined (test_first_hits_guards.cut: the file as the preprocessor sees it)."""
    from test_first_hits_guards import cut
    src = open(os.path.join(CSRC, "fast_search.hip")).read()
    new = r"batch_bound|BatchBound"
    assert len(re.findall(r"batch_bound<j, m>", src)) == 1
    for macro in ("MH_BATCH", "MH_HITS", "MH_STOP"):
        assert re.search(new, cut(src, macro, True)) and not re.search(new, cut(src, macro, False)), macro
