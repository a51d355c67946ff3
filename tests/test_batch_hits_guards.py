"""Static guards on the hits batch code object (CPU, no GPU touched).

mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST) runs batch_hits<J, MODE>: fast_search.hip built with
-DMH_BATCH -DMH_HITS through the product's passes into build/fast_batch_hits.hsaco, embedded in the
library as a sixth blob (mh_batch_hits_co_begin).  The chunk body is hits_scan's, so for each of the
26 layouts:

  * the blob holds one batch_hits kernel and nothing else, its own marker and no hook symbols, and
    the other five blobs do not contain it;
  * the marker has the size of layout.hpp's BatchHitsItem;
  * the per-nonce loop issues hits_scan's half-rate VALU count exactly and no more VALU instructions
    than hits_scan's loop (csrc/loop_mix.py over build/fast_batch_hits_prio.s against
    build/fast_hits_prio.s), with no private-memory access inside it;
  * the register file holds no fewer waves per SIMD than with hits_scan;
  * every code object that existed before, and build/fast_loop_mix.json, is byte-identical to the
    parent commit's build (tests/golden/parent_code_objects_hits_batch.json, per compiler).

These are conditions of the build, not measurements.
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

NAME = r"_ZN2mh10batch_hitsILi(\d+)ELi(\d+)EEEvPKNS_13BatchHitsItemEPKjPNS_7PartialE$"


def test_sixth_code_object_holds_one_kernel_per_layout():
    co = codeobj.batch_hits_code_object()
    assert co == open(os.path.join(BUILD, "fast_batch_hits.hsaco"), "rb").read()
    kernels = codeobj.metadata(co)["amdhsa.kernels"]
    got = [tuple(int(x) for x in re.match(NAME, k[".name"]).groups()) for k in kernels]
    assert len(got) == len(KERNELS) == 26 and set(got) == KERNELS == loop_mix.fast_kernels()
    # three pointers: the items, the per-chunk item table, the partials
    assert {tuple(a[".size"] for a in k[".args"][:3]) for k in kernels} == {(8, 8, 8)}
    assert all(len(k[".args"]) == 3 or k[".args"][3].get(".value_kind", "").startswith("hidden") for k in kernels)
    # its own marker, none of the others', no hook symbols
    assert b"mh_fast_batch_hits_items" in co
    for other in (b"mh_fast_batch_items", b"mh_fast_batch_first_items", b"mh_fast_queue_args", b"mh_fast_hash_keep",
                  b"mh_dev_hash_xor", b"first_scan", b"batch_fast", b"batch_first", b"fast_search", b"hits_scan"):
        assert other not in co, other
    # the other five blobs know nothing of it
    for other in (codeobj.fast_code_object(), codeobj.first_code_object(), codeobj.hits_code_object(),
                  codeobj.batch_code_object(), codeobj.batch_first_code_object()):
        assert b"batch_hits" not in other and other != co


def test_marker_is_sized_as_the_item_struct():
    """layout.hpp BatchHitsItem: FastArgs (520), the unused pointer, HitsArgs (32), chunk0, slot0,
    padded to a multiple of 16."""
    readelf = os.path.join(os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin"), "llvm-readelf")   # the Makefile's LLVM
    if not os.path.exists(readelf):
        pytest.skip("no llvm-readelf")
    r = subprocess.run([readelf, "-sW", os.path.join(BUILD, "fast_batch_hits.hsaco")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes = {int(l.split()[2]) for l in r.stdout.splitlines() if l.split()[-1:] == ["mh_fast_batch_hits_items"]}
    assert sizes == {(520 + 8 + 32 + 8 + 15) // 16 * 16} == {576}     # in .dynsym and .symtab alike


def test_batch_hits_loops_are_hits_scans():
    bh = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_batch_hits_prio.s")).read(), loop_mix.BATCH_HITS)
    hits = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_hits_prio.s")).read(), loop_mix.HITS)
    assert set(bh) == set(hits) == {f"{j},{m}" for j, m in KERNELS}
    off = {k: (bh[k], hits[k]) for k in hits
           if bh[k]["half"] != hits[k]["half"] or bh[k]["valu"] > hits[k]["valu"]}
    assert not off, off
    assert all(v["valu"] > 1000 for v in bh.values())          # a whole per-nonce loop was found
    assert {v["loop_spill_ops"] for v in bh.values()} == {0}


def test_batch_hits_kernels_keep_hits_scans_occupancy():
    bh, hits = codeobj.batch_hits_kernel_resources(), codeobj.hits_kernel_resources()
    assert set(bh) == set(hits) == KERNELS
    lower = {k: (bh[k], hits[k]) for k in hits if bh[k]["max_waves_per_simd"] < hits[k]["max_waves_per_simd"]}
    assert not lower, lower


def _compiler():
    out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True,
                         text=True).stdout
    return next((l.strip() for l in out.splitlines() if "clang version" in l), "")


def test_existing_code_objects_are_the_parents():
    """The bytes every existing call loads did not change: each code object built from
    fast_search.hip before this feature, build/fast_batch_first.hsaco included, and the loop mix
    bench.py reads, hash as the parent commit's build did.  A code object's bytes belong to one
    compiler, so the recorded hashes hold for the recorded compiler only."""
    want = json.load(open(os.path.join(GOLDEN, "parent_code_objects_hits_batch.json")))
    if _compiler() != want["compiler"]:
        pytest.skip("another compiler than the recorded hashes': " + _compiler())
    files = [f for f in want if f not in ("comment", "compiler")]
    assert sorted(files) == ["fast_batch.hsaco", "fast_batch_first.hsaco", "fast_batch_keep.hsaco", "fast_first.hsaco",
                             "fast_hits.hsaco", "fast_loop_mix.json", "fast_search.hsaco", "fast_search_keep.hsaco"]
    for f in files:
        assert hashlib.sha256(open(os.path.join(BUILD, f), "rb").read()).hexdigest() == want[f], f
    before = json.load(open(os.path.join(GOLDEN, "parent_code_objects.json")))
    assert all(before[f] == want[f] for f in before if f not in ("comment", "compiler"))
