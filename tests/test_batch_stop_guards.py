"""Static guards on the stopping first-hit batch code object (CPU, no GPU touched).

mh_search_first_batch_stop runs batch_stop<J, MODE>: fast_search.hip built with -DMH_BATCH -DMH_FIRST
-DMH_STOP through the product's passes into build/fast_batch_first_stop.hsaco, embedded in the
library as a blob of its own (mh_batch_first_stop_co_begin).  The wrapper is batch_first's and the
chunk body stop_scan's, so for each of the 26 layouts:

  * the blob holds one batch_stop kernel and nothing else, its own marker (sized as BatchFirstItem)
    and no hook symbols, and no other blob contains it;
  * the per-nonce loop issues batch_first's half-rate VALU count exactly and no more VALU
    instructions than batch_first's loop (csrc/loop_mix.py over the two _prio.s files, whole-function
    mode), with no private-memory access inside it;
  * the register file holds no fewer waves per SIMD than with the product kernel;
  * the per-nonce loop holds no global, flat or buffer access and no barrier; against batch_first
    the kernel has one more `global_load_dwordx2 ... sc1` (the poll, once per group) and one more
    global_atomic_umin_x2 (the published hit), and as many global_atomic_add_x2: the wrapper's
    up-front add of `scanned` is gone, the waves' add at the chunk's end replaces it one for one;
  * every code object that existed before, and build/fast_loop_mix.json, is byte-identical to the
    parent commit's build (tests/golden/parent_code_objects_batch_stop.json, per compiler).

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

NAME = r"_ZN2mh10batch_stopILi(\d+)ELi(\d+)EEEvPKNS_14BatchFirstItemEPKjS5_PNS_7PartialE$"


def test_stop_batch_code_object_holds_one_kernel_per_layout():
    co = codeobj.batch_first_stop_code_object()
    assert co == open(os.path.join(BUILD, "fast_batch_first_stop.hsaco"), "rb").read()
    kernels = codeobj.metadata(co)["amdhsa.kernels"]
    got = [tuple(int(x) for x in re.match(NAME, k[".name"]).groups()) for k in kernels]    # every kernel is a batch_stop
    assert len(got) == len(KERNELS) == 26 and set(got) == KERNELS == loop_mix.fast_kernels()
    # batch_first's four pointers: the items, the per-chunk item table, the order table, the partials
    assert {tuple(a[".size"] for a in k[".args"][:4]) for k in kernels} == {(8, 8, 8, 8)}
    assert all(len(k[".args"]) == 4 or k[".args"][4].get(".value_kind", "").startswith("hidden") for k in kernels)
    # its own marker, none of the others', no hook symbols, no other kernel family
    assert b"mh_fast_batch_stop_items" in co
    for other in (b"mh_fast_batch_items", b"mh_fast_batch_first_items", b"mh_fast_batch_hits_items", b"mh_fast_queue_args",
                  b"mh_fast_hash_keep", b"mh_dev_hash_xor", b"stop_scan", b"first_scan", b"batch_fast", b"batch_first",
                  b"batch_hits", b"fast_search", b"hits_scan"):
        assert other not in co, other
    # no other blob knows anything of it
    for other in (codeobj.fast_code_object(), codeobj.first_code_object(), codeobj.hits_code_object(),
                  codeobj.batch_code_object(), codeobj.batch_first_code_object(), codeobj.batch_hits_code_object(),
                  codeobj.first_stop_code_object()):
        assert b"batch_stop" not in other and other != co
    for f in ("fast_search_keep.hsaco", "fast_batch_keep.hsaco"):
        assert b"batch_stop" not in open(os.path.join(BUILD, f), "rb").read(), f


def test_marker_is_sized_as_the_item_struct():
    """layout.hpp BatchFirstItem: FastArgs (520), the unused pointer, FirstArgs (24), chunk0, slot0."""
    readelf = os.path.join(os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin"), "llvm-readelf")   # the Makefile's LLVM
    if not os.path.exists(readelf):
        pytest.skip("no llvm-readelf")
    r = subprocess.run([readelf, "-sW", os.path.join(BUILD, "fast_batch_first_stop.hsaco")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes = {int(l.split()[2]) for l in r.stdout.splitlines() if l.split()[-1:] == ["mh_fast_batch_stop_items"]}
    assert sizes == {520 + 8 + 24 + 8} == {560}     # in .dynsym and .symtab alike


def test_batch_stop_loops_are_batch_firsts():
    """Per layout: no more VALU and exactly as many half-rate instructions as batch_first's loop.

    With the chunk body as stop_scan has it and nothing more, eight loops issued one or two more
    full-rate adds than batch_first's (<2, Pre>, <3, One>, <3, Pre>, <4, One> one, <10..13, One>
    two): a store inside the group loop -- the published hit -- made the compiler leave
    `K[t] + W[t]` sums of group-level words in the per-nonce loop.  The batch_stop build therefore
    makes those sums opaque per group, as the run-level ones are, and takes round J's two outputs
    from two pre-added group-level registers (fast_search.hip, under MH_STOP and MH_BATCH): as built
    by AMD clang 22.0.0git (roc-7.2.0) every loop now issues 0 to 3 fewer VALU instructions than
    batch_first's and the same half-rate count."""
    bs = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_batch_first_stop_prio.s")).read(), loop_mix.BATCH_STOP,
                           whole=True)
    bf = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_batch_first_prio.s")).read(), loop_mix.BATCH_FIRST,
                           whole=True)
    assert set(bs) == set(bf) == {f"{j},{m}" for j, m in KERNELS}
    for k in sorted(bf, key=lambda s: tuple(int(x) for x in s.split(","))):
        print("<%s>: batch_stop %s, batch_first %s" % (k, bs[k], bf[k]))
    assert all(v["valu"] > 1000 for v in bs.values())          # a whole per-nonce loop was found
    assert {v["loop_spill_ops"] for v in bs.values()} == {0}
    assert not {k: (bs[k]["half"], bf[k]["half"]) for k in bf if bs[k]["half"] != bf[k]["half"]}
    off = {k: (bs[k]["valu"], bf[k]["valu"]) for k in bf if bs[k]["valu"] > bf[k]["valu"]}
    assert not off, off


def test_batch_stop_kernels_keep_the_products_occupancy():
    bs, prod = codeobj.batch_first_stop_kernel_resources(), codeobj.fast_kernel_resources()
    assert set(bs) == set(prod) == KERNELS
    lower = {k: (bs[k], prod[k]) for k in prod if bs[k]["max_waves_per_simd"] < prod[k]["max_waves_per_simd"]}
    assert not lower, lower
    assert {v["lds_bytes"] for v in bs.values()} == {v["lds_bytes"] for v in codeobj.batch_first_kernel_resources().values()}


def test_the_poll_and_the_atomics():
    """Per kernel against batch_first's: the word is read by `global_load_dwordx2 ... sc1` (a relaxed
    agent-scope load, served past the CU's L1) once in the wrapper, as batch_first reads it, and once
    more in the group loop; one more global_atomic_umin_x2 (the published hit; the chunk end's is
    batch_first's); global_atomic_add_x2: found 1 in every batch_stop kernel and 1 in every
    batch_first kernel -- the wrapper's add is gone and the waves' add replaces it one for one.  The
    per-nonce loop holds no load, store, atomic or barrier of its own."""
    stop = loop_mix.kernels(open(os.path.join(BUILD, "fast_batch_first_stop_prio.s")).read(), whole=True)
    first = loop_mix.kernels(open(os.path.join(BUILD, "fast_batch_first_prio.s")).read(), whole=True)
    first = {loop_mix.BATCH_FIRST.match(n).groups(): b for n, b in first.items() if loop_mix.BATCH_FIRST.match(n)}
    count = lambda body, pat: sum(bool(re.search(pat, l)) for l in body.split("\n"))     # noqa: E731
    seen = 0
    for name, body in stop.items():
        m = loop_mix.BATCH_STOP.match(name)
        if not m:
            continue
        seen += 1
        other = first[m.groups()]
        poll = r"^\s+global_load_dwordx2 .* sc1\s*$"
        assert count(body, poll) == count(other, poll) + 1 == 2, (name, count(body, poll), count(other, poll))
        assert count(body, "global_atomic_umin_x2") == count(other, "global_atomic_umin_x2") + 1 == 2, name
        assert count(body, "global_atomic_add_x2") == count(other, "global_atomic_add_x2") == 1, name
        inner = loop_mix.per_nonce_loop(body)
        assert not [o for o in inner if o.startswith(("global_", "flat_", "buffer_", "scratch_", "s_barrier"))], name
        other_inner = loop_mix.per_nonce_loop(other)       # (scalar loads: the sigma table's, as batch_first's)
        assert sum(o.startswith("s_load") for o in inner) <= sum(o.startswith("s_load") for o in other_inner), name
    assert seen == len(KERNELS)


def _compiler():
    out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True,
                         text=True).stdout
    return next((l.strip() for l in out.splitlines() if "clang version" in l), "")


def test_existing_code_objects_are_the_parents():
    """The bytes every existing call loads did not change: each code object built from
    fast_search.hip before this feature -- the seven embedded ones and the two coarse-hash test
    variants -- and the loop mix bench.py reads, hash as the parent commit's build did.  A code
    object's bytes belong to one compiler, so the recorded hashes hold for the recorded compiler only."""
    want = json.load(open(os.path.join(GOLDEN, "parent_code_objects_batch_stop.json")))
    if _compiler() != want["compiler"]:
        pytest.skip("another compiler than the recorded hashes': " + _compiler())
    files = [f for f in want if f not in ("comment", "compiler")]
    assert sorted(files) == ["fast_batch.hsaco", "fast_batch_first.hsaco", "fast_batch_hits.hsaco", "fast_batch_keep.hsaco",
                             "fast_first.hsaco", "fast_first_stop.hsaco", "fast_hits.hsaco", "fast_loop_mix.json",
                             "fast_search.hsaco", "fast_search_keep.hsaco"]
    for f in files:
        assert hashlib.sha256(open(os.path.join(BUILD, f), "rb").read()).hexdigest() == want[f], f
    before = json.load(open(os.path.join(GOLDEN, "parent_code_objects_hits_batch.json")))
    assert all(before[f] == want[f] for f in before if f not in ("comment", "compiler"))
