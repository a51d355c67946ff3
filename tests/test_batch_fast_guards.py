"""Static guards on the batch code objects (CPU, no GPU touched).

mh_search_batch_ex(MH_BATCH_FUSE_FAST) runs batch_fast<J, MODE>: fast_search.hip built with
-DMH_BATCH through the product's passes into build/fast_batch.hsaco, embedded in the library as a
fourth blob (mh_batch_co_begin); build/fast_batch_keep.hsaco (-DMH_BATCH -DMH_HASH_KEEP) is its
test variant for the dev build.  The per-nonce loop is the product's, so for each of the 26 layouts:

  * the loop issues the product loop's half-rate VALU count exactly and no more VALU instructions
    than the product's loop (csrc/loop_mix.py over build/fast_batch_prio.s against
    build/fast_loop_mix.json).  The compiler emits up to two full-rate register moves fewer in
    some batch loops (the chunk body is not inside a work-queue loop there), never an instruction
    more, so the VALU count is bounded from both sides: product - 2 <= batch <= product;
  * no private-memory access inside the loop;
  * the register file holds the product kernel's waves per SIMD.

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

BATCH_NAME = r"_ZN2mh10batch_fastILi(\d+)ELi(\d+)EEEvPKNS_13BatchFastItemEPKjPNS_7PartialE$"


def test_batch_code_object_holds_one_kernel_per_layout():
    co = codeobj.batch_code_object()
    assert co == open(os.path.join(BUILD, "fast_batch.hsaco"), "rb").read()
    kernels = codeobj.metadata(co)["amdhsa.kernels"]
    got = [tuple(int(x) for x in re.match(BATCH_NAME, k[".name"]).groups()) for k in kernels]
    assert len(got) == len(KERNELS) == 26 and set(got) == KERNELS == loop_mix.fast_kernels()
    # three pointers: the items, the per-chunk item table, the partials
    assert {tuple(a[".size"] for a in k[".args"][:3]) for k in kernels} == {(8, 8, 8)}
    assert b"mh_fast_batch_items" in co and b"mh_fast_hash_keep" not in co and b"mh_dev_hash_xor" not in co
    # the other blobs know nothing of it
    for other in (codeobj.fast_code_object(), codeobj.first_code_object(), codeobj.hits_code_object()):
        assert b"batch_fast" not in other and other != co


def test_keep_variant_holds_the_same_kernels_and_the_hooks():
    keep = open(os.path.join(BUILD, "fast_batch_keep.hsaco"), "rb").read()
    names = {k[".name"] for k in codeobj.metadata(keep)["amdhsa.kernels"]}
    assert names == {k[".name"] for k in codeobj.metadata(codeobj.batch_code_object())["amdhsa.kernels"]}
    assert b"mh_fast_batch_items" in keep and b"mh_fast_hash_keep" in keep and b"mh_dev_hash_xor" in keep
    assert set(codeobj.batch_kernel_resources(keep)) == KERNELS
    # the variant pays for its hooks outside the product: only its loops' private memory is guarded
    mix = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_batch_keep_prio.s")).read(), loop_mix.BATCH)
    assert set(mix) == {f"{j},{m}" for j, m in KERNELS} and {v["loop_spill_ops"] for v in mix.values()} == {0}


def test_batch_loops_are_the_products():
    batch = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_batch_prio.s")).read(), loop_mix.BATCH)
    prod = json.load(open(os.path.join(BUILD, "fast_loop_mix.json")))
    assert set(batch) == set(prod) == {f"{j},{m}" for j, m in KERNELS}
    # the product's own file is what its assembly gives (the comparison is like for like)
    assert prod == loop_mix.loop_mix(open(os.path.join(BUILD, "fast_search_prio.s")).read())
    off = {k: (batch[k], prod[k]) for k in prod
           if batch[k]["half"] != prod[k]["half"] or not prod[k]["valu"] - 2 <= batch[k]["valu"] <= prod[k]["valu"]}
    assert not off, off
    assert all(v["valu"] > 1000 for v in batch.values())        # a whole per-nonce loop was found
    assert {v["loop_spill_ops"] for v in batch.values()} == {0}


def test_batch_kernels_keep_the_products_occupancy():
    batch, prod = codeobj.batch_kernel_resources(), codeobj.fast_kernel_resources()
    assert set(batch) == set(prod) == KERNELS
    lower = {k: (batch[k], prod[k]) for k in prod
             if batch[k]["max_waves_per_simd"] < prod[k]["max_waves_per_simd"]}
    assert not lower, lower
