"""Static guards on the first-hit code object (CPU, no GPU touched).

mh_search_first runs first_scan<J, MODE>: fast_search.hip built with -DMH_FIRST through the
product's passes into build/fast_first.hsaco, embedded in the library as a second blob
(mh_first_co_begin).  The feature may cost the per-nonce loop nothing and must leave the product's
code object alone:

  * the blob holds one first_scan kernel per entry of layout.hpp's MH_FAST_KERNELS, and no
    fast_search kernel; the product's blob holds no first_scan kernel;
  * per <J, MODE> the per-nonce loop issues no more VALU instructions and no more half-rate ones
    than the product kernel's loop (csrc/loop_mix.py over build/fast_first_prio.s against
    build/fast_loop_mix.json), with no private-memory access inside it;
  * per <J, MODE> the register file holds no fewer waves per SIMD than with the product kernel;
  * build/fast_search.hsaco and build/fast_loop_mix.json are byte-identical to the build of the
    commit before the feature (tests/golden/product_code_object.json, per compiler), and everything
    the feature added to fast_search.hip sits under MH_FIRST.
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

FIRST_NAME = r"_ZN2mh10first_scanILi(\d+)ELi(\d+)EEEvNS_8FastArgsEPNS_7PartialENS_9FirstArgsE$"


def first_kernels(co):
    return [k for k in codeobj.metadata(co)["amdhsa.kernels"] if "first_scan" in k[".name"]]


def test_first_code_object_holds_one_kernel_per_layout():
    co = codeobj.first_code_object()
    assert co == open(os.path.join(BUILD, "fast_first.hsaco"), "rb").read()
    ks = first_kernels(co)
    got = [tuple(int(x) for x in re.match(FIRST_NAME, k[".name"]).groups()) for k in ks]
    assert len(got) == len(KERNELS) and set(got) == KERNELS == loop_mix.fast_kernels()
    names = [k[".name"] for k in codeobj.metadata(co)["amdhsa.kernels"]]
    assert len(names) == len(KERNELS) and not [n for n in names if "fast_search" in n]
    # FastArgs by value at its product size, then the partials pointer, then FirstArgs (24 bytes)
    assert {tuple(a[".size"] for a in k[".args"][:3]) for k in ks} == {(520, 8, 24)}
    assert b"mh_fast_queue_args" in co and b"mh_fast_hash_keep" not in co and b"mh_dev_hash_xor" not in co
    # and the product's blob knows nothing of it
    prod = codeobj.fast_code_object()
    assert b"first_scan" not in prod and prod != co


def test_first_loops_issue_no_more_than_the_products():
    first = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_first_prio.s")).read(), loop_mix.FIRST)
    prod = json.load(open(os.path.join(BUILD, "fast_loop_mix.json")))
    assert set(first) == set(prod) == {f"{j},{m}" for j, m in KERNELS}
    # the product's own file is what its assembly gives (the comparison is like for like)
    assert prod == loop_mix.loop_mix(open(os.path.join(BUILD, "fast_search_prio.s")).read())
    worse = {k: (first[k], prod[k]) for k in prod
             if first[k]["valu"] > prod[k]["valu"] or first[k]["half"] > prod[k]["half"]}
    assert not worse, worse
    assert all(v["valu"] > 1000 for v in first.values())        # a whole per-nonce loop was found
    assert {v["loop_spill_ops"] for v in first.values()} == {0}


def test_first_kernels_keep_the_products_occupancy():
    first, prod = codeobj.first_kernel_resources(), codeobj.fast_kernel_resources()
    assert set(first) == set(prod) == KERNELS
    lower = {k: (first[k], prod[k]) for k in prod
             if first[k]["max_waves_per_simd"] < prod[k]["max_waves_per_simd"]}
    assert not lower, lower
    assert {v["lds_bytes"] for v in first.values()} == {v["lds_bytes"] for v in prod.values()}


def _compiler():
    out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True,
                         text=True).stdout
    return next((l.strip() for l in out.splitlines() if "clang version" in l), "")


def test_product_code_object_is_the_parents():
    """The bytes every mh_search loads did not change: build/fast_search.hsaco (and the loop mix
    bench.py reads) hash as the parent commit's build did.  A code object's bytes belong to one
    compiler, so the recorded hashes hold for the recorded compiler only."""
    want = json.load(open(os.path.join(GOLDEN, "product_code_object.json")))
    if _compiler() != want["compiler"]:
        pytest.skip("another compiler than the recorded hashes': " + _compiler())
    for f in ("fast_search.hsaco", "fast_loop_mix.json"):
        assert hashlib.sha256(open(os.path.join(BUILD, f), "rb").read()).hexdigest() == want[f], f
    assert codeobj.fast_code_object() == open(os.path.join(BUILD, "fast_search.hsaco"), "rb").read()


def test_everything_new_in_the_kernel_source_is_under_mh_first():
    """fast_search.hip with MH_FIRST undefined, comments removed, mentions nothing of the feature:
    the product build cannot have picked any of it up."""
    src = open(os.path.join(CSRC, "fast_search.hip")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    keep, stack = [], []            # stack of (this branch is taken, the condition was about MH_FIRST)
    for line in src.split("\n"):
        s = line.strip()
        if re.match(r"#\s*if", s):
            m = re.match(r"#\s*(ifdef|ifndef)\s+MH_FIRST\b", s)
            stack.append((m.group(1) == "ifndef", True) if m else (True, False))
            assert m or "MH_FIRST" not in s, s
        elif re.match(r"#\s*else", s):
            taken, first = stack.pop()
            stack.append((not taken if first else taken, first))
        elif re.match(r"#\s*elif", s):
            assert not stack[-1][1], "no #elif on an MH_FIRST conditional"
        elif re.match(r"#\s*endif", s):
            stack.pop()
        elif all(t for t, _ in stack):
            keep.append(line)
    assert not stack
    left = "\n".join(keep)
    assert "fast_search" in left and "MH_FAST_KERNELS(MH_INST)" in left
    assert not re.search(r"MH_FIRST|FirstArgs|FirstKernArgs|first_args|first_scan|claim_first|chunk_floor", left)
