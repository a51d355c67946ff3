"""Static guards on the stopping first-hit code object (CPU, no GPU touched).

mh_search_first_ex(MH_FIRST_STOP_RUNNING) runs stop_scan<J, MODE>: fast_search.hip built with
-DMH_FIRST -DMH_STOP through the product's passes into build/fast_first_stop.hsaco, embedded in the
library as a blob of its own (mh_first_stop_co_begin).  The poll sits outside the per-nonce loop and
may cost that loop nothing, and the feature must leave every other code object alone:

  * the blob holds one stop_scan kernel per entry of layout.hpp's MH_FAST_KERNELS and no other
    kernel; no other blob holds a stop_scan kernel;
  * per <J, MODE> the per-nonce loop issues no more VALU instructions and no more half-rate ones
    than the product kernel's loop (csrc/loop_mix.py over build/fast_first_stop_prio.s against
    build/fast_loop_mix.json), with no private-memory access inside it;
  * per <J, MODE> the register file holds no fewer waves per SIMD than with the product kernel;
  * the poll is a vector load past the CU's L1 (sc1), once per group: never a scalar-cache load of
    the word other workgroups' atomics write;
  * build/fast_search.hsaco and build/fast_loop_mix.json are the recorded parent's
    (tests/golden/product_code_object.json), and build/fast_first.hsaco is what the same sources
    give with MH_STOP undefined: the recorded bytes of the commit before the feature
    (tests/golden/first_code_object.json, per compiler), and the same translation unit as
    fast_search.hip with every MH_STOP branch cut out;
  * everything the feature added to fast_search.hip sits under MH_STOP.
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

STOP_NAME = r"_ZN2mh9stop_scanILi(\d+)ELi(\d+)EEEvNS_8FastArgsEPNS_7PartialENS_9FirstArgsE$"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_stop_code_object_holds_one_kernel_per_layout():
    co = codeobj.first_stop_code_object()
    assert co == open(os.path.join(BUILD, "fast_first_stop.hsaco"), "rb").read()
    names = [k[".name"] for k in codeobj.metadata(co)["amdhsa.kernels"]]
    got = [tuple(int(x) for x in re.match(STOP_NAME, n).groups()) for n in names]   # every kernel is a stop_scan
    assert len(got) == len(KERNELS) == 26 and set(got) == KERNELS == loop_mix.fast_kernels()
    # first_scan's parameters: FastArgs by value at its product size, the partials pointer, FirstArgs
    ks = codeobj.metadata(co)["amdhsa.kernels"]
    assert {tuple(a[".size"] for a in k[".args"][:3]) for k in ks} == {(520, 8, 24)}
    assert b"mh_fast_queue_args" in co and b"mh_fast_hash_keep" not in co and b"mh_dev_hash_xor" not in co
    # and no other blob knows anything of it
    for other in (codeobj.fast_code_object(), codeobj.first_code_object(), codeobj.hits_code_object(),
                  codeobj.batch_code_object(), codeobj.batch_first_code_object(), codeobj.batch_hits_code_object()):
        assert b"stop_scan" not in other and other != co


def test_stop_loops_issue_no_more_than_the_products():
    stop = loop_mix.loop_mix(open(os.path.join(BUILD, "fast_first_stop_prio.s")).read(), loop_mix.STOP)
    prod = json.load(open(os.path.join(BUILD, "fast_loop_mix.json")))
    assert set(stop) == set(prod) == {f"{j},{m}" for j, m in KERNELS}
    # the product's own file is what its assembly gives (the comparison is like for like)
    assert prod == loop_mix.loop_mix(open(os.path.join(BUILD, "fast_search_prio.s")).read())
    worse = {k: (stop[k], prod[k]) for k in prod
             if stop[k]["valu"] > prod[k]["valu"] or stop[k]["half"] > prod[k]["half"]}
    assert not worse, worse
    assert all(v["valu"] > 1000 for v in stop.values())         # a whole per-nonce loop was found
    assert {v["loop_spill_ops"] for v in stop.values()} == {0}


def test_stop_kernels_keep_the_products_occupancy():
    stop, prod = codeobj.first_stop_kernel_resources(), codeobj.fast_kernel_resources()
    assert set(stop) == set(prod) == KERNELS
    lower = {k: (stop[k], prod[k]) for k in prod
             if stop[k]["max_waves_per_simd"] < prod[k]["max_waves_per_simd"]}
    assert not lower, lower
    assert {v["lds_bytes"] for v in stop.values()} == {v["lds_bytes"] for v in prod.values()}


def test_the_poll_is_a_vector_load_outside_the_per_nonce_loop():
    """Per kernel: the word is read by `global_load_dwordx2 ... sc1` (a relaxed agent-scope load,
    served past the CU's L1) -- in claim_first, as first_scan reads it, and once more in the group
    loop's header block -- and the per-nonce loop holds no load, atomic or barrier of its own."""
    text = open(os.path.join(BUILD, "fast_first_stop_prio.s")).read()
    first = loop_mix.kernels(open(os.path.join(BUILD, "fast_first_prio.s")).read())
    first = {loop_mix.FIRST.match(n).groups(): b for n, b in first.items() if loop_mix.FIRST.match(n)}
    seen = 0
    for name, body in loop_mix.kernels(text).items():
        m = loop_mix.STOP.match(name)
        if not m:
            continue
        seen += 1
        polls = [l for l in body.split("\n") if re.match(r"\s+global_load_dwordx2 .* sc1\s*$", l)]
        claims = [l for l in first[m.groups()].split("\n") if re.match(r"\s+global_load_dwordx2 .* sc1\s*$", l)]
        assert len(polls) == len(claims) + 1, (name, len(polls), len(claims))
        inner = loop_mix.per_nonce_loop(body)
        assert not [o for o in inner if o.startswith(("global_", "flat_", "buffer_", "s_barrier"))], name
        first_inner = loop_mix.per_nonce_loop(first[m.groups()])    # (scalar loads: the sigma table's, as first_scan's)
        assert sum(o.startswith("s_load") for o in inner) <= sum(o.startswith("s_load") for o in first_inner), name
        # the published hit and the chunk end's: vector atomics, one more than first_scan has
        umin = lambda b: sum("global_atomic_umin_x2" in l for l in b.split("\n"))     # noqa: E731
        assert umin(body) == umin(first[m.groups()]) + 1, name
    assert seen == len(KERNELS)


def _compiler():
    out = subprocess.run([HIPCC, "--version"], capture_output=True, text=True).stdout
    return next((l.strip() for l in out.splitlines() if "clang version" in l), "")


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_product_code_object_is_the_parents():
    want = json.load(open(os.path.join(GOLDEN, "product_code_object.json")))
    if _compiler() != want["compiler"]:
        pytest.skip("another compiler than the recorded hashes': " + _compiler())
    for f in ("fast_search.hsaco", "fast_loop_mix.json"):
        assert _sha(os.path.join(BUILD, f)) == want[f], f
    assert codeobj.fast_code_object() == open(os.path.join(BUILD, "fast_search.hsaco"), "rb").read()


def without_mh_stop(src):
    """fast_search.hip as the preprocessor sees it with MH_STOP undefined: every `#ifdef MH_STOP`
    branch cut, every `#else` branch of one kept, line for line (cut lines stay as empty lines, so
    line numbers hold).  MH_STOP appears in no other kind of conditional."""
    out, stack = [], []             # stack of (this branch is taken, the condition was about MH_STOP)
    for line in src.split("\n"):
        s = line.strip()
        directive = True
        if re.match(r"#\s*if", s):
            m = re.match(r"#\s*(ifdef|ifndef)\s+MH_STOP\b", s)
            assert m or "MH_STOP" not in s, s
            stack.append((m.group(1) == "ifndef", True) if m else (True, False))
            directive = bool(m)
        elif re.match(r"#\s*else", s):
            taken, stop = stack.pop()
            stack.append((not taken if stop else taken, stop))
            directive = stop
        elif re.match(r"#\s*elif", s):
            assert not stack[-1][1], "no #elif on an MH_STOP conditional"
            directive = False
        elif re.match(r"#\s*endif", s):
            directive = stack.pop()[1]
        else:
            directive = False
        cut = directive or not all(t for t, st in stack if st)
        out.append("" if cut else line)
    assert not stack
    return "\n".join(out)


def test_everything_new_in_the_kernel_source_is_under_mh_stop():
    src = open(os.path.join(CSRC, "fast_search.hip")).read()
    assert re.search(r"stop_scan", src) and re.search(r"#ifdef MH_STOP", src)
    left = without_mh_stop(src)
    left = re.sub(r"/\*.*?\*/", "", left, flags=re.S)
    left = re.sub(r"//[^\n]*", "", left)
    assert "first_scan" in left and "claim_first" in left and "MH_FAST_KERNELS(MH_INST)" in left
    assert not re.search(r"MH_STOP|stop_scan|KStop|\bsk\b|\bks\b", left)
    # what the feature's code uses appears, outside MH_STOP, only where first_scan had it
    assert left.count("chunk_floor") == 3 and left.count("f.scanned") == 2 and left.count("atomicMin") == 1
    assert left.count("for (uint32_t g = 0; g < a.n_groups; ++g) {") == 1


def test_first_code_object_is_the_one_without_mh_stop(tmp_path):
    """build/fast_first.hsaco equals the one the same sources give with MH_STOP undefined.  Its
    bytes are the recorded ones of the commit before the feature (per compiler); and the compiler
    is handed the same translation unit with or without the MH_STOP branches in the file: the
    device-side preprocessed text of fast_search.hip -DMH_FIRST equals that of the cut source."""
    want = json.load(open(os.path.join(GOLDEN, "first_code_object.json")))
    assert codeobj.first_code_object() == open(os.path.join(BUILD, "fast_first.hsaco"), "rb").read()
    src = open(os.path.join(CSRC, "fast_search.hip")).read()
    cut = tmp_path / "fast_search.hip"
    cut.write_text(without_mh_stop(src))

    def pre(path, *defs):
        r = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-E", "-P",
                            "-I", CSRC, *defs, str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout
    tree = pre(os.path.join(CSRC, "fast_search.hip"), "-DMH_FIRST")
    assert "first_scan" in tree and "stop_scan" not in tree
    assert tree == pre(cut, "-DMH_FIRST")
    assert tree == pre(cut, "-DMH_FIRST", "-DMH_STOP")          # nothing of MH_STOP is left in the cut source
    assert "stop_scan" in pre(os.path.join(CSRC, "fast_search.hip"), "-DMH_FIRST", "-DMH_STOP")
    if _compiler() != want["compiler"]:
        pytest.skip("another compiler than the recorded hash's: " + _compiler())
    assert _sha(os.path.join(BUILD, "fast_first.hsaco")) == want["fast_first.hsaco"]
