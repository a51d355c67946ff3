"""Static guards on the batch kernels of csrc/search_kernels.hip (CPU, no GPU touched).

mh_search_hits_batch runs batch_scan_hits: batch_scan with an append of every hit on a rare branch
of the per-nonce loop.  The append may not cost the kernel its occupancy, and adding the kernel may
not change its siblings: search_kernels.hip is compiled to gfx950 assembly with the Makefile's
flags and the kernels' metadata is read.

  * batch_scan_hits uses no scratch, spills no VGPR and needs at most 128 VGPRs: four waves per
    SIMD, as batch_scan;
  * batch_scan and batch_scan_first keep the register counts they had before the feature (125 and
    127 VGPRs) and stay without scratch.

These are conditions of the build, not measurements.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "bitcoin-miner_amd", "csrc")


def _makefile_var(name):
    text = open(os.path.join(ROOT, "Makefile")).read()
    return re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1).strip()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel function name: {metadata key: int}} of search_kernels.hip's gfx950 assembly, compiled once."""
    tmp = str(tmp_path_factory.mktemp("asm"))
    hipcc = os.environ.get("HIPCC", _makefile_var("HIPCC"))
    arch = os.environ.get("ARCH", _makefile_var("ARCH"))
    flags = _makefile_var("HIPFLAGS").replace("$(ARCH)", arch).split()
    out = os.path.join(tmp, "search_kernels.s")
    r = subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "search_kernels.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"^  - ", meta, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M)
        if not name:
            continue
        m = re.match(r"_ZN2mh(\d+)", name.group(1))
        short = name.group(1)[len(m.group(0)):][:int(m.group(1))] if m else name.group(1)
        kernels[short] = {k: int(v) for k, v in re.findall(r"^\s+\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_batch_scan_hits_keeps_four_waves_per_simd(kernels):
    k = kernels
    assert {"batch_scan", "batch_scan_first", "batch_scan_hits", "merge_segments_hits"} <= set(k), sorted(k)
    hits = k["batch_scan_hits"]
    assert hits["private_segment_fixed_size"] == 0 and hits["vgpr_spill_count"] == 0, hits
    assert hits["vgpr_count"] <= 128, hits
    assert hits.get("agpr_count", 0) == 0 and hits["max_flat_workgroup_size"] == 256, hits


def test_the_sibling_kernels_keep_their_registers(kernels):
    k = kernels
    for name, vgprs in (("batch_scan", 125), ("batch_scan_first", 127)):
        assert k[name]["vgpr_count"] == vgprs, (name, k[name])
        assert k[name]["private_segment_fixed_size"] == 0 and k[name]["vgpr_spill_count"] == 0, (name, k[name])
