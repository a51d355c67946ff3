"""GPU tests of the batched hits search with fused fast pieces:
mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST), the batch_hits<J, MODE> kernels of the sixth embedded
code object, batch_scan_hits_slots and merge_segments_hits over slot segments.

Every expected value comes from the reference alone (test_hits.hits_ref: the oracle's hashes of the
whole range, in numpy).  Every request is also compared, in the child, with search_hits of the same
request under the same environment.  Before a test looks at the GPU's results it asserts, from
batch_plan_ex and the reference, the premises it rests on: which requests are fused with a kind-2
piece, the chunk counts, and that every reference count is within the cap where a full list is
expected.  One child process per test.

The shapes are test_gpu_batch_fast's, the smallest that plan a fast piece.  At target 2^64 // 10^3
one nonce in 1,000 qualifies, so nearly every 2,560-nonce chunk and tile holds a hit and piece,
chunk and tile borders are covered without placing hits."""
import json
import subprocess
import sys

import pytest

import minehip
from conftest import PKG, ROOT
from test_gpu_batch_fast import EXTRA, L2, L3, NO_EARLY, SHAPES, SLOTS
from test_hits import hits_ref

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
T6, T3 = 2 ** 64 // 10 ** 6, 2 ** 64 // 10 ** 3
ONE = SHAPES[0]          # ("cmu440", 1_048_000, 2_200_000): one piece of exactly 450 chunks plus one nonce
EDGE = SHAPES[1]         # ("cmu440", 0, 3_000_000): generic head, a last chunk of 64 lanes, one nonce behind it
assert ONE == (b"cmu440", 1_048_000, 2_200_000) and EDGE == (b"cmu440", 0, 3_000_000)

CHILD = """
import json, os, minehip
spec = json.load(open({path!r}))
out = []
def plain(res):
    return [[r[0], [list(e) for e in r[1]], list(r[2])] if isinstance(r, tuple) else ["error", r.code] for r in res]
for j in spec["jobs"]:
    kv = {{k: str(v) for k, v in j["env"].items()}}
    os.environ.update(kv)
    try:
        reqs = [(bytes.fromhex(m), lo, hi, T, c) for m, lo, hi, T, c in j["reqs"]]
        ok = [r for r in reqs if r[1] <= r[2] and len(r[0]) <= (1 << 20) and r[4] <= minehip.MH_HITS_MAX_CAP]
        if j.get("profile"):
            minehip.profile_enable(0, True)
            before = minehip.profile_read(0)
        d = dict(plan=minehip.batch_plan_ex([r[:3] for r in ok]) if j.get("plan", True) else None)
        if j.get("regions"):
            d["regions"] = minehip.hits_batch_regions(ok, fuse_fast=True)
        res = minehip.search_hits_batch(reqs, fuse_fast=j.get("fuse", True), errors="return")
        d["results"] = plain(res)
        if j.get("profile"):
            after = minehip.profile_read(0)
            d["profile"] = {{k: after[k] - before[k] for k in after}}
            d["kernels"] = [[k["word"], k["mode"], k["lo_digits"], k["nonces"], k["launches"]]
                            for k in minehip.profile_kernels(0)]
            minehip.profile_enable(0, False)
        if j.get("singles"):      # search_hits of every request alone, under the same environment
            singles = plain([minehip.search_hits(*r) for r in ok])
            mine = [g for r, g in zip(reqs, d["results"]) if r in ok]
            d["singles_differ"] = [[i, s[0], s[2]] for i, (s, g) in enumerate(zip(singles, mine)) if s != g]
        if j.get("unfused"):
            d["unfused"] = plain(minehip.search_hits_batch(reqs, errors="return"))
    finally:
        for k in kv:
            del os.environ[k]
    out.append(d)
print(json.dumps(out))
"""


def run_jobs(tmp_path, jobs, timeout=240):
    path = str(tmp_path / "jobs.json")
    with open(path, "w") as f:
        json.dump(dict(jobs=jobs), f)
    pre = f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]\n"
    r = subprocess.run([sys.executable, "-c", pre + CHILD.format(path=path)], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def job(reqs, env=None, **kw):
    return dict(reqs=[(m.hex(), lo, hi, T, c) for m, lo, hi, T, c in reqs], env=env or {}, **kw)


def ref(r):
    count, entries, mn = hits_ref(*r)
    return [count, [list(e) for e in entries], list(mn)]


def check(reqs, d, env=None):
    """One job's results against the reference; the child found search_hits of every request equal."""
    assert len(d["results"]) == len(reqs)
    for i, (r, g) in enumerate(zip(reqs, d["results"])):
        exp = ref(r)
        assert g[0] == exp[0] and g[2] == exp[2], (env, i, r[0][:8], r[1:], g[0], g[2], exp[0], exp[2])
        assert len(g[1]) == min(exp[0], r[4]) and g[1] == exp[1], (env, i, r[0][:8], r[1:], g[1][:3], exp[1][:3])
    if "singles_differ" in d:
        assert d["singles_differ"] == [], (env, d["singles_differ"])


def fast_pieces(plan, req=None):
    return [p for p in plan if p["kind"] == 2 and (req is None or p["req"] == req)]


def check_shapes_plan(plan):
    """The default plan of SHAPES + EXTRA (twice: two targets): every shape fused with a kind-2
    piece, the generic-only extras without one, nothing falls back."""
    n = len(SHAPES) + len(EXTRA)
    for base in (0, n):
        assert {p["req"] - base for p in fast_pieces(plan) if base <= p["req"] < base + n} == \
            set(range(len(SHAPES))) | {n - 1}
    assert not [p for p in plan if p["kind"] == 1] and {p["pass"] for p in plan} == {0}
    (one,) = fast_pieces(plan, 0)
    assert (one["first"], one["count"], one["slots"], one["word"], one["mode"], one["lo_digits"]) == \
        (1_048_000, 1_152_000, 450, 3, 0, 1)
    (edge,) = fast_pieces(plan, 1)
    assert (edge["first"], edge["count"], edge["slots"]) == (1_000_000, 2_000_000, 782)
    assert 200_000 - 781 * 256 == 64                                  # the last chunk's valid lanes
    assert [(p["kind"], p["first"], p["count"]) for p in plan if p["req"] == 1 and p["kind"] == 0] == \
        [(0, 0, 1_000_000), (0, 3_000_000, 1)]
    assert {(p["word"], p["mode"]) for p in fast_pieces(plan)} == {(13, 5), (0, 1), (13, 0), (3, 0), (6, 0)}


def test_all_shapes_in_one_call(gpu, tmp_path):
    """SHAPES + EXTRA at 2^64 // 10^6 and 2^64 // 10^3, cap 4096: count, stored, minimum and the
    full list, under the default plan, L = 3, L = 2, without the Early layouts and with a slot
    capacity that gives several passes and fallbacks."""
    reqs = [r + (T, 4096) for T in (T6, T3) for r in SHAPES + EXTRA]
    counts = [hits_ref(*r)[0] for r in reqs]
    assert all(c <= 4096 for c in counts) and sum(c > 1000 for c in counts) >= 7   # every list is a full list
    envs = [{}, L3, L2, NO_EARLY, SLOTS]
    out = run_jobs(tmp_path, [job(reqs, env, singles=True) for env in envs], timeout=420)
    check_shapes_plan(out[0]["plan"])
    plans = [d["plan"] for d in out]
    assert {p["lo_digits"] for p in fast_pieces(plans[1])} == {3} and {p["lo_digits"] for p in fast_pieces(plans[2])} == {2}
    assert not [p for p in fast_pieces(plans[3]) if p["mode"] >= 3] and [p for p in fast_pieces(plans[0]) if p["mode"] >= 3]
    assert {p["kind"] for p in plans[4]} == {0, 1, 2} and max(p["pass"] for p in plans[4]) >= 1
    for env, d in zip(envs, out):
        check(reqs, d, env)


def dense_requests():
    reqs = [ONE + (0, 4096), ONE + (T6, 4096), ONE + (T3, 4096), ONE + (2 ** 64 // 64, 65_536),
            ONE + (2 ** 64 // 16, 0), ONE + (U64, 0), ONE + (T3, 4096),
            EDGE + (U64, 0), EDGE + (2 ** 64 // 64, 65_536), EDGE + (T3, 4096)]
    return reqs


def test_one_message_many_targets_one_launch(gpu, tmp_path):
    """One message, many targets, the same request twice: a cursor and a region per
    request, not per message.  At 2^64 - 1 every nonce is counted exactly once; at 2^64 // 64 about a
    quarter of the wave steps hold two or more hits."""
    reqs = dense_requests()
    exp = [hits_ref(*r) for r in reqs]
    assert exp[0][0] == 0 and exp[5][0] == 1_152_001 and exp[7][0] == 3_000_001
    assert all(e[0] <= r[4] for e, r in zip(exp, reqs) if r[4])        # every list wanted is a full list
    assert 15_000 < exp[3][0] < 21_000 and 60_000 < exp[4][0] < 84_000 and 40_000 < exp[8][0] < 54_000
    assert exp[2] == exp[6] and exp[2][0] > 1000
    out = run_jobs(tmp_path, [job(reqs, {}, singles=True), job(reqs, L3, singles=True)])
    plan = out[0]["plan"]
    for i in range(7):
        (p,) = fast_pieces(plan, i)
        assert (p["first"], p["count"], p["slots"], p["launch"], p["pass"]) == (1_048_000, 1_152_000, 450, 0, 0)
    assert {p["launch"] for p in fast_pieces(plan)} == {0} and not [p for p in plan if p["kind"] == 1]
    assert [p["slots"] for i in (7, 8, 9) for p in fast_pieces(plan, i)] == [782] * 3
    for env, d in zip(({}, L3), out):
        check(reqs, d, env)
        assert d["results"][5][0] == ONE[2] - ONE[1] + 1 and d["results"][7][0] == 3_000_001


def test_truncation_and_rebuild(gpu, tmp_path):
    """cap in {1, count - 1, count, count + 1} for one fused request: the entries are the cap
    smallest nonces (cap < count: rebuilt from a prefix of the range, which for cap = 1 is doubled
    until it holds a hit); the neighbours of the call are untouched."""
    count = hits_ref(*EDGE, T3, 0)[0]
    assert 2_500 < count < 3_500
    neighbours = [EXTRA[0] + (T3, 4096), ONE + (T6, 4096), SHAPES[2] + (T3, 4096)]
    cut = [EDGE + (T3, c) for c in (1, count - 1, count, count + 1)]
    reqs = [neighbours[0], cut[0], cut[1], neighbours[1], cut[2], cut[3], neighbours[2]]
    assert all(0 < hits_ref(*r)[0] <= 4096 for r in neighbours)
    out = run_jobs(tmp_path, [job(reqs, {}, singles=True, regions=True), job(neighbours, {}, plan=False)])
    d = out[0]
    assert all(fast_pieces(d["plan"], i) for i in (1, 2, 3, 4, 5, 6)) and not [p for p in d["plan"] if p["kind"] == 1]
    assert [g["slots"] for g in d["regions"]] == [4096, 1, count - 1, 4096, count, count + 1, 4096]
    check(reqs, d)
    full = ref(EDGE + (T3, 1 << 20))[1]
    assert len(full) == count
    assert [g[1] for g in d["results"][1:3]] == [full[:1], full[:count - 1]]
    assert d["results"][4][1] == full == d["results"][5][1]
    assert [d["results"][i] for i in (0, 3, 6)] == out[1]["results"]


def test_small_device_buffer(gpu, tmp_path):
    """MINEHIP_HITS_SLOTS small: several windows and drains, regions cut short by the window, and
    with MINEHIP_BATCH_SLOTS several passes and fallbacks: the results do not change."""
    reqs = [r + (T3, 4096) for r in SHAPES + EXTRA]
    counts = [hits_ref(*r)[0] for r in reqs]
    assert all(c <= 4096 for c in counts)
    envs = [dict(MINEHIP_HITS_SLOTS=5000), dict(MINEHIP_HITS_SLOTS=1500, **SLOTS)]
    out = run_jobs(tmp_path, [job(reqs, env, regions=True) for env in envs], timeout=420)
    for env, d in zip(envs, out):
        check(reqs, d, env)
        window = int(env["MINEHIP_HITS_SLOTS"])
        regs, plan = d["regions"], d["plan"]
        assert len(regs) == len(reqs)
        for i, g in enumerate(regs):                       # kind and pass follow the ex plan
            mine = [p for p in plan if p["req"] == i]
            assert g["kind"] == (1 if mine[0]["kind"] == 1 else 0) and {p["pass"] for p in mine} == {g["pass"]}
        fused = [g for g in regs if g["kind"] == 0]
        by_window = {}
        for g in fused:
            by_window.setdefault(g["window"], []).append(g)
        assert len(by_window) >= (2 if "MINEHIP_BATCH_SLOTS" in env else 1)   # a window ends between passes only
        for gs in by_window.values():                      # disjoint, in order, inside the buffer
            end = 0
            for g in gs:
                assert g["offset"] >= end and g["offset"] + g["slots"] <= window
                end = g["offset"] + g["slots"]
        # a region cut short by the window: fewer slots than the request has hits, yet the full list came back
        cut = [i for i, g in enumerate(regs) if g["kind"] == 0 and g["slots"] < counts[i]]
        assert cut and any(fast_pieces(plan, i) for i in cut)
    assert {g["kind"] for g in out[1]["regions"]} == {0, 1} and max(g["pass"] for g in out[1]["regions"]) >= 1


def test_request_errors_beside_fused_requests(gpu, tmp_path):
    """MH_ERANGE, MH_ETOOLONG and a cap above MH_HITS_MAX_CAP leave the other requests intact."""
    reqs = [ONE + (T3, 4096), (b"x", 5, 4, 7, 16), SHAPES[3] + (T3, 4096), (b"y" * ((1 << 20) + 1), 0, 10, 7, 16),
            EXTRA[0] + (T3, 4096), EDGE + (T6, (1 << 20) + 1), EDGE + (T6, 16)]
    ok = [0, 2, 4, 6]
    assert all(hits_ref(*reqs[i])[0] <= reqs[i][4] for i in ok)
    (d,) = run_jobs(tmp_path, [job(reqs, singles=True)])
    assert [d["results"][i] for i in (1, 3, 5)] == [["error", minehip.MH_ERANGE], ["error", minehip.MH_ETOOLONG],
                                                    ["error", minehip.MH_EINVAL]]
    assert [bool(fast_pieces(d["plan"], k)) for k in range(4)] == [True, True, False, True]   # the plan of the valid ones
    check([reqs[i] for i in ok], dict(results=[d["results"][i] for i in ok], singles_differ=d["singles_differ"]))


def test_profile_counts_the_fused_fast_pieces(gpu, tmp_path):
    """The fused fast pieces count in the fast class under their layout and L with the planned
    nonce counts; a generic-only call counts none."""
    reqs = [r + (T6, 64) for r in SHAPES + EXTRA]
    generic = [r + (T6, 64) for r in EXTRA[:3]]
    assert all(hits_ref(*r)[0] <= 64 for r in reqs)
    out = run_jobs(tmp_path, [job(reqs, profile=True), job(generic, profile=True)])
    d = out[0]
    check(reqs, d)
    fast = fast_pieces(d["plan"])
    launches = len({(p["pass"], p["launch"]) for p in fast})
    assert d["profile"]["fast_launches"] == launches == 5
    assert d["profile"]["fast_nonces"] == sum(p["count"] for p in fast) > 10 ** 7
    assert d["profile"]["generic_nonces"] == sum(p["count"] for p in d["plan"] if p["kind"] == 0)
    assert d["profile"]["fast_ns"] > 0 and d["profile"]["fast_ops"] > 0 and d["profile"]["fast_slots"] > 0
    per = {}
    for p in fast:
        k = (p["word"], p["mode"], p["lo_digits"])
        per[k] = per.get(k, 0) + p["count"]
    assert {(w, m, L): n for w, m, L, n, _ in d["kernels"] if n} == per
    g = out[1]
    check(generic, g)
    assert not fast_pieces(g["plan"]) and g["profile"]["fast_launches"] == 0 and g["profile"]["fast_nonces"] == 0


def test_flag_zero_is_search_hits_batch(gpu, tmp_path):
    """fuse_fast=False gives search_hits_batch's results for a mixed batch, and both the reference's."""
    reqs = [ONE + (T3, 4096), EXTRA[0] + (T3, 4096), (b"x", 5, 4, 7, 16), SHAPES[4] + (T6, 16), EXTRA[2] + (U64, 4096)]
    ok = [0, 1, 3, 4]
    assert all(hits_ref(*reqs[i])[0] <= reqs[i][4] for i in ok)
    out = run_jobs(tmp_path, [job(reqs, fuse=False, unfused=True, plan=False), job(reqs, plan=False)])
    assert out[0]["results"] == out[0]["unfused"] == out[1]["results"]
    check([reqs[i] for i in ok], dict(results=[out[0]["results"][i] for i in ok]))
