"""GPU tests of the batched first-hit search with fused fast pieces:
mh_search_first_batch_ex(MH_BATCH_FUSE_FAST), the batch_first<J, MODE> kernels of the fifth embedded
code object, batch_scan_first_slots and merge_segments_first_ex.

Every expected value comes from the reference alone (test_first.first_ref / hits_of /
kth_smallest_hash: the oracle's hashes of the whole range, in numpy).  Every request is also
compared with search_first of the same request under the same environment and, where nothing
qualifies, with search.  `scanned` is held to its bounds only, and no test asserts a skip.

The first-hit path has no hash hooks, so a test places the answer with a record low: a nonce whose
hash is below every earlier hash of the range.  With target = Hash(n) of a record low n the answer
is exactly n, and every later record low qualifies too, so "the first hit wins, not the smallest
hash" is exercised for free.  Every test re-asserts its record lows from first_ref, and the piece,
chunk and lane positions from batch_plan_ex, before it touches the GPU.  One child process per test.
"""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_first import first_ref, hits_of, kth_smallest_hash
from test_gpu_batch_fast import EXTRA, L2, L3, NO_EARLY, SHAPES, SLOTS
from test_gpu_ties import full_hashes

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
T6 = 2 ** 64 // 10 ** 6
ORDER = dict(MINEHIP_FIRST_BATCH_ORDER="request")

ONE_PIECE = (b"cmu441", 1_048_000, 2_200_000)     # one <3, One> piece of 450 chunks exactly + 1 nonce
ONE_PIECE_LOWS = [(1_049_781, None), (1_051_953, None), (1_074_728, None), (1_102_958, None),
                  (1_340_627, 6426288448911), (1_591_415, 3200136698158), (2_151_989, 158342842482)]


@functools.lru_cache(maxsize=None)
def record_lows(msg, lo, hi):
    """{nonce: hash} of every nonce of the range whose hash is below every earlier one's."""
    h = full_hashes(msg, lo, hi)
    before = np.minimum.accumulate(h)
    idx = np.flatnonzero(np.concatenate(([True], h[1:] < before[:-1])))
    return {lo + int(i): int(h[i]) for i in idx}


def low_target(req, n, want_hash=None):
    """The request with target Hash(n) of its record low n: the reference answers exactly n."""
    msg, lo, hi = req
    lows = record_lows(msg, lo, hi)
    assert n in lows and (want_hash is None or lows[n] == want_hash), (msg[:8], n)
    assert first_ref(msg, lo, hi, lows[n]) == (True, lows[n], n)
    return (msg, lo, hi, lows[n])


CHILD = """
import json, os, minehip
spec = json.load(open({path!r}))
out = []
for j in spec["jobs"]:
    kv = {{k: str(v) for k, v in j["env"].items()}}
    os.environ.update(kv)
    try:
        reqs = [(bytes.fromhex(m), lo, hi, T) for m, lo, hi, T in j["reqs"]]
        if j.get("profile"):
            minehip.profile_enable(0, True)
            before = minehip.profile_read(0)
        d = dict(plan=minehip.batch_plan_ex([r[:3] for r in reqs]) if j.get("plan", True) else None)
        res = minehip.search_first_batch(reqs, fuse_fast=j.get("fuse", True), errors="return")
        d["results"] = [list(r) if isinstance(r, tuple) else ["error", r.code] for r in res]
        if j.get("profile"):
            after = minehip.profile_read(0)
            d["profile"] = {{k: after[k] - before[k] for k in after}}
            d["kernels"] = [[k["word"], k["mode"], k["lo_digits"], k["nonces"], k["launches"]]
                            for k in minehip.profile_kernels(0)]
            minehip.profile_enable(0, False)
        if j.get("singles"):
            d["singles"] = [list(minehip.search_first(*r)) for r in reqs]
            d["mins"] = [list(minehip.search(*r[:3])) if not s[0] else None for r, s in zip(reqs, d["singles"])]
    finally:
        for k in kv:
            del os.environ[k]
    out.append(d)
print(json.dumps(out))
"""


def run_jobs(tmp_path, jobs, timeout=120):
    path = str(tmp_path / "jobs.json")
    with open(path, "w") as f:
        json.dump(dict(jobs=jobs), f)
    pre = f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]\n"
    r = subprocess.run([sys.executable, "-c", pre + CHILD.format(path=path)], capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def job(reqs, env=None, **kw):
    return dict(reqs=[(m.hex(), lo, hi, T) for m, lo, hi, T in reqs], env=env or {}, **kw)


def check_scanned(r, g):
    msg, lo, hi, T = r
    if g[0]:
        assert g[2] - lo + 1 <= g[3] <= hi - lo + 1, (msg[:8], lo, hi, T, g)
    else:
        assert g[3] == hi - lo + 1, (msg[:8], lo, hi, T, g)


def check(reqs, d, env=None):
    """One job's results against the reference, against search_first of every request and, where
    nothing qualifies, against search; scanned within its bounds."""
    assert len(d["results"]) == len(reqs)
    for i, (r, g) in enumerate(zip(reqs, d["results"])):
        msg, lo, hi, T = r
        exp = first_ref(msg, lo, hi, T)
        assert tuple(g[:3]) == exp, (env, i, msg[:8], len(msg), lo, hi, T, g)
        check_scanned(r, g)
        if "singles" in d:
            assert tuple(d["singles"][i][:3]) == exp, (env, i, d["singles"][i])
            if not exp[0]:
                assert tuple(d["mins"][i]) == exp[1:], (env, i, d["mins"][i])


def fast_pieces(plan, req=None):
    return [p for p in plan if p["kind"] == 2 and (req is None or p["req"] == req)]


def one_piece_requests():
    msg, lo, hi = ONE_PIECE
    reqs = [low_target(ONE_PIECE, n, h) for n, h in ONE_PIECE_LOWS]
    mn = kth_smallest_hash(msg, lo, hi, 1)
    assert mn == 158342842482 and not hits_of(msg, lo, hi, mn - 1)
    assert first_ref(msg, lo, hi, U64)[2] == lo and not first_ref(msg, lo, hi, 0)[0]
    # the later record lows qualify too: the first hit wins, not the smallest hash
    assert [len(hits_of(*r)) for r in reqs][-1] == 1 and all(len(hits_of(*r)) >= 2 for r in reqs[:-1])
    return reqs + [(msg, lo, hi, mn - 1), (msg, lo, hi, U64), (msg, lo, hi, 0)]


def check_one_piece_plans(plan, plan3, reqs):
    for i in range(len(reqs)):   # default plan: one <3, One> piece of 450 chunks exactly, then 1 nonce
        (p,) = fast_pieces(plan, i)
        assert (p["first"], p["count"], p["slots"], p["word"], p["mode"], p["lo_digits"]) == \
            (1_048_000, 1_152_000, 450, 3, 0, 1)
        assert [(q["kind"], q["first"], q["count"]) for q in plan if q["req"] == i and q["kind"] != 2] == \
            [(0, 2_200_000, 1)]
    assert {p["launch"] for p in fast_pieces(plan)} == {0} and {p["pass"] for p in plan} == {0}
    assert [(n - 1_048_000) // 2560 for n, _ in ONE_PIECE_LOWS][:2] == [0, 1]
    assert (2_151_989 - 1_048_000) // 2560 == 431
    assert {p["lo_digits"] for p in fast_pieces(plan3)} == {3} and len(fast_pieces(plan3)) == len(reqs)
    assert not [p for p in plan3 if p["kind"] == 1]


def test_record_lows_along_one_fast_piece(gpu, tmp_path):
    """Ten requests of one message and one range in one launch, one per record low of the piece and
    three more (nothing qualifies below the minimum, everything at 2^64 - 1, nothing at 0): the
    device words are per request, not per message.  Default plan and L = 3."""
    reqs = one_piece_requests()
    out = run_jobs(tmp_path, [job(reqs, {}, singles=True), job(reqs, L3, singles=True)])
    check_one_piece_plans(out[0]["plan"], out[1]["plan"], reqs)
    for env, d in zip(({}, L3), out):
        check(reqs, d, env)
    for d in out:
        assert [g[2] for g in d["results"][:7]] == [n for n, _ in ONE_PIECE_LOWS]
        assert not d["results"][7][0] and d["results"][7][3] == 1_152_001
        assert d["results"][8][:3] == [True, first_ref(*reqs[8])[1], 1_048_000] and not d["results"][9][0]


def test_order_independence(gpu, tmp_path):
    """The same call under the request-major order: found, hash and nonce are the same."""
    reqs = one_piece_requests()
    out = run_jobs(tmp_path, [job(reqs, {}, plan=False), job(reqs, ORDER, plan=False), job(reqs, dict(L3, **ORDER), plan=False)])
    for d in out:
        check(reqs, d)
    assert [g[:3] for g in out[0]["results"]] == [g[:3] for g in out[1]["results"]] == [g[:3] for g in out[2]["results"]]


def test_last_partial_chunk(gpu, tmp_path):
    """The minimum of ("cmu474", 0, 3 * 10^6) lies in the last chunk of the L = 3 plan, the one with
    208 valid lanes, at lane 3; under the default plan in chunk 701 of 782."""
    req = (b"cmu474", 0, 3_000_000)
    reqs = [low_target(req, 2_795_132, 393812568028), low_target(req, 2_341_601, 16628061397712),
            low_target(req, 2_569_652, 14186423739864)]
    assert kth_smallest_hash(*req, 1) == 393812568028
    out = run_jobs(tmp_path, [job(reqs, L3, singles=True), job(reqs, {}, singles=True)])
    (p3,) = fast_pieces(out[0]["plan"], 0)
    assert (p3["first"], p3["count"], p3["lo_digits"], p3["slots"]) == (1_000_000, 2_000_000, 3, 8)
    run = (2_795_132 - p3["first"]) // 1000
    assert (run // 256, run % 256, 2000 - 7 * 256) == (7, 3, 208)
    (p1,) = fast_pieces(out[1]["plan"], 0)
    assert (p1["first"], p1["lo_digits"], p1["slots"]) == (1_000_000, 1, 782)
    assert (2_795_132 - p1["first"]) // 2560 == 701
    for env, d in zip((L3, {}), out):
        check(reqs, d, env)
        assert [g[2] for g in d["results"]] == [2_795_132, 2_341_601, 2_569_652]


def test_generic_head_beats_the_fast_piece(gpu, tmp_path):
    """A hit in the generic head of a request wins over the hits of its fast piece; a request whose
    first slot is a fast chunk; record lows in the generic head and along the fast piece."""
    a = (b"cmu440", 0, 3_000_000, T6)
    b = (b"cmu440", 1_048_000, 2_200_000, T6)
    assert first_ref(*a)[2] == 393_322 and 1_067_492 in hits_of(*a)
    assert first_ref(*b) == (True, 1228377698034, 1_067_492)
    c = (b"cmu441", 0, 3_000_000)
    reqs = [a, b] + [low_target(c, n) for n in (631_451, 1_340_627, 1_591_415, 2_151_989)]
    out = run_jobs(tmp_path, [job(reqs, {}, singles=True), job(reqs, L3, singles=True)])
    plan = out[0]["plan"]
    assert [p["kind"] for p in plan if p["req"] == 0] == [0, 2, 0] and [p["kind"] for p in plan if p["req"] == 1] == [2, 0]
    (pc,) = fast_pieces(plan, 5)
    assert pc["first"] == 1_000_000 and 631_451 < pc["first"] and pc["lo_digits"] == 1
    assert ((2_151_989 - pc["first"]) // 2560, (2_151_989 - pc["first"]) // 10 % 256) == (449, 254)
    for env, d in zip(({}, L3), out):
        check(reqs, d, env)
        assert [g[2] for g in d["results"]] == [393_322, 1_067_492, 631_451, 1_340_627, 1_591_415, 2_151_989]


def layout_requests():
    reqs = [low_target(SHAPES[2], 1_533_239), low_target(SHAPES[3], 1_327_121)]
    reqs += [low_target(SHAPES[4], n) for n in (1_024_049, 1_197_199, 1_457_050, 1_637_233)]
    for shape in (SHAPES[5], SHAPES[6]):
        assert shape[2] == U64 or shape[1] == 5 * 10 ** 8
        ks = [kth_smallest_hash(*shape, k) for k in (1, 2, 5)]
        assert [len(hits_of(*shape, T)) for T in ks] == [1, 2, 5] and not hits_of(*shape, ks[0] - 1)
        reqs += [shape + (T,) for T in ks + [ks[0] - 1]]
    for msg, lo, hi in EXTRA[:3]:          # generic-only requests beside them
        reqs.append((msg, lo, hi, kth_smallest_hash(msg, lo, hi, min(2, hi - lo + 1))))
    return reqs


def test_every_layout_class_in_one_call(gpu, tmp_path):
    """<13, TwoEarly> (the candidate nonce goes through spread), <0, Pre>, <13, One>, 9 digits and 20
    digits ending at 2^64 - 1, with generic-only requests, under the default plan, L = 3, L = 2, a
    slot capacity that gives several passes and fallbacks, and without the Early layouts."""
    reqs = layout_requests()
    assert len(reqs) == 17
    envs = [{}, L3, L2, SLOTS, NO_EARLY]
    out = run_jobs(tmp_path, [job(reqs, env, singles=True) for env in envs], timeout=240)
    for env, d in zip(envs, out):
        check(reqs, d, env)
    plans = [d["plan"] for d in out]
    fast = [fast_pieces(plan) for plan in plans]
    # the plans are the ones the cases are about
    assert {p["req"] for p in fast[0]} == set(range(14)) and not [p for p in plans[0] if p["kind"] == 1]
    assert {(p["word"], p["mode"]) for p in fast[0]} == {(13, 5), (0, 1), (13, 0), (3, 0), (6, 0)}
    assert {(p["word"], p["mode"]) for p in fast[0] if p["req"] == 0} == {(13, 5)}
    assert {(p["word"], p["mode"]) for p in fast[0] if p["req"] == 1} == {(0, 1)}
    assert {(p["word"], p["mode"]) for p in fast[0] if p["req"] in (2, 3, 4, 5)} == {(13, 0)}
    assert {(p["word"], p["mode"]) for p in fast[0] if p["req"] >= 10} == {(6, 0)}
    assert {p["lo_digits"] for p in fast[0]} == {1} and max(p["pass"] for p in plans[0]) == 0
    assert {p["lo_digits"] for p in fast[1]} == {3} and {p["lo_digits"] for p in fast[2]} == {2}
    assert {p["kind"] for p in plans[3]} == {0, 1, 2} and max(p["pass"] for p in plans[3]) >= 1
    assert not [p for p in fast[4] if p["mode"] >= 3] and [p for p in fast[0] if p["mode"] >= 3]
    # the record lows lie inside the fast pieces
    for i, r in enumerate(reqs[:6]):
        n = first_ref(*r)[2]
        assert any(p["first"] <= n < p["first"] + p["count"] for p in fast_pieces(plans[0], i)), (i, n)


def test_request_errors_and_flag_zero(gpu, tmp_path):
    """MH_ERANGE and MH_ETOOLONG leave the other requests intact; fuse_fast=False gives exactly
    search_first_batch's results for a mixed list."""
    lows = one_piece_requests()
    reqs = [lows[4], (b"x", 5, 4, 7), low_target(SHAPES[3], 1_327_121), (b"y" * ((1 << 20) + 1), 0, 10, 7),
            (b"cmu440", 0, 199_999, kth_smallest_hash(b"cmu440", 0, 199_999, 2)), (b"z", U64, 0, 7), lows[7]]
    ok = [0, 2, 4, 6]
    out = run_jobs(tmp_path, [job(reqs, plan=False), job(reqs, plan=False, fuse=False)])
    for d in out:
        assert [d["results"][i] for i in (1, 3, 5)] == [["error", -2], ["error", -3], ["error", -2]]
        check([reqs[i] for i in ok], dict(results=[d["results"][i] for i in ok]))
    assert [out[0]["results"][i][:3] for i in ok] == [out[1]["results"][i][:3] for i in ok]


def test_profile_counts_the_fused_fast_pieces(gpu, tmp_path):
    """A call with fused fast pieces counts fast launches equal to the plan's launches, each piece's
    planned nonces under its (J, MODE, L); a generic-only call counts none."""
    reqs = layout_requests()
    generic = [r for r in reqs[14:]] + [(b"cmu440", 0, 199_999, T6)]
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
    assert g["profile"]["generic_nonces"] == sum(hi - lo + 1 for _, lo, hi, _ in generic)
