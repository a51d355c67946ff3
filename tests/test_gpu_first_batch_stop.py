"""GPU tests of mh_search_first_batch_stop: mh_search_first_batch_ex(MH_BATCH_FUSE_FAST) whose fast
launches are batch_stop<J, MODE>'s -- batch_first's tables, order and skip of an unbegun chunk around
stop_scan's chunk body, which publishes a hit when it finds it and leaves a running chunk that lies
wholly above its request's published hit.

Every expected value comes from the reference alone (test_first.first_ref / hits_of /
kth_smallest_hash), asserted before the GPU is looked at.  found, hash and nonce are compared with the
reference, with search_first_batch(fuse_fast=True) of the same list and with a loop of search_first;
where nothing qualifies, with search.  `scanned`, counted by the waves themselves, is held to its
bounds: the range's size when nothing qualifies, within [nonce - lower + 1, size] otherwise.  One
assertion rests on timing (test_the_stop_is_live_at_the_smallest_shape), the one
tests/test_gpu_first_stop.py makes for the single search at the same chunk geometry.

One child process per test (the job runner of tests/test_gpu_first_batch_fast.py, with both calls)."""
import json
import subprocess
import sys

import pytest

from conftest import PKG, ROOT
from test_abi import KERNELS, KERNEL_CASE_NONCES, kernel_cases
from test_first import first_ref, hits_of, kth_smallest_hash
from test_gpu_batch_fast import L2, L3, NO_EARLY, SHAPES, SLOTS
from test_gpu_first_batch_fast import (ORDER, T6, U64, check, fast_pieces, job, layout_requests, low_target,
                                       one_piece_requests)
from test_gpu_parity import env

pytestmark = pytest.mark.gpu

FAST = dict(MINEHIP_GENERIC_BELOW=0, MINEHIP_MIN_LANES=1)
CHUNK1 = 2560  # nonces of one workgroup's chunk at L = 1 (256 lanes x 10)

CHILD = """
import json, os, minehip
spec = json.load(open({path!r}))
out = []
for j in spec["jobs"]:
    kv = {{k: str(v) for k, v in j["env"].items()}}
    os.environ.update(kv)
    try:
        reqs = [(bytes.fromhex(m), lo, hi, T) for m, lo, hi, T in j["reqs"]]
        pack = lambda res: [list(r) if isinstance(r, tuple) else ["error", r.code] for r in res]
        if j.get("profile"):
            minehip.profile_enable(0, True)
            before = minehip.profile_read(0)
        d = dict(plan=minehip.batch_plan_ex([r[:3] for r in reqs]) if j.get("plan", True) else None)
        d["results"] = pack(minehip.search_first_batch(reqs, fuse_fast=True, stop_running=True, errors="return"))
        if j.get("profile"):
            after = minehip.profile_read(0)
            d["profile"] = {{k: after[k] - before[k] for k in after}}
            d["kernels"] = [[k["word"], k["mode"], k["lo_digits"], k["nonces"], k["launches"]]
                            for k in minehip.profile_kernels(0)]
            minehip.profile_enable(0, False)
        if j.get("twice"):
            d["again"] = pack(minehip.search_first_batch(reqs, fuse_fast=True, stop_running=True, errors="return"))
        if j.get("fused", True):
            d["fused"] = pack(minehip.search_first_batch(reqs, fuse_fast=True, errors="return"))
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


def check_all(reqs, d, what=None):
    """The stopping call's results against the reference, search_first and search (check), and the
    non-stopping fused call's against the same; both calls' scanned within the bounds."""
    check(reqs, d, what)
    if "fused" in d:
        check(reqs, dict(results=d["fused"]), what)
        assert [g[:3] for g in d["fused"]] == [g[:3] for g in d["results"]], what
    if "again" in d:
        check(reqs, dict(results=d["again"]), what)
        assert [g[:3] for g in d["again"]] == [g[:3] for g in d["results"]], what


def test_same_answers_under_every_plan(gpu, tmp_path):
    """Ten requests of one <3, One> piece of 450 chunks + 1 nonce, and the 17 requests of every layout
    class, under the default plan, L = 3, L = 2, a slot capacity that gives several passes and
    fallbacks, without the Early layouts and under the request-major order; each call twice in one
    process (the words are re-initialised per pass)."""
    envs = [{}, L3, L2, SLOTS, NO_EARLY, ORDER]
    answers = {}
    for name, reqs in (("one piece", one_piece_requests()), ("layouts", layout_requests())):
        assert len(reqs) == (10 if name == "one piece" else 17)
        out = run_jobs(tmp_path, [job(reqs, e, singles=True, twice=True) for e in envs], timeout=300)
        for e, d in zip(envs, out):
            check_all(reqs, d, (name, e))
            answers.setdefault(name, set()).add(json.dumps([g[:3] for g in d["results"]]))
            for r, g in zip(reqs, d["results"]):
                if not g[0]:
                    assert g[3] == r[2] - r[1] + 1
        plans = [d["plan"] for d in out]
        assert fast_pieces(plans[0]) and {p["lo_digits"] for p in fast_pieces(plans[1])} == {3}
        if name == "layouts":
            assert {p["kind"] for p in plans[3]} == {0, 1, 2} and max(p["pass"] for p in plans[3]) >= 1   # SLOTS
            assert {(p["word"], p["mode"]) for p in fast_pieces(plans[0])} == {(13, 5), (0, 1), (13, 0), (3, 0), (6, 0)}
            assert not [p for p in fast_pieces(plans[4]) if p["mode"] >= 3]
    assert all(len(v) == 1 for v in answers.values())      # identical throughout


def layout_jobs():
    """[(J, mode, Ld, early, msg, lo, hi, T5, T1 - 1)]: each of the 26 layouts over
    test_abi.kernel_cases()' range plus 3,456 nonces, at MINEHIP_LOWER_DIGITS in {1, 3}."""
    cases = kernel_cases()
    assert set(cases) == KERNELS and len(KERNELS) == 26
    out = []
    for (J, mode), (m, lo, _, early) in sorted(cases.items()):
        hi = lo + KERNEL_CASE_NONCES + 3_456
        T5, T1 = kth_smallest_hash(m, lo, hi, 5), kth_smallest_hash(m, lo, hi, 1)
        hits = hits_of(m, lo, hi, T5)
        assert len(hits) == 5 and hits[-1] - hits[0] > CHUNK1, (J, mode, hits)       # five hits over more than 2,560 nonces
        assert not hits_of(m, lo, hi, T1 - 1)
        for Ld in (1, 3):
            out.append((J, mode, Ld, early, m, lo, hi, T5, T1 - 1, hits))
    return out


def test_every_fast_layout(gpu, tmp_path):
    """One request per call (a single-request batch keeps mh_search's own plan): five hits spread
    over more than one chunk -- chunks above the first of them may be left -- and no hit at all."""
    cases = layout_jobs()
    jobs, interleaved = [], set()
    for J, mode, Ld, early, m, lo, hi, T5, T0, hits in cases:
        e = dict(FAST, MINEHIP_LOWER_DIGITS=Ld, MINEHIP_EARLY=early)
        with env(**e):
            if mode >= 3:   # an Early piece at innermost position p >= L: its lanes interleave
                t = (len(m) + 1) % 64
                for pc in gpu.plan(m, lo, hi):
                    if pc["kind"] != 0 or (pc["word"], pc["mode"]) != (J, mode):
                        continue
                    pl = t + pc["digits"] - 1
                    base = 64 if (pc["blocks"] == 2 and pl >= 64) else 0
                    p = pl - (base + 4 * J + 3)
                    if p >= pc["lo_digits"] and any(pc["first"] <= n < pc["first"] + pc["count"] for n in hits):
                        interleaved.add((J, mode))
        for T in (T5, T0):
            jobs.append(job([(m, lo, hi, T)], e, singles=True))
    out = run_jobs(tmp_path, jobs, timeout=300)
    planned = set()
    for k, (J, mode, Ld, early, m, lo, hi, T5, T0, hits) in enumerate(cases):
        for d, T in zip(out[2 * k:2 * k + 2], (T5, T0)):
            check_all([(m, lo, hi, T)], d, (J, mode, Ld))
            assert d["results"][0][0] == (T == T5)
            if any((p["word"], p["mode"]) == (J, mode) for p in fast_pieces(d["plan"])):
                planned.add((J, mode))
    assert planned == KERNELS, KERNELS - planned
    assert interleaved == {k for k in KERNELS if k[1] >= 3}, interleaved


LIVE = [  # message, hits of [1,000,000, 1,999,999] at target 2^64 // 10^6, (chunk, run, group) of the first
    (b"cmu440", [1_067_492, 1_456_236, 1_999_610], (0, 67, 49)),
    (b"cmu440-04", [1_251_090], (0, 251, 9)),
    (b"cmu440-30", [1_016_285], (0, 16, 28)),
    (b"cmu440-37", [1_208_230], (0, 208, 23)),
    (b"cmu440-41", [1_019_237, 1_314_079], (0, 19, 23)),
    (b"cmu440-43", [1_101_357, 1_155_873, 1_567_429], (0, 101, 35)),
    (b"cmu440-55", [1_026_146, 1_679_057], (0, 26, 14)),
    (b"cmu440-18", [1_354_051, 1_474_545], (1, 354, 5)),
    (b"cmu440-00", [], None),
    (b"cmu440-06", [], None),
]


def test_the_stop_is_live_at_the_smallest_shape(gpu, tmp_path):
    """Ten requests of one kind-2 piece each: four chunks of 256 runs x 1,000 nonces, 40 workgroups
    in the two launches of one pass, each launch's all resident at once.  Seven have their first hit in chunk 0, whose three other
    chunks lie wholly above it: without the stop those chunks have begun before the hit is known
    and run to their end; with it they are left once the hit is published, so fewer nonces than
    the range are hashed."""
    lo, hi = 1_000_000, 1_999_999
    reqs = [(m, lo, hi, T6) for m, _, _ in LIVE]
    for (m, hits, pos), r in zip(LIVE, reqs):
        assert hits_of(*r) == hits, m
        exp = first_ref(*r)
        assert exp[0] == bool(hits) and (not hits or exp[2] == hits[0])
        if hits:
            run = (hits[0] - lo) // 1000
            assert (run // 256, run, (hits[0] - lo) % 1000 // 10) == pos, m
            if pos[0] == 0:
                assert all(lo + c * 256_000 > hits[0] for c in (1, 2, 3)), m       # the floors of chunks 1..3
    e = dict(FAST, MINEHIP_LOWER_DIGITS=3, MINEHIP_EARLY=0)
    (d,) = run_jobs(tmp_path, [job(reqs, e, singles=True)])
    plan = d["plan"]
    assert len(plan) == len(reqs) == 10
    for i, p in enumerate(plan):
        assert (p["req"], p["kind"], p["first"], p["count"], p["lo_digits"], p["slots"]) == (i, 2, lo, 10 ** 6, 3, 4), p
        assert p["mode"] < 3 and p["pass"] == 0, p
    # one pass; one launch per layout: the nine "cmu440-NN" messages share <J, MODE> and one launch
    # of 36 workgroups, "cmu440" (three bytes shorter, another word J) is a launch of 4 -- either
    # way every chunk of a launch is resident at once
    assert len({p["launch"] for p in plan[1:]}) == 1 and len({(p["word"], p["mode"]) for p in plan[1:]}) == 1
    assert {p["launch"] for p in plan} == {0, 1} and plan[0]["word"] != plan[1]["word"]
    for (m, hits, pos), s, f in zip(LIVE, d["results"], d["fused"]):
        print("%-10s scanned: fuse_fast %d, stop_running %d" % (m.decode(), f[3], s[3]))
    check_all(reqs, d, e)
    for (m, hits, pos), r, g in zip(LIVE, reqs, d["results"]):
        if not hits:
            assert g[3] == 1_000_000 and not g[0] and tuple(g[1:3]) == tuple(d["mins"][reqs.index(r)]), (m, g)
        elif pos[0] == 0:
            assert hits[0] - lo + 1 <= g[3] < 1_000_000, (m, g)        # strictly below: chunks 1..3 were left
        else:
            assert 354_052 <= g[3] <= 1_000_000, (m, g)


def test_generic_head_and_fast_piece_share_the_word(gpu, tmp_path):
    """A hit in the generic head of a request wins over the hits of its fast piece, whose running
    chunks poll the word the head's tiles lower; a request whose first slot is a fast chunk; record
    lows in the generic head and along the fast piece."""
    a = (b"cmu440", 0, 3_000_000, T6)
    b = (b"cmu440", 1_048_000, 2_200_000, T6)
    assert first_ref(*a)[2] == 393_322 and 1_067_492 in hits_of(*a)
    assert first_ref(*b) == (True, 1228377698034, 1_067_492)
    c = (b"cmu441", 0, 3_000_000)
    reqs = [a, b] + [low_target(c, n) for n in (631_451, 1_340_627, 1_591_415, 2_151_989)]
    out = run_jobs(tmp_path, [job(reqs, {}, singles=True), job(reqs, L3, singles=True)])
    plan = out[0]["plan"]
    assert [p["kind"] for p in plan if p["req"] == 0] == [0, 2, 0] and [p["kind"] for p in plan if p["req"] == 1] == [2, 0]
    for e, d in zip(({}, L3), out):
        check_all(reqs, d, e)
        assert [g[2] for g in d["results"]] == [393_322, 1_067_492, 631_451, 1_340_627, 1_591_415, 2_151_989]


def test_last_partial_chunk(gpu, tmp_path):
    """The minimum of ("cmu474", 0, 3 * 10^6) lies in the last chunk of the L = 3 plan, the one with
    208 valid lanes, at lane 3; and target 0 over the same range: the waves' count over the invalid
    lanes of that chunk gives exactly the range."""
    req = (b"cmu474", 0, 3_000_000)
    reqs = [low_target(req, 2_795_132, 393812568028), low_target(req, 2_341_601, 16628061397712),
            low_target(req, 2_569_652, 14186423739864), req + (0,)]
    assert kth_smallest_hash(*req, 1) == 393812568028 and not first_ref(*reqs[3])[0]
    out = run_jobs(tmp_path, [job(reqs, L3, singles=True), job(reqs, {}, singles=True)])
    (p3,) = fast_pieces(out[0]["plan"], 0)
    assert (p3["first"], p3["count"], p3["lo_digits"], p3["slots"]) == (1_000_000, 2_000_000, 3, 8)
    run = (2_795_132 - p3["first"]) // 1000
    assert (run // 256, run % 256, 2000 - 7 * 256) == (7, 3, 208)
    for e, d in zip((L3, {}), out):
        check_all(reqs, d, e)
        assert [g[2] for g in d["results"][:3]] == [2_795_132, 2_341_601, 2_569_652]
        assert d["results"][3][0] is False and d["results"][3][3] == 3_000_001


def test_errors_fallbacks_and_profile(gpu, tmp_path):
    """MH_ERANGE and MH_ETOOLONG leave the other requests intact; under a small slot capacity the
    plan has fallbacks, which run through the stopping single search; with the profile on, the fast
    launches are the plan's launches and the fast nonces the planned piece counts."""
    lows = one_piece_requests()
    mixed = [lows[4], (b"x", 5, 4, 7), low_target(SHAPES[3], 1_327_121), (b"y" * ((1 << 20) + 1), 0, 10, 7),
             (b"cmu440", 0, 199_999, kth_smallest_hash(b"cmu440", 0, 199_999, 2)), (b"z", U64, 0, 7), lows[7]]
    ok = [0, 2, 4, 6]
    reqs = layout_requests()
    out = run_jobs(tmp_path, [job(mixed, plan=False), job(reqs, SLOTS, singles=True), job(reqs, profile=True, fused=False)],
                   timeout=240)
    d = out[0]
    for res in (d["results"], d["fused"]):
        assert [res[i] for i in (1, 3, 5)] == [["error", -2], ["error", -3], ["error", -2]]
        check([mixed[i] for i in ok], dict(results=[res[i] for i in ok]))
    d = out[1]
    fallbacks = [p["req"] for p in d["plan"] if p["kind"] == 1]
    assert fallbacks and max(p["pass"] for p in d["plan"]) >= 1
    check_all(reqs, d, SLOTS)
    d = out[2]
    check(reqs, d)
    fast = fast_pieces(d["plan"])
    launches = len({(p["pass"], p["launch"]) for p in fast})
    assert d["profile"]["fast_launches"] == launches == 5
    assert d["profile"]["fast_nonces"] == sum(p["count"] for p in fast) > 10 ** 7
    assert d["profile"]["generic_nonces"] == sum(p["count"] for p in d["plan"] if p["kind"] == 0)
    per = {}
    for p in fast:
        k = (p["word"], p["mode"], p["lo_digits"])
        per[k] = per.get(k, 0) + p["count"]
    assert {(w, m, L): n for w, m, L, n, _ in d["kernels"] if n} == per
