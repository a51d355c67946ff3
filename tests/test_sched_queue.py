"""CPU tests of the scheduler's per-miner chunk queue (mh_sched_create_ex / mh_server_create_ex,
include/minehip_server.h "Queueing"): a miner may hold up to `depth` chunks while the nonces it
holds stay under its budget, Results complete its chunks oldest first, and with depth > 1 every
Result is checked against the host Hash so a miner that skips an answer is removed instead of
having its later Results credited to the wrong chunks.

Depth 1 must be the scheduler as it was: tests/golden/sched_depth1_trace.json holds an event list
and what mh_sched_create answered to it before the queue existed (every assignment, completion,
error code and the final stats; the chunk sizes follow the measured rates, so those are pinned
too), and both constructors must reproduce it.

Miners are simulated with the CPU oracle (test infrastructure) on small ranges, as in
test_sched.py; the GPU form is tests/test_gpu_queue.py."""
import json
import random

import pytest

import minehip
from minehip import Scheduler, Server, MinehipError
from conftest import load_golden
from oracle import oracle
from test_sched import covered

U64 = (1 << 64) - 1
SMALL = dict(init_chunk=10 ** 6, min_chunk=1, max_chunk=10 ** 9, target_ns=10 ** 6)
# with several miners a job's chunk is capped at a share of it: min_chunk above the job sizes keeps
# small jobs whole, as the product's 2^24 does
WHOLE = dict(SMALL, min_chunk=10 ** 5)


def answer(msg, lo, hi):
    return oracle.search(msg, lo, hi, threads=1)


# ---- depth 1 is the scheduler as it was ------------------------------------------------------

def fake_hash(nonce):
    return ((nonce * 0x9E3779B97F4A7C15) & U64) >> 16


def run_trace(s, events):
    """Feed `events` to a scheduler and return everything it answered, as JSON values.  A result
    event answers the chunk the miner holds with its lower bound (or, flagged bad, with a nonce
    past its upper bound) and a made-up hash: depth 1 checks no hash."""
    held, out = {}, []
    for ev in events:
        op = ev[0]
        try:
            r = None
            if op == "add":
                s.add_miner(ev[1])
            elif op == "remove":
                held.pop(ev[1], None)
                s.remove_miner(ev[1])
            elif op == "submit":
                r = s.submit(ev[1], ev[2].encode(), ev[3], ev[4])
            elif op == "drop":
                r = s.drop_client(ev[1])
            elif op == "next":
                r = s.next(ev[1], now=ev[2])
                if r is not None:
                    held.setdefault(r[0], []).append(r)
            elif op == "result":
                q = held.get(ev[1]) or []
                nonce = 0
                if q:
                    a = q.pop(0)
                    nonce = a[3] + 1 if ev[3] and a[3] < U64 else a[2]
                r = s.result(ev[1], fake_hash(nonce), nonce, now=ev[2])
            else:
                raise AssertionError(op)
        except MinehipError as e:
            r = ["err", e.code]
        out.append(r)
    out.append(s.stats())
    return json.loads(json.dumps(out))


@pytest.mark.parametrize("how", ["create", "create_ex"])
def test_depth_1_reproduces_the_recorded_trace(how):
    g = load_golden("sched_depth1_trace.json")
    s = Scheduler(**g["opts"]) if how == "create" else Scheduler(depth=1, queue_ns=0, **g["opts"])
    got = run_trace(s, g["events"])
    assert len(got) == len(g["answers"])
    for k, (a, b) in enumerate(zip(got, g["answers"])):
        assert a == b, (k, g["events"][k] if k < len(g["events"]) else "stats", a, b)
    # the trace is not trivial: chunks of many sizes (rates moved), losses, rejects, cancels
    st = g["answers"][-1]
    assert st["chunks_requeued"] > 5 and st["jobs_cancelled"] > 0 and st["jobs_done"] > 5
    sizes = {a[3] - a[2] for ev, a in zip(g["events"], g["answers"]) if ev[0] == "next" and a and a[0] != "err"}
    assert len(sizes) > 20


# ---- the queue rule -------------------------------------------------------------------------

def test_first_drain_hands_out_depth_chunks_oldest_first():
    s = Scheduler(depth=16, **SMALL)
    s.add_miner(7)
    jobs = [s.submit(100 + k, b"m%d" % k, 0, 9_999) for k in range(40)]
    got = []
    while (a := s.next(now=0)) is not None:
        got.append(a)
    assert len(got) == 16
    assert [a[1:] for a in got] == [(j, 0, 9_999) for j in jobs[:16]]
    assert s.queue(7) == [(j, 0, 9_999) for j in jobs[:16]]
    assert s.next(7, now=0) is None                       # a specific miner that may take no more
    st = s.stats()
    assert st["idle_miners"] == 0 and st["chunks_assigned"] == 16
    # Results complete the chunks in FIFO order, and each frees one place
    for k in range(40):
        msg = b"m%d" % k
        h, n = answer(msg, 0, 9_999)
        assert s.queue(7)[0][0] == jobs[k]
        assert s.result(7, h, n, now=1 + k) == (jobs[k], 100 + k, h, n)
        a = s.next(now=1 + k)
        assert (a is None) == (k + 16 >= 40) and (a is None or a[1] == jobs[k + 16])
    assert s.queue(7) == [] and s.stats()["idle_miners"] == 1 and s.stats()["jobs"] == 0
    with pytest.raises(MinehipError):
        s.queue(8)


def test_two_miners_alternate_fewest_out_first():
    s = Scheduler(depth=4, **WHOLE)
    s.add_miner(1)
    s.add_miner(2)
    for k in range(20):
        s.submit(k, b"x", 0, 999)
    order = []
    while (a := s.next(now=0)) is not None:
        order.append(a[0])
    assert order == [1, 2, 1, 2, 1, 2, 1, 2]
    h, n = answer(b"x", 0, 999)
    s.result(2, h, n, now=5)
    s.result(2, h, n, now=6)
    assert [s.next(now=6)[0] for _ in range(2)] == [2, 2] and s.next(now=6) is None


@pytest.mark.parametrize("depth", [1, 2, 16, 64])
def test_large_job_leaves_one_chunk_per_miner(depth):
    """The budget rule: a large job's chunk is rate x target_ns (init_chunk before a rate), which is
    the whole budget, so at any depth large jobs are scheduled as at depth 1."""
    s = Scheduler(depth=depth)                            # the product's sizing options
    for m in (1, 2, 3):
        s.add_miner(m)
    s.submit(0, b"cmu440", 0, (1 << 36) - 1)
    got = []
    while (a := s.next(now=0)) is not None:
        got.append(a)
    assert [a[0] for a in got] == [1, 2, 3] and all(a[3] - a[2] + 1 == 1 << 30 for a in got)
    assert [len(s.queue(m)) for m in (1, 2, 3)] == [1, 1, 1]
    # and with a measured rate: the next chunk is rate x target_ns, again the whole budget
    n = got[0][2]
    s2 = Scheduler(depth=depth)
    s2.add_miner(1)
    s2.submit(0, b"cmu440", 0, (1 << 40) - 1)
    a = s2.next(now=0)
    s2.result(1, oracle.hash_(b"cmu440", n), n, now=25_000_000)   # 2^30 in 25 ms
    a = s2.next(now=25_000_000)
    assert a[3] - a[2] + 1 == int((1 << 30) / 25e6 * 250e6)
    assert s2.next(now=25_000_000) is None and len(s2.queue(1)) == 1


def test_a_large_jobs_last_chunks_may_stack():
    """The exception to the above, stated in minehip_server.h: the fair-share cap (pending / (2 x
    miners)) cuts a job's last chunks smaller than the budget, and those do queue behind each other,
    the miner with the fewest chunks out first."""
    s = Scheduler(depth=64, init_chunk=1_000, min_chunk=10, max_chunk=1_000)
    s.add_miner(1)
    s.add_miner(2)
    s.submit(0, b"tail", 0, 3_999)
    got = []
    while (a := s.next(now=0)) is not None:
        got.append((a[0], a[3] - a[2] + 1))
    # 1,000 (= the budget: miner 1 is full), then 3,000 / 4 and 2,250 / 4 on miner 2 (1,312 >= 1,000)
    assert got == [(1, 1_000), (2, 750), (2, 562)] and [len(s.queue(m)) for m in (1, 2)] == [1, 2]


def test_budget_stops_small_jobs_before_depth():
    s = Scheduler(depth=16, init_chunk=35_000, min_chunk=1, max_chunk=10 ** 9, target_ns=10 ** 6)
    s.add_miner(1)
    for k in range(10):
        s.submit(k, b"b", 0, 9_999)
    n = 0
    while s.next(now=0) is not None:
        n += 1
    assert n == 4                                         # held 0, 10k, 20k, 30k < 35k; 40k is not
    # queue_ns scales the budget once a rate is known: 1 nonce/ns x 25,000 ns
    s = Scheduler(depth=16, queue_ns=25_000, **SMALL)
    s.add_miner(1)
    for k in range(10):
        s.submit(k, b"b", 0, 9_999)
    assert s.next(now=0) is not None
    s.result(1, oracle.hash_(b"b", 0), 0, now=10_000)
    n = 0
    while s.next(now=10_000) is not None:
        n += 1
    assert n == 3                                         # held 0, 10k, 20k < 25k; 30k is not


# ---- rate sampling ---------------------------------------------------------------------------

def next_chunk_size(s, miner, now):
    """The size of the chunk a big job gives `miner`: rate x target_ns."""
    s.submit(999, b"big", 0, 10 ** 12)
    a = s.next(miner, now=now)
    return a[3] - a[2] + 1


def test_rate_from_a_burst_of_results():
    """16 Results at one timestamp: one sample, the burst's nonces over the burst's time -- not 15
    infinite ones.  Depth 1 with the same work at the same speed measures the same."""
    s = Scheduler(depth=16, **SMALL)                      # target_ns = 10^6
    s.add_miner(1)
    for k in range(16):
        s.submit(k, b"r", 0, 9_999)
    while s.next(now=1_000) is not None:
        pass
    assert len(s.queue(1)) == 16
    for k in range(16):
        s.result(1, oracle.hash_(b"r", 3), 3, now=81_000)  # 160,000 nonces in 80,000 ns
    assert next_chunk_size(s, 1, 81_000) == 2 * 10 ** 6
    s = Scheduler(**SMALL)
    s.add_miner(1)
    for k in range(16):
        s.submit(k, b"r", 0, 9_999)
    for k in range(16):
        assert s.next(now=1_000 + 5_000 * k) is not None
        s.result(1, 0, 3, now=1_000 + 5_000 * (k + 1))    # 10,000 nonces in 5,000 ns, every time
    assert next_chunk_size(s, 1, 81_000) == 2 * 10 ** 6


def test_rate_folds_a_long_queue_every_target_ns():
    """Results that trickle in from a deep queue give a sample whenever target_ns has passed, with
    weight 0.5 each, and the time a miner sat idle is not counted."""
    s = Scheduler(depth=8, init_chunk=10 ** 6, min_chunk=1, max_chunk=10 ** 9, target_ns=10_000)
    s.add_miner(1)
    for k in range(4):
        s.submit(k, b"t", 0, 9_999)
    while s.next(now=0) is not None:
        pass
    assert len(s.queue(1)) == 4
    h = oracle.hash_(b"t", 0)
    s.result(1, h, 0, now=10_000)                          # 1.0 nonce/ns: sample (acc_ns = target)
    s.result(1, h, 0, now=15_000)                          # 2.0, not yet folded
    s.result(1, h, 0, now=20_000)                          # 2.0: acc 20,000 / 10,000 -> 0.5*1 + 0.5*2
    s.result(1, h, 0, now=22_500)                          # 4.0, folded as the queue empties: 2.75
    s.submit(9, b"t", 0, 9_999)
    assert s.next(now=1_000_000) is not None               # idle for ~1 ms, then 10,000 in 2,500 ns
    s.result(1, h, 0, now=1_002_500)                       # 4.0 -> 3.375
    assert next_chunk_size(s, 1, 1_002_500) == 33_750


# ---- loss ------------------------------------------------------------------------------------

def test_lost_miner_requeues_every_chunk_in_order():
    s = Scheduler(depth=8, init_chunk=10 ** 6, min_chunk=1, max_chunk=1_000, target_ns=10 ** 6)
    s.add_miner(1)
    ja = s.submit(1, b"a", 0, 2_999)
    jb = s.submit(2, b"b", 5_000, 6_999)
    lost = [s.next(1, now=0) for _ in range(5)]
    assert [(a[1], a[2]) for a in lost] == [(ja, 0), (jb, 5_000), (ja, 1_000), (jb, 6_000), (ja, 2_000)]
    assert s.queue(1) == [a[1:] for a in lost]
    s.remove_miner(1)
    st = s.stats()
    assert st["chunks_requeued"] == 5 and st["miners"] == 0 and st["jobs"] == 2
    s.add_miner(2)
    again = [s.next(now=1) for _ in range(5)]
    assert s.next(now=1) is None
    for j in (ja, jb):                                    # handed out again in nonce order per job
        assert [a[2:] for a in again if a[1] == j] == [a[2:] for a in lost if a[1] == j]
    done = {}
    for a in again:
        msg = b"a" if a[1] == ja else b"b"
        r = s.result(2, *answer(msg, a[2], a[3]), now=2)
        if r:
            done[r[0]] = r[2:]
    assert done == {ja: answer(b"a", 0, 2_999), jb: answer(b"b", 5_000, 6_999)}
    assert s.stats()["chunks_requeued"] == 5


def test_cancelled_jobs_chunks_in_a_queue_are_counted_off():
    s = Scheduler(depth=8, **SMALL)
    s.add_miner(1)
    ja = s.submit(1, b"a", 0, 99)
    jb = s.submit(2, b"b", 0, 99)
    assert [s.next(now=0)[1] for _ in range(2)] == [ja, jb]
    assert s.drop_client(1) == 1
    assert s.stats()["jobs"] == 2                         # the cancelled job lives while its chunk is out
    assert s.result(1, *answer(b"a", 0, 99), now=1) is None
    assert s.stats()["jobs"] == 1
    assert s.result(1, *answer(b"b", 0, 99), now=1) == (jb, 2) + answer(b"b", 0, 99)
    # a lost miner's chunk of a cancelled job is dropped, not requeued
    jc = s.submit(3, b"c", 0, 99)
    assert s.next(now=2)[1] == jc
    s.drop_client(3)
    s.remove_miner(1)
    st = s.stats()
    assert st["jobs"] == 0 and st["chunks_requeued"] == 0 and st["jobs_cancelled"] == 2


# ---- the desynchronisation guard -------------------------------------------------------------

def guard_setup(depth):
    s = Scheduler(depth=depth, **SMALL)
    s.add_miner(1)
    msgs = [b"client-%d" % k for k in range(8)]
    jobs = [s.submit(50 + k, m, 0, 9_999) for k, m in enumerate(msgs)]
    return s, msgs, jobs, [answer(m, 0, 9_999) for m in msgs]


def test_guard_removes_a_miner_that_skips_an_answer():
    s, msgs, jobs, exp = guard_setup(8)
    while s.next(now=0) is not None:
        pass
    assert [q[0] for q in s.queue(1)] == jobs
    assert s.result(1, *exp[0], now=1) == (jobs[0], 50) + exp[0]
    # the miner skips job 1's answer: job 2's Result arrives for job 1's chunk.  Its nonce lies in
    # [0, 9999] like every chunk here, so only the hash can tell
    with pytest.raises(MinehipError) as e:
        s.result(1, *exp[2], now=2)
    assert e.value.code == minehip.MH_EREJECTED
    st = s.stats()
    assert st["miners"] == 0 and st["chunks_requeued"] == 7 and st["jobs"] == 7
    with pytest.raises(MinehipError) as e:
        s.result(1, *exp[3], now=3)                       # the miner is gone
    assert e.value.code == minehip.MH_EINVAL
    s.add_miner(2)
    got = []
    while (a := s.next(now=4)) is not None:
        got.append(a[1])
    assert got == jobs[1:]
    done = {}
    for k in range(1, 8):
        r = s.result(2, *exp[k], now=5)
        done[r[0]] = (r[1], r[2], r[3])
    assert done == {jobs[k]: (50 + k,) + exp[k] for k in range(1, 8)}
    assert s.stats()["jobs"] == 0 and s.stats()["jobs_done"] == 8


def test_guard_rejects_a_nonce_outside_the_oldest_chunk():
    s = Scheduler(depth=2, **SMALL)
    s.add_miner(1)
    s.submit(1, b"a", 0, 99)
    s.submit(2, b"a", 100, 199)
    s.next(now=0), s.next(now=0)
    with pytest.raises(MinehipError) as e:
        s.result(1, *answer(b"a", 100, 199))              # right hash for its nonce, wrong chunk
    assert e.value.code == minehip.MH_EREJECTED and s.stats()["chunks_requeued"] == 2


def test_depth_1_keeps_its_behaviour_for_the_same_sequence():
    """No hash check at depth 1: the Result that skipped ahead is taken for the chunk that is out
    (as before), and a nonce outside the chunk is MH_ERANGE with the miner kept."""
    for s, msgs, jobs, exp in (guard_setup(1), guard_setup(None)):
        assert s.next(now=0)[1] == jobs[0]
        assert s.result(1, *exp[0], now=1) == (jobs[0], 50) + exp[0]
        assert s.next(now=1)[1] == jobs[1]
        assert s.result(1, *exp[2], now=2) == (jobs[1], 51) + exp[2]
        assert s.next(now=2)[1] == jobs[2]
        with pytest.raises(MinehipError) as e:
            s.result(1, 5, 10_000, now=3)
        assert e.value.code == minehip.MH_ERANGE
        st = s.stats()
        assert st["miners"] == 1 and st["idle_miners"] == 1 and st["chunks_requeued"] == 1
        again = []                                        # the rejected chunk goes out again, in its turn
        while (a := s.next(now=3)) is not None:
            again.append(a[1:])
            s.result(1, 5, 0, now=4)
        assert sorted(again) == [(j, 0, 9_999) for j in jobs[2:]] and s.stats()["jobs"] == 0


def test_host_hash_equals_the_oracle(golden_hash):
    """The guard's host Hash (plan.cpp host_hash) is bitcoin/hash.go's: for a one-nonce job the
    scheduler accepts exactly the oracle's hash.  Message lengths on both sides of the one / two
    tail block edge (55 + digits + 9 > 64) and of a full prefix block, nonces of 1, 2 and 20 digits."""
    cases = [(m, n, h) for m, n, h in golden_hash]
    for L in (0, 54, 55, 56, 63, 64, 119):
        msg = bytes(33 + (7 * i + L) % 90 for i in range(L))
        cases += [(msg, n, oracle.hash_(msg, n)) for n in (0, 9, 10, U64)]
    assert len(cases) > 28
    for msg, n, h in cases:
        for sent in (h, h ^ 1, h ^ (1 << 63), (h + (1 << 32)) & U64):
            s = Scheduler(depth=2, **SMALL)
            s.add_miner(1)
            j = s.submit(1, msg, n, n)
            assert s.next(now=0) == (1, j, n, n)
            if sent == h:
                assert s.result(1, h, n, now=1) == (j, 1, h, n), (msg, n)
                continue
            with pytest.raises(MinehipError) as e:
                s.result(1, sent, n, now=1)
            assert e.value.code == minehip.MH_EREJECTED and s.stats()["miners"] == 0


# ---- bad options -----------------------------------------------------------------------------

def test_bad_queue_options_raise():
    for cls in (Scheduler, Server):
        for bad in (dict(depth=0), dict(depth=65), dict(depth=1 << 31), dict(depth=-1), dict(depth=1 << 32),
                    dict(queue_ns=1 << 64), dict(depth=2, min_chunk=10, max_chunk=5)):
            with pytest.raises(MinehipError) as e:
                cls(**bad)
            assert e.value.code == minehip.MH_EINVAL, bad
        for ok in (dict(depth=1), dict(depth=64), dict(queue_ns=5), dict(depth=64, queue_ns=U64)):
            cls(**ok).close()
    import ctypes
    for create, destroy in ((minehip.lib.mh_sched_create_ex, minehip.lib.mh_sched_destroy),
                            (minehip.lib.mh_server_create_ex, minehip.lib.mh_server_destroy)):
        h = create(None, None)                             # NULL, NULL: the defaults
        assert h
        destroy(h)
        for depth, reserved in ((2, 1), (1, 7)):           # the reserved word must be zero
            q = minehip.mh_sched_queue_opts(depth, reserved, 0)
            assert not create(None, ctypes.byref(q)) and b"queue options" in minehip.lib.mh_last_error()
    assert minehip.lib.mh_sched_miner_queue(None, 0, None, 0) == minehip.MH_EINVAL
    s = Scheduler(depth=4, **SMALL)
    s.add_miner(1)
    for k in range(3):
        s.submit(k, b"q", 0, 9)
        s.next(now=0)
    assert len(s.queue(1)) == 3
    with pytest.raises(ValueError):
        s.queue(1, cap=2)                                  # cap + 1: truncated
    assert minehip.lib.mh_sched_miner_queue(s._h, 1, None, 8) == 3   # count only


# ---- the event simulation of test_sched.py, with queues ---------------------------------------

def simulate(seed, jobs, n_miners, depth, p_loss=0.1, p_join=0.1):
    """test_sched.simulate with miners that hold up to `depth` chunks and answer their whole queue
    at once, in order (one batch): random speeds, losses mid-queue, joins.  Every chunk is scanned
    with the oracle.  Returns the answers, the chunks completed per job and the stats."""
    rng = random.Random(seed)
    s = Scheduler(depth=depth, init_chunk=2000, min_chunk=300, max_chunk=20000, target_ns=10 ** 6)
    ids = list(range(n_miners))
    for m in ids:
        s.add_miner(m)
    speed = {m: rng.uniform(0.2, 5.0) for m in ids}
    job_of = {}
    for k, (msg, lo, hi) in enumerate(jobs):
        job_of[s.submit(1000 + k, msg, lo, hi)] = (msg, lo, hi)
    now, next_id, deepest = 0, n_miners, 0
    busy = {}                                             # miner -> time its current batch ends
    done, chunks = {}, {j: [] for j in job_of}
    while len(done) < len(job_of):
        while (a := s.next(now=now)) is not None:
            busy.setdefault(a[0], now)                    # chunks that join a running batch wait for the next
        for m in busy:
            if busy[m] == now and s.queue(m):
                busy[m] = now + int(sum(hi - lo + 1 for _, lo, hi in s.queue(m)) / speed[m]) + 1
        assert busy, "scheduler stalled with work left"
        m = min(busy, key=lambda x: busy[x])
        now = busy.pop(m)
        q = s.queue(m)
        deepest = max(deepest, len(q))
        assert len(q) <= depth
        if rng.random() < p_loss and len(busy) + 1 > 1:
            s.remove_miner(m)                             # lost with its whole queue
        else:
            for j, lo, hi in q:                           # the batch's Results, in order, at one time
                assert s.queue(m)[0] == (j, lo, hi)       # FIFO
                h, n = oracle.search(job_of[j][0], lo, hi, threads=1)
                chunks[j].append((lo, hi))
                r = s.result(m, h, n, now=now)
                if r is not None:
                    done[r[0]] = (r[2], r[3])
            assert s.queue(m) == []
        if rng.random() < p_join:
            s.add_miner(next_id)
            speed[next_id] = rng.uniform(0.2, 5.0)
            next_id += 1
    return done, chunks, job_of, s.stats(), deepest


@pytest.mark.parametrize("depth", [2, 8, 64])
def test_simulated_cluster_with_queues_matches_oracle(depth):
    rng = random.Random(depth)
    jobs = [(b"cmu440", 0, 59_999), (b"x" * 60, 10 ** 9 - 7_000, 10 ** 9 + 20_000),
            (b"a" * 100, U64 - 25_000, U64), (b"", 123, 9_876)]
    for k in range(40):                                   # many small ones: these stack up
        lo = rng.choice([0, 0, 10 ** rng.randrange(3, 19) - rng.randrange(0, 500), U64 - 3_000])
        jobs.append((b"small-%d" % k, lo, lo + rng.randrange(0, 3_000)))
    assert sum(hi - lo + 1 for _, lo, hi in jobs) < 3 * 10 ** 7
    done, chunks, job_of, st, deepest = simulate(440 + depth, jobs, n_miners=3, depth=depth)
    for j, (msg, lo, hi) in job_of.items():
        assert covered(chunks[j]) == [(lo, hi)]           # every nonce scanned exactly once
        assert done[j] == oracle.search(msg, lo, hi, threads=8), j
    assert st["jobs"] == 0 and st["chunks_requeued"] > 0 and st["jobs_done"] == len(jobs)
    assert deepest >= 2                                   # queues did form


# ---- the server loop -------------------------------------------------------------------------

def test_server_loop_with_queues():
    v = Server(depth=8, **WHOLE)
    for miner in (10, 11):
        v.read(miner, minehip.marshal(minehip.NewJoin()))
    msgs = {c: b"job-%d" % c for c in range(21, 33)}
    for c, m in msgs.items():
        v.read(c, minehip.marshal(minehip.NewRequest(m, 0, 4_999 + c)))
    w = v.writes()
    assert [c for c, _ in w] == [10, 11] * 6               # alternating, every job out at once
    per = {10: [minehip.unmarshal(p) for c, p in w if c == 10], 11: [minehip.unmarshal(p) for c, p in w if c == 11]}
    assert [r.Data for r in per[10]] == [msgs[c] for c in range(21, 33, 2)]
    assert v.stats()["idle_miners"] == 0 and v.stats()["chunks_assigned"] == 12
    # client 23 (in miner 10's queue) is lost: its chunk's Result is ignored when it comes back
    v.lost(23)
    assert v.stats()["jobs_cancelled"] == 1
    results = {}
    for miner in (10, 11):                                 # each miner answers its queue in order
        for r in per[miner]:
            v.read(miner, minehip.marshal(minehip.NewResult(*answer(r.Data, r.Lower, r.Upper))), now=5)
            for c, p in v.writes():
                m = minehip.unmarshal(p)
                assert m.Type == minehip.Result and c not in results
                results[c] = (m.Hash, m.Nonce)
    assert results == {c: answer(m, 0, 4_999 + c) for c, m in msgs.items() if c != 23}
    st = v.stats()
    assert st["jobs"] == 0 and st["jobs_done"] == 11 and st["idle_miners"] == 2


def test_server_guard_drops_the_miner_and_hands_its_chunks_on():
    v = Server(depth=8, **WHOLE)
    v.read(10, minehip.marshal(minehip.NewJoin()))
    for c in (1, 2, 3):
        v.read(c, minehip.marshal(minehip.NewRequest(b"g%d" % c, 0, 999)))
    assert [c for c, _ in v.writes()] == [10, 10, 10]
    v.read(11, minehip.marshal(minehip.NewJoin()))
    assert v.writes() == []
    with pytest.raises(MinehipError) as e:                 # miner 10 answers chunk 2 first
        v.read(10, minehip.marshal(minehip.NewResult(*answer(b"g2", 0, 999))), now=1)
    assert e.value.code == minehip.MH_EREJECTED
    w = v.writes()                                         # all three go to miner 11, oldest first
    assert [c for c, _ in w] == [11, 11, 11] and [minehip.unmarshal(p).Data for _, p in w] == [b"g1", b"g2", b"g3"]
    assert v.stats()["miners"] == 1 and v.stats()["chunks_requeued"] == 3
    with pytest.raises(MinehipError):                      # conn 10 is no miner any more
        v.read(10, minehip.marshal(minehip.NewResult(*answer(b"g1", 0, 999))), now=2)
    v.lost(10)                                             # the transport closes it: nothing left to undo
    for c in (1, 2, 3):
        v.read(11, minehip.marshal(minehip.NewResult(*answer(b"g%d" % c, 0, 999))), now=3)
    assert [(c, minehip.unmarshal(p).Nonce) for c, p in v.writes()] == [(c, answer(b"g%d" % c, 0, 999)[1])
                                                                       for c in (1, 2, 3)]
    assert v.stats()["jobs"] == 0
