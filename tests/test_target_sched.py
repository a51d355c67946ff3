"""CPU: target jobs of the scheduler (mh_sched_submit_first, include/minehip_server.h): ascending
hand-out, nothing above a known hit, done once everything below the hit is answered, the chunks
still out above it drained like a cancelled job's.  A seeded simulation over random chunk options,
miners, depths, answer orders and miner losses: every target job completes with the brute-force
answer of its whole range, every plain job mixed in with oracle.search's."""
import random

import pytest

import minehip
from oracle import oracle
from target_cases import FIXTURES, FIXTURE_ANSWERS, FIXTURE_MINIMA, T3, T6, U64, brute_first, chunk_answer, hashes

RANGES = FIXTURES + [(b"a" * 100, U64 - 200_000, U64, T3), (b"", 7, 7, T3), (b"", 7, 7, U64)]
CHUNKS = [dict(init_chunk=50_000, min_chunk=20_000, max_chunk=100_000),
          dict(init_chunk=100_000, min_chunk=100_000, max_chunk=100_000),
          dict(init_chunk=30_011, min_chunk=7, max_chunk=250_000),
          dict(init_chunk=400_000, min_chunk=150_000, max_chunk=1_000_000)]


def test_fixtures_are_what_the_issue_states():
    for (msg, lo, hi, t), ans, mn in zip(FIXTURES, FIXTURE_ANSWERS, FIXTURE_MINIMA):
        assert oracle.search(msg, lo, hi, threads=4) == mn
        assert brute_first(msg, lo, hi, t) == ans
        assert oracle.hash_(msg, ans[1]) == ans[0] and (ans[0] <= t or ans == mn)
    h = hashes(b"cmu440", 0, 1_999_999)
    assert [int(i) for i in (h <= T6).nonzero()[0]] == [393_322, 1_067_492, 1_456_236, 1_999_610]
    h = hashes(b"cmu440", 0, 299_999)
    assert int((h <= T3).sum()) == 285 and brute_first(b"cmu440", 0, 299_999, T3)[1] == 1_081


_minima = {}


def minimum(msg, lo, hi):
    """oracle.search of the range, computed once."""
    if (msg, lo, hi) not in _minima:
        _minima[(msg, lo, hi)] = oracle.search(msg, lo, hi, threads=4)
    return _minima[(msg, lo, hi)]


class Sim:
    """One scheduler, its jobs and what the test itself knows of them."""

    def __init__(self, rng, depth, opts):
        self.rng, self.depth = rng, depth
        self.s = minehip.Scheduler(depth=depth, **opts) if depth > 1 else minehip.Scheduler(**opts)
        self.jobs = {}      # job id -> dict(msg, lo, hi, target, client, hit (smallest reported), done, dropped)
        self.held = {}      # miner -> [(job, lo, hi)], oldest first
        self.now = 0
        self.next_miner = 100
        self.completed = {}

    def add_miner(self):
        self.s.add_miner(self.next_miner)
        self.held[self.next_miner] = []
        self.next_miner += 1

    def submit(self, client, msg, lo, hi, target):
        j = (self.s.submit(client, msg, lo, hi) if target is None
             else self.s.submit_first(client, msg, lo, hi, target))
        assert self.s.job_target(j) == target
        self.jobs[j] = dict(msg=msg, lo=lo, hi=hi, target=target, client=client, hit=None, done=False, dropped=False,
                            fresh=lo, back=[])  # the first nonce never handed out; the requeued chunks, ascending
        return j

    def hand_out(self):
        while True:
            self.now += self.rng.randrange(1, 1000)
            a = self.s.next(-1, self.now)
            if a is None:
                return
            m, j, lo, hi = a
            job = self.jobs[j]
            assert not job["done"] and not job["dropped"]
            assert job["lo"] <= lo <= hi <= job["hi"]
            if job["hit"] is not None:  # nothing above a reported hit is handed out any more
                assert lo <= job["hit"], (lo, job["hit"])
            if job["target"] is not None:
                # ascending: the lowest pending nonces first -- the lowest requeued chunk (or the
                # front of it), and fresh nonces only when none is requeued
                back = job["back"]
                if back:
                    assert lo == back[0][0] and hi <= back[0][1], (lo, hi, back)
                    if hi == back[0][1]:
                        back.pop(0)
                    else:
                        back[0] = (hi + 1, back[0][1])
                else:
                    assert lo == job["fresh"], (lo, job["fresh"])
                    job["fresh"] = hi + 1
            self.held[m].append((j, lo, hi))
            assert len(self.held[m]) <= self.depth

    def live(self, j, lo):
        """Would a lost miner's chunk of job j starting at lo be requeued?"""
        job = self.jobs[j]
        if job["done"] or job["dropped"]:
            return False
        return job["target"] is None or job["hit"] is None or lo < job["hit"]

    def lose(self, m):
        before = self.s.stats()["chunks_requeued"]
        want = sum(self.live(j, lo) for j, lo, _ in self.held[m])
        for j, lo, hi in self.held[m]:
            if self.live(j, lo):
                self.jobs[j]["back"] = sorted(self.jobs[j]["back"] + [(lo, hi)])
        self.s.remove_miner(m)
        assert self.s.stats()["chunks_requeued"] == before + want
        del self.held[m]

    def answer(self, m):
        j, lo, hi = self.held[m].pop(0)
        job = self.jobs[j]
        h, n = chunk_answer(job["msg"], lo, hi, job["target"])
        late = job["done"]
        ignored = self.s.first_stats()["results_ignored"]
        self.now += self.rng.randrange(1, 1000)
        c = self.s.result(m, h, n, self.now)
        if late:
            assert c is None and self.s.first_stats()["results_ignored"] == ignored + 1
            return
        assert self.s.first_stats()["results_ignored"] == ignored
        if job["dropped"]:
            assert c is None
            return
        if job["target"] is not None and h <= job["target"] and (job["hit"] is None or n < job["hit"]):
            job["hit"] = n
            job["back"] = [c2 for c2 in job["back"] if c2[0] < n]
        if c is not None:
            assert c[0] == j and c[1] == job["client"]
            job["done"] = True
            self.completed[j] = (c[2], c[3])

    def run(self, p_lose):
        while True:
            self.hand_out()
            busy = [m for m, q in self.held.items() if q]
            if not busy:
                break
            m = self.rng.choice(busy)
            if self.rng.random() < p_lose:
                self.lose(m)
                if not self.held or self.rng.random() < 0.7:
                    self.add_miner()
            else:
                self.answer(m)
        assert all(j["done"] or j["dropped"] for j in self.jobs.values())
        st = self.s.stats()
        assert st["jobs"] == 0 and st["idle_miners"] == st["miners"]


@pytest.mark.parametrize("seed", range(6))
def test_simulation(seed):
    rng = random.Random(4400 + seed)
    for _ in range(50):
        depth = rng.choice((1, 8))
        sim = Sim(rng, depth, rng.choice(CHUNKS))
        for _ in range(rng.randrange(1, 6)):
            sim.add_miner()
        want = {}
        for client in range(rng.randrange(1, 4)):
            msg, lo, hi, t = rng.choice(RANGES)
            if rng.random() < 0.3:
                t = None  # a plain job mixed in
            j = sim.submit(client, msg, lo, hi, t)
            want[j] = minimum(msg, lo, hi) if t is None else brute_first(msg, lo, hi, t)
        sim.run(p_lose=rng.choice((0.0, 0.05, 0.2)))
        assert sim.completed == want
        fs = sim.s.first_stats()
        targets = [j for j in sim.jobs.values() if j["target"] is not None]
        assert fs["jobs_first"] == len(targets)
        assert fs["jobs_found"] == sum(j["hit"] is not None for j in targets)
        assert sim.s.stats()["jobs_done"] == len(sim.jobs)


def fixed(miners=5, chunk=100_000, depth=None):
    s = minehip.Scheduler(init_chunk=chunk, min_chunk=chunk, max_chunk=chunk, depth=depth)
    for m in range(miners):
        s.add_miner(m)
    return s


def test_completes_while_a_chunk_above_the_hit_is_out():
    msg, lo, hi, t = FIXTURES[0]
    s = fixed()
    j = s.submit_first(9, msg, lo, hi, t)
    chunks = [s.next(-1, 0) for _ in range(5)]
    assert [(c[0], c[2], c[3]) for c in chunks] == [(m, m * 100_000, m * 100_000 + 99_999) for m in range(5)]
    assert s.next(-1, 0) is None
    for m in (0, 1, 2):
        assert s.result(m, *chunk_answer(msg, m * 100_000, m * 100_000 + 99_999, t), now=1) is None
    # the hit's chunk is the last one below it: done, with miner 4's chunk still out
    assert s.result(3, *chunk_answer(msg, 300_000, 399_999, t), now=2) == (j, 9) + FIXTURE_ANSWERS[0]
    st, fs = s.stats(), s.first_stats()
    assert st["jobs_done"] == 1 and st["jobs"] == 1 and st["idle_miners"] == 4          # finished, draining
    assert fs == dict(jobs_first=1, jobs_found=1, nonces_dropped=1_500_000, results_ignored=0)
    assert s.next(-1, 3) is None                                                         # nothing more goes out
    assert s.drop_client(9) == 0                                                         # the job is already done
    assert s.result(4, *chunk_answer(msg, 400_000, 499_999, t), now=4) is None          # the late Result
    assert s.first_stats()["results_ignored"] == 1
    st = s.stats()
    assert st["jobs"] == 0 and st["idle_miners"] == 5 and st["chunks_done"] == 5 and st["jobs_cancelled"] == 0


def test_hit_first_then_the_chunks_below_it():
    """The hit's chunk answers first: the job waits for every chunk below it, hands out nothing above
    it, does not requeue a lost chunk above it, and requeues one below it -- the lowest goes out first."""
    msg, lo, hi, t = FIXTURES[0]
    s = fixed()
    j = s.submit_first(9, msg, lo, hi, t)
    for _ in range(5):
        s.next(-1, 0)
    assert s.result(3, *chunk_answer(msg, 300_000, 399_999, t), now=1) is None
    assert s.first_stats()["nonces_dropped"] == 1_500_000
    assert s.next(3, 2) is None                       # miner 3 is idle, and everything left lies above the hit
    s.remove_miner(4)                                 # holds [400000, 499999], above the hit
    assert s.stats()["chunks_requeued"] == 0
    s.remove_miner(2)
    s.remove_miner(0)                                 # below the hit: both go back
    assert s.stats()["chunks_requeued"] == 2
    assert s.next(3, 3) == (3, j, 0, 99_999)          # ascending, whatever the order of the losses
    s.add_miner(7)
    assert s.next(-1, 3) == (7, j, 200_000, 299_999)
    assert s.next(-1, 3) is None
    assert s.result(1, *chunk_answer(msg, 100_000, 199_999, t), now=4) is None
    assert s.result(7, *chunk_answer(msg, 200_000, 299_999, t), now=5) is None
    assert s.result(3, *chunk_answer(msg, 0, 99_999, t), now=6) == (j, 9) + FIXTURE_ANSWERS[0]
    assert s.stats()["jobs"] == 0 and s.first_stats()["results_ignored"] == 0


def test_a_smaller_hit_replaces_a_larger_one():
    msg, lo, hi, t = FIXTURES[2]                     # 285 hits: every 20,000-nonce chunk has some
    s = fixed(miners=3, chunk=20_000)
    j = s.submit_first(1, msg, lo, hi, t)
    for _ in range(3):
        s.next(-1, 0)
    assert s.result(2, *chunk_answer(msg, 40_000, 59_999, t), now=1) is None
    assert s.result(1, *chunk_answer(msg, 20_000, 39_999, t), now=2) is None
    assert s.next(-1, 2) is None
    assert s.result(0, *chunk_answer(msg, 0, 19_999, t), now=3) == (j, 1) + brute_first(msg, lo, hi, t)
    assert s.first_stats() == dict(jobs_first=1, jobs_found=1, nonces_dropped=240_000, results_ignored=0)


def test_no_hit_completes_with_the_minimum_when_every_chunk_is_back():
    msg, lo, hi, t = FIXTURES[1]
    s = fixed(miners=2, chunk=400_000)
    j = s.submit_first(1, msg, lo, hi, t)
    done = []
    while not done:
        m, _, clo, chi = s.next(-1, 0)
        c = s.result(m, *chunk_answer(msg, clo, chi, t), now=1)
        if c:
            done.append(c)
    assert done == [(j, 1) + FIXTURE_MINIMA[1]]
    assert s.stats()["chunks_done"] == 5 and s.first_stats()["jobs_found"] == 0
    assert s.first_stats()["nonces_dropped"] == 0


def test_every_nonce_qualifies_answers_lower_after_one_chunk():
    msg, lo, hi = b"a" * 100, U64 - 200_000, U64
    s = fixed(miners=1, chunk=50_000)
    j = s.submit_first(1, msg, lo, hi, U64)
    m, _, clo, chi = s.next(-1, 0)
    h, n = chunk_answer(msg, clo, chi, U64)
    assert n == lo
    assert s.result(m, h, n, now=1) == (j, 1, h, lo)
    assert s.stats()["chunks_assigned"] == 1 and s.stats()["jobs"] == 0


def test_drop_client_on_a_target_job():
    msg, lo, hi, t = FIXTURES[0]
    s = fixed(miners=2)
    s.submit_first(5, msg, lo, hi, t)
    keep = s.submit(6, msg, 0, 99_999)
    a = s.next(-1, 0)
    b = s.next(-1, 0)
    assert (a[1], b[1]) == (0, keep)
    assert s.drop_client(5) == 1
    assert s.stats()["jobs"] == 2 and s.stats()["jobs_cancelled"] == 1     # its chunk is still out
    assert s.result(a[0], *chunk_answer(msg, a[2], a[3], t), now=1) is None
    assert s.stats()["jobs"] == 1 and s.first_stats()["results_ignored"] == 0
    assert s.result(b[0], *chunk_answer(msg, 0, 99_999), now=2) == (keep, 6) + chunk_answer(msg, 0, 99_999)
    assert s.next(-1, 3) is None and s.stats()["jobs"] == 0


def test_late_result_is_still_validated():
    """A finished job's late Results pass the usual checks: at depth 1 a nonce outside the chunk is
    MH_ERANGE, at depth > 1 a wrong hash removes the miner; either way the chunk is only counted off."""
    msg, lo, hi, t = FIXTURES[0]
    for depth, code in ((None, minehip.MH_ERANGE), (8, minehip.MH_EREJECTED)):
        s = fixed(miners=2, chunk=400_000, depth=depth)
        s.submit_first(1, msg, lo, hi, t)
        s.next(0, 0)
        s.next(1, 0)
        assert s.result(0, *chunk_answer(msg, 0, 399_999, t), now=1) is not None
        with pytest.raises(minehip.MinehipError) as e:
            s.result(1, 5, 5, now=2)                   # not in [400000, 799999]
        assert e.value.code == code
        st = s.stats()
        assert st["jobs"] == 0 and st["chunks_requeued"] == 0 and st["miners"] == (2 if depth is None else 1)


def test_plain_jobs_keep_the_recorded_schedule():
    """A job from mh_sched_submit takes none of the new paths: requeued chunks still go back to the
    front, newest loss first."""
    s = fixed(miners=3)
    j = s.submit(1, b"cmu440", 0, 999_999)
    for _ in range(3):
        s.next(-1, 0)
    s.remove_miner(0)
    s.remove_miner(2)
    s.add_miner(8)
    assert s.next(8, 1) == (8, j, 200_000, 299_999)   # the latest loss is at the front, as it always was
    assert s.job_target(j) is None
    assert s.first_stats() == dict(jobs_first=0, jobs_found=0, nonces_dropped=0, results_ignored=0)
