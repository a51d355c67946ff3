// sched.cpp -- Scheduler (sched.hpp) and the mh_sched_* C-ABI
// (include/minehip_server.h).  SURVEY.md §8(f) N2; reference stub
// bitcoin/server/server.go:62.
#include "sched.hpp"

#include <string.h>

#include <algorithm>
#include <cmath>

#include "../../include/minehip.h"

namespace mh {
int set_error(int code, const char* what);

namespace {
inline bool lex_less(uint64_t ha, uint64_t na, uint64_t hb, uint64_t nb) {
    return ha < hb || (ha == hb && na < nb);
}
}  // namespace

bool Scheduler::valid_opts(const mh_sched_opts& o) {
    return o.init_chunk >= 1 && o.min_chunk >= 1 && o.max_chunk >= o.min_chunk && o.target_ns >= 1;
}

Scheduler::Scheduler(const mh_sched_opts& opts) : o_(opts) {}

Scheduler::u128 Scheduler::Job::pending() const {
    u128 p = exhausted ? 0 : (u128)(upper - next) + 1u;
    for (const auto& r : requeue) p += (u128)(r.second - r.first) + 1u;
    return p;
}

Scheduler::Job* Scheduler::find_job(int64_t id) {
    for (auto& j : jobs_)
        if (j->id == id) return j.get();
    return nullptr;
}

Scheduler::Miner* Scheduler::find_miner(int64_t id) {
    for (auto& m : miners_)
        if (m.id == id) return &m;
    return nullptr;
}

void Scheduler::erase_job(int64_t id) {
    for (size_t i = 0; i < jobs_.size(); ++i) {
        if (jobs_[i]->id != id) continue;
        jobs_.erase(jobs_.begin() + (ptrdiff_t)i);
        if (rr_ > i) --rr_;
        if (rr_ >= jobs_.size()) rr_ = 0;
        return;
    }
}

// rate x target, capped at the job's fair share of what is left (guided
// self-scheduling: half of an even split, so the tail is spread over every
// miner; a lone miner has no tail to share), clamped.
uint64_t Scheduler::chunk_size(const Miner& m, const Job& j) const {
    double want = m.rate > 0.0 ? m.rate * (double)o_.target_ns : (double)o_.init_chunk;
    const size_t nm = miners_.size();
    const u128 share = j.pending() / (u128)(nm > 1 ? 2u * nm : 1u);
    if ((double)share < want) want = (double)share;
    if (want < (double)o_.min_chunk) want = (double)o_.min_chunk;
    if (want > (double)o_.max_chunk) want = (double)o_.max_chunk;
    const uint64_t c = (uint64_t)want;
    return c < 1 ? 1 : c;
}

// Cut up to c nonces from the job: requeued chunks first (oldest loss first).
bool Scheduler::take(Job& j, uint64_t c, uint64_t* lo, uint64_t* hi) {
    if (!j.requeue.empty()) {
        auto& r = j.requeue.front();
        *lo = r.first;
        if (r.second - r.first <= c - 1u) {
            *hi = r.second;
            j.requeue.pop_front();
        } else {
            *hi = r.first + (c - 1u);
            r.first = *hi + 1u;
        }
        return true;
    }
    if (j.exhausted) return false;
    *lo = j.next;
    if (j.upper - j.next <= c - 1u) {
        *hi = j.upper;
        j.exhausted = true;
    } else {
        *hi = j.next + (c - 1u);
        j.next = *hi + 1u;
    }
    return true;
}

bool Scheduler::valid_queue_opts(const mh_sched_queue_opts& q) {
    return q.depth >= 1 && q.depth <= MH_SCHED_MAX_DEPTH && q.reserved == 0;
}

void Scheduler::set_queue(const mh_sched_queue_opts& q, HostHash hash) {
    std::lock_guard<std::mutex> lk(mu_);
    q_ = q;
    hash_ = hash;
}

// May m be handed another chunk?  Idle: always.  Otherwise while it holds fewer than depth chunks
// and fewer nonces than it works off in queue_ns -- a large job's chunk (rate x target_ns) fills
// that alone, so only small jobs stack up.
bool Scheduler::eligible(const Miner& m) const {
    if (m.q.empty()) return true;
    if (m.q.size() >= q_.depth) return false;
    const double ns = (double)(q_.queue_ns ? q_.queue_ns : o_.target_ns);
    const double budget = m.rate > 0.0 ? m.rate * ns : (double)o_.init_chunk;
    return (double)m.held < std::floor(budget);  // whole nonces, as chunk_size cuts them
}

// A chunk that will not be answered goes back to the front of its job (a cancelled job only
// counts it off).  A target job's requeued chunks stay in ascending order (take cuts from the
// front: the lowest nonces first), and one that lies above a known hit is not wanted any more; a
// finished job only counts it off, as a cancelled one does.
void Scheduler::requeue_chunk(const Chunk& c) {
    Job* j = find_job(c.job);
    if (!j) return;
    j->outstanding -= 1u;
    if (j->cancelled || j->finished) {
        if (j->outstanding == 0) erase_job(j->id);
    } else if (!j->first) {
        j->requeue.emplace_front(c.lo, c.hi);
        st_.chunks_requeued += 1u;
    } else if (!j->hit || c.lo < j->hit_nonce) {
        auto it = j->requeue.begin();
        while (it != j->requeue.end() && it->first < c.lo) ++it;
        j->requeue.insert(it, std::make_pair(c.lo, c.hi));
        st_.chunks_requeued += 1u;
    }
}

// A (smaller) hit became known: nothing above it is handed out any more.  The fresh remainder goes
// (next is already above the hit's chunk), and so do the requeued chunks above the hit.  Chunks are
// disjoint and the hit lies in an answered one, so every other chunk is wholly below or above it.
void Scheduler::prune_above_hit(Job& j) {
    if (!j.exhausted) {
        fst_.nonces_dropped += j.upper - j.next + 1u;
        j.exhausted = true;
    }
    while (!j.requeue.empty() && j.requeue.back().first > j.hit_nonce) j.requeue.pop_back();
}

// Does some miner still hold a chunk of j below its hit?
bool Scheduler::out_below_hit(const Job& j) const {
    for (const auto& m : miners_)
        for (const Chunk& c : m.q)
            if (c.job == j.id && c.lo < j.hit_nonce) return true;
    return false;
}

// Miner i is gone: its chunks go back, newest first, so that the oldest ends up at the front.
void Scheduler::drop_miner(size_t i) {
    Miner& m = miners_[i];
    for (auto it = m.q.rbegin(); it != m.q.rend(); ++it) requeue_chunk(*it);
    miners_.erase(miners_.begin() + (ptrdiff_t)i);
}

int Scheduler::add_miner(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    if (find_miner(id)) return set_error(MH_EINVAL, "miner already joined");
    miners_.push_back(Miner{id, {}, 0, 0, 0.0, 0, 0.0});
    return MH_OK;
}

int Scheduler::remove_miner(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t i = 0; i < miners_.size(); ++i) {
        if (miners_[i].id != id) continue;
        drop_miner(i);
        return MH_OK;
    }
    return set_error(MH_EINVAL, "unknown miner");
}

int64_t Scheduler::submit(int64_t client, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper) {
    return submit_job(client, msg, len, lower, upper, false, 0);
}

int64_t Scheduler::submit_first(int64_t client, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                                uint64_t target) {
    return submit_job(client, msg, len, lower, upper, true, target);
}

int64_t Scheduler::submit_job(int64_t client, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                              bool first, uint64_t target) {
    if (!msg && len) return set_error(MH_EINVAL, "msg is NULL");
    if (len > MH_MAX_MSG_LEN) return set_error(MH_ETOOLONG, "message longer than MH_MAX_MSG_LEN");
    if (lower > upper) return set_error(MH_ERANGE, "lower > upper");
    std::lock_guard<std::mutex> lk(mu_);
    std::unique_ptr<Job> j(new Job());
    j->id = next_job_++;
    j->client = client;
    j->msg.assign((const char*)msg, len);
    j->lower = lower;
    j->upper = upper;
    j->next = lower;
    j->exhausted = false;
    j->outstanding = 0;
    j->best_hash = j->best_nonce = ~0ull;
    j->cancelled = false;
    j->first = first;
    j->hit = j->finished = false;
    j->target = target;
    j->hit_hash = j->hit_nonce = ~0ull;
    if (first) fst_.jobs_first += 1u;
    jobs_.push_back(std::move(j));
    return jobs_.back()->id;
}

int Scheduler::drop_client(int64_t client) {
    std::lock_guard<std::mutex> lk(mu_);
    int n = 0;
    std::vector<int64_t> gone;
    for (auto& j : jobs_) {
        if (j->client != client || j->cancelled || j->finished) continue;  // a finished job only drains
        j->cancelled = true;
        j->exhausted = true;
        j->requeue.clear();
        st_.jobs_cancelled += 1u;
        ++n;
        if (j->outstanding == 0) gone.push_back(j->id);
    }
    for (int64_t id : gone) erase_job(id);
    return n;
}

int Scheduler::next(int64_t miner, uint64_t now_ns, mh_assignment* out) {
    if (!out) return set_error(MH_EINVAL, "NULL output");
    std::lock_guard<std::mutex> lk(mu_);
    Miner* m = nullptr;
    if (miner >= 0) {
        m = find_miner(miner);
        if (!m) return set_error(MH_EINVAL, "unknown miner");
        if (!eligible(*m)) return 0;
    } else {
        // the eligible miner with the fewest chunks out, ties in join order: every miner gets its
        // first chunk before any gets a second
        for (auto& x : miners_)
            if (eligible(x) && (!m || x.q.size() < m->q.size())) m = &x;
        if (!m) return 0;
    }
    const size_t nj = jobs_.size();
    for (size_t k = 0; k < nj; ++k) {
        const size_t idx = (rr_ + k) % nj;
        Job& j = *jobs_[idx];
        if (j.cancelled || j.finished) continue;
        uint64_t lo, hi;
        if (!take(j, chunk_size(*m, j), &lo, &hi)) continue;
        rr_ = (idx + 1) % nj;
        j.outstanding += 1u;
        if (m->q.empty()) m->t_busy = now_ns;
        m->q.push_back(Chunk{j.id, lo, hi});
        m->held += (u128)(hi - lo) + 1u;
        st_.chunks_assigned += 1u;
        out->miner = m->id;
        out->job = j.id;
        out->lower = lo;
        out->upper = hi;
        out->msg_len = j.msg.size();
        return 1;
    }
    return 0;
}

int Scheduler::job_msg(int64_t job, std::string* out) {
    std::lock_guard<std::mutex> lk(mu_);
    Job* j = find_job(job);
    if (!j) return set_error(MH_EINVAL, "unknown job");
    *out = j->msg;
    return MH_OK;
}

int Scheduler::job_target(int64_t job, bool* has_target, uint64_t* target) {
    std::lock_guard<std::mutex> lk(mu_);
    Job* j = find_job(job);
    if (!j) return set_error(MH_EINVAL, "unknown job");
    *has_target = j->first;
    *target = j->first ? j->target : 0;
    return MH_OK;
}

int Scheduler::miner_queue(int64_t miner, std::vector<mh_assignment>* out) {
    std::lock_guard<std::mutex> lk(mu_);
    Miner* m = find_miner(miner);
    if (!m) return set_error(MH_EINVAL, "unknown miner");
    out->clear();
    for (const Chunk& c : m->q) {
        Job* j = find_job(c.job);
        out->push_back(mh_assignment{m->id, c.job, c.lo, c.hi, j ? j->msg.size() : 0});
    }
    return MH_OK;
}

int Scheduler::result(int64_t miner, uint64_t hash, uint64_t nonce, uint64_t now_ns, mh_completion* out) {
    std::lock_guard<std::mutex> lk(mu_);
    Miner* m = find_miner(miner);
    if (!m || m->q.empty()) return set_error(MH_EINVAL, "Result from a miner with no chunk out");
    const Chunk c = m->q.front();  // a Result carries no id: it answers the oldest chunk
    Job* j = find_job(c.job);
    if (q_.depth > 1) {
        // Several chunks out: a miner that skipped or reordered an answer would have every later
        // Result credited to the wrong chunk, and the nonce test cannot see that when clients ask
        // for the same range with different Data.  The hash ties the Result to this job's Data.
        const bool ok = j && nonce >= c.lo && nonce <= c.hi && hash_ &&
                        hash_((const uint8_t*)j->msg.data(), j->msg.size(), nonce) == hash;
        if (!ok) {
            drop_miner((size_t)(m - miners_.data()));
            return set_error(MH_EREJECTED, "Result does not answer the miner's oldest chunk; miner removed");
        }
    }
    m->q.pop_front();
    m->held -= (u128)(c.hi - c.lo) + 1u;
    if (!j) return 0;  // cannot happen: a job lives while chunks are out
    if (nonce < c.lo || nonce > c.hi) {
        requeue_chunk(c);  // depth 1 only: the miner stays, idle
        return set_error(MH_ERANGE, "Result nonce outside the miner's chunk");
    }
    // Rate: nonces completed over the time the miner was busy with them.  Results of one batch
    // arrive in a burst, so samples are folded when the queue runs empty or spans target_ns, not
    // per Result; with one chunk out this is one sample per chunk, cnt / (now - t0).
    m->acc_nonces += (double)(c.hi - c.lo) + 1.0;
    if (now_ns > m->t_busy) m->acc_ns += now_ns - m->t_busy;
    m->t_busy = now_ns;
    if (m->q.empty() || m->acc_ns >= o_.target_ns) {
        if (m->acc_ns > 0) {
            const double r = m->acc_nonces / (double)m->acc_ns;
            m->rate = m->rate > 0.0 ? 0.5 * m->rate + 0.5 * r : r;
        }
        m->acc_nonces = 0.0;
        m->acc_ns = 0;
    }
    st_.chunks_done += 1u;
    st_.nonces_done += c.hi - c.lo + 1u;  // wraps only for a single 2^64 chunk
    j->outstanding -= 1u;
    if (j->cancelled || j->finished) {  // a late Result: counted off and ignored
        if (j->finished) fst_.results_ignored += 1u;
        if (j->outstanding == 0) erase_job(j->id);
        return 0;
    }
    if (j->first && hash <= j->target) {
        // a hit: the job keeps the one with the smallest nonce
        if (!j->hit || nonce < j->hit_nonce) {
            j->hit = true;
            j->hit_hash = hash;
            j->hit_nonce = nonce;
            prune_above_hit(*j);
        }
    } else if (lex_less(hash, nonce, j->best_hash, j->best_nonce)) {
        j->best_hash = hash;
        j->best_nonce = nonce;
    }
    // Done: every chunk is back -- or, with a hit, every chunk below it (after prune_above_hit the
    // requeued ones all are); chunks still out above the hit drain like a cancelled job's.
    if (j->hit ? (!j->requeue.empty() || out_below_hit(*j))
               : (j->outstanding != 0 || !j->exhausted || !j->requeue.empty()))
        return 0;
    if (out) {
        out->job = j->id;
        out->client = j->client;
        out->hash = j->hit ? j->hit_hash : j->best_hash;
        out->nonce = j->hit ? j->hit_nonce : j->best_nonce;
    }
    st_.jobs_done += 1u;
    if (j->hit) fst_.jobs_found += 1u;
    if (j->outstanding == 0)
        erase_job(j->id);
    else
        j->finished = true;
    return 1;
}

void Scheduler::stats(mh_sched_stats* out) {
    std::lock_guard<std::mutex> lk(mu_);
    *out = st_;
    out->miners = miners_.size();
    out->idle_miners = 0;
    for (const auto& m : miners_) out->idle_miners += m.q.empty() ? 1u : 0u;
    out->jobs = jobs_.size();
}

void Scheduler::first_stats(mh_sched_first_stats* out) {
    std::lock_guard<std::mutex> lk(mu_);
    *out = fst_;
}

bool Scheduler::idle_jobs() {
    std::lock_guard<std::mutex> lk(mu_);
    return jobs_.empty();
}

}  // namespace mh

extern "C" {

void mh_sched_default_opts(mh_sched_opts* o) {
    if (!o) return;
    o->init_chunk = 1ull << 30;
    o->min_chunk = 1ull << 24;
    o->max_chunk = 1ull << 38;
    o->target_ns = 250000000ull;
}

mh_sched* mh_sched_create(const mh_sched_opts* opts) {
    mh_sched_opts o;
    mh_sched_default_opts(&o);
    if (opts) o = *opts;
    if (!mh::Scheduler::valid_opts(o)) {
        mh::set_error(MH_EINVAL, "bad scheduler options");
        return nullptr;
    }
    return new mh_sched(o);
}

void mh_sched_default_queue_opts(mh_sched_queue_opts* q) {
    if (!q) return;
    q->depth = 1;
    q->reserved = 0;
    q->queue_ns = 0;
}

void mh_sched_destroy(mh_sched* s) { delete s; }

#define MH_NEED(s) \
    if (!(s)) return mh::set_error(MH_EINVAL, "NULL scheduler")

int mh_sched_add_miner(mh_sched* s, int64_t miner) {
    MH_NEED(s);
    return s->s.add_miner(miner);
}

int mh_sched_remove_miner(mh_sched* s, int64_t miner) {
    MH_NEED(s);
    return s->s.remove_miner(miner);
}

int64_t mh_sched_submit(mh_sched* s, int64_t client, const uint8_t* msg, size_t len, uint64_t lower,
                        uint64_t upper) {
    MH_NEED(s);
    return s->s.submit(client, msg, len, lower, upper);
}

int64_t mh_sched_submit_first(mh_sched* s, int64_t client, const uint8_t* msg, size_t len, uint64_t lower,
                              uint64_t upper, uint64_t target) {
    MH_NEED(s);
    return s->s.submit_first(client, msg, len, lower, upper, target);
}

int mh_sched_job_target(mh_sched* s, int64_t job, int* has_target, uint64_t* target) {
    MH_NEED(s);
    if (!has_target || !target) return mh::set_error(MH_EINVAL, "NULL output");
    bool has = false;
    const int rc = s->s.job_target(job, &has, target);
    if (rc) return rc;
    *has_target = has ? 1 : 0;
    return MH_OK;
}

int mh_sched_drop_client(mh_sched* s, int64_t client) {
    MH_NEED(s);
    return s->s.drop_client(client);
}

int mh_sched_next(mh_sched* s, int64_t miner, uint64_t now_ns, mh_assignment* out) {
    MH_NEED(s);
    return s->s.next(miner, now_ns, out);
}

int mh_sched_job_msg(mh_sched* s, int64_t job, uint8_t* buf, size_t cap, size_t* len) {
    MH_NEED(s);
    std::string m;
    int rc = s->s.job_msg(job, &m);
    if (rc) return rc;
    if (len) *len = m.size();
    if (m.size() > cap || (!buf && !m.empty())) return mh::set_error(MH_ETOOLONG, "buffer too small");
    if (!m.empty()) memcpy(buf, m.data(), m.size());
    return MH_OK;
}

int64_t mh_sched_miner_queue(mh_sched* s, int64_t miner, mh_assignment* out, int64_t cap) {
    MH_NEED(s);
    if (cap < 0) return mh::set_error(MH_EINVAL, "cap < 0");
    std::vector<mh_assignment> q;
    const int rc = s->s.miner_queue(miner, &q);
    if (rc) return rc;
    int64_t k = 0;
    for (const mh_assignment& a : q) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = a;
        ++k;
    }
    return k;
}

int mh_sched_result(mh_sched* s, int64_t miner, uint64_t hash, uint64_t nonce, uint64_t now_ns,
                    mh_completion* out) {
    MH_NEED(s);
    return s->s.result(miner, hash, nonce, now_ns, out);
}

int mh_sched_stats_read(mh_sched* s, mh_sched_stats* out) {
    MH_NEED(s);
    if (!out) return mh::set_error(MH_EINVAL, "NULL output");
    s->s.stats(out);
    return MH_OK;
}

int mh_sched_first_stats_read(mh_sched* s, mh_sched_first_stats* out) {
    MH_NEED(s);
    if (!out) return mh::set_error(MH_EINVAL, "NULL output");
    s->s.first_stats(out);
    return MH_OK;
}

}  // extern "C"
