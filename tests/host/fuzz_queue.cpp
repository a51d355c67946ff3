// fuzz_queue.cpp -- the scheduler's per-miner chunk queues and the server loop on top of them
// (mh_sched_create_ex / mh_server_create_ex, include/minehip_server.h "Queueing") under
// AddressSanitizer + UBSan: tests/test_queue_sanitize.py builds this file with plan.cpp,
// sched.cpp, server.cpp and message.cpp and runs it directly.  Host code only.
//
// Random join / submit / next / result / lose / drop sequences at random depths, against a
// model that keeps, per miner, the chunks it was handed.  Checked after every step:
//   - a miner never holds more than depth chunks, and mh_sched_miner_queue lists exactly the
//     model's chunks, oldest first (FIFO);
//   - next(-1) hands an idle miner (the earliest joined) a chunk before a busy one gets another;
//   - an honest Result (a nonce of the oldest chunk with its host Hash) is accepted and completes
//     the oldest chunk; a Result for another chunk is MH_EREJECTED at depth > 1 and removes the
//     miner, whose chunks all come back;
//   - the chunks completed for a finished job tile its range exactly once, and its answer is the
//     lexicographic minimum of the Results given;
// and at the end honest miners finish every job that was not cancelled.
//
//   fuzz_queue [seed] [iterations]      prints "... failures=0" and exits 0 when clean
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../bitcoin-miner_amd/csrc/msgcodec.hpp"
#include "../../bitcoin-miner_amd/csrc/plan.hpp"
#include "../../include/minehip.h"
#include "../../include/minehip_server.h"

namespace mh {
int set_error(int code, const char*) { return code; }
}  // namespace mh

// message.cpp's miner step calls the searches; nothing here does
extern "C" int mh_search(int, const uint8_t*, size_t, uint64_t, uint64_t, uint64_t*, uint64_t*) { return MH_ENODEV; }
extern "C" int mh_search_multi(const int*, int, const uint8_t*, size_t, uint64_t, uint64_t, uint64_t, uint64_t*,
                               uint64_t*) {
    return MH_ENODEV;
}

static int g_fail = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                             \
            return;                                                               \
        }                                                                         \
    } while (0)

static std::mt19937_64 rng;
static uint64_t rnd(uint64_t n) { return n ? rng() % n : 0; }
static uint64_t g_results = 0, g_rejected = 0, g_deepest = 0;
static bool g_handed = false;  // the last hand_out handed a chunk out

static uint64_t hash_of(const std::string& msg, uint64_t nonce) {
    return mh::host_hash((const uint8_t*)msg.data(), msg.size(), nonce);
}

namespace {

struct JobModel {
    std::string msg;
    uint64_t lo, hi;
    int64_t client;
    bool cancelled = false, done = false;
    std::vector<std::pair<uint64_t, uint64_t>> got;  // completed chunks
    uint64_t best_hash = ~0ull, best_nonce = ~0ull;
};

struct Model {
    mh_sched* s = nullptr;
    uint32_t depth = 1;
    std::map<int64_t, JobModel> jobs;
    std::map<int64_t, std::deque<mh_assignment>> held;  // live miners -> their chunks, oldest first
    std::vector<int64_t> order;                         // live miners in join order
    uint64_t requeued = 0;                              // chunks that went back (lost or rejected miners)
};

void check_queues(Model& m) {
    for (auto& kv : m.held) {
        CHECK(kv.second.size() <= m.depth);
        if (kv.second.size() > g_deepest) g_deepest = kv.second.size();
        mh_assignment buf[MH_SCHED_MAX_DEPTH];
        const int64_t k = mh_sched_miner_queue(m.s, kv.first, buf, MH_SCHED_MAX_DEPTH);
        CHECK(k == (int64_t)kv.second.size());
        for (int64_t i = 0; i < k; ++i) {
            const mh_assignment& a = kv.second[(size_t)i];
            CHECK(buf[i].miner == kv.first && buf[i].job == a.job && buf[i].lower == a.lower && buf[i].upper == a.upper);
        }
        if (k > 1) CHECK(mh_sched_miner_queue(m.s, kv.first, buf, k - 1) == k);  // cap + 1: truncated
    }
    mh_sched_stats st;
    CHECK(mh_sched_stats_read(m.s, &st) == MH_OK);
    uint64_t idle = 0;
    for (auto& kv : m.held) idle += kv.second.empty();
    CHECK(st.miners == m.held.size() && st.idle_miners == idle);
}

// the chunks of a lost or rejected miner: counted, unless their job was cancelled
void give_back(Model& m, int64_t miner) {
    for (const mh_assignment& a : m.held[miner])
        if (!m.jobs[a.job].cancelled) ++m.requeued;
    m.held.erase(miner);
    m.order.erase(std::find(m.order.begin(), m.order.end(), miner));
}

void finish_job(Model& m, const mh_completion& c) {
    JobModel& j = m.jobs[c.job];
    CHECK(!j.cancelled && !j.done && c.client == j.client);
    j.done = true;
    auto v = j.got;
    std::sort(v.begin(), v.end());
    CHECK(!v.empty() && v.front().first == j.lo && v.back().second == j.hi);
    for (size_t k = 1; k < v.size(); ++k) CHECK(v[k].first == v[k - 1].second + 1u && v[k - 1].second >= v[k - 1].first);
    CHECK(c.hash == j.best_hash && c.nonce == j.best_nonce);
}

// the miner's oldest chunk, answered honestly
void honest_result(Model& m, int64_t miner, uint64_t now) {
    auto& q = m.held[miner];
    CHECK(!q.empty());
    const mh_assignment a = q.front();
    q.pop_front();
    JobModel& j = m.jobs[a.job];
    const uint64_t nonce = a.lower + rnd(a.upper - a.lower + 1u);
    const uint64_t h = hash_of(j.msg, nonce);
    mh_completion c;
    const int r = mh_sched_result(m.s, miner, h, nonce, now, &c);
    CHECK(r == 0 || r == 1);
    ++g_results;
    if (j.cancelled) {
        CHECK(r == 0);
        return;
    }
    j.got.push_back({a.lower, a.upper});
    if (h < j.best_hash || (h == j.best_hash && nonce < j.best_nonce)) {
        j.best_hash = h;
        j.best_nonce = nonce;
    }
    if (r == 1) {
        CHECK(c.job == a.job);
        finish_job(m, c);
    }
}

void hand_out(Model& m, int64_t want, uint64_t now) {
    mh_assignment a;
    const int r = mh_sched_next(m.s, want, now, &a);
    CHECK(r == 0 || r == 1);
    if (r == 0) return;
    CHECK(m.held.count(a.miner) && (want < 0 || a.miner == want));
    JobModel& j = m.jobs[a.job];
    CHECK(!j.cancelled && !j.done && a.lower <= a.upper && a.lower >= j.lo && a.upper <= j.hi && a.msg_len == j.msg.size());
    auto& q = m.held[a.miner];
    if (want < 0) {
        // an idle miner goes first, the earliest joined of them
        for (int64_t id : m.order) {
            if (!m.held[id].empty()) continue;
            CHECK(a.miner == id);
            break;
        }
    }
    q.push_back(a);
    g_handed = true;
}

}  // namespace

static void fuzz_sched_queue() {
    Model m;
    mh_sched_opts o;
    o.init_chunk = 1 + rnd(20000);
    o.min_chunk = 1 + rnd(2000);
    o.max_chunk = o.min_chunk + rnd(20000);
    o.target_ns = 1 + rnd(100000);
    mh_sched_queue_opts q;
    mh_sched_default_queue_opts(&q);
    CHECK(q.depth == 1 && q.reserved == 0 && q.queue_ns == 0);
    q.depth = rnd(4) == 0 ? 1u : 1u + (uint32_t)rnd(MH_SCHED_MAX_DEPTH);
    q.queue_ns = rnd(3) ? 0 : rnd(1000000);
    m.depth = q.depth;
    m.s = mh_sched_create_ex(&o, &q);
    CHECK(m.s != nullptr);
    int64_t next_miner = 0;
    uint64_t now = 0;
    for (int step = 0; step < 500 && !g_fail; ++step) {
        now += rnd(4) ? rnd(1000) : 0;  // bursts share a timestamp
        switch (rnd(10)) {
            case 0:
                CHECK(mh_sched_add_miner(m.s, next_miner) == MH_OK);
                m.held[next_miner];
                m.order.push_back(next_miner++);
                break;
            case 1:
                if (!m.order.empty() && rnd(3) == 0) {
                    const int64_t id = m.order[rnd(m.order.size())];
                    CHECK(mh_sched_remove_miner(m.s, id) == MH_OK);
                    give_back(m, id);
                }
                break;
            case 2:
            case 3: {
                uint64_t lo = rnd(3) ? rnd(1000000) : ~0ull - rnd(30000), hi = lo + rnd(rnd(2) ? 3000 : 40000);
                if (hi < lo) hi = ~0ull;
                JobModel j;
                j.msg = "job " + std::to_string(step) + std::string(rnd(70), 'x');  // unique per job
                j.lo = lo;
                j.hi = hi;
                j.client = (int64_t)rnd(6);
                const int64_t id = mh_sched_submit(m.s, j.client, (const uint8_t*)j.msg.data(), j.msg.size(), lo, hi);
                CHECK(id >= 0 && !m.jobs.count(id));
                m.jobs[id] = j;
                break;
            }
            case 4:
                if (rnd(4) == 0) {
                    const int64_t c = (int64_t)rnd(6);
                    int n = 0;
                    for (auto& kv : m.jobs)
                        if (kv.second.client == c && !kv.second.cancelled && !kv.second.done) {
                            kv.second.cancelled = true;
                            ++n;
                        }
                    CHECK(mh_sched_drop_client(m.s, c) == n);
                }
                break;
            case 5:
                if (!m.order.empty()) hand_out(m, m.order[rnd(m.order.size())], now);
                break;
            case 6:
            case 7:
                for (uint64_t k = rnd(2) ? 1 : 1 + rnd(2 * m.depth); k > 0 && !g_fail; --k) hand_out(m, -1, now);
                break;
            default: {
                if (m.order.empty()) break;
                const int64_t id = m.order[rnd(m.order.size())];
                auto& qd = m.held[id];
                if (qd.empty()) {
                    CHECK(mh_sched_result(m.s, id, 1, 2, now, nullptr) == MH_EINVAL);
                } else if (qd.size() > 1 && rnd(8) == 0) {
                    // the miner skips its oldest chunk and answers the second: a nonce of the second
                    // chunk is outside the first, or hashed with another job's Data
                    const mh_assignment b = qd[1];
                    const uint64_t h = hash_of(m.jobs[b.job].msg, b.lower);
                    CHECK(mh_sched_result(m.s, id, h, b.lower, now, nullptr) == MH_EREJECTED);
                    ++g_rejected;
                    give_back(m, id);
                    CHECK(mh_sched_result(m.s, id, h, b.lower, now, nullptr) == MH_EINVAL);  // gone
                } else {
                    // one Result, or the whole queue in a burst
                    for (size_t k = rnd(2) ? 1 : qd.size(); k > 0 && !g_fail; --k) honest_result(m, id, now);
                }
            }
        }
        if (g_fail) break;
        check_queues(m);
        mh_sched_stats st;
        mh_sched_stats_read(m.s, &st);
        CHECK(st.chunks_requeued == m.requeued);
    }
    // honest miners finish what is left
    if (!g_fail) {
        if (m.order.empty()) {
            CHECK(mh_sched_add_miner(m.s, next_miner) == MH_OK);
            m.held[next_miner];
            m.order.push_back(next_miner);
        }
        for (int guard = 0; guard < 100000 && !g_fail; ++guard) {
            now += 1 + rnd(500);
            do {
                g_handed = false;
                hand_out(m, -1, now);
            } while (g_handed && !g_fail);
            bool any = false;
            for (int64_t id : std::vector<int64_t>(m.order))
                while (!m.held[id].empty() && !g_fail) {
                    honest_result(m, id, now);
                    any = true;
                }
            if (!any) break;
        }
        mh_sched_stats st;
        mh_sched_stats_read(m.s, &st);
        CHECK(st.jobs == 0);
        for (auto& kv : m.jobs) CHECK(kv.second.done || kv.second.cancelled);
    }
    mh_sched_destroy(m.s);
}

// The server loop at a random depth: every job is one chunk (min_chunk above the job sizes), miners
// answer their queued Requests in order, some are lost with their queue, one skips an answer (and
// must be dropped: MH_EREJECTED), clients are lost.  Every client that stays gets exactly one
// Result per Request, the right one.
static void fuzz_server_queue() {
    mh_sched_opts o;
    mh_sched_default_opts(&o);
    o.init_chunk = 1000000;
    o.min_chunk = 100000;
    o.max_chunk = 1000000;
    mh_sched_queue_opts q;
    mh_sched_default_queue_opts(&q);
    q.depth = 1u + (uint32_t)rnd(MH_SCHED_MAX_DEPTH);
    mh_server* v = mh_server_create_ex(&o, &q);
    CHECK(v != nullptr);
    std::map<int64_t, std::deque<mh::Msg>> inbox;              // miner conn -> Requests it holds
    std::map<int64_t, std::pair<uint64_t, uint64_t>> expect;   // client conn -> its Result
    std::map<int64_t, int> answered;
    int64_t next_conn = 1;
    std::vector<char> buf(1 << 12);
    auto drain = [&]() {
        int64_t c;
        size_t n;
        for (;;) {
            const int k = mh_server_pop_write(v, &c, buf.data(), buf.size(), &n);
            if (k == MH_EINVAL) {
                buf.resize(n);
                continue;
            }
            if (k != 1) return;
            mh::Msg m;
            CHECK(mh::decode(buf.data(), n, &m));
            if (m.type == 1) {
                CHECK(inbox.count(c));
                inbox[c].push_back(m);
                CHECK(inbox[c].size() <= q.depth);
            } else {
                CHECK(m.type == 2 && expect.count(c));
                CHECK(m.hash == expect[c].first && m.nonce == expect[c].second);
                ++answered[c];
            }
        }
    };
    const std::string join = mh::encode(0, nullptr, 0, 0, 0, 0, 0);
    for (int step = 0; step < 300 && !g_fail; ++step) {
        const uint64_t now = (uint64_t)step * 1000u;
        switch (rnd(8)) {
            case 0: {
                CHECK(mh_server_read(v, next_conn, join.data(), join.size(), now) == MH_OK);
                inbox[next_conn++];
                break;
            }
            case 1:
            case 2:
            case 3: {  // a client with one Request of one nonce range [n, n + k]
                const std::string data = "c" + std::to_string(next_conn);
                const uint64_t lo = rnd(2) ? rnd(100000) : ~0ull - rnd(5000), k = rnd(3), hi = lo + k < lo ? ~0ull : lo + k;
                // the only Result its one chunk can give, as the miners below answer: (Hash(lo), lo)
                expect[next_conn] = {hash_of(data, lo), lo};
                const std::string p = mh::encode(1, (const uint8_t*)data.data(), data.size(), lo, hi, 0, 0);
                CHECK(mh_server_read(v, next_conn++, p.data(), p.size(), now) == MH_OK);
                break;
            }
            case 4:
                if (!inbox.empty() && rnd(4) == 0) {  // a miner is lost with its queue
                    auto it = inbox.begin();
                    std::advance(it, (long)rnd(inbox.size()));
                    CHECK(mh_server_lost(v, it->first, now) == MH_OK);
                    inbox.erase(it);
                }
                break;
            case 5:
                if (!expect.empty() && rnd(4) == 0) {  // a client is lost
                    auto it = expect.begin();
                    std::advance(it, (long)rnd(expect.size()));
                    if (answered[it->first] == 0) {
                        CHECK(mh_server_lost(v, it->first, now) == MH_OK);
                        answered.erase(it->first);
                        expect.erase(it);
                    }
                }
                break;
            default: {
                if (inbox.empty()) break;
                auto it = inbox.begin();
                std::advance(it, (long)rnd(inbox.size()));
                const int64_t conn = it->first;
                auto& in = it->second;
                if (in.size() > 1 && rnd(10) == 0) {  // skips one answer
                    const mh::Msg& r = in[1];
                    const std::string p = mh::encode(2, nullptr, 0, 0, 0, hash_of(r.data, r.lower), r.lower);
                    CHECK(mh_server_read(v, conn, p.data(), p.size(), now) == MH_EREJECTED);
                    inbox.erase(it);
                    CHECK(mh_server_lost(v, conn, now) == MH_OK);  // the transport closes it
                    break;
                }
                for (size_t k = rnd(2) ? 1 : in.size(); k > 0 && !in.empty() && !g_fail; --k) {
                    const mh::Msg r = in.front();
                    in.pop_front();
                    const std::string p = mh::encode(2, nullptr, 0, 0, 0, hash_of(r.data, r.lower), r.lower);
                    CHECK(mh_server_read(v, conn, p.data(), p.size(), now) == MH_OK);
                    drain();
                }
            }
        }
        drain();
    }
    // one honest miner finishes the rest
    CHECK(mh_server_read(v, next_conn, join.data(), join.size(), 0) == MH_OK);
    inbox[next_conn];
    drain();
    for (int guard = 0; guard < 100000 && !g_fail; ++guard) {
        bool any = false;
        for (auto& kv : inbox)
            while (!kv.second.empty() && !g_fail) {
                const mh::Msg r = kv.second.front();
                kv.second.pop_front();
                const std::string p = mh::encode(2, nullptr, 0, 0, 0, hash_of(r.data, r.lower), r.lower);
                CHECK(mh_server_read(v, kv.first, p.data(), p.size(), 1) == MH_OK);
                any = true;
                drain();
            }
        if (!any) break;
    }
    for (auto& kv : expect) CHECK(answered[kv.first] == 1);
    mh_sched_stats st;
    CHECK(mh_server_stats(v, &st) == MH_OK && st.jobs == 0);
    mh_server_destroy(v);
}

static void bad_options() {
    mh_sched_queue_opts q;
    for (uint32_t d : {0u, (uint32_t)MH_SCHED_MAX_DEPTH + 1u, ~0u}) {
        q = mh_sched_queue_opts{d, 0, 0};
        CHECK(mh_sched_create_ex(nullptr, &q) == nullptr && mh_server_create_ex(nullptr, &q) == nullptr);
    }
    q = mh_sched_queue_opts{2, 1, 0};
    CHECK(mh_sched_create_ex(nullptr, &q) == nullptr && mh_server_create_ex(nullptr, &q) == nullptr);
    mh_sched* s = mh_sched_create_ex(nullptr, nullptr);
    CHECK(s != nullptr);
    CHECK(mh_sched_miner_queue(s, 3, nullptr, 4) == MH_EINVAL && mh_sched_miner_queue(nullptr, 3, nullptr, 4) == MH_EINVAL);
    mh_sched_destroy(s);
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 440;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    rng.seed(seed);
    bad_options();
    for (int i = 0; i < iters && !g_fail; ++i) {
        fuzz_sched_queue();
        fuzz_server_queue();
    }
    printf("fuzz_queue seed=%llu iters=%d failures=%d results=%llu rejected=%llu deepest=%llu\n",
           (unsigned long long)seed, iters, g_fail, (unsigned long long)g_results, (unsigned long long)g_rejected,
           (unsigned long long)g_deepest);
    return g_fail ? 1 : 0;
}
