// sched.hpp -- the bitcoin server's chunk scheduler (SURVEY.md §8(f) N2;
// reference stub bitcoin/server/server.go:62).  Host-only C++, no HIP: used by
// the mh_sched_* / mh_server_* C-ABI (include/minehip_server.h) and by
// mh_search_multi, whose per-device worker threads are its miners.
//
// A job is a client's Request range [lower, upper] (message.go:27-34).  It is
// cut into chunks on demand, sized from the miner's measured rate and the work
// left (guided self-scheduling), and merged by the lexicographic min of
// (hash, nonce) -- associative and commutative, so the answer does not depend
// on chunking, order or reassignment (tests/test_sched.py checks exactly that
// against the oracle).
//
// A miner holds a FIFO of outstanding chunks: one by default, up to
// mh_sched_queue_opts.depth after set_queue, while the nonces it holds stay
// under rate x queue_ns -- so the small Requests of many clients stack up on a
// miner and run there as one batch, and a large job's chunk (rate x target_ns)
// fills the budget alone.  A Result carries no id and completes the oldest
// chunk; with depth > 1 it is checked against the host Hash given to
// set_queue, and a miner that fails the check is removed (its later Results
// would be credited to the wrong chunks).
//
// A target job (submit_first) asks the proof-of-work question instead: the smallest nonce whose
// hash is <= target.  Its chunks go out in ascending order, a Result with hash <= target is a hit,
// nothing above the smallest known hit b is handed out, and the job is done once no chunk below b
// is pending or out; chunks still out above b drain as a cancelled job's do (minehip_server.h has
// the rules, DESIGN.md §7 the argument).  A job from submit() takes none of these paths.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/minehip_server.h"

namespace mh {

class Scheduler {
  public:
    // opts must be valid (see valid_opts)
    explicit Scheduler(const mh_sched_opts& opts);

    static bool valid_opts(const mh_sched_opts& o);
    static bool valid_queue_opts(const mh_sched_queue_opts& q);

    // Hash(msg, nonce) on the host (plan.hpp host_hash; passed in, so that this file needs no
    // SHA-256 of its own)
    using HostHash = uint64_t (*)(const uint8_t* msg, size_t len, uint64_t nonce);
    // Before the first miner joins: q must be valid; hash may be NULL only for depth 1.
    void set_queue(const mh_sched_queue_opts& q, HostHash hash);

    int add_miner(int64_t id);
    int remove_miner(int64_t id);
    int64_t submit(int64_t client, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper);
    int64_t submit_first(int64_t client, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                         uint64_t target);
    int job_target(int64_t job, bool* has_target, uint64_t* target);
    int drop_client(int64_t client);
    int next(int64_t miner, uint64_t now_ns, mh_assignment* out);
    int job_msg(int64_t job, std::string* out);
    // the chunks `miner` holds, oldest first
    int miner_queue(int64_t miner, std::vector<mh_assignment>* out);
    int result(int64_t miner, uint64_t hash, uint64_t nonce, uint64_t now_ns, mh_completion* out);
    void stats(mh_sched_stats* out);
    void first_stats(mh_sched_first_stats* out);
    // true when no live job is left (all done or cancelled and drained)
    bool idle_jobs();

  private:
    using u128 = unsigned __int128;
    struct Job {
        int64_t id, client;
        std::string msg;
        uint64_t lower, upper;
        uint64_t next;       // first nonce never handed out
        bool exhausted;      // every nonce handed out at least once
        std::deque<std::pair<uint64_t, uint64_t>> requeue;  // chunks of lost miners
        uint64_t outstanding;
        uint64_t best_hash, best_nonce;
        bool cancelled;
        // a target job: first; hit once some Result had hash <= target, (hit_hash, hit_nonce) the one
        // with the smallest nonce; finished: completed while chunks above the hit are still out
        bool first, hit, finished;
        uint64_t target, hit_hash, hit_nonce;
        u128 pending() const;  // nonces not handed out (fresh + requeued)
    };
    struct Chunk {
        int64_t job;
        uint64_t lo, hi;
    };
    struct Miner {
        int64_t id;
        std::deque<Chunk> q;  // chunks out, oldest first
        u128 held;            // their nonces
        uint64_t t_busy;      // the later of: q became non-empty, the last Result
        double acc_nonces;    // completed since the last rate sample
        uint64_t acc_ns;      // and the busy time that took
        double rate;          // nonces per ns, EWMA; 0 before the first sample
    };

    Job* find_job(int64_t id);
    Miner* find_miner(int64_t id);
    void erase_job(int64_t id);
    uint64_t chunk_size(const Miner& m, const Job& j) const;
    bool take(Job& j, uint64_t c, uint64_t* lo, uint64_t* hi);
    bool eligible(const Miner& m) const;
    void requeue_chunk(const Chunk& c);
    int64_t submit_job(int64_t client, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, bool first,
                       uint64_t target);
    void prune_above_hit(Job& j);
    bool out_below_hit(const Job& j) const;
    void drop_miner(size_t i);

    std::mutex mu_;
    mh_sched_opts o_;
    mh_sched_queue_opts q_{1, 0, 0};
    HostHash hash_ = nullptr;
    std::vector<std::unique_ptr<Job>> jobs_;  // submission order
    std::vector<Miner> miners_;               // join order
    size_t rr_ = 0;                           // round-robin cursor into jobs_
    int64_t next_job_ = 0;
    mh_sched_stats st_{};
    mh_sched_first_stats fst_{};
};

}  // namespace mh

struct mh_sched {
    mh::Scheduler s;
    explicit mh_sched(const mh_sched_opts& o) : s(o) {}
};
