// server.cpp -- the bitcoin server's message loop (reference stub
// bitcoin/server/server.go:62) over the Scheduler, as the
// mh_server_* C-ABI (include/minehip_server.h).
//
// Transport-agnostic: the Go server keeps its lsp.Server (server.go:12-14)
// and, for every Read, calls mh_server_read (payload) or mh_server_lost
// (error), then drains mh_server_pop_write into lsp.Server.Write.  Payloads
// are Go encoding/json bitcoin.Messages (msgcodec.hpp):
//   Join (message.go:47)     -> the connection becomes a miner;
//   Request (message.go:27)  -> a job for the connection (a client);
//   Result (message.go:38)   -> the miner's chunk is done;
// and every idle miner is handed a chunk as a Request carrying the job's
// Data.  A finished job writes NewResult(hash, nonce) to its client.  A Request
// with a Target is a target job: its chunks carry the Target, its Result is plain.
#include <string.h>

#include <deque>
#include <set>
#include <string>
#include <utility>

#include "../../include/minehip.h"
#include "msgcodec.hpp"
#include "plan.hpp"
#include "sched.hpp"

struct mh_server {
    std::mutex mu;  // serialises read/lost/pop (the scheduler locks itself too)
    mh::Scheduler s;
    std::set<int64_t> miners;
    std::deque<std::pair<int64_t, std::string>> out;
    explicit mh_server(const mh_sched_opts& o) : s(o) {}

    // hand out chunks until no miner may take another
    int dispatch(uint64_t now) {
        mh_assignment a;
        for (;;) {
            const int r = s.next(-1, now, &a);
            if (r < 0) return r;
            if (r == 0) return MH_OK;
            std::string m;
            const int rc = s.job_msg(a.job, &m);
            if (rc) return rc;
            bool has_target = false;
            uint64_t target = 0;
            const int tc = s.job_target(a.job, &has_target, &target);
            if (tc) return tc;
            out.emplace_back(a.miner, mh::encode(1, (const uint8_t*)m.data(), m.size(), a.lower, a.upper, 0, 0,
                                                 has_target, target));
        }
    }
};

namespace {

// The options of the _ex constructors: NULL = defaults; false (MH_EINVAL) when either is bad.
bool resolve_opts(const mh_sched_opts* opts, const mh_sched_queue_opts* q, mh_sched_opts* o, mh_sched_queue_opts* qo) {
    mh_sched_default_opts(o);
    mh_sched_default_queue_opts(qo);
    if (opts) *o = *opts;
    if (q) *qo = *q;
    if (!mh::Scheduler::valid_opts(*o)) {
        mh::set_error(MH_EINVAL, "bad scheduler options");
        return false;
    }
    if (!mh::Scheduler::valid_queue_opts(*qo)) {
        mh::set_error(MH_EINVAL, "bad queue options: depth must be 1..MH_SCHED_MAX_DEPTH, reserved 0");
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

// Here and not in sched.cpp: the queueing scheduler checks Results with plan.cpp's host Hash, and
// sched.cpp alone stays free of that dependency.
mh_sched* mh_sched_create_ex(const mh_sched_opts* opts, const mh_sched_queue_opts* q) {
    mh_sched_opts o;
    mh_sched_queue_opts qo;
    if (!resolve_opts(opts, q, &o, &qo)) return nullptr;
    mh_sched* s = new mh_sched(o);
    s->s.set_queue(qo, &mh::host_hash);
    return s;
}

mh_server* mh_server_create(const mh_sched_opts* opts) { return mh_server_create_ex(opts, nullptr); }

mh_server* mh_server_create_ex(const mh_sched_opts* opts, const mh_sched_queue_opts* q) {
    mh_sched_opts o;
    mh_sched_queue_opts qo;
    if (!resolve_opts(opts, q, &o, &qo)) return nullptr;
    mh_server* v = new mh_server(o);
    v->s.set_queue(qo, &mh::host_hash);
    return v;
}

void mh_server_destroy(mh_server* v) { delete v; }

int mh_server_read(mh_server* v, int64_t conn, const char* payload, size_t len, uint64_t now_ns) {
    if (!v || (!payload && len)) return mh::set_error(MH_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(v->mu);
    mh::Msg m;
    if (!mh::decode(payload ? payload : "", len, &m))
        return mh::set_error(MH_EINVAL, "payload is not a JSON bitcoin.Message");
    int rc = MH_OK;
    switch (m.type) {
        case 0:  // Join
            rc = v->s.add_miner(conn);
            if (rc == MH_OK) v->miners.insert(conn);
            break;
        case 1: {  // Request from a client
            const uint8_t* d = (const uint8_t*)m.data.data();
            const int64_t id = m.has_target ? v->s.submit_first(conn, d, m.data.size(), m.lower, m.upper, m.target)
                                            : v->s.submit(conn, d, m.data.size(), m.lower, m.upper);
            if (id < 0)  // nothing will ever answer it: the transport closes the client (Disconnected)
                rc = mh::set_error(MH_EREJECTED, id == MH_ERANGE ? "Request refused: Lower > Upper"
                                                                 : "Request refused: Data too long");
            break;
        }
        case 2: {  // Result from a miner
            mh_completion c;
            const int r = v->s.result(conn, m.hash, m.nonce, now_ns, &c);
            if (r < 0) {
                rc = r;
                if (r == MH_EREJECTED) v->miners.erase(conn);  // the scheduler removed it as lost
            } else if (r == 1) {
                v->out.emplace_back(c.client, mh::encode(2, nullptr, 0, 0, 0, c.hash, c.nonce));
            }
            break;
        }
        default:
            rc = mh::set_error(MH_EINVAL, "unknown message type");
    }
    // a rejected Result requeued its chunk(s): hand the work out again either way
    const int d = v->dispatch(now_ns);
    return rc ? rc : d;
}

int mh_server_lost(mh_server* v, int64_t conn, uint64_t now_ns) {
    if (!v) return mh::set_error(MH_EINVAL, "NULL server");
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->miners.erase(conn)) {
        const int rc = v->s.remove_miner(conn);
        if (rc) return rc;
    } else {
        v->s.drop_client(conn);
        // writes still queued for a lost client are dropped
        for (auto it = v->out.begin(); it != v->out.end();)
            it = (it->first == conn) ? v->out.erase(it) : it + 1;
    }
    return v->dispatch(now_ns);
}

int mh_server_pop_write(mh_server* v, int64_t* conn, char* out, size_t cap, size_t* len) {
    if (!v || !conn) return mh::set_error(MH_EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->out.empty()) return 0;
    const auto& w = v->out.front();
    if (len) *len = w.second.size();
    if (!out || cap < w.second.size()) return mh::set_error(MH_EINVAL, "output buffer too small");
    *conn = w.first;
    memcpy(out, w.second.data(), w.second.size());
    v->out.pop_front();
    return 1;
}

int mh_server_stats(mh_server* v, mh_sched_stats* out) {
    if (!v || !out) return mh::set_error(MH_EINVAL, "bad arguments");
    v->s.stats(out);
    return MH_OK;
}

int mh_server_first_stats(mh_server* v, mh_sched_first_stats* out) {
    if (!v || !out) return mh::set_error(MH_EINVAL, "bad arguments");
    v->s.first_stats(out);
    return MH_OK;
}

}  // extern "C"
