// hits_batch_host.cpp -- the host schedule of mh_search_hits_batch (bitcoin-miner_amd/csrc/plan.cpp:
// plan_hits_batch_pass, hits_batch_tables_ok), driven on the host, to be built with
// -fsanitize=address,undefined (tests/test_hits_batch.py).  No HIP.
//
//   hits_batch_host <seed> <batches>
//
// Per random batch, random caps, random slot capacity of a pass and random size of the device hit
// buffer, pass after pass as the library runs them: the tables pass the check; every request's
// region has min(cap, its nonce count, slots left in the window) slots at the next free offset; the
// regions of a window are disjoint, in order and inside the buffer; a pass starts after a drain
// exactly when its tables or results do not fit or when its requests want more slots than the
// window has left and the window is not empty, so a drain never leaves a window empty that had
// room; every entry's request owns the entry's slots; corrupted tables are refused.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../bitcoin-miner_amd/csrc/plan.hpp"

namespace {

int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            ++failures;                                              \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
        }                                                            \
    } while (0)

constexpr uint64_t kP10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull,
                               100000000ull, 1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull,
                               10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                               100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};
constexpr uint64_t kMaxCap = 1u << 20;  // MH_HITS_MAX_CAP

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 440;
    const int batches = argc > 2 ? atoi(argv[2]) : 20;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    const mh::PlanOpts opt;
    uint64_t passes_seen = 0, drains_seen = 0, slot_drains = 0, cut_regions = 0;
    for (int b = 0; b < batches; ++b) {
        const size_t n = 1 + (size_t)below(300);
        std::vector<mh::BatchRequest> reqs(n);
        std::vector<uint64_t> caps(n);
        for (size_t i = 0; i < n; ++i) {
            std::vector<uint8_t> msg((size_t)below(131));
            for (auto& c : msg) c = (uint8_t)below(256);
            mh::absorb_prefix(msg.data(), msg.size(), &reqs[i].pre);
            const int d = 1 + (int)below(20);
            const uint64_t lo_b = d == 1 ? 0 : kP10[d - 1], hi_b = d == 20 ? ~0ull : kP10[d] - 1u;
            const uint64_t lo = below(8) == 0 ? hi_b - below(std::min<uint64_t>(hi_b - lo_b, 5000)) : lo_b + below(hi_b - lo_b);
            const uint64_t kind = below(4);
            const uint64_t span = kind == 0 ? 1 : kind == 1 ? 1 + below(3000) : kind == 2 ? 1 + below(40000) : 1 + below(2000000);
            reqs[i].lower = below(16) == 0 ? ~0ull - below(20000) : lo;
            reqs[i].upper = (~0ull - reqs[i].lower < span - 1u) ? ~0ull : reqs[i].lower + (span - 1u);
            reqs[i].id = i;
            const uint64_t ck = below(6);
            caps[i] = ck == 0 ? 0 : ck == 1 ? 1 : ck == 2 ? 4 : ck == 3 ? 4096 : ck == 4 ? 1 + below(100) : kMaxCap;
        }
        const uint32_t slot_caps[] = {2, 8, 300, mh::kMaxBlocksPerLaunch};
        const uint32_t slot_cap = slot_caps[below(4)];
        const uint64_t windows[] = {1, 8, 64, 5000, kMaxCap};
        const size_t tables[] = {4u << 20, 64u << 10};
        const size_t results[] = {1u << 16, 5};
        const mh::HitsBatchLimits lim{tables[below(2)], results[below(2)], windows[below(5)]};
        std::vector<mh::BatchItem> items;
        mh::plan_batch(reqs.data(), n, opt, slot_cap, &items);
        int passes = 0;
        for (const mh::BatchItem& it : items)
            if (it.kind == 0) passes = std::max(passes, it.pass + 1);
        mh::BatchTables t;
        mh::HitsBatchState st;
        std::vector<mh::HitsRegion> window;  // the regions handed out since the last drain
        for (int p = 0; p < passes; ++p) {
            mh::build_batch_tables(reqs.data(), items, p, &t);
            if (!mh::batch_tables_ok(t, slot_cap)) {
                CHECK(!"batch_tables_ok");
                continue;
            }
            ++passes_seen;
            const size_t nreq = t.req_idx.size();
            const size_t bytes = mh::hits_batch_table_bytes(t.entries.size(), nreq, t.tile_entry.size());
            uint64_t want = 0;
            for (size_t r = 0; r < nreq; ++r)
                want += std::min(caps[t.req_idx[r]], reqs[t.req_idx[r]].upper - reqs[t.req_idx[r]].lower + 1u);
            const mh::HitsBatchState before = st;
            mh::HitsBatchTables h;
            const bool drain = mh::plan_hits_batch_pass(t, reqs.data(), caps.data(), lim, &st, &h);
            const bool by_room = before.toff + bytes > lim.table_bytes || before.nres + nreq > lim.results;
            const bool by_slots = before.used != 0 && want > lim.window_slots - before.used;
            const bool in_flight = before.toff != 0 || before.nres != 0 || before.used != 0;
            CHECK(drain == (in_flight && (by_room || by_slots)));
            if (drain) {
                ++drains_seen;
                if (by_slots && !by_room) {
                    ++slot_drains;
                    CHECK(!window.empty() && before.used > 0);  // never a drain of an empty window
                }
                CHECK(st.window == before.window + 1);
                window.clear();
            } else {
                CHECK(st.window == before.window);
            }
            const uint64_t used_before = drain ? 0 : before.used;
            CHECK(mh::hits_batch_tables_ok(t, reqs.data(), h, used_before, lim.window_slots));
            CHECK(h.region.size() == nreq && h.entry_req.size() == t.entries.size());
            CHECK(st.toff == (drain ? 0 : before.toff) + bytes && st.nres == (drain ? 0 : before.nres) + nreq);
            uint64_t next = used_before;
            for (size_t r = 0; r < nreq && r < h.region.size(); ++r) {
                const mh::BatchRequest& q = reqs[t.req_idx[r]];
                const uint64_t size = q.upper - q.lower + 1u;  // a fused request: never 2^64
                const uint64_t left = lim.window_slots - next;
                const uint64_t rule = std::min(std::min(caps[t.req_idx[r]], size), left);
                CHECK(h.region[r].offset == next && h.region[r].slots == rule);
                CHECK(h.region[r].offset + h.region[r].slots <= lim.window_slots && lim.window_slots <= kMaxCap);
                if (rule < std::min(caps[t.req_idx[r]], size)) ++cut_regions;
                for (const mh::HitsRegion& g : window)  // disjoint from every region of the window so far
                    CHECK(g.offset + g.slots <= h.region[r].offset || g.slots == 0 || h.region[r].slots == 0);
                window.push_back(h.region[r]);
                next += h.region[r].slots;
            }
            CHECK(st.used == next);
            for (size_t ei = 0; ei < t.entries.size() && ei < h.entry_req.size(); ++ei) {
                const uint32_t r = h.entry_req[ei];
                CHECK(r < nreq && t.seg[r] <= t.entries[ei].slot0 && t.entries[ei].slot0 < t.seg[r + 1]);
            }
            // one field wrong: refused
            mh::HitsBatchTables bad = h;
            switch (below(6)) {
                case 0: bad.entry_req[below(bad.entry_req.size())] = (uint32_t)nreq; break;
                case 1: bad.region.pop_back(); break;
                case 2: bad.region.push_back(mh::HitsRegion{0, 0}); break;
                case 3: bad.region[below(nreq)].offset = lim.window_slots + 1u; break;
                case 4: bad.region[below(nreq)].slots = lim.window_slots + 1u; break;
                default: bad.entry_req.push_back(0); break;
            }
            CHECK(!mh::hits_batch_tables_ok(t, reqs.data(), bad, used_before, lim.window_slots));
            if (nreq > 1) {  // an entry handed to a neighbouring request
                bad = h;
                bad.entry_req[0] = 1;
                CHECK(!mh::hits_batch_tables_ok(t, reqs.data(), bad, used_before, lim.window_slots));
                if (h.region[0].slots > 0) {  // two regions that overlap
                    bad = h;
                    bad.region[1].offset = h.region[0].offset;
                    CHECK(!mh::hits_batch_tables_ok(t, reqs.data(), bad, used_before, lim.window_slots));
                }
            }
            if (used_before > 0 && h.region[0].slots > 0) {  // a region inside an earlier pass's of the window
                bad = h;
                bad.region[0].offset = used_before - 1u;
                CHECK(!mh::hits_batch_tables_ok(t, reqs.data(), bad, used_before, lim.window_slots));
            }
            {  // a region larger than its request
                bad = h;
                const size_t r = (size_t)below(nreq);
                bad.region[r].slots = reqs[t.req_idx[r]].upper - reqs[t.req_idx[r]].lower + 2u;
                CHECK(!mh::hits_batch_tables_ok(t, reqs.data(), bad, used_before, lim.window_slots));
            }
        }
    }
    CHECK(drains_seen > 0 && slot_drains > 0 && cut_regions > 0);  // the run did visit these paths
    printf("passes=%llu drains=%llu slot_drains=%llu cut=%llu failures=%d\n", (unsigned long long)passes_seen,
           (unsigned long long)drains_seen, (unsigned long long)slot_drains, (unsigned long long)cut_regions, failures);
    return failures ? 1 : 0;
}
