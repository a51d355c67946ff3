// batch_plan_host.cpp -- the batch planner of libminehip (bitcoin-miner_amd/csrc/plan.cpp:
// plan_batch, build_batch_tables, batch_tables_ok) driven on the host, to be built with
// -fsanitize=address,undefined (tests/test_batch_plan.py).  No HIP.
//
//   batch_plan_host <seed> <batches>
//
// Per random batch and random slot capacity: every pass's tables pass batch_tables_ok; the walk
// batch_scan does over them (tile -> entry -> decades of that tile, the first and last decade cut
// to the entry's nonces) visits every nonce of every fused request exactly once, counted per
// request segment; and tables corrupted in one field are refused.
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

// Nonces the kernel's index arithmetic gives tile `tile` of the pass (search_kernels.hip batch_scan).
uint64_t tile_nonces(const mh::BatchTables& t, uint32_t tile) {
    const mh::BatchEntry& e = t.entries[t.tile_entry[tile]];
    const uint64_t first = e.g.first, lastn = e.g.first + (e.g.count - 1u);
    const uint64_t u_first = first / 10u, u_last = lastn / 10u;
    const uint32_t j_first = (uint32_t)(first % 10u), j_last = (uint32_t)(lastn % 10u);
    const uint64_t nd = u_last - u_first + 1u;
    const uint64_t base = (uint64_t)(tile - e.tile0) * mh::kBatchTileDecades;
    uint64_t n = 0;
    for (uint64_t off = base; off < base + mh::kBatchTileDecades && off < nd; ++off) {
        const uint64_t u = u_first + off;
        const uint32_t jlo = off == 0 ? j_first : 0u, jhi = u == u_last ? j_last : 9u;
        CHECK(jlo <= jhi);
        CHECK(u * 10u + jhi >= u * 10u);  // the last nonce of the decade does not wrap
        CHECK(u * 10u + jlo >= first && u * 10u + jhi <= lastn);
        n += jhi - jlo + 1u;
    }
    return n;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 440;
    const int batches = argc > 2 ? atoi(argv[2]) : 20;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    const mh::PlanOpts opt;
    uint64_t passes_seen = 0, fused_seen = 0, fallback_seen = 0;
    for (int b = 0; b < batches; ++b) {
        const size_t n = 1 + (size_t)below(300);
        std::vector<mh::BatchRequest> reqs(n);
        for (size_t i = 0; i < n; ++i) {
            std::vector<uint8_t> msg((size_t)below(131));
            for (auto& c : msg) c = (uint8_t)below(256);
            mh::absorb_prefix(msg.data(), msg.size(), &reqs[i].pre);
            const int d = 1 + (int)below(20);
            const uint64_t lo_b = d == 1 ? 0 : kP10[d - 1], hi_b = d == 20 ? ~0ull : kP10[d] - 1u;
            const uint64_t lo = below(8) == 0 ? hi_b - below(std::min<uint64_t>(hi_b - lo_b, 5000)) : lo_b + below(hi_b - lo_b);
            const uint64_t kind = below(4);
            const uint64_t span = kind == 0 ? 1 : kind == 1 ? 1 + below(3000) : kind == 2 ? 1 + below(40000) : 1 + below(3000000);
            reqs[i].lower = below(16) == 0 ? ~0ull - below(20000) : lo;
            reqs[i].upper = (~0ull - reqs[i].lower < span - 1u) ? ~0ull : reqs[i].lower + (span - 1u);
            reqs[i].id = 1000 + i;
        }
        const uint32_t caps[] = {1, 2, 8, 300, mh::kMaxBlocksPerLaunch};
        const uint32_t cap = caps[below(5)];
        std::vector<mh::BatchItem> items;
        mh::plan_batch(reqs.data(), n, opt, cap, &items);
        int passes = 0;
        std::vector<uint64_t> covered(n, 0);
        std::vector<int> seen(n, 0);
        for (const mh::BatchItem& it : items) {
            CHECK(it.idx < n && it.req == 1000 + it.idx);
            if (it.kind == 0) passes = std::max(passes, it.pass + 1);
            if (it.kind == 1) {
                ++fallback_seen;
                CHECK(!seen[it.idx]++);
            }
        }
        mh::BatchTables t;
        for (int p = 0; p < passes; ++p) {
            mh::build_batch_tables(reqs.data(), items, p, &t);
            CHECK(mh::batch_tables_ok(t, cap));
            if (!mh::batch_tables_ok(t, cap)) continue;
            ++passes_seen;
            for (size_t r = 0; r < t.req_idx.size(); ++r) {
                CHECK(!seen[t.req_idx[r]]++);
                ++fused_seen;
                for (uint32_t tile = t.seg[r]; tile < t.seg[r + 1]; ++tile) covered[t.req_idx[r]] += tile_nonces(t, tile);
            }
            // one field wrong: refused
            mh::BatchTables bad = t;
            switch (below(7)) {
                case 0: bad.tile_entry[below(bad.tile_entry.size())] = (uint32_t)bad.entries.size(); break;
                case 1: bad.entries[below(bad.entries.size())].tile0 += 1; break;
                case 2: bad.entries[below(bad.entries.size())].g.count = 0; break;
                case 3: bad.seg.back() += 1; break;
                case 4: bad.tile_entry.push_back(bad.tile_entry.back()); break;
                case 5: bad.entries[below(bad.entries.size())].g.count += 10u * mh::kBatchTileDecades; break;
                default: bad.seg[below(bad.seg.size() - 1)] += 1; break;
            }
            CHECK(!mh::batch_tables_ok(bad, cap));
            CHECK(!mh::batch_tables_ok(t, (uint32_t)t.tile_entry.size() - 1u));
        }
        for (size_t i = 0; i < n; ++i) {
            CHECK(seen[i] == 1);
            if (covered[i]) CHECK(covered[i] == reqs[i].upper - reqs[i].lower + 1u);
        }
    }
    printf("passes=%llu fused=%llu fallback=%llu failures=%d\n", (unsigned long long)passes_seen,
           (unsigned long long)fused_seen, (unsigned long long)fallback_seen, failures);
    return failures ? 1 : 0;
}
