// first_batch_host.cpp -- the host tables of mh_search_first_batch (bitcoin-miner_amd/csrc/plan.cpp:
// build_first_batch_tables, first_batch_tables_ok) and the per-tile arithmetic of batch_scan_first,
// driven on the host, to be built with -fsanitize=address,undefined (tests/test_first_batch.py).
// No HIP.
//
//   first_batch_host <seed> <batches>
//
// Per random batch and random slot capacity, for every pass and both orders: the tables pass the
// check; the order is a permutation, rank-major where asked (ranks never decrease, requests in
// order within a rank); every entry's request owns the entry's slots; the nonce count the kernel
// adds to `scanned` for a tile (n_hi - n_lo + 1, formed without first + count or 10u + 9 at the
// last decade) equals a walk over the tile's decades, its floor n_lo is the tile's smallest
// nonce, and a request's tiles sum to its size; corrupted tables are refused.
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

// What batch_scan_first computes for tile `tile` (search_kernels.hip), against a walk over its decades.
uint64_t tile_count(const mh::BatchTables& t, uint32_t tile) {
    const mh::BatchEntry& e = t.entries[t.tile_entry[tile]];
    const uint64_t first = e.g.first, lastn = e.g.first + (e.g.count - 1u);
    const uint64_t u_first = first / 10u, u_last = lastn / 10u;
    const uint64_t nd = u_last - u_first + 1u;
    const uint64_t base = (uint64_t)(tile - e.tile0) * mh::kBatchTileDecades;
    CHECK(base < nd);
    const uint64_t d_lo = u_first + base;
    const uint64_t d_hi = nd - base > (uint64_t)mh::kBatchTileDecades ? d_lo + (mh::kBatchTileDecades - 1u) : u_last;
    const uint64_t n_lo = base == 0u ? first : d_lo * 10u;
    CHECK(d_hi == u_last || d_hi <= (~0ull - 9u) / 10u);  // d_hi * 10 + 9 does not wrap
    const uint64_t n_hi = d_hi == u_last ? lastn : d_hi * 10u + 9u;
    CHECK(n_lo == std::max(first, (u_first + base) * 10u));  // the floor as DESIGN.md states it
    CHECK(n_lo >= first && n_hi <= lastn && n_lo <= n_hi);
    uint64_t walk = 0, smallest = ~0ull;
    for (uint64_t off = base; off < base + mh::kBatchTileDecades && off < nd; ++off) {
        const uint64_t u = u_first + off;
        const uint32_t jlo = off == 0 ? (uint32_t)(first % 10u) : 0u, jhi = u == u_last ? (uint32_t)(lastn % 10u) : 9u;
        walk += jhi - jlo + 1u;
        smallest = std::min(smallest, u * 10u + jlo);
    }
    CHECK(walk == n_hi - n_lo + 1u && smallest == n_lo);
    return n_hi - n_lo + 1u;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 440;
    const int batches = argc > 2 ? atoi(argv[2]) : 20;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    const mh::PlanOpts opt;
    uint64_t passes_seen = 0, tiles_seen = 0;
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
            const uint64_t span = kind == 0 ? 1 : kind == 1 ? 1 + below(3000) : kind == 2 ? 1 + below(40000) : 1 + below(2000000);
            reqs[i].lower = below(16) == 0 ? ~0ull - below(20000) : lo;
            reqs[i].upper = (~0ull - reqs[i].lower < span - 1u) ? ~0ull : reqs[i].lower + (span - 1u);
            reqs[i].id = i;
        }
        const uint32_t caps[] = {2, 8, 300, mh::kMaxBlocksPerLaunch};
        const uint32_t cap = caps[below(4)];
        std::vector<mh::BatchItem> items;
        mh::plan_batch(reqs.data(), n, opt, cap, &items);
        int passes = 0;
        for (const mh::BatchItem& it : items)
            if (it.kind == 0) passes = std::max(passes, it.pass + 1);
        mh::BatchTables t;
        for (int p = 0; p < passes; ++p) {
            mh::build_batch_tables(reqs.data(), items, p, &t);
            if (!mh::batch_tables_ok(t, cap)) {
                CHECK(!"batch_tables_ok");
                continue;
            }
            ++passes_seen;
            const size_t tiles = t.tile_entry.size(), nreq = t.req_idx.size();
            tiles_seen += tiles;
            for (size_t r = 0; r < nreq; ++r) {
                uint64_t sum = 0;
                for (uint32_t tile = t.seg[r]; tile < t.seg[r + 1]; ++tile) sum += tile_count(t, tile);
                CHECK(sum == reqs[t.req_idx[r]].upper - reqs[t.req_idx[r]].lower + 1u);
            }
            for (int rank_major = 0; rank_major < 2; ++rank_major) {
                mh::FirstBatchTables f;
                mh::build_first_batch_tables(t, rank_major != 0, &f);
                CHECK(mh::first_batch_tables_ok(t, f));
                CHECK(f.order.size() == tiles && f.entry_req.size() == t.entries.size());
                for (size_t ei = 0; ei < t.entries.size(); ++ei) {
                    const uint32_t r = f.entry_req[ei];
                    CHECK(r < nreq && t.seg[r] <= t.entries[ei].slot0 && t.entries[ei].slot0 < t.seg[r + 1]);
                }
                std::vector<uint32_t> req_of(tiles);
                for (size_t r = 0; r < nreq; ++r)
                    for (uint32_t s = t.seg[r]; s < t.seg[r + 1]; ++s) req_of[s] = (uint32_t)r;
                uint32_t prev_rank = 0, prev_req = 0;
                for (size_t i = 0; i < f.order.size() && f.order[i] < tiles; ++i) {
                    const uint32_t s = f.order[i], r = req_of[s], rank = s - t.seg[r];
                    if (!rank_major) {
                        CHECK(s == i);
                        continue;
                    }
                    if (i) CHECK(rank > prev_rank || (rank == prev_rank && r > prev_req));
                    prev_rank = rank;
                    prev_req = r;
                }
                // one field wrong: refused
                mh::FirstBatchTables bad = f;
                switch (below(5)) {
                    case 0: bad.order[below(tiles)] = (uint32_t)tiles; break;
                    case 1: bad.order.pop_back(); break;
                    case 2: bad.order.push_back(0); break;
                    case 3: bad.entry_req[below(bad.entry_req.size())] = (uint32_t)nreq; break;
                    default:
                        if (tiles > 1) bad.order[0] = bad.order[1];  // a repeat
                        else bad.entry_req.push_back(0);
                        break;
                }
                CHECK(!mh::first_batch_tables_ok(t, bad));
                if (nreq > 1) {  // an entry handed to a neighbouring request
                    bad = f;
                    bad.entry_req[0] = 1;
                    CHECK(!mh::first_batch_tables_ok(t, bad));
                }
            }
        }
    }
    printf("passes=%llu tiles=%llu failures=%d\n", (unsigned long long)passes_seen, (unsigned long long)tiles_seen,
           failures);
    return failures ? 1 : 0;
}
