// first_batch_fast_host.cpp -- the host tables of mh_search_first_batch_ex(MH_BATCH_FUSE_FAST)
// (bitcoin-miner_amd/csrc/plan.cpp: build_first_batch_tables_ex, first_batch_tables_ex_ok,
// chunk_floor_host, first_batch_order_slot) and the per-chunk arithmetic of batch_first, driven on
// the host, to be built with -fsanitize=address,undefined (tests/test_first_batch_fast_host.py).
// No HIP.
//
//   first_batch_fast_host <seed> <batches>
//
// Over the shapes of the GPU tests under the plans they use, and over random request lists at
// random slot capacities, for every pass and both orders: the tables pass the check; every slot
// has exactly one writer; every entry's and every item's request owns its slots; the nonce counts
// batch_scan_first_slots and batch_first add to `scanned` sum to the request's size, at the top of
// u64 as well; per chunk the host form of chunk_floor equals the smallest nonce of the chunk by
// enumeration (the last-digit and the Early layouts), and every enumerated nonce lies inside the
// piece; the orders are permutations, rank-major where asked; corrupted tables are refused.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
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

// x with w zero decimal digits inserted at digit index k (layout.hpp), by powers of ten
uint64_t insert_zeros(uint64_t x, uint32_t k, uint32_t w) {
    if (k >= 20u) return x;
    return x / kP10[k] * kP10[k] * kP10[w] + x % kP10[k];
}

// nonce(U, g, i) of a fast piece as layout.hpp documents it
uint64_t lane_nonce(const mh::FastArgs& a, uint64_t U, uint32_t g, uint32_t i) {
    if (a.mode < mh::kModeOneEarly) return U * a.pow10L + (uint64_t)g * 10u + i;
    return insert_zeros(U, a.hole, a.hole_w) * a.u_mul + insert_zeros(g, a.g_hole, 1u) * a.g_mul + i * a.i_mul;
}

// The nonces batch_scan_first_slots adds to `scanned` for tile `tile` (search_kernels.hip).
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
    const uint64_t n_hi = d_hi == u_last ? lastn : d_hi * 10u + 9u;
    CHECK(n_lo >= first && n_hi <= lastn && n_lo <= n_hi);
    return n_hi - n_lo + 1u;
}

// The nonces batch_first adds to `scanned` for chunk blk of an item (fast_search.hip).
uint64_t chunk_count(const mh::FastArgs& a, uint32_t blk) {
    const uint32_t left = a.n_runs - blk * (uint32_t)mh::kBlockThreads;
    const uint32_t lanes = left < (uint32_t)mh::kBlockThreads ? left : (uint32_t)mh::kBlockThreads;
    return (uint64_t)lanes * a.n_groups * 10ull;
}

// chunk_floor_host against the chunk's nonces, all of them
void check_chunk_floor(const mh::FastArgs& a, uint32_t blk, uint64_t first, uint64_t count) {
    const uint32_t left = a.n_runs - blk * (uint32_t)mh::kBlockThreads;
    const uint32_t lanes = std::min<uint32_t>(left, mh::kBlockThreads);
    uint64_t smallest = ~0ull;
    bool inside = true;
    for (uint32_t l = 0; l < lanes; ++l) {
        const uint64_t U = a.u_start + (uint64_t)blk * mh::kBlockThreads + l;
        for (uint32_t g = 0; g < a.n_groups; ++g)
            for (uint32_t i = 0; i < 10u; ++i) {
                const uint64_t n = lane_nonce(a, U, g, i);
                smallest = std::min(smallest, n);
                inside = inside && n >= first && n - first < count;
            }
    }
    CHECK(inside);
    CHECK(mh::chunk_floor_host(a, blk) == smallest);
}

struct Stats {
    uint64_t passes = 0, slots = 0, items = 0, early_chunks = 0, last_chunks = 0, fallbacks = 0;
};

void check_batch(const std::vector<mh::BatchRequest>& reqs, const mh::PlanOpts& opt, uint32_t cap, bool all_chunks,
                 std::mt19937_64& rng, Stats* st) {
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(reqs.data(), reqs.size(), opt, cap, false, mh::kBatchFastMaxNonces, &pieces, &args);
    int passes = 0;
    for (const mh::BatchPiece& p : pieces) {
        if (p.kind != 1) passes = std::max(passes, p.pass + 1);
        else ++st->fallbacks;
    }
    mh::BatchTables t;
    mh::BatchFastTables f;
    for (int p = 0; p < passes; ++p) {
        mh::build_batch_tables_ex(reqs.data(), pieces, args, p, &t, &f);
        const size_t tiles = t.tile_entry.size(), chunks = f.chunk_item.size(), nreq = t.req_idx.size();
        const size_t slots = tiles + chunks;
        ++st->passes;
        st->slots += slots;
        st->items += f.items.size();
        for (int rank_major = 0; rank_major < 2; ++rank_major) {
            mh::FirstBatchFastTables x;
            mh::build_first_batch_tables_ex(t, f, rank_major != 0, &x);
            if (!mh::first_batch_tables_ex_ok(t, f, x, cap)) {
                CHECK(!"first_batch_tables_ex_ok");
                continue;
            }
            CHECK(x.entry_req.size() == t.entries.size() && x.item_req.size() == f.items.size());
            CHECK(x.tile_order.size() == tiles && x.chunk_order.size() == chunks);
            // every slot has exactly one writer, found through the order tables as the kernels find it,
            // and that writer's request owns the slot
            std::vector<uint32_t> writers(slots, 0);
            std::vector<uint32_t> req_of(slots, 0);
            for (size_t r = 0; r < nreq; ++r)
                for (uint32_t s = t.seg[r]; s < t.seg[r + 1] && s < slots; ++s) req_of[s] = (uint32_t)r;
            std::vector<uint64_t> sum(nreq, 0);
            for (size_t b = 0; b < tiles; ++b) {
                const uint32_t tile = x.tile_order[b];
                const uint32_t ei = t.tile_entry[tile];
                const uint32_t slot = mh::first_batch_order_slot(t, f, -1, tile);
                CHECK(slot == t.entries[ei].slot0 + (tile - t.entries[ei].tile0) && slot < slots);
                if (slot >= slots) continue;
                ++writers[slot];
                CHECK(req_of[slot] == x.entry_req[ei]);
                sum[x.entry_req[ei]] += tile_count(t, tile);
            }
            for (size_t li = 0; li < f.launches.size(); ++li) {
                const mh::BatchFastLaunch& l = f.launches[li];
                uint32_t prev_rank = 0, prev_item = 0;
                for (uint32_t b = 0; b < l.chunks; ++b) {
                    const uint32_t c = x.chunk_order[l.chunk0 + b];
                    const uint32_t ii = f.chunk_item[l.chunk0 + c];
                    const mh::BatchFastItem& it = f.items[ii];
                    const uint32_t blk = c - it.chunk0;
                    CHECK(c >= it.chunk0 && blk < it.args.n_chunks);
                    const uint32_t slot = mh::first_batch_order_slot(t, f, (int)li, c);
                    CHECK(slot == it.slot0 + blk && slot < slots);
                    if (slot >= slots) continue;
                    ++writers[slot];
                    CHECK(req_of[slot] == x.item_req[ii]);
                    sum[x.item_req[ii]] += chunk_count(it.args, blk);
                    if (!rank_major) {
                        CHECK(c == b);
                    } else {
                        if (b) CHECK(blk > prev_rank || (blk == prev_rank && ii > prev_item));
                        prev_rank = blk;
                        prev_item = ii;
                    }
                }
            }
            for (size_t s = 0; s < slots; ++s) CHECK(writers[s] == 1);
            for (size_t r = 0; r < nreq; ++r)
                CHECK(sum[r] == reqs[t.req_idx[r]].upper - reqs[t.req_idx[r]].lower + 1u);
            if (rank_major) {  // generic launch: a request's tiles in order, ranks never decrease
                std::vector<uint32_t> seen(nreq, 0);
                uint32_t prev = 0;
                for (size_t b = 0; b < tiles; ++b) {
                    const uint32_t r = x.entry_req[t.tile_entry[x.tile_order[b]]];
                    if (b) CHECK(seen[r] >= prev);
                    prev = seen[r]++;
                }
            } else {
                for (size_t b = 0; b < tiles; ++b) CHECK(x.tile_order[b] == b);
            }
            if (rank_major) continue;
            // chunk_floor, once per pass: every chunk, or the first, the last and a few others of every item
            for (size_t k = 0; k < f.items.size(); ++k) {
                const mh::FastArgs& a = f.items[k].args;
                const mh::BatchPiece& pc = pieces[f.piece[k]];
                CHECK(a.n_chunks == pc.slots && f.items[k].slot0 == pc.slot);
                std::vector<uint32_t> pick;
                if (all_chunks) {
                    for (uint32_t blk = 0; blk < a.n_chunks; ++blk) pick.push_back(blk);
                } else {
                    pick = {0u, a.n_chunks - 1u, (uint32_t)below(a.n_chunks), (uint32_t)below(a.n_chunks)};
                }
                for (const uint32_t blk : pick) {
                    check_chunk_floor(a, blk, pc.first, pc.count);
                    ++(a.mode >= mh::kModeOneEarly ? st->early_chunks : st->last_chunks);
                }
            }
            // corrupted tables are refused: a duplicate slot, an item or entry of another request, an
            // order that is no permutation
            if (!f.items.empty()) {
                mh::BatchFastTables fb = f;
                const size_t k = below(fb.items.size());
                fb.items[k].slot0 = fb.items[k].slot0 ? fb.items[k].slot0 - 1u : 1u;  // overlaps a neighbour's slot
                CHECK(!mh::first_batch_tables_ex_ok(t, fb, x, cap));
                if (nreq > 1) {
                    mh::FirstBatchFastTables xb = x;
                    xb.item_req[k] = (xb.item_req[k] + 1u) % (uint32_t)nreq;
                    CHECK(!mh::first_batch_tables_ex_ok(t, f, xb, cap));
                }
                mh::FirstBatchFastTables xb = x;
                xb.item_req.pop_back();
                CHECK(!mh::first_batch_tables_ex_ok(t, f, xb, cap));
                const mh::BatchFastLaunch& l = f.launches[below(f.launches.size())];
                xb = x;
                if (l.chunks > 1) xb.chunk_order[l.chunk0] = xb.chunk_order[l.chunk0 + 1];  // a repeat
                else xb.chunk_order[l.chunk0] = 1u;                                          // out of the launch
                CHECK(!mh::first_batch_tables_ex_ok(t, f, xb, cap));
                xb = x;
                xb.chunk_order.push_back(0u);
                CHECK(!mh::first_batch_tables_ex_ok(t, f, xb, cap));
            }
            if (tiles) {
                mh::FirstBatchFastTables xb = x;
                if (tiles > 1) xb.tile_order[0] = xb.tile_order[1];
                else xb.tile_order[0] = 1u;
                CHECK(!mh::first_batch_tables_ex_ok(t, f, xb, cap));
                if (nreq > 1) {
                    xb = x;
                    xb.entry_req[0] = (xb.entry_req[0] + 1u) % (uint32_t)nreq;
                    CHECK(!mh::first_batch_tables_ex_ok(t, f, xb, cap));
                }
                mh::BatchTables tb = t;
                tb.entries[below(tb.entries.size())].slot0 += 1u;  // past its own slots: a duplicate or a hole
                CHECK(!mh::first_batch_tables_ex_ok(tb, f, x, cap));
            }
        }
    }
}

mh::BatchRequest request(const std::string& msg, uint64_t lo, uint64_t hi, size_t id) {
    mh::BatchRequest r;
    mh::absorb_prefix((const uint8_t*)msg.data(), msg.size(), &r.pre);
    r.lower = lo;
    r.upper = hi;
    r.id = id;
    return r;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 440;
    const int batches = argc > 2 ? atoi(argv[2]) : 10;
    std::mt19937_64 rng(seed);
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    Stats st;

    // the shapes of tests/test_gpu_first_batch_fast.py, under the plans it uses
    const uint64_t top = ~0ull;
    std::vector<mh::BatchRequest> shapes;
    const struct {
        std::string msg;
        uint64_t lo, hi;
    } kShapes[] = {{"cmu441", 1048000, 2200000},  {"cmu474", 0, 3000000},      {"cmu440", 0, 3000000},
                   {"cmu440", 1048000, 2200000},  {std::string(51, 'a'), 0, 3000000}, {std::string(60, 'a'), 0, 3000000},
                   {std::string(47, 'a'), 900000, 3000000}, {"cmu440", 500000000, 503000000},
                   {"cmu440", top - 3000000, top}, {"cmu440", 0, 199999},     {"x", 5, 5},  {"", 0, 1000}};
    for (const auto& s : kShapes) shapes.push_back(request(s.msg, s.lo, s.hi, shapes.size()));
    mh::PlanOpts dflt, l3, l2, no_early;
    l3.lower_digits = 3;
    l3.min_lanes = 16;
    l2.lower_digits = 2;
    l2.min_lanes = 16;
    no_early.early = 0;
    check_batch(shapes, dflt, mh::kMaxBlocksPerLaunch, true, rng, &st);
    CHECK(st.early_chunks > 0 && st.last_chunks > 0 && st.fallbacks == 0);
    check_batch(shapes, l3, mh::kMaxBlocksPerLaunch, true, rng, &st);
    check_batch(shapes, l2, mh::kMaxBlocksPerLaunch, true, rng, &st);
    check_batch(shapes, no_early, mh::kMaxBlocksPerLaunch, false, rng, &st);
    check_batch(shapes, dflt, 1000, false, rng, &st);
    CHECK(st.fallbacks > 0);

    // a seeded fuzz of request lists: small generic requests beside ones of a few 10^6 nonces, which
    // plan fast pieces, in every decimal length, the top of u64 included
    for (int b = 0; b < batches; ++b) {
        const size_t n = 1 + (size_t)below(24);
        std::vector<mh::BatchRequest> reqs;
        for (size_t i = 0; i < n; ++i) {
            std::string msg((size_t)below(131), 'a');
            for (auto& c : msg) c = (char)below(256);
            const int d = 1 + (int)below(20);
            const uint64_t lo_b = d == 1 ? 0 : kP10[d - 1], hi_b = d == 20 ? top : kP10[d] - 1u;
            uint64_t lo = below(8) == 0 ? hi_b - below(std::min<uint64_t>(hi_b - lo_b, 5000)) : lo_b + below(hi_b - lo_b);
            const uint64_t kind = below(4);
            const uint64_t span = kind == 0 ? 1 + below(3000) : kind == 1 ? 1 + below(40000) : 1 + below(4000000);
            if (below(12) == 0) lo = top - below(3000000);
            const uint64_t hi = (top - lo < span - 1u) ? top : lo + (span - 1u);
            reqs.push_back(request(msg, lo, hi, i));
        }
        const uint32_t caps[] = {300, 1000, 5000, mh::kMaxBlocksPerLaunch};
        mh::PlanOpts opt;
        switch (below(4)) {
            case 1: opt = l3; break;
            case 2: opt = l2; break;
            case 3: opt = no_early; break;
            default: break;
        }
        check_batch(reqs, opt, caps[below(4)], false, rng, &st);
    }
    printf("passes=%llu slots=%llu items=%llu early_chunks=%llu last_digit_chunks=%llu fallbacks=%llu failures=%d\n",
           (unsigned long long)st.passes, (unsigned long long)st.slots, (unsigned long long)st.items,
           (unsigned long long)st.early_chunks, (unsigned long long)st.last_chunks, (unsigned long long)st.fallbacks,
           failures);
    return failures ? 1 : 0;
}
