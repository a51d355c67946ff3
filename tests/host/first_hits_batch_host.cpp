// first_hits_batch_host.cpp -- the host side of mh_search_first_hits_batch
// (bitcoin-miner_amd/csrc/plan.cpp: plan_first_hits_batch_pass, first_hits_batch_layout,
// first_hits_batch_tables_ok, build_first_hits_batch_image, first_hits_batch_image_ok,
// read_first_hits_batch), driven on the host as minehip.cpp's first_hits_batch_run_pass drives it,
// to be built with -fsanitize=address,undefined (tests/test_first_hits_batch_host.py).  No HIP.
//
//   first_hits_batch_host <seed> <batches>
//
// Over the shapes of tests/test_gpu_first_hits_batch.py under the plans it uses, and over random
// request lists, k values, slot capacities, hit-buffer sizes and table-buffer sizes, pass after pass
// as the library queues them, with flags == 0 (plan_batch) and MH_BATCH_FUSE_FAST (plan_batch_ex):
// the tables pass the check; the image is written into a buffer of exactly the layout's bytes at the
// window's offset, inside the table buffer, and passes its check; every request's words hold its
// region, its own range's slicing and the initial values; every item's bound, cursor, scanned, region
// and slice counters are its request's, inside the image, the window and the counters' buffer; the
// counters of different requests do not overlap; the regions of a window are disjoint, in order and
// sized min(nonce count, max(4 k, 256), what the window has left); every slot has exactly one writer,
// whose request owns it, and both orders run every tile and chunk exactly once; a request's tiles and
// chunks count each nonce once; corrupted tables and images are refused.  Then the host's reading of
// a pass (read_first_hits_batch) over made-up cursors and entries: the sort, stored, the minimum of
// the k entries and the rebuild decision.
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
constexpr uint64_t kMaxCap = 1u << 20;  // MH_HITS_MAX_CAP: the device hit buffer's entries

// The nonces of tile `tile` that batch_scan_bound hashes and counts as scanned (search_kernels.hip).
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

// The valid nonces of chunk blk of an item: what batch_bound's waves count when the chunk runs whole.
uint64_t chunk_count(const mh::FastArgs& a, uint32_t blk) {
    const uint32_t left = a.n_runs - blk * (uint32_t)mh::kBlockThreads;
    const uint32_t lanes = left < (uint32_t)mh::kBlockThreads ? left : (uint32_t)mh::kBlockThreads;
    return (uint64_t)lanes * a.n_groups * 10ull;
}

struct Stats {
    uint64_t passes = 0, fast_passes = 0, items = 0, windows = 0, cut = 0, drains = 0, fallbacks = 0, rebuilds = 0,
             answered = 0;
};

uint64_t request_size(const mh::BatchRequest& r) {
    const uint64_t d = r.upper - r.lower;
    return d == ~(uint64_t)0 ? d : d + 1u;
}

void check_batch(const std::vector<mh::BatchRequest>& reqs, const std::vector<uint64_t>& ks, const mh::PlanOpts& opt,
                 bool fuse_fast, uint32_t slot_cap, const mh::HitsBatchLimits& lim, bool rank_major, std::mt19937_64& rng,
                 Stats* st) {
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    std::vector<uint64_t> targets, wants;
    for (size_t i = 0; i < reqs.size(); ++i) {
        targets.push_back(1000u + i);
        wants.push_back(mh::first_hits_batch_want(ks[i]));
        CHECK(wants.back() == std::max<uint64_t>(4u * ks[i], 256u));
    }
    std::vector<mh::BatchItem> items;
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    int passes = 0;
    if (fuse_fast) {
        mh::plan_batch_ex(reqs.data(), reqs.size(), opt, slot_cap, false, mh::kBatchFastMaxNonces, &pieces, &args);
        for (const mh::BatchPiece& p : pieces) {
            if (p.kind != 1) passes = std::max(passes, p.pass + 1);
            else ++st->fallbacks;
        }
    } else {
        mh::plan_batch(reqs.data(), reqs.size(), opt, slot_cap, &items);
        for (const mh::BatchItem& it : items) {
            if (it.kind == 0) passes = std::max(passes, it.pass + 1);
            else ++st->fallbacks;
        }
    }
    const uint64_t window = std::min<uint64_t>(lim.window_slots, kMaxCap);
    // stand-ins for the device buffers: the addresses are only compared, never followed
    const uint64_t d_tab = 0x700000000000ull, d_hits = 0x710000000000ull, d_slices = 0x720000000000ull;
    const uint64_t slices_bytes = (uint64_t)mh::kBatchMaxRequests * mh::kFirstHitsSlices * sizeof(uint32_t);
    std::vector<uint8_t> h_tab(lim.table_bytes);
    mh::HitsBatchState state;
    mh::BatchTables t;
    mh::BatchFastTables f;
    for (int p = 0; p < passes; ++p) {
        if (fuse_fast) mh::build_batch_tables_ex(reqs.data(), pieces, args, p, &t, &f);
        else mh::build_batch_tables(reqs.data(), items, p, &t);
        const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
        const size_t ni = f.items.size(), chunks = f.chunk_item.size(), slots = tiles + chunks;
        const mh::FirstHitsBatchLayout l = mh::first_hits_batch_layout(ne, nreq, tiles, ni, chunks);
        CHECK(l.o_seg % 16 == 0 && l.o_tile % 16 == 0 && l.o_ereq % 16 == 0 && l.o_order % 16 == 0 && l.o_words % 16 == 0 &&
              l.o_item % 16 == 0 && l.o_chunk % 16 == 0 && l.o_corder % 16 == 0 && l.bytes % 16 == 0);
        CHECK(l.o_item == l.o_words + nreq * sizeof(mh::BatchBoundWords) && l.o_chunk == l.o_item + ni * sizeof(mh::BatchBoundItem));
        if (l.bytes > lim.table_bytes) continue;  // the library refuses such a pass (MH_EINTERNAL)
        ++st->passes;
        st->fast_passes += ni != 0;
        st->items += ni;
        mh::FirstHitsBatchTables x;
        mh::HitsBatchState next = state;
        const bool drain = mh::plan_first_hits_batch_pass(t, f, reqs.data(), wants.data(), lim, rank_major, &next, &x);
        const uint64_t used_before = drain ? 0u : state.used;
        const size_t toff = drain ? 0u : state.toff;
        if (drain) {
            ++st->drains;
            ++st->windows;
            CHECK(next.window == state.window + 1);
        }
        CHECK(next.toff == toff + l.bytes && toff + l.bytes <= lim.table_bytes);
        state = next;
        if (!mh::first_hits_batch_tables_ok(t, f, reqs.data(), x, slot_cap, used_before, window)) {
            CHECK(!"first_hits_batch_tables_ok");
            continue;
        }
        // the regions: request order, disjoint, inside the window, sized by the rule
        uint64_t used = used_before;
        for (size_t r = 0; r < nreq; ++r) {
            const mh::HitsRegion& g = x.region[r];
            const uint64_t want = std::min(wants[t.req_idx[r]], request_size(reqs[t.req_idx[r]]));
            CHECK(g.offset == used && g.slots == std::min(want, lim.window_slots - std::min(used, lim.window_slots)));
            CHECK(g.offset + g.slots <= window && g.slots <= request_size(reqs[t.req_idx[r]]));
            if (g.slots < want) ++st->cut;
            used += g.slots;
        }
        CHECK(used == state.used);
        // the image, written where it goes, and its check
        uint8_t* h = h_tab.data() + toff;
        const mh::FirstHitsBatchAddrs at{d_tab + toff, d_hits, d_slices};
        mh::build_first_hits_batch_image(t, f, x, reqs.data(), targets.data(), ks.data(), at, h);
        CHECK(mh::first_hits_batch_image_ok(t, f, x, reqs.data(), at, window, h));
        const mh::BatchBoundWords* hw = (const mh::BatchBoundWords*)(h + l.o_words);
        const mh::BatchBoundItem* hi = (const mh::BatchBoundItem*)(h + l.o_item);
        for (size_t r = 0; r < nreq; ++r) {
            const mh::BatchRequest& q = reqs[t.req_idx[r]];
            CHECK(hw[r].target == targets[t.req_idx[r]] && hw[r].k == ks[t.req_idx[r]] && hw[r].cursor == 0 &&
                  hw[r].bound == ~0ull && hw[r].scanned == 0);
            CHECK(hw[r].offset == x.region[r].offset && hw[r].slots == x.region[r].slots);
            CHECK(hw[r].lower == q.lower && hw[r].span == q.upper - q.lower && hw[r].shift == mh::first_hits_shift(q.upper - q.lower));
            CHECK(mh::first_hits_slices(hw[r].span, hw[r].shift) <= mh::kFirstHitsSlices);
        }
        // what a tile or chunk finds: its request's words; every slot has exactly one writer, owned by
        // its request; both orders run every tile and chunk exactly once
        std::vector<uint32_t> writers(slots, 0), req_of(slots, 0);
        for (size_t r = 0; r < nreq; ++r)
            for (uint32_t s = t.seg[r]; s < t.seg[r + 1] && s < slots; ++s) req_of[s] = (uint32_t)r;
        std::vector<uint64_t> sum(nreq, 0);
        const uint32_t* order = (const uint32_t*)(h + l.o_order);
        for (uint32_t b = 0; b < tiles; ++b) {
            const uint32_t tile = order[b];
            CHECK(tile < tiles);
            if (tile >= tiles) continue;
            const uint32_t ei = ((const uint32_t*)(h + l.o_tile))[tile];
            const mh::BatchEntry& e = ((const mh::BatchEntry*)h)[ei];
            const uint32_t slot = e.slot0 + (tile - e.tile0);
            CHECK(slot < slots && (ni != 0 || slot == tile));
            if (slot >= slots) continue;
            ++writers[slot];
            const uint32_t r = ((const uint32_t*)(h + l.o_ereq))[ei];
            CHECK(r < nreq && req_of[slot] == r);
            sum[r] += tile_count(t, tile);
        }
        std::vector<uint8_t> owner(nreq, 0);  // the requests whose counters some item uses
        for (const mh::BatchFastLaunch& fl : f.launches) {
            const uint32_t* chunk_item = (const uint32_t*)(h + l.o_chunk) + fl.chunk0;
            const uint32_t* corder = (const uint32_t*)(h + l.o_corder) + fl.chunk0;
            for (uint32_t b = 0; b < fl.chunks; ++b) {
                const uint32_t c = corder[b];
                CHECK(c < fl.chunks);
                if (c >= fl.chunks) continue;
                const uint32_t ii = chunk_item[c];
                CHECK(ii < ni);
                if (ii >= ni) continue;
                const mh::BatchBoundItem& it = hi[ii];
                const uint32_t blk = c - it.chunk0;
                CHECK(c >= it.chunk0 && blk < it.args.n_chunks && it.args.counter == nullptr && it.unused == nullptr);
                CHECK((int)it.args.mode == fl.mode);
                const uint32_t slot = it.slot0 + blk;
                CHECK(slot < slots);
                if (slot >= slots) continue;
                ++writers[slot];
                const uint32_t r = req_of[slot];
                const uint64_t words = at.image + l.o_words + (uint64_t)r * sizeof(mh::BatchBoundWords);
                CHECK((uint64_t)it.h.h.cursor == words + offsetof(mh::BatchBoundWords, cursor));
                CHECK((uint64_t)it.h.bound == words + offsetof(mh::BatchBoundWords, bound));
                CHECK((uint64_t)it.h.scanned == words + offsetof(mh::BatchBoundWords, scanned));
                CHECK(words >= at.image + l.o_words && words + sizeof(mh::BatchBoundWords) <= at.image + l.o_item);
                CHECK(it.h.h.target == hw[r].target && it.h.k == hw[r].k && it.h.lower == hw[r].lower &&
                      it.h.span == hw[r].span && it.h.shift == hw[r].shift);
                CHECK((uint64_t)it.h.h.hits == d_hits + x.region[r].offset * sizeof(mh::Hit) && it.h.h.cap == x.region[r].slots);
                CHECK(x.region[r].offset + it.h.h.cap <= window);
                const uint64_t sl = (uint64_t)it.h.slices;
                CHECK(sl == d_slices + (uint64_t)r * mh::kFirstHitsSlices * sizeof(uint32_t));
                CHECK(sl + mh::kFirstHitsSlices * sizeof(uint32_t) <= d_slices + slices_bytes);
                owner[r] = 1;
                sum[r] += chunk_count(it.args, blk);
            }
        }
        // (the counters of request r are kFirstHitsSlices words at r * kFirstHitsSlices: distinct r, disjoint counters)
        CHECK(nreq <= mh::kBatchMaxRequests);
        for (size_t s = 0; s < slots; ++s) CHECK(writers[s] == 1);
        for (size_t r = 0; r < nreq; ++r) CHECK(sum[r] == reqs[t.req_idx[r]].upper - reqs[t.req_idx[r]].lower + 1u);
        // corrupted tables and images are refused
        if (ni) {
            mh::BatchFastTables fb = f;
            const size_t k = below(ni);
            fb.items[k].slot0 = fb.items[k].slot0 ? fb.items[k].slot0 - 1u : 1u;  // overlaps a neighbour's slot
            CHECK(!mh::first_hits_batch_tables_ok(t, fb, reqs.data(), x, slot_cap, used_before, window));
            mh::FirstHitsBatchTables xb = x;
            if (nreq > 1) {
                xb.o.item_req[k] = (xb.o.item_req[k] + 1u) % (uint32_t)nreq;  // another request's words
                CHECK(!mh::first_hits_batch_tables_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            }
            xb = x;
            xb.o.chunk_order[below(chunks)] = (uint32_t)chunks;  // no such chunk
            CHECK(!mh::first_hits_batch_tables_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            std::vector<uint8_t> img(h, h + l.bytes);
            mh::BatchBoundItem* bi = (mh::BatchBoundItem*)(img.data() + l.o_item);
            bi[k].h.bound = (unsigned long long*)((uint64_t)bi[k].h.bound + sizeof(mh::BatchBoundWords));  // a neighbour's bound
            CHECK(!mh::first_hits_batch_image_ok(t, f, x, reqs.data(), at, window, img.data()));
            img.assign(h, h + l.bytes);
            bi[k].h.slices += mh::kFirstHitsSlices;  // a neighbour's counters
            CHECK(!mh::first_hits_batch_image_ok(t, f, x, reqs.data(), at, window, img.data()));
            img.assign(h, h + l.bytes);
            bi[k].h.h.cap += 1u;  // past the region's end
            CHECK(!mh::first_hits_batch_image_ok(t, f, x, reqs.data(), at, window, img.data()));
            img.assign(h, h + l.bytes);
            bi[k].h.k += 1u;  // not the request's k
            CHECK(!mh::first_hits_batch_image_ok(t, f, x, reqs.data(), at, window, img.data()));
        }
        {
            mh::FirstHitsBatchTables xb = x;
            const size_t r = below(nreq);
            xb.region[r].offset = window + 1u;  // outside the buffer
            CHECK(!mh::first_hits_batch_tables_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            xb = x;
            xb.region[r].slots = request_size(reqs[t.req_idx[r]]) + 1u;  // more than the request can fill
            if (xb.region[r].slots) CHECK(!mh::first_hits_batch_tables_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            if (nreq > 1 && x.region[0].slots) {
                xb = x;
                xb.region[1].offset = xb.region[0].offset;  // overlaps its neighbour
                CHECK(!mh::first_hits_batch_tables_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            }
            if (tiles > 1) {
                xb = x;
                xb.o.tile_order[0] = xb.o.tile_order[1];  // a tile twice, another never
                CHECK(!mh::first_hits_batch_tables_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            }
            if (ne && nreq > 1) {
                xb = x;
                xb.o.entry_req[0] = (xb.o.entry_req[0] + 1u) % (uint32_t)nreq;
                CHECK(!mh::first_hits_batch_tables_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            }
            std::vector<uint8_t> img(h, h + l.bytes);
            mh::BatchBoundWords* bw = (mh::BatchBoundWords*)(img.data() + l.o_words);
            bw[r].bound = 5u;  // not all ones at the start
            CHECK(!mh::first_hits_batch_image_ok(t, f, x, reqs.data(), at, window, img.data()));
            img.assign(h, h + l.bytes);
            bw[r].shift += 1u;  // not the request's slicing
            CHECK(!mh::first_hits_batch_image_ok(t, f, x, reqs.data(), at, window, img.data()));
            img.assign(h, h + l.bytes);
            bw[r].slots += 1u;  // not the region
            CHECK(!mh::first_hits_batch_image_ok(t, f, x, reqs.data(), at, window, img.data()));
        }
        // the host's reading of the pass: made-up cursors and entries per request
        for (size_t r = 0; r < nreq; ++r) {
            const mh::BatchRequest& q = reqs[t.req_idx[r]];
            const uint64_t k = ks[t.req_idx[r]], slots_r = x.region[r].slots, size = request_size(q);
            const uint64_t picks[] = {0, k ? k - 1u : 0, k, k + 1u, slots_r, slots_r + 1u};
            const uint64_t count = std::min<uint64_t>(picks[below(6)], std::min<uint64_t>(size, 5000));
            std::vector<mh::Hit> got((size_t)std::min(count, slots_r));
            std::vector<uint64_t> nonces;
            for (size_t i = 0; i < got.size(); ++i) nonces.push_back(q.lower + (size > 1 ? below(size) : 0));
            std::sort(nonces.begin(), nonces.end());
            nonces.erase(std::unique(nonces.begin(), nonces.end()), nonces.end());
            got.resize(nonces.size());
            const uint64_t c = count > slots_r ? count : got.size();  // a cursor the region could hold, or one past it
            for (size_t i = 0; i < got.size(); ++i) got[i] = mh::Hit{rng() % 1000u, nonces[i]};
            std::vector<mh::Hit> sorted = got;
            std::shuffle(got.begin(), got.end(), rng);
            uint64_t stored = ~0ull, hash = 1, nonce = 2;
            const bool ok = mh::read_first_hits_batch(got.data(), c, slots_r, k, &stored, &hash, &nonce);
            CHECK(ok == (c <= slots_r));
            if (!ok) {
                ++st->rebuilds;
                CHECK(stored == ~0ull && hash == 1 && nonce == 2);  // nothing of the answer is touched
                continue;
            }
            ++st->answered;
            CHECK(stored == std::min<uint64_t>(c, k));
            for (size_t i = 0; i < got.size(); ++i) CHECK(got[i].nonce == sorted[i].nonce && got[i].hash == sorted[i].hash);
            if (stored == k) {
                uint64_t bh = ~0ull, bn = ~0ull;
                for (uint64_t i = 0; i < k; ++i)
                    if (sorted[i].hash < bh || (sorted[i].hash == bh && sorted[i].nonce < bn)) bh = sorted[i].hash, bn = sorted[i].nonce;
                CHECK(hash == bh && nonce == bn);
            } else {
                CHECK(hash == 1 && nonce == 2);  // left to the caller: the merged minimum
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

    // the shapes of tests/test_gpu_first_hits_batch.py, under the plans and buffer sizes it uses
    const uint64_t top = ~0ull;
    std::vector<mh::BatchRequest> shapes;
    const struct {
        std::string msg;
        uint64_t lo, hi;
    } kShapes[] = {{"cmu440", 0, 1999999},        {"cmu441", 0, 999999},       {std::string(60, 'x'), 1000000, 1499999},
                   {"cmu440", 1000000, 1999999},  {"cmu441", 1000000, 1999999}, {std::string(60, 'x'), 1000000, 1999999},
                   {"cmu440", 95000, 105123},     {"cmu440", 123456789, 123456789}, {"", top, top},
                   {std::string(60, 'q'), top - 30000, top}, {"cmu440", 0, 2999}, {"cmu440", 0, 1999999999}, {"cmu440-07", 0, 999999}};
    for (const auto& s : kShapes) shapes.push_back(request(s.msg, s.lo, s.hi, shapes.size()));
    const std::vector<uint64_t> ks = {1, 2, 300, 2, 4, 4, 100, 4, 1, 3, 3, 2, 4};
    mh::PlanOpts dflt, fast1, fast3;
    fast1.generic_below = 0;
    fast1.min_lanes = 1;
    fast1.lower_digits = 1;
    fast3 = fast1;
    fast3.lower_digits = 3;
    const size_t table_bytes = 5u << 20, results = 1u << 16;
    const mh::HitsBatchLimits full{table_bytes, results, kMaxCap};
    for (const bool fuse : {false, true})
        for (const bool rank : {true, false})
            for (const mh::PlanOpts& o : {dflt, fast1, fast3}) check_batch(shapes, ks, o, fuse, mh::kMaxBlocksPerLaunch, full, rank, rng, &st);
    CHECK(st.fast_passes >= 2 && st.fallbacks > 0 && st.cut == 0 && st.windows == 0);
    check_batch(shapes, ks, dflt, false, 4000, full, true, rng, &st);  // MINEHIP_BATCH_SLOTS=4000
    for (const uint64_t w : {64u, 1u}) {                              // MINEHIP_HITS_SLOTS=64 and =1
        check_batch(shapes, ks, dflt, false, 1000, mh::HitsBatchLimits{table_bytes, results, w}, true, rng, &st);  // several passes
        check_batch(shapes, ks, fast3, true, mh::kMaxBlocksPerLaunch, mh::HitsBatchLimits{table_bytes, results, w}, true, rng, &st);
    }
    CHECK(st.cut > 0 && st.windows > 0);
    {   // 64 requests of one shape, and a table buffer that holds only a few passes: a drain follows
        std::vector<mh::BatchRequest> many;
        for (size_t i = 0; i < 64; ++i) many.push_back(request("cmu440-" + std::to_string(i), 0, 999999, i));
        const std::vector<uint64_t> k4(64, 4);
        check_batch(many, k4, dflt, false, mh::kMaxBlocksPerLaunch, full, true, rng, &st);
        const uint64_t before = st.drains;
        check_batch(many, k4, dflt, false, 2000, mh::HitsBatchLimits{96u << 10, results, kMaxCap}, true, rng, &st);
        CHECK(st.drains > before);
    }

    // a seeded fuzz of request lists, k values and window sizes: small generic requests beside ones of
    // a few 10^6 nonces, which plan fast pieces, in every decimal length, the top of u64 included
    for (int b = 0; b < batches; ++b) {
        const size_t n = 1 + (size_t)below(24);
        std::vector<mh::BatchRequest> reqs;
        std::vector<uint64_t> kk;
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
            const uint64_t cs[] = {1, 2, 16, 64, 100, 4096, 65536, kMaxCap};
            kk.push_back(cs[below(8)]);
        }
        const uint32_t slot_caps[] = {300, 1000, 5000, mh::kMaxBlocksPerLaunch};
        const uint64_t windows[] = {1, 64, 1500, 5000, 100000, kMaxCap};
        const size_t tables[] = {96u << 10, 512u << 10, table_bytes};
        mh::PlanOpts opt;
        switch (below(3)) {
            case 1: opt = fast1; opt.generic_below = dflt.generic_below; opt.min_lanes = 16; break;
            case 2: opt = fast3; opt.generic_below = dflt.generic_below; opt.min_lanes = 16; break;
            default: break;
        }
        check_batch(reqs, kk, opt, below(2) != 0, slot_caps[below(4)], mh::HitsBatchLimits{tables[below(3)], results, windows[below(6)]},
                    below(2) != 0, rng, &st);
    }
    printf("passes=%llu fast_passes=%llu items=%llu windows=%llu cut=%llu drains=%llu fallbacks=%llu rebuilds=%llu answered=%llu "
           "failures=%d\n",
           (unsigned long long)st.passes, (unsigned long long)st.fast_passes, (unsigned long long)st.items,
           (unsigned long long)st.windows, (unsigned long long)st.cut, (unsigned long long)st.drains,
           (unsigned long long)st.fallbacks, (unsigned long long)st.rebuilds, (unsigned long long)st.answered, failures);
    return failures ? 1 : 0;
}
