// hits_batch_fast_host.cpp -- the host side of mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST)
// (bitcoin-miner_amd/csrc/plan.cpp: plan_hits_batch_pass_ex, hits_batch_table_bytes_ex,
// hits_batch_tables_ex_ok) and the table image hits_batch_run_pass_ex copies to the device, driven on
// the host, to be built with -fsanitize=address,undefined (tests/test_hits_batch_fast_host.py).
// No HIP.
//
//   hits_batch_fast_host <seed> <batches>
//
// Over the shapes of the GPU tests under the plans they use, and over random request lists, caps,
// slot capacities, hit-buffer sizes and table-buffer sizes, pass after pass as the library queues
// them: the tables pass the check; the pass's table image is written into a buffer of exactly
// hits_batch_table_bytes_ex bytes at the window's offset, inside the table buffer; every item's
// cursor address is its request's BatchHitsWords::cursor inside that image and its region the
// request's, inside the window; the regions of a window are disjoint, in order and sized
// min(cap, nonce count, what the window has left); every slot has exactly one writer, whose request
// owns it; a request's tiles and chunks count each of its nonces exactly once, at the top of u64 as
// well; corrupted tables are refused.
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

inline size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }
// memcpy that takes an empty table (a null source with n == 0)
inline void copy(void* dst, const void* src, size_t n) {
    if (n) memcpy(dst, src, n);
}

// The nonces of tile `tile` that batch_scan_hits_slots hashes (search_kernels.hip).
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

// The valid nonces of chunk blk of an item: the lanes batch_hits lets append (fast_search.hip).
uint64_t chunk_count(const mh::FastArgs& a, uint32_t blk) {
    const uint32_t left = a.n_runs - blk * (uint32_t)mh::kBlockThreads;
    const uint32_t lanes = left < (uint32_t)mh::kBlockThreads ? left : (uint32_t)mh::kBlockThreads;
    return (uint64_t)lanes * a.n_groups * 10ull;
}

struct Stats {
    uint64_t passes = 0, fast_passes = 0, items = 0, windows = 0, cut = 0, fallbacks = 0, table_drains = 0;
};

uint64_t request_size(const mh::BatchRequest& r) {
    const uint64_t d = r.upper - r.lower;
    return d == ~(uint64_t)0 ? d : d + 1u;
}

void check_batch(const std::vector<mh::BatchRequest>& reqs, const std::vector<uint64_t>& caps, const mh::PlanOpts& opt,
                 uint32_t slot_cap, const mh::HitsBatchLimits& lim, std::mt19937_64& rng, Stats* st) {
    auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(reqs.data(), reqs.size(), opt, slot_cap, false, mh::kBatchFastMaxNonces, &pieces, &args);
    int passes = 0;
    for (const mh::BatchPiece& p : pieces) {
        if (p.kind != 1) passes = std::max(passes, p.pass + 1);
        else ++st->fallbacks;
    }
    const uint64_t window = std::min<uint64_t>(lim.window_slots, kMaxCap);
    // stand-ins for the device buffers: the addresses are only compared, never followed
    uint8_t* const d_btab = (uint8_t*)(uintptr_t)0x700000000000ull;
    mh::Hit* const d_hits = (mh::Hit*)(uintptr_t)0x710000000000ull;
    std::vector<uint8_t> h_btab(lim.table_bytes);
    mh::HitsBatchState state;
    mh::BatchTables t;
    mh::BatchFastTables f;
    for (int p = 0; p < passes; ++p) {
        mh::build_batch_tables_ex(reqs.data(), pieces, args, p, &t, &f);
        const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
        const size_t ni = f.items.size(), chunks = f.chunk_item.size(), slots = tiles + chunks;
        const size_t bytes = mh::hits_batch_table_bytes_ex(ne, nreq, tiles, ni, chunks);
        CHECK(bytes == mh::hits_batch_table_bytes(ne, nreq, tiles) + ni * sizeof(mh::BatchHitsItem) +
                           align16(chunks * sizeof(uint32_t)));
        if (bytes > lim.table_bytes) continue;  // the library refuses such a pass (MH_EINTERNAL)
        ++st->passes;
        st->fast_passes += ni != 0;
        st->items += ni;
        mh::HitsBatchFastTables x;
        mh::HitsBatchState next = state;
        const bool drain = mh::plan_hits_batch_pass_ex(t, f, reqs.data(), caps.data(), lim, &next, &x);
        const uint64_t used_before = drain ? 0u : state.used;
        const size_t toff = drain ? 0u : state.toff;
        if (drain) {
            ++st->windows;
            CHECK(next.window == state.window + 1);
            if (state.toff + bytes > lim.table_bytes) ++st->table_drains;
        }
        CHECK(next.toff == toff + bytes && toff + bytes <= lim.table_bytes);
        state = next;
        if (!mh::hits_batch_tables_ex_ok(t, f, reqs.data(), x, slot_cap, used_before, window)) {
            CHECK(!"hits_batch_tables_ex_ok");
            continue;
        }
        // the regions: request order, disjoint, inside the window, sized by the rule
        uint64_t used = used_before;
        for (size_t r = 0; r < nreq; ++r) {
            const mh::HitsRegion& g = x.h.region[r];
            const uint64_t want = std::min(caps[t.req_idx[r]], request_size(reqs[t.req_idx[r]]));
            CHECK(g.offset == used && g.slots == std::min(want, lim.window_slots - std::min(used, lim.window_slots)));
            CHECK(g.offset + g.slots <= window);
            if (g.slots < want) ++st->cut;
            used += g.slots;
        }
        CHECK(used == state.used);
        // the table image, as hits_batch_run_pass_ex lays it out (minehip.cpp), written where it goes
        const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
        const size_t o_ereq = o_tile + align16(tiles * sizeof(uint32_t)), o_words = o_ereq + align16(ne * sizeof(uint32_t));
        const size_t o_item = o_words + align16(nreq * sizeof(mh::BatchHitsWords));
        const size_t o_chunk = o_item + ni * sizeof(mh::BatchHitsItem);
        CHECK(o_chunk + align16(chunks * sizeof(uint32_t)) == bytes);
        uint8_t* h = h_btab.data() + toff;
        uint8_t* d = d_btab + toff;
        copy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
        copy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
        copy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
        copy(h + o_ereq, x.h.entry_req.data(), ne * sizeof(uint32_t));
        mh::BatchHitsWords* hw = (mh::BatchHitsWords*)(h + o_words);
        mh::BatchHitsWords* dw = (mh::BatchHitsWords*)(d + o_words);
        for (size_t r = 0; r < nreq; ++r) hw[r] = mh::BatchHitsWords{7u + r, 0ull, x.h.region[r].offset, x.h.region[r].slots};
        mh::BatchHitsItem* hi = (mh::BatchHitsItem*)(h + o_item);
        for (size_t k = 0; k < ni; ++k) {
            const uint32_t r = x.item_req[k];
            mh::BatchHitsItem it;
            memset(&it, 0, sizeof it);
            it.args = f.items[k].args;
            it.h = mh::HitsArgs{hw[r].target, &dw[r].cursor, d_hits + hw[r].offset, hw[r].slots};
            it.chunk0 = f.items[k].chunk0;
            it.slot0 = f.items[k].slot0;
            hi[k] = it;
        }
        copy(h + o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t));
        // what a chunk of the launch finds: its item, its request's cursor inside this pass's words, its
        // request's region inside the window; and every slot has exactly one writer, owned by its request
        std::vector<uint32_t> writers(slots, 0), req_of(slots, 0);
        for (size_t r = 0; r < nreq; ++r)
            for (uint32_t s = t.seg[r]; s < t.seg[r + 1] && s < slots; ++s) req_of[s] = (uint32_t)r;
        std::vector<uint64_t> sum(nreq, 0);
        for (uint32_t tile = 0; tile < tiles; ++tile) {
            const uint32_t ei = ((const uint32_t*)(h + o_tile))[tile];
            const mh::BatchEntry& e = ((const mh::BatchEntry*)h)[ei];
            const uint32_t slot = e.slot0 + (tile - e.tile0);
            CHECK(slot < slots);
            if (slot >= slots) continue;
            ++writers[slot];
            const uint32_t r = ((const uint32_t*)(h + o_ereq))[ei];
            CHECK(req_of[slot] == r);
            sum[r] += tile_count(t, tile);
        }
        for (const mh::BatchFastLaunch& l : f.launches) {
            const uint32_t* chunk_item = (const uint32_t*)(h + o_chunk) + l.chunk0;
            for (uint32_t b = 0; b < l.chunks; ++b) {
                const uint32_t ii = chunk_item[b];
                CHECK(ii < ni);
                const mh::BatchHitsItem& it = hi[ii];
                const uint32_t blk = b - it.chunk0;
                CHECK(b >= it.chunk0 && blk < it.args.n_chunks && it.args.counter == nullptr && it.unused == nullptr);
                CHECK((int)it.args.mode == l.mode);
                const uint32_t slot = it.slot0 + blk;
                CHECK(slot < slots);
                if (slot >= slots) continue;
                ++writers[slot];
                const uint32_t r = req_of[slot];
                CHECK(it.h.cursor == &dw[r].cursor && it.h.target == hw[r].target);
                CHECK((uint8_t*)it.h.cursor >= d + o_words && (uint8_t*)it.h.cursor + 8 <= d + o_item);
                CHECK(it.h.hits == d_hits + x.h.region[r].offset && it.h.cap == x.h.region[r].slots);
                CHECK((uint64_t)(it.h.hits - d_hits) + it.h.cap <= window);
                sum[r] += chunk_count(it.args, blk);
            }
        }
        for (size_t s = 0; s < slots; ++s) CHECK(writers[s] == 1);
        for (size_t r = 0; r < nreq; ++r) CHECK(sum[r] == reqs[t.req_idx[r]].upper - reqs[t.req_idx[r]].lower + 1u);
        // corrupted tables are refused
        if (ni) {
            mh::BatchFastTables fb = f;
            const size_t k = below(ni);
            fb.items[k].slot0 = fb.items[k].slot0 ? fb.items[k].slot0 - 1u : 1u;  // overlaps a neighbour's slot
            CHECK(!mh::hits_batch_tables_ex_ok(t, fb, reqs.data(), x, slot_cap, used_before, window));
            mh::HitsBatchFastTables xb = x;
            if (nreq > 1) {
                xb.item_req[k] = (xb.item_req[k] + 1u) % (uint32_t)nreq;  // another request's cursor and region
                CHECK(!mh::hits_batch_tables_ex_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            }
            xb = x;
            xb.item_req.pop_back();
            CHECK(!mh::hits_batch_tables_ex_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            fb = f;
            fb.chunk_item[below(chunks)] = (uint32_t)ni;  // no such item
            CHECK(!mh::hits_batch_tables_ex_ok(t, fb, reqs.data(), x, slot_cap, used_before, window));
        }
        {
            mh::HitsBatchFastTables xb = x;
            const size_t r = below(nreq);
            xb.h.region[r].offset = window + 1u;  // outside the buffer
            CHECK(!mh::hits_batch_tables_ex_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            xb = x;
            xb.h.region[r].slots = request_size(reqs[t.req_idx[r]]) + 1u;  // more than the request can fill
            if (xb.h.region[r].slots) CHECK(!mh::hits_batch_tables_ex_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            if (nreq > 1 && x.h.region[0].slots) {
                xb = x;
                xb.h.region[1].offset = xb.h.region[0].offset;  // overlaps its neighbour
                CHECK(!mh::hits_batch_tables_ex_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
            }
            // a region below where the window's earlier passes end
            CHECK(!mh::hits_batch_tables_ex_ok(t, f, reqs.data(), x, slot_cap, x.h.region[0].offset + 1u, window));
            if (ne && nreq > 1) {
                xb = x;
                xb.h.entry_req[0] = (xb.h.entry_req[0] + 1u) % (uint32_t)nreq;
                CHECK(!mh::hits_batch_tables_ex_ok(t, f, reqs.data(), xb, slot_cap, used_before, window));
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

    // the shapes of tests/test_gpu_hits_batch_fast.py, under the plans and buffer sizes it uses
    const uint64_t top = ~0ull;
    std::vector<mh::BatchRequest> shapes;
    const struct {
        std::string msg;
        uint64_t lo, hi;
    } kShapes[] = {{"cmu440", 1048000, 2200000},  {"cmu440", 0, 3000000}, {std::string(51, 'a'), 0, 3000000},
                   {std::string(60, 'a'), 0, 3000000}, {std::string(47, 'a'), 900000, 3000000},
                   {"cmu440", 500000000, 503000000}, {"cmu440", top - 3000000, top}, {"cmu440", 0, 199999},
                   {"x", 5, 5}, {"", 0, 1000}, {"cmu441", 1048000, 2200000}};
    for (const auto& s : kShapes) shapes.push_back(request(s.msg, s.lo, s.hi, shapes.size()));
    const std::vector<uint64_t> caps4096(shapes.size(), 4096);
    mh::PlanOpts dflt, l3, l2, no_early;
    l3.lower_digits = 3;
    l3.min_lanes = 16;
    l2.lower_digits = 2;
    l2.min_lanes = 16;
    no_early.early = 0;
    const size_t table_bytes = 4u << 20, results = 1u << 16;
    const mh::HitsBatchLimits full{table_bytes, results, kMaxCap};
    for (const mh::PlanOpts& o : {dflt, l3, l2, no_early}) check_batch(shapes, caps4096, o, mh::kMaxBlocksPerLaunch, full, rng, &st);
    CHECK(st.fast_passes == 4 && st.fallbacks == 0 && st.cut == 0 && st.windows == 0);
    check_batch(shapes, caps4096, dflt, 1000, full, rng, &st);
    CHECK(st.fallbacks > 0);
    check_batch(shapes, caps4096, dflt, mh::kMaxBlocksPerLaunch, mh::HitsBatchLimits{table_bytes, results, 5000}, rng, &st);
    CHECK(st.cut > 0);
    check_batch(shapes, caps4096, dflt, 1000, mh::HitsBatchLimits{table_bytes, results, 1500}, rng, &st);
    CHECK(st.windows > 0);
    {   // a table buffer that holds two or three passes: the items and per-chunk tables count, and a drain follows
        const std::vector<uint64_t> caps16(shapes.size(), 16);
        check_batch(shapes, caps16, dflt, 500, mh::HitsBatchLimits{4u << 10, results, kMaxCap}, rng, &st);
        CHECK(st.table_drains > 0);
    }
    {   // caps around a count, a count-only request and the largest cap, as the truncation test has them
        std::vector<uint64_t> caps = {1, 2999, 3000, 3001, 0, kMaxCap, 16, 4096, 4096, 4096, 65536};
        check_batch(shapes, caps, dflt, mh::kMaxBlocksPerLaunch, full, rng, &st);
    }

    // a seeded fuzz of request lists, caps and window sizes: small generic requests beside ones of a
    // few 10^6 nonces, which plan fast pieces, in every decimal length, the top of u64 included
    for (int b = 0; b < batches; ++b) {
        const size_t n = 1 + (size_t)below(24);
        std::vector<mh::BatchRequest> reqs;
        std::vector<uint64_t> caps;
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
            const uint64_t cs[] = {0, 1, 16, 4096, 65536, kMaxCap};
            caps.push_back(cs[below(6)]);
        }
        const uint32_t slot_caps[] = {300, 1000, 5000, mh::kMaxBlocksPerLaunch};
        const uint64_t windows[] = {1, 8, 1500, 5000, 100000, kMaxCap};
        const size_t tables[] = {64u << 10, 256u << 10, table_bytes};
        mh::PlanOpts opt;
        switch (below(4)) {
            case 1: opt = l3; break;
            case 2: opt = l2; break;
            case 3: opt = no_early; break;
            default: break;
        }
        check_batch(reqs, caps, opt, slot_caps[below(4)], mh::HitsBatchLimits{tables[below(3)], results, windows[below(6)]},
                    rng, &st);
    }
    printf("passes=%llu fast_passes=%llu items=%llu windows=%llu cut=%llu fallbacks=%llu table_drains=%llu failures=%d\n",
           (unsigned long long)st.passes, (unsigned long long)st.fast_passes, (unsigned long long)st.items,
           (unsigned long long)st.windows, (unsigned long long)st.cut, (unsigned long long)st.fallbacks,
           (unsigned long long)st.table_drains, failures);
    return failures ? 1 : 0;
}
