// layout.hpp -- host/device shared launch descriptors for libminehip.
//
// The message the reference hashes per nonce is  msg ' ' decimal(nonce)
// (bitcoin/hash.go:15).  The host absorbs every full 64-byte block of the
// constant prefix P = msg ' ' into a midstate; what remains is the "tail":
// t = len(P) mod 64 prefix bytes, then the d digits, 0x80, zeros and the
// 64-bit bit length -- one or two 64-byte tail blocks (tail byte positions
// 0..127, big-endian words 0..31).
//
// A search over one decimal-length bucket (all nonces have d digits) splits
// every nonce n = U * 10^L + q into a run index U (the d-L "higher" digits,
// one run per GPU lane) and q in [0, 10^L) (the L "lower" digits, enumerated
// inside the lane).  See DESIGN.md §3.
#pragma once
#include <stdint.h>

namespace mh {

constexpr int kBlockThreads = 256;         // 4 waves of 64 per workgroup
constexpr uint32_t kMaxBlocksPerLaunch = 1u << 18;  // partials buffer slots; hard cap of one grid

struct Partial {          // one (hash, nonce) candidate; ordered lexicographically
    uint64_t hash;
    uint64_t nonce;
};

enum FastMode : uint32_t {
    kModeOne = 0,   // one tail block, compressed per nonce from the host midstate
    kModePre = 1,   // two tail blocks; block 0 holds no lower digit and is compressed once per run
    kModeTwo = 2,   // two tail blocks; the lower digits sit in block 0 -> both blocks per nonce
    // The same three tail layouts with an earlier innermost digit (mode - 3 is the tail layout):
    // the digit enumerated per nonce is not the last one but the digit ending word J, the word
    // before the last digit's, at decimal position p = 1..4, and the other enumerated digits (a
    // group, per 10 nonces) are the L - 1 right before it in word J.  A nonce then costs
    // nonce_cost(J) instead of nonce_cost(J + 1), which is less for J + 1 = 1 (W[1] reaches W[16]
    // through sigma0), J + 1 = 9 (W[9] is W[16]'s t-7 term) and J + 1 = 14, and
    // only word J changes inside a lane.  A lane's nonces are not contiguous: its U digits are the
    // p below and the ones above the L enumerated positions p .. p+L-1.
    kModeOneEarly = 3,
    kModePreEarly = 4,
    kModeTwoEarly = 5,
};
constexpr int kModes = 6;

// The instantiated fast_search<J, MODE> kernels: every layout a bucket with d <= 20 can produce
// (One J = 0..13, Pre J = 0..4, Two J = 13..15) and the Early layouts the planner takes (One
// J = 0, 8, Pre J = 0, Two J = 13).  The one list: fast_search.hip instantiates it, the planner
// (plan.cpp) and the launcher (search_kernels.hip) accept exactly it, csrc/loop_mix.py and the
// tests read it from here.
#define MH_FAST_KERNELS(X)                                                                                 \
    X(0, kModeOne) X(1, kModeOne) X(2, kModeOne) X(3, kModeOne) X(4, kModeOne) X(5, kModeOne)              \
    X(6, kModeOne) X(7, kModeOne) X(8, kModeOne) X(9, kModeOne) X(10, kModeOne) X(11, kModeOne)            \
    X(12, kModeOne) X(13, kModeOne)                                                                        \
    X(0, kModePre) X(1, kModePre) X(2, kModePre) X(3, kModePre) X(4, kModePre)                             \
    X(13, kModeTwo) X(14, kModeTwo) X(15, kModeTwo)                                                        \
    X(0, kModeOneEarly) X(8, kModeOneEarly) X(0, kModePreEarly) X(13, kModeTwoEarly)

struct FastKernelId {
    int J;
    int mode;
};
#define MH_FAST_KERNEL_ID(j, m) FastKernelId{j, m},
constexpr FastKernelId kFastKernels[] = {MH_FAST_KERNELS(MH_FAST_KERNEL_ID)};
#undef MH_FAST_KERNEL_ID
constexpr int kNumFastKernels = (int)(sizeof(kFastKernels) / sizeof(kFastKernels[0]));

constexpr bool fast_kernel_exists(int J, int mode) {
    for (const FastKernelId& k : kFastKernels)
        if (k.J == J && k.mode == mode) return true;
    return false;
}
constexpr uint32_t kNoHole = 20;  // a digit index no layout reaches (d <= 20)

// Coarse-hash word of the dev build (MINEHIP_DEV_HASH_KEEP=k0,k1): a test hook that
// makes many nonces share a hash, so the (hash, nonce) tie-breaking of every kernel and merge runs
// on the GPU.  It travels in the padding words FastArgs::pad_ and GenArgs::pad: 0 is off (all the
// product library ever passes); otherwise kKeepFlag | k0 << 8 | k1, and a scan kernel built with
// the hook replaces each nonce's (H0, H1) by (H0 & keep_mask(k0), H1 & keep_mask(k1)), the top
// k0 / k1 bits, before any comparison.
constexpr uint32_t kKeepFlag = 1u << 31;
constexpr uint32_t keep_word(uint32_t k0, uint32_t k1) { return kKeepFlag | (k0 << 8) | k1; }
constexpr uint32_t keep_mask(uint32_t k) { return k ? ~0u << (32u - k) : 0u; }  // k = 0..32
constexpr uint32_t keep_mask0(uint32_t word) { return word ? keep_mask((word >> 8) & 63u) : ~0u; }
constexpr uint32_t keep_mask1(uint32_t word) { return word ? keep_mask(word & 63u) : ~0u; }
// Hash-XOR constant of the dev build (MINEHIP_DEV_HASH_XOR=<1-16 hex digits>): a scan
// kernel built with the hook XORs each nonce's (H0, H1) with the constant's high and low 32 bits
// before the keep mask above, so a test chooses which nonce wins (x = Hash(msg, n): the search must
// return (0, n)).  The padding words are the keep word's, so it travels in no argument struct but
// in a device word mh_dev_hash_xor[2] = {high, low}, zero (off) unless the dev build writes it: one
// in the dev library (search_kernels.hip), one in the variant fast code object (fast_search.hip).

// Arguments of the fast (run) kernel.  Passed by value: lands in SGPRs.
struct FastArgs {
    uint32_t mid[8];      // chaining state before tail block 0
    uint32_t blk[32];     // tail words: prefix bytes, '0' at every digit byte, 0x80, bit length
    uint64_t u_start;     // run index U of lane 0 of block 0
    uint64_t pow10L;      // 10^L
    uint32_t n_runs;      // active lanes in this launch
    uint32_t hi_end;      // tail byte index one past U's last digit
    uint32_t n_hi;        // digits of U (= d - L)
    uint32_t lo_pos;      // byte index (within the per-nonce block) of the first lower digit
    uint32_t L;           // lower digits enumerated inside a lane (1..5)
    uint32_t n_groups;    // 10^(L-1): groups of 10 consecutive nonces per lane
    uint32_t mode;        // FastMode
    uint32_t n_chunks;    // workgroup-sized chunks (256 runs each) in this launch
    // Early modes only (the per-run digit formatting and the nonce of a candidate):
    //   U's digit k sits at tail byte hi_end - 1 - k - (k >= hole ? hole_w : 0), the group's
    //   digit j at per-nonce-block byte g_last - j - (j >= g_hole), the innermost digit at byte
    //   `inner`; nonce(U, g, i) = spread(U, hole, hole_w) * u_mul + spread(g, g_hole, 1) * g_mul
    //   + i * i_mul, where spread(x, k, w) inserts w zero decimal digits at digit index k
    //   (k >= 20: x itself).
    uint32_t inner;
    uint32_t hole;
    uint32_t g_last;
    uint32_t g_hole;
    uint32_t hole_w;
    uint32_t pad_;        // 0; dev build: the coarse-hash word (keep_word above)
    uint64_t u_mul;
    uint64_t g_mul;
    uint64_t i_mul;
    uint32_t kw1[64];     // kModeTwo: K[i] + W[i] of tail block 1 (padding + length only)
    // Work queue: non-null -> the launch's workgroups claim chunks from this zeroed device
    // counter until it passes n_chunks, so an XCD that clocks faster takes more of them;
    // null -> workgroup b runs chunk b (grid = n_chunks).  DESIGN.md §3.
    uint32_t* counter;
};

// Arguments of the generic per-nonce kernels (range edges, small buckets,
// batch hashing): any nonce, any digit count, one nonce per lane.
struct GenArgs {
    uint32_t mid[8];      // chaining state before tail block 0
    uint32_t tail[16];    // the t prefix bytes of the tail, zero elsewhere
    uint64_t plen;        // len(msg) + 1 (bytes before the digits, all blocks)
    uint64_t first;       // scan: first nonce
    uint64_t count;       // scan: nonces in this launch
    uint32_t t;           // tail prefix length, 0..63
    uint32_t pad;         // 0; dev build: the coarse-hash word (keep_word above)
};

// ---- first-hit search (mh_search_first) ----
// Extra kernel parameters of the first-hit scan kernels (first_scan<J, MODE> of the
// build/fast_first.hsaco code object, generic_scan_first), after the product kernels' own two;
// FastArgs and GenArgs stay as they are.  A nonce's key is 0 if Hash <= target, else Hash: the
// lexicographic minimum of (key, nonce) is the smallest qualifying nonce, or without one the
// product's (Hash, nonce) minimum, so Partial, block_min and merge_partials serve unchanged.
struct FirstArgs {
    uint64_t target;
    unsigned long long* first;    // smallest qualifying nonce found so far; all ones: none yet
    unsigned long long* scanned;  // valid nonces of the chunks / workgroups that were not skipped
};

// ---- every hit (mh_search_hits) ----
// One qualifying nonce as the hits kernels append it and the host returns it (mh_hit).
struct Hit {
    uint64_t hash;
    uint64_t nonce;
};

// Extra kernel parameters of the hits kernels (hits_scan<J, MODE> of the build/fast_hits.hsaco
// code object, generic_scan_hits), after the product kernels' own two.  Every nonce of the range
// with Hash <= target takes one slot from *cursor -- a wave takes the slots of its step's hits
// with one atomic add -- and its {hash, nonce} goes to hits[slot] if slot < cap.  The cursor
// advances for every hit, stored or not, so its final value is the exact count.
struct HitsArgs {
    uint64_t target;
    unsigned long long* cursor;  // hits so far (zeroed by the host before the scan)
    Hit* hits;                   // cap entries, in the order the slots were taken
    uint64_t cap;
};

// ---- the first k hits (mh_search_first_hits) ----
// The range [lower, upper] (span = upper - lower) is cut into at most kFirstHitsSlices slices of
// 2^shift nonces, shift the smallest value with kFirstHitsSlices << shift >= span + 1; every hit
// that is appended also counts in its slice, and once the counts hold k hits the end of the first
// slice whose prefix sum reaches k is a nonce no larger nonce than which can belong to the k
// smallest hits: the bound the kernels publish (first_hits_bound) and skip or leave chunks by.
constexpr uint32_t kFirstHitsSlices = 1024;
constexpr uint32_t first_hits_shift(uint64_t span) {
    uint32_t shift = 0;
    while ((span >> shift) >= kFirstHitsSlices) ++shift;  // span >> shift < 1024  <=>  1024 << shift >= span + 1
    return shift;
}
constexpr uint32_t first_hits_slices(uint64_t span, uint32_t shift) { return (uint32_t)(span >> shift) + 1u; }
// The last nonce of slice s: lower + min(span, ((s + 1) << shift) - 1), without leaving 64 bits
// (the last slice's end is cut to the range's, and (s + 1) << shift is only formed below it).
constexpr uint64_t first_hits_slice_end(uint64_t lower, uint64_t span, uint32_t shift, uint32_t s) {
    return lower + ((uint64_t)s >= (span >> shift) ? span : (((uint64_t)s + 1u) << shift) - 1u);
}
// The value published from the slice counts counts[0 .. first_hits_slices): all ones while they
// sum to fewer than k.
constexpr uint64_t first_hits_bound(uint64_t lower, uint64_t span, uint32_t shift, uint64_t k, const uint32_t* counts) {
    uint64_t sum = 0;
    const uint32_t n = first_hits_slices(span, shift);
    for (uint32_t s = 0; s < n; ++s) {
        sum += counts[s];
        if (sum >= k) return first_hits_slice_end(lower, span, shift, s);
    }
    return ~0ull;
}

// Extra kernel parameters of the stopping hits kernels (hits_stop<J, MODE> of the
// build/fast_hits_stop.hsaco code object, generic_scan_hits_stop), after the product kernels' own
// two: a HitsArgs first, so the append reads it as hits_scan does, then the search's k, its bound
// word (all ones at the start, only ever lowered), the kFirstHitsSlices slice counters, the range
// the slices cut, and the count of nonces hashed.
struct HitsStopArgs {
    HitsArgs h;
    uint64_t k;
    unsigned long long* bound;    // whenever it holds B < 2^64-1, at least k hits of the range are <= B
    uint32_t* slices;             // kFirstHitsSlices counters, zeroed by the host
    uint64_t lower;
    uint64_t span;                // upper - lower
    uint32_t shift;
    uint32_t pad_;                // 0
    unsigned long long* scanned;  // nonces hashed
};

// ---- batched search (batch_scan / merge_segments) ----
// Many small Requests in one launch.  A lane's unit of work is an aligned decade, the ten nonces
// 10u .. 10u+9: they share their digit count, so u is formatted once for the ten.  A tile is one
// workgroup: kBlockThreads lanes x kBatchDecades decades = 2,560 nonces, one Partial.  One decade
// per lane, measured against 2 and 4 (HISTORY.md): a batch of a few small requests has too few
// larger tiles to fill the device, and a large batch runs as fast with small ones.
constexpr int kBatchDecades = 1;
constexpr uint32_t kBatchTileDecades = (uint32_t)kBlockThreads * (uint32_t)kBatchDecades;
constexpr uint32_t kBatchMaxRequests = 4096;  // requests (segments) of one pass
constexpr uint32_t kBatchMaxEntries = 8192;   // entries of one pass

// One generic piece of one request.  Its decades first/10 .. (first+count-1)/10 are cut into
// tiles of kBatchTileDecades; tile tile0 + k of the pass runs decades k * kBatchTileDecades ..
// of them and writes partials[slot0 + k].  Tiles are ordered by request; slot0 == tile0 unless the
// pass also holds fast pieces (BatchFastItem below), whose chunks take slots between the tiles'.
struct BatchEntry {
    GenArgs g;            // mid, tail, plen, t; first / count: the entry's nonces
    uint32_t tile0;       // first tile of the entry in its pass
    uint32_t slot0;       // first partial slot of the entry in its pass
};

// ---- fused fast pieces of a batch (batch_fast<J, MODE> of build/fast_batch.hsaco) ----
// One fast piece of one request of a pass of mh_search_batch_ex(MH_BATCH_FUSE_FAST).  The pieces of
// one layout (J, MODE) share a launch of batch_fast<J, MODE> with a static grid, one workgroup per
// 256-run chunk: workgroup b of the launch runs chunk b - chunk0 of the item chunk_item[b] names
// and writes partials[slot0 + b - chunk0].  args.counter is null and args.n_chunks the item's chunks.
constexpr uint32_t kBatchMaxFastItems = 1024;  // fast pieces of one pass
struct BatchFastItem {
    FastArgs args;
    uint32_t chunk0;      // first chunk of the item in its launch
    uint32_t slot0;       // first partial slot of the item in its pass
};
static_assert(sizeof(BatchFastItem) % 16 == 0, "items are laid out back to back in the pass's tables");

// ---- batched first-hit search (batch_scan_first / merge_segments_first) ----
// The device words of one request of a pass, in a table parallel to the segments; BatchEntry stays
// as it is, and entry_req[entry] (a table parallel to the entries) names the request.  The key is
// the request: two requests of one message and range with different targets have words of their
// own.  The initial values travel in the pass's table copy.
struct BatchFirstWords {
    uint64_t target;
    unsigned long long first;    // smallest qualifying nonce reported so far; all ones: none yet
    unsigned long long scanned;  // valid nonces of the tiles that were not skipped
};

// One request's result of a pass, as merge_segments_first writes it and the host copies it back.
struct BatchFirstResult {
    uint64_t hash, nonce, scanned;
};

// ---- fused fast pieces of a first-hit batch (batch_first<J, MODE> of build/fast_batch_first.hsaco) ----
// One fast piece of one request of a pass of mh_search_first_batch_ex(MH_BATCH_FUSE_FAST): a
// BatchFastItem with the request's first-hit parameters where first_scan's kernarg segment holds
// them -- FirstArgs one pointer behind FastArgs -- so the chunk body reaches them as it does there.
// f.first and f.scanned are device addresses into the request's BatchFirstWords, filled in by the
// host once it knows where the pass's tables go.  Workgroup b of the launch runs chunk
// order[b] - chunk0 of the item chunk_item[order[b]] names and writes partials[slot0 + that chunk].
struct BatchFirstItem {
    FastArgs args;
    Partial* unused;      // null; where first_scan's partials parameter sits
    FirstArgs f;
    uint32_t chunk0;      // first chunk of the item in its launch
    uint32_t slot0;       // first partial slot of the item in its pass
};
static_assert(sizeof(BatchFirstItem) % 16 == 0, "items are laid out back to back in the pass's tables");

// ---- batched hits (batch_scan_hits / merge_segments_hits) ----
// The device words of one request of a pass of mh_search_hits_batch, in a table parallel to the
// segments, found by a tile through entry_req[entry] as BatchFirstWords are.  Every nonce of the
// request with Hash <= target takes one slot from `cursor`, and its {hash, nonce} goes to entry
// offset + slot of the device hit buffer if slot < slots: the request's region, which the host
// hands out and checks (plan.hpp HitsBatchTables).  The cursor advances for every hit, stored or
// not, so it ends as the request's exact count.  Only the cursor is written on the device; the
// initial values (cursor = 0) travel in the pass's table copy.
struct BatchHitsWords {
    uint64_t target;
    unsigned long long cursor;
    uint64_t offset;
    uint64_t slots;
};

// One request's result of a pass, as merge_segments_hits writes it and the host copies it back.
struct BatchHitsResult {
    uint64_t hash, nonce, count;
};

// ---- fused fast pieces of a hits batch (batch_hits<J, MODE> of build/fast_batch_hits.hsaco) ----
// One fast piece of one request of a pass of mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST): a
// BatchFastItem with the request's hits parameters where hits_scan's kernarg segment holds them --
// HitsArgs one pointer behind FastArgs -- so the chunk body reaches them as it does there.  The host
// fills in the pointers once it knows where the pass's tables go: h.cursor is the device address of
// the request's BatchHitsWords::cursor, h.hits the request's region of the device hit buffer and
// h.cap the region's slots, so the fast pieces and the generic tiles of one request append through
// one cursor into one region.  Workgroup b of the launch runs chunk b - chunk0 of the item
// chunk_item[b] names and writes partials[slot0 + b - chunk0].
struct BatchHitsItem {
    FastArgs args;
    Partial* unused;      // null; where hits_scan's partials parameter sits
    HitsArgs h;
    uint32_t chunk0;      // first chunk of the item in its launch
    uint32_t slot0;       // first partial slot of the item in its pass
    uint32_t pad_[2];     // 0
};
static_assert(sizeof(BatchHitsItem) % 16 == 0, "items are laid out back to back in the pass's tables");

// ---- batched first k hits (batch_scan_bound / merge_segments_bound) ----
// The device words of one request of a pass of mh_search_first_hits_batch, in a table parallel to
// the segments, found by a tile through entry_req[entry] as BatchHitsWords are: BatchHitsWords'
// four (the append through `cursor` into the request's region), the request's k, its bound word
// (all ones at the start, only ever lowered: whenever it holds B < 2^64-1, at least k hits of the
// request are <= B), the range its slices cut (layout.hpp first_hits_shift / first_hits_slices of
// the request's own range) and the count of nonces hashed.  The request's kFirstHitsSlices slice
// counters sit at slices + request * kFirstHitsSlices of a buffer of the pass's own, zeroed before
// the pass.  cursor, bound and scanned are written on the device; the initial values (cursor = 0,
// bound = all ones, scanned = 0) travel in the pass's table copy.
struct BatchBoundWords {
    uint64_t target;
    unsigned long long cursor;
    uint64_t offset;
    uint64_t slots;
    uint64_t k;
    unsigned long long bound;
    uint64_t lower;
    uint64_t span;                // upper - lower
    uint32_t shift;
    uint32_t pad_;                // 0
    unsigned long long scanned;
};
static_assert(sizeof(BatchBoundWords) % 16 == 0, "the words are laid out back to back in the pass's tables");

// One request's result of a pass, as merge_segments_bound writes it and the host copies it back.
struct BatchBoundResult {
    uint64_t hash, nonce, count, scanned;
};

// ---- fused fast pieces of such a batch (batch_bound<J, MODE> of build/fast_batch_bound.hsaco) ----
// One fast piece of one request of a pass of mh_search_first_hits_batch(MH_BATCH_FUSE_FAST): a
// BatchFastItem with the request's parameters where hits_stop's kernarg segment holds them -- a
// HitsStopArgs one pointer behind FastArgs -- so the chunk body reaches them through the item as it
// reaches them through the kernarg segment there.  The host fills in the pointers once it knows
// where the pass's tables go: cursor, bound and scanned are the device addresses of the request's
// BatchBoundWords, h.h.hits and h.h.cap the request's region, h.slices the request's counters: the
// words its generic tiles use.  Workgroup b of the launch runs chunk order[b] - chunk0 of the item
// chunk_item[order[b]] names and writes partials[slot0 + that chunk].
struct BatchBoundItem {
    FastArgs args;
    Partial* unused;      // null; where hits_stop's partials parameter sits
    HitsStopArgs h;
    uint32_t chunk0;      // first chunk of the item in its launch
    uint32_t slot0;       // first partial slot of the item in its pass
};
static_assert(sizeof(BatchBoundItem) % 16 == 0, "items are laid out back to back in the pass's tables");

}  // namespace mh
