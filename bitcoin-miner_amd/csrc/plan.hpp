// plan.hpp -- host-side search planning for libminehip (no HIP dependency).
//
// Splits a Request range [lower, upper] (bitcoin/message.go:18-34) into
// kernel launches: per decimal-length bucket, the nonces that form whole runs
// of 10^L go to fast_search, the ragged edges and tiny buckets go to
// generic_scan.  The prefix "msg " is absorbed here into a SHA-256 midstate
// (the constant part of fmt.Sprintf("%s %d") at bitcoin/hash.go:15).
#pragma once
#include <stdint.h>
#include <stddef.h>

#include <functional>
#include <vector>

#include "layout.hpp"

namespace mh {

// Every full 64-byte block of P = msg ' ' compressed into mid; the rest of P
// is the tail.
struct Prefix {
    uint32_t mid[8];
    uint8_t tail[64];
    uint32_t t;     // len(P) mod 64
    uint64_t plen;  // len(P) = len(msg) + 1
};

void absorb_prefix(const uint8_t* msg, size_t len, Prefix* out);

// FIPS 180-4 compression on the host (midstates and the fixed schedule of a
// padding-only block).
void host_compress(uint32_t st[8], const uint32_t w16[16]);

// Hash(msg, nonce) of bitcoin/hash.go:13-17 on the host: one or two compressions past the
// prefix.  Not a search path (there is no CPU fallback): the scheduler checks one miner Result
// with it when miners hold several chunks (sched.hpp).
uint64_t host_hash(const uint8_t* msg, size_t len, uint64_t nonce);

// One launch of the plan.
struct Piece {
    uint64_t first;   // first nonce
    uint64_t count;   // nonces
    int kind;         // 0 fast, 1 generic
    int digits;
    int L;            // fast only
    int J;            // fast only
    int mode;         // fast only: FastMode
    int blocks;       // tail blocks of the final message
    uint32_t ops;     // fast only: nonce_cost(J, mode).ops
    uint32_t slots;   // fast only: nonce_cost(J, mode).slots
    FastArgs fa;      // kind 0
    GenArgs ga;       // both (generic launch args; also used by hash_batch)
};

struct PlanOpts {
    // L <= 3 (round 2: then with >= 2^21 runs per bucket) and up to 2^34 nonces (~67k
    // workgroups at L = 3) per launch.  With the issue-priority build the per-run work
    // (digit formatting, hoisted rounds, the first-nonce candidate scan, wave
    // start and the workgroup reduction) costs more than the longer tail of
    // 1,000-nonce lanes: +2% on configs[1], +5% / +4% on configs[2]'s halves,
    // +3% on configs[3] against L <= 2, 2^23 runs, 2^32-nonce launches, the
    // round-1 choice (profiles/r02ap_kbench_plan.json).
    int lower_digits = 3;                        // L upper bound (nonces per lane = 10^L)
    // Lower L until a bucket has min_lanes runs: 2^19 runs = 2,048 workgroups, about one generation
    // of the resident grid (7 x 256 CUs).  Round 4, with work queues and two streams, A/B in one
    // process against the round-2 2^21: configs[1] +1.4% (its d = 9 bucket now runs 1,000-nonce
    // lanes), configs[2] +0.4% / +0.6%; 2^16 (buckets of a fifth of a generation at L = 3) -4.7%
    // (profiles/r04c_kbench_min_lanes_*.json).
    uint64_t min_lanes = 1u << 19;
    // Nonces per fast launch: 2^35, so with the 2^17-workgroup cap one launch takes up to ~3.4e10
    // nonces at L = 3 (~0.6 s with one tail block).  A bucket's launches run back to back on the
    // high-priority stream and every boundary drains; round 4 against 2^34, A/B in one process: a
    // configs[3] step (5.5e10 nonces, 2 launches instead of 4) +0.52% / +0.58% on two boxes, a
    // 2-GPU shard +0.41%, configs[1] and [2] unchanged plans (profiles/r04r_kbench_launch_size_*.json).
    uint64_t max_nonces_per_launch = 1ull << 35;
    uint32_t max_blocks = 1u << 17;              // workgroups per launch (<= kMaxBlocksPerLaunch; +0.1% over 2^16)
    uint64_t generic_below = 1u << 20;           // a bucket this small goes to the generic kernel whole
    // Execution (minehip.cpp, not the plan itself): 1 = every piece on one stream in nonce
    // order; 2 = the pieces at the full L (coarse: 1,000-nonce lanes) on a high-priority
    // stream, the others (shorter lanes, generic edges) on a low-priority one, so that the
    // short workgroups back-fill the coarse launch's tail instead of each launch draining alone.
    // Tail split: the last fine_tail nonces (whole runs) of every bucket planned at the full L
    // go out as one more piece at L - 1 -- 100-nonce lanes whose workgroups end ~10x sooner --
    // so that the coarse launch's drain has short work to back-fill.  0: off.
    // Round 3 (profiles/r03d_*): 2 streams + a 2^28-nonce tail against one stream,
    // wall clock, A/B in one process: configs[1] +1.6%, configs[2] +1.0% / +1.1%, an 8-GPU
    // configs[3] shard +0.2%, and the predicted 8-GPU per-GPU efficiency 0.982 -> 1.00.
    int streams = 2;
    uint64_t fine_tail = 1ull << 28;
    // Work queue (execution): a fast launch's workgroups claim 256-run chunks from a counter
    // instead of one chunk each, so the 8 XCDs, whose clocks differ by a few percent, finish
    // together.  Round 3, A/B in one process against one chunk per workgroup
    // with the same code object: +0.6% to +1.9% on configs[1], configs[2]'s halves and the d = 10
    // bucket (profiles/r03u_*).  0: one workgroup per chunk.
    int queue = 1;
    // Innermost digit (execution of the plan's fast pieces): 1 = where a nonce costs
    // less with the digit ending the word before the last digit's enumerated innermost (the
    // kMode*Early layouts, layout.hpp), take that layout; 0 = always the last digit.
    int early = 1;
    // Round 4 A/B-rejected three more execution knobs and they were removed from the library in
    // round 5 (HISTORY.md §3): full-L pieces below 2^31 / 2^33 nonces on the low-priority stream
    // (-4% / -5%), a finest tail at L - 2 on a third stream (+-0.3%), and the tail split fused
    // into the coarse launch's work queue (-0.2% to -1.0%).
};

// Calls cb for every piece in increasing nonce order; stops early when cb
// returns false.  lower <= upper required.  A fast piece lies in one decimal
// bucket; a generic piece may span several (contiguous small buckets and
// edges are coalesced into one launch).
void plan_search(const Prefix& pre, uint64_t lower, uint64_t upper, const PlanOpts& opt,
                 const std::function<bool(const Piece&)>& cb);

// Generic-kernel arguments for this prefix (first/count left 0).
void make_gen_args(const Prefix& pre, GenArgs* ga);

// Algorithmic VALU instructions per nonce of a fast piece: the SHA-256 work
// that depends on the nonce's last digit (word J), with gfx950's 3-input ops
// (14 per round, 4 per sigma, add3 sums); work shared by a group or a run is
// amortised like the host midstate of SURVEY.md §8(d).  DESIGN.md §4.
uint32_t nonce_ops(int J, int mode);

// The same work in SIMD-32 issue slots (full-rate op 1, v_alignbit 2, one per
// addition) -- the unit of the roofline peak, 128 lanes/clk/CU.
struct NonceCost {
    uint32_t ops, slots;
};
NonceCost nonce_cost(int J, int mode);

int decimal_digits(uint64_t n);

// ---- relative search cost, for splitting a range over devices (mh_search_multi) ----
// One segment per decimal bucket of [lower, upper]: every nonce of [a, b] costs `per` issue slots
// -- the fast kernel's nonce_cost slots at the bucket's planned L (shorter lanes a few percent
// more), or kGenericSlotsPerBlock per tail block for a bucket the planner gives the generic
// kernel.  A device's rate in these units (slots per ns) does not depend on which layouts its
// range happened to hold, so rates measured on one range size the shards of the next.
struct CostSeg {
    uint64_t a, b;  // inclusive
    double per;
    // the bucket runs at the full L in a launch of many generations of workgroups (>= 2^21 runs):
    // its time follows `per`; the shorter-lane, few-generation and generic buckets run a few to
    // ~20% off the model (drains), so a device's rate is only measured on steady spans
    bool steady;
};
// Share of [lo, hi]'s cost in segments that are not steady.
double unsteady_share(const std::vector<CostSeg>& segs, uint64_t lo, uint64_t hi);
constexpr double kGenericSlotsPerBlock = 2.0 * 1760.0;  // estimate: a full compression + per-nonce formatting
constexpr double kUnsteadyFactor = 1.15;                 // fast buckets that are not steady (below)
void cost_segments(const Prefix& pre, uint64_t lower, uint64_t upper, const PlanOpts& opt,
                   std::vector<CostSeg>* out);
double segments_cost(const std::vector<CostSeg>& segs, uint64_t lo, uint64_t hi);

struct Span {
    uint64_t lo, hi;  // inclusive
    bool empty;
};
// Cut the segments' range into w.size() contiguous spans in order, span k carrying a share of the
// total cost proportional to w[k] (>= 0).  The spans tile the range exactly (integer cut
// positions); a span whose share rounds to no nonce is empty.
void split_by_cost(const std::vector<CostSeg>& segs, const std::vector<double>& w, std::vector<Span>* out);

// ---- batched search (mh_search_batch / mh_batch_plan) ----
// Many small Requests in one launch of batch_scan (layout.hpp BatchEntry).  plan_search runs per
// request: a request whose plan holds only generic pieces is fused, one entry per piece; one with
// a fast piece, or with more tiles or entries than a pass holds, is a fallback and runs through
// the single-search path afterwards.  A pass packs whole fused requests, in request order, until
// it runs out of partial slots (slot_cap), requests (kBatchMaxRequests) or entries
// (kBatchMaxEntries); a request never spans passes.
struct BatchRequest {
    Prefix pre;
    uint64_t lower, upper;  // lower <= upper
    uint64_t id;            // the caller's index of the request (BatchItem::req)
};

struct BatchItem {
    uint64_t req;           // BatchRequest::id
    uint64_t first, count;  // fused: the entry's nonces; fallback: the request's (count mod 2^64)
    int kind;               // 0 fused, 1 fallback
    int pass;               // fused: its pass, from 0; fallback: -1
    uint32_t slot, slots;   // fused: the entry's first partial slot in its pass and its tiles; fallback: 0
    size_t idx;             // position of the request in the array given to plan_batch
};

// Tiles of an entry: its aligned decades first/10 .. (first+count-1)/10 in tiles of
// kBatchTileDecades.  count >= 1 and first + (count - 1) <= 2^64 - 1.
uint64_t batch_tiles(uint64_t first, uint64_t count);

// One item per entry of a fused request and one per fallback request, in request order.
void plan_batch(const BatchRequest* reqs, size_t n, const PlanOpts& opt, uint32_t slot_cap,
                std::vector<BatchItem>* items);

// The device tables of one pass.
struct BatchTables {
    std::vector<BatchEntry> entries;
    std::vector<uint32_t> tile_entry;  // per tile: its entry
    std::vector<uint32_t> seg;         // per request of the pass: its first slot; then the pass's slot count
    std::vector<size_t> req_idx;       // per request of the pass: its position (BatchItem::idx)
    uint64_t nonces = 0;
};
// From the items of pass `pass` (items as plan_batch wrote them).
void build_batch_tables(const BatchRequest* reqs, const std::vector<BatchItem>& items, int pass, BatchTables* out);

// What batch_scan and merge_segments rely on, checked before every launch: slots within slot_cap,
// every tile's entry in range and the tile inside that entry's tiles, entries non-empty with
// exactly batch_tiles slots and no overflow of their last nonce, segments contiguous and
// non-empty and together all slots.
bool batch_tables_ok(const BatchTables& t, uint32_t slot_cap);

// ---- batched search with fused fast pieces (mh_search_batch_ex / mh_batch_plan_ex) ----
// plan_batch with MH_BATCH_FUSE_FAST: a request whose plan holds fast pieces is fused too, while its
// tiles and chunks fit one pass (slot_cap), its entries kBatchMaxEntries, its fast pieces
// kBatchMaxFastItems, and its nonce count is at most max_nonces; anything else is a fallback.  A
// fused request's pieces take one contiguous slot segment in nonce order: a generic piece
// batch_tiles slots, a fast piece one slot per 256-run chunk.  The fast pieces of a pass are grouped
// by layout (J, mode), one launch of batch_fast<J, mode> per group, the groups in the order their
// layouts first appear; inside a launch the pieces are ordered longest lanes first (L descending,
// then request order).
// Lanes: every request keeps its own plan's (shared_lanes false, the library's default).  The
// batch-aware rule (shared_lanes; MINEHIP_BATCH_FAST_LANES=shared) plans the candidates -- the
// requests whose own plan (opt) holds a fast piece and which pass the size cap -- with min_lanes =
// batch_min_lanes(opt.min_lanes, their number): the other requests of the call fill the device, so
// a request could afford longer lanes than alone.  Measured, it did not win.
constexpr uint64_t kBatchFastMaxNonces = 1000000000ull;  // default max_nonces, MH_BATCH_FAST_MAX_NONCES (measured)
uint64_t batch_min_lanes(uint64_t min_lanes, size_t fast_requests);

struct BatchPiece {
    uint64_t req;           // BatchRequest::id
    uint64_t first, count;  // the piece's nonces; fallback: the request's (count mod 2^64)
    int kind;               // 0 fused generic entry, 1 fallback, 2 fused fast piece
    int pass;               // fallback: -1
    uint32_t slot, slots;   // first partial slot in the pass; tiles (kind 0) or chunks (kind 2)
    int J, mode, L;         // kind 2; else 0
    int launch;             // kind 2: its batch_fast launch within the pass; else -1
    uint32_t chunk0;        // kind 2: its first chunk within that launch
    size_t idx;             // position of the request in the array given to plan_batch_ex
    uint32_t ops, nslots;   // kind 2: nonce_cost(J, mode)
    size_t fa;              // kind 2: its launch arguments, args[fa] (counter null, n_chunks = slots)
};
void plan_batch_ex(const BatchRequest* reqs, size_t n, const PlanOpts& opt, uint32_t slot_cap, bool shared_lanes,
                   uint64_t max_nonces, std::vector<BatchPiece>* pieces, std::vector<FastArgs>* args);

// The device tables of one pass: BatchTables (entries with slot0 apart from tile0; seg over tiles
// and chunks together), the fast items in launch order and, per launch, its chunks' items.
struct BatchFastLaunch {
    int J, mode;
    uint32_t item0, items;    // its items in BatchFastTables::items
    uint32_t chunk0, chunks;  // its part of BatchFastTables::chunk_item
};
struct BatchFastTables {
    std::vector<BatchFastItem> items;
    std::vector<uint32_t> chunk_item;  // per launch, per chunk: its item (index into items)
    std::vector<BatchFastLaunch> launches;
    std::vector<size_t> piece;         // per item: its BatchPiece (index into the plan)
};
void build_batch_tables_ex(const BatchRequest* reqs, const std::vector<BatchPiece>& pieces,
                           const std::vector<FastArgs>& args, int pass, BatchTables* t, BatchFastTables* f);

// What batch_scan, batch_fast and merge_segments rely on, checked before every launch of a pass:
// every tile maps to an entry and lies inside its tiles, every chunk maps to an item of its launch's
// layout and lies inside that item's n_chunks, every item's lanes cover exactly its runs, every slot
// of every segment is written by exactly one tile or chunk, the segments are contiguous, non-empty
// and together all slots, and nothing lies beyond slot_cap.
bool batch_tables_ex_ok(const BatchTables& t, const BatchFastTables& f, uint32_t slot_cap);

// ---- batched first-hit search (mh_search_first_batch / mh_first_batch_order) ----
// The tables batch_scan_first reads beside a pass's BatchTables (the plan does not depend on the
// targets, so plan_batch and build_batch_tables serve unchanged).
struct FirstBatchTables {
    std::vector<uint32_t> entry_req;  // per entry: its request of the pass (index into seg / req_idx)
    std::vector<uint32_t> order;      // per workgroup: the tile (= partial slot) it runs
};
// rank_major: tile 0 of every request of the pass in request order, then tile 1 of every request
// that has one, and so on -- a request's rank counts across its entries in nonce order, i.e. along
// its slot segment -- so that a pass of many requests hashes each request's lowest nonces first;
// otherwise the identity (request-major) order.
void build_first_batch_tables(const BatchTables& t, bool rank_major, FirstBatchTables* out);

// Checked before every launch, after batch_tables_ok(t): every entry's request is the one whose
// segment holds the entry's slots, and order is a permutation of the pass's tiles.
bool first_batch_tables_ok(const BatchTables& t, const FirstBatchTables& f);

// ---- batched first-hit search with fused fast pieces (mh_search_first_batch_ex) ----
// The plan is plan_batch_ex's and the tables build_batch_tables_ex's (the targets play no part in
// either); these are the tables batch_scan_first_slots and batch_first<J, MODE> read beside them.
struct FirstBatchFastTables {
    std::vector<uint32_t> entry_req;    // per entry: its request of the pass (index into seg / req_idx)
    std::vector<uint32_t> item_req;     // per fast item: likewise
    std::vector<uint32_t> tile_order;   // per workgroup of the generic launch: the tile it runs
    std::vector<uint32_t> chunk_order;  // per launch (laid out as chunk_item), per workgroup: the chunk of the launch it runs
};
// rank_major: the generic launch runs tile 0 of every request that has one, in request order, then
// tile 1 of every request that has one, and so on (a request's tiles counted across its entries in
// nonce order); a batch_first launch runs chunk 0 of every item in item order, then chunk 1 of
// every item that has one, and so on.  Otherwise both are the identity.
void build_first_batch_tables_ex(const BatchTables& t, const BatchFastTables& f, bool rank_major,
                                 FirstBatchFastTables* out);

// Checked before every pass: batch_tables_ex_ok(t, f, slot_cap); every entry's and every item's
// request is the one whose segment holds all of that entry's or item's slots; tile_order is a
// permutation of the pass's tiles and every launch's part of chunk_order one of that launch's chunks.
bool first_batch_tables_ex_ok(const BatchTables& t, const BatchFastTables& f, const FirstBatchFastTables& x,
                              uint32_t slot_cap);

// The partial slot a workgroup's tile (launch < 0) or chunk of launch `launch` writes, for the
// order tables as slots (mh_first_batch_order_ex); the tables have passed the check above.
uint32_t first_batch_order_slot(const BatchTables& t, const BatchFastTables& f, int launch, uint32_t v);

// Host form of the kernels' chunk_floor (fast_search.hip): no nonce of chunk blk of the piece is
// smaller, and lane 0's first nonce attains it.  Last-digit layouts: (u_start + 256 blk) * 10^L;
// Early layouts: spread(u_start + 256 blk, hole, hole_w) * u_mul.
uint64_t chunk_floor_host(const FastArgs& a, uint32_t blk);

// ---- batched hits (mh_search_hits_batch / mh_hits_batch_regions) ----
// The tables batch_scan_hits reads beside a pass's BatchTables (the plan depends neither on the
// targets nor on the caps, so plan_batch and build_batch_tables serve unchanged), and the schedule
// of the passes: which ones start after a drain.  The device hit buffer is handed out in windows:
// between two drains the fused requests of the passes in flight own disjoint regions of it, in
// request order.
struct HitsRegion {
    uint64_t offset, slots;  // entries offset .. offset + slots - 1 of the device hit buffer
};
struct HitsBatchTables {
    std::vector<uint32_t> entry_req;  // per entry: its request of the pass (index into seg / req_idx)
    std::vector<HitsRegion> region;   // per request of the pass
};
// What the passes in flight may use before a drain empties it all: bytes of the table buffer,
// results, and entries of the device hit buffer (window_slots >= 1).
struct HitsBatchLimits {
    size_t table_bytes, results;
    uint64_t window_slots;
};
// In use since the last drain, and how many drains there were.
struct HitsBatchState {
    size_t toff = 0, nres = 0;
    uint64_t used = 0;
    int window = 0;
};
// Bytes of one pass's tables in the table buffer: entries, segments, per-tile entry, per-entry
// request, per-request words, each aligned to 16 bytes.
size_t hits_batch_table_bytes(size_t entries, size_t requests, size_t tiles);
// A drain: everything in flight is home, the next window starts.
void hits_batch_drained(HitsBatchState* st);
// Plan pass `t` behind the passes in *st: it starts after a drain (the return value; *st is then
// hits_batch_drained first) when its tables or results do not fit behind those in flight, or when
// its requests want more slots than the window has left and the window is not empty -- a request
// wants min(cap, its nonce count), caps[BatchItem::idx] being its cap.  Then, in request order,
// request r gets slots = min(cap, its nonce count, slots left in the window) at the next free
// offset, and *st advances.  A request that got fewer slots than it has hits is rebuilt by the
// caller (minehip.cpp).
bool plan_hits_batch_pass(const BatchTables& t, const BatchRequest* reqs, const uint64_t* caps,
                          const HitsBatchLimits& lim, HitsBatchState* st, HitsBatchTables* out);
// Checked before every launch, after batch_tables_ok(t): every entry's request is the one whose
// segment holds the entry's slots; one region per request of the pass, each no larger than its
// request's nonce count, in order and disjoint, none below used_before (where the regions of the
// window's earlier passes end) and none beyond window_slots.
bool hits_batch_tables_ok(const BatchTables& t, const BatchRequest* reqs, const HitsBatchTables& h,
                          uint64_t used_before, uint64_t window_slots);

// ---- batched hits with fused fast pieces (mh_search_hits_batch_ex / mh_hits_batch_regions_ex) ----
// The plan is plan_batch_ex's and the tables build_batch_tables_ex's (targets and caps play no part
// in either); these are the tables batch_scan_hits_slots and batch_hits<J, MODE> read beside them.
// Windows, regions and drains are plan_hits_batch_pass's; the pass's items (BatchHitsItem each) and
// per-chunk item table count against the table buffer too.
struct HitsBatchFastTables {
    HitsBatchTables h;               // per entry its request; per request its region
    std::vector<uint32_t> item_req;  // per fast item: its request of the pass (index into seg / req_idx)
};
// Bytes of such a pass's tables: hits_batch_table_bytes, the items, the per-chunk item table.
size_t hits_batch_table_bytes_ex(size_t entries, size_t requests, size_t tiles, size_t items, size_t chunks);
// plan_hits_batch_pass with those bytes, and the items' requests.
bool plan_hits_batch_pass_ex(const BatchTables& t, const BatchFastTables& f, const BatchRequest* reqs,
                             const uint64_t* caps, const HitsBatchLimits& lim, HitsBatchState* st,
                             HitsBatchFastTables* out);
// Checked before every pass: batch_tables_ex_ok(t, f, slot_cap), hits_batch_tables_ok(t, reqs, x.h,
// used_before, window_slots), and every entry's and every item's request is the one whose segment
// holds all of that entry's or item's slots -- so a tile or chunk appends through the cursor, into
// the region, of the request whose segment its partial goes to.
bool hits_batch_tables_ex_ok(const BatchTables& t, const BatchFastTables& f, const BatchRequest* reqs,
                             const HitsBatchFastTables& x, uint32_t slot_cap, uint64_t used_before,
                             uint64_t window_slots);

// ---- batched first k hits (mh_search_first_hits_batch / mh_first_hits_batch_regions) ----
// The plan is plan_batch's or plan_batch_ex's and the tables build_batch_tables[_ex]'s (targets and
// k play no part in either; a pass without fast pieces has an empty BatchFastTables).  Windows,
// regions and drains are plan_hits_batch_pass's with a want per request in the cap's place: a
// request of k wants min(its nonce count, first_hits_batch_want(k)) entries of the device hit
// buffer -- room for the hits appended before the bound takes effect -- and gets what the window has
// left of that.  Neither constant affects a returned entry: a request that appends more than its
// region holds is rebuilt by the caller.
constexpr uint64_t kFirstHitsBatchFactor = 4, kFirstHitsBatchFloor = 256;
constexpr uint64_t first_hits_batch_want(uint64_t k) {
    return k * kFirstHitsBatchFactor > kFirstHitsBatchFloor ? k * kFirstHitsBatchFactor : kFirstHitsBatchFloor;
}
struct FirstHitsBatchTables {
    FirstBatchFastTables o;          // per entry and per item its request; the tile and chunk orders
    std::vector<HitsRegion> region;  // per request of the pass
};
// Where the tables of one pass lie in its image, each aligned to 16 bytes: entries, segments,
// per-tile entry, per-entry request, tile order, per-request words (BatchBoundWords), items
// (BatchBoundItem), per-chunk item, chunk order.
struct FirstHitsBatchLayout {
    size_t o_seg, o_tile, o_ereq, o_order, o_words, o_item, o_chunk, o_corder, bytes;
};
FirstHitsBatchLayout first_hits_batch_layout(size_t entries, size_t requests, size_t tiles, size_t items, size_t chunks);
// plan_hits_batch_pass_ex with those bytes and the wants (wants[BatchPiece::idx], as caps there),
// plus the order tables of the first-hit batch (build_first_batch_tables_ex).
bool plan_first_hits_batch_pass(const BatchTables& t, const BatchFastTables& f, const BatchRequest* reqs,
                                const uint64_t* wants, const HitsBatchLimits& lim, bool rank_major,
                                HitsBatchState* st, FirstHitsBatchTables* out);
// Checked before every pass: batch_tables_ok (no fast piece) or batch_tables_ex_ok, the regions as
// hits_batch_tables_ok checks them, every entry's and item's request the one whose segment holds all
// of its slots, the orders permutations (first_batch_tables_ex_ok's conditions), and no more
// requests than a pass's slice counters serve (kBatchMaxRequests).
bool first_hits_batch_tables_ok(const BatchTables& t, const BatchFastTables& f, const BatchRequest* reqs,
                                const FirstHitsBatchTables& x, uint32_t slot_cap, uint64_t used_before,
                                uint64_t window_slots);
// The device addresses an image is built for: where the image itself goes, the device hit buffer
// and the pass's slice counters (kFirstHitsSlices per request of a pass).
struct FirstHitsBatchAddrs {
    uint64_t image, hits, slices;
};
// Write the pass's image (first_hits_batch_layout(...).bytes bytes at `image`): the tables, the
// requests' words with their initial values (cursor 0, bound all ones, scanned 0; the slicing of
// the request's own range) and the items, each with the device addresses of its request's words,
// region and counters.  targets and ks are indexed as wants (BatchPiece::idx).
void build_first_hits_batch_image(const BatchTables& t, const BatchFastTables& f, const FirstHitsBatchTables& x,
                                  const BatchRequest* reqs, const uint64_t* targets, const uint64_t* ks,
                                  const FirstHitsBatchAddrs& at, uint8_t* image);
// Checked on the image before it is copied: every request's words hold its region, its own range's
// slicing, 1 <= k and the initial values; every item's target, k, range and slicing are its
// request's words', its cursor, bound and scanned pointers the addresses of those words, its region
// its request's and inside the hit buffer's window, its counters its request's kFirstHitsSlices --
// so the counters of different requests never overlap -- and the order tables are the checked ones.
bool first_hits_batch_image_ok(const BatchTables& t, const BatchFastTables& f, const FirstHitsBatchTables& x,
                               const BatchRequest* reqs, const FirstHitsBatchAddrs& at, uint64_t window_slots,
                               const uint8_t* image);
// The host's reading of one fused request after a drain: `got` holds the min(count, slots) entries
// its region kept.  count > slots: false (which entries were kept depends on timing; the caller
// rebuilds the request).  Otherwise the entries are sorted by nonce, *stored = min(count, k), and
// with stored == k {*hash, *nonce} is the minimum of the first k; with stored < k it is left to the
// caller (the merged minimum; scanned must then be the whole range).
bool read_first_hits_batch(Hit* got, uint64_t count, uint64_t slots, uint64_t k, uint64_t* stored, uint64_t* hash,
                           uint64_t* nonce);

}  // namespace mh
