// minehip.cpp -- C-ABI of libminehip.so (declared in include/minehip.h).
//
// Per device: one HIP stream, a partials buffer, a 16-byte running minimum
// and a pinned 16-byte host slot, created on first use and reused by every
// call.  A search enqueues all of its launches (fast runs, generic edges,
// merges) on that stream and synchronises once, when it copies the 16-byte
// result back.  No CPU fallback exists: without a gfx950 device the calls fail
// with MH_ENODEV.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../include/minehip.h"
#include "../../include/minehip_server.h"
#include "layout.hpp"
#include "msgcodec.hpp"
#include "multi.hpp"
#include "plan.hpp"
#include "sched.hpp"

namespace mh {
hipError_t fast_module_init(int dev);
#ifdef MH_DEV_HOOKS
hipError_t fast_keep_ok(int dev, bool* ok);
hipError_t set_hash_xor(int dev, uint64_t x, hipStream_t s, bool* fast_ok);
#endif
hipError_t launch_fast(int dev, int J, int mode, const FastArgs& a, Partial* partials, hipStream_t s);
hipError_t launch_generic_scan(const GenArgs& a, Partial* partials, uint32_t blocks, hipStream_t s);
hipError_t launch_hash_batch(const GenArgs& a, const uint64_t* d_nonces, uint64_t* d_out, uint64_t n,
                             hipStream_t s);
hipError_t launch_merge(const Partial* partials, uint32_t n, Partial* best, hipStream_t s);
hipError_t launch_fast_first(int dev, int J, int mode, const FastArgs& a, Partial* partials, const FirstArgs& f,
                             bool stop, hipStream_t s);
hipError_t launch_generic_scan_first(const GenArgs& a, Partial* partials, uint32_t blocks, const FirstArgs& f,
                                     hipStream_t s);
hipError_t launch_finish_first(const GenArgs& a, const Partial* best, const unsigned long long* scanned, uint64_t* out,
                               hipStream_t s);
hipError_t launch_fast_hits(int dev, int J, int mode, const FastArgs& a, Partial* partials, const HitsArgs& h,
                            hipStream_t s);
hipError_t launch_generic_scan_hits(const GenArgs& a, Partial* partials, uint32_t blocks, const HitsArgs& h,
                                    hipStream_t s);
hipError_t launch_fast_hits_stop(int dev, int J, int mode, const FastArgs& a, Partial* partials, const HitsStopArgs& h,
                                 hipStream_t s);
hipError_t launch_generic_scan_hits_stop(const GenArgs& a, Partial* partials, uint32_t blocks, const HitsStopArgs& h,
                                         hipStream_t s);
hipError_t launch_batch_scan(const BatchEntry* entries, const uint32_t* tile_entry, Partial* partials, uint32_t tiles,
                             hipStream_t s);
hipError_t launch_merge_segments(const Partial* partials, const uint32_t* seg, Partial* results, uint32_t requests,
                                 hipStream_t s);
hipError_t launch_batch_scan_slots(const BatchEntry* entries, const uint32_t* tile_entry, Partial* partials,
                                   uint32_t tiles, hipStream_t s);
hipError_t launch_batch_fast(int dev, int J, int mode, const BatchFastItem* items, const uint32_t* chunk_item,
                             Partial* partials, uint32_t chunks, hipStream_t s);
#ifdef MH_DEV_HOOKS
hipError_t batch_fast_hooks(int dev, uint64_t x, hipStream_t s, bool* keep_ok, bool* xor_ok);
#endif
hipError_t launch_batch_scan_first(const BatchEntry* entries, const uint32_t* tile_entry, const uint32_t* entry_req,
                                   const uint32_t* order, BatchFirstWords* words, Partial* partials, uint32_t tiles,
                                   hipStream_t s);
hipError_t launch_merge_segments_first(const Partial* partials, const uint32_t* seg, const BatchEntry* entries,
                                       const uint32_t* tile_entry, const BatchFirstWords* words,
                                       BatchFirstResult* results, uint32_t requests, hipStream_t s);
hipError_t launch_batch_scan_first_slots(const BatchEntry* entries, const uint32_t* tile_entry,
                                         const uint32_t* entry_req, const uint32_t* order, BatchFirstWords* words,
                                         Partial* partials, uint32_t tiles, hipStream_t s);
hipError_t launch_merge_segments_first_ex(const Partial* partials, const uint32_t* seg, const GenArgs* req_gen,
                                          const BatchFirstWords* words, BatchFirstResult* results, uint32_t requests,
                                          hipStream_t s);
hipError_t launch_batch_first(int dev, int J, int mode, const BatchFirstItem* items, const uint32_t* chunk_item,
                              const uint32_t* order, Partial* partials, uint32_t chunks, hipStream_t s);
hipError_t launch_batch_stop(int dev, int J, int mode, const BatchFirstItem* items, const uint32_t* chunk_item,
                             const uint32_t* order, Partial* partials, uint32_t chunks, hipStream_t s);
hipError_t launch_batch_scan_hits(const BatchEntry* entries, const uint32_t* tile_entry, const uint32_t* entry_req,
                                  BatchHitsWords* words, Hit* hits, Partial* partials, uint32_t tiles,
                                  hipStream_t s);
hipError_t launch_batch_scan_hits_slots(const BatchEntry* entries, const uint32_t* tile_entry, const uint32_t* entry_req,
                                        BatchHitsWords* words, Hit* hits, Partial* partials, uint32_t tiles,
                                        hipStream_t s);
hipError_t launch_batch_hits(int dev, int J, int mode, const BatchHitsItem* items, const uint32_t* chunk_item,
                             Partial* partials, uint32_t chunks, hipStream_t s);
hipError_t launch_batch_scan_bound(bool slots, const BatchEntry* entries, const uint32_t* tile_entry,
                                   const uint32_t* entry_req, const uint32_t* order, BatchBoundWords* words,
                                   uint32_t* slices, Hit* hits, Partial* partials, uint32_t tiles, hipStream_t s);
hipError_t launch_batch_bound(int dev, int J, int mode, const BatchBoundItem* items, const uint32_t* chunk_item,
                              const uint32_t* order, Partial* partials, uint32_t chunks, hipStream_t s);
hipError_t launch_merge_segments_bound(const Partial* partials, const uint32_t* seg, const BatchBoundWords* words,
                                       const Hit* hits, Hit* packed, uint64_t limit, const unsigned long long* base_in,
                                       unsigned long long* base_out, BatchBoundResult* results, uint32_t requests,
                                       hipStream_t s);
hipError_t launch_merge_segments_hits(const Partial* partials, const uint32_t* seg, const BatchHitsWords* words,
                                      const Hit* hits, Hit* packed, uint64_t limit, const unsigned long long* base_in,
                                      unsigned long long* base_out, BatchHitsResult* results, uint32_t requests,
                                      hipStream_t s);
}  // namespace mh

namespace {

using mh::Partial;

thread_local std::string g_err;

int fail(int code, const std::string& what) {
    g_err = what;
    return code;
}

}  // namespace

namespace mh {
int set_error(int code, const char* what) { return fail(code, what); }
}  // namespace mh

namespace {

#define MH_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return fail(MH_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

constexpr uint64_t kBatchChunk = 1u << 22;  // nonces per hash_batch transfer
constexpr int kEventPairs = 512;             // profiled launches buffered before harvesting
constexpr uint32_t kQueueSlots = 4096;       // work-queue counters per search (one per fast launch)
constexpr size_t kBatchTableBytes = 4u << 20;  // device tables (and their pinned staging) of the batch passes in flight
constexpr uint32_t kBatchResults = 1u << 16;   // results of the batch passes in flight
// Tables of the first-hit passes with fused fast pieces in flight, a buffer of their own: such a pass
// carries two words per slot (its item or entry, and the order), a GenArgs and the words per request
// and 560-byte items, at most 8 * 2^18 + 8,192 * 136 + 4,096 * (128 + 24 + 4) + 1,024 * 560 + 8,192 * 4
// = ~4.3 MiB, more than kBatchTableBytes
// (the passes of mh_search_first_hits_batch use the same buffer: no GenArgs per request, 80-byte words
// and 624-byte items, at most 8 * 2^18 + 8,192 * 140 + 4,097 * 4 + 4,096 * 80 + 1,024 * 624 = ~4.1 MiB)
constexpr size_t kFirstBatchFastTableBytes = 5u << 20;
// the largest pass of either kind fits: its tiles and chunks share kMaxBlocksPerLaunch slots (two
// words each), plus every per-entry, per-request and per-item table at its limit and 16 bytes of
// alignment for each of the nine tables
static_assert(8u * (size_t)mh::kMaxBlocksPerLaunch + mh::kBatchMaxEntries * (sizeof(mh::BatchEntry) + 4u) +
                      (mh::kBatchMaxRequests + 1u) * 4u +
                      mh::kBatchMaxRequests * (sizeof(mh::GenArgs) + sizeof(mh::BatchFirstWords)) +
                      mh::kBatchMaxFastItems * sizeof(mh::BatchFirstItem) + 9u * 16u <= kFirstBatchFastTableBytes,
              "a first-hit pass with fast pieces fits its table buffer");
static_assert(8u * (size_t)mh::kMaxBlocksPerLaunch + mh::kBatchMaxEntries * (sizeof(mh::BatchEntry) + 4u) +
                      (mh::kBatchMaxRequests + 1u) * 4u + mh::kBatchMaxRequests * sizeof(mh::BatchBoundWords) +
                      mh::kBatchMaxFastItems * sizeof(mh::BatchBoundItem) + 9u * 16u <= kFirstBatchFastTableBytes,
              "a first-k-hits pass fits its table buffer");

struct Timed {
    hipEvent_t start = nullptr, stop = nullptr;
    int kind;  // 0 fast, 1 generic
    int var;   // fast: kernel variant and lane length, var_index(J, mode, L)
};

// per fast_search<J, MODE> variant: launches, nonces, ns, algorithmic instructions
struct VarStat {
    uint64_t launches = 0, nonces = 0, ns = 0, ops = 0, slots = 0;
};
constexpr int kVariants = 16 * mh::kModes * 5;  // J < 16, mode < kModes, L = 1..5
inline int var_index(int J, int mode, int L) { return J + 16 * mode + 16 * mh::kModes * (L - 1); }

struct DevCtx {
    std::mutex mu;
    int dev = -1;
    bool ready = false;
    hipStream_t stream = nullptr;              // every search's merge and copy; pieces with streams = 1
    // streams = 2: the pieces' streams, by priority: [0] coarse pieces (high), [1] the other pieces (low)
    hipStream_t ps[2] = {nullptr, nullptr};
    hipEvent_t ev_piece[2] = {nullptr, nullptr};  // each piece stream's work so far
    hipEvent_t ev_main = nullptr;                          // the main stream's (reset / merge)
    Partial* d_partials = nullptr;
    Partial* d_best = nullptr;
    Partial* h_best = nullptr;  // pinned
    uint64_t* d_nonces = nullptr;
    uint64_t* d_hashes = nullptr;
    uint32_t poff = 0;  // partials written since the last merge
    uint32_t* d_counters = nullptr;  // work-queue counters, zeroed at each search's start
    uint32_t qoff = 0;               // counters used by this search
    // batched search (mh_search_batch), allocated by the first batch call
    uint8_t* d_btab = nullptr;  // the passes' tables: entries, segments, per-tile entry index
    uint8_t* h_btab = nullptr;  // pinned staging of the same bytes
    Partial* d_bres = nullptr;  // one result per request of the passes in flight
    Partial* h_bres = nullptr;  // pinned
    // batched first-hit search (mh_search_first_batch), allocated by the first such call
    mh::BatchFirstResult* d_fres = nullptr;  // one result per request of the passes in flight
    mh::BatchFirstResult* h_fres = nullptr;  // pinned
    // ... with fused fast pieces (mh_search_first_batch_ex), allocated by the first such call that fuses one
    uint8_t* d_ftab = nullptr;  // the passes' tables (first_batch_run_pass_ex)
    uint8_t* h_ftab = nullptr;  // pinned staging of the same bytes
    // first-hit search (mh_search_first), allocated by the first such call
    uint64_t* d_first = nullptr;  // [0] smallest qualifying nonce so far, [1] nonces scanned, [2..4] the result
    uint64_t* h_first = nullptr;  // pinned: hash, nonce, scanned
    const mh::FirstArgs* first = nullptr;  // set while an mh_search_first enqueues its pieces
    bool first_stop = false;               // ... of mh_search_first_ex(MH_FIRST_STOP_RUNNING): stop_scan for first_scan
    // every hit (mh_search_hits), allocated by the first such call
    mh::Hit* d_hits = nullptr;      // MH_HITS_MAX_CAP entries
    uint64_t* d_hcursor = nullptr;  // hits of the scan in flight
    uint64_t* h_hcursor = nullptr;  // pinned
    const mh::HitsArgs* hits = nullptr;  // set while an mh_search_hits enqueues its pieces
    // the first k hits (mh_search_first_hits), allocated by the first such call; the hit buffer and the cursor are mh_search_hits'
    uint64_t* d_fhits = nullptr;    // [0] the bound word, [1] nonces scanned
    uint32_t* d_slices = nullptr;   // kFirstHitsSlices slice counters
    uint64_t* h_fhits = nullptr;    // pinned: the scanned count
    const mh::HitsStopArgs* hits_stop = nullptr;  // set while an mh_search_first_hits enqueues its pieces
    // batched hits (mh_search_hits_batch), allocated by the first such call; the hit buffer is d_hits
    mh::BatchHitsResult* d_hres = nullptr;  // one result per request of the passes in flight
    mh::BatchHitsResult* h_hres = nullptr;  // pinned
    mh::Hit* d_hpacked = nullptr;   // MH_HITS_MAX_CAP entries: what the regions of a window kept, packed by the merges
    uint64_t* d_hbase = nullptr;    // two words: entries packed by the window's passes so far (written and read in turn)
    // batched first k hits (mh_search_first_hits_batch), allocated by the first such call; the hit buffer, the packed
    // entries and the base words are mh_search_hits_batch's, the tables' buffer mh_search_first_batch_ex's
    mh::BatchBoundResult* d_kres = nullptr;  // one result per request of the passes in flight
    mh::BatchBoundResult* h_kres = nullptr;  // pinned
    uint32_t* d_bslices = nullptr;           // kFirstHitsSlices counters per request of one pass (kBatchMaxRequests of them)
#ifdef MH_DEV_HOOKS
    uint32_t keep = 0;        // this call's coarse-hash word (MINEHIP_DEV_HASH_KEEP; 0: unset)
    bool keep_fast = false;   // ... and the fast code object in use is the variant that reads it
    bool xor_on = false;      // this call XORs every hash with a constant (MINEHIP_DEV_HASH_XOR, non-zero)
    bool xor_fast = false;    // ... and the fast code object in use has the word its kernels read it from
#endif
    // profiling
    bool prof = false;
    std::vector<Timed> pool;
    int used = 0;
    uint64_t cnt[8] = {0};
    VarStat var[kVariants];
};

std::mutex g_tab_mu;
std::vector<std::unique_ptr<DevCtx>> g_tab;
int g_ndev = -1;

int device_count_impl() {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    if (g_ndev < 0) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        g_ndev = n;
        g_tab.resize((size_t)n);
        for (auto& p : g_tab) p.reset(new DevCtx());
    }
    return g_ndev;
}

// Returns the context for dev, initialised, with its mutex NOT held.
int get_ctx(int dev, DevCtx** out) {
    const int n = device_count_impl();
    if (n <= 0) return fail(MH_ENODEV, "no HIP device visible");
    if (dev < 0 || dev >= n) return fail(MH_EINVAL, "device index out of range");
    DevCtx* c = g_tab[(size_t)dev].get();
    *out = c;
    return MH_OK;
}

int init_locked(DevCtx* c, int dev) {
    if (c->ready) return MH_OK;
    MH_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    MH_HIP(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MH_ENODEV, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    // each resource only once: a call after a failed init (e.g. the code object
    // did not load) resumes where that one stopped instead of allocating again
    if (!c->stream) MH_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (!c->ps[0] || !c->ps[1]) {
        int least = 0, greatest = 0;
        MH_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));  // gfx950: 1 .. -1
        if (!c->ps[0]) MH_HIP(hipStreamCreateWithPriority(&c->ps[0], hipStreamNonBlocking, greatest));
        if (!c->ps[1]) MH_HIP(hipStreamCreateWithPriority(&c->ps[1], hipStreamNonBlocking, least));
    }
    for (auto& e : c->ev_piece)
        if (!e) MH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (!c->ev_main) MH_HIP(hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming));
    if (!c->d_partials) MH_HIP(hipMalloc(&c->d_partials, sizeof(Partial) * mh::kMaxBlocksPerLaunch));
    if (!c->d_best) MH_HIP(hipMalloc(&c->d_best, sizeof(Partial)));
    if (!c->d_counters) MH_HIP(hipMalloc(&c->d_counters, sizeof(uint32_t) * kQueueSlots));
    if (!c->h_best) MH_HIP(hipHostMalloc(&c->h_best, sizeof(Partial), hipHostMallocDefault));
    if (!c->d_nonces) MH_HIP(hipMalloc(&c->d_nonces, sizeof(uint64_t) * kBatchChunk));
    if (!c->d_hashes) MH_HIP(hipMalloc(&c->d_hashes, sizeof(uint64_t) * kBatchChunk));
    if (c->pool.empty()) c->pool.resize(kEventPairs);
    for (auto& t : c->pool) {
        if (!t.start) MH_HIP(hipEventCreate(&t.start));
        if (!t.stop) MH_HIP(hipEventCreate(&t.stop));
    }
    MH_HIP(mh::fast_module_init(dev));  // the fast_search code object (issue-priority build)
    c->dev = dev;
    c->ready = true;
    return MH_OK;
}

#ifdef MH_DEV_HOOKS
// MINEHIP_DEV_HASH_KEEP=k0,k1 (dev build only, 0 <= k <= 32): every scan kernel keeps
// only the top k0 bits of H0 and the top k1 bits of H1 of each nonce's hash, so that many nonces
// tie and the (hash, nonce) tie-breaking of the kernels and merges decides the result; the search
// returns the masked hash.  Read by every search (one process can run many settings) into
// c->keep, the word the pieces carry (layout.hpp keep_word).  The fast kernels mask only in the
// variant code object (build/fast_search_keep.hsaco through MINEHIP_DEV_CODE_OBJECT): with any
// other, a fast piece fails the search (enqueue_piece) instead of mixing masked and full hashes.
int read_hash_keep(DevCtx* c) {
    c->keep = 0;
    c->keep_fast = false;
    const char* e = getenv("MINEHIP_DEV_HASH_KEEP");
    if (!e || !*e) return MH_OK;
    unsigned k0 = 0, k1 = 0;
    char rest = 0;
    if (sscanf(e, "%u,%u%c", &k0, &k1, &rest) != 2 || k0 > 32u || k1 > 32u)
        return fail(MH_EINVAL, "MINEHIP_DEV_HASH_KEEP: expected k0,k1 with 0 <= k <= 32");
    MH_HIP(mh::fast_keep_ok(c->dev, &c->keep_fast));
    c->keep = mh::keep_word(k0, k1);
    return MH_OK;
}

// MINEHIP_DEV_HASH_XOR=<1-16 hex digits> (dev build only): every scan kernel XORs each
// nonce's (H0, H1) with the high and low 32 bits of the constant before the keep mask and before any
// comparison, so a test decides which nonce of a range wins: with x = Hash(msg, n) the search returns
// (0, n) exactly if it hashes n correctly, considers it and rebuilds its value.  Unset or zero: off.
// Read by every search, after read_hash_keep and before anything of the search is enqueued; the
// constant reaches the kernels through a device word (search_kernels.hip set_hash_xor) rewritten only
// when the value changes.  The fast kernels XOR only in the variant code object: with any other,
// a fast piece fails the search (enqueue_piece).
int read_hash_xor(DevCtx* c) {
    c->xor_on = c->xor_fast = false;
    const char* e = getenv("MINEHIP_DEV_HASH_XOR");
    uint64_t x = 0;
    if (e && *e) {
        size_t n = 0;
        for (; e[n]; ++n) {
            const char ch = e[n];
            const int v = (ch >= '0' && ch <= '9') ? ch - '0' : (ch >= 'a' && ch <= 'f') ? ch - 'a' + 10
                        : (ch >= 'A' && ch <= 'F') ? ch - 'A' + 10 : -1;
            if (v < 0 || n >= 16) return fail(MH_EINVAL, "MINEHIP_DEV_HASH_XOR: expected 1 to 16 hex digits");
            x = (x << 4) | (uint64_t)v;
        }
    }
    MH_HIP(mh::set_hash_xor(c->dev, x, c->stream, &c->xor_fast));
    c->xor_on = x != 0;
    return MH_OK;
}
#endif

// Stream must be idle or synchronised by the caller.
int harvest_locked(DevCtx* c) {
    for (int i = 0; i < c->used; ++i) {
        float ms = 0.f;
        MH_HIP(hipEventElapsedTime(&ms, c->pool[(size_t)i].start, c->pool[(size_t)i].stop));
        const uint64_t ns = (uint64_t)((double)ms * 1.0e6);
        c->cnt[c->pool[(size_t)i].kind == 0 ? 2 : 5] += ns;
        if (c->pool[(size_t)i].kind == 0) c->var[c->pool[(size_t)i].var].ns += ns;
    }
    c->used = 0;
    return MH_OK;
}

// The piece streams start after the main stream's work so far (the reset, a merge).
int piece_streams_wait_main(DevCtx* c) {
    MH_HIP(hipEventRecord(c->ev_main, c->stream));
    for (auto s : c->ps) MH_HIP(hipStreamWaitEvent(s, c->ev_main, 0));
    return MH_OK;
}

// Fold the pending partials into the running minimum.  With two piece
// streams the merge (on the main stream) first waits for both, and both wait
// for the merge before any later piece reuses the partials buffer.
int flush_partials(DevCtx* c, bool split) {
    if (!c->poff) return MH_OK;
    if (split) {
        for (int k = 0; k < 2; ++k) {
            MH_HIP(hipEventRecord(c->ev_piece[k], c->ps[k]));
            MH_HIP(hipStreamWaitEvent(c->stream, c->ev_piece[k], 0));
        }
    }
    MH_HIP(mh::launch_merge(c->d_partials, c->poff, c->d_best, c->stream));
    c->poff = 0;
    if (split) return piece_streams_wait_main(c);
    return MH_OK;
}

// Coarse pieces (the full L: 1,000-nonce lanes) go to the high-priority stream, the others
// (shorter lanes, generic edges, the tail split) to the low-priority one.
bool coarse_piece(const mh::Piece& p, const mh::PlanOpts& opt) { return p.kind == 0 && p.L == opt.lower_digits; }

// An Early piece (layout.hpp kMode*Early) enumerates its innermost digit and the L - 1 group digits
// before it inside word J: the kernel adds every group digit into word J, so a digit elsewhere
// would be hashed at the wrong place.  make_fast_args only builds such pieces; this re-checks it
// where a piece reaches the kernel, with the U digits' hole inside the d digits.
bool early_piece_ok(const mh::FastArgs& a, int word) {
    const uint32_t J = (uint32_t)word;
    if ((a.inner >> 2) != J || a.hole + a.hole_w > a.n_hi + a.L) return false;
    for (uint32_t j = 0; j + 1u < a.L; ++j) {
        const uint32_t pos = a.g_last - j - (j >= a.g_hole ? 1u : 0u);
        if (pos > a.g_last || (pos >> 2) != J) return false;
    }
    return true;
}

// Enqueue one piece on the context's stream.  Its workgroups write their
// partials after those of the previous pieces; one merge folds them all (or
// earlier, when the buffer would overflow), instead of one merge per piece.
int enqueue_piece(DevCtx* c, const mh::Piece& p, const mh::PlanOpts& opt, bool split) {
    hipStream_t s = !split ? c->stream : c->ps[coarse_piece(p, opt) ? 0 : 1];
    uint32_t blocks;
    if (p.kind == 0) {
        // host-side shape checks: the grid covers exactly n_runs lanes and the
        // partials buffer holds one slot per block
        if (p.fa.n_runs == 0 || p.fa.L < 1 || p.fa.L > 5 || p.fa.n_hi + p.fa.L > 20)
            return fail(MH_EINTERNAL, "internal: bad fast piece");
        if (p.fa.mode >= mh::kModeOneEarly && !early_piece_ok(p.fa, p.J))
            return fail(MH_EINTERNAL, "internal: bad Early piece (an enumerated digit outside word J)");
        blocks = (p.fa.n_runs + mh::kBlockThreads - 1) / mh::kBlockThreads;
    } else {
        if (p.ga.count == 0 || p.ga.count > (uint64_t)mh::kMaxBlocksPerLaunch * mh::kBlockThreads)
            return fail(MH_EINTERNAL, "internal: bad generic piece");
        blocks = (uint32_t)((p.ga.count + mh::kBlockThreads - 1) / mh::kBlockThreads);
    }
    if (blocks > mh::kMaxBlocksPerLaunch) return fail(MH_EINTERNAL, "internal: grid too large");
    if (c->poff + blocks > mh::kMaxBlocksPerLaunch) {
        const int rc = flush_partials(c, split);
        if (rc) return rc;
    }
    Partial* out = c->d_partials + c->poff;
    Timed* tm = nullptr;
    mh::FastArgs fa = p.fa;
#ifdef MH_DEV_HOOKS
    mh::GenArgs ga = p.ga;
    ga.pad = c->keep;
    if (p.kind == 0) {
        if (c->keep && !c->keep_fast)
            return fail(MH_EINVAL, "MINEHIP_DEV_HASH_KEEP is set but the fast code object is not the coarse-hash "
                                   "variant (MINEHIP_DEV_CODE_OBJECT=build/fast_search_keep.hsaco)");
        if (c->xor_on && !c->xor_fast)
            return fail(MH_EINVAL, "MINEHIP_DEV_HASH_XOR is set but the fast code object has no mh_dev_hash_xor "
                                   "(MINEHIP_DEV_CODE_OBJECT=build/fast_search_keep.hsaco)");
        fa.pad_ = c->keep;
    }
#else
    const mh::GenArgs& ga = p.ga;
#endif
    if (p.kind == 0) {
        fa.n_chunks = blocks;
        // work queue while this search has counters left (a longer search runs the rest static)
        fa.counter = (opt.queue && c->qoff < kQueueSlots) ? c->d_counters + c->qoff++ : nullptr;
    }
    if (c->prof) {
        if (c->used == kEventPairs) {
            MH_HIP(hipStreamSynchronize(c->stream));
            for (auto ps : c->ps) MH_HIP(hipStreamSynchronize(ps));
            int rc = harvest_locked(c);
            if (rc) return rc;
        }
        tm = &c->pool[(size_t)c->used++];
        tm->kind = p.kind;
        tm->var = p.kind == 0 ? var_index(p.J, p.mode, p.L) : 0;
        MH_HIP(hipEventRecord(tm->start, s));
    }
    if (c->first) {  // mh_search_first: the first-hit kernels over the same pieces
        if (p.kind == 0)
            MH_HIP(mh::launch_fast_first(c->dev, p.J, p.mode, fa, out, *c->first, c->first_stop, s));
        else
            MH_HIP(mh::launch_generic_scan_first(ga, out, blocks, *c->first, s));
    } else if (c->hits_stop) {  // mh_search_first_hits: the stopping hits kernels over the same pieces
        if (p.kind == 0)
            MH_HIP(mh::launch_fast_hits_stop(c->dev, p.J, p.mode, fa, out, *c->hits_stop, s));
        else
            MH_HIP(mh::launch_generic_scan_hits_stop(ga, out, blocks, *c->hits_stop, s));
    } else if (c->hits) {  // mh_search_hits: the hits kernels over the same pieces
        if (p.kind == 0)
            MH_HIP(mh::launch_fast_hits(c->dev, p.J, p.mode, fa, out, *c->hits, s));
        else
            MH_HIP(mh::launch_generic_scan_hits(ga, out, blocks, *c->hits, s));
    } else if (p.kind == 0)
        MH_HIP(mh::launch_fast(c->dev, p.J, p.mode, fa, out, s));
    else
        MH_HIP(mh::launch_generic_scan(ga, out, blocks, s));
    if (tm) MH_HIP(hipEventRecord(tm->stop, s));
    c->poff += blocks;
    if (c->prof) {
        if (p.kind == 0) {
            const uint64_t n = p.count;
            c->cnt[0] += 1;
            c->cnt[1] += n;
            c->cnt[3] += n * (uint64_t)p.ops;
            c->cnt[6] += n * (uint64_t)p.slots;
            VarStat& v = c->var[var_index(p.J, p.mode, p.L)];
            v.launches += 1;
            v.nonces += n;
            v.ops += n * (uint64_t)p.ops;
            v.slots += n * (uint64_t)p.slots;
        } else {
            c->cnt[4] += p.count;
        }
    }
    return MH_OK;
}

// Planner knobs, overridable for tests and tuning (the result never depends
// on them -- tests/test_gpu_parity.py checks exactly that):
//   MINEHIP_LOWER_DIGITS   L, digits enumerated inside one lane (1..5, default 3)
//   MINEHIP_MIN_LANES      lower L per bucket until it has this many runs (2^19)
//   MINEHIP_LAUNCH_NONCES  nonces per fast launch (default 2^35)
//   MINEHIP_GENERIC_BELOW  buckets with fewer nonces go to the generic kernel (2^20)
//   MINEHIP_MAX_BLOCKS     workgroups per launch (1..kMaxBlocksPerLaunch)
//   MINEHIP_STREAMS        1: one stream; 2: coarse / fine pieces on high / low priority
//                          streams (default 2)
//   MINEHIP_FINE_TAIL      nonces at the end of each full-L bucket planned at L - 1 (default
//                          2^28; 0: none)
//   MINEHIP_QUEUE          1: fast launches as work queues (workgroups claim chunks, so faster
//                          XCDs take more; default); 0: one workgroup per chunk
//   MINEHIP_EARLY          1: the Early layouts where a nonce costs less with the digit ending the
//                          word before the last digit's innermost (default); 0: never
mh::PlanOpts plan_opts() {
    mh::PlanOpts o;
    if (const char* e = getenv("MINEHIP_LOWER_DIGITS")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 5) o.lower_digits = v;
    }
    if (const char* e = getenv("MINEHIP_MIN_LANES")) o.min_lanes = strtoull(e, nullptr, 10);
    if (const char* e = getenv("MINEHIP_LAUNCH_NONCES")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1) o.max_nonces_per_launch = v;
    }
    if (const char* e = getenv("MINEHIP_GENERIC_BELOW")) o.generic_below = strtoull(e, nullptr, 10);
    if (const char* e = getenv("MINEHIP_MAX_BLOCKS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= mh::kMaxBlocksPerLaunch) o.max_blocks = (uint32_t)v;
    }
    if (const char* e = getenv("MINEHIP_STREAMS")) {
        const int v = atoi(e);
        if (v == 1 || v == 2) o.streams = v;
    }
    if (const char* e = getenv("MINEHIP_FINE_TAIL")) o.fine_tail = strtoull(e, nullptr, 10);
    if (const char* e = getenv("MINEHIP_QUEUE")) {
        const int v = atoi(e);
        if (v == 0 || v == 1) o.queue = v;
    }
    if (const char* e = getenv("MINEHIP_EARLY")) {
        const int v = atoi(e);
        if (v == 0 || v == 1) o.early = v;
    }
    return o;
}

uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

// busy_ns (optional): the search's own wall time, from holding the initialised device to having
// its result -- without the wait for another thread's search on the same device.
int search_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t* oh, uint64_t* on,
                uint64_t* busy_ns = nullptr) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    const uint64_t t0 = now_ns();
    MH_HIP(hipSetDevice(dev));
#ifdef MH_DEV_HOOKS
    rc = read_hash_keep(c);
    if (rc) return rc;
    rc = read_hash_xor(c);
    if (rc) return rc;
#endif
    MH_HIP(hipMemsetAsync(c->d_best, 0xFF, sizeof(Partial), c->stream));
    const mh::PlanOpts opt = plan_opts();
    if (opt.queue) MH_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(uint32_t) * kQueueSlots, c->stream));
    c->qoff = 0;
    // Two streams only when there is something to overlap: coarse pieces and others.  A small
    // search (generic edges, short-lane buckets) stays on one stream and skips the events.  The
    // plan is streamed, never stored (a range can hold ~2^30 pieces); this first pass stops as
    // soon as it has seen both kinds.
    bool any_coarse = false, any_fine = false;
    if (opt.streams == 2)
        mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
            (coarse_piece(p, opt) ? any_coarse : any_fine) = true;
            return !(any_coarse && any_fine);
        });
    const bool split = opt.streams == 2 && any_coarse && any_fine;
    if (split) {  // the piece streams start after the reset (and after the previous search)
        rc = piece_streams_wait_main(c);
        if (rc) return rc;
    }
    int err = MH_OK;
    c->poff = 0;
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        err = enqueue_piece(c, p, opt, split);
        return err == MH_OK;
    });
    if (!err) err = flush_partials(c, split);
    if (err) {
        for (auto ps : c->ps)
            if (ps) (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return err;
    }
    MH_HIP(hipMemcpyAsync(c->h_best, c->d_best, sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    *oh = c->h_best->hash;
    *on = c->h_best->nonce;
    if (busy_ns) *busy_ns = now_ns() - t0;
    return MH_OK;
}

// mh_search_first: search_impl's plan, streams, partial flushes and work-queue counters over the
// first-hit kernels (first_scan<J, MODE>, generic_scan_first; layout.hpp FirstArgs), then
// finish_first on the main stream and one 24-byte copy-back with the one synchronise.  The word
// the kernels skip later chunks by and the scanned count are reset beside the running minimum.
// flags (mh_search_first_ex, checked by the caller): MH_FIRST_STOP_RUNNING launches stop_scan<J, MODE>
// in place of first_scan<J, MODE>; nothing else differs.
int search_first_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, uint32_t flags,
                      mh_first* out) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    if (!c->d_first) MH_HIP(hipMalloc(&c->d_first, 5 * sizeof(uint64_t)));
    if (!c->h_first) MH_HIP(hipHostMalloc(&c->h_first, 3 * sizeof(uint64_t), hipHostMallocDefault));
#ifdef MH_DEV_HOOKS
    c->keep = 0;  // mh_search_first refused the hash hooks; nothing of an earlier search's stays
    c->keep_fast = c->xor_on = c->xor_fast = false;
#endif
    MH_HIP(hipMemsetAsync(c->d_best, 0xFF, sizeof(Partial), c->stream));
    MH_HIP(hipMemsetAsync(c->d_first, 0xFF, sizeof(uint64_t), c->stream));
    MH_HIP(hipMemsetAsync(c->d_first + 1, 0, sizeof(uint64_t), c->stream));
    const mh::PlanOpts opt = plan_opts();
    if (opt.queue) MH_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(uint32_t) * kQueueSlots, c->stream));
    c->qoff = 0;
    bool any_coarse = false, any_fine = false;
    if (opt.streams == 2)
        mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
            (coarse_piece(p, opt) ? any_coarse : any_fine) = true;
            return !(any_coarse && any_fine);
        });
    const bool split = opt.streams == 2 && any_coarse && any_fine;
    if (split) {
        rc = piece_streams_wait_main(c);
        if (rc) return rc;
    }
    const mh::FirstArgs fargs{target, (unsigned long long*)c->d_first, (unsigned long long*)(c->d_first + 1)};
    int err = MH_OK;
    c->poff = 0;
    c->first = &fargs;
    c->first_stop = (flags & MH_FIRST_STOP_RUNNING) != 0;
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        err = enqueue_piece(c, p, opt, split);
        return err == MH_OK;
    });
    c->first = nullptr;
    c->first_stop = false;
    if (!err) err = flush_partials(c, split);
    if (err) {
        for (auto ps : c->ps)
            if (ps) (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return err;
    }
    mh::GenArgs ga;
    mh::make_gen_args(pre, &ga);
    MH_HIP(mh::launch_finish_first(ga, c->d_best, (const unsigned long long*)(c->d_first + 1), c->d_first + 2, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_first, c->d_first + 2, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    out->hash = c->h_first[0];
    out->nonce = c->h_first[1];
    out->scanned = c->h_first[2];
    out->found = out->hash <= target ? 1 : 0;  // without a qualifying nonce the minimum itself is > target
    out->reserved = 0;
    return MH_OK;
}

//   MINEHIP_HITS_SLOTS     entries of the device hit buffer one scan of mh_search_hits may fill
//                          (1..MH_HITS_MAX_CAP, the default): a lower value makes a search with more
//                          hits rebuild its list window by window (tests; the results never depend
//                          on it)
uint64_t hits_slots() {
    if (const char* e = getenv("MINEHIP_HITS_SLOTS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= MH_HITS_MAX_CAP) return v;
    }
    return MH_HITS_MAX_CAP;
}

// One scan of [lower, upper] for mh_search_hits, under the device's lock: search_impl's plan,
// streams, partial flushes and work-queue counters over the hits kernels (hits_scan<J, MODE>,
// generic_scan_hits; layout.hpp HitsArgs), one synchronise, then the range's minimum in c->h_best,
// its hit count in *count and, if `got` is given, the min(count, slots) entries the device buffer
// holds in *got (in no particular order; all of the range's hits exactly if count <= slots).
int hits_scan_range(DevCtx* c, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, uint64_t slots,
                    uint64_t* count, std::vector<mh::Hit>* got) {
    MH_HIP(hipMemsetAsync(c->d_best, 0xFF, sizeof(Partial), c->stream));
    MH_HIP(hipMemsetAsync(c->d_hcursor, 0, sizeof(uint64_t), c->stream));
    const mh::PlanOpts opt = plan_opts();
    if (opt.queue) MH_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(uint32_t) * kQueueSlots, c->stream));
    c->qoff = 0;
    bool any_coarse = false, any_fine = false;
    if (opt.streams == 2)
        mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
            (coarse_piece(p, opt) ? any_coarse : any_fine) = true;
            return !(any_coarse && any_fine);
        });
    const bool split = opt.streams == 2 && any_coarse && any_fine;
    if (split) {
        const int rc = piece_streams_wait_main(c);
        if (rc) return rc;
    }
    const mh::HitsArgs hargs{target, (unsigned long long*)c->d_hcursor, c->d_hits, slots};
    int err = MH_OK;
    c->poff = 0;
    c->hits = &hargs;
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        err = enqueue_piece(c, p, opt, split);
        return err == MH_OK;
    });
    c->hits = nullptr;
    if (!err) err = flush_partials(c, split);
    if (err) {
        for (auto ps : c->ps)
            if (ps) (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return err;
    }
    MH_HIP(hipMemcpyAsync(c->h_best, c->d_best, sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_hcursor, c->d_hcursor, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        const int rc = harvest_locked(c);
        if (rc) return rc;
    }
    *count = *c->h_hcursor;
    if (got) {
        got->resize((size_t)std::min(*count, slots));
        if (!got->empty()) MH_HIP(hipMemcpy(got->data(), c->d_hits, got->size() * sizeof(mh::Hit), hipMemcpyDeviceToHost));
    }
    return MH_OK;
}

bool hit_by_nonce(const mh::Hit& x, const mh::Hit& y) { return x.nonce < y.nonce; }

// The window walk of mh_search_hits and mh_search_first_hits, under the device's lock: the hits of
// [lower, upper] from `lower` upward, in nonce order, out of windows [cur, cur + w - 1] scanned by
// the non-stopping hits kernels (hits_scan_range), until `want` entries are collected or `upper` is
// reached.  w is sized from `spacing`, the nonces per hit the caller observed, for about a quarter
// of the buffer per window; a window that overflows the buffer all the same is halved and scanned
// again (one of at most `slots` nonces cannot overflow), one that fits is complete, so sorted and
// appended.  The last window's entries are all kept: *list may hold more than `want`.
// widen (the rebuilds of mh_search_first_hits_batch only; mh_search_hits and mh_search_first_hits walk
// as they always did): after a window that fit the next one is twice as wide again, up to the first
// size, so that two hits that lie close together narrow the windows around them only.  A walk that
// keeps its narrowest width takes range / smallest gap scans with a buffer of one entry, and a batch
// under a small MINEHIP_HITS_SLOTS rebuilds most of its requests.  The widths decide which windows
// are scanned, never what the list holds.
int hits_window_walk(DevCtx* c, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, uint64_t slots,
                     uint64_t want, double spacing, std::vector<mh::Hit>* list, bool widen = false) {
    const double per_window = std::max(1.0, (double)slots / 4.0 * spacing);
    uint64_t w = per_window >= 9.0e18 ? (uint64_t)9.0e18 : (uint64_t)per_window;
    const uint64_t w0 = w;
    std::vector<mh::Hit> win;
    uint64_t cur = lower;
    list->clear();
    while (list->size() < want) {
        const uint64_t hi = (upper - cur < w - 1u) ? upper : cur + (w - 1u);
        uint64_t wc = 0;
        const int rc = hits_scan_range(c, pre, cur, hi, target, slots, &wc, &win);
        if (rc) return rc;
        if (wc > slots) {  // hi - cur + 1 > slots >= 1 here
            w = (hi - cur + 1u) / 2u;
            continue;
        }
        std::sort(win.begin(), win.end(), hit_by_nonce);
        list->insert(list->end(), win.begin(), win.end());
        if (hi == upper) break;
        cur = hi + 1u;
        if (widen && w < w0) w = w0 - w < w ? w0 : w * 2u;
    }
    return MH_OK;
}

// mh_search_hits: one scan of the whole range gives the minimum, the exact count (the cursor
// advances for every hit) and, while the count fits the device buffer, every hit; the host sorts
// them by nonce and returns the first `cap`.  When the buffer overflowed, which entries it kept
// depends on timing, so the list is rebuilt from `lower` upward out of windows [cur, cur + w - 1]
// scanned by the same kernels: w is sized from the observed density for about a quarter of the
// buffer per window, a window that overflows all the same is halved and scanned again (one of at
// most `slots` nonces cannot overflow), one that fits is complete, so sorted and appended, until
// min(count, cap) entries are collected (hits_window_walk).  The count and the minimum are the first scan's.
int search_hits_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, mh_hit* hits,
                     size_t cap, mh_hits* out) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    if (!c->d_hits) MH_HIP(hipMalloc(&c->d_hits, sizeof(mh::Hit) * MH_HITS_MAX_CAP));
    if (!c->d_hcursor) MH_HIP(hipMalloc(&c->d_hcursor, sizeof(uint64_t)));
    if (!c->h_hcursor) MH_HIP(hipHostMalloc(&c->h_hcursor, sizeof(uint64_t), hipHostMallocDefault));
#ifdef MH_DEV_HOOKS
    c->keep = 0;  // mh_search_hits refused the hash hooks; nothing of an earlier search's stays
    c->keep_fast = c->xor_on = c->xor_fast = false;
#endif
    const uint64_t slots = hits_slots();
    std::vector<mh::Hit> got;
    uint64_t count = 0;
    rc = hits_scan_range(c, pre, lower, upper, target, slots, &count, cap ? &got : nullptr);
    if (rc) return rc;
    out->count = count;
    out->stored = std::min<uint64_t>(count, cap);
    out->hash = c->h_best->hash;
    out->nonce = c->h_best->nonce;
    if (cap && count > slots) {  // the buffer dropped entries: rebuild the list window by window
        const double total = (double)(upper - lower) + 1.0;
        std::vector<mh::Hit> list;
        rc = hits_window_walk(c, pre, lower, upper, target, slots, out->stored, total / (double)count, &list);
        if (rc) return rc;
        if (list.size() < out->stored) return fail(MH_EINTERNAL, "internal: the hit windows hold fewer hits than the scan counted");
        got.swap(list);
    } else {
        std::sort(got.begin(), got.end(), hit_by_nonce);
    }
    for (uint64_t i = 0; i < out->stored; ++i) hits[i] = mh_hit{got[(size_t)i].hash, got[(size_t)i].nonce};
    return MH_OK;
}

// mh_search_first_hits: hits_scan_range's plan, streams, partial flushes and work-queue counters over
// the stopping hits kernels (hits_stop<J, MODE>, generic_scan_hits_stop; layout.hpp HitsStopArgs),
// one synchronise, then the k smallest of the appended hits.  Every nonce <= the bound word's final
// value was hashed (a chunk or tile is only skipped or left above a value the word held, and the
// word only decreases) and at least k hits are <= it, so the appended hits hold the k smallest of
// the range whenever they are k or more; with fewer the word was never lowered (it is lowered only
// from slice counts that hold k appended hits), nothing was skipped and the minimum is the range's.
// When the device buffer dropped entries, which ones depends on timing: the list is rebuilt from
// `lower` upward by the window walk of mh_search_hits, on the non-stopping kernels, until k entries
// are collected or `upper` is reached.
// widen_walk: hits_window_walk's `widen`, for the rebuilds and fallbacks of mh_search_first_hits_batch.
int search_first_hits_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, mh_hit* hits,
                           size_t k, mh_first_hits* out, bool widen_walk = false) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    if (!c->d_hits) MH_HIP(hipMalloc(&c->d_hits, sizeof(mh::Hit) * MH_HITS_MAX_CAP));
    if (!c->d_hcursor) MH_HIP(hipMalloc(&c->d_hcursor, sizeof(uint64_t)));
    if (!c->h_hcursor) MH_HIP(hipHostMalloc(&c->h_hcursor, sizeof(uint64_t), hipHostMallocDefault));
    if (!c->d_fhits) MH_HIP(hipMalloc(&c->d_fhits, 2 * sizeof(uint64_t)));
    if (!c->d_slices) MH_HIP(hipMalloc(&c->d_slices, sizeof(uint32_t) * mh::kFirstHitsSlices));
    if (!c->h_fhits) MH_HIP(hipHostMalloc(&c->h_fhits, sizeof(uint64_t), hipHostMallocDefault));
#ifdef MH_DEV_HOOKS
    c->keep = 0;  // mh_search_first_hits refused the hash hooks; nothing of an earlier search's stays
    c->keep_fast = c->xor_on = c->xor_fast = false;
#endif
    const uint64_t slots = hits_slots();
    const uint64_t total_m1 = upper - lower;  // the range's size minus 1 (its size may be 2^64)
    MH_HIP(hipMemsetAsync(c->d_best, 0xFF, sizeof(Partial), c->stream));
    MH_HIP(hipMemsetAsync(c->d_hcursor, 0, sizeof(uint64_t), c->stream));
    MH_HIP(hipMemsetAsync(c->d_fhits, 0xFF, sizeof(uint64_t), c->stream));
    MH_HIP(hipMemsetAsync(c->d_fhits + 1, 0, sizeof(uint64_t), c->stream));
    MH_HIP(hipMemsetAsync(c->d_slices, 0, sizeof(uint32_t) * mh::kFirstHitsSlices, c->stream));
    const mh::PlanOpts opt = plan_opts();
    if (opt.queue) MH_HIP(hipMemsetAsync(c->d_counters, 0, sizeof(uint32_t) * kQueueSlots, c->stream));
    c->qoff = 0;
    bool any_coarse = false, any_fine = false;
    if (opt.streams == 2)
        mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
            (coarse_piece(p, opt) ? any_coarse : any_fine) = true;
            return !(any_coarse && any_fine);
        });
    const bool split = opt.streams == 2 && any_coarse && any_fine;
    if (split) {
        rc = piece_streams_wait_main(c);
        if (rc) return rc;
    }
    const mh::HitsStopArgs hs{mh::HitsArgs{target, (unsigned long long*)c->d_hcursor, c->d_hits, slots},
                              (uint64_t)k,
                              (unsigned long long*)c->d_fhits,
                              c->d_slices,
                              lower,
                              total_m1,
                              mh::first_hits_shift(total_m1),
                              0u,
                              (unsigned long long*)(c->d_fhits + 1)};
    int err = MH_OK;
    c->poff = 0;
    c->hits_stop = &hs;
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        err = enqueue_piece(c, p, opt, split);
        return err == MH_OK;
    });
    c->hits_stop = nullptr;
    if (!err) err = flush_partials(c, split);
    if (err) {
        for (auto ps : c->ps)
            if (ps) (void)hipStreamSynchronize(ps);
        (void)hipStreamSynchronize(c->stream);
        return err;
    }
    MH_HIP(hipMemcpyAsync(c->h_best, c->d_best, sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_hcursor, c->d_hcursor, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_fhits, c->d_fhits + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    const uint64_t appended = *c->h_hcursor, scanned = *c->h_fhits;
    const Partial best = *c->h_best;  // the window walk below reuses the pinned words
    std::vector<mh::Hit> got;
    if (appended <= slots) {
        got.resize((size_t)appended);
        if (!got.empty()) MH_HIP(hipMemcpy(got.data(), c->d_hits, got.size() * sizeof(mh::Hit), hipMemcpyDeviceToHost));
        std::sort(got.begin(), got.end(), hit_by_nonce);
    } else {  // the buffer dropped entries: rebuild the list window by window, from the observed density
        rc = hits_window_walk(c, pre, lower, upper, target, slots, k, std::max(1.0, (double)scanned) / (double)appended, &got,
                              widen_walk);
        if (rc) return rc;
    }
    out->stored = std::min<uint64_t>(got.size(), k);
    out->scanned = scanned;
    if (out->stored < k) {
        // fewer than k hits: the bound was never lowered, so nothing was skipped
        if (scanned != total_m1 + 1u)
            return fail(MH_EINTERNAL, "internal: fewer than k hits, but the scan did not hash the whole range");
        out->hash = best.hash;
        out->nonce = best.nonce;
    } else {
        out->hash = got[0].hash;
        out->nonce = got[0].nonce;
        for (size_t i = 1; i < k; ++i)
            if (got[i].hash < out->hash || (got[i].hash == out->hash && got[i].nonce < out->nonce)) {
                out->hash = got[i].hash;
                out->nonce = got[i].nonce;
            }
    }
    for (uint64_t i = 0; i < out->stored; ++i) hits[i] = mh_hit{got[(size_t)i].hash, got[(size_t)i].nonce};
    return MH_OK;
}

int check_common(const uint8_t* msg, size_t len) {
    if (msg == nullptr && len != 0) return fail(MH_EINVAL, "msg is NULL");
    if (len > MH_MAX_MSG_LEN) return fail(MH_ETOOLONG, "message longer than MH_MAX_MSG_LEN");
    return MH_OK;
}

// ---- batched search ----

//   MINEHIP_BATCH_SLOTS    partial slots (tiles) one pass of mh_search_batch may use
//                          (1..kMaxBlocksPerLaunch, the default): a lower value makes small
//                          batches run several passes and send their larger requests to the
//                          fallback path (tests; the results never depend on it)
uint32_t batch_slots() {
    if (const char* e = getenv("MINEHIP_BATCH_SLOTS")) {
        const unsigned long long v = strtoull(e, nullptr, 10);
        if (v >= 1 && v <= mh::kMaxBlocksPerLaunch) return (uint32_t)v;
    }
    return mh::kMaxBlocksPerLaunch;
}

inline size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }

int batch_init_locked(DevCtx* c) {
    if (!c->d_btab) MH_HIP(hipMalloc(&c->d_btab, kBatchTableBytes));
    if (!c->h_btab) MH_HIP(hipHostMalloc(&c->h_btab, kBatchTableBytes, hipHostMallocDefault));
    if (!c->d_bres) MH_HIP(hipMalloc(&c->d_bres, sizeof(Partial) * kBatchResults));
    if (!c->h_bres) MH_HIP(hipHostMalloc(&c->h_bres, sizeof(Partial) * kBatchResults, hipHostMallocDefault));
    return MH_OK;
}

// The results of the passes enqueued since the last drain, waiting in h_bres for the synchronise.
struct BatchPending {
    std::vector<size_t> req_idx;  // in h_bres order
    size_t toff = 0;              // table bytes in use
};

int batch_drain(DevCtx* c, const mh::BatchRequest* reqs, BatchPending* pend, mh_result* out) {
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        const int rc = harvest_locked(c);
        if (rc) return rc;
    }
    for (size_t k = 0; k < pend->req_idx.size(); ++k) {
        mh_result& r = out[reqs[pend->req_idx[k]].id];
        r.hash = c->h_bres[k].hash;
        r.nonce = c->h_bres[k].nonce;
    }
    pend->req_idx.clear();
    pend->toff = 0;
    return MH_OK;
}

// One pass on c->stream: one H2D copy of its tables from the pinned staging, batch_scan,
// merge_segments, one D2H copy of its results.  No synchronise: the tables and results of
// successive passes sit behind one another until a buffer is full.
int batch_run_pass(DevCtx* c, const mh::BatchRequest* reqs, const mh::BatchTables& t, uint32_t slot_cap,
                   BatchPending* pend, mh_result* out) {
    if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t bytes = o_tile + align16(tiles * sizeof(uint32_t));
    if (bytes > kBatchTableBytes || nreq > kBatchResults) return fail(MH_EINTERNAL, "internal: batch pass too large");
    if (pend->toff + bytes > kBatchTableBytes || pend->req_idx.size() + nreq > kBatchResults ||
        (c->prof && c->used == kEventPairs)) {
        const int rc = batch_drain(c, reqs, pend, out);
        if (rc) return rc;
    }
    uint8_t* h = c->h_btab + pend->toff;
    uint8_t* d = c->d_btab + pend->toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
#ifdef MH_DEV_HOOKS
    for (size_t i = 0; i < ne; ++i) ((mh::BatchEntry*)h)[i].g.pad = c->keep;
#endif
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    Timed* tm = nullptr;
    if (c->prof) {  // the batch launches count in the generic class (mh_profile_read out[4], out[5])
        tm = &c->pool[(size_t)c->used++];
        tm->kind = 1;
        tm->var = 0;
        MH_HIP(hipEventRecord(tm->start, c->stream));
    }
    MH_HIP(mh::launch_batch_scan((const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile), c->d_partials, (uint32_t)tiles,
                                 c->stream));
    if (tm) {
        MH_HIP(hipEventRecord(tm->stop, c->stream));
        c->cnt[4] += t.nonces;
    }
    const size_t roff = pend->req_idx.size();
    MH_HIP(mh::launch_merge_segments(c->d_partials, (const uint32_t*)(d + o_seg), c->d_bres + roff, (uint32_t)nreq,
                                     c->stream));
    MH_HIP(hipMemcpyAsync(c->h_bres + roff, c->d_bres + roff, nreq * sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->toff += bytes;
    return MH_OK;
}

// The fused passes of a batch, under the device's lock.
int batch_run_fused(int dev, const mh::BatchRequest* reqs, const std::vector<mh::BatchItem>& items, int passes,
                    uint32_t slot_cap, mh_result* out) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    rc = batch_init_locked(c);
    if (rc) return rc;
#ifdef MH_DEV_HOOKS
    rc = read_hash_keep(c);
    if (rc) return rc;
    rc = read_hash_xor(c);
    if (rc) return rc;
#endif
    BatchPending pend;
    mh::BatchTables t;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables(reqs, items, p, &t);
        rc = batch_run_pass(c, reqs, t, slot_cap, &pend, out);
    }
    if (!rc) rc = batch_drain(c, reqs, &pend, out);
    if (rc) (void)hipStreamSynchronize(c->stream);  // nothing of this call stays in flight
    return rc;
}

// ---- batched search with fused fast pieces (mh_search_batch_ex) ----

//   MINEHIP_BATCH_FAST_MAX    most nonces of a request mh_search_batch_ex(MH_BATCH_FUSE_FAST) fuses
//                             (default kBatchFastMaxNonces; 0: no request with a fast piece is fused)
//   MINEHIP_BATCH_FAST_LANES  "shared": the batch-aware lane rule (plan.hpp batch_min_lanes), which the
//                             measurement did not favour; otherwise every request
//                             keeps the lanes of its own mh_search plan (default)
// (tests and tools/batch_fast_latency.py; the results never depend on them)
uint64_t batch_fast_max() {
    if (const char* e = getenv("MINEHIP_BATCH_FAST_MAX"))
        if (*e) return strtoull(e, nullptr, 10);
    return mh::kBatchFastMaxNonces;
}
bool batch_fast_shared_lanes() {
    const char* e = getenv("MINEHIP_BATCH_FAST_LANES");
    return e && strcmp(e, "shared") == 0;
}

// batch_run_pass for a pass that may hold fast pieces: one H2D copy of all its tables (entries,
// segments, per-tile entry, fast items, per-chunk item), batch_scan_slots for the generic entries,
// one batch_fast<J, MODE> launch per layout present, merge_segments, one D2H copy.  The fast
// launches count in the fast class of the profile: per piece its nonces, ops and slots under its
// (J, MODE, L); a launch's time under the (J, MODE, L) of its first, longest-lane piece.
int batch_run_pass_ex(DevCtx* c, const mh::BatchRequest* reqs, const std::vector<mh::BatchPiece>& pieces,
                      const mh::BatchTables& t, const mh::BatchFastTables& f, uint32_t slot_cap, BatchPending* pend,
                      mh_result* out) {
    if (!mh::batch_tables_ex_ok(t, f, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
    for (size_t k = 0; k < f.items.size(); ++k) {
        const mh::BatchPiece& p = pieces[f.piece[k]];
        if (f.items[k].args.mode >= mh::kModeOneEarly && !early_piece_ok(f.items[k].args, p.J))
            return fail(MH_EINTERNAL, "internal: bad Early piece (an enumerated digit outside word J)");
    }
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t ni = f.items.size(), chunks = f.chunk_item.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_item = o_tile + align16(tiles * sizeof(uint32_t)), o_chunk = o_item + ni * sizeof(mh::BatchFastItem);
    const size_t bytes = o_chunk + align16(chunks * sizeof(uint32_t));
    if (bytes > kBatchTableBytes || nreq > kBatchResults) return fail(MH_EINTERNAL, "internal: batch pass too large");
    if (pend->toff + bytes > kBatchTableBytes || pend->req_idx.size() + nreq > kBatchResults ||
        (c->prof && c->used + 1 + (int)f.launches.size() > kEventPairs)) {
        const int rc = batch_drain(c, reqs, pend, out);
        if (rc) return rc;
    }
    uint8_t* h = c->h_btab + pend->toff;
    uint8_t* d = c->d_btab + pend->toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_item, f.items.data(), ni * sizeof(mh::BatchFastItem));
    memcpy(h + o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t));
#ifdef MH_DEV_HOOKS
    for (size_t i = 0; i < ne; ++i) ((mh::BatchEntry*)h)[i].g.pad = c->keep;
    for (size_t i = 0; i < ni; ++i) ((mh::BatchFastItem*)(h + o_item))[i].args.pad_ = c->keep;
#endif
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    if (tiles) {
        Timed* tm = nullptr;
        if (c->prof) {  // generic class, as batch_run_pass
            tm = &c->pool[(size_t)c->used++];
            tm->kind = 1;
            tm->var = 0;
            MH_HIP(hipEventRecord(tm->start, c->stream));
        }
        MH_HIP(mh::launch_batch_scan_slots((const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile), c->d_partials,
                                           (uint32_t)tiles, c->stream));
        if (tm) {
            MH_HIP(hipEventRecord(tm->stop, c->stream));
            c->cnt[4] += t.nonces;
        }
    }
    for (const mh::BatchFastLaunch& l : f.launches) {
        Timed* tm = nullptr;
        if (c->prof) {
            tm = &c->pool[(size_t)c->used++];
            tm->kind = 0;
            tm->var = var_index(l.J, l.mode, (int)f.items[l.item0].args.L);
            MH_HIP(hipEventRecord(tm->start, c->stream));
        }
        MH_HIP(mh::launch_batch_fast(c->dev, l.J, l.mode, (const mh::BatchFastItem*)(d + o_item),
                                     (const uint32_t*)(d + o_chunk) + l.chunk0, c->d_partials, l.chunks, c->stream));
        if (tm) {
            MH_HIP(hipEventRecord(tm->stop, c->stream));
            c->cnt[0] += 1;
            c->var[tm->var].launches += 1;
            for (uint32_t k = l.item0; k < l.item0 + l.items; ++k) {
                const mh::BatchPiece& p = pieces[f.piece[k]];
                c->cnt[1] += p.count;
                c->cnt[3] += p.count * (uint64_t)p.ops;
                c->cnt[6] += p.count * (uint64_t)p.nslots;
                VarStat& v = c->var[var_index(p.J, p.mode, p.L)];
                v.nonces += p.count;
                v.ops += p.count * (uint64_t)p.ops;
                v.slots += p.count * (uint64_t)p.nslots;
            }
        }
    }
    const size_t roff = pend->req_idx.size();
    MH_HIP(mh::launch_merge_segments(c->d_partials, (const uint32_t*)(d + o_seg), c->d_bres + roff, (uint32_t)nreq,
                                     c->stream));
    MH_HIP(hipMemcpyAsync(c->h_bres + roff, c->d_bres + roff, nreq * sizeof(Partial), hipMemcpyDeviceToHost, c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->toff += bytes;
    return MH_OK;
}

// The fused passes of mh_search_batch_ex(MH_BATCH_FUSE_FAST), under the device's lock.
int batch_run_fused_ex(int dev, const mh::BatchRequest* reqs, const std::vector<mh::BatchPiece>& pieces,
                       const std::vector<mh::FastArgs>& args, int passes, uint32_t slot_cap, mh_result* out) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    rc = batch_init_locked(c);
    if (rc) return rc;
#ifdef MH_DEV_HOOKS
    rc = read_hash_keep(c);
    if (rc) return rc;
    rc = read_hash_xor(c);
    if (rc) return rc;
    const bool any_fast = std::any_of(pieces.begin(), pieces.end(), [](const mh::BatchPiece& p) { return p.kind == 2; });
    if (any_fast && (c->keep || c->xor_on)) {  // the hooks of the batch code object, as enqueue_piece's of the product's
        uint64_t x = 0;
        if (const char* e = getenv("MINEHIP_DEV_HASH_XOR")) x = strtoull(e, nullptr, 16);  // read_hash_xor accepted it
        bool keep_ok = false, xor_ok = false;
        MH_HIP(mh::batch_fast_hooks(c->dev, x, c->stream, &keep_ok, &xor_ok));
        if (c->keep && !keep_ok)
            return fail(MH_EINVAL, "MINEHIP_DEV_HASH_KEEP is set but the batch code object is not the coarse-hash "
                                   "variant (MINEHIP_DEV_BATCH_CODE_OBJECT=build/fast_batch_keep.hsaco)");
        if (c->xor_on && !xor_ok)
            return fail(MH_EINVAL, "MINEHIP_DEV_HASH_XOR is set but the batch code object has no mh_dev_hash_xor "
                                   "(MINEHIP_DEV_BATCH_CODE_OBJECT=build/fast_batch_keep.hsaco)");
    } else if (any_fast) {  // off: a variant code object's word may still hold an earlier call's constant
        bool keep_ok = false, xor_ok = false;
        if (getenv("MINEHIP_DEV_BATCH_CODE_OBJECT")) MH_HIP(mh::batch_fast_hooks(c->dev, 0, c->stream, &keep_ok, &xor_ok));
    }
#endif
    BatchPending pend;
    mh::BatchTables t;
    mh::BatchFastTables f;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables_ex(reqs, pieces, args, p, &t, &f);
        // a pass without a fast piece is mh_search_batch's own pass (slot0 == tile0 throughout)
        rc = f.items.empty() ? batch_run_pass(c, reqs, t, slot_cap, &pend, out)
                             : batch_run_pass_ex(c, reqs, pieces, t, f, slot_cap, &pend, out);
    }
    if (!rc) rc = batch_drain(c, reqs, &pend, out);
    if (rc) (void)hipStreamSynchronize(c->stream);  // nothing of this call stays in flight
    return rc;
}

// A fallback request's search: (request, hash, nonce) -> MH_*.
using BatchFallback = std::function<int(const mh::BatchRequest&, uint64_t*, uint64_t*)>;

int search_batch_impl(int dev, const mh_request* reqs, size_t n, mh_result* out, const BatchFallback& fallback) {
    std::vector<mh::BatchRequest> valid;
    valid.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        int st = check_common(reqs[i].msg, reqs[i].len);
        if (!st && reqs[i].lower > reqs[i].upper) st = fail(MH_ERANGE, "lower > upper");
        out[i] = mh_result{st, 0, 0, 0};
        if (st) continue;
        valid.emplace_back();
        mh::BatchRequest& r = valid.back();
        mh::absorb_prefix(reqs[i].msg, reqs[i].len, &r.pre);
        r.lower = reqs[i].lower;
        r.upper = reqs[i].upper;
        r.id = i;
    }
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    mh::plan_batch(valid.data(), valid.size(), plan_opts(), slot_cap, &items);
    int passes = 0;
    for (const mh::BatchItem& it : items)
        if (it.kind == 0) passes = std::max(passes, it.pass + 1);
    if (passes) {
        const int rc = batch_run_fused(dev, valid.data(), items, passes, slot_cap, out);
        if (rc) return rc;
    }
    for (const mh::BatchItem& it : items) {
        if (it.kind != 1) continue;
        const mh::BatchRequest& r = valid[it.idx];
        const int rc = fallback(r, &out[r.id].hash, &out[r.id].nonce);
        if (rc) return rc;
    }
    return MH_OK;
}

// ---- batched first-hit search ----

//   MINEHIP_FIRST_BATCH_ORDER  "request": workgroup b of batch_scan_first runs tile b (the identity,
//                              request-major order) instead of the rank-major order; read per
//                              call (measurement and tests; found, hash and nonce never depend on it)
bool first_batch_rank_major() {
    const char* e = getenv("MINEHIP_FIRST_BATCH_ORDER");
    return !(e && strcmp(e, "request") == 0);
}

// The per-request checks of a batch (mh_request or mh_first_request): a status for every request,
// and the valid ones as BatchRequests.
template <class Req>
void batch_requests(const Req* reqs, size_t n, std::vector<int>* status, std::vector<mh::BatchRequest>* valid) {
    status->assign(n, MH_OK);
    valid->clear();
    valid->reserve(n);
    for (size_t i = 0; i < n; ++i) {
        int st = check_common(reqs[i].msg, reqs[i].len);
        if (!st && reqs[i].lower > reqs[i].upper) st = fail(MH_ERANGE, "lower > upper");
        (*status)[i] = st;
        if (st) continue;
        valid->emplace_back();
        mh::BatchRequest& r = valid->back();
        mh::absorb_prefix(reqs[i].msg, reqs[i].len, &r.pre);
        r.lower = reqs[i].lower;
        r.upper = reqs[i].upper;
        r.id = i;
    }
}

int first_batch_init_locked(DevCtx* c) {
    if (!c->d_fres) MH_HIP(hipMalloc(&c->d_fres, sizeof(mh::BatchFirstResult) * kBatchResults));
    if (!c->h_fres)
        MH_HIP(hipHostMalloc(&c->h_fres, sizeof(mh::BatchFirstResult) * kBatchResults, hipHostMallocDefault));
    return MH_OK;
}

void put_first_result(mh_first_result* r, uint64_t hash, uint64_t nonce, uint64_t scanned, uint64_t target) {
    r->hash = hash;
    r->nonce = nonce;
    r->scanned = scanned;
    r->found = hash <= target ? 1 : 0;  // without a qualifying nonce the minimum itself is > target
}

int first_batch_drain(DevCtx* c, const mh::BatchRequest* reqs, const mh_first_request* src, BatchPending* pend,
                      mh_first_result* out) {
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        const int rc = harvest_locked(c);
        if (rc) return rc;
    }
    for (size_t k = 0; k < pend->req_idx.size(); ++k) {
        const size_t id = reqs[pend->req_idx[k]].id;
        put_first_result(&out[id], c->h_fres[k].hash, c->h_fres[k].nonce, c->h_fres[k].scanned, src[id].target);
    }
    pend->req_idx.clear();
    pend->toff = 0;
    return MH_OK;
}

// batch_run_pass over the first-hit kernels: the pass's one H2D copy also carries the per-entry
// request index, the dispatch order and the requests' device words with their initial values
// (target; first = all ones; scanned = 0), so there is no memset and no fill kernel; then
// batch_scan_first, merge_segments_first and one D2H copy of {hash, nonce, scanned} per request.
int first_batch_run_pass(DevCtx* c, const mh::BatchRequest* reqs, const mh_first_request* src, const mh::BatchTables& t,
                         uint32_t slot_cap, bool rank_major, BatchPending* pend, mh_first_result* out) {
    if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
    mh::FirstBatchTables ft;
    mh::build_first_batch_tables(t, rank_major, &ft);
    if (!mh::first_batch_tables_ok(t, ft)) return fail(MH_EINTERNAL, "internal: bad first-hit batch tables");
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_ereq = o_tile + align16(tiles * sizeof(uint32_t)), o_order = o_ereq + align16(ne * sizeof(uint32_t));
    const size_t o_words = o_order + align16(tiles * sizeof(uint32_t));
    const size_t bytes = o_words + align16(nreq * sizeof(mh::BatchFirstWords));
    if (bytes > kBatchTableBytes || nreq > kBatchResults) return fail(MH_EINTERNAL, "internal: batch pass too large");
    if (pend->toff + bytes > kBatchTableBytes || pend->req_idx.size() + nreq > kBatchResults ||
        (c->prof && c->used == kEventPairs)) {
        const int rc = first_batch_drain(c, reqs, src, pend, out);
        if (rc) return rc;
    }
    uint8_t* h = c->h_btab + pend->toff;
    uint8_t* d = c->d_btab + pend->toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_ereq, ft.entry_req.data(), ne * sizeof(uint32_t));
    memcpy(h + o_order, ft.order.data(), tiles * sizeof(uint32_t));
    mh::BatchFirstWords* hw = (mh::BatchFirstWords*)(h + o_words);
    for (size_t r = 0; r < nreq; ++r) hw[r] = mh::BatchFirstWords{src[reqs[t.req_idx[r]].id].target, ~0ull, 0ull};
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    Timed* tm = nullptr;
    if (c->prof) {  // generic class, with the planned nonces, as the batch launches
        tm = &c->pool[(size_t)c->used++];
        tm->kind = 1;
        tm->var = 0;
        MH_HIP(hipEventRecord(tm->start, c->stream));
    }
    MH_HIP(mh::launch_batch_scan_first((const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile),
                                       (const uint32_t*)(d + o_ereq), (const uint32_t*)(d + o_order),
                                       (mh::BatchFirstWords*)(d + o_words), c->d_partials, (uint32_t)tiles, c->stream));
    if (tm) {
        MH_HIP(hipEventRecord(tm->stop, c->stream));
        c->cnt[4] += t.nonces;
    }
    const size_t roff = pend->req_idx.size();
    MH_HIP(mh::launch_merge_segments_first(c->d_partials, (const uint32_t*)(d + o_seg), (const mh::BatchEntry*)d,
                                           (const uint32_t*)(d + o_tile), (const mh::BatchFirstWords*)(d + o_words),
                                           c->d_fres + roff, (uint32_t)nreq, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_fres + roff, c->d_fres + roff, nreq * sizeof(mh::BatchFirstResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->toff += bytes;
    return MH_OK;
}

// The fused passes of a first-hit batch, under the device's lock.
int first_batch_run_fused(int dev, const mh::BatchRequest* reqs, const mh_first_request* src,
                          const std::vector<mh::BatchItem>& items, int passes, uint32_t slot_cap, mh_first_result* out) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    rc = batch_init_locked(c);
    if (!rc) rc = first_batch_init_locked(c);
    if (rc) return rc;
    const bool rank_major = first_batch_rank_major();
    BatchPending pend;
    mh::BatchTables t;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables(reqs, items, p, &t);
        rc = first_batch_run_pass(c, reqs, src, t, slot_cap, rank_major, &pend, out);
    }
    if (!rc) rc = first_batch_drain(c, reqs, src, &pend, out);
    if (rc) (void)hipStreamSynchronize(c->stream);  // nothing of this call stays in flight
    return rc;
}

// ---- batched first-hit search with fused fast pieces (mh_search_first_batch_ex) ----

int first_batch_fast_init_locked(DevCtx* c) {
    if (!c->d_ftab) MH_HIP(hipMalloc(&c->d_ftab, kFirstBatchFastTableBytes));
    if (!c->h_ftab) MH_HIP(hipHostMalloc(&c->h_ftab, kFirstBatchFastTableBytes, hipHostMallocDefault));
    return MH_OK;
}

// first_batch_run_pass for a pass that holds fast pieces: one H2D copy of all its tables -- entries,
// segments, per-tile entry, per-entry request, tile order, the requests' words with their initial
// values, a GenArgs per request, the fast items (each with its request's target and the device
// addresses of its request's words), per-chunk item and chunk order -- then, on the one stream,
// batch_scan_first_slots for the generic entries, one batch_first<J, MODE> launch per layout in the
// plan's order, merge_segments_first_ex and one D2H copy of {hash, nonce, scanned} per request.
// *toff: bytes of the d_ftab / h_ftab buffer in use by the passes in flight.  The fast launches
// count in the fast class of the profile as batch_run_pass_ex counts them, each piece with its
// planned nonces, skipped chunks included (mh_search_first's rule for its first_scan launches).
// stop (mh_search_first_batch_stop): the fast launches are batch_stop<J, MODE>'s, over the same tables
// in the same order; nothing else of the pass differs.
int first_batch_run_pass_ex(DevCtx* c, const mh::BatchRequest* reqs, const mh_first_request* src,
                            const std::vector<mh::BatchPiece>& pieces, const mh::BatchTables& t,
                            const mh::BatchFastTables& f, uint32_t slot_cap, bool rank_major, bool stop,
                            BatchPending* pend, size_t* toff, mh_first_result* out) {
    mh::FirstBatchFastTables x;
    mh::build_first_batch_tables_ex(t, f, rank_major, &x);
    if (!mh::first_batch_tables_ex_ok(t, f, x, slot_cap)) return fail(MH_EINTERNAL, "internal: bad first-hit batch tables");
    for (size_t k = 0; k < f.items.size(); ++k) {
        const mh::BatchPiece& p = pieces[f.piece[k]];
        if (f.items[k].args.mode >= mh::kModeOneEarly && !early_piece_ok(f.items[k].args, p.J))
            return fail(MH_EINTERNAL, "internal: bad Early piece (an enumerated digit outside word J)");
    }
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t ni = f.items.size(), chunks = f.chunk_item.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_ereq = o_tile + align16(tiles * sizeof(uint32_t)), o_order = o_ereq + align16(ne * sizeof(uint32_t));
    const size_t o_words = o_order + align16(tiles * sizeof(uint32_t));
    const size_t o_gen = o_words + align16(nreq * sizeof(mh::BatchFirstWords));
    const size_t o_item = o_gen + nreq * sizeof(mh::GenArgs), o_chunk = o_item + ni * sizeof(mh::BatchFirstItem);
    const size_t o_corder = o_chunk + align16(chunks * sizeof(uint32_t));
    const size_t bytes = o_corder + align16(chunks * sizeof(uint32_t));
    static_assert(sizeof(mh::GenArgs) % 16 == 0 && sizeof(mh::BatchFirstItem) % 16 == 0, "tables stay 16-byte aligned");
    if (bytes > kFirstBatchFastTableBytes || nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: batch pass too large");
    if (*toff + bytes > kFirstBatchFastTableBytes || pend->req_idx.size() + nreq > kBatchResults ||
        (c->prof && c->used + 1 + (int)f.launches.size() > kEventPairs)) {
        const int rc = first_batch_drain(c, reqs, src, pend, out);
        if (rc) return rc;
        *toff = 0;
    }
    uint8_t* h = c->h_ftab + *toff;
    uint8_t* d = c->d_ftab + *toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_ereq, x.entry_req.data(), ne * sizeof(uint32_t));
    memcpy(h + o_order, x.tile_order.data(), tiles * sizeof(uint32_t));
    mh::BatchFirstWords* hw = (mh::BatchFirstWords*)(h + o_words);
    mh::BatchFirstWords* dw = (mh::BatchFirstWords*)(d + o_words);
    mh::GenArgs* hg = (mh::GenArgs*)(h + o_gen);
    for (size_t r = 0; r < nreq; ++r) {
        hw[r] = mh::BatchFirstWords{src[reqs[t.req_idx[r]].id].target, ~0ull, 0ull};
        mh::make_gen_args(reqs[t.req_idx[r]].pre, &hg[r]);
    }
    mh::BatchFirstItem* hi = (mh::BatchFirstItem*)(h + o_item);
    for (size_t k = 0; k < ni; ++k) {
        const uint32_t r = x.item_req[k];  // < nreq, and the request owns the item's slots (checked above)
        mh::BatchFirstItem it;
        memset(&it, 0, sizeof it);
        it.args = f.items[k].args;
        it.unused = nullptr;
        it.f = mh::FirstArgs{hw[r].target, &dw[r].first, &dw[r].scanned};
        it.chunk0 = f.items[k].chunk0;
        it.slot0 = f.items[k].slot0;
        hi[k] = it;
    }
    memcpy(h + o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t));
    memcpy(h + o_corder, x.chunk_order.data(), chunks * sizeof(uint32_t));
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    if (tiles) {
        Timed* tm = nullptr;
        if (c->prof) {  // generic class, as first_batch_run_pass
            tm = &c->pool[(size_t)c->used++];
            tm->kind = 1;
            tm->var = 0;
            MH_HIP(hipEventRecord(tm->start, c->stream));
        }
        MH_HIP(mh::launch_batch_scan_first_slots((const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile),
                                                 (const uint32_t*)(d + o_ereq), (const uint32_t*)(d + o_order), dw,
                                                 c->d_partials, (uint32_t)tiles, c->stream));
        if (tm) {
            MH_HIP(hipEventRecord(tm->stop, c->stream));
            c->cnt[4] += t.nonces;
        }
    }
    for (const mh::BatchFastLaunch& l : f.launches) {
        Timed* tm = nullptr;
        if (c->prof) {
            tm = &c->pool[(size_t)c->used++];
            tm->kind = 0;
            tm->var = var_index(l.J, l.mode, (int)f.items[l.item0].args.L);
            MH_HIP(hipEventRecord(tm->start, c->stream));
        }
        MH_HIP((stop ? mh::launch_batch_stop : mh::launch_batch_first)(
            c->dev, l.J, l.mode, (const mh::BatchFirstItem*)(d + o_item), (const uint32_t*)(d + o_chunk) + l.chunk0,
            (const uint32_t*)(d + o_corder) + l.chunk0, c->d_partials, l.chunks, c->stream));
        if (tm) {
            MH_HIP(hipEventRecord(tm->stop, c->stream));
            c->cnt[0] += 1;
            c->var[tm->var].launches += 1;
            for (uint32_t k = l.item0; k < l.item0 + l.items; ++k) {
                const mh::BatchPiece& p = pieces[f.piece[k]];
                c->cnt[1] += p.count;
                c->cnt[3] += p.count * (uint64_t)p.ops;
                c->cnt[6] += p.count * (uint64_t)p.nslots;
                VarStat& v = c->var[var_index(p.J, p.mode, p.L)];
                v.nonces += p.count;
                v.ops += p.count * (uint64_t)p.ops;
                v.slots += p.count * (uint64_t)p.nslots;
            }
        }
    }
    const size_t roff = pend->req_idx.size();
    MH_HIP(mh::launch_merge_segments_first_ex(c->d_partials, (const uint32_t*)(d + o_seg), (const mh::GenArgs*)(d + o_gen),
                                              dw, c->d_fres + roff, (uint32_t)nreq, c->stream));
    MH_HIP(hipMemcpyAsync(c->h_fres + roff, c->d_fres + roff, nreq * sizeof(mh::BatchFirstResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    *toff += bytes;
    return MH_OK;
}

// The fused passes of mh_search_first_batch_ex(MH_BATCH_FUSE_FAST), under the device's lock (stop: of
// mh_search_first_batch_stop, first_batch_run_pass_ex).
int first_batch_run_fused_ex(int dev, const mh::BatchRequest* reqs, const mh_first_request* src,
                             const std::vector<mh::BatchPiece>& pieces, const std::vector<mh::FastArgs>& args, int passes,
                             uint32_t slot_cap, bool stop, mh_first_result* out) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    rc = batch_init_locked(c);
    if (!rc) rc = first_batch_init_locked(c);
    if (rc) return rc;
    const bool rank_major = first_batch_rank_major();
    BatchPending pend;
    size_t toff_fast = 0;
    mh::BatchTables t;
    mh::BatchFastTables f;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables_ex(reqs, pieces, args, p, &t, &f);
        if (f.items.empty()) {  // mh_search_first_batch's own pass (slot0 == tile0 throughout)
            rc = first_batch_run_pass(c, reqs, src, t, slot_cap, rank_major, &pend, out);
        } else {
            rc = first_batch_fast_init_locked(c);
            if (!rc) rc = first_batch_run_pass_ex(c, reqs, src, pieces, t, f, slot_cap, rank_major, stop, &pend, &toff_fast, out);
        }
    }
    if (!rc) rc = first_batch_drain(c, reqs, src, &pend, out);
    if (rc) (void)hipStreamSynchronize(c->stream);  // nothing of this call stays in flight
    return rc;
}

// ---- batched hits ----

// The per-request checks of mh_search_hits_batch: batch_requests' and the cap.
void hits_batch_requests(const mh_hits_request* reqs, size_t n, std::vector<int>* status,
                         std::vector<mh::BatchRequest>* valid, std::vector<uint64_t>* caps) {
    status->assign(n, MH_OK);
    valid->clear();
    caps->clear();
    for (size_t i = 0; i < n; ++i) {
        int st = check_common(reqs[i].msg, reqs[i].len);
        if (!st && reqs[i].cap > MH_HITS_MAX_CAP) st = fail(MH_EINVAL, "cap is larger than MH_HITS_MAX_CAP");
        if (!st && reqs[i].lower > reqs[i].upper) st = fail(MH_ERANGE, "lower > upper");
        (*status)[i] = st;
        if (st) continue;
        valid->emplace_back();
        mh::BatchRequest& r = valid->back();
        mh::absorb_prefix(reqs[i].msg, reqs[i].len, &r.pre);
        r.lower = reqs[i].lower;
        r.upper = reqs[i].upper;
        r.id = i;
        caps->push_back(reqs[i].cap);
    }
}

mh::HitsBatchLimits hits_batch_limits() { return mh::HitsBatchLimits{kBatchTableBytes, kBatchResults, hits_slots()}; }

int hits_batch_init_locked(DevCtx* c) {
    if (!c->d_hits) MH_HIP(hipMalloc(&c->d_hits, sizeof(mh::Hit) * MH_HITS_MAX_CAP));
    if (!c->d_hres) MH_HIP(hipMalloc(&c->d_hres, sizeof(mh::BatchHitsResult) * kBatchResults));
    if (!c->h_hres)
        MH_HIP(hipHostMalloc(&c->h_hres, sizeof(mh::BatchHitsResult) * kBatchResults, hipHostMallocDefault));
    if (!c->d_hpacked) MH_HIP(hipMalloc(&c->d_hpacked, sizeof(mh::Hit) * MH_HITS_MAX_CAP));
    if (!c->d_hbase) MH_HIP(hipMalloc(&c->d_hbase, 2 * sizeof(uint64_t)));
    return MH_OK;
}

// The requests of the passes enqueued since the last drain (one window), in h_hres order.
struct HitsBatchPending {
    std::vector<size_t> req_idx;
    std::vector<mh::HitsRegion> region;
    mh::HitsBatchState st;
    uint32_t passes = 0;  // of this window
};

// The end of a window: one synchronise, one copy of the entries the window's regions kept (the
// merges packed them, in request order: min(count, slots) per request), then per request its
// minimum and count, and -- where its region held every hit -- its entries sorted by nonce into
// the caller's buffer.  A request that wanted entries and has more hits than its region had slots
// goes to *rebuild.  pend->st is left to the caller.
int hits_batch_drain(DevCtx* c, const mh::BatchRequest* reqs, const mh_hits_request* src, HitsBatchPending* pend,
                     mh_hit* hits, mh_hits_result* out, std::vector<size_t>* rebuild, std::vector<mh::Hit>* stage) {
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        const int rc = harvest_locked(c);
        if (rc) return rc;
    }
    uint64_t kept = 0;
    for (size_t k = 0; k < pend->req_idx.size(); ++k) kept += std::min(c->h_hres[k].count, pend->region[k].slots);
    if (kept > pend->st.used || kept > MH_HITS_MAX_CAP) return fail(MH_EINTERNAL, "internal: hit window larger than the buffer");
    if (stage->size() < kept) stage->resize((size_t)kept);
    if (kept) MH_HIP(hipMemcpy(stage->data(), c->d_hpacked, (size_t)kept * sizeof(mh::Hit), hipMemcpyDeviceToHost));
    uint64_t pos = 0;  // of the request's entries in the packed order
    for (size_t k = 0; k < pend->req_idx.size(); ++k) {
        const size_t id = reqs[pend->req_idx[k]].id;
        const mh::HitsRegion& g = pend->region[k];
        const mh::BatchHitsResult& res = c->h_hres[k];
        mh_hits_result& r = out[id];
        r.hash = res.hash;
        r.nonce = res.nonce;
        r.count = res.count;
        r.stored = std::min<uint64_t>(res.count, src[id].cap);
        mh::Hit* first = stage->data() + pos;
        pos += std::min(res.count, g.slots);
        if (!src[id].cap) continue;
        if (res.count > g.slots) {  // the region dropped entries; which ones depends on timing
            rebuild->push_back(pend->req_idx[k]);
            continue;
        }
        // count <= slots <= cap: all of them, stored == count
        std::sort(first, first + res.count, [](const mh::Hit& x, const mh::Hit& y) { return x.nonce < y.nonce; });
        for (uint64_t i = 0; i < res.count; ++i) hits[r.offset + i] = mh_hit{first[i].hash, first[i].nonce};
    }
    pend->req_idx.clear();
    pend->region.clear();
    pend->passes = 0;
    return MH_OK;
}

// batch_run_pass over the hits kernels: the pass's one H2D copy also carries the per-entry request
// index and the requests' device words with their initial values (target; cursor = 0; the region),
// so there is no memset and no fill kernel; then batch_scan_hits, merge_segments_hits and one D2H
// copy of {hash, nonce, count} per request.  The passes of one window queue without a synchronise.
int hits_batch_run_pass(DevCtx* c, const mh::BatchRequest* reqs, const mh_hits_request* src, const uint64_t* caps,
                        const mh::BatchTables& t, uint32_t slot_cap, const mh::HitsBatchLimits& lim,
                        HitsBatchPending* pend, mh_hit* hits, mh_hits_result* out, std::vector<size_t>* rebuild,
                        std::vector<mh::Hit>* stage) {
    if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_ereq = o_tile + align16(tiles * sizeof(uint32_t)), o_words = o_ereq + align16(ne * sizeof(uint32_t));
    const size_t bytes = o_words + align16(nreq * sizeof(mh::BatchHitsWords));
    if (bytes != mh::hits_batch_table_bytes(ne, nreq, tiles) || bytes > kBatchTableBytes || nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: batch pass too large");
    if (c->prof && c->used == kEventPairs && !pend->req_idx.empty()) {  // the event pool is full: a drain of its own
        const int rc = hits_batch_drain(c, reqs, src, pend, hits, out, rebuild, stage);
        if (rc) return rc;
        mh::hits_batch_drained(&pend->st);
    }
    mh::HitsBatchTables ht;
    mh::HitsBatchState next = pend->st;
    const bool drain = mh::plan_hits_batch_pass(t, reqs, caps, lim, &next, &ht);
    if (drain) {
        const int rc = hits_batch_drain(c, reqs, src, pend, hits, out, rebuild, stage);
        if (rc) return rc;
    }
    const uint64_t used_before = drain ? 0u : pend->st.used;
    const size_t toff = drain ? 0u : pend->st.toff;
    pend->st = next;
    if (!mh::hits_batch_tables_ok(t, reqs, ht, used_before, std::min<uint64_t>(lim.window_slots, MH_HITS_MAX_CAP)) ||
        toff + bytes > kBatchTableBytes || pend->req_idx.size() + nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: bad hits batch tables");
    uint8_t* h = c->h_btab + toff;
    uint8_t* d = c->d_btab + toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_ereq, ht.entry_req.data(), ne * sizeof(uint32_t));
    mh::BatchHitsWords* hw = (mh::BatchHitsWords*)(h + o_words);
    for (size_t r = 0; r < nreq; ++r)
        hw[r] = mh::BatchHitsWords{src[reqs[t.req_idx[r]].id].target, 0ull, ht.region[r].offset, ht.region[r].slots};
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    Timed* tm = nullptr;
    if (c->prof) {  // generic class, with the planned nonces, as the batch launches
        tm = &c->pool[(size_t)c->used++];
        tm->kind = 1;
        tm->var = 0;
        MH_HIP(hipEventRecord(tm->start, c->stream));
    }
    MH_HIP(mh::launch_batch_scan_hits((const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile),
                                      (const uint32_t*)(d + o_ereq), (mh::BatchHitsWords*)(d + o_words), c->d_hits,
                                      c->d_partials, (uint32_t)tiles, c->stream));
    if (tm) {
        MH_HIP(hipEventRecord(tm->stop, c->stream));
        c->cnt[4] += t.nonces;
    }
    const size_t roff = pend->req_idx.size();
    const unsigned long long* base_in = pend->passes ? (const unsigned long long*)c->d_hbase + (pend->passes & 1u) : nullptr;
    unsigned long long* base_out = (unsigned long long*)c->d_hbase + ((pend->passes + 1u) & 1u);
    MH_HIP(mh::launch_merge_segments_hits(c->d_partials, (const uint32_t*)(d + o_seg),
                                          (const mh::BatchHitsWords*)(d + o_words), c->d_hits, c->d_hpacked,
                                          pend->st.used, base_in, base_out, c->d_hres + roff, (uint32_t)nreq, c->stream));
    ++pend->passes;
    MH_HIP(hipMemcpyAsync(c->h_hres + roff, c->d_hres + roff, nreq * sizeof(mh::BatchHitsResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->region.insert(pend->region.end(), ht.region.begin(), ht.region.end());
    return MH_OK;
}

// The fused passes of a hits batch, under the device's lock.
int hits_batch_run_fused(int dev, const mh::BatchRequest* reqs, const mh_hits_request* src, const uint64_t* caps,
                         const std::vector<mh::BatchItem>& items, int passes, uint32_t slot_cap, mh_hit* hits,
                         mh_hits_result* out, std::vector<size_t>* rebuild) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    rc = batch_init_locked(c);
    if (!rc) rc = hits_batch_init_locked(c);
    if (rc) return rc;
    const mh::HitsBatchLimits lim = hits_batch_limits();
    HitsBatchPending pend;
    std::vector<mh::Hit> stage;
    mh::BatchTables t;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables(reqs, items, p, &t);
        rc = hits_batch_run_pass(c, reqs, src, caps, t, slot_cap, lim, &pend, hits, out, rebuild, &stage);
    }
    if (!rc) rc = hits_batch_drain(c, reqs, src, &pend, hits, out, rebuild, &stage);
    if (rc) (void)hipStreamSynchronize(c->stream);  // nothing of this call stays in flight
    return rc;
}

// ---- batched hits with fused fast pieces (mh_search_hits_batch_ex) ----

// hits_batch_run_pass for a pass that holds fast pieces: one H2D copy of all its tables -- entries,
// segments, per-tile entry, per-entry request, the requests' words with their initial values
// (cursor = 0), the fast items (each with its request's target, the device address of its request's
// cursor and its request's region of the device hit buffer) and per-chunk item -- then, on the one
// stream, batch_scan_hits_slots for the generic entries, one batch_hits<J, MODE> launch per layout
// in the plan's order, merge_segments_hits (it reads segments and words, so it serves slot segments
// unchanged) and one D2H copy of {hash, nonce, count} per request.  Windows, regions and drains are
// hits_batch_run_pass's; the items and the per-chunk table count against the window's table buffer.
// The fast launches count in the fast class of the profile as batch_run_pass_ex counts them.
int hits_batch_run_pass_ex(DevCtx* c, const mh::BatchRequest* reqs, const mh_hits_request* src, const uint64_t* caps,
                           const std::vector<mh::BatchPiece>& pieces, const mh::BatchTables& t,
                           const mh::BatchFastTables& f, uint32_t slot_cap, const mh::HitsBatchLimits& lim,
                           HitsBatchPending* pend, mh_hit* hits, mh_hits_result* out, std::vector<size_t>* rebuild,
                           std::vector<mh::Hit>* stage) {
    if (!mh::batch_tables_ex_ok(t, f, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
    for (size_t k = 0; k < f.items.size(); ++k) {
        const mh::BatchPiece& p = pieces[f.piece[k]];
        if (f.items[k].args.mode >= mh::kModeOneEarly && !early_piece_ok(f.items[k].args, p.J))
            return fail(MH_EINTERNAL, "internal: bad Early piece (an enumerated digit outside word J)");
    }
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const size_t ni = f.items.size(), chunks = f.chunk_item.size();
    const size_t o_seg = align16(ne * sizeof(mh::BatchEntry)), o_tile = o_seg + align16((nreq + 1u) * sizeof(uint32_t));
    const size_t o_ereq = o_tile + align16(tiles * sizeof(uint32_t)), o_words = o_ereq + align16(ne * sizeof(uint32_t));
    const size_t o_item = o_words + align16(nreq * sizeof(mh::BatchHitsWords));
    const size_t o_chunk = o_item + ni * sizeof(mh::BatchHitsItem);
    const size_t bytes = o_chunk + align16(chunks * sizeof(uint32_t));
    static_assert(sizeof(mh::BatchHitsItem) % 16 == 0 && sizeof(mh::BatchHitsWords) % 16 == 0, "tables stay 16-byte aligned");
    if (bytes != mh::hits_batch_table_bytes_ex(ne, nreq, tiles, ni, chunks) || bytes > kBatchTableBytes ||
        nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: batch pass too large");
    // the event pool cannot take the pass's launches: a drain of its own
    if (c->prof && c->used + 1 + (int)f.launches.size() > kEventPairs) {
        const int rc = hits_batch_drain(c, reqs, src, pend, hits, out, rebuild, stage);
        if (rc) return rc;
        mh::hits_batch_drained(&pend->st);
    }
    mh::HitsBatchFastTables x;
    mh::HitsBatchState next = pend->st;
    const bool drain = mh::plan_hits_batch_pass_ex(t, f, reqs, caps, lim, &next, &x);
    if (drain) {
        const int rc = hits_batch_drain(c, reqs, src, pend, hits, out, rebuild, stage);
        if (rc) return rc;
    }
    const uint64_t used_before = drain ? 0u : pend->st.used;
    const size_t toff = drain ? 0u : pend->st.toff;
    pend->st = next;
    if (!mh::hits_batch_tables_ex_ok(t, f, reqs, x, slot_cap, used_before,
                                     std::min<uint64_t>(lim.window_slots, MH_HITS_MAX_CAP)) ||
        toff + bytes > kBatchTableBytes || pend->req_idx.size() + nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: bad hits batch tables");
    uint8_t* h = c->h_btab + toff;
    uint8_t* d = c->d_btab + toff;
    memcpy(h, t.entries.data(), ne * sizeof(mh::BatchEntry));
    memcpy(h + o_seg, t.seg.data(), (nreq + 1u) * sizeof(uint32_t));
    memcpy(h + o_tile, t.tile_entry.data(), tiles * sizeof(uint32_t));
    memcpy(h + o_ereq, x.h.entry_req.data(), ne * sizeof(uint32_t));
    mh::BatchHitsWords* hw = (mh::BatchHitsWords*)(h + o_words);
    mh::BatchHitsWords* dw = (mh::BatchHitsWords*)(d + o_words);
    for (size_t r = 0; r < nreq; ++r)
        hw[r] = mh::BatchHitsWords{src[reqs[t.req_idx[r]].id].target, 0ull, x.h.region[r].offset, x.h.region[r].slots};
    mh::BatchHitsItem* hi = (mh::BatchHitsItem*)(h + o_item);
    for (size_t k = 0; k < ni; ++k) {
        const uint32_t r = x.item_req[k];  // < nreq, and the request owns the item's slots (checked above)
        mh::BatchHitsItem it;
        memset(&it, 0, sizeof it);
        it.args = f.items[k].args;
        it.unused = nullptr;
        // the region lies inside the window, the window inside the device hit buffer (checked above)
        it.h = mh::HitsArgs{hw[r].target, &dw[r].cursor, c->d_hits + hw[r].offset, hw[r].slots};
        it.chunk0 = f.items[k].chunk0;
        it.slot0 = f.items[k].slot0;
        hi[k] = it;
    }
    memcpy(h + o_chunk, f.chunk_item.data(), chunks * sizeof(uint32_t));
    MH_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    if (tiles) {
        Timed* tm = nullptr;
        if (c->prof) {  // generic class, as hits_batch_run_pass
            tm = &c->pool[(size_t)c->used++];
            tm->kind = 1;
            tm->var = 0;
            MH_HIP(hipEventRecord(tm->start, c->stream));
        }
        MH_HIP(mh::launch_batch_scan_hits_slots((const mh::BatchEntry*)d, (const uint32_t*)(d + o_tile),
                                                (const uint32_t*)(d + o_ereq), dw, c->d_hits, c->d_partials,
                                                (uint32_t)tiles, c->stream));
        if (tm) {
            MH_HIP(hipEventRecord(tm->stop, c->stream));
            c->cnt[4] += t.nonces;
        }
    }
    for (const mh::BatchFastLaunch& l : f.launches) {
        Timed* tm = nullptr;
        if (c->prof) {
            tm = &c->pool[(size_t)c->used++];
            tm->kind = 0;
            tm->var = var_index(l.J, l.mode, (int)f.items[l.item0].args.L);
            MH_HIP(hipEventRecord(tm->start, c->stream));
        }
        MH_HIP(mh::launch_batch_hits(c->dev, l.J, l.mode, (const mh::BatchHitsItem*)(d + o_item),
                                     (const uint32_t*)(d + o_chunk) + l.chunk0, c->d_partials, l.chunks, c->stream));
        if (tm) {
            MH_HIP(hipEventRecord(tm->stop, c->stream));
            c->cnt[0] += 1;
            c->var[tm->var].launches += 1;
            for (uint32_t k = l.item0; k < l.item0 + l.items; ++k) {
                const mh::BatchPiece& p = pieces[f.piece[k]];
                c->cnt[1] += p.count;
                c->cnt[3] += p.count * (uint64_t)p.ops;
                c->cnt[6] += p.count * (uint64_t)p.nslots;
                VarStat& v = c->var[var_index(p.J, p.mode, p.L)];
                v.nonces += p.count;
                v.ops += p.count * (uint64_t)p.ops;
                v.slots += p.count * (uint64_t)p.nslots;
            }
        }
    }
    const size_t roff = pend->req_idx.size();
    const unsigned long long* base_in = pend->passes ? (const unsigned long long*)c->d_hbase + (pend->passes & 1u) : nullptr;
    unsigned long long* base_out = (unsigned long long*)c->d_hbase + ((pend->passes + 1u) & 1u);
    MH_HIP(mh::launch_merge_segments_hits(c->d_partials, (const uint32_t*)(d + o_seg), dw, c->d_hits, c->d_hpacked,
                                          pend->st.used, base_in, base_out, c->d_hres + roff, (uint32_t)nreq, c->stream));
    ++pend->passes;
    MH_HIP(hipMemcpyAsync(c->h_hres + roff, c->d_hres + roff, nreq * sizeof(mh::BatchHitsResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->region.insert(pend->region.end(), x.h.region.begin(), x.h.region.end());
    return MH_OK;
}

// The fused passes of mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST), under the device's lock.
int hits_batch_run_fused_ex(int dev, const mh::BatchRequest* reqs, const mh_hits_request* src, const uint64_t* caps,
                            const std::vector<mh::BatchPiece>& pieces, const std::vector<mh::FastArgs>& args, int passes,
                            uint32_t slot_cap, mh_hit* hits, mh_hits_result* out, std::vector<size_t>* rebuild) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    rc = batch_init_locked(c);
    if (!rc) rc = hits_batch_init_locked(c);
    if (rc) return rc;
    const mh::HitsBatchLimits lim = hits_batch_limits();
    HitsBatchPending pend;
    std::vector<mh::Hit> stage;
    mh::BatchTables t;
    mh::BatchFastTables f;
    for (int p = 0; p < passes && !rc; ++p) {
        mh::build_batch_tables_ex(reqs, pieces, args, p, &t, &f);
        // a pass without a fast piece is mh_search_hits_batch's own pass (slot0 == tile0 throughout)
        rc = f.items.empty()
                 ? hits_batch_run_pass(c, reqs, src, caps, t, slot_cap, lim, &pend, hits, out, rebuild, &stage)
                 : hits_batch_run_pass_ex(c, reqs, src, caps, pieces, t, f, slot_cap, lim, &pend, hits, out, rebuild,
                                          &stage);
    }
    if (!rc) rc = hits_batch_drain(c, reqs, src, &pend, hits, out, rebuild, &stage);
    if (rc) (void)hipStreamSynchronize(c->stream);  // nothing of this call stays in flight
    return rc;
}

// ---- batched first k hits (mh_search_first_hits_batch) ----

// The per-request checks of mh_search_first_hits_batch: batch_requests' and k; per valid request its
// target, k and want (plan.hpp first_hits_batch_want), indexed as `valid`.
void first_hits_batch_requests(const mh_first_hits_request* reqs, size_t n, std::vector<int>* status,
                               std::vector<mh::BatchRequest>* valid, std::vector<uint64_t>* targets,
                               std::vector<uint64_t>* ks, std::vector<uint64_t>* wants) {
    status->assign(n, MH_OK);
    valid->clear();
    targets->clear();
    ks->clear();
    wants->clear();
    for (size_t i = 0; i < n; ++i) {
        int st = check_common(reqs[i].msg, reqs[i].len);
        if (!st && reqs[i].k == 0) st = fail(MH_EINVAL, "k is 0");
        if (!st && reqs[i].k > MH_HITS_MAX_CAP) st = fail(MH_EINVAL, "k is larger than MH_HITS_MAX_CAP");
        if (!st && reqs[i].lower > reqs[i].upper) st = fail(MH_ERANGE, "lower > upper");
        (*status)[i] = st;
        if (st) continue;
        valid->emplace_back();
        mh::BatchRequest& r = valid->back();
        mh::absorb_prefix(reqs[i].msg, reqs[i].len, &r.pre);
        r.lower = reqs[i].lower;
        r.upper = reqs[i].upper;
        r.id = i;
        targets->push_back(reqs[i].target);
        ks->push_back(reqs[i].k);
        wants->push_back(mh::first_hits_batch_want(reqs[i].k));
    }
}

mh::HitsBatchLimits first_hits_batch_limits() {
    return mh::HitsBatchLimits{kFirstBatchFastTableBytes, kBatchResults, hits_slots()};
}

int first_hits_batch_init_locked(DevCtx* c) {
    if (!c->d_kres) MH_HIP(hipMalloc(&c->d_kres, sizeof(mh::BatchBoundResult) * kBatchResults));
    if (!c->h_kres)
        MH_HIP(hipHostMalloc(&c->h_kres, sizeof(mh::BatchBoundResult) * kBatchResults, hipHostMallocDefault));
    if (!c->d_bslices)
        MH_HIP(hipMalloc(&c->d_bslices, sizeof(uint32_t) * mh::kFirstHitsSlices * mh::kBatchMaxRequests));
    return MH_OK;
}

// What a call hands to its passes and drains.
struct FirstHitsBatchCall {
    const mh::BatchRequest* reqs;
    const mh_first_hits_request* src;
    const uint64_t *targets, *ks, *wants;  // indexed as reqs
    mh_hit* hits;
    mh_first_hits_result* out;
    std::vector<size_t>* rebuild;
    std::vector<mh::Hit> stage;
};

// The end of a window, as hits_batch_drain: one synchronise, one copy of the entries the window's
// regions kept, then the host's reading of every request (plan.hpp read_first_hits_batch): a request
// whose region dropped entries goes to *rebuild; any other has its entries sorted by nonce into the
// caller's buffer, stored = min(count, k), and with stored == k the minimum of those k, with fewer
// the merged minimum -- nothing of it was then skipped, so scanned must be its whole range.
int first_hits_batch_drain(DevCtx* c, FirstHitsBatchCall* call, HitsBatchPending* pend) {
    MH_HIP(hipStreamSynchronize(c->stream));
    if (c->prof) {
        const int rc = harvest_locked(c);
        if (rc) return rc;
    }
    uint64_t kept = 0;
    for (size_t k = 0; k < pend->req_idx.size(); ++k) kept += std::min(c->h_kres[k].count, pend->region[k].slots);
    if (kept > pend->st.used || kept > MH_HITS_MAX_CAP) return fail(MH_EINTERNAL, "internal: hit window larger than the buffer");
    if (call->stage.size() < kept) call->stage.resize((size_t)kept);
    if (kept) MH_HIP(hipMemcpy(call->stage.data(), c->d_hpacked, (size_t)kept * sizeof(mh::Hit), hipMemcpyDeviceToHost));
    uint64_t pos = 0;  // of the request's entries in the packed order
    for (size_t k = 0; k < pend->req_idx.size(); ++k) {
        const size_t idx = pend->req_idx[k];
        const mh::BatchRequest& q = call->reqs[idx];
        const mh::HitsRegion& g = pend->region[k];
        const mh::BatchBoundResult& res = c->h_kres[k];
        mh_first_hits_result& r = call->out[q.id];
        mh::Hit* first = call->stage.data() + pos;
        pos += std::min(res.count, g.slots);
        r.scanned = res.scanned;
        r.path = 0;
        uint64_t stored = 0, hash = res.hash, nonce = res.nonce;
        if (!mh::read_first_hits_batch(first, res.count, g.slots, call->ks[idx], &stored, &hash, &nonce)) {
            call->rebuild->push_back(idx);
            continue;
        }
        if (stored < call->ks[idx] && res.scanned != q.upper - q.lower + 1u)
            return fail(MH_EINTERNAL, "internal: fewer than k hits, but the fused scan did not hash the whole range");
        r.stored = stored;
        r.hash = hash;
        r.nonce = nonce;
        for (uint64_t i = 0; i < stored; ++i) call->hits[r.offset + i] = mh_hit{first[i].hash, first[i].nonce};
    }
    pend->req_idx.clear();
    pend->region.clear();
    pend->passes = 0;
    return MH_OK;
}

// One pass: its image (plan.cpp build_first_hits_batch_image: every table, the requests' words with
// their initial values, the items with the addresses of their request's words, region and counters)
// checked and copied in one H2D copy, a memset of the pass's slice counters, then on the one stream
// batch_scan_bound[_slots] for the generic entries, one batch_bound<J, MODE> launch per layout in the
// plan's order, merge_segments_bound and one D2H copy of {hash, nonce, count, scanned} per request.
// Windows, regions and drains are hits_batch_run_pass_ex's with the wants in the caps' place; the
// profile counts the launches as that function does.
int first_hits_batch_run_pass(DevCtx* c, FirstHitsBatchCall* call, const std::vector<mh::BatchPiece>* pieces,
                              const mh::BatchTables& t, const mh::BatchFastTables& f, uint32_t slot_cap,
                              const mh::HitsBatchLimits& lim, bool rank_major, HitsBatchPending* pend) {
    for (size_t k = 0; k < f.items.size(); ++k) {
        const mh::BatchPiece& p = (*pieces)[f.piece[k]];
        if (f.items[k].args.mode >= mh::kModeOneEarly && !early_piece_ok(f.items[k].args, p.J))
            return fail(MH_EINTERNAL, "internal: bad Early piece (an enumerated digit outside word J)");
    }
    const size_t ne = t.entries.size(), nreq = t.req_idx.size(), tiles = t.tile_entry.size();
    const mh::FirstHitsBatchLayout l = mh::first_hits_batch_layout(ne, nreq, tiles, f.items.size(), f.chunk_item.size());
    if (l.bytes > kFirstBatchFastTableBytes || nreq > kBatchResults || nreq > mh::kBatchMaxRequests)
        return fail(MH_EINTERNAL, "internal: batch pass too large");
    // the event pool cannot take the pass's launches: a drain of its own
    if (c->prof && c->used + 1 + (int)f.launches.size() > kEventPairs) {
        const int rc = first_hits_batch_drain(c, call, pend);
        if (rc) return rc;
        mh::hits_batch_drained(&pend->st);
    }
    mh::FirstHitsBatchTables x;
    mh::HitsBatchState next = pend->st;
    const bool drain = mh::plan_first_hits_batch_pass(t, f, call->reqs, call->wants, lim, rank_major, &next, &x);
    if (drain) {
        const int rc = first_hits_batch_drain(c, call, pend);
        if (rc) return rc;
    }
    const uint64_t used_before = drain ? 0u : pend->st.used;
    const size_t toff = drain ? 0u : pend->st.toff;
    pend->st = next;
    const uint64_t window = std::min<uint64_t>(lim.window_slots, MH_HITS_MAX_CAP);
    if (!mh::first_hits_batch_tables_ok(t, f, call->reqs, x, slot_cap, used_before, window) ||
        toff + l.bytes > kFirstBatchFastTableBytes || pend->req_idx.size() + nreq > kBatchResults)
        return fail(MH_EINTERNAL, "internal: bad first-hits batch tables");
    uint8_t* h = c->h_ftab + toff;
    uint8_t* d = c->d_ftab + toff;
    const mh::FirstHitsBatchAddrs at{(uint64_t)(uintptr_t)d, (uint64_t)(uintptr_t)c->d_hits, (uint64_t)(uintptr_t)c->d_bslices};
    mh::build_first_hits_batch_image(t, f, x, call->reqs, call->targets, call->ks, at, h);
    if (!mh::first_hits_batch_image_ok(t, f, x, call->reqs, at, window, h))
        return fail(MH_EINTERNAL, "internal: bad first-hits batch image");
    MH_HIP(hipMemcpyAsync(d, h, l.bytes, hipMemcpyHostToDevice, c->stream));
    MH_HIP(hipMemsetAsync(c->d_bslices, 0, nreq * sizeof(uint32_t) * mh::kFirstHitsSlices, c->stream));
    mh::BatchBoundWords* dw = (mh::BatchBoundWords*)(d + l.o_words);
    if (tiles) {
        Timed* tm = nullptr;
        if (c->prof) {  // generic class, as hits_batch_run_pass
            tm = &c->pool[(size_t)c->used++];
            tm->kind = 1;
            tm->var = 0;
            MH_HIP(hipEventRecord(tm->start, c->stream));
        }
        MH_HIP(mh::launch_batch_scan_bound(!f.items.empty(), (const mh::BatchEntry*)d, (const uint32_t*)(d + l.o_tile),
                                           (const uint32_t*)(d + l.o_ereq), (const uint32_t*)(d + l.o_order), dw,
                                           c->d_bslices, c->d_hits, c->d_partials, (uint32_t)tiles, c->stream));
        if (tm) {
            MH_HIP(hipEventRecord(tm->stop, c->stream));
            c->cnt[4] += t.nonces;
        }
    }
    for (const mh::BatchFastLaunch& fl : f.launches) {
        Timed* tm = nullptr;
        if (c->prof) {
            tm = &c->pool[(size_t)c->used++];
            tm->kind = 0;
            tm->var = var_index(fl.J, fl.mode, (int)f.items[fl.item0].args.L);
            MH_HIP(hipEventRecord(tm->start, c->stream));
        }
        MH_HIP(mh::launch_batch_bound(c->dev, fl.J, fl.mode, (const mh::BatchBoundItem*)(d + l.o_item),
                                      (const uint32_t*)(d + l.o_chunk) + fl.chunk0,
                                      (const uint32_t*)(d + l.o_corder) + fl.chunk0, c->d_partials, fl.chunks, c->stream));
        if (tm) {
            MH_HIP(hipEventRecord(tm->stop, c->stream));
            c->cnt[0] += 1;
            c->var[tm->var].launches += 1;
            for (uint32_t k = fl.item0; k < fl.item0 + fl.items; ++k) {
                const mh::BatchPiece& p = (*pieces)[f.piece[k]];
                c->cnt[1] += p.count;
                c->cnt[3] += p.count * (uint64_t)p.ops;
                c->cnt[6] += p.count * (uint64_t)p.nslots;
                VarStat& v = c->var[var_index(p.J, p.mode, p.L)];
                v.nonces += p.count;
                v.ops += p.count * (uint64_t)p.ops;
                v.slots += p.count * (uint64_t)p.nslots;
            }
        }
    }
    const size_t roff = pend->req_idx.size();
    const unsigned long long* base_in = pend->passes ? (const unsigned long long*)c->d_hbase + (pend->passes & 1u) : nullptr;
    unsigned long long* base_out = (unsigned long long*)c->d_hbase + ((pend->passes + 1u) & 1u);
    MH_HIP(mh::launch_merge_segments_bound(c->d_partials, (const uint32_t*)(d + l.o_seg), dw, c->d_hits, c->d_hpacked,
                                           pend->st.used, base_in, base_out, c->d_kres + roff, (uint32_t)nreq, c->stream));
    ++pend->passes;
    MH_HIP(hipMemcpyAsync(c->h_kres + roff, c->d_kres + roff, nreq * sizeof(mh::BatchBoundResult), hipMemcpyDeviceToHost,
                          c->stream));
    pend->req_idx.insert(pend->req_idx.end(), t.req_idx.begin(), t.req_idx.end());
    pend->region.insert(pend->region.end(), x.region.begin(), x.region.end());
    return MH_OK;
}

// The fused passes of mh_search_first_hits_batch, under the device's lock.  items: the plan of
// flags == 0 (plan_batch); else pieces and args (plan_batch_ex).
int first_hits_batch_run_fused(int dev, FirstHitsBatchCall* call, const std::vector<mh::BatchItem>* items,
                               const std::vector<mh::BatchPiece>* pieces, const std::vector<mh::FastArgs>* args, int passes,
                               uint32_t slot_cap) {
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    rc = batch_init_locked(c);
    if (!rc) rc = hits_batch_init_locked(c);
    if (!rc) rc = first_batch_fast_init_locked(c);
    if (!rc) rc = first_hits_batch_init_locked(c);
    if (rc) return rc;
#ifdef MH_DEV_HOOKS
    c->keep = 0;  // mh_search_first_hits_batch refused the hash hooks; nothing of an earlier search's stays
    c->keep_fast = c->xor_on = c->xor_fast = false;
#endif
    const mh::HitsBatchLimits lim = first_hits_batch_limits();
    const bool rank_major = first_batch_rank_major();
    HitsBatchPending pend;
    mh::BatchTables t;
    mh::BatchFastTables f;
    for (int p = 0; p < passes && !rc; ++p) {
        if (items)
            mh::build_batch_tables(call->reqs, *items, p, &t);
        else
            mh::build_batch_tables_ex(call->reqs, *pieces, *args, p, &t, &f);
        rc = first_hits_batch_run_pass(c, call, pieces, t, f, slot_cap, lim, rank_major, &pend);
    }
    if (!rc) rc = first_hits_batch_drain(c, call, &pend);
    if (rc) (void)hipStreamSynchronize(c->stream);  // nothing of this call stays in flight
    return rc;
}

// mh_search_batch_ex(MH_BATCH_FUSE_FAST) over n >= 1 requests, the fallbacks through `fallback`.
int search_batch_ex_impl(int dev, const mh_request* reqs, size_t n, mh_result* out, const BatchFallback& fallback) {
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    batch_requests(reqs, n, &status, &valid);
    for (size_t i = 0; i < n; ++i) out[i] = mh_result{status[i], 0, 0, 0};
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(valid.data(), valid.size(), plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(),
                      &pieces, &args);
    int passes = 0;
    for (const mh::BatchPiece& p : pieces)
        if (p.kind != 1) passes = std::max(passes, p.pass + 1);
    if (passes) {
        const int rc = batch_run_fused_ex(dev, valid.data(), pieces, args, passes, slot_cap, out);
        if (rc) return rc;
    }
    for (const mh::BatchPiece& p : pieces) {  // the fallbacks, after the fused passes
        if (p.kind != 1) continue;
        const mh::BatchRequest& r = valid[p.idx];
        const int rc = fallback(r, &out[r.id].hash, &out[r.id].nonce);
        if (rc) return rc;
    }
    return MH_OK;
}

}  // namespace

extern "C" {

int mh_abi_version(void) { return MH_ABI_VERSION; }

int mh_device_count(void) { return device_count_impl(); }

const char* mh_last_error(void) { return g_err.c_str(); }

int mh_search(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t* out_hash,
              uint64_t* out_nonce) {
    g_err.clear();
    if (!out_hash || !out_nonce) return fail(MH_EINVAL, "NULL output pointer");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    return search_impl(dev, pre, lower, upper, out_hash, out_nonce);
}

int mh_search_first(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                    mh_first* out) {
    return mh_search_first_ex(dev, msg, len, lower, upper, target, 0u, out);
}

int mh_search_first_ex(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                       uint32_t flags, mh_first* out) {
    g_err.clear();
    if (flags & ~MH_FIRST_STOP_RUNNING) return fail(MH_EINVAL, "unknown flag bit");
    if (!out) return fail(MH_EINVAL, "NULL output pointer");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
#ifdef MH_DEV_HOOKS
    // the first-hit kernels have no variants of these hooks: refuse, never ignore them
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string("mh_search_first does not support ") + hook);
#endif
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    return search_first_impl(dev, pre, lower, upper, target, flags, out);
}

int mh_search_hits(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                   mh_hit* hits, size_t cap, mh_hits* out) {
    g_err.clear();
    if (!out) return fail(MH_EINVAL, "NULL output pointer");
    if (cap > MH_HITS_MAX_CAP) return fail(MH_EINVAL, "cap is larger than MH_HITS_MAX_CAP");
    if (!hits && cap > 0) return fail(MH_EINVAL, "hits is NULL with cap > 0");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
#ifdef MH_DEV_HOOKS
    // the hits kernels have no variants of these hooks: refuse, never ignore them
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string("mh_search_hits does not support ") + hook);
#endif
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    return search_hits_impl(dev, pre, lower, upper, target, hits, cap, out);
}

int mh_search_first_hits(int dev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, uint64_t target,
                         mh_hit* hits, size_t k, mh_first_hits* out) {
    g_err.clear();
    if (!out) return fail(MH_EINVAL, "NULL output pointer");
    if (!hits) return fail(MH_EINVAL, "hits is NULL");
    if (k == 0) return fail(MH_EINVAL, "k is 0");
    if (k > MH_HITS_MAX_CAP) return fail(MH_EINVAL, "k is larger than MH_HITS_MAX_CAP");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
#ifdef MH_DEV_HOOKS
    // the stopping hits kernels have no variants of these hooks: refuse, never ignore them
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string("mh_search_first_hits does not support ") + hook);
#endif
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    return search_first_hits_impl(dev, pre, lower, upper, target, hits, k, out);
}

int mh_first_hits_slices(uint64_t lower, uint64_t upper, uint32_t* shift, uint32_t* slices) {
    g_err.clear();
    if (!shift || !slices) return fail(MH_EINVAL, "NULL output pointer");
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    *shift = mh::first_hits_shift(upper - lower);
    *slices = mh::first_hits_slices(upper - lower, *shift);
    return MH_OK;
}

uint64_t mh_first_hits_bound(uint64_t lower, uint64_t upper, uint64_t k, const uint32_t* counts) {
    if (!counts || k == 0 || lower > upper) return ~0ull;
    return mh::first_hits_bound(lower, upper - lower, mh::first_hits_shift(upper - lower), k, counts);
}

int mh_search_multi(const int* devs, int ndev, const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper,
                    uint64_t chunk, uint64_t* out_hash, uint64_t* out_nonce) {
    g_err.clear();
    if (!out_hash || !out_nonce || !devs || ndev <= 0) return fail(MH_EINVAL, "bad arguments");
    if (ndev > MH_MAX_WORKERS) return fail(MH_EINVAL, "more than MH_MAX_WORKERS devices listed");
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    const int n = mh_device_count();
    for (int i = 0; i < ndev; ++i)
        if (devs[i] < 0 || devs[i] >= n) return fail(n <= 0 ? MH_ENODEV : MH_EINVAL, "device index out of range");
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    // One device and adaptive chunks: nothing to balance, so one search (one
    // plan, full-size launches) instead of a chain of shrinking chunks.
    // test hook of the dev build only (`make dev`, -DMH_DEV_HOOKS):
    // MINEHIP_TEST_FAIL_WORKER=i makes worker i's first search fail with
    // MH_EHIP, to exercise the hand-back path on a one-GPU box
    int fail_worker = -1;
    // MINEHIP_TEST_SPAWN_LIMIT=k (dev build only): the host thread of every worker after the first
    // k fails to start (std::system_error, as when the process is out of threads), so the
    // start-failure path of both coordinators runs on any box
    mh::ThreadStart start;
#ifdef MH_DEV_HOOKS
    if (const char* e = getenv("MINEHIP_TEST_FAIL_WORKER")) fail_worker = atoi(e);
    if (const char* e = getenv("MINEHIP_TEST_SPAWN_LIMIT")) {
        auto started = std::make_shared<std::atomic<int>>(0);
        const int limit = atoi(e);
        start = [started, limit](std::function<void()> fn) {
            if ((*started)++ >= limit)
                throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
            return std::thread(std::move(fn));
        };
    }
#endif
    if (ndev == 1 && chunk == 0 && fail_worker < 0 && !start)
        return search_impl(devs[0], pre, lower, upper, out_hash, out_nonce);
    // Adaptive: one rate-weighted shard per device (+ a short dynamic tail on long ranges), multi.hpp.
    if (chunk == 0) {
        const mh::SpanSearch search = [&](int worker, int dev, uint64_t lo, uint64_t hi, uint64_t* h, uint64_t* n,
                                          uint64_t* ns, std::string* err) {
            const int r = (worker == fail_worker) ? fail(MH_EHIP, "injected failure (dev build test hook)")
                                                  : search_impl(dev, pre, lo, hi, h, n, ns);
            if (r) *err = g_err;  // this worker thread's description
            return r;
        };
        std::string err;
        const int r = mh::search_shards(devs, ndev, pre, lower, upper, plan_opts(), search, out_hash, out_nonce, &err,
                                        start);
        return r ? fail(r, err) : MH_OK;
    }
    // Fixed chunks: one miner per listed device, fed by the server's scheduler (sched.hpp) with
    // chunks of exactly `chunk` nonces (multi.cpp search_chunks).  A device that fails hands its
    // chunk back to the others.
    const mh::ChunkSearch csearch = [&](int worker, uint64_t lo, uint64_t hi, uint64_t* h, uint64_t* nn,
                                        std::string* err) {
        const int r = (worker == fail_worker) ? fail(MH_EHIP, "injected failure (dev build test hook)")
                                              : search_impl(devs[worker], pre, lo, hi, h, nn);
        if (r) *err = g_err;
        return r;
    };
    std::string err;
    const int r = mh::search_chunks(ndev, msg, len, lower, upper, chunk, csearch, out_hash, out_nonce, &err, start);
    return r ? fail(r, err) : MH_OK;
}

int mh_search_batch(int dev, const mh_request* reqs, size_t n, mh_result* out) {
    g_err.clear();
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    return search_batch_impl(dev, reqs, n, out, [dev](const mh::BatchRequest& r, uint64_t* h, uint64_t* nn) {
        return search_impl(dev, r.pre, r.lower, r.upper, h, nn);
    });
}

int mh_search_batch_ex(int dev, const mh_request* reqs, size_t n, uint32_t flags, mh_result* out) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) return mh_search_batch(dev, reqs, n, out);
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
    return search_batch_ex_impl(dev, reqs, n, out, [dev](const mh::BatchRequest& r, uint64_t* h, uint64_t* nn) {
        return search_impl(dev, r.pre, r.lower, r.upper, h, nn);
    });
}

int64_t mh_batch_plan_ex(const mh_request* reqs, size_t n, uint32_t flags, mh_batch_piece* out, int64_t cap) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<mh::BatchRequest> all(n);
    for (size_t i = 0; i < n; ++i) {
        const int rc = check_common(reqs[i].msg, reqs[i].len);
        if (rc) return rc;
        if (reqs[i].lower > reqs[i].upper) return fail(MH_ERANGE, "lower > upper");
        mh::absorb_prefix(reqs[i].msg, reqs[i].len, &all[i].pre);
        all[i].lower = reqs[i].lower;
        all[i].upper = reqs[i].upper;
        all[i].id = i;
    }
    int64_t k = 0;
    if (!(flags & MH_BATCH_FUSE_FAST)) {  // mh_batch_plan's plan in the new struct
        std::vector<mh::BatchItem> items;
        mh::plan_batch(all.data(), n, plan_opts(), batch_slots(), &items);
        for (const mh::BatchItem& it : items) {
            if (k >= cap) return cap + 1;  // cap + 1 signals truncation
            if (out) out[k] = mh_batch_piece{it.req, it.first, it.count, it.kind, it.pass, it.slot, it.slots, 0, 0, 0, -1};
            ++k;
        }
        return k;
    }
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(all.data(), n, plan_opts(), batch_slots(), batch_fast_shared_lanes(), batch_fast_max(), &pieces,
                      &args);
    for (const mh::BatchPiece& p : pieces) {
        if (k >= cap) return cap + 1;
        if (out)
            out[k] = mh_batch_piece{p.req, p.first, p.count, p.kind, p.pass, p.slot, p.slots, p.J, p.mode, p.L, p.launch};
        ++k;
    }
    return k;
}

int64_t mh_batch_plan(const mh_request* reqs, size_t n, mh_batch_item* out, int64_t cap) {
    g_err.clear();
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<mh::BatchRequest> all(n);
    for (size_t i = 0; i < n; ++i) {
        const int rc = check_common(reqs[i].msg, reqs[i].len);
        if (rc) return rc;
        if (reqs[i].lower > reqs[i].upper) return fail(MH_ERANGE, "lower > upper");
        mh::absorb_prefix(reqs[i].msg, reqs[i].len, &all[i].pre);
        all[i].lower = reqs[i].lower;
        all[i].upper = reqs[i].upper;
        all[i].id = i;
    }
    std::vector<mh::BatchItem> items;
    mh::plan_batch(all.data(), n, plan_opts(), batch_slots(), &items);
    int64_t k = 0;
    for (const mh::BatchItem& it : items) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = mh_batch_item{it.req, it.first, it.count, it.kind, it.pass, it.slot, it.slots};
        ++k;
    }
    return k;
}

int mh_search_first_batch(int dev, const mh_first_request* reqs, size_t n, mh_first_result* out) {
    g_err.clear();
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
#ifdef MH_DEV_HOOKS
    // as mh_search_first: the first-hit kernels have no variants of these hooks
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string("mh_search_first_batch does not support ") + hook);
#endif
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    batch_requests(reqs, n, &status, &valid);
    for (size_t i = 0; i < n; ++i) out[i] = mh_first_result{status[i], 0, 0, 0, 0};
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    mh::plan_batch(valid.data(), valid.size(), plan_opts(), slot_cap, &items);
    int passes = 0;
    for (const mh::BatchItem& it : items)
        if (it.kind == 0) passes = std::max(passes, it.pass + 1);
    if (passes) {
        const int rc = first_batch_run_fused(dev, valid.data(), reqs, items, passes, slot_cap, out);
        if (rc) return rc;
    }
    for (const mh::BatchItem& it : items) {  // the fallbacks, after the fused passes
        if (it.kind != 1) continue;
        const mh::BatchRequest& r = valid[it.idx];
        mh_first f;
        const int rc = search_first_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target, 0u, &f);
        if (rc) return rc;
        put_first_result(&out[r.id], f.hash, f.nonce, f.scanned, reqs[r.id].target);
    }
    return MH_OK;
}

// mh_search_first_batch_ex(MH_BATCH_FUSE_FAST) and, with stop, mh_search_first_batch_stop (`name`: the
// caller's, for messages): the same plan, passes and order; stop selects batch_stop<J, MODE> for the
// fast launches and mh_search_first_ex(MH_FIRST_STOP_RUNNING)'s path for the fallbacks.
static int first_batch_fused_impl(int dev, const mh_first_request* reqs, size_t n, bool stop, const char* name,
                           mh_first_result* out) {
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
#ifdef MH_DEV_HOOKS
    // as mh_search_first_batch: the first-hit kernels have no variants of these hooks
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string(name) + " does not support " + hook);
#else
    (void)name;
#endif
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    batch_requests(reqs, n, &status, &valid);
    for (size_t i = 0; i < n; ++i) out[i] = mh_first_result{status[i], 0, 0, 0, 0};
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(valid.data(), valid.size(), plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(),
                      &pieces, &args);
    int passes = 0;
    for (const mh::BatchPiece& p : pieces)
        if (p.kind != 1) passes = std::max(passes, p.pass + 1);
    if (passes) {
        const int rc = first_batch_run_fused_ex(dev, valid.data(), reqs, pieces, args, passes, slot_cap, stop, out);
        if (rc) return rc;
    }
    for (const mh::BatchPiece& p : pieces) {  // the fallbacks, after the fused passes
        if (p.kind != 1) continue;
        const mh::BatchRequest& r = valid[p.idx];
        mh_first f;
        const int rc = search_first_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target,
                                         stop ? (uint32_t)MH_FIRST_STOP_RUNNING : 0u, &f);
        if (rc) return rc;
        put_first_result(&out[r.id], f.hash, f.nonce, f.scanned, reqs[r.id].target);
    }
    return MH_OK;
}

int mh_search_first_batch_ex(int dev, const mh_first_request* reqs, size_t n, uint32_t flags, mh_first_result* out) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) return mh_search_first_batch(dev, reqs, n, out);
    return first_batch_fused_impl(dev, reqs, n, false, "mh_search_first_batch_ex", out);
}

int mh_search_first_batch_stop(int dev, const mh_first_request* reqs, size_t n, mh_first_result* out) {
    g_err.clear();
    return first_batch_fused_impl(dev, reqs, n, true, "mh_search_first_batch_stop", out);
}

int64_t mh_first_batch_order(const mh_request* reqs, size_t n, int32_t pass, uint32_t* out, int64_t cap) {
    g_err.clear();
    if (!reqs && n > 0) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    batch_requests(reqs, n, &status, &all);
    for (size_t i = 0; i < n; ++i)
        if (status[i])  // the first request mh_search would refuse, as mh_batch_plan
            return fail(status[i], status[i] == MH_ERANGE ? "lower > upper"
                                   : status[i] == MH_ETOOLONG ? "message longer than MH_MAX_MSG_LEN" : "msg is NULL");
    std::vector<mh::BatchItem> items;
    const uint32_t slot_cap = batch_slots();
    mh::plan_batch(all.data(), n, plan_opts(), slot_cap, &items);
    int passes = 0;
    for (const mh::BatchItem& it : items)
        if (it.kind == 0) passes = std::max(passes, it.pass + 1);
    if (pass < 0 || pass >= passes) return fail(MH_EINVAL, "no such pass");
    mh::BatchTables t;
    mh::build_batch_tables(all.data(), items, pass, &t);
    if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
    mh::FirstBatchTables ft;
    mh::build_first_batch_tables(t, first_batch_rank_major(), &ft);
    if (!mh::first_batch_tables_ok(t, ft)) return fail(MH_EINTERNAL, "internal: bad first-hit batch tables");
    int64_t k = 0;
    for (const uint32_t s : ft.order) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = s;
        ++k;
    }
    return k;
}

int64_t mh_first_batch_order_ex(const mh_request* reqs, size_t n, uint32_t flags, int32_t pass, int32_t launch,
                                uint32_t* out, int64_t cap) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) {
        if (launch != -1) return fail(MH_EINVAL, "no such launch");
        return mh_first_batch_order(reqs, n, pass, out, cap);
    }
    if (!reqs && n > 0) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    batch_requests(reqs, n, &status, &all);
    for (size_t i = 0; i < n; ++i)
        if (status[i])  // the first request mh_search would refuse, as mh_batch_plan
            return fail(status[i], status[i] == MH_ERANGE ? "lower > upper"
                                   : status[i] == MH_ETOOLONG ? "message longer than MH_MAX_MSG_LEN" : "msg is NULL");
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(all.data(), n, plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(), &pieces, &args);
    int passes = 0;
    for (const mh::BatchPiece& p : pieces)
        if (p.kind != 1) passes = std::max(passes, p.pass + 1);
    if (pass < 0 || pass >= passes) return fail(MH_EINVAL, "no such pass");
    mh::BatchTables t;
    mh::BatchFastTables f;
    mh::build_batch_tables_ex(all.data(), pieces, args, pass, &t, &f);
    if (launch < -1 || launch >= (int32_t)f.launches.size()) return fail(MH_EINVAL, "no such launch");
    mh::FirstBatchFastTables x;
    mh::build_first_batch_tables_ex(t, f, first_batch_rank_major(), &x);
    if (!mh::first_batch_tables_ex_ok(t, f, x, slot_cap)) return fail(MH_EINTERNAL, "internal: bad first-hit batch tables");
    const uint32_t* ord = launch < 0 ? x.tile_order.data() : x.chunk_order.data() + f.launches[(size_t)launch].chunk0;
    const size_t cnt = launch < 0 ? x.tile_order.size() : f.launches[(size_t)launch].chunks;
    int64_t k = 0;
    for (size_t b = 0; b < cnt; ++b) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = mh::first_batch_order_slot(t, f, launch, ord[b]);
        ++k;
    }
    return k;
}

int mh_search_hits_batch(int dev, const mh_hits_request* reqs, size_t n, mh_hit* hits, size_t hits_cap,
                         mh_hits_result* out) {
    g_err.clear();
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
#ifdef MH_DEV_HOOKS
    // as mh_search_hits: the hits kernels have no variants of these hooks
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string("mh_search_hits_batch does not support ") + hook);
#endif
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    std::vector<uint64_t> caps;
    hits_batch_requests(reqs, n, &status, &valid, &caps);
    uint64_t total = 0;  // the offsets: prefix sums of the caps, whatever the status; an out-of-range cap counts as 0
    for (size_t i = 0; i < n; ++i) {
        out[i] = mh_hits_result{status[i], 0, 0, 0, 0, 0, total};
        if (reqs[i].cap <= MH_HITS_MAX_CAP) total += reqs[i].cap;
        if (total > hits_cap) return fail(MH_EINVAL, "the caps add up to more than hits_cap");
    }
    if (!hits && total > 0) return fail(MH_EINVAL, "hits is NULL with a cap > 0");
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    mh::plan_batch(valid.data(), valid.size(), plan_opts(), slot_cap, &items);
    int passes = 0;
    for (const mh::BatchItem& it : items)
        if (it.kind == 0) passes = std::max(passes, it.pass + 1);
    std::vector<size_t> rebuild;  // fused requests whose region dropped entries
    if (passes) {
        const int rc = hits_batch_run_fused(dev, valid.data(), reqs, caps.data(), items, passes, slot_cap, hits, out,
                                            &rebuild);
        if (rc) return rc;
    }
    for (const size_t idx : rebuild) {  // the list again through the mh_search_hits path: count and minimum must agree
        const mh::BatchRequest& r = valid[idx];
        mh_hits_result& o = out[r.id];
        mh_hits h;
        const int rc = search_hits_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target, hits + o.offset,
                                        (size_t)reqs[r.id].cap, &h);
        if (rc) return rc;
        if (h.count != o.count || h.hash != o.hash || h.nonce != o.nonce || h.stored != o.stored)
            return fail(MH_EINTERNAL, "internal: a rebuilt hit list disagrees with the fused scan");
    }
    for (const mh::BatchItem& it : items) {  // the fallbacks, after the fused passes
        if (it.kind != 1) continue;
        const mh::BatchRequest& r = valid[it.idx];
        mh_hits_result& o = out[r.id];
        mh_hits h;
        const int rc = search_hits_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target,
                                        reqs[r.id].cap ? hits + o.offset : nullptr, (size_t)reqs[r.id].cap, &h);
        if (rc) return rc;
        o.count = h.count;
        o.stored = h.stored;
        o.hash = h.hash;
        o.nonce = h.nonce;
    }
    return MH_OK;
}

int64_t mh_hits_batch_regions(const mh_hits_request* reqs, size_t n, mh_hits_region* out, int64_t cap) {
    g_err.clear();
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    std::vector<uint64_t> caps;
    hits_batch_requests(reqs, n, &status, &all, &caps);
    for (size_t i = 0; i < n; ++i)
        if (status[i])  // the first request mh_search_hits_batch would refuse
            return fail(status[i], status[i] == MH_ERANGE     ? "lower > upper"
                                   : status[i] == MH_ETOOLONG ? "message longer than MH_MAX_MSG_LEN"
                                   : reqs[i].cap > MH_HITS_MAX_CAP ? "cap is larger than MH_HITS_MAX_CAP"
                                                                   : "msg is NULL");
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    mh::plan_batch(all.data(), n, plan_opts(), slot_cap, &items);
    int passes = 0;
    for (const mh::BatchItem& it : items)
        if (it.kind == 0) passes = std::max(passes, it.pass + 1);
    std::vector<mh_hits_region> regions(n);
    for (const mh::BatchItem& it : items)
        if (it.kind == 1) regions[it.idx] = mh_hits_region{it.req, 1, -1, -1, 0, 0, 0};
    const mh::HitsBatchLimits lim = hits_batch_limits();
    mh::HitsBatchState st;
    mh::BatchTables t;
    mh::HitsBatchTables ht;
    for (int p = 0; p < passes; ++p) {
        mh::build_batch_tables(all.data(), items, p, &t);
        if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
        const uint64_t before = st.used;
        const bool drain = mh::plan_hits_batch_pass(t, all.data(), caps.data(), lim, &st, &ht);
        if (!mh::hits_batch_tables_ok(t, all.data(), ht, drain ? 0u : before, lim.window_slots))
            return fail(MH_EINTERNAL, "internal: bad hits batch tables");
        for (size_t r = 0; r < t.req_idx.size(); ++r)
            regions[t.req_idx[r]] = mh_hits_region{all[t.req_idx[r]].id, 0, p, st.window, 0, ht.region[r].offset,
                                                   ht.region[r].slots};
    }
    int64_t k = 0;
    for (const mh_hits_region& g : regions) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = g;
        ++k;
    }
    return k;
}

int mh_search_hits_batch_ex(int dev, const mh_hits_request* reqs, size_t n, uint32_t flags, mh_hit* hits,
                            size_t hits_cap, mh_hits_result* out) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) return mh_search_hits_batch(dev, reqs, n, hits, hits_cap, out);
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
#ifdef MH_DEV_HOOKS
    // as mh_search_hits_batch: the hits kernels have no variants of these hooks
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string("mh_search_hits_batch_ex does not support ") + hook);
#endif
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    std::vector<uint64_t> caps;
    hits_batch_requests(reqs, n, &status, &valid, &caps);
    uint64_t total = 0;  // the offsets, as mh_search_hits_batch
    for (size_t i = 0; i < n; ++i) {
        out[i] = mh_hits_result{status[i], 0, 0, 0, 0, 0, total};
        if (reqs[i].cap <= MH_HITS_MAX_CAP) total += reqs[i].cap;
        if (total > hits_cap) return fail(MH_EINVAL, "the caps add up to more than hits_cap");
    }
    if (!hits && total > 0) return fail(MH_EINVAL, "hits is NULL with a cap > 0");
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(valid.data(), valid.size(), plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(),
                      &pieces, &args);
    int passes = 0;
    for (const mh::BatchPiece& p : pieces)
        if (p.kind != 1) passes = std::max(passes, p.pass + 1);
    std::vector<size_t> rebuild;  // fused requests whose region dropped entries
    if (passes) {
        const int rc = hits_batch_run_fused_ex(dev, valid.data(), reqs, caps.data(), pieces, args, passes, slot_cap, hits,
                                               out, &rebuild);
        if (rc) return rc;
    }
    // The lists again through the mh_search_hits path.  The fused scan has the exact count, so a
    // list cut by its cap (stored < count) is rebuilt from a prefix of the range: the `stored`
    // smallest qualifying nonces of [lower, hi] are those of the whole range once [lower, hi] holds
    // at least `stored` hits.  The prefix is sized from the observed density with a quarter to
    // spare and doubled while it holds too few; at hi == upper the count and minimum must agree.
    for (const size_t idx : rebuild) {
        const mh::BatchRequest& r = valid[idx];
        mh_hits_result& o = out[r.id];
        const double total = (double)(r.upper - r.lower) + 1.0;
        double want = o.stored < o.count ? 1.25 * total * (double)o.stored / (double)o.count + 1024.0 : total;
        for (;;) {
            const uint64_t span = want >= total ? r.upper - r.lower : (uint64_t)want;  // hi - lower
            const uint64_t hi = span >= r.upper - r.lower ? r.upper : r.lower + span;
            mh_hits h;
            const int rc = search_hits_impl(dev, r.pre, r.lower, hi, reqs[r.id].target, hits + o.offset,
                                            (size_t)reqs[r.id].cap, &h);
            if (rc) return rc;
            if (hi == r.upper) {
                if (h.count != o.count || h.hash != o.hash || h.nonce != o.nonce || h.stored != o.stored)
                    return fail(MH_EINTERNAL, "internal: a rebuilt hit list disagrees with the fused scan");
                break;
            }
            if (h.count > o.count) return fail(MH_EINTERNAL, "internal: a prefix holds more hits than the fused scan counted");
            if (h.stored == o.stored) break;  // stored == cap here: the prefix held at least cap hits
            want *= 2.0;
        }
    }
    for (const mh::BatchPiece& p : pieces) {  // the fallbacks, after the fused passes
        if (p.kind != 1) continue;
        const mh::BatchRequest& r = valid[p.idx];
        mh_hits_result& o = out[r.id];
        mh_hits h;
        const int rc = search_hits_impl(dev, r.pre, r.lower, r.upper, reqs[r.id].target,
                                        reqs[r.id].cap ? hits + o.offset : nullptr, (size_t)reqs[r.id].cap, &h);
        if (rc) return rc;
        o.count = h.count;
        o.stored = h.stored;
        o.hash = h.hash;
        o.nonce = h.nonce;
    }
    return MH_OK;
}

int64_t mh_hits_batch_regions_ex(const mh_hits_request* reqs, size_t n, uint32_t flags, mh_hits_region* out,
                                 int64_t cap) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (!(flags & MH_BATCH_FUSE_FAST)) return mh_hits_batch_regions(reqs, n, out, cap);
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    std::vector<uint64_t> caps;
    hits_batch_requests(reqs, n, &status, &all, &caps);
    for (size_t i = 0; i < n; ++i)
        if (status[i])  // the first request mh_search_hits_batch would refuse
            return fail(status[i], status[i] == MH_ERANGE     ? "lower > upper"
                                   : status[i] == MH_ETOOLONG ? "message longer than MH_MAX_MSG_LEN"
                                   : reqs[i].cap > MH_HITS_MAX_CAP ? "cap is larger than MH_HITS_MAX_CAP"
                                                                   : "msg is NULL");
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    mh::plan_batch_ex(all.data(), n, plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(), &pieces, &args);
    int passes = 0;
    for (const mh::BatchPiece& p : pieces)
        if (p.kind != 1) passes = std::max(passes, p.pass + 1);
    std::vector<mh_hits_region> regions(n);
    for (const mh::BatchPiece& p : pieces)
        if (p.kind == 1) regions[p.idx] = mh_hits_region{p.req, 1, -1, -1, 0, 0, 0};
    const mh::HitsBatchLimits lim = hits_batch_limits();
    mh::HitsBatchState st;
    mh::BatchTables t;
    mh::BatchFastTables f;
    mh::HitsBatchFastTables x;
    for (int p = 0; p < passes; ++p) {
        mh::build_batch_tables_ex(all.data(), pieces, args, p, &t, &f);
        const uint64_t before = st.used;
        bool drain;
        if (f.items.empty()) {  // mh_search_hits_batch's own pass
            if (!mh::batch_tables_ok(t, slot_cap)) return fail(MH_EINTERNAL, "internal: bad batch tables");
            drain = mh::plan_hits_batch_pass(t, all.data(), caps.data(), lim, &st, &x.h);
            if (!mh::hits_batch_tables_ok(t, all.data(), x.h, drain ? 0u : before, lim.window_slots))
                return fail(MH_EINTERNAL, "internal: bad hits batch tables");
        } else {
            drain = mh::plan_hits_batch_pass_ex(t, f, all.data(), caps.data(), lim, &st, &x);
            if (!mh::hits_batch_tables_ex_ok(t, f, all.data(), x, slot_cap, drain ? 0u : before, lim.window_slots))
                return fail(MH_EINTERNAL, "internal: bad hits batch tables");
        }
        for (size_t r = 0; r < t.req_idx.size(); ++r)
            regions[t.req_idx[r]] = mh_hits_region{all[t.req_idx[r]].id, 0, p, st.window, 0, x.h.region[r].offset,
                                                   x.h.region[r].slots};
    }
    int64_t k = 0;
    for (const mh_hits_region& g : regions) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = g;
        ++k;
    }
    return k;
}

int mh_search_first_hits_batch(int dev, const mh_first_hits_request* reqs, size_t n, uint32_t flags, mh_hit* hits,
                               size_t hits_cap, mh_first_hits_result* out) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (n == 0) return MH_OK;
    if (!reqs || !out) return fail(MH_EINVAL, "NULL array");
#ifdef MH_DEV_HOOKS
    // as mh_search_first_hits: the stopping hits kernels have no variants of these hooks
    for (const char* hook : {"MINEHIP_DEV_HASH_KEEP", "MINEHIP_DEV_HASH_XOR", "MINEHIP_DEV_CODE_OBJECT"})
        if (const char* e = getenv(hook))
            if (*e) return fail(MH_EINVAL, std::string("mh_search_first_hits_batch does not support ") + hook);
#endif
    std::vector<int> status;
    std::vector<mh::BatchRequest> valid;
    std::vector<uint64_t> targets, ks, wants;
    first_hits_batch_requests(reqs, n, &status, &valid, &targets, &ks, &wants);
    uint64_t total = 0;  // the offsets: prefix sums of k, whatever the status; a k out of range counts as 0
    for (size_t i = 0; i < n; ++i) {
        out[i] = mh_first_hits_result{status[i], 0, 0, 0, 0, 0, total};
        if (reqs[i].k <= MH_HITS_MAX_CAP) total += reqs[i].k;
        if (total > hits_cap) return fail(MH_EINVAL, "the k add up to more than hits_cap");
    }
    if (!hits && total > 0) return fail(MH_EINVAL, "hits is NULL with a k > 0");
    if (valid.empty()) return MH_OK;
    g_err.clear();
    const uint32_t slot_cap = batch_slots();
    std::vector<mh::BatchItem> items;
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    std::vector<size_t> fallback;  // positions in `valid`
    int passes = 0;
    if (flags & MH_BATCH_FUSE_FAST) {
        mh::plan_batch_ex(valid.data(), valid.size(), plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(),
                          &pieces, &args);
        for (const mh::BatchPiece& p : pieces)
            if (p.kind != 1)
                passes = std::max(passes, p.pass + 1);
            else
                fallback.push_back(p.idx);
    } else {
        mh::plan_batch(valid.data(), valid.size(), plan_opts(), slot_cap, &items);
        for (const mh::BatchItem& it : items)
            if (it.kind == 0)
                passes = std::max(passes, it.pass + 1);
            else
                fallback.push_back(it.idx);
    }
    std::vector<size_t> rebuild;  // fused requests whose region dropped entries
    if (passes) {
        FirstHitsBatchCall call{valid.data(), reqs, targets.data(), ks.data(), wants.data(), hits, out, &rebuild, {}};
        const int rc = first_hits_batch_run_fused(dev, &call, (flags & MH_BATCH_FUSE_FAST) ? nullptr : &items, &pieces, &args,
                                                  passes, slot_cap);
        if (rc) return rc;
    }
    // the rebuilt requests and the fallbacks through the mh_search_first_hits path, after the fused passes
    for (int which = 0; which < 2; ++which)
        for (const size_t idx : which ? fallback : rebuild) {
            const mh::BatchRequest& r = valid[idx];
            mh_first_hits_result& o = out[r.id];
            mh_first_hits h;
            const int rc = search_first_hits_impl(dev, r.pre, r.lower, r.upper, targets[idx], hits + o.offset, (size_t)ks[idx], &h,
                                                  true);
            if (rc) return rc;
            o.stored = h.stored;
            o.scanned = h.scanned;
            o.hash = h.hash;
            o.nonce = h.nonce;
            o.path = which ? 1 : 2;
        }
    return MH_OK;
}

int64_t mh_first_hits_batch_regions(const mh_first_hits_request* reqs, size_t n, uint32_t flags, mh_hits_region* out,
                                    int64_t cap) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (n == 0) return 0;
    if (!reqs) return fail(MH_EINVAL, "NULL array");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    std::vector<int> status;
    std::vector<mh::BatchRequest> all;
    std::vector<uint64_t> targets, ks, wants;
    first_hits_batch_requests(reqs, n, &status, &all, &targets, &ks, &wants);
    for (size_t i = 0; i < n; ++i)
        if (status[i])  // the first request mh_search_first_hits_batch would refuse
            return fail(status[i], status[i] == MH_ERANGE      ? "lower > upper"
                                   : status[i] == MH_ETOOLONG  ? "message longer than MH_MAX_MSG_LEN"
                                   : reqs[i].k == 0            ? "k is 0"
                                   : reqs[i].k > MH_HITS_MAX_CAP ? "k is larger than MH_HITS_MAX_CAP"
                                                               : "msg is NULL");
    const uint32_t slot_cap = batch_slots();
    const bool fast = (flags & MH_BATCH_FUSE_FAST) != 0;
    std::vector<mh::BatchItem> items;
    std::vector<mh::BatchPiece> pieces;
    std::vector<mh::FastArgs> args;
    std::vector<mh_hits_region> regions(n);
    int passes = 0;
    if (fast) {
        mh::plan_batch_ex(all.data(), n, plan_opts(), slot_cap, batch_fast_shared_lanes(), batch_fast_max(), &pieces, &args);
        for (const mh::BatchPiece& p : pieces)
            if (p.kind != 1)
                passes = std::max(passes, p.pass + 1);
            else
                regions[p.idx] = mh_hits_region{p.req, 1, -1, -1, 0, 0, 0};
    } else {
        mh::plan_batch(all.data(), n, plan_opts(), slot_cap, &items);
        for (const mh::BatchItem& it : items)
            if (it.kind == 0)
                passes = std::max(passes, it.pass + 1);
            else
                regions[it.idx] = mh_hits_region{it.req, 1, -1, -1, 0, 0, 0};
    }
    const mh::HitsBatchLimits lim = first_hits_batch_limits();
    const bool rank_major = first_batch_rank_major();
    mh::HitsBatchState st;
    mh::BatchTables t;
    mh::BatchFastTables f;
    mh::FirstHitsBatchTables x;
    for (int p = 0; p < passes; ++p) {
        if (fast)
            mh::build_batch_tables_ex(all.data(), pieces, args, p, &t, &f);
        else
            mh::build_batch_tables(all.data(), items, p, &t);
        const uint64_t before = st.used;
        const bool drain = mh::plan_first_hits_batch_pass(t, f, all.data(), wants.data(), lim, rank_major, &st, &x);
        if (!mh::first_hits_batch_tables_ok(t, f, all.data(), x, slot_cap, drain ? 0u : before, lim.window_slots))
            return fail(MH_EINTERNAL, "internal: bad first-hits batch tables");
        for (size_t r = 0; r < t.req_idx.size(); ++r)
            regions[t.req_idx[r]] = mh_hits_region{all[t.req_idx[r]].id, 0, p, st.window, 0, x.region[r].offset,
                                                   x.region[r].slots};
    }
    int64_t k = 0;
    for (const mh_hits_region& g : regions) {
        if (k >= cap) return cap + 1;  // cap + 1 signals truncation
        if (out) out[k] = g;
        ++k;
    }
    return k;
}

int mh_miner_handle_batch(const int* devs, int ndev, const char* const* requests, const size_t* lens, size_t n,
                          char* out, size_t cap_each, size_t* out_lens, int* status) {
    return mh_miner_handle_batch_ex(devs, ndev, requests, lens, n, 0, out, cap_each, out_lens, status);
}

int mh_miner_handle_batch_ex(const int* devs, int ndev, const char* const* requests, const size_t* lens, size_t n,
                             uint32_t flags, char* out, size_t cap_each, size_t* out_lens, int* status) {
    g_err.clear();
    if (flags & ~(uint32_t)MH_BATCH_FUSE_FAST) return fail(MH_EINVAL, "unknown flag");
    if (n == 0) return MH_OK;
    if (!devs || ndev <= 0 || !requests || !lens || !status) return fail(MH_EINVAL, "bad arguments");
    std::vector<mh::Msg> msgs(n);
    std::vector<mh_request> reqs;
    std::vector<size_t> where;  // reqs[k] is payload where[k]
    for (size_t i = 0; i < n; ++i) {
        if (out_lens) out_lens[i] = 0;
        mh::Msg& m = msgs[i];
        if (!requests[i]) {
            status[i] = fail(MH_EINVAL, "bad arguments");
        } else if (!mh::decode(requests[i], lens[i], &m)) {
            status[i] = fail(MH_ENOTREQ, "payload is not a JSON bitcoin.Message");
        } else if (m.type != 1) {
            status[i] = fail(MH_ENOTREQ, "not a Request");  // message.go:10
        } else if (m.lower > m.upper) {
            status[i] = fail(MH_ERANGE, "lower > upper");
        } else {
            status[i] = MH_OK;
            reqs.push_back(mh_request{(const uint8_t*)m.data.data(), m.data.size(), m.lower, m.upper});
            where.push_back(i);
        }
    }
    if (reqs.empty()) return MH_OK;
    std::vector<mh_result> res(reqs.size());
    // fallbacks as mh_miner_handle searches: one device through mh_search's path, several through
    // mh_search_multi's adaptive split
    const BatchFallback fallback = [&](const mh::BatchRequest& r, uint64_t* h, uint64_t* nn) {
        if (ndev == 1) return search_impl(devs[0], r.pre, r.lower, r.upper, h, nn);
        const mh_request& q = reqs[r.id];
        return mh_search_multi(devs, ndev, q.msg, q.len, q.lower, q.upper, 0, h, nn);
    };
    const int rc = (flags & MH_BATCH_FUSE_FAST)
                       ? search_batch_ex_impl(devs[0], reqs.data(), reqs.size(), res.data(), fallback)
                       : search_batch_impl(devs[0], reqs.data(), reqs.size(), res.data(), fallback);
    if (rc) return rc;
    for (size_t k = 0; k < reqs.size(); ++k) {
        const size_t i = where[k];
        status[i] = res[k].status;
        if (res[k].status) continue;
        const std::string s = mh::encode(2, nullptr, 0, 0, 0, res[k].hash, res[k].nonce);  // NewResult (message.go:38-44)
        if (out_lens) out_lens[i] = s.size();
        if (!out || cap_each < s.size()) {
            status[i] = fail(MH_EINVAL, "output buffer too small");
            continue;
        }
        memcpy(out + i * cap_each, s.data(), s.size());
    }
    return MH_OK;
}

int mh_hash_batch(int dev, const uint8_t* msg, size_t len, const uint64_t* nonces, size_t n, uint64_t* out_hashes) {
    g_err.clear();
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (n == 0) return MH_OK;
    if (!nonces || !out_hashes) return fail(MH_EINVAL, "NULL buffer");
    DevCtx* c;
    rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipSetDevice(dev));
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    mh::GenArgs ga;
    mh::make_gen_args(pre, &ga);
    for (size_t off = 0; off < n; off += kBatchChunk) {
        const size_t m = (n - off < kBatchChunk) ? n - off : kBatchChunk;
        MH_HIP(hipMemcpyAsync(c->d_nonces, nonces + off, m * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        MH_HIP(mh::launch_hash_batch(ga, c->d_nonces, c->d_hashes, m, c->stream));
        MH_HIP(hipMemcpyAsync(out_hashes + off, c->d_hashes, m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        MH_HIP(hipStreamSynchronize(c->stream));
    }
    return MH_OK;
}

int mh_profile_enable(int dev, int on) {
    g_err.clear();
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    rc = init_locked(c, dev);
    if (rc) return rc;
    MH_HIP(hipStreamSynchronize(c->stream));
    rc = harvest_locked(c);  // timings of launches already recorded stay counted
    if (rc) return rc;
    if (on) {  // enabling starts a fresh count; disabling keeps the counts readable
        memset(c->cnt, 0, sizeof c->cnt);
        for (auto& v : c->var) v = VarStat();
    }
    c->prof = on != 0;
    return MH_OK;
}

int mh_profile_read(int dev, uint64_t* out, int n) {
    g_err.clear();
    if (!out || n < 0) return fail(MH_EINVAL, "bad arguments");
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->ready) {
        MH_HIP(hipStreamSynchronize(c->stream));
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    for (int i = 0; i < n && i < 8; ++i) out[i] = c->cnt[i];
    return MH_OK;
}

int mh_profile_kernels(int dev, mh_kernel_stat* out, int cap) {
    g_err.clear();
    if (cap < 0 || (!out && cap > 0)) return fail(MH_EINVAL, "bad arguments");
    DevCtx* c;
    int rc = get_ctx(dev, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->ready) {
        MH_HIP(hipStreamSynchronize(c->stream));
        rc = harvest_locked(c);
        if (rc) return rc;
    }
    int n = 0;
    for (int i = 0; i < kVariants; ++i) {
        const VarStat& v = c->var[i];
        // (a fused batch launch of mixed lane lengths counts under its first piece's L, the
        // other pieces' nonces under theirs, with no launch of their own)
        if (!v.launches && !v.nonces) continue;
        if (n < cap) {
            out[n].word = i % 16;
            out[n].mode = (i / 16) % mh::kModes;
            out[n].lo_digits = i / (16 * mh::kModes) + 1;
            out[n].reserved = 0;
            out[n].launches = v.launches;
            out[n].nonces = v.nonces;
            out[n].ns = v.ns;
            out[n].ops = v.ops;
            out[n].slots = v.slots;
        }
        ++n;
    }
    return n;
}

int64_t mh_plan(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, mh_piece* out, int64_t cap) {
    g_err.clear();
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    if (cap < 0) return fail(MH_EINVAL, "cap < 0");
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    int64_t k = 0;
    const mh::PlanOpts opt = plan_opts();
    mh::plan_search(pre, lower, upper, opt, [&](const mh::Piece& p) {
        if (k >= cap) {
            ++k;  // cap + 1 signals truncation
            return false;
        }
        if (out) {
            mh_piece& q = out[k];
            q.first = p.first;
            q.count = p.count;
            q.kind = p.kind;
            q.digits = p.digits;
            q.lo_digits = p.L;
            q.word = p.J;
            q.mode = p.mode;
            q.blocks = p.blocks;
            q.nonce_ops = p.ops;
            q.nonce_slots = p.slots;
        }
        ++k;
        return true;
    });
    return k;
}

int64_t mh_multi_plan(const uint8_t* msg, size_t len, uint64_t lower, uint64_t upper, const double* weights,
                      int ndev, mh_span* out, int64_t cap) {
    g_err.clear();
    int rc = check_common(msg, len);
    if (rc) return rc;
    if (lower > upper) return fail(MH_ERANGE, "lower > upper");
    if (ndev <= 0 || ndev > MH_MAX_WORKERS || cap < 0) return fail(MH_EINVAL, "bad arguments");
    std::vector<double> w((size_t)ndev, 1.0);
    if (weights)
        for (int i = 0; i < ndev; ++i) {
            if (!(weights[i] > 0.0) || !std::isfinite(weights[i])) return fail(MH_EINVAL, "weights must be finite and > 0");
            w[(size_t)i] = weights[i];
        }
    mh::Prefix pre;
    mh::absorb_prefix(msg, len, &pre);
    mh::MultiPlan mp;
    mh::multi_plan(pre, lower, upper, plan_opts(), w, &mp);
    int64_t k = 0;
    auto put = [&](const mh::Span& s, int worker, int kind) {
        if (k < cap && out) {
            out[k].lower = s.lo;
            out[k].upper = s.hi;
            out[k].worker = worker;
            out[k].kind = kind;
            out[k].cost = mh::segments_cost(mp.segs, s.lo, s.hi);
        }
        ++k;
    };
    for (int i = 0; i < ndev; ++i)
        if (!mp.head[(size_t)i].empty) put(mp.head[(size_t)i], i, 0);
    for (const auto& s : mp.tail) put(s, -1, 1);
    return k;
}

int mh_multi_rates(const int* devs, int ndev, double* out) {
    g_err.clear();
    if (ndev < 0 || (ndev > 0 && (!devs || !out))) return fail(MH_EINVAL, "bad arguments");
    for (int i = 0; i < ndev; ++i) out[i] = mh::device_rate(devs[i]);
    return MH_OK;
}

}  // extern "C"
