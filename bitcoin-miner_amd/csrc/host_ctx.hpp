// host_ctx.hpp -- what the host code of libminehip.so shares between its translation units
// (minehip.cpp: the device context, the single searches and the rest of the C-ABI; batch.cpp: the
// batched entry points): the kernels' launchers, the per-device context, the error and profile
// plumbing and the single searches the batch fallbacks run.  Private: nothing of mh::host is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/minehip.h"
#include "layout.hpp"
#include "plan.hpp"

// the launchers (search_kernels.hip)
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

namespace mh {
namespace host __attribute__((visibility("hidden"))) {

// mh_last_error's text, of the calling thread (defined in minehip.cpp); fail sets it and returns `code`
extern thread_local std::string g_err;
int fail(int code, const std::string& what);

#define MH_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return fail(MH_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// the same for a call that returns an MH_* code (and has described its failure)
#define MH_TRY(call)              \
    do {                          \
        const int rc_ = (call);   \
        if (rc_) return rc_;      \
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

// minehip.cpp (each described at its definition)
int get_ctx(int dev, DevCtx** out);
int init_locked(DevCtx* c, int dev);
int harvest_locked(DevCtx* c);
#ifdef MH_DEV_HOOKS
int read_hash_keep(DevCtx* c);
int read_hash_xor(DevCtx* c);
#endif
bool early_piece_ok(const mh::FastArgs& a, int word);
mh::PlanOpts plan_opts();
uint64_t hits_slots();
int check_common(const uint8_t* msg, size_t len);
int refuse_hash_hooks(const char* name);
// the single searches, which the batch fallbacks and rebuilds run
int search_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t* oh, uint64_t* on,
                uint64_t* busy_ns = nullptr);
int search_first_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, uint32_t flags,
                      mh_first* out);
int search_hits_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, mh_hit* hits,
                     size_t cap, mh_hits* out);
int search_first_hits_impl(int dev, const mh::Prefix& pre, uint64_t lower, uint64_t upper, uint64_t target, mh_hit* hits,
                           size_t k, mh_first_hits* out, bool widen_walk = false);

}  // namespace host
}  // namespace mh
