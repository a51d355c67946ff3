// search_kernels.hip -- gfx950 kernels of libminehip (fat binary) and the
// launchers of every kernel, including the embedded fast_search module.
//
// Hot path replaced: the miner's scan over bitcoin.Hash (reference
// bitcoin/hash.go:13-17, scan spec SURVEY.md §8(a) A2 / stub
// bitcoin/miner/miner.go:33).  Design: DESIGN.md §3.
//
//   fast_search<J, MODE>  (fast_search.hip) the run kernel; it reaches the
//                         library as a code object built through the
//                         issue-priority pass and is launched from here by
//                         name (fast_module below).
//   generic_scan          one lane = one nonce, any layout (range edges,
//                         buckets too small for runs).
//   hash_batch            out[i] = Hash(msg, nonces[i]) (GPU bitcoin.Hash).
//   merge_partials        folds per-workgroup (hash, nonce) candidates into
//                         the search's running minimum (one 1024-thread
//                         workgroup).
//   batch_scan            many small Requests in one launch: one workgroup per
//                         2,560-nonce tile of a table of entries, one lane = aligned
//                         decades of ten nonces formatted once (mh_search_batch).
//   merge_segments        one workgroup per request of a batch pass folds that
//                         request's slot segment into its result.
//   first_scan<J, MODE>   (fast_search.hip, -DMH_FIRST) fast_search for mh_search_first: the
//                         smallest nonce whose hash is <= a target, later chunks skipped; a
//                         second embedded code object, loaded by the first such search.
//   stop_scan<J, MODE>    (fast_search.hip, -DMH_FIRST -DMH_STOP) first_scan whose waves publish a hit
//                         when found and leave a running chunk that lies wholly above a published
//                         hit, for mh_search_first_ex(MH_FIRST_STOP_RUNNING); a seventh embedded
//                         code object, loaded by the first such search.
//   generic_scan_first    generic_scan for mh_search_first.
//   finish_first          one thread: the winning key back into its hash, the result out.
//   hits_scan<J, MODE>    (fast_search.hip, -DMH_HITS) fast_search for mh_search_hits: every nonce
//                         whose hash is <= a target appended to a device buffer; a third embedded
//                         code object, loaded by the first such search.
//   generic_scan_hits     generic_scan for mh_search_hits.
//   hits_stop<J, MODE>    (fast_search.hip, -DMH_HITS -DMH_STOP) hits_scan for mh_search_first_hits:
//                         its hits count in slices of the range, its waves publish a bound once the
//                         slices hold k hits and leave a running chunk that lies above it.
//   generic_scan_hits_stop  generic_scan_hits for mh_search_first_hits: skipped above the bound.
//   batch_scan_first      batch_scan for mh_search_first_batch: first-hit keys, per-request device
//                         words, tiles dispatched in the host's rank-major order.
//   merge_segments_first  merge_segments, then the winning key back into its hash and the
//                         request's {hash, nonce, scanned} out.
//   batch_scan_hits       batch_scan for mh_search_hits_batch: the same minimum, and every nonce
//                         whose hash is <= its request's target appended to the request's region
//                         of the device hit buffer through a per-request cursor.
//   merge_segments_hits   merge_segments, and the request's {hash, nonce, count} out.
//   batch_fast<J, MODE>   (fast_search.hip, -DMH_BATCH) the fast pieces of many requests in one
//                         launch, one workgroup per 256-run chunk of a table of items; a fourth
//                         embedded code object, loaded by the first mh_search_batch_ex that fuses one.
//   batch_scan_slots      batch_scan writing partials[slot0 + tile - tile0]: the generic entries of
//                         a pass whose slot segments also hold fast chunks.
//   batch_first<J, MODE>  (fast_search.hip, -DMH_BATCH -DMH_FIRST) batch_fast's table and grid around
//                         the first-hit chunk body, chunks dispatched in the host's order and skipped
//                         above their request's hit; a fifth embedded code object, loaded by the first
//                         mh_search_first_batch_ex that fuses one.
//   batch_stop<J, MODE>   (fast_search.hip, -DMH_BATCH -DMH_FIRST -DMH_STOP) batch_first whose waves publish
//                         a hit when found and leave a running chunk that lies wholly above their
//                         request's published hit; an eighth embedded code object, loaded by the first
//                         mh_search_first_batch_stop.
//   batch_scan_first_slots  batch_scan_first writing partials[slot0 + tile - tile0], as
//                         batch_scan_slots relates to batch_scan.
//   merge_segments_first_ex  merge_segments_first with the message state per request, not per tile:
//                         a fused request may hold no generic entry.
//
//   batch_hits<J, MODE>   (fast_search.hip, -DMH_BATCH -DMH_HITS) batch_fast's table and grid around
//                         the hits chunk body, appending through the request's cursor into its
//                         region; a sixth embedded code object, loaded by the first
//                         mh_search_hits_batch_ex that fuses one.
//   batch_scan_hits_slots  batch_scan_hits writing partials[slot0 + tile - tile0], as
//                         batch_scan_slots relates to batch_scan.  merge_segments_hits serves such
//                         passes unchanged: it reads the segments and the words, not the entries.
//   batch_scan_bound      batch_scan_hits for mh_search_first_hits_batch: tiles in batch_scan_first's
//                         order, skipped above their request's bound; the hits count in the request's
//                         slices and the wave that reaches k publishes the bound.
//   batch_scan_bound_slots  batch_scan_bound writing partials[slot0 + tile - tile0].
//   batch_bound<J, MODE>  (fast_search.hip, -DMH_BATCH -DMH_HITS -DMH_STOP) batch_first's table, order and
//                         grid around hits_stop's chunk body, through the request's words; a tenth
//                         embedded code object, loaded by the first mh_search_first_hits_batch that
//                         fuses a fast piece.
//   merge_segments_bound  merge_segments_hits, and the request's {hash, nonce, count, scanned} out.
//
// Every candidate comparison is the lexicographic (hash, nonce) order, which
// equals the reference loop's strict-< first minimum.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "kernel_common.hpp"
#include "layout.hpp"
#include "sha256_gfx950.hpp"

// fast_search.hip's code object after the issue-priority pass (fast_co.S)
extern "C" const unsigned char mh_fast_co_begin[];
// the same source built with -DMH_FIRST: first_scan<J, MODE>, the fast kernels of mh_search_first
extern "C" const unsigned char mh_first_co_begin[];
// the same source built with -DMH_HITS: hits_scan<J, MODE>, the fast kernels of mh_search_hits
extern "C" const unsigned char mh_hits_co_begin[];
// the same source built with -DMH_BATCH: batch_fast<J, MODE>, the fused fast pieces of mh_search_batch_ex
extern "C" const unsigned char mh_batch_co_begin[];
// the same source built with -DMH_BATCH -DMH_FIRST: batch_first<J, MODE>, the fused fast pieces of mh_search_first_batch_ex
extern "C" const unsigned char mh_batch_first_co_begin[];
// the same source built with -DMH_FIRST -DMH_STOP: stop_scan<J, MODE>, the fast kernels of mh_search_first_ex(MH_FIRST_STOP_RUNNING)
extern "C" const unsigned char mh_first_stop_co_begin[];
// the same source built with -DMH_BATCH -DMH_FIRST -DMH_STOP: batch_stop<J, MODE>, the fused fast pieces of mh_search_first_batch_stop
extern "C" const unsigned char mh_batch_first_stop_co_begin[];
// the same source built with -DMH_BATCH -DMH_HITS: batch_hits<J, MODE>, the fused fast pieces of mh_search_hits_batch_ex
extern "C" const unsigned char mh_batch_hits_co_begin[];
// the same source built with -DMH_HITS -DMH_STOP: hits_stop<J, MODE>, the fast kernels of mh_search_first_hits
extern "C" const unsigned char mh_hits_stop_co_begin[];
// the same source built with -DMH_BATCH -DMH_HITS -DMH_STOP: batch_bound<J, MODE>, the fused fast pieces of mh_search_first_hits_batch
extern "C" const unsigned char mh_batch_bound_co_begin[];

namespace mh {
#ifdef MH_DEV_HOOKS
// Hash-XOR test hook (MINEHIP_DEV_HASH_XOR, layout.hpp): {high, low} 32 bits of the constant the
// scan kernels of this library XOR every nonce's (H0, H1) with before the keep mask; zero (off)
// unless set_hash_xor below writes it before a search.
__device__ uint32_t mh_dev_hash_xor[2];
#endif
namespace dev {

// Generic Hash(msg, n): formats n in registers and hashes the 1 or 2 tail
// blocks from the host midstate.  Handles any digit count per lane.
__device__ __forceinline__ void hash_generic(const GenArgs& a, uint64_t n, uint32_t& h0, uint32_t& h1) {
    constexpr uint64_t P10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull,
                                  100000000ull, 1000000000ull, 10000000000ull, 100000000000ull,
                                  1000000000000ull, 10000000000000ull, 100000000000000ull,
                                  1000000000000000ull, 10000000000000000ull, 100000000000000000ull,
                                  1000000000000000000ull, 10000000000000000000ull};
    uint32_t nd = 1;  // Go %d: no leading zeros, "0" for 0
#pragma unroll
    for (int k = 1; k < 20; ++k) nd += (n >= P10[k]) ? 1u : 0u;
    uint32_t w[32];
#pragma unroll
    for (int x = 0; x < 16; ++x) w[x] = a.tail[x];
#pragma unroll
    for (int x = 16; x < 32; ++x) w[x] = 0u;
    uint64_t u = n;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        if ((uint32_t)k < nd) {
            const uint64_t q = u / 10u;
            const uint32_t dg = (uint32_t)(u - q * 10u);
            u = q;
            const uint32_t pos = a.t + nd - 1u - (uint32_t)k;
            add_word(w, pos >> 2, (0x30u + dg) << (24u - 8u * (pos & 3u)));
        }
    }
    const uint32_t end = a.t + nd;  // tail length; the 0x80 byte goes here
    add_word(w, end >> 2, 0x80u << (24u - 8u * (end & 3u)));
    const uint64_t bits = (a.plen + nd) * 8u;
    const bool two = end + 9u > 64u;
    const uint32_t bhi = (uint32_t)(bits >> 32), blo = (uint32_t)bits;
    w[14] = two ? w[14] : bhi;
    w[15] = two ? w[15] : blo;
    w[30] = two ? bhi : 0u;
    w[31] = two ? blo : 0u;
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = a.mid[i];
    if (!two) {
        sha256_block_h01(st, w, h0, h1);
    } else {
        sha256_block(st, w);
        sha256_block_h01(st, w + 16, h0, h1);
    }
}

}  // namespace dev

__global__ __launch_bounds__(kBlockThreads) void generic_scan(const GenArgs a, Partial* __restrict__ partials) {
    using namespace dev;
    const uint32_t gid = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint64_t n = a.first + gid;
    uint32_t h0, h1;
    hash_generic(a, n, h0, h1);
#ifdef MH_DEV_HOOKS  // hash-XOR, then coarse-hash test hook (layout.hpp keep_word): a.pad = 0, all bits, unless set
    h0 = (h0 ^ mh_dev_hash_xor[0]) & keep_mask0(a.pad);
    h1 = (h1 ^ mh_dev_hash_xor[1]) & keep_mask1(a.pad);
#endif
    uint64_t hash = ((uint64_t)h0 << 32) | h1, nonce = n;
    if (gid >= a.count) {
        hash = ~0ull;
        nonce = ~0ull;
    }
    block_min(hash, nonce);
    if (threadIdx.x == 0) partials[blockIdx.x] = Partial{hash, nonce};
}

// generic_scan for mh_search_first: a nonce's key is 0 if its hash is <= f.target,
// else the hash.  The workgroup is skipped when its first nonce -- its smallest -- is larger than
// *f.first, the smallest qualifying nonce reported so far (the skip rule of first_scan,
// fast_search.hip); it then writes the sentinel the merge reads.  No test hooks: mh_search_first
// refuses them.
__global__ __launch_bounds__(kBlockThreads) void generic_scan_first(const GenArgs a, Partial* __restrict__ partials,
                                                                    const FirstArgs f) {
    using namespace dev;
    __shared__ uint32_t s_skip;
    const uint64_t base = a.first + (uint64_t)blockIdx.x * kBlockThreads;  // a valid nonce: blocks = ceil(count / 256)
    if (threadIdx.x == 0)
        s_skip = base > __hip_atomic_load(f.first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
    __syncthreads();
    if (s_skip) {  // one value per workgroup
        if (threadIdx.x == 0) partials[blockIdx.x] = Partial{~0ull, ~0ull};
        return;
    }
    const uint64_t n = base + threadIdx.x;
    uint32_t h0, h1;
    hash_generic(a, n, h0, h1);
    uint64_t hash = ((uint64_t)h0 << 32) | h1, nonce = n;
    if (hash <= f.target) hash = 0ull;
    const uint64_t left = a.count - (uint64_t)blockIdx.x * kBlockThreads;  // >= 1
    if (threadIdx.x >= left) {
        hash = ~0ull;
        nonce = ~0ull;
    }
    block_min(hash, nonce);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = Partial{hash, nonce};
        if (hash == 0ull) atomicMin(f.first, (unsigned long long)nonce);
        atomicAdd(f.scanned, (unsigned long long)(left < (uint64_t)kBlockThreads ? left : (uint64_t)kBlockThreads));
    }
}

// generic_scan for mh_search_hits: the same minimum, and every thread below a.count
// whose hash is <= h.target appends {hash, nonce} to the hit buffer.  Per wave, the lowest hit lane
// takes one slot per hit from the cursor with one atomic add and hit number r of the wave (in lane
// order) goes to base + r if that lies below the capacity; the cursor advances either way, so it
// ends as the exact count.  No test hooks: mh_search_hits refuses them.
__global__ __launch_bounds__(kBlockThreads) void generic_scan_hits(const GenArgs a, Partial* __restrict__ partials,
                                                                   const HitsArgs h) {
    using namespace dev;
    const uint32_t gid = blockIdx.x * kBlockThreads + threadIdx.x;
    const uint64_t n = a.first + gid;
    uint32_t h0, h1;
    hash_generic(a, n, h0, h1);
    uint64_t hash = ((uint64_t)h0 << 32) | h1, nonce = n;
    const bool hit = gid < a.count && hash <= h.target;
    const uint64_t hm = __builtin_amdgcn_ballot_w64(hit);
    if (hm) {  // one value per wave
        const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const uint32_t lead = (uint32_t)__builtin_ctzll(hm);
        unsigned long long taken = 0ull;
        if (lane == lead) taken = atomicAdd(h.cursor, (unsigned long long)__builtin_popcountll(hm));
        const uint64_t base =
            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(taken >> 32), (int)lead) << 32) |
            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)taken, (int)lead);
        const uint64_t slot = base + (uint32_t)__builtin_popcountll(hm & ((1ull << lane) - 1ull));
        if (hit && slot < h.cap) h.hits[slot] = Hit{hash, nonce};
    }
    if (gid >= a.count) {
        hash = ~0ull;
        nonce = ~0ull;
    }
    block_min(hash, nonce);
    if (threadIdx.x == 0) partials[blockIdx.x] = Partial{hash, nonce};
}

// generic_scan_hits for mh_search_first_hits (layout.hpp HitsStopArgs): the workgroup
// is skipped when its first nonce -- its smallest -- lies above the search's bound word (at least k
// hits of the range are <= the word's value, so none of the tile's nonces is among the k smallest
// hits); it then writes the sentinel the merge reads and counts nothing.  Otherwise every hit first
// counts in its slice of the range, lane-parallel, and the counts are back before the wave's lead
// lane advances the cursor -- whoever gets a cursor value back finds every hit it stands for in the
// slices -- and the wave whose cursor value plus its own hits reaches k publishes the bound
// (kernel_common.hpp publish_first_hits_bound).  The workgroup adds its valid nonces to `scanned`.
// No stop inside a tile.  No test hooks: mh_search_first_hits refuses them.
__global__ __launch_bounds__(kBlockThreads) void generic_scan_hits_stop(const GenArgs a, Partial* __restrict__ partials,
                                                                        const HitsStopArgs hs) {
    using namespace dev;
    __shared__ uint32_t s_skip;
    const uint64_t base = a.first + (uint64_t)blockIdx.x * kBlockThreads;  // a valid nonce: blocks = ceil(count / 256)
    if (threadIdx.x == 0)
        s_skip = base > __hip_atomic_load(hs.bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
    __syncthreads();
    if (s_skip) {  // one value per workgroup
        if (threadIdx.x == 0) partials[blockIdx.x] = Partial{~0ull, ~0ull};
        return;
    }
    const uint64_t n = base + threadIdx.x;
    const uint64_t left = a.count - (uint64_t)blockIdx.x * kBlockThreads;  // >= 1
    uint32_t h0, h1;
    hash_generic(a, n, h0, h1);
    uint64_t hash = ((uint64_t)h0 << 32) | h1, nonce = n;
    const bool hit = threadIdx.x < left && hash <= hs.h.target;
    const uint64_t hm = __builtin_amdgcn_ballot_w64(hit);
    if (hm) {  // one value per wave
        const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const uint32_t lead = (uint32_t)__builtin_ctzll(hm);
        uint32_t back = 0u;
        if (hit) back = atomicAdd(first_hits_slice(hs, n), 1u);
        asm volatile("" ::"v"(back) : "memory");  // the slice counts are back before the cursor advances
        unsigned long long taken = 0ull;
        if (lane == lead) taken = atomicAdd(hs.h.cursor, (unsigned long long)__builtin_popcountll(hm));
        const uint64_t first =
            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(taken >> 32), (int)lead) << 32) |
            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)taken, (int)lead);
        const uint64_t slot = first + (uint32_t)__builtin_popcountll(hm & ((1ull << lane) - 1ull));
        if (hit && slot < hs.h.cap) hs.h.hits[slot] = Hit{hash, nonce};
        if (first + (uint32_t)__builtin_popcountll(hm) >= hs.k) publish_first_hits_bound(hs, lane);
    }
    if (threadIdx.x >= left) {
        hash = ~0ull;
        nonce = ~0ull;
    }
    block_min(hash, nonce);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = Partial{hash, nonce};
        atomicAdd(hs.scanned, (unsigned long long)(left < (uint64_t)kBlockThreads ? left : (uint64_t)kBlockThreads));
    }
}

// The end of an mh_search_first, one thread on the main stream after the last merge: a winning
// key 0 (some nonce qualified; best->nonce is the smallest) becomes that nonce's real hash again,
// and the result leaves in one piece: out = {hash, nonce, nonces scanned}.
__global__ void finish_first(const GenArgs a, const Partial* __restrict__ best,
                             const unsigned long long* __restrict__ scanned, uint64_t* __restrict__ out) {
    Partial b = *best;
    if (b.hash == 0ull) {  // only a qualifying nonce has key 0 (the sentinel's is all ones)
        uint32_t h0, h1;
        dev::hash_generic(a, b.nonce, h0, h1);
        b.hash = ((uint64_t)h0 << 32) | h1;
    }
    out[0] = b.hash;
    out[1] = b.nonce;
    out[2] = *scanned;
}

__global__ __launch_bounds__(kBlockThreads) void hash_batch(const GenArgs a, const uint64_t* __restrict__ nonces,
                                                            uint64_t* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t h0, h1;
    dev::hash_generic(a, nonces[i], h0, h1);
    out[i] = ((uint64_t)h0 << 32) | h1;
}

// One workgroup of 1024 threads; each thread keeps 8 independent 16-byte
// loads in flight, so folding a full 65,536-slot buffer (1 MiB) takes ~8
// load round trips instead of 256 (the loop was latency-bound at 256 threads
// and one load per iteration).
constexpr int kMergeThreads = 1024;
constexpr int kMergeUnroll = 8;

__global__ __launch_bounds__(kMergeThreads) void merge_partials(const Partial* __restrict__ p, uint32_t n,
                                                                Partial* __restrict__ best) {
    using namespace dev;
    uint64_t h = ~0ull, nn = ~0ull;
    for (uint32_t base = 0; base < n; base += kMergeThreads * kMergeUnroll) {
        Partial x[kMergeUnroll];
#pragma unroll
        for (int u = 0; u < kMergeUnroll; ++u) {
            const uint32_t i = base + (uint32_t)u * kMergeThreads + threadIdx.x;
            x[u] = (i < n) ? p[i] : Partial{~0ull, ~0ull};
        }
#pragma unroll
        for (int u = 0; u < kMergeUnroll; ++u)
            if (lex_less(x[u].hash, x[u].nonce, h, nn)) {
                h = x[u].hash;
                nn = x[u].nonce;
            }
    }
    block_min<kMergeThreads>(h, nn);
    if (threadIdx.x == 0) {
        const Partial b = *best;
        if (lex_less(h, nn, b.hash, b.nonce)) *best = Partial{h, nn};
    }
}

// ---------------------------------------------------------------------------
// batched search: many small Requests in one launch
// ---------------------------------------------------------------------------
namespace dev {

// The ten nonces 10u .. 10u+9 of one aligned decade, digits jlo .. jhi of them (jlo > jhi: none),
// folded into the lane's running (bh, bn).  All ten have digits(u) + 1 digits (one for u = 0), so
// the tail image, the one- or two-block choice and the length words are made once; only the last
// digit's byte changes.  With two tail blocks and the last digit in the second, block 0 is
// compressed once for the ten.
// FIRST: the first-hit key (batch_scan_first): a hash <= target counts as 0, so the fold keeps the
// smallest qualifying nonce; no test hooks there (mh_search_first_batch refuses them).  Without
// FIRST, target is unused and the function is batch_scan's as before.
// HITS (batch_scan_hits): the product's own (hash, nonce) fold, and on a rare branch every nonce
// with hash <= target takes one slot from its request's cursor and stores {hash, nonce} at
// region[slot] if slot < region_slots (layout.hpp BatchHitsWords); no test hooks there either
// (mh_search_hits_batch refuses them).  Without HITS the three parameters after bn are unused.
// BOUND (batch_scan_bound): the product's fold with generic_scan_hits_stop's append, which whole
// waves make: every lane of the wave calls this and runs all ten digits, so the wave stays
// converged, and a digit outside jlo .. jhi, or any digit of a lane that is not `live` (it has no
// decade of the tile; u is then any decade of the entry), is hashed and ignored.  Per step, the
// wave's hits first count in their slices of the request's range, the counts are back before the
// lead lane advances the request's cursor, the hits go to the request's region below its end, and
// the wave whose cursor value plus its own hits reaches k publishes the request's bound (hs: the
// request's words as a HitsStopArgs).  No test hooks.  Without BOUND the two last parameters are unused.
template <bool FIRST, bool HITS = false, bool BOUND = false>
__device__ __forceinline__ void scan_decade(const GenArgs& a, uint64_t u, uint32_t jlo, uint32_t jhi, uint64_t target,
                                            uint64_t& bh, uint64_t& bn, unsigned long long* cursor = nullptr,
                                            Hit* region = nullptr, uint64_t region_slots = 0,
                                            const HitsStopArgs* hs = nullptr, bool live = true) {
    // digits of u; u <= (2^64 - 1) / 10 has at most 19
    constexpr uint64_t P10[19] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull,
                                  100000000ull, 1000000000ull, 10000000000ull, 100000000000ull, 1000000000000ull,
                                  10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                                  100000000000000000ull, 1000000000000000000ull};
    uint32_t nu = 0;  // Go %d of 10u + j: no leading zeros, so u = 0 contributes no digit
#pragma unroll
    for (int k = 0; k < 19; ++k) nu += (u >= P10[k]) ? 1u : 0u;
    uint32_t w[32];
#pragma unroll
    for (int x = 0; x < 16; ++x) w[x] = a.tail[x];
#pragma unroll
    for (int x = 16; x < 32; ++x) w[x] = 0u;
    uint64_t q = u;
#pragma unroll
    for (int k = 0; k < 19; ++k) {
        if ((uint32_t)k < nu) {
            const uint64_t q10 = q / 10u;
            const uint32_t dg = (uint32_t)(q - q10 * 10u);
            q = q10;
            const uint32_t pos = a.t + nu - 1u - (uint32_t)k;
            add_word(w, pos >> 2, (0x30u + dg) << (24u - 8u * (pos & 3u)));
        }
    }
    const uint32_t last = a.t + nu;  // tail byte of the last digit: '0' here, the digit is or-ed in per nonce
    const uint32_t lsh = 24u - 8u * (last & 3u);
    add_word(w, last >> 2, 0x30u << lsh);
    const uint32_t end = last + 1u;  // tail length; the 0x80 byte goes here
    add_word(w, end >> 2, 0x80u << (24u - 8u * (end & 3u)));
    const uint64_t bits = (a.plen + nu + 1u) * 8u;
    const bool two = end + 9u > 64u;
    const uint32_t bhi = (uint32_t)(bits >> 32), blo = (uint32_t)bits;
    w[14] = two ? w[14] : bhi;
    w[15] = two ? w[15] : blo;
    w[30] = two ? bhi : 0u;
    w[31] = two ? blo : 0u;
    // the block the last digit sits in varies per nonce; with two blocks it is block 1 (block 0
    // then compressed here, once) or block 0 (both blocks per nonce)
    const bool in1 = last >= 64u;
    const bool both = two && !in1;
    const uint32_t jw = (last >> 2) & 15u;
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = a.mid[i];
    if (in1) sha256_block(st, w);
    uint32_t v[16];
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        // both words read first: a select between two elements of w becomes a load through a
        // selected address, which keeps w out of registers (128 bytes of scratch)
        const uint32_t lo = w[x], hi = w[16 + x];
        v[x] = in1 ? hi : lo;
    }
    const uint32_t w16 = w[16];
    const uint64_t n0 = u * 10u;
#pragma unroll 1
    for (uint32_t j = BOUND ? 0u : jlo; j <= (BOUND ? 9u : jhi); ++j) {
        const uint32_t dj = j << lsh;
        uint32_t x[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = v[i] | ((jw == (uint32_t)i) ? dj : 0u);
        uint32_t s[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = st[i];
        if (both) {
            // block 1 is then padding only: the 0x80 byte if the tail ends at byte 64, and the
            // length (three live values instead of sixteen registers: 4 waves per SIMD, not 3)
            sha256_block(s, x);
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = 0u;
            x[0] = w16;
            x[14] = bhi;
            x[15] = blo;
        }
        uint32_t h0, h1;
        sha256_block_h01(s, x, h0, h1);
#ifdef MH_DEV_HOOKS  // hash-XOR and coarse-hash test hooks, as in generic_scan
        if constexpr (!FIRST && !HITS) {
            h0 = (h0 ^ mh_dev_hash_xor[0]) & keep_mask0(a.pad);
            h1 = (h1 ^ mh_dev_hash_xor[1]) & keep_mask1(a.pad);
        }
#endif
        uint64_t hash = ((uint64_t)h0 << 32) | h1;
        const uint64_t n = n0 + j;
        if constexpr (FIRST) {
            if (hash <= target) hash = 0ull;
        }
        if constexpr (HITS) {
            if (hash <= target) {  // rare with a sparse target
                const unsigned long long slot = atomicAdd(cursor, 1ull);
                if (slot < region_slots) region[slot] = Hit{hash, n};
            }
        }
        if constexpr (BOUND) {
            const bool mine = live && j >= jlo && j <= jhi;
            const bool hit = mine && hash <= target;
            const uint64_t hm = __builtin_amdgcn_ballot_w64(hit);
            if (hm) {  // one value per wave: generic_scan_hits_stop's append
                const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                const uint32_t lead = (uint32_t)__builtin_ctzll(hm);
                uint32_t back = 0u;
                if (hit) back = atomicAdd(first_hits_slice(*hs, n), 1u);
                asm volatile("" ::"v"(back) : "memory");  // the slice counts are back before the cursor advances
                unsigned long long taken = 0ull;
                if (lane == lead) taken = atomicAdd(hs->h.cursor, (unsigned long long)__builtin_popcountll(hm));
                const uint64_t first =
                    ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(taken >> 32), (int)lead) << 32) |
                    (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)taken, (int)lead);
                const uint64_t slot = first + (uint32_t)__builtin_popcountll(hm & ((1ull << lane) - 1ull));
                if (hit && slot < hs->h.cap) hs->h.hits[slot] = Hit{hash, n};
                if (first + (uint32_t)__builtin_popcountll(hm) >= hs->k) publish_first_hits_bound(*hs, lane);
            }
            if (!mine) continue;
        }
        if (lex_less(hash, n, bh, bn)) {
            bh = hash;
            bn = n;
        }
    }
}

}  // namespace dev

// One workgroup per tile of the pass; tile i runs kBatchTileDecades decades of its entry and
// writes partials[i].  The entry index comes from the host's per-tile table through
// readfirstlane, so the entry's fields are scalar loads.  No atomics, no counters and no
// dependency between workgroups: the grid always drains.
// SLOTS: the tile writes partials[slot0 + tile - tile0] instead of partials[tile] (batch_scan_slots).
template <bool SLOTS>
__device__ __forceinline__ void batch_scan_tile(const BatchEntry* __restrict__ entries,
                                                const uint32_t* __restrict__ tile_entry,
                                                Partial* __restrict__ partials) {
    using namespace dev;
    const uint32_t ei = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_entry[blockIdx.x]);
    const BatchEntry& e = entries[ei];
    const GenArgs& a = e.g;
    // decades of the entry, and the digits of its first and last decade that lie in the range
    // (first + count and 10u + 9 overflow at the top of u64; last = first + (count - 1) does not)
    const uint64_t first = a.first, lastn = a.first + (a.count - 1u);
    const uint64_t u_first = first / 10u, u_last = lastn / 10u;
    const uint32_t j_first = (uint32_t)(first - u_first * 10u), j_last = (uint32_t)(lastn - u_last * 10u);
    const uint64_t nd = u_last - u_first + 1u;  // >= 1; offsets below it are decades of the entry
    const uint64_t base = (uint64_t)(blockIdx.x - e.tile0) * kBatchTileDecades;
    uint64_t bh = ~0ull, bn = ~0ull;
#pragma unroll 1
    for (int k = 0; k < kBatchDecades; ++k) {
        const uint64_t off = base + (uint32_t)k * (uint32_t)kBlockThreads + threadIdx.x;
        if (off < nd) {
            const uint64_t u = u_first + off;
            scan_decade<false>(a, u, off == 0u ? j_first : 0u, u == u_last ? j_last : 9u, 0ull, bh, bn);
        }
    }
    block_min(bh, bn);
    if (threadIdx.x == 0) partials[SLOTS ? e.slot0 + (blockIdx.x - e.tile0) : blockIdx.x] = Partial{bh, bn};
}

__global__ __launch_bounds__(kBlockThreads) void batch_scan(const BatchEntry* __restrict__ entries,
                                                            const uint32_t* __restrict__ tile_entry,
                                                            Partial* __restrict__ partials) {
    batch_scan_tile<false>(entries, tile_entry, partials);
}

// batch_scan for a pass of mh_search_batch_ex(MH_BATCH_FUSE_FAST): a request's slot segment holds
// its tiles and its fast pieces' chunks in nonce order, so an entry's slots start at slot0, apart
// from tile0 (the host checks that every slot has exactly one writer, plan.cpp batch_tables_ex_ok).
__global__ __launch_bounds__(kBlockThreads) void batch_scan_slots(const BatchEntry* __restrict__ entries,
                                                                  const uint32_t* __restrict__ tile_entry,
                                                                  Partial* __restrict__ partials) {
    batch_scan_tile<true>(entries, tile_entry, partials);
}

// batch_scan for mh_search_first_batch: workgroup b runs tile order[b] -- the host's
// rank-major dispatch order, a permutation of the pass's tiles -- with first-hit keys, and writes
// partials[order[b]], so slots and segments keep batch_scan's layout.  The tile's request
// (entry_req[entry]) has three device words (layout.hpp BatchFirstWords).  Thread 0 reads the
// request's `first` word once before any hashing; the tile is skipped -- it writes the sentinel --
// only when its smallest in-range nonce is larger than that word.  The word only decreases and
// always holds a qualifying nonce of the request's range, so the tile of the smallest one, and
// every tile with a smaller nonce, runs whatever value the read returns.  A tile that ran lowers
// the word if it found a hit and adds its valid nonces to `scanned`.  No workgroup waits for
// another: the grid always drains.  No test hooks.
// SLOTS: the tile writes partials[slot0 + tile - tile0] instead of partials[tile] (batch_scan_first_slots).
template <bool SLOTS>
__device__ __forceinline__ void batch_scan_first_tile(const BatchEntry* __restrict__ entries,
                                                      const uint32_t* __restrict__ tile_entry,
                                                      const uint32_t* __restrict__ entry_req,
                                                      const uint32_t* __restrict__ order, BatchFirstWords* words,
                                                      Partial* __restrict__ partials) {
    using namespace dev;
    __shared__ uint32_t s_skip;
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)order[blockIdx.x]);
    const uint32_t ei = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_entry[tile]);
    const uint32_t ri = (uint32_t)__builtin_amdgcn_readfirstlane((int)entry_req[ei]);
    const BatchEntry& e = entries[ei];
    const GenArgs& a = e.g;
    BatchFirstWords* w = words + ri;
    const uint32_t slot = SLOTS ? e.slot0 + (tile - e.tile0) : tile;
    const uint64_t first = a.first, lastn = a.first + (a.count - 1u);
    const uint64_t u_first = first / 10u, u_last = lastn / 10u;
    const uint32_t j_first = (uint32_t)(first - u_first * 10u), j_last = (uint32_t)(lastn - u_last * 10u);
    const uint64_t nd = u_last - u_first + 1u;
    const uint64_t base = (uint64_t)(tile - e.tile0) * kBatchTileDecades;  // < nd (the host's table check)
    // the tile's decades d_lo .. d_hi and its nonces n_lo .. n_hi, ragged at the entry's two ends;
    // (u_first + base) * 10 <= lastn, and d_hi * 10 + 9 is formed only below the entry's last decade
    const uint64_t d_lo = u_first + base;
    const uint64_t d_hi = nd - base > (uint64_t)kBatchTileDecades ? d_lo + (kBatchTileDecades - 1u) : u_last;
    const uint64_t n_lo = base == 0u ? first : d_lo * 10u;  // the tile's smallest in-range nonce
    const uint64_t n_hi = d_hi == u_last ? lastn : d_hi * 10u + 9u;
    if (threadIdx.x == 0)
        s_skip = n_lo > __hip_atomic_load(&w->first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
    __syncthreads();
    if (s_skip) {  // one value per workgroup
        if (threadIdx.x == 0) partials[slot] = Partial{~0ull, ~0ull};
        return;
    }
    const uint64_t target = w->target;  // never written on the device
    uint64_t bh = ~0ull, bn = ~0ull;
#pragma unroll 1
    for (int k = 0; k < kBatchDecades; ++k) {
        const uint64_t off = base + (uint32_t)k * (uint32_t)kBlockThreads + threadIdx.x;
        if (off < nd) {
            const uint64_t u = u_first + off;
            scan_decade<true>(a, u, off == 0u ? j_first : 0u, u == u_last ? j_last : 9u, target, bh, bn);
        }
    }
    block_min(bh, bn);
    if (threadIdx.x == 0) {
        partials[slot] = Partial{bh, bn};
        if (bh == 0ull) atomicMin(&w->first, (unsigned long long)bn);
        atomicAdd(&w->scanned, (unsigned long long)(n_hi - n_lo + 1u));
    }
}

__global__ __launch_bounds__(kBlockThreads) void batch_scan_first(const BatchEntry* __restrict__ entries,
                                                                  const uint32_t* __restrict__ tile_entry,
                                                                  const uint32_t* __restrict__ entry_req,
                                                                  const uint32_t* __restrict__ order,
                                                                  BatchFirstWords* words,
                                                                  Partial* __restrict__ partials) {
    batch_scan_first_tile<false>(entries, tile_entry, entry_req, order, words, partials);
}

// batch_scan_first for a pass of mh_search_first_batch_ex(MH_BATCH_FUSE_FAST) that holds fast
// pieces: a request's slot segment holds its tiles and its fast chunks in nonce order, so an
// entry's slots start at slot0, apart from tile0; order is still a permutation of the pass's tiles
// (the host checks both and that every slot has exactly one writer, plan.cpp first_batch_tables_ex_ok).
// The words a tile reads and lowers are the ones batch_first's chunks of the same request use.
__global__ __launch_bounds__(kBlockThreads) void batch_scan_first_slots(const BatchEntry* __restrict__ entries,
                                                                        const uint32_t* __restrict__ tile_entry,
                                                                        const uint32_t* __restrict__ entry_req,
                                                                        const uint32_t* __restrict__ order,
                                                                        BatchFirstWords* words,
                                                                        Partial* __restrict__ partials) {
    batch_scan_first_tile<true>(entries, tile_entry, entry_req, order, words, partials);
}

// batch_scan for mh_search_hits_batch: batch_scan's static grid and identity tile
// order -- workgroup b runs tile b and writes partials[b] -- with the product's (hash, nonce)
// minimum, so slots, segments and merge keep batch_scan's layout and give mh_search's result.  The
// tile's request (entry_req[entry]) has four device words (layout.hpp BatchHitsWords): every nonce
// with Hash <= target takes one slot from the request's cursor and stores {hash, nonce} at entry
// offset + slot of the device hit buffer only if slot < slots, so nothing is written outside the
// request's region (the host checks the regions of a window before every launch: inside the
// buffer and disjoint).  Every nonce of a request belongs to exactly one (tile, lane, digit) and
// every tile runs exactly once, so the cursor ends as the request's exact count.  No skipping, no
// waiting, no dependency between workgroups: the grid always drains.  No test hooks.
// SLOTS: the tile writes partials[slot0 + tile - tile0] instead of partials[tile] (batch_scan_hits_slots).
template <bool SLOTS>
__device__ __forceinline__ void batch_scan_hits_tile(const BatchEntry* __restrict__ entries,
                                                     const uint32_t* __restrict__ tile_entry,
                                                     const uint32_t* __restrict__ entry_req, BatchHitsWords* words,
                                                     Hit* hits, Partial* __restrict__ partials) {
    using namespace dev;
    const uint32_t ei = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_entry[blockIdx.x]);
    const uint32_t ri = (uint32_t)__builtin_amdgcn_readfirstlane((int)entry_req[ei]);
    const BatchEntry& e = entries[ei];
    const GenArgs& a = e.g;
    BatchHitsWords* w = words + ri;
    const uint64_t target = w->target, region_slots = w->slots;  // never written on the device
    Hit* region = hits + w->offset;
    const uint64_t first = a.first, lastn = a.first + (a.count - 1u);
    const uint64_t u_first = first / 10u, u_last = lastn / 10u;
    const uint32_t j_first = (uint32_t)(first - u_first * 10u), j_last = (uint32_t)(lastn - u_last * 10u);
    const uint64_t nd = u_last - u_first + 1u;
    const uint64_t base = (uint64_t)(blockIdx.x - e.tile0) * kBatchTileDecades;
    uint64_t bh = ~0ull, bn = ~0ull;
#pragma unroll 1
    for (int k = 0; k < kBatchDecades; ++k) {
        const uint64_t off = base + (uint32_t)k * (uint32_t)kBlockThreads + threadIdx.x;
        if (off < nd) {
            const uint64_t u = u_first + off;
            scan_decade<false, true>(a, u, off == 0u ? j_first : 0u, u == u_last ? j_last : 9u, target, bh, bn,
                                     &w->cursor, region, region_slots);
        }
    }
    block_min(bh, bn);
    if (threadIdx.x == 0) partials[SLOTS ? e.slot0 + (blockIdx.x - e.tile0) : blockIdx.x] = Partial{bh, bn};
}

__global__ __launch_bounds__(kBlockThreads) void batch_scan_hits(const BatchEntry* __restrict__ entries,
                                                                 const uint32_t* __restrict__ tile_entry,
                                                                 const uint32_t* __restrict__ entry_req,
                                                                 BatchHitsWords* words, Hit* hits,
                                                                 Partial* __restrict__ partials) {
    batch_scan_hits_tile<false>(entries, tile_entry, entry_req, words, hits, partials);
}

// batch_scan_hits for a pass of mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST) that holds fast pieces:
// a request's slot segment holds its tiles and its fast chunks in nonce order, so an entry's slots
// start at slot0, apart from tile0 (the host checks that every slot has exactly one writer, plan.cpp
// hits_batch_tables_ex_ok).  The cursor and the region a tile appends to are the ones batch_hits'
// chunks of the same request use.
__global__ __launch_bounds__(kBlockThreads) void batch_scan_hits_slots(const BatchEntry* __restrict__ entries,
                                                                       const uint32_t* __restrict__ tile_entry,
                                                                       const uint32_t* __restrict__ entry_req,
                                                                       BatchHitsWords* words, Hit* hits,
                                                                       Partial* __restrict__ partials) {
    batch_scan_hits_tile<true>(entries, tile_entry, entry_req, words, hits, partials);
}

// batch_scan for mh_search_first_hits_batch: batch_scan_hits' tile -- the product's
// (hash, nonce) minimum, every hit appended through the request's cursor into the request's region
// of the device hit buffer, nothing stored at or past the region's end -- taken in
// batch_scan_first's order: workgroup b runs tile order[b], the host's rank-major dispatch order, a
// permutation of the pass's tiles.  The tile's request (entry_req[entry]) has its device words
// (layout.hpp BatchBoundWords) and kFirstHitsSlices slice counters at slices + request *
// kFirstHitsSlices.  Before any hashing thread 0 reads the request's bound once; a tile whose
// smallest in-range nonce is above it writes the sentinel and ends (at least k hits of the request
// are <= the word's value, so none of the tile's nonces is among the request's k smallest hits; the
// word only decreases, so a stale read only skips less).  A tile that runs adds its valid nonces to
// the request's `scanned`; its hits count in their slices before the cursor advances, and the wave
// whose cursor value plus its own hits reaches k publishes the bound (scan_decade<.., BOUND>).  No
// stop inside a tile, no workgroup waits for another: the grid always drains.  No test hooks.
// SLOTS: the tile writes partials[slot0 + tile - tile0] instead of partials[tile] (batch_scan_bound_slots).
template <bool SLOTS>
__device__ __forceinline__ void batch_scan_bound_tile(const BatchEntry* __restrict__ entries,
                                                      const uint32_t* __restrict__ tile_entry,
                                                      const uint32_t* __restrict__ entry_req,
                                                      const uint32_t* __restrict__ order, BatchBoundWords* words,
                                                      uint32_t* slices, Hit* hits, Partial* __restrict__ partials) {
    using namespace dev;
    __shared__ uint32_t s_skip;
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)order[blockIdx.x]);
    const uint32_t ei = (uint32_t)__builtin_amdgcn_readfirstlane((int)tile_entry[tile]);
    const uint32_t ri = (uint32_t)__builtin_amdgcn_readfirstlane((int)entry_req[ei]);
    const BatchEntry& e = entries[ei];
    const GenArgs& a = e.g;
    BatchBoundWords* w = words + ri;
    const uint32_t slot = SLOTS ? e.slot0 + (tile - e.tile0) : tile;
    const uint64_t first = a.first, lastn = a.first + (a.count - 1u);
    const uint64_t u_first = first / 10u, u_last = lastn / 10u;
    const uint32_t j_first = (uint32_t)(first - u_first * 10u), j_last = (uint32_t)(lastn - u_last * 10u);
    const uint64_t nd = u_last - u_first + 1u;
    const uint64_t base = (uint64_t)(tile - e.tile0) * kBatchTileDecades;  // < nd (the host's table check)
    // the tile's nonces n_lo .. n_hi, ragged at the entry's two ends (batch_scan_first's)
    const uint64_t d_lo = u_first + base;
    const uint64_t d_hi = nd - base > (uint64_t)kBatchTileDecades ? d_lo + (kBatchTileDecades - 1u) : u_last;
    const uint64_t n_lo = base == 0u ? first : d_lo * 10u;  // the tile's smallest in-range nonce
    const uint64_t n_hi = d_hi == u_last ? lastn : d_hi * 10u + 9u;
    if (threadIdx.x == 0)
        s_skip = n_lo > __hip_atomic_load(&w->bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
    __syncthreads();
    if (s_skip) {  // one value per workgroup
        if (threadIdx.x == 0) partials[slot] = Partial{~0ull, ~0ull};
        return;
    }
    // the request's words as the stopping hits kernels take them; none but cursor, bound and scanned
    // (and the counters) is written on the device
    const HitsStopArgs hs{HitsArgs{w->target, &w->cursor, hits + w->offset, w->slots},
                          w->k,
                          &w->bound,
                          slices + (size_t)ri * kFirstHitsSlices,
                          w->lower,
                          w->span,
                          w->shift,
                          0u,
                          &w->scanned};
    uint64_t bh = ~0ull, bn = ~0ull;
#pragma unroll 1
    for (int k = 0; k < kBatchDecades; ++k) {
        // every lane runs a decade, so that the waves stay whole for the append: one past the
        // entry's last runs the entry's first with nothing of it counted
        const uint64_t off = base + (uint32_t)k * (uint32_t)kBlockThreads + threadIdx.x;
        const bool live = off < nd;
        const uint64_t u = live ? u_first + off : u_first;
        scan_decade<false, false, true>(a, u, live && off == 0u ? j_first : 0u, u == u_last ? j_last : 9u, hs.h.target, bh,
                                        bn, nullptr, nullptr, 0, &hs, live);
    }
    block_min(bh, bn);
    if (threadIdx.x == 0) {
        partials[slot] = Partial{bh, bn};
        atomicAdd(&w->scanned, (unsigned long long)(n_hi - n_lo + 1u));
    }
}

__global__ __launch_bounds__(kBlockThreads) void batch_scan_bound(const BatchEntry* __restrict__ entries,
                                                                  const uint32_t* __restrict__ tile_entry,
                                                                  const uint32_t* __restrict__ entry_req,
                                                                  const uint32_t* __restrict__ order,
                                                                  BatchBoundWords* words, uint32_t* slices, Hit* hits,
                                                                  Partial* __restrict__ partials) {
    batch_scan_bound_tile<false>(entries, tile_entry, entry_req, order, words, slices, hits, partials);
}

// batch_scan_bound for a pass of mh_search_first_hits_batch(MH_BATCH_FUSE_FAST) that holds fast
// pieces: a request's slot segment holds its tiles and its fast chunks in nonce order, so an entry's
// slots start at slot0, apart from tile0; order is still a permutation of the pass's tiles.  The
// words, the region and the counters a tile uses are the ones batch_bound's chunks of the same
// request use.
__global__ __launch_bounds__(kBlockThreads) void batch_scan_bound_slots(const BatchEntry* __restrict__ entries,
                                                                        const uint32_t* __restrict__ tile_entry,
                                                                        const uint32_t* __restrict__ entry_req,
                                                                        const uint32_t* __restrict__ order,
                                                                        BatchBoundWords* words, uint32_t* slices,
                                                                        Hit* hits, Partial* __restrict__ partials) {
    batch_scan_bound_tile<true>(entries, tile_entry, entry_req, order, words, slices, hits, partials);
}

// One workgroup per request of the pass: results[r] = the lexicographic minimum of
// partials[seg[r] .. seg[r + 1]) (never empty; the host checks the table before the launch).
__global__ __launch_bounds__(kBlockThreads) void merge_segments(const Partial* __restrict__ partials,
                                                                const uint32_t* __restrict__ seg,
                                                                Partial* __restrict__ results) {
    using namespace dev;
    const uint32_t r = blockIdx.x;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r]);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r + 1]);
    uint64_t h = ~0ull, n = ~0ull;
    for (uint32_t i = a + threadIdx.x; i < b; i += kBlockThreads) {
        const Partial x = partials[i];
        if (lex_less(x.hash, x.nonce, h, n)) {
            h = x.hash;
            n = x.nonce;
        }
    }
    block_min(h, n);
    if (threadIdx.x == 0) results[r] = Partial{h, n};
}

// merge_segments for mh_search_first_batch: the same fold, then thread 0 turns a winning key 0
// (some nonce of the request qualified; n is the smallest) back into that nonce's hash -- with the
// GenArgs of the request's first entry: mid, tail, plen and t are per message -- and writes
// results[r] = {hash, nonce, the request's scanned count}.
__global__ __launch_bounds__(kBlockThreads) void merge_segments_first(const Partial* __restrict__ partials,
                                                                      const uint32_t* __restrict__ seg,
                                                                      const BatchEntry* __restrict__ entries,
                                                                      const uint32_t* __restrict__ tile_entry,
                                                                      const BatchFirstWords* __restrict__ words,
                                                                      BatchFirstResult* __restrict__ results) {
    using namespace dev;
    const uint32_t r = blockIdx.x;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r]);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r + 1]);
    uint64_t h = ~0ull, n = ~0ull;
    for (uint32_t i = a + threadIdx.x; i < b; i += kBlockThreads) {
        const Partial x = partials[i];
        if (lex_less(x.hash, x.nonce, h, n)) {
            h = x.hash;
            n = x.nonce;
        }
    }
    block_min(h, n);
    if (threadIdx.x == 0) {
        if (h == 0ull) {  // only a qualifying nonce has key 0 (the sentinel's is all ones)
            uint32_t h0, h1;
            hash_generic(entries[tile_entry[a]].g, n, h0, h1);
            h = ((uint64_t)h0 << 32) | h1;
        }
        results[r] = BatchFirstResult{h, n, words[r].scanned};
    }
}

// merge_segments_first for a pass of mh_search_first_batch_ex that holds fast pieces: seg[r] is a
// slot, not a tile, and a request whose range is one fast piece has no entry, so the message state
// of the winner's hash comes from req_gen[r], a GenArgs per request (mid, tail, plen, t).
__global__ __launch_bounds__(kBlockThreads) void merge_segments_first_ex(const Partial* __restrict__ partials,
                                                                         const uint32_t* __restrict__ seg,
                                                                         const GenArgs* __restrict__ req_gen,
                                                                         const BatchFirstWords* __restrict__ words,
                                                                         BatchFirstResult* __restrict__ results) {
    using namespace dev;
    const uint32_t r = blockIdx.x;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r]);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r + 1]);
    uint64_t h = ~0ull, n = ~0ull;
    for (uint32_t i = a + threadIdx.x; i < b; i += kBlockThreads) {
        const Partial x = partials[i];
        if (lex_less(x.hash, x.nonce, h, n)) {
            h = x.hash;
            n = x.nonce;
        }
    }
    block_min(h, n);
    if (threadIdx.x == 0) {
        if (h == 0ull) {  // only a qualifying nonce has key 0 (the sentinel's is all ones)
            uint32_t h0, h1;
            hash_generic(req_gen[r], n, h0, h1);
            h = ((uint64_t)h0 << 32) | h1;
        }
        results[r] = BatchFirstResult{h, n, words[r].scanned};
    }
}

// merge_segments for mh_search_hits_batch: the same fold, and results[r] = {hash, nonce, the
// request's cursor}, final since every tile of the pass has run (stream order).  Then the entries
// the request's region kept, min(cursor, slots) of them, move to packed[]: behind those of the
// pass's earlier requests (every workgroup sums them itself: at most 4,096 words) and of the
// window's earlier passes (*base_in, written by the last workgroup of the pass before; null in a
// window's first pass: 0), so that a drain copies home the entries stored and not the regions'
// whole extent.  The last workgroup writes the running total to *base_out, another word than
// *base_in.  Nothing is stored at or beyond packed[limit], where the window's regions end.
__global__ __launch_bounds__(kBlockThreads) void merge_segments_hits(const Partial* __restrict__ partials,
                                                                     const uint32_t* __restrict__ seg,
                                                                     const BatchHitsWords* __restrict__ words,
                                                                     const Hit* __restrict__ hits,
                                                                     Hit* __restrict__ packed, uint64_t limit,
                                                                     const unsigned long long* base_in,
                                                                     unsigned long long* base_out,
                                                                     BatchHitsResult* __restrict__ results) {
    using namespace dev;
    __shared__ unsigned long long s_before;
    const uint32_t r = blockIdx.x;
    if (threadIdx.x == 0) s_before = base_in ? *base_in : 0ull;
    __syncthreads();
    unsigned long long before = 0ull;
    for (uint32_t j = threadIdx.x; j < r; j += kBlockThreads) {
        const unsigned long long c = words[j].cursor, sl = words[j].slots;
        before += c < sl ? c : sl;
    }
    if (before) atomicAdd(&s_before, before);
    __syncthreads();
    const uint64_t base = s_before;
    const uint64_t count = words[r].cursor;
    const uint64_t kept = count < words[r].slots ? count : words[r].slots;
    const Hit* region = hits + words[r].offset;
    for (uint64_t i = threadIdx.x; i < kept; i += kBlockThreads)
        if (base + i < limit) packed[base + i] = region[i];
    if (threadIdx.x == 0 && r + 1u == gridDim.x) *base_out = base + kept;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r]);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r + 1]);
    uint64_t h = ~0ull, n = ~0ull;
    for (uint32_t i = a + threadIdx.x; i < b; i += kBlockThreads) {
        const Partial x = partials[i];
        if (lex_less(x.hash, x.nonce, h, n)) {
            h = x.hash;
            n = x.nonce;
        }
    }
    block_min(h, n);
    if (threadIdx.x == 0) results[r] = BatchHitsResult{h, n, count};
}

// merge_segments_hits for mh_search_first_hits_batch: the same fold and the same packing of the
// entries the request's region kept, over BatchBoundWords, and results[r] = {hash, nonce, the
// request's cursor, its scanned count}, all final since every tile and chunk of the pass has run
// (stream order).  The minimum is the request's only when nothing of it was skipped or left (the
// sentinel of a skipped tile or chunk is all ones); the host uses it only then.
__global__ __launch_bounds__(kBlockThreads) void merge_segments_bound(const Partial* __restrict__ partials,
                                                                      const uint32_t* __restrict__ seg,
                                                                      const BatchBoundWords* __restrict__ words,
                                                                      const Hit* __restrict__ hits,
                                                                      Hit* __restrict__ packed, uint64_t limit,
                                                                      const unsigned long long* base_in,
                                                                      unsigned long long* base_out,
                                                                      BatchBoundResult* __restrict__ results) {
    using namespace dev;
    __shared__ unsigned long long s_before;
    const uint32_t r = blockIdx.x;
    if (threadIdx.x == 0) s_before = base_in ? *base_in : 0ull;
    __syncthreads();
    unsigned long long before = 0ull;
    for (uint32_t j = threadIdx.x; j < r; j += kBlockThreads) {
        const unsigned long long c = words[j].cursor, sl = words[j].slots;
        before += c < sl ? c : sl;
    }
    if (before) atomicAdd(&s_before, before);
    __syncthreads();
    const uint64_t base = s_before;
    const uint64_t count = words[r].cursor;
    const uint64_t kept = count < words[r].slots ? count : words[r].slots;
    const Hit* region = hits + words[r].offset;
    for (uint64_t i = threadIdx.x; i < kept; i += kBlockThreads)
        if (base + i < limit) packed[base + i] = region[i];
    if (threadIdx.x == 0 && r + 1u == gridDim.x) *base_out = base + kept;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r]);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[r + 1]);
    uint64_t h = ~0ull, n = ~0ull;
    for (uint32_t i = a + threadIdx.x; i < b; i += kBlockThreads) {
        const Partial x = partials[i];
        if (lex_less(x.hash, x.nonce, h, n)) {
            h = x.hash;
            n = x.nonce;
        }
    }
    block_min(h, n);
    if (threadIdx.x == 0) results[r] = BatchBoundResult{h, n, count, words[r].scanned};
}

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------
// fast_search<J, MODE> lives in a code object of its own, loaded once per
// device and launched by its mangled name.  The product library knows only the
// embedded code object.  The dev build (`make dev`, -DMH_DEV_HOOKS,
// build/dev/libminehip.so; never shipped as the package's library) also
// reads MINEHIP_DEV_CODE_OBJECT, a code object file to use instead (e.g. the
// same kernels without the issue-priority pass, tools/isa_variant.py), on
// every launch so that tools/kbench.py can interleave variants in one process.
namespace {
std::mutex g_mod_mu;
std::map<std::pair<std::string, int>, hipModule_t> g_mods;                    // (file or "", dev)
std::map<std::pair<hipModule_t, int>, hipFunction_t> g_funcs;                // (module, J + 16 * mode)
std::map<hipModule_t, bool> g_queue_ok;  // the module's kernels run the work-queue loop (marker)
#ifdef MH_DEV_HOOKS
std::map<hipModule_t, bool> g_keep_ok;   // the module's kernels mask hashes by FastArgs::pad_ (marker)
std::map<hipModule_t, hipDeviceptr_t> g_xor_ptr;  // the module's mh_dev_hash_xor (null: its kernels do not XOR)
std::map<hipModule_t, uint64_t> g_xor_mod;        // ... and the value it holds
std::map<int, uint64_t> g_xor_lib;                // the value this library's own mh_dev_hash_xor holds, per device
#endif

// queue_ok: the code object carries fast_search.hip's mh_fast_queue_args marker at this
// library's sizeof(FastArgs), i.e. its kernels claim chunks from a.counter
// variant: kFastFirst, the first-hit kernels first_scan<J, MODE> of the second embedded code object
// (module key ":first", no file of that name is ever loaded), or kFastHits, the hits kernels
// hits_scan<J, MODE> of the third (":hits"); no hook replaces either
// or kFastBatch, batch_fast<J, MODE> of the fourth (":batch"; the dev build reads
// MINEHIP_DEV_BATCH_CODE_OBJECT, a code object file to use instead: build/fast_batch_keep.hsaco)
// or kFastBatchFirst, batch_first<J, MODE> of the fifth (":batch_first"; no hook replaces it), whose
// marker is mh_fast_batch_first_items at sizeof(BatchFirstItem)
// or kFastBatchHits, batch_hits<J, MODE> of the sixth (":batch_hits"; no hook replaces it), whose
// marker is mh_fast_batch_hits_items at sizeof(BatchHitsItem)
// or kFastFirstStop, stop_scan<J, MODE> of the seventh (":first_stop"; no hook replaces it): first_scan's
// parameters and marker
// or kFastBatchStop, batch_stop<J, MODE> of the eighth (":batch_first_stop"; no hook replaces it):
// batch_first's parameters, its marker mh_fast_batch_stop_items at sizeof(BatchFirstItem)
// or kFastHitsStop, hits_stop<J, MODE> of the ninth (":hits_stop"; no hook replaces it): hits_scan's
// first two parameters, a HitsStopArgs as the third, and fast_search's marker
// or kFastBatchBound, batch_bound<J, MODE> of the tenth (":batch_bound"; no hook replaces it):
// batch_first's parameters over BatchBoundItems, its marker mh_fast_batch_bound_items at sizeof(BatchBoundItem)
enum FastVariant { kFastProduct = 0, kFastFirst = 1, kFastHits = 2, kFastBatch = 3, kFastBatchFirst = 4, kFastBatchHits = 5,
                   kFastFirstStop = 6, kFastBatchStop = 7, kFastHitsStop = 8, kFastBatchBound = 9 };
#ifdef MH_DEV_HOOKS
std::string batch_module_path() {
    const char* co = getenv("MINEHIP_DEV_BATCH_CODE_OBJECT");
    return (co && *co) ? co : ":batch";
}
#else
std::string batch_module_path() { return ":batch"; }
#endif
hipError_t fast_function(int dev, int J, int mode, hipFunction_t* f, bool* queue_ok = nullptr,
                         FastVariant variant = kFastProduct) {
    const bool first = variant == kFastFirst, hits = variant == kFastHits, batch = variant == kFastBatch;
    const bool bfirst = variant == kFastBatchFirst, bhits = variant == kFastBatchHits, fstop = variant == kFastFirstStop;
    const bool bstop = variant == kFastBatchStop, hstop = variant == kFastHitsStop, bbound = variant == kFastBatchBound;
#ifdef MH_DEV_HOOKS
    const char* co = getenv("MINEHIP_DEV_CODE_OBJECT");
    const std::string path = first ? ":first" : fstop ? ":first_stop" : hits ? ":hits" : hstop ? ":hits_stop" : batch ? batch_module_path()
                             : bfirst ? ":batch_first" : bstop ? ":batch_first_stop" : bhits ? ":batch_hits" : bbound ? ":batch_bound" : (co && *co) ? co : "";
#else
    const std::string path = first ? ":first" : fstop ? ":first_stop" : hits ? ":hits" : hstop ? ":hits_stop" : batch ? batch_module_path()
                             : bfirst ? ":batch_first" : bstop ? ":batch_first_stop" : bhits ? ":batch_hits" : bbound ? ":batch_bound" : "";
#endif
    std::lock_guard<std::mutex> g(g_mod_mu);
    auto it = g_mods.find({path, dev});
    if (it == g_mods.end()) {
        hipModule_t m;
        const hipError_t e = first          ? hipModuleLoadData(&m, mh_first_co_begin)
                             : fstop        ? hipModuleLoadData(&m, mh_first_stop_co_begin)
                             : hits         ? hipModuleLoadData(&m, mh_hits_co_begin)
                             : hstop        ? hipModuleLoadData(&m, mh_hits_stop_co_begin)
                             : path == ":batch" ? hipModuleLoadData(&m, mh_batch_co_begin)
                             : bfirst       ? hipModuleLoadData(&m, mh_batch_first_co_begin)
                             : bstop        ? hipModuleLoadData(&m, mh_batch_first_stop_co_begin)
                             : bhits        ? hipModuleLoadData(&m, mh_batch_hits_co_begin)
                             : bbound       ? hipModuleLoadData(&m, mh_batch_bound_co_begin)
                             : path.empty() ? hipModuleLoadData(&m, mh_fast_co_begin)
                                            : hipModuleLoad(&m, path.c_str());
        if (e != hipSuccess) {
            (void)hipGetLastError();  // the failure is returned here; do not leave it for the next launch check
            return e;
        }
        it = g_mods.emplace(std::make_pair(path, dev), m).first;
        hipDeviceptr_t gp = nullptr;
        size_t gsz = 0;
        // (a batch code object: mh_fast_batch_items at sizeof(BatchFastItem), the table layout its kernels read)
        const bool marked = batch ? hipModuleGetGlobal(&gp, &gsz, m, "mh_fast_batch_items") == hipSuccess &&
                                        gsz == sizeof(BatchFastItem)
                            : bfirst ? hipModuleGetGlobal(&gp, &gsz, m, "mh_fast_batch_first_items") == hipSuccess &&
                                        gsz == sizeof(BatchFirstItem)
                            : bstop ? hipModuleGetGlobal(&gp, &gsz, m, "mh_fast_batch_stop_items") == hipSuccess &&
                                        gsz == sizeof(BatchFirstItem)
                            : bhits ? hipModuleGetGlobal(&gp, &gsz, m, "mh_fast_batch_hits_items") == hipSuccess &&
                                        gsz == sizeof(BatchHitsItem)
                            : bbound ? hipModuleGetGlobal(&gp, &gsz, m, "mh_fast_batch_bound_items") == hipSuccess &&
                                        gsz == sizeof(BatchBoundItem)
                                  : hipModuleGetGlobal(&gp, &gsz, m, "mh_fast_queue_args") == hipSuccess &&
                                        gsz == sizeof(FastArgs);
        (void)hipGetLastError();
        g_queue_ok[m] = marked;
#ifdef MH_DEV_HOOKS
        const bool keeps = hipModuleGetGlobal(&gp, &gsz, m, "mh_fast_hash_keep") == hipSuccess &&
                           gsz == sizeof(FastArgs);
        (void)hipGetLastError();
        g_keep_ok[m] = keeps;
        const bool xors = hipModuleGetGlobal(&gp, &gsz, m, "mh_dev_hash_xor") == hipSuccess &&
                          gsz == 2 * sizeof(uint32_t);
        (void)hipGetLastError();
        g_xor_ptr[m] = xors ? gp : nullptr;
        g_xor_mod[m] = 0;
#endif
    }
    if (queue_ok) *queue_ok = g_queue_ok[it->second];
    auto fit = g_funcs.find({it->second, J + 16 * mode});
    if (fit == g_funcs.end()) {
        char name[96];
        snprintf(name, sizeof name,
                 bfirst ? "_ZN2mh11batch_firstILi%dELi%dEEEvPKNS_14BatchFirstItemEPKjS5_PNS_7PartialE"
                 : bstop ? "_ZN2mh10batch_stopILi%dELi%dEEEvPKNS_14BatchFirstItemEPKjS5_PNS_7PartialE"
                 : bhits ? "_ZN2mh10batch_hitsILi%dELi%dEEEvPKNS_13BatchHitsItemEPKjPNS_7PartialE"
                 : bbound ? "_ZN2mh11batch_boundILi%dELi%dEEEvPKNS_14BatchBoundItemEPKjS5_PNS_7PartialE"
                 : first ? "_ZN2mh10first_scanILi%dELi%dEEEvNS_8FastArgsEPNS_7PartialENS_9FirstArgsE"
                 : fstop ? "_ZN2mh9stop_scanILi%dELi%dEEEvNS_8FastArgsEPNS_7PartialENS_9FirstArgsE"
                 : hits ? "_ZN2mh9hits_scanILi%dELi%dEEEvNS_8FastArgsEPNS_7PartialENS_8HitsArgsE"
                 : hstop ? "_ZN2mh9hits_stopILi%dELi%dEEEvNS_8FastArgsEPNS_7PartialENS_12HitsStopArgsE"
                 : batch ? "_ZN2mh10batch_fastILi%dELi%dEEEvPKNS_13BatchFastItemEPKjPNS_7PartialE"
                        : "_ZN2mh11fast_searchILi%dELi%dEEEvNS_8FastArgsEPNS_7PartialE",
                 J, mode);
        hipFunction_t fn;
        const hipError_t e = hipModuleGetFunction(&fn, it->second, name);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return e;
        }
        fit = g_funcs.emplace(std::make_pair(it->second, J + 16 * mode), fn).first;
    }
    *f = fit->second;
    return hipSuccess;
}

bool fast_variant_exists(int J, int mode) { return fast_kernel_exists(J, mode); }  // layout.hpp MH_FAST_KERNELS
}  // namespace

// Load the fast_search module on dev (the current device) at context setup,
// so the first search does not pay for it.
hipError_t fast_module_init(int dev) {
    hipFunction_t f;
    return fast_function(dev, 4, kModeOne, &f);
}

#ifdef MH_DEV_HOOKS
// Whether the fast code object in use on dev (MINEHIP_DEV_CODE_OBJECT, or the embedded one) is the
// coarse-hash variant (fast_search.hip, mh_fast_hash_keep): only such kernels read FastArgs::pad_.
hipError_t fast_keep_ok(int dev, bool* ok) {
    hipFunction_t f;
    *ok = false;
    const hipError_t e = fast_function(dev, 4, kModeOne, &f);  // loads the code object if need be
    if (e != hipSuccess) return e;
    const char* co = getenv("MINEHIP_DEV_CODE_OBJECT");
    std::lock_guard<std::mutex> g(g_mod_mu);
    const auto it = g_mods.find({(co && *co) ? co : "", dev});
    if (it != g_mods.end()) *ok = g_keep_ok[it->second];
    return hipSuccess;
}

// Make x the hash-XOR constant (MINEHIP_DEV_HASH_XOR; 0: off) of this library's scan kernels on dev
// (the current device) and of the fast code object in use there, if that one has the word
// (*fast_ok).  Each word is rewritten only when its value changes, by a copy on s that has
// completed on return; the caller holds the device idle.
hipError_t set_hash_xor(int dev, uint64_t x, hipStream_t s, bool* fast_ok) {
    hipFunction_t f;
    *fast_ok = false;
    hipError_t e = fast_function(dev, 4, kModeOne, &f);  // loads the code object if need be
    if (e != hipSuccess) return e;
    const char* co = getenv("MINEHIP_DEV_CODE_OBJECT");
    const uint32_t w[2] = {(uint32_t)(x >> 32), (uint32_t)x};
    std::lock_guard<std::mutex> g(g_mod_mu);
    bool wrote = false;
    if (g_xor_lib[dev] != x) {  // a new key: 0, the words' initial value
        e = hipMemcpyToSymbolAsync(HIP_SYMBOL(mh_dev_hash_xor), w, sizeof w, 0, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return e;
        wrote = true;
    }
    const auto it = g_mods.find({(co && *co) ? co : "", dev});
    hipDeviceptr_t gp = it != g_mods.end() ? g_xor_ptr[it->second] : nullptr;
    if (gp) {
        *fast_ok = true;
        if (g_xor_mod[it->second] != x) {
            e = hipMemcpyHtoDAsync(gp, (void*)w, sizeof w, s);
            if (e != hipSuccess) return e;
            wrote = true;
        }
    }
    if (wrote) {
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        g_xor_lib[dev] = x;
        if (gp) g_xor_mod[it->second] = x;
    }
    return hipSuccess;
}
#endif

// Workgroups of f that fit on dev at once (occupancy x CUs), cached per function.
hipError_t resident_groups(int dev, hipFunction_t f, unsigned lds, uint32_t* out) {
    static std::mutex mu;
    static std::map<std::pair<hipFunction_t, unsigned>, uint32_t> cache;
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find({f, lds});
    if (it == cache.end()) {
        int per_cu = 0, cus = 0;
        hipError_t e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, kBlockThreads, lds);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return e;
        }
        it = cache.emplace(std::make_pair(f, lds), (uint32_t)std::max(1, per_cu) * (uint32_t)std::max(1, cus)).first;
    }
    *out = it->second;
    return hipSuccess;
}

// a.n_chunks chunks of 256 runs; static (a.counter null): one workgroup per chunk; work queue:
// as many workgroups as fit at once (an over-estimate only queues some of them), each claiming
// chunks from a.counter (zeroed by the caller, one counter per launch).
hipError_t launch_fast(int dev, int J, int mode, const FastArgs& a, Partial* partials, hipStream_t s) {
    if (!fast_variant_exists(J, mode)) return hipErrorInvalidValue;
#ifdef MH_DEV_HOOKS
    // MINEHIP_DEV_LDS (dev build only): reserve dynamic LDS per workgroup to
    // cap occupancy, e.g. 54000 -> 3 workgroups (waves/SIMD) per CU.  Read at every launch, so
    // that one A/B process can interleave settings.
    const char* lds_env = getenv("MINEHIP_DEV_LDS");
    const unsigned lds = lds_env ? (unsigned)atoi(lds_env) : 0u;
#else
    constexpr unsigned lds = 0;
#endif
    hipFunction_t f;
    bool queue_ok = false;
    hipError_t e = fast_function(dev, J, mode, &f, &queue_ok);
    if (e != hipSuccess) return e;
    FastArgs args = a;
    if (!queue_ok) args.counter = nullptr;  // a code object without the loop: one workgroup per chunk
    uint32_t grid = args.n_chunks;
    if (args.counter) {
        uint32_t resident = 0;
        e = resident_groups(dev, f, lds, &resident);
        if (e != hipSuccess) return e;
        grid = std::min(grid, resident);
    }
    Partial* out = partials;
    void* params[] = {&args, &out};
    return hipModuleLaunchKernel(f, grid, 1, 1, kBlockThreads, 1, 1, lds, s, params, nullptr);
}

// launch_fast for the kernels of another embedded code object (loaded on dev, the current device,
// by the first call): the same grid rule, `extra` as the third kernel parameter.
namespace {
hipError_t launch_fast_variant(int dev, int J, int mode, const FastArgs& a, Partial* partials, FastVariant variant,
                               void* extra, hipStream_t s) {
    if (!fast_variant_exists(J, mode)) return hipErrorInvalidValue;
    hipFunction_t fn;
    bool queue_ok = false;
    hipError_t e = fast_function(dev, J, mode, &fn, &queue_ok, variant);
    if (e != hipSuccess) return e;
    FastArgs args = a;
    if (!queue_ok) args.counter = nullptr;
    uint32_t grid = args.n_chunks;
    if (args.counter) {
        uint32_t resident = 0;
        e = resident_groups(dev, fn, 0, &resident);
        if (e != hipSuccess) return e;
        grid = std::min(grid, resident);
    }
    Partial* out = partials;
    void* params[] = {&args, &out, extra};
    return hipModuleLaunchKernel(fn, grid, 1, 1, kBlockThreads, 1, 1, 0, s, params, nullptr);
}
}  // namespace

// mh_search_first: first_scan<J, mode> of the first-hit code object, f as the third kernel parameter.
// stop: stop_scan<J, mode> of the stopping first-hit code object instead (mh_search_first_ex,
// MH_FIRST_STOP_RUNNING), loaded on dev by the first such call.
hipError_t launch_fast_first(int dev, int J, int mode, const FastArgs& a, Partial* partials, const FirstArgs& f,
                             bool stop, hipStream_t s) {
    FirstArgs fa = f;
    return launch_fast_variant(dev, J, mode, a, partials, stop ? kFastFirstStop : kFastFirst, &fa, s);
}

// mh_search_hits: hits_scan<J, mode> of the hits code object, h as the third kernel parameter.
hipError_t launch_fast_hits(int dev, int J, int mode, const FastArgs& a, Partial* partials, const HitsArgs& h,
                            hipStream_t s) {
    HitsArgs ha = h;
    return launch_fast_variant(dev, J, mode, a, partials, kFastHits, &ha, s);
}

// mh_search_first_hits: hits_stop<J, mode> of the stopping hits code object (loaded on dev by the
// first such call), h as the third kernel parameter.
hipError_t launch_fast_hits_stop(int dev, int J, int mode, const FastArgs& a, Partial* partials, const HitsStopArgs& h,
                                 hipStream_t s) {
    HitsStopArgs ha = h;
    return launch_fast_variant(dev, J, mode, a, partials, kFastHitsStop, &ha, s);
}

hipError_t launch_generic_scan_hits_stop(const GenArgs& a, Partial* partials, uint32_t blocks, const HitsStopArgs& h,
                                         hipStream_t s) {
    hipLaunchKernelGGL(generic_scan_hits_stop, dim3(blocks), dim3(kBlockThreads), 0, s, a, partials, h);
    return hipGetLastError();
}

hipError_t launch_generic_scan_hits(const GenArgs& a, Partial* partials, uint32_t blocks, const HitsArgs& h,
                                    hipStream_t s) {
    hipLaunchKernelGGL(generic_scan_hits, dim3(blocks), dim3(kBlockThreads), 0, s, a, partials, h);
    return hipGetLastError();
}

hipError_t launch_generic_scan_first(const GenArgs& a, Partial* partials, uint32_t blocks, const FirstArgs& f,
                                     hipStream_t s) {
    hipLaunchKernelGGL(generic_scan_first, dim3(blocks), dim3(kBlockThreads), 0, s, a, partials, f);
    return hipGetLastError();
}

hipError_t launch_finish_first(const GenArgs& a, const Partial* best, const unsigned long long* scanned, uint64_t* out,
                               hipStream_t s) {
    hipLaunchKernelGGL(finish_first, dim3(1), dim3(1), 0, s, a, best, scanned, out);
    return hipGetLastError();
}

hipError_t launch_generic_scan(const GenArgs& a, Partial* partials, uint32_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(generic_scan, dim3(blocks), dim3(kBlockThreads), 0, s, a, partials);
    return hipGetLastError();
}

hipError_t launch_hash_batch(const GenArgs& a, const uint64_t* d_nonces, uint64_t* d_out, uint64_t n,
                             hipStream_t s) {
    const uint64_t blocks = (n + kBlockThreads - 1) / kBlockThreads;
    hipLaunchKernelGGL(hash_batch, dim3((uint32_t)blocks), dim3(kBlockThreads), 0, s, a, d_nonces, d_out, n);
    return hipGetLastError();
}

// One pass of a batch: tiles workgroups of batch_scan, then requests workgroups of merge_segments
// (the caller has checked the tables, minehip.cpp run_pass).
hipError_t launch_batch_scan(const BatchEntry* entries, const uint32_t* tile_entry, Partial* partials, uint32_t tiles,
                             hipStream_t s) {
    hipLaunchKernelGGL(batch_scan, dim3(tiles), dim3(kBlockThreads), 0, s, entries, tile_entry, partials);
    return hipGetLastError();
}

// The generic entries of a pass that also holds fast pieces: batch_scan_slots.
hipError_t launch_batch_scan_slots(const BatchEntry* entries, const uint32_t* tile_entry, Partial* partials,
                                   uint32_t tiles, hipStream_t s) {
    hipLaunchKernelGGL(batch_scan_slots, dim3(tiles), dim3(kBlockThreads), 0, s, entries, tile_entry, partials);
    return hipGetLastError();
}

// One launch of batch_fast<J, mode> of the batch code object (loaded on dev, the current device, by
// the first call): one workgroup per chunk, chunk_item[b] the item of chunk b (the caller has
// checked the tables, minehip.cpp batch_run_pass_ex).  A code object without the table marker at
// this library's sizeof(BatchFastItem) is refused.
hipError_t launch_batch_fast(int dev, int J, int mode, const BatchFastItem* items, const uint32_t* chunk_item,
                             Partial* partials, uint32_t chunks, hipStream_t s) {
    if (!fast_variant_exists(J, mode) || chunks == 0 || chunks > kMaxBlocksPerLaunch) return hipErrorInvalidValue;
    hipFunction_t fn;
    bool marked = false;
    const hipError_t e = fast_function(dev, J, mode, &fn, &marked, kFastBatch);
    if (e != hipSuccess) return e;
    if (!marked) return hipErrorInvalidImage;
    void* params[] = {&items, &chunk_item, &partials};
    return hipModuleLaunchKernel(fn, chunks, 1, 1, kBlockThreads, 1, 1, 0, s, params, nullptr);
}

// One launch of batch_first<J, mode> of the first-hit batch code object (loaded on dev, the current
// device, by the first call): one workgroup per chunk, workgroup b running chunk order[b] of the
// launch, chunk_item[c] the item of chunk c (the caller has checked the tables and the order,
// minehip.cpp first_batch_run_pass_ex).  A code object without the table marker at this library's
// sizeof(BatchFirstItem) is refused.
hipError_t launch_batch_first(int dev, int J, int mode, const BatchFirstItem* items, const uint32_t* chunk_item,
                              const uint32_t* order, Partial* partials, uint32_t chunks, hipStream_t s) {
    if (!fast_variant_exists(J, mode) || chunks == 0 || chunks > kMaxBlocksPerLaunch) return hipErrorInvalidValue;
    hipFunction_t fn;
    bool marked = false;
    const hipError_t e = fast_function(dev, J, mode, &fn, &marked, kFastBatchFirst);
    if (e != hipSuccess) return e;
    if (!marked) return hipErrorInvalidImage;
    void* params[] = {&items, &chunk_item, &order, &partials};
    return hipModuleLaunchKernel(fn, chunks, 1, 1, kBlockThreads, 1, 1, 0, s, params, nullptr);
}

// launch_batch_first with batch_stop<J, mode> of the stopping first-hit batch code object (loaded on
// dev, the current device, by the first call) in batch_first's place: the same tables, order and grid
// (mh_search_first_batch_stop).  A code object without its marker at sizeof(BatchFirstItem) is refused.
hipError_t launch_batch_stop(int dev, int J, int mode, const BatchFirstItem* items, const uint32_t* chunk_item,
                             const uint32_t* order, Partial* partials, uint32_t chunks, hipStream_t s) {
    if (!fast_variant_exists(J, mode) || chunks == 0 || chunks > kMaxBlocksPerLaunch) return hipErrorInvalidValue;
    hipFunction_t fn;
    bool marked = false;
    const hipError_t e = fast_function(dev, J, mode, &fn, &marked, kFastBatchStop);
    if (e != hipSuccess) return e;
    if (!marked) return hipErrorInvalidImage;
    void* params[] = {&items, &chunk_item, &order, &partials};
    return hipModuleLaunchKernel(fn, chunks, 1, 1, kBlockThreads, 1, 1, 0, s, params, nullptr);
}

// One launch of batch_hits<J, mode> of the hits batch code object (loaded on dev, the current device,
// by the first call): one workgroup per chunk, chunk_item[b] the item of chunk b (the caller has
// checked the tables and the regions, minehip.cpp hits_batch_run_pass_ex).  A code object without
// the table marker at this library's sizeof(BatchHitsItem) is refused.
hipError_t launch_batch_hits(int dev, int J, int mode, const BatchHitsItem* items, const uint32_t* chunk_item,
                             Partial* partials, uint32_t chunks, hipStream_t s) {
    if (!fast_variant_exists(J, mode) || chunks == 0 || chunks > kMaxBlocksPerLaunch) return hipErrorInvalidValue;
    hipFunction_t fn;
    bool marked = false;
    const hipError_t e = fast_function(dev, J, mode, &fn, &marked, kFastBatchHits);
    if (e != hipSuccess) return e;
    if (!marked) return hipErrorInvalidImage;
    void* params[] = {&items, &chunk_item, &partials};
    return hipModuleLaunchKernel(fn, chunks, 1, 1, kBlockThreads, 1, 1, 0, s, params, nullptr);
}

// launch_batch_first with batch_bound<J, mode> of the first-k-hits batch code object (loaded on dev,
// the current device, by the first call) over BatchBoundItems: the same per-chunk table, order and
// grid (the caller has checked the tables, the regions and the items' words, minehip.cpp
// first_hits_batch_run_pass).  A code object without its marker at sizeof(BatchBoundItem) is refused.
hipError_t launch_batch_bound(int dev, int J, int mode, const BatchBoundItem* items, const uint32_t* chunk_item,
                              const uint32_t* order, Partial* partials, uint32_t chunks, hipStream_t s) {
    if (!fast_variant_exists(J, mode) || chunks == 0 || chunks > kMaxBlocksPerLaunch) return hipErrorInvalidValue;
    hipFunction_t fn;
    bool marked = false;
    const hipError_t e = fast_function(dev, J, mode, &fn, &marked, kFastBatchBound);
    if (e != hipSuccess) return e;
    if (!marked) return hipErrorInvalidImage;
    void* params[] = {&items, &chunk_item, &order, &partials};
    return hipModuleLaunchKernel(fn, chunks, 1, 1, kBlockThreads, 1, 1, 0, s, params, nullptr);
}

#ifdef MH_DEV_HOOKS
// The hooks of the batch code object in use on dev (the current device; loaded if need be): whether
// its kernels mask hashes by FastArgs::pad_ (*keep_ok), and x made its hash-XOR constant if it has
// the word (*xor_ok), by a copy on s that has completed on return; the caller holds the device idle.
hipError_t batch_fast_hooks(int dev, uint64_t x, hipStream_t s, bool* keep_ok, bool* xor_ok) {
    hipFunction_t f;
    *keep_ok = *xor_ok = false;
    hipError_t e = fast_function(dev, 4, kModeOne, &f, nullptr, kFastBatch);
    if (e != hipSuccess) return e;
    const uint32_t w[2] = {(uint32_t)(x >> 32), (uint32_t)x};
    std::lock_guard<std::mutex> g(g_mod_mu);
    const auto it = g_mods.find({batch_module_path(), dev});
    if (it == g_mods.end()) return hipSuccess;
    *keep_ok = g_keep_ok[it->second];
    hipDeviceptr_t gp = g_xor_ptr[it->second];
    if (!gp) return hipSuccess;
    *xor_ok = true;
    if (g_xor_mod[it->second] != x) {
        e = hipMemcpyHtoDAsync(gp, (void*)w, sizeof w, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        g_xor_mod[it->second] = x;
    }
    return hipSuccess;
}
#endif

hipError_t launch_merge_segments(const Partial* partials, const uint32_t* seg, Partial* results, uint32_t requests,
                                 hipStream_t s) {
    hipLaunchKernelGGL(merge_segments, dim3(requests), dim3(kBlockThreads), 0, s, partials, seg, results);
    return hipGetLastError();
}

// One pass of a first-hit batch: tiles workgroups of batch_scan_first, then requests workgroups of
// merge_segments_first (the caller has checked the tables and the order, minehip.cpp first_batch_run_pass).
hipError_t launch_batch_scan_first(const BatchEntry* entries, const uint32_t* tile_entry, const uint32_t* entry_req,
                                   const uint32_t* order, BatchFirstWords* words, Partial* partials, uint32_t tiles,
                                   hipStream_t s) {
    hipLaunchKernelGGL(batch_scan_first, dim3(tiles), dim3(kBlockThreads), 0, s, entries, tile_entry, entry_req, order,
                       words, partials);
    return hipGetLastError();
}

hipError_t launch_merge_segments_first(const Partial* partials, const uint32_t* seg, const BatchEntry* entries,
                                       const uint32_t* tile_entry, const BatchFirstWords* words,
                                       BatchFirstResult* results, uint32_t requests, hipStream_t s) {
    hipLaunchKernelGGL(merge_segments_first, dim3(requests), dim3(kBlockThreads), 0, s, partials, seg, entries,
                       tile_entry, words, results);
    return hipGetLastError();
}

// The generic side of a first-hit pass that also holds fast pieces: batch_scan_first_slots and
// merge_segments_first_ex.
hipError_t launch_batch_scan_first_slots(const BatchEntry* entries, const uint32_t* tile_entry,
                                         const uint32_t* entry_req, const uint32_t* order, BatchFirstWords* words,
                                         Partial* partials, uint32_t tiles, hipStream_t s) {
    hipLaunchKernelGGL(batch_scan_first_slots, dim3(tiles), dim3(kBlockThreads), 0, s, entries, tile_entry, entry_req,
                       order, words, partials);
    return hipGetLastError();
}

hipError_t launch_merge_segments_first_ex(const Partial* partials, const uint32_t* seg, const GenArgs* req_gen,
                                          const BatchFirstWords* words, BatchFirstResult* results, uint32_t requests,
                                          hipStream_t s) {
    hipLaunchKernelGGL(merge_segments_first_ex, dim3(requests), dim3(kBlockThreads), 0, s, partials, seg, req_gen, words,
                       results);
    return hipGetLastError();
}

// One pass of a hits batch: tiles workgroups of batch_scan_hits, then requests workgroups of
// merge_segments_hits (the caller has checked the tables and the regions, minehip.cpp hits_batch_run_pass).
hipError_t launch_batch_scan_hits(const BatchEntry* entries, const uint32_t* tile_entry, const uint32_t* entry_req,
                                  BatchHitsWords* words, Hit* hits, Partial* partials, uint32_t tiles,
                                  hipStream_t s) {
    hipLaunchKernelGGL(batch_scan_hits, dim3(tiles), dim3(kBlockThreads), 0, s, entries, tile_entry, entry_req, words,
                       hits, partials);
    return hipGetLastError();
}

// The generic side of a hits pass that also holds fast pieces: batch_scan_hits_slots.
hipError_t launch_batch_scan_hits_slots(const BatchEntry* entries, const uint32_t* tile_entry, const uint32_t* entry_req,
                                        BatchHitsWords* words, Hit* hits, Partial* partials, uint32_t tiles,
                                        hipStream_t s) {
    hipLaunchKernelGGL(batch_scan_hits_slots, dim3(tiles), dim3(kBlockThreads), 0, s, entries, tile_entry, entry_req,
                       words, hits, partials);
    return hipGetLastError();
}

hipError_t launch_merge_segments_hits(const Partial* partials, const uint32_t* seg, const BatchHitsWords* words,
                                      const Hit* hits, Hit* packed, uint64_t limit, const unsigned long long* base_in,
                                      unsigned long long* base_out, BatchHitsResult* results, uint32_t requests,
                                      hipStream_t s) {
    hipLaunchKernelGGL(merge_segments_hits, dim3(requests), dim3(kBlockThreads), 0, s, partials, seg, words, hits, packed,
                       limit, base_in, base_out, results);
    return hipGetLastError();
}

// One pass of a first-k-hits batch: tiles workgroups of batch_scan_bound (slots: batch_scan_bound_slots,
// a pass that also holds fast pieces), then requests workgroups of merge_segments_bound (the caller
// has checked the tables, the order, the regions and the slices, minehip.cpp first_hits_batch_run_pass).
hipError_t launch_batch_scan_bound(bool slots, const BatchEntry* entries, const uint32_t* tile_entry,
                                   const uint32_t* entry_req, const uint32_t* order, BatchBoundWords* words,
                                   uint32_t* slices, Hit* hits, Partial* partials, uint32_t tiles, hipStream_t s) {
    if (slots)
        hipLaunchKernelGGL(batch_scan_bound_slots, dim3(tiles), dim3(kBlockThreads), 0, s, entries, tile_entry, entry_req,
                           order, words, slices, hits, partials);
    else
        hipLaunchKernelGGL(batch_scan_bound, dim3(tiles), dim3(kBlockThreads), 0, s, entries, tile_entry, entry_req, order,
                           words, slices, hits, partials);
    return hipGetLastError();
}

hipError_t launch_merge_segments_bound(const Partial* partials, const uint32_t* seg, const BatchBoundWords* words,
                                       const Hit* hits, Hit* packed, uint64_t limit, const unsigned long long* base_in,
                                       unsigned long long* base_out, BatchBoundResult* results, uint32_t requests,
                                       hipStream_t s) {
    hipLaunchKernelGGL(merge_segments_bound, dim3(requests), dim3(kBlockThreads), 0, s, partials, seg, words, hits, packed,
                       limit, base_in, base_out, results);
    return hipGetLastError();
}

hipError_t launch_merge(const Partial* partials, uint32_t n, Partial* best, hipStream_t s) {
    hipLaunchKernelGGL(merge_partials, dim3(1), dim3(kMergeThreads), 0, s, partials, n, best);
    return hipGetLastError();
}

}  // namespace mh
