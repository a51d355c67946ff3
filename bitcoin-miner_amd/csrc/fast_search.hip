// fast_search.hip -- the run kernel of libminehip, fast_search<J, MODE>.
//
// Hot path replaced: the miner's scan over bitcoin.Hash (reference
// bitcoin/hash.go:13-17, scan spec SURVEY.md §8(a) A2 / stub
// bitcoin/miner/miner.go:33).  Design: DESIGN.md §2-§4.
//
// One lane = one run of 10^L consecutive nonces that share their d-L higher
// digits; the L lower digits are enumerated in wave-uniform loops (digit
// arithmetic is SALU); only message word J (the last digit's word) changes per
// nonce, so rounds 0..J-1 and every schedule term that does not depend on W[J]
// are hoisted out of the per-nonce loop.
//
// Build (Makefile): this file is compiled to gfx950 assembly only, run through
// the issue-priority pass (issue_prio.py: s_setprio 3 before every run of
// half-rate VALU ops, 0 before every run of full-rate ones),
// assembled into a code object and embedded in libminehip.so (fast_co.S),
// which loads it per device (search_kernels.hip, fast_module).  It is never
// part of the library's fat binary.  -DMH_HASH_KEEP builds the coarse-hash test variant
// (build/fast_search_keep.hsaco, through the same passes), which only the dev
// build's MINEHIP_DEV_CODE_OBJECT hook ever loads.  -DMH_FIRST builds the first-hit kernels
// first_scan<J, MODE> (build/fast_first.hsaco, through the same passes), embedded as a
// second code object that mh_search_first loads; without it nothing below differs from before.
// -DMH_HITS builds the hits kernels hits_scan<J, MODE> (build/fast_hits.hsaco, through the same
// passes), a third embedded code object that mh_search_hits loads; likewise.
// -DMH_BATCH builds batch_fast<J, MODE> (build/fast_batch.hsaco, through the same passes; DESIGN.md
// §3): the same chunk body, one workgroup per chunk of a table of many requests' pieces, a fourth
// embedded code object that mh_search_batch_ex loads; likewise (with -DMH_HASH_KEEP: its test variant).
// -DMH_BATCH -DMH_FIRST builds batch_first<J, MODE> (build/fast_batch_first.hsaco, through the same
// passes): batch_fast's table and grid around the first-hit chunk body, a fifth
// embedded code object that mh_search_first_batch_ex loads; likewise.
// -DMH_BATCH -DMH_HITS builds batch_hits<J, MODE> (build/fast_batch_hits.hsaco, through the same
// passes): batch_fast's table and grid around the hits chunk body, a sixth embedded
// code object that mh_search_hits_batch_ex loads; likewise.
// -DMH_FIRST -DMH_STOP builds stop_scan<J, MODE> (build/fast_first_stop.hsaco, through the same
// passes): first_scan whose waves publish a hit when they find it and leave a running
// chunk once it lies wholly above a published hit, a seventh embedded code object that
// mh_search_first_ex(MH_FIRST_STOP_RUNNING) loads; likewise (everything of it sits under MH_STOP).
// -DMH_BATCH -DMH_FIRST -DMH_STOP builds batch_stop<J, MODE> (build/fast_batch_first_stop.hsaco, through
// the same passes): batch_first's table, order and grid around stop_scan's chunk body,
// which polls its request's word through the item, an eighth embedded code object that
// mh_search_first_batch_stop loads; likewise (everything of it sits under MH_STOP).
// -DMH_HITS -DMH_STOP builds hits_stop<J, MODE> (build/fast_hits_stop.hsaco, through the same passes;
// DESIGN.md §3): hits_scan whose hits also count in slices of the range, whose waves publish a bound
// once the slices hold k hits and leave a running chunk that lies wholly above it, a ninth embedded
// code object that mh_search_first_hits loads; likewise (everything of it sits under MH_HITS and MH_STOP).
// -DMH_BATCH -DMH_HITS -DMH_STOP builds batch_bound<J, MODE> (build/fast_batch_bound.hsaco, through the
// same passes): batch_first's table, order and grid around that stopping hits chunk body,
// which reaches its request's words through the item, a tenth embedded code object that
// mh_search_first_hits_batch loads; likewise (everything of it sits under MH_HITS and MH_STOP).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_common.hpp"
#include "layout.hpp"
#include "sha256_gfx950.hpp"

// Minimum waves per SIMD each fast_search<J, MODE> is compiled for (its register budget): the
// occupancy the layout reaches as a one-chunk-per-workgroup kernel (VGPRs 59..79 -> 7 or 6 waves,
// the Two layouts 98..110 -> 4).  The work-queue loop around the chunk body would otherwise let
// the allocator take 4..6 more VGPRs and cost a wave per SIMD.  -DMH_MIN_WAVES=n overrides all.
// The Early modes (layout.hpp) of the one-block and Pre layouts take 7 (72 VGPRs, spills outside
// the per-nonce loop only): against their layouts' 6, +0.1% to +1.1% on the three buckets of the
// round-5 A/B (profiles/r05d_kbench_early_waves_*.json); TwoEarly keeps Two's 4 (at 6 or 7 it
// spills 56-120 B).  -DMH_EARLY_WAVES=n overrides the One/Pre Early kernels' budget.
// -DMH_ONEPRE_WAVES=n (A/B builds, tools/co_variants.py) sets every One/Pre kernel's budget.
#ifndef MH_EARLY_WAVES
#define MH_EARLY_WAVES 7
#endif
#ifndef MH_ONEPRE_WAVES
#define MH_ONEPRE_WAVES 0
#endif
constexpr int min_waves(int J, int MODE) {
#ifdef MH_MIN_WAVES
    return MH_MIN_WAVES;
#else
#ifdef MH_BATCH
#ifdef MH_HITS
#ifdef MH_STOP
    // batch_bound<0, OneEarly>: hits_stop's kernel of the layout takes 64 VGPRs, 8 waves; left at the
    // Early budget of 7 this build took 65
    if (J == 0 && MODE == 3 && !MH_ONEPRE_WAVES) return 8;
#endif
#endif
#endif
    return (MH_ONEPRE_WAVES && MODE % 3 != 2) ? MH_ONEPRE_WAVES
         : (MODE == 3 || MODE == 4) ? MH_EARLY_WAVES
         : MODE % 3 == 2 ? 4
         : MODE % 3 == 1 ? ((J == 0 || J == 4) ? 6 : 7)
                         : ((J == 7 || J == 8 || J >= 10) ? 6 : 7);
#endif
}

namespace mh {

// ---------------------------------------------------------------------------
// fast_search<J, MODE>
// ---------------------------------------------------------------------------
// Inside a lane only message word J (the last digit's word; Early modes: the
// word the innermost digit ends) changes from one nonce to the next, and word
// J-1 (Early: J+1) changes once per group of 10 nonces.  Every
// schedule word W[t] therefore lives at one of three levels, fixed at compile
// time by J:
//   nonce  depends on W[J]                    -> computed per nonce
//   group  depends on W[J-1] (Early: W[J+1]) but not on W[J] -> once per 10 nonces
//   run    neither                            -> once per lane (10^L nonces)
// and each per-nonce / per-group word is split into its cheaper-level partial
// sum plus the terms of its own level.  Words after J hold only padding and
// length, so they come from the kernel arguments (SGPRs), never VGPRs.
// The hoisting is explicit: left to LICM it does not happen, because SROA
// turns the message array into a loop-carried vector.
struct Dep {
    static constexpr uint64_t from(int j) {  // words whose value depends on word j
        if (j < 0) return 0;
        uint64_t m = 1ull << j;
        for (int t = 16; t < 64; ++t)
            if (((m >> (t - 2)) | (m >> (t - 7)) | (m >> (t - 15)) | (m >> (t - 16))) & 1ull) m |= 1ull << t;
        return m;
    }
};

// sigma0/sigma1 of the last digit's contribution inc = i << 8k (i = 0..9,
// k = byte slot).  The last digit's byte of word J is '0' before the digit
// is added and 0x30 + i never carries, so W[J] = wJ ^ inc and, sigma being
// GF(2)-linear, sigma(W[J]) = sigma(wJ) ^ sigma(inc): one VALU xor per nonce
// with a scalar (SMEM) operand instead of four VALU ops.
struct IncSigma {
    uint32_t s0[4][10], s1[4][10];
};
constexpr uint32_t crotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
constexpr IncSigma make_inc_sigma() {
    IncSigma t{};
    for (int k = 0; k < 4; ++k)
        for (uint32_t i = 0; i < 10; ++i) {
            const uint32_t x = i << (8 * k);
            t.s0[k][i] = crotr(x, 7) ^ crotr(x, 18) ^ (x >> 3);
            t.s1[k][i] = crotr(x, 17) ^ crotr(x, 19) ^ (x >> 10);
        }
    return t;
}
static __constant__ IncSigma kIncSigma = make_inc_sigma();  // static: one copy per translation unit

namespace dev {
// Last round of a compression when only H0 = st0 + a64 is needed:
// kw_st0 = K[63] + W[63] + st0.  Seven terms, three add3.
__device__ __forceinline__ uint32_t last_round_h0(uint32_t a, uint32_t b, uint32_t c, uint32_t e, uint32_t f,
                                                  uint32_t g, uint32_t h, uint32_t kw_st0) {
    return ((h + kw_st0) + bsig1(e) + ch(e, f, g)) + (bsig0(a) + maj(a, b, c));
}

// Block whose schedule is host-known (kw[i] = K[i] + W[i]): H0 and a63.
__device__ __forceinline__ void sha256_block_kw_last(const uint32_t st[8], const uint32_t* kw, uint32_t& h0,
                                                     uint32_t& a63);

// One round; kw = K[t] + W[t].  (h + kw) first, so it folds into a single
// hoisted value whenever both are invariant.
__device__ __forceinline__ void round_kw(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t& e,
                                         uint32_t& f, uint32_t& g, uint32_t& h, uint32_t kw) {
    const uint32_t t1 = (h + kw) + bsig1(e) + ch(e, f, g);
    const uint32_t t2 = bsig0(a) + maj(a, b, c);
    h = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + t2;
}

__device__ __forceinline__ void sha256_block_kw_last(const uint32_t st[8], const uint32_t* kw, uint32_t& h0,
                                                     uint32_t& a63) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 63; ++i) round_kw(a, b, c, d, e, f, g, h, kw[i]);
    a63 = a;
    h0 = last_round_h0(a, b, c, e, f, g, h, kw[63] + st[0]);
}
}  // namespace dev

// spread(x, k, w) = x with w zero decimal digits inserted at digit index k (k >= 20: x itself),
// by divisions by the constant 10 (no general 64-bit division); on the rare new-best branch of
// the Early modes only
__device__ __forceinline__ uint64_t spread(uint64_t x, uint32_t k, uint32_t w) {
    if (k >= 20u) return x;
    uint64_t lo = 0, p = 1;
    for (uint32_t j = 0; j < k; ++j) {
        const uint64_t q = x / 10u;
        lo += (x - q * 10u) * p;
        p *= 10u;
        x = q;
    }
    for (uint32_t j = 0; j < w; ++j) p *= 10u;
    return x * p + lo;
}

#ifdef MH_HASH_KEEP
// Hash-XOR word of the test variant (MINEHIP_DEV_HASH_XOR, layout.hpp): {high, low} 32 bits of the
// constant every nonce's (H0, H1) is XORed with before the keep mask; zero (off) unless the dev
// build writes it before a search (search_kernels.hip, set_hash_xor).  Its presence also marks the
// code object as one whose kernels apply it.
extern "C" {
__device__ __attribute__((used)) uint32_t mh_dev_hash_xor[2];
}
#endif

// One workgroup-sized chunk: the 256 runs u_start + 256 * blk + threadIdx.x, their minimum
// written to partials[blk].
// MODE % 3 is the tail layout (One, Pre, Two); MODE >= 3 (Early): the per-nonce digit ends word
// J and the group digits sit right before it in word J, so no word but J changes inside a run:
// rounds 0..J-1 and every schedule word that does not depend on W[J] are run-level; otherwise
// the per-nonce digit is the last one (word J) and the group digits lie in words J - 1 and J.
#ifdef MH_FIRST
// The parameters of first_scan<J, MODE> (below) as the kernarg segment holds them.
struct FirstKernArgs {
    FastArgs a;
    Partial* partials;
    FirstArgs f;
};
// The first-hit parameters of the kernel whose FastArgs `a` is: they follow it in the kernarg
// segment, so the chunk body reads them through the pointer it already holds (the rare candidate
// branch and the chunk's end only).
__device__ __forceinline__ const FirstArgs& first_args(const FastArgs& a) {
    return ((const FirstKernArgs*)&a)->f;
}
#ifdef MH_STOP
template <int MODE>
__device__ __forceinline__ uint64_t chunk_floor(const FastArgs& a, uint32_t blk);  // below, beside claim_first
#endif
#endif
#ifdef MH_HITS
// The parameters of hits_scan<J, MODE> (below) as the kernarg segment holds them.
struct HitsKernArgs {
    FastArgs a;
    Partial* partials;
    HitsArgs h;
};
// The hits parameters of the kernel whose FastArgs `a` is: they follow it in the kernarg segment,
// so the chunk body reads them through the pointer it already holds.
__device__ __forceinline__ const HitsArgs& hits_args(const FastArgs& a) {
    return ((const HitsKernArgs*)&a)->h;
}
#ifdef MH_STOP
// The parameters of hits_stop<J, MODE> (below) as the kernarg segment holds them: HitsStopArgs
// begins with a HitsArgs, so hits_args serves this build unchanged.
struct HitsStopKernArgs {
    FastArgs a;
    Partial* partials;
    HitsStopArgs h;
};
static_assert(__builtin_offsetof(HitsStopKernArgs, h.h) == __builtin_offsetof(HitsKernArgs, h),
              "hits_args finds the HitsArgs that HitsStopArgs begins with");
__device__ __forceinline__ const HitsStopArgs& hits_stop_args(const FastArgs& a) {
    return ((const HitsStopKernArgs*)&a)->h;
}
// No nonce of chunk blk is smaller: lane 0's first, attained, so exact (the first-hit builds'
// floor: last-digit layouts U * 10^L, Early layouts spread(U) * u_mul, spread strictly increasing).
template <int MODE>
__device__ __forceinline__ uint64_t hits_floor(const FastArgs& a, uint32_t blk) {
    const uint64_t u0 = a.u_start + (uint64_t)blk * kBlockThreads;
    if constexpr (MODE < (int)kModeOneEarly)
        return u0 * a.pow10L;
    else
        return spread(u0, a.hole, a.hole_w) * a.u_mul;
}
#endif
#endif
template <int J, int MODE>
__device__ __forceinline__ void fast_chunk(const FastArgs& a, Partial* __restrict__ partials, const uint32_t blk) {
    using namespace dev;
    constexpr uint32_t K[64] = MH_K256;
    constexpr int BM = MODE % 3;                          // tail layout
    constexpr bool EARLY = MODE >= 3;
    constexpr int JG = EARLY ? J : J - 1;                 // the other word of the group digits
    constexpr uint64_t NM = Dep::from(J);                 // nonce-level words
    constexpr uint64_t GM = Dep::from(JG) & ~NM;          // group-level words (Early: none)
    constexpr int BASE = (BM == kModePre) ? 16 : 0;       // per-nonce block inside the tail
#define MH_N(t) ((NM >> (t)) & 1ull)
#define MH_G(t) ((GM >> (t)) & 1ull)
#define MH_R(t) (!MH_N(t) && !MH_G(t))
    const uint32_t gid = blk * kBlockThreads + threadIdx.x;
    const uint64_t U = a.u_start + gid;

    // ---- per run --------------------------------------------------------
    // Tail words: host template + the d-L digits of U, right-aligned so U's
    // last digit sits at tail byte hi_end-1 (Early: skipping the L enumerated
    // digits' bytes).  Only words up to the last digit's can receive them
    // (words <= BASE + J, Early BASE + J + 1).
    constexpr int JM = EARLY ? J + 1 : J;                 // the last per-lane word
    constexpr int NW = BASE + JM + 1;
    uint32_t w[NW];
#pragma unroll
    for (int x = 0; x < NW; ++x) w[x] = a.blk[x];
    {
        uint64_t u = U;
#pragma unroll
        for (int k = 0; k < 20; ++k) {
            if ((uint32_t)k < a.n_hi) {
                const uint64_t q = u / 10u;
                const uint32_t dg = (uint32_t)(u - q * 10u);
                u = q;
                uint32_t pos = a.hi_end - 1u - (uint32_t)k;
                if constexpr (EARLY) pos -= ((uint32_t)k >= a.hole) ? a.hole_w : 0u;
                add_word(w, pos >> 2, dg << (24u - 8u * (pos & 3u)));
            }
        }
    }
    // words of the per-nonce block: per-lane up to JM, uniform (SGPR) after it
    uint32_t W[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) W[t] = (t <= JM) ? w[BASE + t] : a.blk[BASE + t];

    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) st[i] = a.mid[i];
    if constexpr (BM == kModePre) {
        uint32_t b0[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) b0[t] = w[t];
        sha256_block(st, b0);  // tail block 0 holds no lower digit: once per run
    }
    // rounds 0..J-2 (Early: 0..J-1) read only run-level words
    uint32_t ra = st[0], rb = st[1], rc = st[2], rd = st[3], re = st[4], rf = st[5], rg = st[6], rh = st[7];
#pragma unroll
    for (int t = 0; t < (EARLY ? J : J - 1); ++t) round_kw(ra, rb, rc, rd, re, rf, rg, rh, K[t] + W[t]);

    // run-level schedule words, and the run-level part of the others
    uint32_t wr[64], pr[64];
#pragma unroll
    for (int t = 0; t < 16; ++t) wr[t] = W[t];
#pragma unroll
    for (int t = 16; t < 64; ++t) {
        uint32_t v = 0u;
        if (MH_R(t - 16)) v += wr[t - 16];
        if (MH_R(t - 7)) v += wr[t - 7];
        if (MH_R(t - 15)) v += ssig0(wr[t - 15]);
        if (MH_R(t - 2)) v += ssig1(wr[t - 2]);
        if (MH_R(t)) wr[t] = v; else pr[t] = v;
    }
    // K[t] + W[t] of the run-level words the per-nonce rounds read, made
    // opaque so the register allocator keeps the sums instead of redoing the
    // add on every nonce (it did, for t = 16..18, once the lane's best moved
    // to SGPRs and freed VGPRs).
    uint32_t kwr[64];
#pragma unroll
    for (int t = 16; t < 64; ++t)
        if (MH_R(t) && t > J) {
            kwr[t] = K[t] + wr[t];
            asm volatile("" : "+v"(kwr[t]));
        }

    // byte of the per-nonce digit, in word J: the last digit, or (Early) the innermost one
    const uint32_t lastpos = EARLY ? a.inner : a.lo_pos + a.L - 1u;
    const uint32_t sh_last = 24u - 8u * (lastpos & 3u);
    // The best (H0, H1, nonce) of the whole wave so far, wave-uniform (SGPRs).
    // A lane is a candidate when its H0 <= the wave's best H0: the compare is
    // already a lane mask, and the scan over its set bits is scalar work.
    // Per wave, the candidate branch is taken ~ln(steps) times per run; per
    // lane it was taken whenever any of 64 lanes improved its own minimum,
    // ~64 + 64 ln(steps / 64) times, i.e. on ~93% of the steps of a 100-nonce
    // run.  Invalid lanes (gid >= n_runs) never become candidates.
    const uint64_t valid_mask = __builtin_amdgcn_ballot_w64(gid < a.n_runs);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t wave_u0 = a.u_start + (uint64_t)blk * kBlockThreads + wave * 64u;
    uint32_t wbh0 = 0xFFFFFFFFu, wbh1 = 0xFFFFFFFFu;
    uint64_t wbn = ~0ull;
#ifdef MH_FIRST
    // First-hit variant: the wave's best is a key (k0, k1) -- (0, 0) for a nonce whose hash is <=
    // the target (a hit), else the hash -- and a lane is a candidate when its H0 <= lim =
    // max(k0, target >> 32): without a hit so far that admits what the product admits and every
    // possible hit, after one (k0 = 0) only possible hits.  The loop carries lim in wbh0's place,
    // not beside it (one more SGPR across the per-nonce loop costs the loop VALU instructions: the
    // compiler then stops hoisting K[t] + W[t] sums out of it), and the rare branch rebuilds k0
    // from it.  With thi = target >> 32: a key that is a hash has k0 >= thi (it is > target), so
    // without a hit lim = k0; with one, lim = thi and k1 = 0 -- and no hash-key has k0 = thi and
    // k1 = 0, since that is <= target.  Hence  hit <=> (lim == thi and k1 == 0),  k0 = hit ? 0 : lim.
    // Below, wbh0 is lim outside the rare branch and k0 inside it; wbh1 is k1.
#endif
#ifdef MH_HASH_KEEP
    // coarse-hash variant (build/fast_search_keep.hsaco, layout.hpp keep_word): the bits of H0 and
    // H1 that enter the comparisons below; the comparisons themselves are the product's
    const uint32_t keep0 = keep_mask0(a.pad_), keep1 = keep_mask1(a.pad_);
    const uint32_t xor0 = mh_dev_hash_xor[0], xor1 = mh_dev_hash_xor[1];  // the hash-XOR hook, before the mask
#endif

#ifdef MH_STOP
    uint32_t g = 0;  // after the loop: the groups this wave hashed
    for (; g < a.n_groups; ++g) {
#else
    for (uint32_t g = 0; g < a.n_groups; ++g) {
#endif
        // ---- per group of 10 nonces --------------------------------------
#ifdef MH_FIRST
#ifdef MH_STOP
        // One poll of the search's word per group, outside the per-nonce loop: once every nonce of
        // this chunk lies above a published hit (chunk_floor, attained, so exact) the wave leaves
        // the loop for the chunk's end -- block_min, its barriers and the chunk's Partial, which then
        // carries a key that loses to the published hit's in every merge.  The word
        // is written by other workgroups' atomics, so it is read as claim_first reads it: a relaxed
        // agent-scope load (a vector load past this CU's L1, never the scalar cache), made
        // wave-uniform.  A poll, never a wait: a stale value only stops later.  The kernel's
        // arguments come through a pointer laundered here, so neither the word's address nor the
        // floor is held across the per-nonce loop.
        {
            using KStop = __attribute__((address_space(4))) const FirstKernArgs;
#ifdef MH_BATCH
            // batch_stop: the kernarg segment holds the launch's four table pointers, so the word's
            // address and the floor's terms come from the item `a` heads (layout.hpp BatchFirstItem:
            // FastArgs and FirstArgs where FirstKernArgs has them), through a copy of the item's
            // address laundered here for the same reason.  The word and the floor are this request's
            // and this piece's.
            KStop* ks = (KStop*)&a;
#else
            KStop* ks = (KStop*)__builtin_amdgcn_kernarg_segment_ptr();
#endif
            asm volatile("" : "+s"(ks));
            const FirstKernArgs& sk = *(const FirstKernArgs*)ks;
            const uint64_t seen = __hip_atomic_load(sk.f.first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(seen >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)seen);
            if (chunk_floor<MODE>(sk.a, blk) > word) break;
        }
#endif
#endif
#ifdef MH_HITS
#ifdef MH_STOP
        // hits_stop: the same poll, of the search's bound word (layout.hpp HitsStopArgs): at least k
        // hits of the range are <= its value, so once every nonce of this chunk lies above it
        // (hits_floor, attained, so exact) none of them is among the k smallest hits, and the wave
        // leaves the loop for the chunk's end -- block_min, its barriers and the chunk's Partial,
        // which the host then does not use.  Read as stop_scan reads its word: a
        // relaxed agent-scope load (a vector load past this CU's L1, never the scalar cache), made
        // wave-uniform, through a kernarg pointer laundered here so that neither the word's address
        // nor the floor is held across the per-nonce loop.  A poll, never a wait.
        {
            using KHStop = __attribute__((address_space(4))) const HitsStopKernArgs;
#ifdef MH_BATCH
            // batch_bound: the kernarg segment holds the launch's four table pointers, so the word's
            // address and the floor's terms come from the item `a` heads (layout.hpp BatchBoundItem:
            // FastArgs and HitsStopArgs where HitsStopKernArgs has them), through a copy of the item's
            // address laundered here for the same reason.  The word and the floor are this request's
            // and this piece's.
            KHStop* kb = (KHStop*)&a;
#else
            KHStop* kb = (KHStop*)__builtin_amdgcn_kernarg_segment_ptr();
#endif
            asm volatile("" : "+s"(kb));
            const HitsStopKernArgs& bk = *(const HitsStopKernArgs*)kb;
            const uint64_t seen = __hip_atomic_load(bk.h.bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(seen >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)seen);
            if (hits_floor<MODE>(bk.a, blk) > word) break;
        }
#endif
#endif
        // the L-1 digits of g: wave-uniform, so this is SALU work.  Into word J (cj) or word
        // J - 1 (cjm; the Early layouts put every group digit in word J)
        uint32_t cj = 0u, cjm = 0u, gq = g;
        if constexpr (!EARLY) {
            // digits 0..L-2 of q = 10*g + i, at bytes lo_pos .. lo_pos+L-2
            for (uint32_t k = a.L - 1u; k-- > 0u;) {
                const uint32_t q = gq / 10u;
                const uint32_t dg = gq - q * 10u;
                gq = q;
                const uint32_t p = a.lo_pos + k;
                const uint32_t v = dg << (24u - 8u * (p & 3u));
                if ((p >> 2) == (uint32_t)J)
                    cj += v;
                else
                    cjm += v;
            }
        } else {
            // g's digit j (least significant first) at byte g_last - j, one more to the left
            // from j = g_hole on (the innermost digit's decimal place); every one in word J
            // (make_fast_args builds only such pieces, enqueue_piece re-checks each one)
            for (uint32_t j = 0; j + 1u < a.L; ++j) {
                const uint32_t q = gq / 10u;
                const uint32_t dg = gq - q * 10u;
                gq = q;
                const uint32_t p = a.g_last - j - (j >= a.g_hole ? 1u : 0u);
                cj += dg << (24u - 8u * (p & 3u));
            }
        }
        const uint32_t wJ = W[J] + cj;  // word J with this group's digits, the per-nonce digit '0'
        const uint32_t s0wJ = ssig0(wJ), s1wJ = ssig1(wJ);
        uint32_t wg[64], pg[64];
        if constexpr (!EARLY && J > 0) wg[J - 1] = W[J - 1] + cjm;
#pragma unroll
        for (int t = 16; t < 64; ++t) {
            if (MH_R(t)) continue;
            uint32_t v = pr[t];
            if (MH_G(t - 16)) v += wg[t - 16];
            if (MH_G(t - 7)) v += wg[t - 7];
            if (MH_G(t - 15)) v += ssig0(wg[t - 15]);
            if (MH_G(t - 2)) v += ssig1(wg[t - 2]);
            if (MH_G(t)) wg[t] = v; else pg[t] = v;
        }
#ifdef MH_STOP
#ifdef MH_BATCH
        // batch_stop: K[t] + W[t] of the group-level words the per-nonce rounds read, made opaque as
        // kwr is.  Left to the compiler, the build with a store inside the group loop (the published
        // hit) redoes one or two of these adds on every nonce in eight layouts, which batch_first's
        // loops take hoisted.
        uint32_t kwg[64];
#pragma unroll
        for (int t = 16; t < (BM == kModeTwo ? 64 : 63); ++t)
            if (MH_G(t) && t > J) {
                kwg[t] = K[t] + wg[t];
                asm volatile("" : "+v"(kwg[t]));
            }
#endif
#ifdef MH_HITS
#ifndef MH_BATCH
        // hits_stop: likewise (its group loop holds the poll's break; left to the compiler, ten
        // One and Pre layouts redo one to four of these adds on every nonce; with MH_BATCH the
        // block above has made them)
        uint32_t kwg[64];
#pragma unroll
        for (int t = 16; t < (BM == kModeTwo ? 64 : 63); ++t)
            if (MH_G(t) && t > J) {
                kwg[t] = K[t] + wg[t];
                asm volatile("" : "+v"(kwg[t]));
            }
#endif
#endif
#endif
        // round J-1 reads the group-level word J-1 (Early: it is run-level, done above)
        uint32_t ga = ra, gb = rb, gc = rc, gd = rd, ge = re, gf = rf, gG = rg, gh = rh;
        if constexpr (!EARLY && J > 0) round_kw(ga, gb, gc, gd, ge, gf, gG, gh, K[J - 1] + wg[J - 1]);
        // round J: every input but W[J]'s last digit is known here
        const uint32_t t1J = (gh + (K[J] + wJ)) + bsig1(ge) + ch(ge, gf, gG);
        const uint32_t t2J = bsig0(ga) + maj(ga, gb, gc);
#ifdef MH_STOP
#ifdef MH_BATCH
        // ... and round J's two outputs without the digit: A = (t1J + t2J) + inc and
        // E = (gd + t1J) + inc are two adds per nonce where t1 = t1J + inc, A = t1 + t2J, E = gd + t1
        // are three, from two group-level registers instead of three
        const uint32_t aJ = t1J + t2J, eJ = gd + t1J;
#endif
#ifdef MH_HITS
#ifndef MH_BATCH
        const uint32_t aJ = t1J + t2J, eJ = gd + t1J;  // hits_stop: likewise (with MH_BATCH: made above)
#endif
#endif
#endif

        for (uint32_t i = 0; i < 10u; ++i) {
            // ---- per nonce ------------------------------------------------
            const uint32_t inc = i << sh_last;  // SALU
            const uint32_t s0inc = kIncSigma.s0[sh_last >> 3][i], s1inc = kIncSigma.s1[sh_last >> 3][i];
            uint32_t x[64];
            x[J] = wJ + inc;
            // schedule word t, computed right before the round that reads it rather
            // than all words first: the same instructions, but the AMDGPU scheduler
            // then emits an order that issues 1.8% faster on configs[1] and 1.5% on
            // the Pre-mode layouts (profiles/r01zz13_cur_vs_ildef.jsonl)
            auto sched = [&](int t) {
                if (t < 16 || !MH_N(t)) return;
                uint32_t v = pg[t];
                if (MH_N(t - 16)) v += x[t - 16];
                if (MH_N(t - 7)) v += x[t - 7];
                if (MH_N(t - 15)) v += (t - 15 == J) ? (s0wJ ^ s0inc) : ssig0(x[t - 15]);
                if (MH_N(t - 2)) v += (t - 2 == J) ? (s1wJ ^ s1inc) : ssig1(x[t - 2]);
                x[t] = v;
            };
#ifdef MH_STOP
#ifdef MH_BATCH
            uint32_t A = aJ + inc, B = ga, C = gb, D = gc, E = eJ + inc, F = ge, G = gf, H = gG;
#else
#ifdef MH_HITS
            uint32_t A = aJ + inc, B = ga, C = gb, D = gc, E = eJ + inc, F = ge, G = gf, H = gG;
#else
            const uint32_t t1 = t1J + inc;
            uint32_t A = t1 + t2J, B = ga, C = gb, D = gc, E = gd + t1, F = ge, G = gf, H = gG;
#endif
#endif
#else
            const uint32_t t1 = t1J + inc;
            uint32_t A = t1 + t2J, B = ga, C = gb, D = gc, E = gd + t1, F = ge, G = gf, H = gG;
#endif
            uint32_t h0, a63;
            if constexpr (BM != kModeTwo) {
#pragma unroll
                for (int t = J + 1; t < 63; ++t) {
                    sched(t);
#ifdef MH_STOP
#ifdef MH_BATCH
                    round_kw(A, B, C, D, E, F, G, H,
                             (t >= 16 && MH_R(t)) ? kwr[t] : (t >= 16 && MH_G(t)) ? kwg[t]
                                                  : K[t] + (MH_N(t) ? x[t] : wr[t]));
#else
#ifdef MH_HITS
                    round_kw(A, B, C, D, E, F, G, H,
                             (t >= 16 && MH_R(t)) ? kwr[t] : (t >= 16 && MH_G(t)) ? kwg[t]
                                                  : K[t] + (MH_N(t) ? x[t] : wr[t]));
#else
                    round_kw(A, B, C, D, E, F, G, H,
                             (t >= 16 && MH_R(t)) ? kwr[t] : K[t] + (MH_N(t) ? x[t] : (MH_G(t) ? wg[t] : wr[t])));
#endif
#endif
#else
                    round_kw(A, B, C, D, E, F, G, H,
                             (t >= 16 && MH_R(t)) ? kwr[t] : K[t] + (MH_N(t) ? x[t] : (MH_G(t) ? wg[t] : wr[t])));
#endif
                }
                sched(63);
                a63 = A;
                h0 = last_round_h0(A, B, C, E, F, G, H,
                                   (K[63] + st[0]) + (MH_N(63) ? x[63] : (MH_G(63) ? wg[63] : wr[63])));
            } else {
#pragma unroll
                for (int t = 16; t < 64; ++t) sched(t);
#pragma unroll
                for (int t = J + 1; t < 64; ++t)
#ifdef MH_STOP
#ifdef MH_BATCH
                    round_kw(A, B, C, D, E, F, G, H,
                             (t >= 16 && MH_R(t)) ? kwr[t] : (t >= 16 && MH_G(t)) ? kwg[t]
                                                  : K[t] + (MH_N(t) ? x[t] : wr[t]));
#else
#ifdef MH_HITS
                    round_kw(A, B, C, D, E, F, G, H,
                             (t >= 16 && MH_R(t)) ? kwr[t] : (t >= 16 && MH_G(t)) ? kwg[t]
                                                  : K[t] + (MH_N(t) ? x[t] : wr[t]));
#else
                    round_kw(A, B, C, D, E, F, G, H,
                             (t >= 16 && MH_R(t)) ? kwr[t] : K[t] + (MH_N(t) ? x[t] : (MH_G(t) ? wg[t] : wr[t])));
#endif
#endif
#else
                    round_kw(A, B, C, D, E, F, G, H,
                             (t >= 16 && MH_R(t)) ? kwr[t] : K[t] + (MH_N(t) ? x[t] : (MH_G(t) ? wg[t] : wr[t])));
#endif
                const uint32_t s2[8] = {st[0] + A, st[1] + B, st[2] + C, st[3] + D,
                                        st[4] + E, st[5] + F, st[6] + G, st[7] + H};
                sha256_block_kw_last(s2, a.kw1, h0, a63);  // block 1: padding + length only
                a63 += s2[1] - st[1];                       // so that H1 = st[1] + a63 below
            }
#ifdef MH_HASH_KEEP
            h0 = (h0 ^ xor0) & keep0;
#endif
            // New wave best (rare): a uniform branch, so H1 and the
            // lexicographic compare cost nothing on the common path.
#ifdef MH_HITS
            // Hits variant: a lane is a candidate when its H0 <= max(wave best H0, target >> 32),
            // which admits what the product admits and every possible hit (a hit has H0 <= target >> 32)
            // (a scalar load per nonce through a laundered pointer: kept in an SGPR across the
            // loop, the word costs the TwoEarly layout's loop two VALU instructions)
#ifdef MH_BATCH
            // batch_hits: the kernarg segment holds the launch's three table pointers, so the word
            // comes from the item `a` heads (layout.hpp BatchHitsItem: HitsArgs where HitsKernArgs
            // has them): still a scalar load per nonce, at the item's address plus a laundered 32-bit
            // offset (a laundered copy of the 64-bit item pointer is one SGPR pair more than
            // <13, TwoEarly> has: two v_readlane_b32 in its loop)
            using KWord = __attribute__((address_space(4))) const uint32_t;
            uint32_t thi_off = (uint32_t)__builtin_offsetof(HitsKernArgs, h.target) + 4u;
            asm volatile("" : "+s"(thi_off));
            const uint32_t hits_thi = *(KWord*)((__attribute__((address_space(4))) const char*)&a + thi_off);
#else
            using KHits = __attribute__((address_space(4))) const HitsKernArgs;
            KHits* kh = (KHits*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(kh));
            const uint32_t hits_thi = (uint32_t)(kh->h.target >> 32);
#endif
            uint64_t cm = __builtin_amdgcn_ballot_w64(h0 <= (wbh0 > hits_thi ? wbh0 : hits_thi)) & valid_mask;
#else
            uint64_t cm = __builtin_amdgcn_ballot_w64(h0 <= wbh0) & valid_mask;  // MH_FIRST: h0 <= lim
#endif
            if (__builtin_expect(cm != 0ull, 0)) {
#ifdef MH_HASH_KEEP
                const uint32_t h1 = ((st[1] + a63) ^ xor1) & keep1;
#else
                const uint32_t h1 = st[1] + a63;
#endif
                const uint32_t q = g * 10u + i;
#ifdef MH_HITS
                // The hits of this step (valid lanes only: cm holds no other): the lowest hit lane
                // takes one slot per hit from the cursor with one atomic add, the base comes back
                // to every lane through readlane, and the hits go to base + rank in lane order,
                // one uniform {hash, nonce} at a time stored by that lane -- the scalar walk of
                // the candidate loop below, so no lane does 64-bit nonce arithmetic.  The cursor
                // advances for every hit, also past the buffer's end, where nothing is stored.
                {
                    const HitsArgs& ha = hits_args(a);
                    const uint32_t thi = (uint32_t)(ha.target >> 32), tlo = (uint32_t)ha.target;
                    uint64_t hm = __builtin_amdgcn_ballot_w64(h0 < thi || (h0 == thi && h1 <= tlo)) & cm;
                    if (hm) {
                        const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                        const uint32_t lead = (uint32_t)__builtin_ctzll(hm);
                        unsigned long long taken = 0ull;
#ifdef MH_STOP
                        // hits_stop: each hit first counts in its slice (layout.hpp HitsStopArgs), by
                        // the same scalar walk, and the counts are back before the cursor advances:
                        // whoever gets a cursor value back finds every hit it stands for in the slices
                        // (the arguments through a kernarg pointer laundered here, in the rare branch: read
                        // through `a` they are loaded ahead of the loops and held in SGPRs across the
                        // per-nonce loop, which costs the Two layouts' loops three to six v_readlane_b32)
                        using KHits2 = __attribute__((address_space(4))) const HitsStopKernArgs;
#ifdef MH_BATCH
                        KHits2* kq = (KHits2*)&a;  // batch_bound: the item's, as the poll's
#else
                        KHits2* kq = (KHits2*)__builtin_amdgcn_kernarg_segment_ptr();
#endif
                        asm volatile("" : "+s"(kq));
                        const HitsStopArgs& hs = ((const HitsStopKernArgs*)kq)->h;
                        {
                            uint64_t sm = hm;
                            uint32_t back = 0u;
                            do {
                                const uint32_t l = (uint32_t)__builtin_ctzll(sm);
                                sm &= sm - 1ull;
                                uint64_t cn;
                                if constexpr (!EARLY)
                                    cn = (wave_u0 + l) * a.pow10L + q;
                                else
                                    cn = spread(wave_u0 + l, a.hole, a.hole_w) * a.u_mul + spread(g, a.g_hole, 1u) * a.g_mul +
                                         i * a.i_mul;
                                if (lane == lead) back += atomicAdd(first_hits_slice(hs, cn), 1u);
                            } while (sm);
                            asm volatile("" ::"v"(back) : "memory");
                        }
#endif
                        if (lane == lead) taken = atomicAdd(ha.cursor, (unsigned long long)__builtin_popcountll(hm));
                        uint64_t slot =
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(taken >> 32), (int)lead) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)taken, (int)lead);
                        do {
                            const uint32_t l = (uint32_t)__builtin_ctzll(hm);
                            hm &= hm - 1ull;
                            const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)h0, (int)l);
                            const uint32_t c1 = (uint32_t)__builtin_amdgcn_readlane((int)h1, (int)l);
                            uint64_t cn;
                            if constexpr (!EARLY)
                                cn = (wave_u0 + l) * a.pow10L + q;
                            else
                                cn = spread(wave_u0 + l, a.hole, a.hole_w) * a.u_mul + spread(g, a.g_hole, 1u) * a.g_mul +
                                     i * a.i_mul;
                            if (slot < ha.cap && lane == lead) ha.hits[slot] = Hit{((uint64_t)c0 << 32) | c1, cn};
                            ++slot;
                        } while (hm);
#ifdef MH_STOP
                        // the cursor value this wave got back plus its own hits reaches k: publish
                        if (slot >= hs.k) publish_first_hits_bound(hs, lane);
#endif
                    }
                }
#endif
#ifdef MH_FIRST
                // The hits of this step: all take key 0, and the lowest lane holds the smallest
                // nonce of them (at one (g, i) the nonce grows with the lane: spread is monotonic),
                // so that lane alone is compared, on a path of its own (few scalars live beside
                // the loop's).  Without a hit the keys are the hashes and the product's selection
                // below applies.
                uint64_t hm;
                {
                    const uint64_t target = first_args(a).target;
                    const uint32_t thi = (uint32_t)(target >> 32), tlo = (uint32_t)target;
                    hm = __builtin_amdgcn_ballot_w64(h0 < thi || (h0 == thi && h1 <= tlo)) & cm;
                    if (wbh0 == thi && wbh1 == 0u) wbh0 = 0u;  // lim -> k0 (above)
                }
                if (hm) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(hm);
                    uint64_t cn;
                    if constexpr (!EARLY)
                        cn = (wave_u0 + l) * a.pow10L + q;
                    else
                        cn = spread(wave_u0 + l, a.hole, a.hole_w) * a.u_mul + spread(g, a.g_hole, 1u) * a.g_mul +
                             i * a.i_mul;
                    if ((wbh0 | wbh1) != 0u || cn < wbn) {  // the wave's first hit, or a smaller nonce than its hit's
#ifdef MH_STOP
                        // published when found, not only at the chunk's end: one lane lowers the
                        // search's word (the chunk end's vector atomic), only when the wave's best
                        // hit changes.  The empty statement keeps the lane branch's join a block of
                        // its own: folded into the join that merges the wave's best, it made that
                        // best lane-varying (VGPRs, and VALU compares in the per-nonce loop).
                        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
                            atomicMin(first_args(a).first, (unsigned long long)cn);
                        asm volatile("");
#endif
                        wbh0 = 0u;
                        wbh1 = 0u;
                        wbn = cn;
                    }
                } else {
#endif
                // Many candidates (the first nonce of a run makes every lane one): keep only
                // the lanes holding their smallest H0, found by a DPP wave-min, instead of a
                // 64-step scalar scan (~1,000 serial SALU / readlane instructions per run).
                if (__builtin_popcountll(cm) > 4) {
                    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                    const uint32_t mh = wave_min_u32(((cm >> lane) & 1ull) ? h0 : 0xFFFFFFFFu);
                    cm &= __builtin_amdgcn_ballot_w64(h0 == mh);
                }
                uint64_t m = cm;
                do {
                    const uint32_t l = (uint32_t)__builtin_ctzll(m);
                    m &= m - 1ull;
                    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)h0, (int)l);
                    const uint32_t c1 = (uint32_t)__builtin_amdgcn_readlane((int)h1, (int)l);
                    uint64_t cn;
                    if constexpr (!EARLY)
                        cn = (wave_u0 + l) * a.pow10L + q;
                    else
                        cn = spread(wave_u0 + l, a.hole, a.hole_w) * a.u_mul + spread(g, a.g_hole, 1u) * a.g_mul +
                             i * a.i_mul;
                    if (c0 < wbh0 || (c0 == wbh0 && (c1 < wbh1 || (c1 == wbh1 && cn < wbn)))) {
                        wbh0 = c0;
                        wbh1 = c1;
                        wbn = cn;
                    }
                } while (m);
#ifdef MH_FIRST
                }
                {  // k0 -> lim
                    const uint32_t thi = (uint32_t)(first_args(a).target >> 32);
                    wbh0 = wbh0 > thi ? wbh0 : thi;
                }
#endif
            }
        }
    }
#undef MH_N
#undef MH_G
#undef MH_R

#ifdef MH_FIRST
#ifdef MH_STOP
    // scanned: what this wave hashed -- its valid lanes x the groups it ran x 10 -- one atomic per wave
    // (claim_first adds nothing in this build)
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(first_args(a).scanned, (unsigned long long)__builtin_popcountll(valid_mask) * g * 10ull);
#endif
    if (wbh0 == (uint32_t)(first_args(a).target >> 32) && wbh1 == 0u) wbh0 = 0u;  // lim -> k0
#endif
#ifdef MH_HITS
#ifdef MH_STOP
    // scanned: what this wave hashed -- its valid lanes x the groups it ran x 10 -- one atomic per wave
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        atomicAdd(hits_stop_args(a).scanned, (unsigned long long)__builtin_popcountll(valid_mask) * g * 10ull);
#endif
#endif
    uint64_t hash = ((uint64_t)wbh0 << 32) | wbh1;  // wave-uniform: the wave step of block_min
    uint64_t nonce = wbn;                            // is a no-op, the LDS step joins the waves
    block_min(hash, nonce);
    if (threadIdx.x == 0) partials[blk] = Partial{hash, nonce};
#ifdef MH_FIRST
    if (threadIdx.x == 0) {
        const FirstArgs& f = first_args(a);
        // key 0: the chunk's smallest qualifying nonce, for later claims to skip what lies above it
        if (hash == 0ull) atomicMin(f.first, (unsigned long long)nonce);
    }
#endif
}

// The chunk the workgroup runs next: thread 0 takes it from the launch's counter (a vector
// atomic, returning the old value), LDS hands it to the other waves.
__device__ __forceinline__ uint32_t claim_chunk(uint32_t* counter) {
    __shared__ uint32_t s_next;
    if (threadIdx.x == 0) s_next = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t blk = __builtin_amdgcn_readfirstlane(s_next);  // one value per workgroup: scalar
    __syncthreads();  // every wave has read it before thread 0 may overwrite it
    return blk;
}

#ifdef MH_FIRST
// (for both first-hit builds: claim_first of first_scan and, with MH_BATCH, batch_first)
// No nonce of chunk blk is smaller: lane 0's first.  Last-digit layouts: run U's nonces are
// U * 10^L + q.  Early layouts: nonce(U, g, i) = spread(U) * u_mul + (terms >= 0 of g and i), and
// spread is strictly increasing in U, so the chunk's smallest U at g = i = 0 bounds every lane's
// interleaved nonces from below (it is attained, so the bound is exact).
template <int MODE>
__device__ __forceinline__ uint64_t chunk_floor(const FastArgs& a, uint32_t blk) {
    const uint64_t u0 = a.u_start + (uint64_t)blk * kBlockThreads;
    if constexpr (MODE < (int)kModeOneEarly)
        return u0 * a.pow10L;
    else
        return spread(u0, a.hole, a.hole_w) * a.u_mul;
}
#endif

#ifdef MH_BATCH
#ifdef MH_FIRST
// ---------------------------------------------------------------------------
// batch_first<J, MODE>: the fast pieces of many first-hit requests in one launch,
// for mh_search_first_batch_ex(MH_BATCH_FUSE_FAST)
// ---------------------------------------------------------------------------
// batch_fast's static grid and tables (below) around the first-hit chunk body.  Workgroup b runs
// chunk order[b] of the launch -- the host's dispatch order, a permutation of the launch's chunks --
// of the item chunk_item[order[b]] names, read through readfirstlane, so the item's arguments are
// scalar loads (layout.hpp BatchFirstItem: the request's FirstArgs sit where first_scan's kernarg
// segment holds them, so fast_chunk reaches them through first_args unchanged).  Before any hashing
// thread 0 reads the request's `first` word once: a chunk all of whose nonces are larger
// (chunk_floor, attained, so exact) writes the sentinel its slot's merge expects and ends;
// otherwise its valid nonces count as scanned and the chunk runs to its end, where key 0 lowers
// the word.  The word only decreases and always holds a qualifying nonce of the request, so the
// chunk of the smallest one and every chunk holding a smaller nonce run whatever value the read
// returns: a stale read only skips less (claim_first's argument).  No workgroup waits for another,
// no counter and no work queue: the grid always drains.
static_assert(__builtin_offsetof(BatchFirstItem, f) == __builtin_offsetof(FirstKernArgs, f) &&
                  __builtin_offsetof(BatchFirstItem, args) == 0,
              "first_args finds an item's FirstArgs where first_scan's kernarg segment holds them");
#ifdef MH_STOP
// (-DMH_STOP: the same wrapper as batch_stop<J, MODE>, whose chunk body may leave a chunk early; a
// chunk that is run adds nothing to scanned here, its waves count what they hash, fast_chunk.)
template <int J, int MODE>
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void batch_stop(const BatchFirstItem* __restrict__ items,
                                                                          const uint32_t* __restrict__ chunk_item,
                                                                          const uint32_t* __restrict__ order,
                                                                          Partial* __restrict__ partials) {
#else
template <int J, int MODE>
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void batch_first(const BatchFirstItem* __restrict__ items,
                                                                           const uint32_t* __restrict__ chunk_item,
                                                                           const uint32_t* __restrict__ order,
                                                                           Partial* __restrict__ partials) {
#endif
    using KItem = __attribute__((address_space(4))) const BatchFirstItem;
    __shared__ uint32_t s_skip;
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)order[blockIdx.x]);
    const uint32_t ii = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk_item[c]);
    KItem* k = (KItem*)(items + ii);
    asm volatile("" : "+s"(k));
    const uint32_t blk = c - k->chunk0, slot0 = k->slot0;
    if (threadIdx.x == 0) {
        const FastArgs& a = ((const BatchFirstItem*)k)->args;
        const FirstArgs& f = ((const BatchFirstItem*)k)->f;
        const uint64_t seen = __hip_atomic_load(f.first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t skip = 0u;
        if (chunk_floor<MODE>(a, blk) > seen) {
            uint64_t ones = ~0ull;
            asm volatile("" : "+v"(ones));  // made here, as claim_first's
            partials[slot0 + blk] = Partial{ones, ones};
            skip = 1u;
        } else {
#ifndef MH_STOP
            // this chunk will be run: its valid nonces count as scanned
            const uint32_t left = a.n_runs - blk * (uint32_t)kBlockThreads;  // blk < n_chunks: >= 1
            const uint32_t lanes = left < (uint32_t)kBlockThreads ? left : (uint32_t)kBlockThreads;
            atomicAdd(f.scanned, (unsigned long long)lanes * a.n_groups * 10ull);
#endif
        }
        s_skip = skip;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(s_skip)) return;  // one value per workgroup: scalar
    asm volatile("" : "+s"(k));
    fast_chunk<J, MODE>(((const BatchFirstItem*)k)->args, partials + slot0, blk);
}
#else
#ifdef MH_HITS
#ifdef MH_STOP
// ---------------------------------------------------------------------------
// batch_bound<J, MODE>: the fast pieces of many first-k-hits requests in one launch,
// for mh_search_first_hits_batch(MH_BATCH_FUSE_FAST)
// ---------------------------------------------------------------------------
// batch_first's wrapper -- a static grid, workgroup b runs chunk order[b] of the launch, the host's
// dispatch order, of the item chunk_item[order[b]] names -- around hits_stop's chunk body (layout.hpp
// BatchBoundItem: the request's HitsStopArgs sit where hits_stop's kernarg segment holds them, and
// the body reaches them through the item).  Before any hashing thread 0 reads the request's bound
// word once: a chunk all of whose nonces are larger (hits_floor, attained, so exact) writes the
// sentinel and ends; otherwise the chunk runs, its waves count what they hash, poll the word once
// per group of ten nonces and leave the chunk once it lies above the word.  The word, the cursor,
// the region and the slice counters of an item are its request's -- the words the request's generic
// tiles (batch_scan_bound) use -- so a request's bound stops that request's chunks and no other's.
// The word only decreases, and whenever it holds B at least k hits of the request are <= B, so no
// chunk holding one of the request's k smallest hits is skipped or left whatever value a read
// returns: a stale read only skips less (claim_below_bound's argument, per request).  Nothing waits
// on a word, every workgroup that runs reaches block_min and its barriers: the grid always drains.
static_assert(__builtin_offsetof(BatchBoundItem, h) == __builtin_offsetof(HitsStopKernArgs, h) &&
                  __builtin_offsetof(BatchBoundItem, args) == 0,
              "the chunk body finds an item's HitsStopArgs where hits_stop's kernarg segment holds them");
template <int J, int MODE>
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void batch_bound(const BatchBoundItem* __restrict__ items,
                                                                           const uint32_t* __restrict__ chunk_item,
                                                                           const uint32_t* __restrict__ order,
                                                                           Partial* __restrict__ partials) {
    using KItem = __attribute__((address_space(4))) const BatchBoundItem;
    __shared__ uint32_t s_skip;
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)order[blockIdx.x]);
    const uint32_t ii = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk_item[c]);
    KItem* k = (KItem*)(items + ii);
    asm volatile("" : "+s"(k));
    const uint32_t blk = c - k->chunk0, slot0 = k->slot0;
    if (threadIdx.x == 0) {
        const FastArgs& a = ((const BatchBoundItem*)k)->args;
        const HitsStopArgs& h = ((const BatchBoundItem*)k)->h;
        const uint64_t seen = __hip_atomic_load(h.bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t skip = 0u;
        if (hits_floor<MODE>(a, blk) > seen) {
            uint64_t ones = ~0ull;
            asm volatile("" : "+v"(ones));  // made here, as claim_below_bound's
            partials[slot0 + blk] = Partial{ones, ones};
            skip = 1u;
        }
        s_skip = skip;
    }
    __syncthreads();
    if (__builtin_amdgcn_readfirstlane(s_skip)) return;  // one value per workgroup: scalar
    asm volatile("" : "+s"(k));
    fast_chunk<J, MODE>(((const BatchBoundItem*)k)->args, partials + slot0, blk);
}
#else
// ---------------------------------------------------------------------------
// batch_hits<J, MODE>: the fast pieces of many hits requests in one launch, for
// mh_search_hits_batch_ex(MH_BATCH_FUSE_FAST)
// ---------------------------------------------------------------------------
// batch_fast's static grid and tables (below) around the hits chunk body: workgroup b runs chunk
// b - chunk0 of the item chunk_item[b] names, read through readfirstlane, so the item's arguments
// are scalar loads (layout.hpp BatchHitsItem: the request's HitsArgs sit where hits_scan's kernarg
// segment holds them, so fast_chunk reaches them through hits_args unchanged; the per-nonce target
// word comes from the item too, see the chunk body).  No order table, no skipping and no counter:
// the count needs every nonce, so every chunk runs exactly once.  The appends are hits_scan's --
// one vector atomic add on the request's cursor per wave step that holds a hit, vector stores by
// the lead lane, nothing stored at or past the region's end -- into the region the request's
// generic tiles (batch_scan_hits_slots) append to through the same cursor.  No workgroup waits for
// another: the grid always drains.
static_assert(__builtin_offsetof(BatchHitsItem, h) == __builtin_offsetof(HitsKernArgs, h) &&
                  __builtin_offsetof(BatchHitsItem, args) == 0,
              "hits_args finds an item's HitsArgs where hits_scan's kernarg segment holds them");
template <int J, int MODE>
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void batch_hits(const BatchHitsItem* __restrict__ items,
                                                                          const uint32_t* __restrict__ chunk_item,
                                                                          Partial* __restrict__ partials) {
    using KItem = __attribute__((address_space(4))) const BatchHitsItem;
    const uint32_t b = blockIdx.x;
    const uint32_t ii = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk_item[b]);
    KItem* k = (KItem*)(items + ii);
    asm volatile("" : "+s"(k));
    const uint32_t chunk0 = k->chunk0, slot0 = k->slot0;
    asm volatile("" : "+s"(k));
    fast_chunk<J, MODE>(((const BatchHitsItem*)k)->args, partials + slot0, b - chunk0);
}
#endif  // MH_STOP
#else
// ---------------------------------------------------------------------------
// batch_fast<J, MODE>: the fast pieces of many requests in one launch, for
// mh_search_batch_ex(MH_BATCH_FUSE_FAST)
// ---------------------------------------------------------------------------
// Static grid, one workgroup per chunk of the launch: workgroup b reads its item's index from the
// host's per-chunk table through readfirstlane, so the item's FastArgs are scalar loads, and runs
// chunk b - chunk0 of that item into partials[slot0 + b - chunk0] (layout.hpp BatchFastItem; the
// host checks every chunk, item and slot before the launch).  No atomics, no counter and no
// dependency between workgroups: the grid always drains.  The chunk body reads its arguments
// through a constant-address-space pointer laundered before the call, as fast_search's loop does:
// the tables are written by the pass's one copy before the launch and by nothing after it.
template <int J, int MODE>
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void batch_fast(const BatchFastItem* __restrict__ items,
                                                                          const uint32_t* __restrict__ chunk_item,
                                                                          Partial* __restrict__ partials) {
    using KItem = __attribute__((address_space(4))) const BatchFastItem;
    const uint32_t b = blockIdx.x;
    const uint32_t ii = (uint32_t)__builtin_amdgcn_readfirstlane((int)chunk_item[b]);
    KItem* k = (KItem*)(items + ii);
    asm volatile("" : "+s"(k));
    const uint32_t chunk0 = k->chunk0, slot0 = k->slot0;
    asm volatile("" : "+s"(k));
    fast_chunk<J, MODE>(((const BatchFastItem*)k)->args, partials + slot0, b - chunk0);
}
#endif  // MH_HITS
#endif
#else
#ifndef MH_FIRST
#ifdef MH_HITS
#ifdef MH_STOP
// ---------------------------------------------------------------------------
// hits_stop<J, MODE>: the same chunks with the hits append, for mh_search_first_hits
// ---------------------------------------------------------------------------
// claim_chunk with one more word per claim: thread 0 reads the search's bound word beside the
// claim (all ones: fewer than k hits counted so far); a chunk all of whose nonces are larger is
// skipped -- thread 0 writes the sentinel its slot's merge expects and claims again -- so the
// workgroup only ever sees a chunk to run, or the end.  The word only ever decreases, and whenever
// it holds B at least k hits of the range are <= B (layout.hpp HitsStopArgs), so no chunk that
// holds one of the k smallest hits is ever skipped, whatever value a claim happens to see: a stale
// read only skips less.  Static launches (no counter): the workgroup's one chunk is blockIdx.x, and
// skipping it ends the workgroup.  A chunk that is run counts what its waves hash (fast_chunk).
template <int MODE>
__device__ __forceinline__ uint32_t claim_below_bound(Partial* __restrict__ partials) {
    __shared__ uint32_t s_next;
    if (threadIdx.x == 0) {
        uint32_t b;
        for (;;) {
            // the arguments through a pointer laundered per claim, as the chunk body's
            using KArgs = __attribute__((address_space(4))) const HitsStopKernArgs;
            KArgs* k = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(k));
            const FastArgs& a = ((const HitsStopKernArgs*)k)->a;
            const HitsStopArgs& h = ((const HitsStopKernArgs*)k)->h;
            b = a.counter ? atomicAdd(a.counter, 1u) : blockIdx.x;
            if (b >= a.n_chunks) break;
            const uint64_t seen = __hip_atomic_load(h.bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (hits_floor<MODE>(a, b) <= seen) break;  // run it
            uint64_t ones = ~0ull;
            asm volatile("" : "+v"(ones));  // made here, not held across the chunk
            partials[b] = Partial{ones, ones};
            if (!a.counter) {
                b = ~0u;  // past every n_chunks
                break;
            }
        }
        s_next = b;
    }
    __syncthreads();
    const uint32_t blk = __builtin_amdgcn_readfirstlane(s_next);  // one value per workgroup: scalar
    __syncthreads();  // every wave has read it before thread 0 may overwrite it
    return blk;
}

// fast_search's loop over claim_below_bound: every chunk the loop sees is run, and may be left early.
template <int J, int MODE>
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void hits_stop(const FastArgs a,
                                                                         Partial* __restrict__ partials,
                                                                         const HitsStopArgs) {
    using KArgs = __attribute__((address_space(4))) const HitsStopKernArgs;
    KArgs* const kp = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t blk = claim_below_bound<MODE>(partials);
    while (blk < a.n_chunks) {
        KArgs* k = kp;
        asm volatile("" : "+s"(k));
        fast_chunk<J, MODE>(((const HitsStopKernArgs*)k)->a, partials, blk);
        if (!a.counter) break;
        blk = claim_below_bound<MODE>(partials);
    }
}
#endif
#endif
template <int J, int MODE>
#ifdef MH_HITS
// hits_scan<J, MODE>: fast_search with the append of every hit in its chunk body, for
// mh_search_hits.  The launch forms are fast_search's own, and no chunk is ever skipped: the count
// needs every nonce.  HitsArgs is read through the kernarg segment (hits_args above).
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void hits_scan(const FastArgs a,
                                                                         Partial* __restrict__ partials,
                                                                         const HitsArgs) {
#else
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void fast_search(const FastArgs a,
                                                                           Partial* __restrict__ partials) {
#endif
    // Static: workgroup b runs chunk b.  Work queue (a.counter set, grid <= the resident
    // workgroups): each workgroup claims chunks until the counter passes n_chunks; every
    // workgroup leaves once a claim comes back >= n_chunks, so the grid always drains.
    // The chunk body reads its arguments through a pointer the loop launders every iteration,
    // so the compiler cannot keep values derived from them live from one chunk to the next:
    // hoisted out of the loop they spilled ~240 SGPRs into VGPR lanes (85 VGPRs instead of 70).
    using KArgs = __attribute__((address_space(4))) const FastArgs;
    KArgs* const kp = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t blk = a.counter ? claim_chunk(a.counter) : blockIdx.x;
    while (blk < a.n_chunks) {
        KArgs* k = kp;
        asm volatile("" : "+s"(k));
        fast_chunk<J, MODE>(*(const FastArgs*)k, partials, blk);
        if (!a.counter) break;
        blk = claim_chunk(a.counter);
    }
}
#else
// ---------------------------------------------------------------------------
// first_scan<J, MODE>: the same chunks, for mh_search_first
// ---------------------------------------------------------------------------
// claim_chunk with one more word per claim: thread 0 reads *f.first, the smallest qualifying
// nonce any finished chunk of this search has reported (all ones: none), beside the claim; a chunk
// all of whose nonces are larger is skipped -- thread 0 writes the sentinel its slot's merge
// expects and claims again -- so the workgroup only ever sees a chunk to run, or the end.  The word
// only ever decreases and always holds a qualifying nonce of the range, so the chunk of the
// smallest qualifying nonce and every chunk holding a smaller nonce are never skipped, whatever
// value a claim happens to see: a stale read only skips less.  Static launches (no counter): the
// workgroup's one chunk is blockIdx.x, and skipping it ends the workgroup.
template <int MODE>
__device__ __forceinline__ uint32_t claim_first(Partial* __restrict__ partials) {
    __shared__ uint32_t s_next;
    if (threadIdx.x == 0) {
        uint32_t b;
        for (;;) {
            // the arguments through a pointer laundered per claim, as the chunk body's: vector
            // copies of values derived from them, hoisted out of the kernel's loop, cost every
            // layout 4 VGPRs across the chunk
            using KArgs = __attribute__((address_space(4))) const FirstKernArgs;
            KArgs* k = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
            asm volatile("" : "+s"(k));
            const FastArgs& a = ((const FirstKernArgs*)k)->a;
            const FirstArgs& f = ((const FirstKernArgs*)k)->f;
            b = a.counter ? atomicAdd(a.counter, 1u) : blockIdx.x;
            if (b >= a.n_chunks) break;
            const uint64_t seen = __hip_atomic_load(f.first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef MH_STOP
            if (chunk_floor<MODE>(a, b) <= seen) break;  // run it: its waves count what they hash (fast_chunk)
#else
            if (chunk_floor<MODE>(a, b) <= seen) {
                // this chunk will be run: its valid nonces count as scanned
                const uint32_t left = a.n_runs - b * (uint32_t)kBlockThreads;  // b < n_chunks: >= 1
                const uint32_t lanes = left < (uint32_t)kBlockThreads ? left : (uint32_t)kBlockThreads;
                atomicAdd(f.scanned, (unsigned long long)lanes * a.n_groups * 10ull);
                break;
            }
#endif
            uint64_t ones = ~0ull;
            asm volatile("" : "+v"(ones));  // made here: hoisted, the sentinel held 4 VGPRs across the chunk
            partials[b] = Partial{ones, ones};
            if (!a.counter) {
                b = ~0u;  // past every n_chunks
                break;
            }
        }
        s_next = b;
    }
    __syncthreads();
    const uint32_t blk = __builtin_amdgcn_readfirstlane(s_next);  // one value per workgroup: scalar
    __syncthreads();  // every wave has read it before thread 0 may overwrite it
    return blk;
}

// fast_search's loop over claim_first: every chunk the loop sees is run.
// (-DMH_STOP: the same loop as stop_scan<J, MODE>, whose chunk body may leave a chunk early.)
template <int J, int MODE>
#ifdef MH_STOP
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void stop_scan(const FastArgs a,
                                                                         Partial* __restrict__ partials,
                                                                         const FirstArgs) {
#else
__global__ __launch_bounds__(kBlockThreads, min_waves(J, MODE)) void first_scan(const FastArgs a,
                                                                          Partial* __restrict__ partials,
                                                                          const FirstArgs) {
#endif
    using KArgs = __attribute__((address_space(4))) const FirstKernArgs;
    KArgs* const kp = (KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t blk = claim_first<MODE>(partials);
    while (blk < a.n_chunks) {
        KArgs* k = kp;
        asm volatile("" : "+s"(k));
        fast_chunk<J, MODE>(((const FirstKernArgs*)k)->a, partials, blk);
        if (!a.counter) break;
        blk = claim_first<MODE>(partials);
    }
}
#endif
#endif  // MH_BATCH

// Marker of a code object whose fast_search kernels run the work-queue loop above over this
// FastArgs layout: its size is sizeof(FastArgs).  The library uses the work queue with a code
// object only if it carries the marker at that size (search_kernels.hip, fast_function) -- the
// embedded object always does; one loaded by the dev build's MINEHIP_DEV_CODE_OBJECT hook from
// older sources runs one workgroup per chunk instead of searching only its first chunks.
extern "C" {
#ifdef MH_BATCH
#ifdef MH_FIRST
// Marker of the first-hit batch code object instead: its kernels read BatchFirstItems of this size
// (the library launches batch_first only from a code object that carries it, search_kernels.hip).
#ifdef MH_STOP
// (of the stopping first-hit batch code object: batch_stop is launched only from one that carries this)
__device__ __attribute__((used)) uint8_t mh_fast_batch_stop_items[sizeof(BatchFirstItem)];
#else
__device__ __attribute__((used)) uint8_t mh_fast_batch_first_items[sizeof(BatchFirstItem)];
#endif
#else
#ifdef MH_HITS
#ifdef MH_STOP
// Marker of the first-k-hits batch code object instead: its kernels read BatchBoundItems of this size
// (the library launches batch_bound only from a code object that carries it, search_kernels.hip).
__device__ __attribute__((used)) uint8_t mh_fast_batch_bound_items[sizeof(BatchBoundItem)];
#else
// Marker of the hits batch code object instead: its kernels read BatchHitsItems of this size (the
// library launches batch_hits only from a code object that carries it, search_kernels.hip).
__device__ __attribute__((used)) uint8_t mh_fast_batch_hits_items[sizeof(BatchHitsItem)];
#endif
#else
// Marker of the batch code object instead: its kernels read BatchFastItems of this size (the
// library launches batch_fast only from a code object that carries it, search_kernels.hip).
__device__ __attribute__((used)) uint8_t mh_fast_batch_items[sizeof(BatchFastItem)];
#endif  // MH_HITS
#endif
#else
__device__ __attribute__((used)) uint8_t mh_fast_queue_args[sizeof(FastArgs)];
#endif
#ifdef MH_HASH_KEEP
// Marker of the coarse-hash variant: its kernels mask (H0, H1) by FastArgs::pad_.  The dev build
// runs a search with MINEHIP_DEV_HASH_KEEP set only on a code object that carries it, so masked
// generic pieces never meet unmasked fast pieces (search_kernels.hip, fast_keep_ok).
__device__ __attribute__((used)) uint8_t mh_fast_hash_keep[sizeof(FastArgs)];
#endif
}

// The instantiations the planner uses (plan.cpp; launch by mangled name in
// search_kernels.hip): kModeOne for every word J of the last digit in a
// one-block tail, kModePre for J <= 4 of block 1 (last digit at tail byte
// 64..82), kModeTwo for J = 13..15 of block 0; the Early modes where a nonce
// costs less with the digit ending word J innermost than with the last digit
// in word J + 1 (plan.cpp: nonce_cost(J) < nonce_cost(J + 1)).
#ifdef MH_BATCH
#ifdef MH_FIRST
#ifdef MH_STOP
#define MH_INST(j, m) \
    template __global__ void batch_stop<j, m>(const BatchFirstItem* __restrict__, const uint32_t* __restrict__, \
                                              const uint32_t* __restrict__, Partial* __restrict__);
#else
#define MH_INST(j, m) \
    template __global__ void batch_first<j, m>(const BatchFirstItem* __restrict__, const uint32_t* __restrict__, \
                                               const uint32_t* __restrict__, Partial* __restrict__);
#endif
#else
#ifdef MH_HITS
#ifdef MH_STOP
#define MH_INST(j, m) \
    template __global__ void batch_bound<j, m>(const BatchBoundItem* __restrict__, const uint32_t* __restrict__, \
                                               const uint32_t* __restrict__, Partial* __restrict__);
#else
#define MH_INST(j, m) \
    template __global__ void batch_hits<j, m>(const BatchHitsItem* __restrict__, const uint32_t* __restrict__, \
                                              Partial* __restrict__);
#endif
#else
#define MH_INST(j, m) \
    template __global__ void batch_fast<j, m>(const BatchFastItem* __restrict__, const uint32_t* __restrict__, \
                                              Partial* __restrict__);
#endif  // MH_HITS
#endif
#else
#ifndef MH_FIRST
#ifdef MH_HITS
#ifdef MH_STOP
#define MH_INST(j, m) \
    template __global__ void hits_stop<j, m>(const FastArgs, Partial* __restrict__, const HitsStopArgs);
#else
#define MH_INST(j, m) \
    template __global__ void hits_scan<j, m>(const FastArgs, Partial* __restrict__, const HitsArgs);
#endif
#else
#define MH_INST(j, m) template __global__ void fast_search<j, m>(const FastArgs, Partial* __restrict__);
#endif
#else
#ifdef MH_STOP
#define MH_INST(j, m) \
    template __global__ void stop_scan<j, m>(const FastArgs, Partial* __restrict__, const FirstArgs);
#else
#define MH_INST(j, m) \
    template __global__ void first_scan<j, m>(const FastArgs, Partial* __restrict__, const FirstArgs);
#endif
#endif
#endif  // MH_BATCH
MH_FAST_KERNELS(MH_INST)  // layout.hpp: the one list of instantiated layouts
#undef MH_INST

}  // namespace mh
