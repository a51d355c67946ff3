// first_batch_stop_host.cpp -- the `scanned` arithmetic of batch_stop<J, MODE> on the host, built with
// -fsanitize=address,undefined by tests/test_first_batch_stop_host.py (a stand-alone program: no GPU,
// no library).
//
// batch_first adds a chunk's valid nonces to its request's `scanned` up front; batch_stop adds
// nothing there: under MH_STOP each wave adds, at the chunk's end,
//     popcount(valid lanes of the wave) x groups it ran x 10
// (fast_search.hip, fast_chunk), and a skipped chunk adds nothing.  This program replays that sum with
// the kernel's types over the chunks and waves of pieces whose last chunk is partial:
//   * no stop: the sum is the piece's nonce count, n_runs x n_groups x 10, and equals what
//     batch_first's up-front adds give;
//   * a hit in chunk c at group gh: chunks 0..c run to their end (their floor is <= the hit), every
//     wave of a chunk above c leaves at some group 0..n_groups or the chunk is skipped unbegun: the sum
//     is at least the nonces of chunks 0..c (so at least hit - first + 1 for any hit of chunk c) and
//     at most the piece's count, for every choice of leaving groups (the extremes and a seeded sample).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../bitcoin-miner_amd/csrc/layout.hpp"

namespace {
int failures = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            ++failures;                                                \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
        }                                                              \
    } while (0)

constexpr uint32_t kWave = 64;

// valid_mask of wave `wave` of chunk `blk`, as fast_chunk's ballot of gid < n_runs
uint64_t valid_mask(uint32_t n_runs, uint32_t blk, uint32_t wave) {
    uint64_t m = 0;
    for (uint32_t l = 0; l < kWave; ++l) {
        const uint32_t gid = blk * (uint32_t)mh::kBlockThreads + wave * kWave + l;
        if (gid < n_runs) m |= 1ull << l;
    }
    return m;
}

// what one wave adds at its chunk's end after g groups (the kernel's expression)
unsigned long long wave_add(uint64_t mask, uint32_t g) {
    return (unsigned long long)__builtin_popcountll(mask) * g * 10ull;
}

// batch_first's up-front add for a chunk that is run
unsigned long long chunk_add_up_front(uint32_t n_runs, uint32_t n_groups, uint32_t blk) {
    const uint32_t left = n_runs - blk * (uint32_t)mh::kBlockThreads;
    const uint32_t lanes = left < (uint32_t)mh::kBlockThreads ? left : (uint32_t)mh::kBlockThreads;
    return (unsigned long long)lanes * n_groups * 10ull;
}

struct Totals {
    uint64_t pieces = 0, chunks = 0, waves = 0, partial_waves = 0, empty_waves = 0, stops = 0;
};

void run(uint32_t n_runs, uint32_t n_groups, std::mt19937_64& rng, Totals* t) {
    const uint32_t waves = (uint32_t)mh::kBlockThreads / kWave;
    const uint32_t n_chunks = (n_runs + (uint32_t)mh::kBlockThreads - 1) / (uint32_t)mh::kBlockThreads;
    const unsigned long long count = (unsigned long long)n_runs * n_groups * 10ull;
    ++t->pieces;
    // no stop: every wave runs n_groups groups
    unsigned long long sum = 0, up_front = 0;
    std::vector<unsigned long long> chunk_nonces(n_chunks);
    for (uint32_t blk = 0; blk < n_chunks; ++blk) {
        unsigned long long c = 0;
        for (uint32_t w = 0; w < waves; ++w) {
            const uint64_t m = valid_mask(n_runs, blk, w);
            c += wave_add(m, n_groups);
            ++t->waves;
            if (m == 0) ++t->empty_waves;
            else if (m != ~0ull) ++t->partial_waves;
        }
        CHECK(c == chunk_add_up_front(n_runs, n_groups, blk));
        chunk_nonces[blk] = c;
        sum += c;
        up_front += chunk_add_up_front(n_runs, n_groups, blk);
        ++t->chunks;
    }
    CHECK(sum == count && up_front == count);
    // a hit in chunk c at group gh: chunks above c leave early or are skipped
    for (uint32_t c = 0; c < n_chunks; ++c) {
        unsigned long long below = 0;   // the nonces of chunks 0..c: all hashed
        for (uint32_t blk = 0; blk <= c; ++blk) below += chunk_nonces[blk];
        for (int variant = 0; variant < 6; ++variant) {
            unsigned long long s = below;
            for (uint32_t blk = c + 1; blk < n_chunks; ++blk) {
                const bool skipped = variant == 0 || (variant >= 3 && (rng() & 3u) == 0);   // unbegun: adds nothing
                if (skipped) continue;
                for (uint32_t w = 0; w < waves; ++w) {
                    const uint32_t g = variant == 1 ? 0u                                   // left at the first poll
                                       : variant == 2 ? n_groups                           // never saw the hit
                                                      : (uint32_t)(rng() % (n_groups + 1u));
                    s += wave_add(valid_mask(n_runs, blk, w), g);
                }
            }
            ++t->stops;
            CHECK(s >= below && s <= count);
            if (variant == 0 || variant == 1) CHECK(s == below);
            if (variant == 2) CHECK(s == count);
            // any hit of chunk c, at any group gh and digit i, lies among the nonces counted in `below`:
            // in nonce order the piece's first `rank` nonces are those of runs 0 .. run, so
            // hit - first + 1 <= (run + 1) x n_groups x 10 <= below
            const uint32_t last_run = std::min(n_runs, (c + 1u) * (uint32_t)mh::kBlockThreads) - 1u;
            CHECK((unsigned long long)(last_run + 1u) * n_groups * 10ull == below);
        }
    }
}
}  // namespace

int main() {
    static_assert(mh::kBlockThreads == 256, "four waves of 64 lanes per chunk");
    std::mt19937_64 rng(440);
    Totals t;
    for (uint32_t n_runs : {1u, 63u, 64u, 65u, 255u, 256u, 257u, 2000u})
        for (uint32_t n_groups : {1u, 10u, 100u}) run(n_runs, n_groups, rng, &t);
    // the largest piece a pass may hold stays far inside 64 bits: 2^32 - 1 runs x 10^9 groups x 10
    CHECK(wave_add(~0ull, 1000000000u) == 640000000000ull);
    printf("pieces=%llu chunks=%llu waves=%llu partial_waves=%llu empty_waves=%llu stops=%llu failures=%d\n",
           (unsigned long long)t.pieces, (unsigned long long)t.chunks, (unsigned long long)t.waves,
           (unsigned long long)t.partial_waves, (unsigned long long)t.empty_waves, (unsigned long long)t.stops, failures);
    return failures ? 1 : 0;
}
