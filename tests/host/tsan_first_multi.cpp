// tsan_first_multi.cpp -- mh_search_first_multi's coordinator (search_first_chunks in
// bitcoin-miner_amd/csrc/multi.cpp: worker threads over a target job of the scheduler) driven with a
// stand-in search from up to 8 worker threads, built with -fsanitize=thread and with
// -fsanitize=address,undefined by tests/test_first_multi_sanitize.py.  The GPU search is replaced by
// a loop over a synthetic hash: a chunk answers with its first nonce whose hash is <= target, else
// with its minimum, sleeps a little, and some workers fail (any of them, possibly all), or only k of
// the host threads start.  Invariants, for random ranges, chunk sizes and targets (none, few or many
// hits):
//   * success <=> at least one worker survived (and started);
//   * the answer is the brute-force one: the smallest qualifying nonce of the range and its hash, or
//     the lexicographic minimum when nothing qualifies;
//   * every chunk searched lies in the range, no chunk that succeeded was searched twice, and every
//     nonce up to the answer (the whole range when nothing qualifies) was searched;
//   * scanned is the sum over the chunks that succeeded.
//
//   tsan_first_multi <seed> <iterations>     exit 0 = every invariant held
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>
#include <random>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "../../bitcoin-miner_amd/csrc/multi.hpp"
#include "../../include/minehip.h"

namespace mh {
int set_error(int code, const char*) { return code; }  // the scheduler's error slot (minehip.cpp's is per thread)
}  // namespace mh

static int g_fail = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                             \
            return;                                                               \
        }                                                                         \
    } while (0)

static uint64_t splitmix(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// the first nonce of [lo, hi] with hash <= target, else the lexicographic minimum
static void answer(uint64_t salt, uint64_t lo, uint64_t hi, uint64_t target, uint64_t* h, uint64_t* n) {
    uint64_t bh = ~0ull, bn = ~0ull;
    for (uint64_t x = lo;; ++x) {
        const uint64_t v = splitmix(x ^ salt);
        if (v <= target) {
            *h = v;
            *n = x;
            return;
        }
        if (v < bh) {
            bh = v;
            bn = x;
        }
        if (x == hi) break;
    }
    *h = bh;
    *n = bn;
}

struct Rec {
    uint64_t lo, hi, scanned;
};

static mh::ThreadStart limited(int k) {
    auto n = std::make_shared<std::atomic<int>>(0);
    return [n, k](std::function<void()> fn) {
        if ((*n)++ >= k) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again));
        return std::thread(std::move(fn));
    };
}

static void one_case(std::mt19937_64& rng) {
    const int ndev = 1 + (int)(rng() % 8);
    std::vector<bool> fails((size_t)ndev, false);
    const int mode = (int)(rng() % 4);  // 0: none fail, 1: one, 2: random set, 3: all
    for (int i = 0; i < ndev; ++i)
        fails[(size_t)i] = mode == 3 || (mode == 1 && i == (int)(rng() % ndev)) || (mode == 2 && rng() % 3 == 0);
    const int started = (rng() % 4 == 0) ? (int)(rng() % (ndev + 1)) : ndev;  // host threads that start
    const uint64_t size = 1 + rng() % 60000;
    const uint64_t lower = (rng() % 3 == 0) ? ~0ull - (size - 1) : rng() % (1ull << 40);
    const uint64_t upper = lower + (size - 1);
    const uint64_t chunk = 1 + rng() % (size / 2 + 1);
    const uint64_t salt = rng();
    uint64_t target;
    switch (rng() % 4) {
        case 0: target = 0; break;                       // nothing qualifies
        case 1: target = ~0ull / size * 2; break;        // about two hits
        case 2: target = ~0ull / 50; break;              // a hit in most chunks
        default: target = ~0ull; break;                  // every nonce
    }
    std::mutex mu;
    std::vector<Rec> done;
    const mh::FirstChunkSearch search = [&](int worker, uint64_t lo, uint64_t hi, uint64_t* h, uint64_t* n,
                                            uint64_t* scanned, std::string* err) -> int {
        std::this_thread::sleep_for(std::chrono::microseconds(splitmix(lo ^ (uint64_t)worker) % 200));
        if (fails[(size_t)worker]) {
            *err = "stand-in failure of worker " + std::to_string(worker);
            return MH_EHIP;
        }
        answer(salt, lo, hi, target, h, n);
        *scanned = (*h <= target) ? *n - lo + 1 : hi - lo + 1;
        std::lock_guard<std::mutex> lk(mu);
        done.push_back(Rec{lo, hi, *scanned});
        return MH_OK;
    };
    uint64_t oh = 0, on = 0, scanned = 0;
    std::string err;
    const int rc = mh::search_first_chunks(ndev, (const uint8_t*)"cmu440", 6, lower, upper, target, chunk, search, &oh,
                                           &on, &scanned, &err, started < ndev ? limited(started) : mh::ThreadStart());
    bool survivor = false;
    for (int i = 0; i < std::min(started, ndev); ++i) survivor = survivor || !fails[(size_t)i];
    if (!survivor) {
        CHECK(rc == MH_EHIP || rc == MH_EINTERNAL);
        CHECK(!err.empty());
        return;
    }
    CHECK(rc == MH_OK);
    uint64_t wh = 0, wn = 0;
    answer(salt, lower, upper, target, &wh, &wn);
    CHECK(oh == wh && on == wn);
    std::sort(done.begin(), done.end(), [](const Rec& a, const Rec& b) { return a.lo < b.lo; });
    CHECK(!done.empty() && done.front().lo == lower);
    uint64_t sum = 0;
    unsigned __int128 covered = lower;  // [lower, covered) is tiled by the chunks that succeeded
    for (size_t k = 0; k < done.size(); ++k) {
        CHECK(done[k].lo >= lower && done[k].hi <= upper && done[k].lo <= done[k].hi);
        if (k) CHECK(done[k - 1].hi < done[k].lo);  // disjoint: no chunk that succeeded ran twice
        if (done[k].lo == covered) covered = (unsigned __int128)done[k].hi + 1u;
        sum += done[k].scanned;
    }
    const uint64_t need = wh <= target ? wn : upper;  // everything up to the answer was searched
    CHECK(covered > need);
    CHECK(scanned == sum);
    CHECK(wh <= target ? (scanned >= wn - lower + 1 && scanned <= size) : scanned == size);
}

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 440;
    const int iters = argc > 2 ? atoi(argv[2]) : 100;
    std::mt19937_64 rng(seed);
    for (int it = 0; it < iters; ++it) one_case(rng);
    printf("iterations=%d failures=%d\n", iters, g_fail);
    return g_fail ? 1 : 0;
}
